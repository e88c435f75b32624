r"""Closed-form inputs of every parity case.  Shared by ``tests/golden/make_golden.py`` (which
feeds them to the REFERENCE in the build container) and by the tests (which feed them to the
oracle and to the HIP path), so that only outputs need to be stored as golden vectors.

Case ``ref3``/``ref512`` reproduce the inputs of the reference's own tests
(``tests/test_slowsims.py:33-62``, ``tests/test_sims.py:36-61``); the others cover what the
reference's tests do not.
"""
from math import pi as π
import os
import sys

import torch
from torch import tensor

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

γH_val, dt0_val = 4257.6, 4e-6


def ref_pulse(nT: int, dtype, *, gr_y: float = 0.0):
    r"""Pulse of test_slowsims.py:54-61 / test_sims.py:55-61: rf = 10[cos,sin](2πt/nT) G with
    a trailing coil dim, gr = [1, gr_y, 10·atan(t - nT/2)/π] G/cm."""
    t = torch.arange(0, nT, dtype=dtype).reshape(1, 1, nT)
    rf = 10 * torch.cat([torch.cos(t / nT * 2 * π), torch.sin(t / nT * 2 * π)], 1)[..., None]
    gr = torch.cat([torch.ones((1, 1, nT), dtype=dtype), torch.full((1, 1, nT), gr_y, dtype=dtype),
                    10 * torch.atan(t - round(nT / 2)) / π], 1)
    return rf, gr


def ref_case(nM: int, dtype, *, nT: int = 512, seed: int = None):
    r"""The reference tests' spin line: loc_x = loc_y = linspace(-1,1,nM), loc_z = 1,
    Δf = -loc_x·γ (cancels gr_x = 1 G/cm), b1Map = [1, 0], T1 = 1 s, T2 = 40 ms.
    ``seed=None``: M0 = eye(3) (needs nM = 3, test_slowsims.py:35); else uniform [0,1)
    (test_sims.py:36, which is unseeded there)."""
    γ, dt = tensor(γH_val, dtype=dtype), tensor(dt0_val, dtype=dtype)
    if seed is None:
        assert nM == 3
        M0 = torch.eye(3, dtype=dtype)[None]
    else:
        gen = torch.Generator(device='cpu').manual_seed(seed)
        M0 = torch.rand((1, nM, 3), generator=gen, dtype=torch.float64).to(dtype)
    lx = torch.linspace(-1., 1., steps=nM, dtype=dtype).reshape(1, nM)
    loc = torch.stack([lx, lx.clone(), torch.ones((1, nM), dtype=dtype)], 2)
    rf, gr = ref_pulse(nT, dtype)
    return dict(M0=M0, loc=loc, Δf=-lx * γ, b1Map=tensor([1., 0.], dtype=dtype).reshape(1, 1, 2, 1),
                rf=rf, gr=gr, T1=tensor([[1.]], dtype=dtype), T2=tensor([[4e-2]], dtype=dtype),
                γ=γ, dt=dt)


def rfgr_variants(dtype, seed: int = 7):
    r"""F3: small rfgr2beff inputs covering every branch: N = 2, nM = 7, nT = 12, nC = 4."""
    gen = torch.Generator(device='cpu').manual_seed(seed)
    rnd = lambda *s: (torch.rand(s, generator=gen, dtype=torch.float64) * 2 - 1).to(dtype)  # noqa
    N, nM, nT, nC = 2, 7, 12, 4
    base = dict(gr=rnd(N, 3, nT), loc=rnd(N, nM, 3) * 5)
    γs = tensor(γH_val, dtype=dtype)
    γm = (γH_val * (1 + 0.1 * rnd(N, nM))).to(dtype)
    return {
        'plain':        dict(base, rf=rnd(N, 2, nT)),
        'df_scalar_γ':  dict(base, rf=rnd(N, 2, nT), Δf=rnd(N, nM) * 100, γ=γs),
        'df_map_γ':     dict(base, rf=rnd(N, 2, nT), Δf=rnd(N, nM) * 100, γ=γm),
        'coil1_dim':    dict(base, rf=rnd(N, 2, nT, 1), b1Map=rnd(N, nM, 2, 1)),
        'coil1_nodim':  dict(base, rf=rnd(N, 2, nT), b1Map=rnd(N, nM, 2)),
        'ptx4':         dict(base, rf=rnd(N, 2, nT, nC), b1Map=rnd(N, nM, 2, nC),
                             Δf=rnd(N, nM) * 100, γ=γm),
        'ptx4_nomap':   dict(base, rf=rnd(N, 2, nT, nC)),
        'batch1_pulse': dict(gr=rnd(1, 3, nT), loc=rnd(N, nM, 3) * 5, rf=rnd(1, 2, nT),
                             Δf=rnd(1, nM) * 100, γ=γs),
        'odd_nT':       dict(gr=rnd(N, 3, 13), loc=rnd(N, nM, 3) * 5, rf=rnd(N, 2, 13, 2),
                             b1Map=rnd(N, nM, 2, 2)),
    }


def bcast_variants(dtype, seed: int = 11):
    r"""F5: the broadcast zoo of sims.blochsim: N = 2, nM = 5, nT = 40; T1/T2/γ as 0-dim,
    (1,1), (N,1), (1,nM), (N,nM); dt as (), (1,), (N,)."""
    gen = torch.Generator(device='cpu').manual_seed(seed)
    rnd = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64)  # noqa: E731
    N, nM, nT = 2, 5, 40
    M0 = rnd(N, nM, 3).to(dtype)
    Beff = ((rnd(N, nM, nT, 3) * 2 - 1) * 8).to(dtype)
    Beff[0, 1] = 0                    # a spin that never rotates (phi = 0 every step)
    Beff[1, 2, 5:9] = 0               # zero-field steps in the middle of a pulse
    t1 = lambda *s: (0.5 + rnd(*s)).to(dtype)         # noqa: E731
    t2 = lambda *s: (0.02 + 0.1 * rnd(*s)).to(dtype)  # noqa: E731
    gm = lambda *s: (γH_val * (0.9 + 0.2 * rnd(*s))).to(dtype)  # noqa: E731
    dt = tensor(dt0_val, dtype=dtype)
    v = {
        'scalar':   dict(T1=t1().reshape(()), T2=t2().reshape(()), γ=gm().reshape(()), dt=dt),
        'one_one':  dict(T1=t1(1, 1), T2=t2(1, 1), γ=gm(1, 1), dt=dt.reshape(1)),
        'per_spin': dict(T1=t1(N, nM), T2=t2(N, nM), γ=gm(N, nM), dt=dt.reshape(1)),
        'mixed':    dict(T1=t1(N, 1), T2=t2(N, 1), γ=gm(1, nM), dt=dt.reshape(1)),  # T1,T2 must share a shape (sims.py:76 cat)
        'dt_batch': dict(T1=t1(N, nM), T2=t2(N, nM), γ=gm(1, 1),
                         dt=(dt0_val * (1 + rnd(N))).to(dtype)),
        'norelax':  dict(T1=None, T2=None, γ=gm(N, nM), dt=dt.reshape(1)),
        'expanded': dict(T1=t1(N, 1).expand(N, nM), T2=t2(1, 1).expand(N, nM),
                         γ=gm(1, 1).expand(N, nM), dt=dt.reshape(1)),   # stride-0 views (mobjs)
    }
    return M0, Beff, v


def onestep_case(dtype, seed: int = 13):
    r"""F4: blochsim_1step in/out, including the all-zero-field branch."""
    gen = torch.Generator(device='cpu').manual_seed(seed)
    rnd = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64)  # noqa: E731
    N, nM = 2, 9
    M = rnd(N, nM, 3).to(dtype)
    b = ((rnd(N, nM, 3) * 2 - 1) * 10).to(dtype)
    b[0, 3] = 0
    dt = tensor(dt0_val, dtype=dtype)
    T1, T2 = (0.5 + rnd(N, nM)).to(dtype), (0.02 + 0.1 * rnd(N, nM)).to(dtype)
    E1, E2 = torch.exp(-dt / T1), torch.exp(-dt / T2)
    g = 2 * π * tensor(γH_val, dtype=dtype) * dt
    return dict(M=M, b=b, E1=E1, E1_1=E1 - 1, E2=E2, γ2πdt=g)


def big_subset(cfg: int, dtype=torch.float32, count: int = 4096, *, coarse: bool = False):
    r"""F7: a seeded ``count``-spin subset of a BASELINE.json config's synthetic cube
    (spins are independent, so the subset's results equal the full run's rows)."""
    import mrphy_amd
    from mrphy_amd import synth
    c = synth.CONFIGS[cfg]
    idx = synth.subset_indices(c['n'], count, seed=1000 + cfg)
    spins = synth.cube_spins(c['n'], idx, dtype=dtype, seed_M0=2000 + cfg)
    if cfg == 4 and coarse:
        pulse = synth.pulse(c['nT'] // 2, dtype=dtype, dt=8e-6)
    else:
        pulse = synth.pulse(c['nT'], dtype=dtype)
    return idx, spins, pulse


def reference_constants(T1, T2, γ, dt, ndim: int):
    r"""γ2πdt, E1, E1-1, E2 formed exactly as the reference forms them (sims.py:62,74-76 after the
    right-padding of sims.py:309-313), on THIS machine's CPU.  ``make_golden.py`` stores them
    next to the reference's outputs: they are per-spin constants applied nT times, and exp() is
    not bit-reproducible across CPUs/GPUs, so a golden comparison must use the very constants
    the reference run used."""
    pad = lambda x: None if x is None else x.reshape(tuple(x.shape) + (ndim - x.ndim) * (1,))  # noqa
    γ, dt, T1, T2 = pad(γ), pad(dt), pad(T1), pad(T2)
    out = {'γ2πdt': 2 * π * γ * dt}
    if T1 is not None:
        E1, E2 = torch.exp(-dt / T1), torch.exp(-dt / T2)
        out.update(E1=E1, E1_1=E1 - 1, E2=E2)
    return out


def freeprec_variants(dtype, seed: int = 17):
    r"""free-precession cases: the reference's known answer (test_slowsims.py:100-121) and a small
    zoo of broadcast forms (N = 2, nM = 6)."""
    gen = torch.Generator(device='cpu').manual_seed(seed)
    rnd = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64)  # noqa: E731
    half = tensor([[0.5]], dtype=dtype)
    dur = tensor(0.5, dtype=dtype)
    Tk = -dur / torch.log(half)                                    # E1 = E2 = 0.5
    known = dict(M=torch.eye(3, dtype=dtype)[None], dur=dur, T1=Tk.reshape(()), T2=Tk.reshape(()),
                 Δf=tensor([[1 / 4 / 0.5, -1 / 4 / 0.5, 1]], dtype=dtype))
    N, nM = 2, 6
    M = rnd(N, nM, 3).to(dtype)
    t1, t2 = (0.5 + rnd(N, nM)).to(dtype), (0.02 + 0.1 * rnd(N, nM)).to(dtype)
    df = ((rnd(N, nM) * 2 - 1) * 300).to(dtype)
    return {
        'known':     known,
        'full':      dict(M=M, dur=tensor(3e-3, dtype=dtype), T1=t1, T2=t2, Δf=df),
        'dur_batch': dict(M=M, dur=tensor([1e-3, 4e-3], dtype=dtype), T1=t1, T2=t2, Δf=df),
        'scalars':   dict(M=M, dur=tensor([2e-3], dtype=dtype), T1=tensor(1.2, dtype=dtype),
                          T2=tensor(0.05, dtype=dtype), Δf=df[:1]),
        'norelax':   dict(M=M, dur=tensor(3e-3, dtype=dtype), T1=None, T2=None, Δf=df),
        'noprec':    dict(M=M, dur=tensor(3e-3, dtype=dtype), T1=t1, T2=t2, Δf=None),
    }


def mask_case(dtype, Nd=(5, 6, 7), N: int = 2):
    r"""a closed-form mask on an ``Nd`` grid (about 3/4 of the voxels), spatial
    tensors of the shapes mobjs moves through extract/embed (M: xyz, a map: scalar, b1Map:
    (xy, nCoils)), and FOV/offset per batch entry."""
    ix, iy, iz = torch.meshgrid(*[torch.arange(n) for n in Nd], indexing='ij')
    mask = (((ix * 7 + iy * 3 + iz * 5) % 4) != 0)[None]
    nV = Nd[0] * Nd[1] * Nd[2]
    nM = int(mask.sum())
    f64 = torch.float64

    def wave(shape, a):
        # exactly representable values (multiples of 1/64 in [-8, 8)): identical bits on any host
        n = 1
        for d in shape:
            n *= d
        k = torch.arange(n, dtype=torch.int64)
        return (((k * a + 11) % 1021 - 510).to(f64) / 64).reshape(shape).to(dtype)
    spatial = {'M': wave((N,) + Nd + (3,), 37), 'map': wave((N,) + Nd, 61),
               'b1': wave((N,) + Nd + (2, 4), 13)}
    compact = {'M': wave((N, nM, 3), 41), 'map': wave((N, nM), 29),
               'b1': wave((N, nM, 2, 4), 17)}
    fov = torch.tensor([[24., 20., 7.5], [3., 30., 12.]], dtype=f64)[:N].to(dtype)
    ofst = torch.tensor([[0., 0.5, -1.25], [2., 0., 0.125]], dtype=f64)[:N].to(dtype)
    return dict(shape=(N,) + Nd, Nd=Nd, N=N, nV=nV, nM=nM, mask=mask, spatial=spatial,
                compact=compact, fov=fov, ofst=ofst)


# ---------------------------------------------------------------------------------------------
# The fused route's operand zoo and the zero-field case (tests/test_fused_operands.py; goldens:
# make_golden.py gen_fusedops)
# ---------------------------------------------------------------------------------------------
FUSED_N, FUSED_ND = 2, (5, 4, 7)
FUSED_NM = 140                        # two full waves plus a ragged 12
FUSED_COILS = (0, 1, 4)               # 0: one coil, no b1Map; 1: one coil with a map; 4: parallel transmit
FUSED_NT53 = ('compact_mixed', 'cube_planes', 'views')       # repeated at nT = 53: fused part + 5 composed steps


def _after(x, n: int = 1):
    r"""The same contiguous values starting ``n`` elements into a larger buffer."""
    buf = torch.zeros(x.numel() + n + 3, dtype=x.dtype)
    y = buf[n:n + x.numel()].view(x.shape)
    y.copy_(x)
    return y


def fused_dense(v: dict):
    r"""Every operand of a variant materialised over ``(N, nM[, ...])``, contiguous: ``.expand(...).contiguous()``
    of the given form, so the numbers are the given ones (a cube's spins flattened in row-major order)."""
    N, Nd = v['loc'].shape[0], tuple(v['loc'].shape[1:-1])
    N = max(N, v['M0'].shape[0])
    nM, lead = 1, 1 + len(Nd)
    for d in Nd:
        nM *= d
    out = dict(v)
    for k in ('Δf', 'γ_beff', 'T1', 'T2', 'γ'):
        x = v.get(k)
        if x is not None:
            x = x.reshape(tuple(x.shape) + (lead - x.ndim) * (1,))
            out[k] = x.expand((N,) + Nd).reshape(N, nM).contiguous()
    if v.get('b1Map') is not None:
        b = v['b1Map']
        tail = tuple(b.shape[lead:])
        out['b1Map'] = b.expand((N,) + Nd + tail).reshape((N, nM) + tail).contiguous()
    if v.get('rx') is not None:           # the receive map of fused.signal_rfgr: the layout of b1Map
        r = v['rx']
        tail = tuple(r.shape[lead:])
        out['rx'] = r.expand((N,) + Nd + tail).reshape((N, nM) + tail).contiguous()
    for k in ('M0', 'loc', 'w'):
        out[k] = v[k].expand((N,) + Nd + (3,)).reshape(N, nM, 3).contiguous()
    for k in ('rf', 'gr'):
        out[k] = v[k].expand((N,) + tuple(v[k].shape[1:])).contiguous()
    out['dt'] = v['dt'].reshape(-1).expand(N).contiguous()
    return out


def fused_operand_variants(dtype, nC: int, nT: int = 48, seed: int = 29):
    r"""One problem class, many spellings: ``{name: (as_given, dense)}`` for ``fused.blochsim_rfgr`` / ``_traj``.
    N = 2, 140 spins per batch entry, ``nC`` transmit coils, 0 .. 8 (the goldens hold :data:`FUSED_COILS`).  A variant is a dict ``M0, rf, gr, loc, Δf, b1Map,
    γ_beff, T1, T2, γ, dt`` and the loss cotangent ``w``; ``dense`` is :func:`fused_dense` of it.  CPU tensors; a view
    keeps its strides and storage offset on a device through ``tests/gpu_common.py: place``.

    ``rx``: the receive map of ``fused.signal_rfgr``, one spelling per variant (batch-1, absent, stride-0, three coils on
    the grid, one weight per plane, fp64 meant to stay on the CPU, a permuted view, off the 16-B grid).  It is drawn from
    a generator of its own, so the other operands keep the bits ``golden/fusedops_*.npz`` was recorded on."""
    assert 0 <= nC <= 8
    gen = torch.Generator(device='cpu').manual_seed(seed + 100 * nC + nT)
    u = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64)        # noqa: E731
    N, nM, Nd = FUSED_N, FUSED_NM, FUSED_ND
    cd = (nC,) if nC > 1 else ()
    c = lambda x: x.to(dtype)                                                # noqa: E731
    M0 = lambda *s: c(u(*s, 3) * 2 - 1)                                      # noqa: E731
    loc = lambda *s: c((u(*s, 3) * 2 - 1) * 6)                               # noqa: E731
    rf = lambda n, T=nT: c((u(n, 2, T, *cd) * 2 - 1) * (1.5 if nC > 1 else 3))   # noqa: E731
    gr = lambda n, T=nT: c(u(n, 3, T) * 2 - 1)                               # noqa: E731
    df = lambda *s: c((u(*s) * 2 - 1) * 200)                                 # noqa: E731
    t1 = lambda *s: c(0.5 + u(*s))                                           # noqa: E731
    t2 = lambda *s: c(0.02 + 0.1 * u(*s))                                    # noqa: E731
    gm = lambda *s: c(γH_val * (0.9 + 0.2 * u(*s)))                          # noqa: E731
    b1 = lambda *s, coil=True: (None if nC == 0 else                         # noqa: E731
                                c((u(*s, 2, *((max(nC, 1),) if coil else ())) * 2 - 1) * (0.7 if nC > 1 else 1)))
    wt = lambda *s: c(u(*s, 3) * 2 - 1)                                      # noqa: E731
    dt1 = tensor([dt0_val], dtype=dtype)
    dtN = c(dt0_val * (1 + u(N)))
    gen_rx = torch.Generator(device='cpu').manual_seed(7919 + seed + 100 * nC + nT)
    rx64 = lambda *s: torch.rand(s, generator=gen_rx, dtype=torch.float64) * 2 - 1   # noqa: E731
    v = {}
    v['compact_mixed'] = dict(M0=M0(N, nM), rf=rf(1), gr=gr(N), loc=loc(N, nM), Δf=df(N, 1), γ_beff=gm(1, nM),
                              b1Map=b1(1, nM, coil=nC > 1), T1=t1(N, 1), T2=t2(N, 1), γ=gm(1, nM), dt=dtN, w=wt(N, nM))
    v['scalars'] = dict(M0=M0(N, nM), rf=rf(N), gr=gr(1), loc=loc(N, nM), Δf=df().reshape(()),
                        γ_beff=tensor(γH_val, dtype=torch.float64), b1Map=b1(N, 1), T1=t1(1, 1), T2=t2(1, 1),
                        γ=gm().reshape(()), dt=tensor(dt0_val, dtype=dtype), w=wt(N, nM))
    ex = lambda x: None if x is None else x.expand((N, nM) + tuple(x.shape[2:]))   # noqa: E731
    v['expanded'] = dict(M0=M0(N, nM), rf=rf(N), gr=gr(N), loc=ex(loc(1, nM)), Δf=ex(df(N, 1)), γ_beff=ex(gm(1, 1)),
                         b1Map=ex(b1(1, nM)), T1=ex(t1(N, 1)), T2=ex(t2(1, 1)), γ=ex(gm(1, nM)), dt=dt1, w=wt(N, nM))
    v['cube'] = dict(M0=M0(N, *Nd), rf=rf(N), gr=gr(N), loc=loc(N, *Nd), Δf=df(N, 1, 1, 1), γ_beff=gm(1, *Nd),
                     b1Map=b1(N, *Nd), T1=t1(1, *Nd), T2=t2(1, *Nd), γ=gm(N, 1, 1, 1), dt=dtN, w=wt(N, *Nd))
    v['cube_planes'] = dict(M0=M0(N, *Nd), rf=rf(1), gr=gr(1), loc=loc(N, *Nd), Δf=df(N, 5, 1, 1),
                            γ_beff=gm(1, 1, 4, 7), b1Map=b1(1, *Nd), T1=t1(N, 5), T2=t2(N, 5), γ=gm().reshape(()),
                            dt=dt1, w=wt(N, *Nd))
    v['gamma_split'] = dict(M0=M0(N, nM), rf=rf(N), gr=gr(N), loc=loc(N, nM), Δf=df(N, nM), γ_beff=gm(N, nM),
                            b1Map=b1(N, nM), T1=t1(N, 1), T2=t2(N, 1), γ=gm(N, nM), dt=dt1, w=wt(N, nM))
    long_rf, long_gr = rf(N, nT + 9), gr(N, nT + 9)
    # permuted views, time slices of a longer pulse, a non-contiguous cotangent
    v['views'] = dict(M0=c(u(3, N, nM) * 2 - 1).permute(1, 2, 0), rf=long_rf[:, :, 4:4 + nT], gr=long_gr[:, :, 4:4 + nT],
                      loc=c((u(3, nM, N) * 2 - 1) * 6).permute(2, 1, 0), Δf=df(nM, N).t(), γ_beff=gm(N, nM),
                      b1Map=b1(N, nM), T1=t1(N, nM), T2=t2(N, nM), γ=gm(1, 1), dt=dt1,
                      w=c(u(N, 3, nM) * 2 - 1).transpose(1, 2))
    v['offset'] = dict(M0=_after(M0(N, nM)), rf=_after(rf(N)), gr=_after(gr(N)), loc=_after(loc(N, nM)), Δf=df(N, nM),
                       γ_beff=gm(1, 1), b1Map=b1(N, nM), T1=t1(N, nM), T2=t2(N, nM), γ=gm(1, 1), dt=dt1,
                       w=_after(wt(N, nM)))
    v['compact_mixed']['rx'] = c(rx64(1, nM, 2))                             # broadcast over the batch
    v['scalars']['rx'] = None                                                # the plain sums of Mx, My
    v['expanded']['rx'] = c(rx64(N, 1, 2)).expand(N, nM, 2)                  # stride 0 over the spins
    v['cube']['rx'] = c(rx64(N, *Nd, 2, 3))                                  # three receive coils on the grid
    v['cube_planes']['rx'] = c(rx64(1, 5, 1, 1, 2))                          # one weight per plane
    v['gamma_split']['rx'] = rx64(N, nM, 2)                                  # fp64 whatever `dtype`; the tests leave it on the CPU
    v['views']['rx'] = c(rx64(2, nM, N)).permute(2, 1, 0)
    v['offset']['rx'] = _after(c(rx64(N, nM, 2)))
    return {k: (d, fused_dense(d)) for k, d in v.items()}


# zero-field steps (0-based, inclusive): every batch entry; batch entry 1 also a whole checkpoint segment
ZERO_STEPS = tuple(range(0, 5)) + tuple(range(14, 19)) + tuple(range(44, 48))
ZERO_SEGMENT = tuple(range(16, 32))
ZERO_RF_ONLY = (8, 9, 10)              # rf = 0, gr live: only the spins at loc = 0 are at zero field
ZERO_SPINS = ((0, 7), (1, 64))         # (batch entry, spin) at loc = 0: mid-wave; first lane of the second tile


def zero_field_case(dtype, nC: int, nT: int = 48, seed: int = 31):
    r"""Dead time through the fused adjoints, sizes as :func:`fused_operand_variants`, no ``Δf``: ``rf = gr = 0`` on
    :data:`ZERO_STEPS` (leading, straddling the checkpoint boundary at 16, trailing), batch entry 1 also on the whole
    segment :data:`ZERO_SEGMENT`; ``rf = 0`` alone on :data:`ZERO_RF_ONLY`, where the two spins at ``loc = 0``
    (:data:`ZERO_SPINS`) are the only lanes of their waves at zero field; with a map, ``b1Map = 0`` for spin 64 of
    entry 1, which then never rotates.  Returns the operand dict (keys as the variants') and ``zero``, the boolean
    `(N, nT)` mask of the steps where a batch entry's whole pulse sample is zero."""
    assert 0 <= nC <= 8
    gen = torch.Generator(device='cpu').manual_seed(seed + 100 * nC + nT)
    u = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64)        # noqa: E731
    N, nM = FUSED_N, FUSED_NM
    cd = (nC,) if nC > 1 else ()
    rf = (u(N, 2, nT, *cd) * 2 - 1) * (1.5 if nC > 1 else 3)
    gr = u(N, 3, nT) * 2 - 1
    loc = (u(N, nM, 3) * 2 - 1) * 6
    b1 = None if nC == 0 else (u(N, nM, 2, *cd) * 2 - 1) * (0.7 if nC > 1 else 1)
    zero = torch.zeros((N, nT), dtype=torch.bool)
    zero[:, list(ZERO_STEPS)] = True
    zero[1, list(ZERO_SEGMENT)] = True
    rf[:, :, list(ZERO_RF_ONLY)] = 0
    rf.movedim(2, 1)[zero] = 0
    gr.movedim(2, 1)[zero] = 0
    for n, s in ZERO_SPINS:
        loc[n, s] = 0
    if b1 is not None:
        b1[1, 64] = 0
    d = dict(M0=(u(N, nM, 3) * 2 - 1), rf=rf, gr=gr, loc=loc, Δf=None, γ_beff=tensor(γH_val), b1Map=b1,
             T1=0.5 + u(N, nM), T2=0.02 + 0.1 * u(N, nM), γ=tensor(γH_val), dt=tensor([dt0_val]),
             w=u(N, nM, 3) * 2 - 1)
    return {k: (None if x is None else x.to(dtype)) for k, x in d.items()}, zero


# ---------------------------------------------------------------------------------------------
# The elementwise helpers (csrc/k_aux.hpp, the 1-step kernel): leading shapes that cross a 256-thread block, the
# spellings of one per-spin constant, special rows of beff2uϕ (tests/test_helpers_operands.py, test_helpers_host.py)
# ---------------------------------------------------------------------------------------------
HELPER_BLOCK = 256                    # every helper kernel: row = blockIdx.x * 256 + threadIdx.x
HELPER_CUBE = (5, 4, 7)


def helper_rows():
    r"""The leading shapes ``(N, *Nd)`` every helper test runs at, the smallest that cross a 256-thread block: one row
    short of a block, a block, one row more; 513 rows in three batch entries of 171, where blocks straddle batch entries
    and per-batch operands differ; a cube of two batch entries (280 rows)."""
    return ((1, 255), (1, 256), (1, 257), (3, 171), (2,) + HELPER_CUBE)


def helper_constant_forms(N: int, Nd: tuple, dtype, fn=None, seed: int = 41):
    r"""``{name: tensor}``: the spellings of ONE per-spin constant over spins ``(N, *Nd)``, as in
    :func:`fused_operand_variants` -- 0-dim, all-singleton, per batch entry, per spin of one entry, per spin, a stride-0
    ``.expand``, the transpose of its stored transpose, one element into a larger buffer, fp64 whatever ``dtype``; on
    a cube (``len(Nd) == 3``) also one value per plane, one per in-plane position, and one map for the whole batch.
    The stored numbers are ``fn(u)`` of uniform ``u`` in [0, 1) (fp64, the same ``u`` for the same ``seed`` whatever
    ``fn``: two constants that must share a form, E1 and E1 - 1, are two calls), cast to ``dtype``.  CPU tensors; a
    view keeps its strides and offset on the device through ``tests/gpu_common.py: place``."""
    gen = torch.Generator(device='cpu').manual_seed(seed + 1000 * N + len(Nd))
    fn = fn or (lambda u: u)
    raw = lambda *s: fn(torch.rand(s, generator=gen, dtype=torch.float64))      # noqa: E731
    mk = lambda *s: raw(*s).to(dtype)                                            # noqa: E731
    Nd = tuple(Nd)
    one = (1,) * len(Nd)
    nM = 1
    for d in Nd:
        nM *= d
    v = {'scalar': mk().reshape(()), 'one_one': mk(1, *one), 'per_batch': mk(N, *one), 'per_spin_of_one': mk(1, *Nd),
         'per_spin': mk(N, *Nd), 'expanded': mk(N, *one).expand(N, *Nd), 'after': _after(mk(N, *Nd)),
         'f64': raw(N, *Nd)}
    if len(Nd) == 1:
        v['transposed'] = mk(nM, N).t()
    else:
        assert len(Nd) == 3
        v['planes'] = mk(N, Nd[0], 1, 1)
        v['in_plane'] = mk(1, 1, Nd[1], Nd[2])
        v['planes_expanded'] = mk(N, Nd[0], 1, 1).expand(N, *Nd)      # no flat view exists: the host layer copies it
    return v


def helper_dense(c, N: int, Nd: tuple):
    r"""A constant form over ``(N, *Nd)``, fp64, contiguous: the numbers it holds, for the oracle."""
    Nd = tuple(Nd)
    x = c.double()
    x = x.reshape(tuple(x.shape) + (1 + len(Nd) - x.ndim) * (1,))
    return x.expand((N,) + Nd).contiguous()


BEFF_EPS = 1e-12                      # F.normalize's eps (reference beffective.py:35)
HELPER_SPECIAL = ('zero', 'below', 'tie', 'above', 'plain')


def beff_special_row(kind: str, dtype):
    r"""One field vector of each kind around the clamp of ``beff2uϕ``: exact zero; |b| = 3e-13 (inside the clamp, not
    zero); |b| = 1e-12 EXACTLY as ``dtype`` holds it, along x so that ``sqrt(x*x + 0 + 0)`` returns it whether or not the
    sum is contracted; |b| = 2e-12 (just outside); an ordinary vector."""
    row = {'zero': [0., 0., 0.], 'below': [1.8e-13, 0., -2.4e-13], 'tie': [BEFF_EPS, 0., 0.],
           'above': [0., -1.2e-12, 1.6e-12], 'plain': [3., -4., 12.]}[kind]
    return tensor(row, dtype=torch.float64).to(dtype)


def helper_special_positions(rows: int):
    r"""Flat row numbers that get a special row: the first, the last of block 0, the first of block 1, the last."""
    return tuple(sorted({p for p in (0, HELPER_BLOCK - 1, HELPER_BLOCK, rows - 1) if 0 <= p < rows}))


def plant_special_rows(b, shift: int = 0):
    r"""``b`` `(N, *Nd, xyz)` with :func:`beff_special_row` s written (in place, through a flat view of a contiguous
    ``b``) at :func:`helper_special_positions`, the kinds rotated by ``shift``; returns ``{flat row: kind}``."""
    flat = b.view(-1, 3)
    out = {}
    for i, p in enumerate(helper_special_positions(flat.shape[0])):
        kind = HELPER_SPECIAL[(i + shift) % len(HELPER_SPECIAL)]
        flat[p] = beff_special_row(kind, b.dtype)
        out[p] = kind
    return out


def beff2uphi_grad_closed(b, g, gU, gΦ, dtype):
    r"""Closed form of the adjoint of ``beff2uϕ`` in fp64, per row: ``b, gU`` `(rows, 3)`, ``g, gΦ`` `(rows,)`, the very
    numbers a ``dtype`` run reads (cast up by the caller).  With ``n = |b|`` and ``eps`` = 1e-12 AS ``dtype`` HOLDS IT --
    ``F.normalize`` clamps in the data type, and so does the kernel --

        n >= eps:  gb = gU/n - b (b·gU)/n³ - gΦ g b/n      (the tie included: ``clamp_min``'s backward passes ``>=``)
        0 < n < eps:  gb = gU/eps - gΦ g b/n               (the clamp cuts the U branch off the norm)
        n == 0:    gb = gU/eps                             (torch's norm backward is 0 at 0)

    and ``gg = -gΦ n`` per row.  ``n`` is compared as ``dtype`` computes it.  Pinned against torch's autograd through
    ``oracle/bloch_oracle.py: beff2uphi`` in ``tests/test_helpers_host.py``."""
    f64 = torch.float64
    eps_t = tensor(BEFF_EPS, dtype=dtype)
    bt = b.to(dtype)
    n_t = torch.sqrt(bt[:, 0] * bt[:, 0] + bt[:, 1] * bt[:, 1] + bt[:, 2] * bt[:, 2])
    b, g, gU, gΦ = b.to(f64), g.to(f64), gU.to(f64), gΦ.to(f64)
    n = b.norm(dim=-1)
    eps = float(eps_t.double())
    free = (n_t >= eps_t)
    safe = torch.where(n > 0, n, torch.ones_like(n))
    phi_term = torch.where((n > 0)[:, None], -(gΦ * g / safe)[:, None] * b, torch.zeros_like(b))
    g_free = gU / safe[:, None] - b * ((b * gU).sum(-1) / safe ** 3)[:, None] + phi_term
    g_clamped = gU / eps + phi_term
    return torch.where(free[:, None], g_free, g_clamped), -gΦ * n


def helper_mask(Nd: tuple):
    r"""A closed-form `(1, *Nd)` bool mask of any rank, about 3/5 of the voxels, first and last voxel included."""
    n = 1
    for d in Nd:
        n *= d
    k = torch.arange(n, dtype=torch.int64)
    m = ((k * k + 3 * k) % 5) != 3
    m[0] = m[-1] = True
    return m.reshape((1,) + tuple(Nd))


# nT, dt -> dt_new, new samples (counted on the CPU; tests/test_helpers_host.py asserts them), what the grid stresses
INTERP_GRIDS = (
    (257, 4e-6, 1.5e-6, 685),      # both sides cross 256; up to 3 outputs per source interval
    (300, 4e-6, 1.3e-5, 92),       # 208 source samples feed no interval's upper end
    (600, 4e-6, 8e-6, 299),        # every w == dx: weights exactly 1 and exactly 0
    (513, 2e-6, 7e-6, 146),
    (1, 4e-6, 1e-6, 4),
    (3, 4e-6, 2e-5, 0),            # a dwell time longer than the pulse: an empty result
)


# ---------------------------------------------------------------------------------------------
# The operand zoo and the zero-field case with the operands of fused.blochsim_rfgr_moving (``vel``) and
# fused.blochsim_rfgr_shim (``sh``, ``shMap``) beside them (tests/test_moving_shim_operands.py, _cases_host.py)
# ---------------------------------------------------------------------------------------------
MOVSHIM_NS = {'compact_mixed': 2, 'scalars': 4, 'expanded': 6, 'cube': 7, 'cube_planes': 2, 'gamma_split': 4, 'views': 6,
              'offset': 7}
MOVSHIM_STEP_CM = 0.02                # |vel dt| per step, cm (tests/test_moving.py)


def moving_shim_dense(v: dict):
    r""":func:`fused_dense` of a variant of :func:`moving_shim_variants`, and ``vel`` `(N, nM, 3)`, ``sh`` `(N, nS, nT)`, ``shMap``
    `(N, nM, nS)` contiguous in the data dtype (that of ``loc``), holding the numbers given."""
    out = fused_dense(v)
    N, nM = out['loc'].shape[:2]
    dtype, nS = v['loc'].dtype, v['nS']
    out['vel'] = v['vel'].to(dtype).expand((N,) + tuple(v['vel'].shape[1:])).reshape(N, nM, 3).contiguous()
    out['sh'] = v['sh'].to(dtype).expand((N,) + tuple(v['sh'].shape[1:])).contiguous()
    out['shMap'] = v['shMap'].to(dtype).expand((N,) + tuple(v['shMap'].shape[1:])).reshape(N, nM, nS).contiguous()
    return out


def moving_shim_variants(dtype, nC: int, nT: int = 48, seed: int = 53):
    r""":func:`fused_operand_variants`'s eight spellings (``nC`` 0 or 1: the kernels take one transmit coil), each with a
    velocity ``vel`` and ``nS`` = :data:`MOVSHIM_NS` field channels ``sh``, ``shMap`` in a spelling that goes with the variant's:
    ``{name: (as_given, dense)}``, ``dense`` by :func:`moving_shim_dense`.

        compact_mixed  vel (1, nM, 3)                  sh (N, 2, nT)                   shMap (1, nM, 2)
        scalars        (N, 1, 3) expanded over nM      (1, 4, nT)                      (N, 1, 4) expanded over nM
        expanded       (1, 1, 3) expanded to (N, nM)   (1, 6, nT) expanded over N      (1, nM, 6) expanded over N
        cube           (N, *Nd, 3)                     (N, 7, nT)                      (N, *Nd, 7)
        cube_planes    (1, *Nd, 3)                     (1, 2, nT)                      (1, 5, 1, 1, 2) expanded over the planes
        gamma_split    fp64 whatever ``dtype`` (holding numbers ``dtype`` holds), nS = 4
        views          (3, nM, N) permuted             channels 1..7, steps 4..4+nT of (N, 9, nT + 9)   (6, N, nM) permuted
        offset         one element into a larger buffer, nS = 7

    ``|vel dt| <= 0.02 cm`` per step with the variant's own ``dt`` (its largest entry), ``sh`` in +-1, ``shMap`` in +-2: the
    amplitudes of ``tests/test_moving.py`` and ``test_shim.py``.  The new operands are drawn from a generator of their own
    after :func:`fused_operand_variants` has returned: that function's tensors keep their bits."""
    assert nC in (0, 1)
    base = fused_operand_variants(dtype, nC, nT)
    gen = torch.Generator(device='cpu').manual_seed(seed + 100 * nC + nT)
    u = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64) * 2 - 1    # noqa: E731
    N, nM, Nd = FUSED_N, FUSED_NM, FUSED_ND
    c = lambda x: x.to(dtype)                                                    # noqa: E731
    out = {}
    for name, (given, _) in base.items():
        nS = MOVSHIM_NS[name]
        amp = MOVSHIM_STEP_CM / float(given['dt'].double().max())
        vel = lambda *s: c(u(*s, 3) * amp)                                       # noqa: E731
        sh = lambda n, T=nT, k=nS: c(u(n, k, T))                                 # noqa: E731
        mp = lambda *s: c(u(*s, nS) * 2)                                         # noqa: E731
        if name == 'compact_mixed':
            new = dict(vel=vel(1, nM), sh=sh(N), shMap=mp(1, nM))
        elif name == 'scalars':
            new = dict(vel=vel(N, 1).expand(N, nM, 3), sh=sh(1), shMap=mp(N, 1).expand(N, nM, nS))
        elif name == 'expanded':
            new = dict(vel=vel(1, 1).expand(N, nM, 3), sh=sh(1).expand(N, nS, nT), shMap=mp(1, nM).expand(N, nM, nS))
        elif name == 'cube':
            new = dict(vel=vel(N, *Nd), sh=sh(N), shMap=mp(N, *Nd))
        elif name == 'cube_planes':
            new = dict(vel=vel(1, *Nd), sh=sh(1), shMap=mp(1, Nd[0], 1, 1).expand(1, *Nd, nS))
        elif name == 'gamma_split':      # fp64 operands beside `dtype` data: numbers that `dtype` holds, widened
            new = dict(vel=vel(N, nM).double(), sh=sh(N).double(), shMap=mp(N, nM).double())
        elif name == 'views':
            new = dict(vel=c(u(3, nM, N) * amp).permute(2, 1, 0), sh=sh(N, nT + 9, 9)[:, 1:1 + nS, 4:4 + nT],
                       shMap=c(u(nS, N, nM) * 2).permute(1, 2, 0))
        else:
            assert name == 'offset'
            new = dict(vel=_after(vel(N, nM)), sh=_after(sh(N)), shMap=_after(mp(N, nM)))
        v = dict(given, nS=nS, **new)
        out[name] = (v, moving_shim_dense(v))
    return out


def moving_shim_zero_field(dtype, nC: int, nT: int = 48, seed: int = 59):
    r""":func:`zero_field_case` with ``vel`` `(N, nM, 3)`, ``sh`` `(N, 3, nT)` and ``shMap`` `(N, nM, 3)`: ``vel = 0`` and
    ``shMap = 0`` for the spins :data:`ZERO_SPINS`, ``sh = 0`` on the mask ``zero`` and on :data:`ZERO_RF_ONLY`, so that through the
    moving call and through the channel call the same lanes are at exactly zero field on the same steps as in the static
    case.  Returns ``(operands, zero)``."""
    assert nC in (0, 1)
    d, zero = zero_field_case(dtype, nC, nT)
    gen = torch.Generator(device='cpu').manual_seed(seed + 100 * nC + nT)
    u = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64) * 2 - 1    # noqa: E731
    N, nM, nS = FUSED_N, FUSED_NM, 3
    vel, sh, mp = u(N, nM, 3) * (MOVSHIM_STEP_CM / dt0_val), u(N, nS, nT), u(N, nM, nS) * 2
    sh[:, :, list(ZERO_RF_ONLY)] = 0
    sh.movedim(2, 1)[zero] = 0
    for n, s in ZERO_SPINS:
        vel[n, s] = 0
        mp[n, s] = 0
    return dict(d, vel=vel.to(dtype), sh=sh.to(dtype), shMap=mp.to(dtype), nS=nS), zero
