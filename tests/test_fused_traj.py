r"""K2t / K2bt: the magnetisation trajectory of the fused simulation, ``fused.blochsim_rfgr_traj`` -- the forward against
prefix runs of ``blochsim_rfgr`` (bit for bit) and the oracle, gradients against the per-segment composition and the
oracle, the composed fallback, memory (no ``Beff`` in HBM) and hipGraph capture."""
import pytest

from gpu_common import *  # noqa: F401,F403
from mrphy_amd.fused import _traj_by_segments, _traj_ends

pytestmark = pytest.mark.gpu

VARIANTS = ['plain', 'b1map', 'norelax', 'ptx4', 'ptx8', 'plain_batch1_pulse']


def _problem(tag, variant, nT, seed=23, N=2, nM=100):
    r"""The operands of ``test_fused.test_fused_adjoint``'s variants (CPU tensors); nM = 100: a ragged second tile."""
    dt_ = DT[tag]
    gen = torch.Generator().manual_seed(seed + nT)
    rnd = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64)  # noqa: E731
    Np = 1 if variant.endswith('batch1_pulse') else N
    nC = {'ptx4': 4, 'ptx8': 8}.get(variant, 0)
    P = dict(M0=rnd(N, nM, 3).to(dt_),
             rf=((rnd(Np, 2, nT) * 2 - 1) * 3).to(dt_), gr=((rnd(Np, 3, nT) * 2 - 1)).to(dt_),
             loc=((rnd(N, nM, 3) * 2 - 1) * 6).to(dt_), df=((rnd(N, nM) * 2 - 1) * 200).to(dt_),
             b1=(rnd(N, nM, 2) * 2 - 1).to(dt_) if variant == 'b1map' else None)
    if nC:
        P['rf'] = ((rnd(Np, 2, nT, nC) * 2 - 1) * 1.5).to(dt_)
        P['b1'] = ((rnd(N, nM, 2, nC) * 2 - 1) * 0.7).to(dt_)
    P['T1'], P['T2'] = (0.5 + rnd(N, nM)).to(dt_), (0.02 + 0.1 * rnd(N, nM)).to(dt_)
    if variant == 'norelax':
        P['T1'] = P['T2'] = None
    P['γ'], P['dt'] = torch.tensor(4257.6, dtype=dt_), torch.tensor([4e-6], dtype=dt_)
    return P


def _kw(P, on):
    return dict(Δf=on(P['df']), b1Map=on(P['b1']), γ_beff=on(P['γ']), T1=on(P['T1']), T2=on(P['T2']),
                γ=on(P['γ']), dt=on(P['dt']))


def _oracle_traj(Mi, rf, gr, P, ends):
    r"""The CPU oracle looped over the record segments: (N, nM, nRec, 3)."""
    be = O.rfgr2beff(rf, gr, P['loc'], Δf=P['df'], b1Map=P['b1'], γ=P['γ'])
    kw = dict(T1=P['T1'], T2=P['T2'], γ=P['γ'], dt=P['dt'])
    out, M, t = [], Mi, 0
    for e in ends:
        M = O.blochsim(M, be[:, :, t:e], **kw)
        out.append(M)
        t = e
    return torch.stack(out, dim=-2)


def _weights(shape, dtype):
    return torch.sin(torch.arange(int(torch.tensor(shape).prod()), dtype=torch.float64) * 0.61 + 1) \
        .reshape(shape).to(dtype)


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('nT', [48, 50, 7])
def test_traj_forward_bits(tag, variant, nT):
    r"""Record j == blochsim_rfgr over the first s_j = min((j+1) every, nT) steps, bit for bit; the last record ==
    blochsim_rfgr; the trajectory is the oracle's, for every stride (inside a segment, on segment boundaries,
    across segments, one record, more than nT)."""
    P = _problem(tag, variant, nT)
    d = lambda x: None if x is None else dev(x)  # noqa: E731
    kw = _kw(P, d)
    Mi, rf, gr, loc = d(P['M0']), d(P['rf']), d(P['gr']), d(P['loc'])
    ora_all = _oracle_traj(P['M0'], P['rf'], P['gr'], P, list(range(1, nT + 1)))     # every step
    with torch.no_grad():
        Mo = fused.blochsim_rfgr(Mi, rf, gr, loc, **kw)
        for every in (1, 3, 16, 40, nT, nT + 5):
            ends = _traj_ends(nT, every)
            Mt = fused.blochsim_rfgr_traj(Mi, rf, gr, loc, every=every, **kw)
            assert Mt.shape == (2, 100, len(ends), 3)
            assert Mt.movedim(-2, 0).is_contiguous()                      # a view of time-major storage
            pre = torch.stack([fused.blochsim_rfgr(Mi, rf[:, :, :e], gr[:, :, :e], loc, **kw) for e in ends], dim=-2)
            assert max_abs(Mt, pre) == 0.0, (every, 'prefix runs')
            assert max_abs(Mt[..., -1, :], Mo) == 0.0, (every, 'last record')
            assert_close(Mt.cpu(), ora_all[..., [e - 1 for e in ends], :], tag, f'Mt vs oracle (every={every})')


def _grad_run(kind, P, every, tag, on, w):
    Mi, r, g = (on(x).clone().requires_grad_(True) for x in (P['M0'], P['rf'], P['gr']))
    kw = _kw(P, on)
    ends = _traj_ends(P['rf'].shape[2], every)
    if kind == 'oracle':
        Mt = _oracle_traj(Mi, r, g, P, ends)
    elif kind == 'segments':
        Mt = _traj_by_segments(Mi, r, g, on(P['loc']), ends, kw).movedim(0, -2)
    else:
        Mt = fused.blochsim_rfgr_traj(Mi, r, g, on(P['loc']), every=every, **kw)
    (Mt * on(w)).sum().backward()
    return Mt.detach(), Mi.grad, r.grad, g.grad


def _check_grads(P, every, tag, with_oracle=True):
    d = lambda x: None if x is None else dev(x)  # noqa: E731
    nRec = len(_traj_ends(P['rf'].shape[2], every))
    w = _weights((2, 100, nRec, 3), P['M0'].dtype)
    tr = _grad_run('traj', P, every, tag, d, w)
    seg = _grad_run('segments', P, every, tag, d, w)
    names = ('Mt', 'grad_Mi', 'grad_rf', 'grad_gr')
    for a, b, nm in zip(tr, seg, names):
        assert a.shape == b.shape, nm
        assert_close(a, b, tag, f'{nm} vs segment loop (every={every})')
    if with_oracle:
        ora = _grad_run('oracle', P, every, tag, lambda x: x, w)
        for a, c, nm in zip(tr, ora, names):
            assert_close(a, c, tag, f'{nm} vs oracle (every={every})')
    again = _grad_run('traj', P, every, tag, d, w)
    for a, b, nm in zip(tr, again, names):
        assert max_abs(a, b) == 0.0, nm                                   # deterministic reduction
    return tr


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('nT,every', [(48, 1), (48, 3), (48, 16), (48, 40), (48, 48), (50, 3), (50, 16),
                                      (16, 1), (16, 5), (16, 16), (16, 21)])
def test_traj_gradients(tag, variant, nT, every):
    r"""Loss (Mt * w).sum(): grad_Mi, grad_rf, grad_gr of the trajectory kernels == autograd through the per-segment
    composition == the oracle; twice the same bits.  every < 16 takes the per-step injection, every >= 16 the
    per-segment one; nT = 50 the fused part + composed tail; nT = 16 one checkpoint segment."""
    _check_grads(_problem(tag, variant, nT), every, tag)


@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('empty', ['nT', 'nM'])
def test_traj_empty_problem(tag, empty):
    r"""No step (nT = 0) or no spin (nM = 0) through the Python API: ``Mt`` is `(N, nM, 0, 3)` / `(N, 0, nRec, 3)` and
    ``blochsim_rfgr``'s ``Mo`` is ``Mi``; the backward runs -- ``grad_Mi`` is the cotangent of ``Mo`` (zero for the
    trajectory without a record), the pulse gradients are zeros of the shapes of ``rf`` and ``gr``."""
    nT, nM, every = (0, 100, 3) if empty == 'nT' else (32, 0, 5)
    P = _problem(tag, 'plain', 32, nM=nM)
    P['rf'], P['gr'] = P['rf'][:, :, :nT], P['gr'][:, :, :nT]
    nRec = len(_traj_ends(nT, every))
    for traj in (True, False):
        Mi, rf, gr = (dev(P[k]).clone().requires_grad_(True) for k in ('M0', 'rf', 'gr'))
        if traj:
            out = fused.blochsim_rfgr_traj(Mi, rf, gr, dev(P['loc']), every=every, **_kw(P, dev))
            assert out.shape == (2, nM, nRec, 3) and out.dtype == DT[tag]
        else:
            out = fused.blochsim_rfgr(Mi, rf, gr, dev(P['loc']), **_kw(P, dev))
            assert out.shape == Mi.shape and (nT > 0 or torch.equal(out, Mi.detach()))
        w = dev(_weights(tuple(out.shape), out.dtype))
        (out * w).sum().backward()
        assert Mi.grad.shape == Mi.shape
        assert torch.equal(Mi.grad, torch.zeros_like(Mi) if traj else w), traj
        for g, x in ((rf.grad, rf), (gr.grad, gr)):
            assert g is not None and g.shape == x.shape and g.dtype == x.dtype and bool((g == 0).all()), traj


@pytest.mark.parametrize('mode,wide', [('fast', False), ('fast', True), ('precise', False), ('precise', True)])
@pytest.mark.parametrize('every', [1, 5, 16, 40])
def test_traj_gradients_dtype_codes(mode, wide, every):
    r"""fp32 data through dtype codes 0 / 2 (fast; fp32 / fp64 constants) and 3 / 4 (precise: the adjoint carries
    t = E h, so a record's cotangent must enter scaled by E), with relaxation, against the per-segment composition in
    the same mode (a raw add in t-state would be off by a factor E per record); code 3 is also held to the oracle."""
    from mrphy_amd import _host
    P = _problem('f32', 'plain', 48, seed=5)
    if wide:                                          # fp64 constants with fp32 data: codes 2 / 4
        P['T1'], P['T2'], P['γ'], P['dt'] = (P[k].double() for k in ('T1', 'T2', 'γ', 'dt'))
    with mrphy_amd.precision(mode):
        code = _host.dtype_code(torch.float32, torch.float64 if wide else torch.float32)
        assert code == {('fast', False): 0, ('fast', True): 2, ('precise', False): 3, ('precise', True): 4}[mode, wide]
        if mode == 'precise' and not wide:
            with mrphy_amd.constants_on('cpu'):
                _check_grads(P, every, 'f32', with_oracle=True)
        else:
            _check_grads(P, every, 'f32', with_oracle=False)


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('case', ['b1map_grad', 'ptx12'])
def test_traj_fallback_matches_oracle(case):
    r"""Outside fused-adjoint coverage -- a gradient w.r.t. the b1 map, a 12-coil pTx gradient -- the trajectory is
    composed per record segment; it still matches the oracle, values and gradients."""
    tag = 'f32'
    P = _problem(tag, 'ptx4' if case == 'ptx12' else 'b1map', 48, seed=77)
    if case == 'ptx12':
        gen = torch.Generator().manual_seed(12)
        P['rf'] = ((torch.rand(2, 2, 48, 12, generator=gen, dtype=torch.float64) * 2 - 1) * 0.6).float()
        P['b1'] = ((torch.rand(2, 100, 2, 12, generator=gen, dtype=torch.float64) * 2 - 1) * 0.5).float()
    every = 5
    ends = _traj_ends(48, every)
    w = _weights((2, 100, len(ends), 3), torch.float32)

    def run(on):
        Mi, r, g = (on(x).clone().requires_grad_(True) for x in (P['M0'], P['rf'], P['gr']))
        b1 = on(P['b1']).clone().requires_grad_(case == 'b1map_grad')
        kw = _kw(P, lambda x: None if x is None else on(x))
        kw['b1Map'] = b1
        if on is dev:
            Mt = fused.blochsim_rfgr_traj(Mi, r, g, on(P['loc']), every=every, **kw)
        else:
            Q = dict(P, b1=b1)
            Mt = _oracle_traj(Mi, r, g, Q, ends)
        (Mt * on(w)).sum().backward()
        return [Mt.detach(), Mi.grad, r.grad, g.grad] + ([b1.grad] if case == 'b1map_grad' else [])
    for a, b, nm in zip(run(dev), run(lambda x: x), ('Mt', 'grad_Mi', 'grad_rf', 'grad_gr', 'grad_b1')):
        assert_close(a, b, tag, f'{case}: {nm}')


def test_traj_materialises_no_beff():
    r"""32^3 x 1024 fp32, every = 16, forward + backward: the rise of the allocator's peak stays within 1.25 x
    (Mt + grad_Mt + checkpoints + workspace), about 2.8 B per spin-step; a Beff would be 12 B per spin-step."""
    lib = mrphy_amd.require_library()
    n, nT, every = 32, 1024, 16
    sp = synth.cube_spins(n, device=DEV)
    p = synth.pulse(nT, device=DEV)
    rf = (0.05 * p['rf']).clone().requires_grad_(True)
    gr = p['gr'].clone().requires_grad_(True)
    nM = n ** 3
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    Mt = fused.blochsim_rfgr_traj(sp['M0'], rf, gr, sp['loc'], every=every, Δf=sp['Δf'], γ_beff=sp['γ'],
                                  T1=sp['T1'], T2=sp['T2'], γ=sp['γ'], dt=p['dt'])
    Mt.sum().backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    nRec = nT // every
    mt = nRec * nM * 3 * 4
    ck = (nT // int(lib.mrphy_blochsim_rfgr_ck_every())) * nM * 3 * 4
    work = int(lib.mrphy_blochsim_rfgr_bwd_workspace(0, 1, nM, nT))
    bound = 1.25 * (2 * mt + ck + work)
    beff = nM * nT * 3 * 4
    record('traj.mem.rise_over_bound', rise / bound, 1.0, note=f'rise {rise} B, bound {bound:.0f} B, Beff {beff} B')
    assert rise <= bound < beff, (rise, bound, beff)
    assert torch.isfinite(rf.grad).all() and torch.isfinite(gr.grad).all()


@pytest.mark.parametrize('every', [4, 16])
def test_traj_hipgraph_capture(every):
    r"""Trajectory forward + adjoint at 16^3 x 256, captured into a HIP graph and replayed: the eager bits, also
    after the static inputs change in place."""
    n, nT = 16, 256
    sp = synth.cube_spins(n, device=DEV)
    p = synth.pulse(nT, device=DEV)
    rf = (0.05 * p['rf']).clone().requires_grad_(True)
    gr = p['gr'].clone().requires_grad_(True)

    def iteration():
        Mt = fused.blochsim_rfgr_traj(sp['M0'], rf, gr, sp['loc'], every=every, Δf=sp['Δf'], γ_beff=sp['γ'],
                                      T1=sp['T1'], T2=sp['T2'], γ=sp['γ'], dt=p['dt'])
        return torch.autograd.grad((Mt[..., 2] ** 2).sum() + Mt[..., 0].sum(), (rf, gr))

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            a0, b0 = iteration()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a1, b1 = iteration()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(a0, a1) and torch.equal(b0, b1)
    with torch.no_grad():
        rf.mul_(1.25)
        gr.add_(0.01)
    g.replay()
    torch.cuda.synchronize()
    a2, b2 = iteration()
    assert torch.equal(a1, a2) and torch.equal(b1, b2) and not torch.equal(a0, a2)
