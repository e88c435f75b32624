r"""K2s / the signal mode of K2b: ``fused.signal_rfgr``, the transverse magnetisation summed over the spins during the pulse
-- the forward against the fp64 reduction of the trajectory kernel's own records and against the oracle, ``Mo`` against
``blochsim_rfgr`` (bit for bit), gradients against autograd through the composed route (trajectory + torch reduction)
and the oracle, the precision modes, the fallbacks, memory (no trajectory) and hipGraph capture."""
import functools

import pytest

from gpu_common import *  # noqa: F401,F403
from mrphy_amd.fused import _signal_composed, _signal_of, _traj_ends
from test_fused_traj import _problem, _kw, _oracle_traj, _weights

pytestmark = pytest.mark.gpu

N, NM = 2, 100
EVERY = lambda nT: (1, 3, 16, 40, nT, nT + 5)  # noqa: E731


def _rx(tag, kind, nM=NM, n=N, seed=91):
    r"""``rx = rnd(N, nM, 2)·2 − 1`` (CPU): 'none' -> None, 'coil' -> (N, nM, 2), 'coil1' -> (N, nM, 2, 1), 'coil3' -> 3 coils."""
    if kind == 'none':
        return None
    gen = torch.Generator().manual_seed(seed)
    nRx = 3 if kind == 'coil3' else 1
    rx = (torch.rand((n, nM, 2, nRx), generator=gen, dtype=torch.float64) * 2 - 1).to(DT[tag])
    return rx[..., 0] if kind == 'coil' else rx


def _sig64(Mt, rx):
    r"""The fp64 product-and-sum of a trajectory ``Mt`` `(N, nM, nRec, 3)` with one receive map `(N, nM, 2)` or None, on the
    CPU: ``S64`` `(N, 2, nRec)`, and the sum of the absolute values of the terms, the scale of the summation's error."""
    M = Mt.detach().double().cpu()
    Mx, My = M[..., 0], M[..., 1]
    if rx is None:
        rr, ri = torch.ones_like(Mx[..., :1]), torch.zeros_like(Mx[..., :1])
    else:
        r = rx.detach().double().cpu().reshape(M.shape[0], M.shape[1], 2)
        rr, ri = r[..., 0:1], r[..., 1:2]
    s = torch.stack(((rr * Mx - ri * My).sum(1), (rr * My + ri * Mx).sum(1)), dim=1)
    a = torch.stack((((rr * Mx).abs() + (ri * My).abs()).sum(1), ((rr * My).abs() + (ri * Mx).abs()).sum(1)), dim=1)
    return s, a


@functools.lru_cache(maxsize=None)
def _oracle_all(tag, variant, nT):
    r"""The oracle's trajectory at every step, once per problem: (N, nM, nT, 3), CPU."""
    P = _problem(tag, variant, nT)
    with mrphy_amd.constants_on('cpu'):
        return _oracle_traj(P['M0'], P['rf'], P['gr'], P, list(range(1, nT + 1)))


# =============================================================================================
# 1. forward
# =============================================================================================
@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('variant', ['plain', 'b1map', 'norelax', 'plain_batch1_pulse'])
@pytest.mark.parametrize('nT', [48, 50, 7])
@pytest.mark.parametrize('rxk', ['none', 'coil', 'coil1'])
def test_signal_forward(tag, variant, nT, rxk):
    r"""Shape and dtype; ``Mo`` == blochsim_rfgr bit for bit; ``sig`` against S64, the fp64 reduction of the trajectory
    kernel's own records (the same M bit for bit: only the products and the order of summation differ) -- fp64 1e-9,
    fp32 relative L2 1e-5 and, elementwise, the first-order worst case of ANY summation order of nM two-product terms,
    (nM + 3) 2^-24 Σ_s (|rx_re M_a| + |rx_im M_b|) (sequential fp32 sums in random orders stay below 0.02 of it on
    these problems; the oracle's own fp32 signal is 1e-7 .. 7e-7 in relative L2 from its fp64 one); ``sig`` against the
    oracle's trajectory reduced in fp64; twice the same bits.  Strides inside a segment, on its boundary, across
    segments, one record, more than nT; lengths with nT % 8 and nT % 16 tails."""
    P = _problem(tag, variant, nT)
    rx = _rx(tag, rxk)
    rx1 = None if rx is None else rx.reshape(N, NM, 2)
    kw = _kw(P, dev)
    Mi, rf, gr, loc = dev(P['M0']), dev(P['rf']), dev(P['gr']), dev(P['loc'])
    ora_all = _oracle_all(tag, variant, nT)
    with torch.no_grad():
        Mo_ref = fused.blochsim_rfgr(Mi, rf, gr, loc, **kw)
        for every in EVERY(nT):
            ends = _traj_ends(nT, every)
            sig, Mo = fused.signal_rfgr(Mi, rf, gr, loc, every=every, rx=dev(rx), return_Mo=True, **kw)
            assert sig.shape == (N, 2, len(ends)) + ((1,) if rxk == 'coil1' else ()) and sig.dtype == DT[tag]
            assert Mo.shape == Mi.shape and Mo.dtype == DT[tag]
            assert max_abs(Mo, Mo_ref) == 0.0, (every, 'Mo')
            only = fused.signal_rfgr(Mi, rf, gr, loc, every=every, rx=dev(rx), **kw)
            assert torch.equal(only, sig), (every, 'twice the same bits')
            s = sig.reshape(N, 2, len(ends))
            Mt = fused.blochsim_rfgr_traj(Mi, rf, gr, loc, every=every, **kw)
            S64, A64 = _sig64(Mt, rx1)
            assert_close(s, S64, tag, f'sig vs S64 (every={every})')
            if tag == 'f32':
                ratio = float(((s.double().cpu() - S64).abs() / ((NM + 3) * 2.0 ** -24 * A64)).max())
                record(f'signal.fwd.{variant}.nT{nT}.{rxk}.every{every}.elementwise_over_bound', ratio, 1.0)
                assert ratio <= 1.0, (every, ratio)
            O64, _ = _sig64(ora_all[..., [e - 1 for e in ends], :], rx1)
            assert_close(s, O64, tag, f'sig vs oracle (every={every})')


# =============================================================================================
# 2. more than one tile per wave: the workspace's read-modify-write path
# =============================================================================================
@pytest.mark.parametrize('tiles', [2048, 4096])
@pytest.mark.parametrize('every', [1, 16])
def test_signal_second_tile_per_wave(tiles, every):
    r"""N = 1, nM = tiles·64 + 100, nT = 32, fp32, with rx: more spin tiles than the forward has persistent waves (its
    cap is 4096 waves; 2048 is the cap of the adjoint's), so a wave adds its later tiles into its workspace row.
    Gate: relative L2 <= 1e-5 against S64 -- the kernel's summation order emulated on the CPU for 131 172 random terms
    gives 1e-5 .. 5e-5 absolute on sums whose vector norm per element is about 120, 1e-7 .. 4e-7 relative; a dropped
    tile would show at about 2e-2.  Twice the same bits."""
    nM, nT = tiles * 64 + 100, 32
    P = _problem('f32', 'plain', nT, N=1, nM=nM)
    rx = _rx('f32', 'coil', nM=nM, n=1)
    kw = _kw(P, dev)
    args = (dev(P['M0']), dev(P['rf']), dev(P['gr']), dev(P['loc']))
    with torch.no_grad():
        sig = fused.signal_rfgr(*args, every=every, rx=dev(rx), **kw)
        again = fused.signal_rfgr(*args, every=every, rx=dev(rx), **kw)
        S64, _ = _sig64(fused.blochsim_rfgr_traj(*args, every=every, **kw), rx)
    assert sig.shape == (1, 2, nT // every)
    d = record(f'signal.fwd.tiles{tiles}.every{every}.vs_S64', rel_l2(sig, S64), 1e-5)
    assert d <= 1e-5, d
    assert torch.equal(sig, again)


# =============================================================================================
# 3. gradients
# =============================================================================================
def _loss(sig, Mo, w, v, terms):
    return ((sig * w).sum() if 's' in terms else 0) + ((Mo * v).sum() if 'm' in terms else 0)


def _grad_run(kind, P, rx, every, on, terms='sm', rx_grad=False, loc_grad=False):
    r"""(sig, Mo, grad_Mi, grad_rf, grad_gr[, grad_rx][, grad_loc]) of the loss ``(sig·w).sum() + (Mo·v).sum()``."""
    Mi, r, g = (on(x).clone().requires_grad_(True) for x in (P['M0'], P['rf'], P['gr']))
    rxl = None if rx is None else on(rx).clone().requires_grad_(rx_grad)
    loc = on(P['loc']).clone().requires_grad_(loc_grad)
    kw = _kw(P, lambda x: None if x is None else on(x))
    nT = P['gr'].shape[2]
    if kind == 'oracle':
        Mt = _oracle_traj(Mi, r, g, dict(P, loc=loc), _traj_ends(nT, every)).movedim(-2, 0)
        sig, Mo = _signal_of(Mt, rxl), Mt[-1]
    elif kind == 'composed':
        sig, Mo = _signal_composed(Mi, r, g, loc, every, rxl, kw)
    else:
        sig, Mo = fused.signal_rfgr(Mi, r, g, loc, every=every, rx=rxl, return_Mo=True, **kw)
    w, v = on(_weights(tuple(sig.shape), sig.dtype)), on(_weights(tuple(Mo.shape), Mo.dtype))
    _loss(sig, Mo, w, v, terms).backward()
    return [sig.detach(), Mo.detach(), Mi.grad, r.grad, g.grad] + ([rxl.grad] if rx_grad else []) + \
        ([loc.grad] if loc_grad else [])


NAMES = ('sig', 'Mo', 'grad_Mi', 'grad_rf', 'grad_gr', 'grad_extra')


def _check_grads(P, rx, every, tag, with_oracle=True):
    for terms in ('sm', 's', 'm'):
        got = _grad_run('signal', P, rx, every, dev, terms)
        comp = _grad_run('composed', P, rx, every, dev, terms)
        for a, b, nm in zip(got, comp, NAMES):
            assert a.shape == b.shape, nm
            assert_close(a, b, tag, f'{nm} vs composed route (every={every}, loss terms {terms})')
        if with_oracle and terms == 'sm':
            for a, c, nm in zip(got, _grad_run('oracle', P, rx, every, lambda x: x, terms), NAMES):
                assert_close(a, c, tag, f'{nm} vs oracle (every={every})')
        for a, b, nm in zip(got, _grad_run('signal', P, rx, every, dev, terms), NAMES):
            assert max_abs(a, b) == 0.0, (nm, terms)                      # deterministic reduction
        if terms == 'm':                                                  # no cotangent on sig: blochsim_rfgr's gradients
            Mi, r, g = (dev(x).clone().requires_grad_(True) for x in (P['M0'], P['rf'], P['gr']))
            Mo = fused.blochsim_rfgr(Mi, r, g, dev(P['loc']), **_kw(P, dev))
            (Mo * dev(_weights(tuple(Mo.shape), Mo.dtype))).sum().backward()
            for a, b, nm in zip(got[2:], (Mi.grad, r.grad, g.grad), NAMES[2:]):
                if P['gr'].shape[2] % 16 == 0:
                    assert max_abs(a, b) == 0.0, nm
                else:
                    assert_close(a, b, tag, f'{nm} vs blochsim_rfgr')


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('variant', ['plain', 'b1map', 'norelax', 'plain_batch1_pulse'])
@pytest.mark.parametrize('nT,every', [(48, 1), (48, 3), (48, 16), (48, 40), (48, 48), (50, 3), (50, 16),
                                      (16, 1), (16, 5), (16, 16), (16, 21)])
def test_signal_gradients(tag, variant, nT, every):
    r"""Loss (sig·w).sum() + (Mo·v).sum(), and each term alone: grad_Mi, grad_rf, grad_gr of the signal kernels ==
    autograd through the composed route == the oracle (the gates of test_traj_gradients on the same problems); twice
    the same bits; with the Mo term alone they are blochsim_rfgr's.  nT = 50: the fused part + composed tail; nT = 16:
    one checkpoint segment (no previous checkpoint to fetch ahead); a batch-1 pulse: its gradients summed over N."""
    _check_grads(_problem(tag, variant, nT), _rx(tag, 'coil'), every, tag)


@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('empty', ['nT', 'nM'])
@pytest.mark.parametrize('rxk', ['none', 'coil'])
def test_signal_empty_problem(tag, empty, rxk):
    r"""No step (nT = 0) or no spin (nM = 0) through the Python API: ``sig`` is `(N, 2, 0)`, or zeros `(N, 2, nRec)`
    without spins; ``Mo`` is ``Mi``; the backward runs -- ``grad_Mi`` is the cotangent of ``Mo``, the pulse gradients are
    zeros of the shapes of ``rf`` and ``gr``."""
    nT, nM, every = (0, NM, 3) if empty == 'nT' else (32, 0, 5)
    P = _problem(tag, 'plain', 32, nM=nM)
    P['rf'], P['gr'] = P['rf'][:, :, :nT], P['gr'][:, :, :nT]
    rx = _rx(tag, rxk, nM=nM)
    Mi, rf, gr = (dev(P[k]).clone().requires_grad_(True) for k in ('M0', 'rf', 'gr'))
    sig, Mo = fused.signal_rfgr(Mi, rf, gr, dev(P['loc']), every=every, rx=dev(rx), return_Mo=True, **_kw(P, dev))
    nRec = len(_traj_ends(nT, every))
    assert sig.shape == (N, 2, nRec) and sig.dtype == DT[tag] and Mo.shape == Mi.shape
    assert nRec == (0 if empty == 'nT' else 7)
    assert bool((sig == 0).all()) and torch.equal(Mo, Mi.detach())
    v = dev(_weights(tuple(Mo.shape), Mo.dtype))
    ((sig * dev(_weights(tuple(sig.shape), sig.dtype))).sum() + (Mo * v).sum()).backward()
    assert Mi.grad.shape == Mi.shape and torch.equal(Mi.grad, v)
    for g, x in ((rf.grad, rf), (gr.grad, gr)):
        assert g is not None and g.shape == x.shape and g.dtype == x.dtype and bool((g == 0).all())


# =============================================================================================
# 4. precision modes and dtype codes
# =============================================================================================
@pytest.mark.parametrize('mode,wide', [('fast', False), ('fast', True), ('precise', False), ('precise', True)])
@pytest.mark.parametrize('every', [1, 5, 16, 40])
def test_signal_gradients_dtype_codes(mode, wide, every):
    r"""fp32 data through dtype codes 0 / 2 and 3 / 4 (precise: the adjoint carries t = E h, so a sample's cotangent must
    enter scaled by E), with relaxation, against the composed route in the same mode; code 3 is also held to the oracle."""
    from mrphy_amd import _host
    P = _problem('f32', 'plain', 48, seed=5)
    if wide:                                          # fp64 constants with fp32 data: codes 2 / 4
        P['T1'], P['T2'], P['γ'], P['dt'] = (P[k].double() for k in ('T1', 'T2', 'γ', 'dt'))
    rx = _rx('f32', 'coil')
    with mrphy_amd.precision(mode):
        code = _host.dtype_code(torch.float32, torch.float64 if wide else torch.float32)
        assert code == {('fast', False): 0, ('fast', True): 2, ('precise', False): 3, ('precise', True): 4}[mode, wide]
        if mode == 'precise' and not wide:
            with mrphy_amd.constants_on('cpu'):
                _check_grads(P, rx, every, 'f32', with_oracle=True)
        else:
            _check_grads(P, rx, every, 'f32', with_oracle=False)


# =============================================================================================
# 5. fallbacks
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_signal_receive_coils_are_one_launch_each(tag):
    r"""nRx = 3 == three one-coil calls stacked, bit for bit -- values and gradients' inputs (sig, Mo)."""
    P = _problem(tag, 'b1map', 48)
    rx = _rx(tag, 'coil3')
    kw = _kw(P, dev)
    args = (dev(P['M0']), dev(P['rf']), dev(P['gr']), dev(P['loc']))
    with torch.no_grad():
        sig, Mo = fused.signal_rfgr(*args, every=5, rx=dev(rx), return_Mo=True, **kw)
        one = [fused.signal_rfgr(*args, every=5, rx=dev(rx[..., c]), return_Mo=True, **kw) for c in range(3)]
    assert sig.shape == (N, 2, 10, 3)
    for c in range(3):
        assert torch.equal(sig[..., c], one[c][0]) and torch.equal(Mo, one[c][1])
    got = _grad_run('signal', P, rx, 5, dev)
    for a, b, nm in zip(got, _grad_run('composed', P, rx, 5, dev), NAMES):
        assert_close(a, b, tag, f'3 receive coils: {nm} vs composed route')


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('case', ['ptx4', 'loc_grad', 'rx_grad'])
def test_signal_fallbacks(case):
    r"""Outside the signal kernels' coverage -- parallel transmit, a gradient w.r.t. loc, a gradient w.r.t. rx -- the
    composed route's values and gradients are returned (the same bits), and they match the oracle."""
    tag = 'f32'
    P = _problem(tag, 'ptx4' if case == 'ptx4' else 'b1map', 48, seed=77)
    rx = _rx(tag, 'coil')
    flags = dict(rx_grad=case == 'rx_grad', loc_grad=case == 'loc_grad')
    got = _grad_run('signal', P, rx, 5, dev, **flags)
    comp = _grad_run('composed', P, rx, 5, dev, **flags)
    ora = _grad_run('oracle', P, rx, 5, lambda x: x, **flags)
    assert len(got) == (5 if case == 'ptx4' else 6)
    for a, b, c, nm in zip(got, comp, ora, NAMES):
        assert a is not None and a.shape == b.shape == c.shape, (case, nm)
        if nm in ('sig', 'Mo'):
            assert max_abs(a, b) == 0.0, (case, nm)
        assert_close(a, b, tag, f'{case}: {nm} vs composed route')
        assert_close(a, c, tag, f'{case}: {nm} vs oracle')


# =============================================================================================
# 6. no trajectory in memory
# =============================================================================================
def test_signal_materialises_no_trajectory():
    r"""N = 1, nM = 4096, nT = 256, every = 1, fp32, forward + backward: the allocator's peak rises by less than a quarter
    of the trajectory's bytes (the composed route needs more than all of them; the fused one the checkpoints, 1/16 of
    that, and two small workspaces)."""
    nM, nT = 4096, 256
    P = _problem('f32', 'plain', nT, N=1, nM=nM)
    rx = dev(_rx('f32', 'coil', nM=nM, n=1))
    kw = _kw(P, dev)
    Mi, loc = dev(P['M0']), dev(P['loc'])
    rf, gr = dev(P['rf']).requires_grad_(True), dev(P['gr']).requires_grad_(True)
    traj = nM * nT * 12

    def rise(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        sig, Mo = fn()
        ((sig ** 2).sum() + Mo.sum()).backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base
    fused_rise = rise(lambda: fused.signal_rfgr(Mi, rf, gr, loc, every=1, rx=rx, return_Mo=True, **kw))
    g = (rf.grad.clone(), gr.grad.clone())
    rf.grad = gr.grad = None
    comp_rise = rise(lambda: _signal_composed(Mi, rf, gr, loc, 1, rx, kw))
    record('signal.mem.rise_over_trajectory', fused_rise / traj, 0.25,
           note=f'fused {fused_rise} B, composed {comp_rise} B, trajectory {traj} B')
    assert fused_rise < 0.25 * traj < traj < comp_rise, (fused_rise, comp_rise, traj)
    assert_close(g[0], rf.grad, 'f32', 'grad_rf')
    assert_close(g[1], gr.grad, 'f32', 'grad_gr')


# =============================================================================================
# 7. hipGraph capture
# =============================================================================================
@pytest.mark.parametrize('every', [1, 16])
def test_signal_hipgraph_capture(every):
    r"""One design iteration (signal_rfgr, the loss, backward) at 16^3 x 256 captured into a HIP graph as
    examples/pulse_design.py does and replayed: the eager bits, also after the static inputs change in place."""
    n, nT = 16, 256
    sp = synth.cube_spins(n, device=DEV)
    p = synth.pulse(nT, device=DEV)
    rf = (0.05 * p['rf']).clone().requires_grad_(True)
    gr = p['gr'].clone().requires_grad_(True)
    rx = dev(_rx('f32', 'coil', nM=n ** 3, n=1)).reshape(sp['M0'].shape[:-1] + (2,))

    def iteration():
        sig, Mo = fused.signal_rfgr(sp['M0'], rf, gr, sp['loc'], every=every, rx=rx, return_Mo=True, Δf=sp['Δf'],
                                    γ_beff=sp['γ'], T1=sp['T1'], T2=sp['T2'], γ=sp['γ'], dt=p['dt'])
        return torch.autograd.grad((sig ** 2).sum() + (Mo[..., 2] ** 2).sum(), (rf, gr))

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
