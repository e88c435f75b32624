r"""K2s / the signal mode of K2b at the coil capacities 2, 4, 8: ``fused.signal_rfgr`` with a receive array -- every coil from
one launch per block of ``mrphy_signal_rfgr_max_rx`` coils.  The forward against the one-coil launches (capacity 1 of the
same kernel: bit for bit) and the fp64 reduction of the trajectory's own records; the number of launches; gradients
against the composed route, the oracle and the sum of the one-coil calls' gradients; more tiles than persistent waves; the
C ABI called directly, also with one coil; empty problems; hipGraph capture; where the tile is flushed, at every capacity."""
import collections
import contextlib

import pytest

from gpu_common import *  # noqa: F401,F403
from mrphy_amd import _host, _lib as L, beffective
from mrphy_amd.fused import _forward_prep, _signal_composed, _signal_of, _traj_ends
from test_fused_traj import _problem, _kw, _weights
from test_signal import _sig64, _grad_run, _check_grads, NAMES

pytestmark = pytest.mark.gpu

N, NM = 2, 100
ENTRY = ('mrphy_signal_rfgr_mrx_fwd', 'mrphy_signal_rfgr_mrx_bwd', 'mrphy_signal_rfgr_fwd', 'mrphy_signal_rfgr_bwd')


def _cap(tag):
    return int(mrphy_amd.require_library().mrphy_signal_rfgr_max_rx(L.F64 if tag == 'f64' else L.F32))


def _rxn(tag, nRx, nM=NM, n=N, seed=91):
    r"""``rx = rnd(N, nM, 2, nRx)·2 − 1`` (CPU), ``test_signal._rx``'s recipe for any coil count."""
    gen = torch.Generator().manual_seed(seed)
    return (torch.rand((n, nM, 2, nRx), generator=gen, dtype=torch.float64) * 2 - 1).to(DT[tag])


def _mode(tag_mode):
    tag, _, mode = tag_mode.partition('-')
    return tag, (mrphy_amd.precision(mode) if mode else contextlib.nullcontext())


# =============================================================================================
# 1. forward == the one-coil launches
# =============================================================================================
@pytest.mark.parametrize('tag_mode', ['f64', 'f32-precise', 'f32-fast'])
@pytest.mark.parametrize('variant', ['plain', 'b1map', 'norelax'])
@pytest.mark.parametrize('nT', [48, 50, 7])
def test_signal_mrx_forward_is_the_one_coil_launches(tag_mode, variant, nT):
    r"""nRx = 2, 3, 5, max_rx, max_rx + 1 (pad coils; the block boundary) x every = 1, 3, 16, 40, nT + 5, under no_grad
    with inputs that require grad: ``sig[..., c]`` and ``Mo`` are the bits of ``signal_rfgr(rx=rx[..., c])``, ``Mo``
    those of ``blochsim_rfgr``; twice the same bits.  Each coil is also held to test_signal_forward's gates against
    S64, the fp64 reduction of the trajectory kernel's own records: assert_close, and in fp32 the elementwise
    (nM + 3) 2^-24 Σ|terms| bound -- implied by the bit equality, asserted so that a failure says which side moved.
    At nT = 48 (whole segments: the checkpoint-writing builds) the same with grad mode on."""
    tag, mode = _mode(tag_mode)
    cap = _cap(tag)
    P = _problem(tag, variant, nT)
    rx = _rxn(tag, cap + 1)
    kw = _kw(P, dev)
    loc = dev(P['loc'])
    Mi, rf, gr = (dev(P[k]).requires_grad_(True) for k in ('M0', 'rf', 'gr'))
    with mode:
        with torch.no_grad():
            Mo_ref = fused.blochsim_rfgr(Mi, rf, gr, loc, **kw)
        for every in (1, 3, 16, 40, nT + 5):
            nRec = len(_traj_ends(nT, every))
            with torch.no_grad():
                one = [fused.signal_rfgr(Mi, rf, gr, loc, every=every, rx=dev(rx[..., c]), return_Mo=True, **kw)
                       for c in range(cap + 1)]
                Mt = fused.blochsim_rfgr_traj(Mi, rf, gr, loc, every=every, **kw)
            for c in range(cap + 1):
                assert torch.equal(one[c][1], Mo_ref)
                S64, A64 = _sig64(Mt, rx[..., c])
                assert_close(one[c][0], S64, tag, f'one-coil sig vs S64 (every={every}, coil {c})')
                if tag == 'f32':
                    ratio = float(((one[c][0].double().cpu() - S64).abs() / ((NM + 3) * 2.0 ** -24 * A64)).max())
                    assert ratio <= 1.0, (every, c, ratio)
            for nRx in (2, 3, 5, cap, cap + 1):
                r = dev(rx[..., :nRx])
                with torch.no_grad():
                    sig, Mo = fused.signal_rfgr(Mi, rf, gr, loc, every=every, rx=r, return_Mo=True, **kw)
                    again = fused.signal_rfgr(Mi, rf, gr, loc, every=every, rx=r, **kw)
                assert sig.shape == (N, 2, nRec, nRx) and sig.dtype == DT[tag] and not sig.requires_grad
                assert torch.equal(Mo, Mo_ref), (every, nRx, 'Mo')
                assert torch.equal(sig, again), (every, nRx, 'twice the same bits')
                for c in range(nRx):
                    S64, A64 = _sig64(Mt, rx[..., c])
                    assert_close(sig[..., c], S64, tag, f'sig vs S64 (every={every}, nRx={nRx}, coil {c})')
                    if tag == 'f32':
                        ratio = float(((sig[..., c].double().cpu() - S64).abs() / ((NM + 3) * 2.0 ** -24 * A64)).max())
                        assert ratio <= 1.0, (every, nRx, c, ratio)
                    assert torch.equal(sig[..., c], one[c][0]), (every, nRx, c, 'sig vs the one-coil launch')
            if nT % 16 == 0:                         # grad mode on: the builds that write checkpoints
                for nRx in (3, cap + 1):
                    sig, Mo = fused.signal_rfgr(Mi, rf, gr, loc, every=every, rx=dev(rx[..., :nRx]), return_Mo=True, **kw)
                    assert sig.requires_grad and torch.equal(Mo, Mo_ref)
                    for c in range(nRx):
                        assert torch.equal(sig[..., c], one[c][0]), (every, nRx, c, 'with checkpoints')


# =============================================================================================
# 2. one launch per block of coils
# =============================================================================================
def _counted(monkeypatch):
    lib = mrphy_amd.require_library()
    calls = collections.Counter()

    def wrap(name, fn):
        def counted(*a):
            calls[name] += 1
            return fn(*a)
        return counted
    for name in ENTRY:
        monkeypatch.setattr(lib, name, wrap(name, getattr(lib, name)))
    return calls


def test_signal_mrx_is_one_launch_per_block(monkeypatch):
    r"""Forward + backward: 3 coils call the multi-coil entry points once each and the one-coil ones not at all;
    max_rx + 1 coils twice each; an rx without a coil axis (or with one of length 1) the one-coil entry points, as before."""
    tag = 'f32'
    cap = _cap(tag)
    P = _problem(tag, 'b1map', 48)
    calls = _counted(monkeypatch)
    for nRx, want in ((3, (1, 1, 0, 0)), (cap, (1, 1, 0, 0)), (cap + 1, (2, 2, 0, 0)), (1, (0, 0, 1, 1)), (0, (0, 0, 1, 1))):
        rx = _rxn(tag, max(nRx, 1))
        calls.clear()
        _grad_run('signal', P, rx[..., 0] if nRx == 0 else rx, 5, dev)
        assert tuple(calls[k] for k in ENTRY) == want, (nRx, dict(calls))


# =============================================================================================
# 3. gradients
# =============================================================================================
def _vs_one_coil_sum(P, rx, every, tag):
    r"""Loss (sig·w).sum() + (Mo·v).sum(): the gradients against the sum of the one-coil calls' gradients, coil c with
    the weights w[..., c] (and the Mo term once) -- another association of the same sum, hence assert_close."""
    got = _grad_run('signal', P, rx, every, dev)
    nRx = rx.shape[-1]
    w = dev(_weights(tuple(got[0].shape), got[0].dtype))
    v = dev(_weights(tuple(got[1].shape), got[1].dtype))
    kw = _kw(P, dev)
    Mi, r, g = (dev(x).clone().requires_grad_(True) for x in (P['M0'], P['rf'], P['gr']))
    for c in range(nRx):
        sig, Mo = fused.signal_rfgr(Mi, r, g, dev(P['loc']), every=every, rx=dev(rx[..., c]), return_Mo=True, **kw)
        if P['gr'].shape[2] % 16 == 0:            # (a composed tail sums the coils' records in torch: not the kernels' bits)
            assert torch.equal(sig, got[0][..., c])
        else:
            assert_close(sig, got[0][..., c], tag, f'sig of coil {c} (every={every}, nRx={nRx})')
        ((sig * w[..., c]).sum() + ((Mo * v).sum() if c == 0 else 0)).backward()
    for a, b, nm in zip(got[2:], (Mi.grad, r.grad, g.grad), NAMES[2:]):
        assert_close(a, b, tag, f'{nm} vs the sum of the one-coil gradients (every={every}, nRx={nRx})')


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('nT,every', [(48, 1), (48, 3), (48, 16), (48, 40), (50, 3), (16, 1), (16, 21)])
def test_signal_mrx_gradients(tag, nT, every):
    r"""nRx = 2, 3, max_rx.  test_signal._check_grads on the multi-coil rx: loss (sig·w).sum() + (Mo·v).sum() and each
    term alone -- grad_Mi, grad_rf, grad_gr == autograd through the composed route == the oracle at assert_close's
    gates; twice the same bits; with the Mo term alone and whole segments, blochsim_rfgr's bits.  And against the sum of
    the one-coil calls' gradients.  nT = 50: the fused part + composed tail; nT = 16: one checkpoint segment."""
    cap = _cap(tag)
    P = _problem(tag, 'b1map', nT)
    rx = _rxn(tag, cap)
    for nRx in (2, 3, cap):
        _check_grads(P, rx[..., :nRx], every, tag, with_oracle=True)
        _vs_one_coil_sum(P, rx[..., :nRx], every, tag)


@pytest.mark.parametrize('mode,wide', [('fast', False), ('fast', True), ('precise', False), ('precise', True)])
@pytest.mark.parametrize('every', [1, 5, 16, 40])
def test_signal_mrx_gradients_dtype_codes(mode, wide, every):
    r"""test_signal_gradients_dtype_codes with 3 receive coils: fp32 data through dtype codes 0 / 2 and 3 / 4 (precise:
    the adjoint carries t = E h, so the coils' summed cotangent must enter scaled by E, once), with relaxation, against
    the composed route in the same mode; code 3 is also held to the oracle."""
    P = _problem('f32', 'plain', 48, seed=5)
    if wide:                                          # fp64 constants with fp32 data: codes 2 / 4
        P['T1'], P['T2'], P['γ'], P['dt'] = (P[k].double() for k in ('T1', 'T2', 'γ', 'dt'))
    rx = _rxn('f32', 3)
    with mrphy_amd.precision(mode):
        code = _host.dtype_code(torch.float32, torch.float64 if wide else torch.float32)
        assert code == {('fast', False): 0, ('fast', True): 2, ('precise', False): 3, ('precise', True): 4}[mode, wide]
        if mode == 'precise' and not wide:
            with mrphy_amd.constants_on('cpu'):
                _check_grads(P, rx, every, 'f32', with_oracle=True)
        else:
            _check_grads(P, rx, every, 'f32', with_oracle=False)
        _vs_one_coil_sum(P, rx, every, 'f32')


# =============================================================================================
# 4. more than one tile per wave: the workspace's read-modify-write path at 2 nRx rows
# =============================================================================================
@pytest.mark.parametrize('every', [1, 16])
def test_signal_mrx_second_tile_per_wave(every):
    r"""N = 1, nT = 32, fp32, 2 coils.  nM = 4096·64 + 100: more spin tiles than the forward has persistent waves, so a
    wave adds its later tiles into its workspace rows -- the one-coil launches' bits.  nM = 2048·64 + 100: the same for
    the adjoint -- assert_close to the composed route."""
    nT = 32
    nM = 4096 * 64 + 100
    P = _problem('f32', 'plain', nT, N=1, nM=nM)
    rx = _rxn('f32', 2, nM=nM, n=1)
    args = (dev(P['M0']), dev(P['rf']), dev(P['gr']), dev(P['loc']))
    with torch.no_grad():
        sig, Mo = fused.signal_rfgr(*args, every=every, rx=dev(rx), return_Mo=True, **_kw(P, dev))
        for c in range(2):
            one, Mo1 = fused.signal_rfgr(*args, every=every, rx=dev(rx[..., c]), return_Mo=True, **_kw(P, dev))
            assert torch.equal(sig[..., c], one) and torch.equal(Mo, Mo1), c
    assert sig.shape == (1, 2, nT // every, 2)
    nM = 2048 * 64 + 100
    P = _problem('f32', 'plain', nT, N=1, nM=nM)
    rx = _rxn('f32', 2, nM=nM, n=1)
    got = _grad_run('signal', P, rx, every, dev)
    for a, b, nm in zip(got, _grad_run('composed', P, rx, every, dev), NAMES):
        assert_close(a, b, 'f32', f'{nm} vs composed route (every={every})')
    for a, b, nm in zip(got, _grad_run('signal', P, rx, every, dev), NAMES):
        assert torch.equal(a, b), nm


# =============================================================================================
# 5. the C ABI, called directly
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_signal_mrx_direct_abi_call(tag):
    r"""mrphy_signal_rfgr_mrx_fwd / _mrx_bwd through ctypes on device buffers of this test's own (N = 1, nM = 100,
    nT = 16, 2 coils, every = 3): both return 0 and give the Python route's sig, Mo and gradients, bit for bit."""
    from mrphy_amd import sims
    lib = mrphy_amd.require_library()
    n, nT, nRx, every = 1, 16, 2, 3
    P = _problem(tag, 'b1map', nT, N=n)
    rx = _rxn(tag, nRx, n=n)
    sig_py, Mo_py, gMi_py, grf_py, ggr_py = _grad_run('signal', P, rx, every, dev)
    dt_ = DT[tag]
    kw = _kw(P, dev)
    p = beffective._PulseOnSpins(dev(P['rf']), dev(P['gr']), dev(P['loc']), kw['Δf'], kw['b1Map'], kw['γ_beff'])
    cs = sims.relax_constants(kw['T1'], kw['T2'], kw['γ'], kw['dt'], 4, DEV)
    code, alive, consts, Mck, ckpt = _forward_prep(lib, p, *cs, dt_, DEV, True)
    assert code == _host.dtype_code(dt_, dt_)
    nRec = len(_traj_ends(nT, every))
    new = lambda *s: torch.full(s, float('nan'), dtype=dt_, device=DEV)  # noqa: E731
    Mi, rxd = dev(P['M0']).contiguous(), dev(rx).contiguous()
    sig, Mo = new(n, 2, nRec, nRx), new(n, NM, 3)
    nb = lib.mrphy_signal_rfgr_mrx_fwd_workspace(code, n, NM, nT, every, nRx)
    assert nb == 2 * n * 2 * nRx * nRec * sig.element_size()
    work = torch.empty(nb, dtype=torch.uint8, device=DEV)
    st = _host.current_stream(DEV)
    rc = lib.mrphy_signal_rfgr_mrx_fwd(code, Mi.data_ptr(), *p.k0_args(), *consts, rxd.data_ptr(), nRx, Mo.data_ptr(),
                                       *ckpt, sig.data_ptr(), every, work.data_ptr(), nb, n, NM, nT, 1, st)
    assert rc == 0
    assert torch.equal(sig, sig_py) and torch.equal(Mo, Mo_py)
    w, v = dev(_weights(tuple(sig.shape), dt_)), dev(_weights(tuple(Mo.shape), dt_))
    gMi, grf, ggr = new(n, NM, 3), new(n, 2, nT, 1), new(n, 3, nT)
    nb = lib.mrphy_blochsim_rfgr_bwd_workspace(code, n, NM, nT)
    work = torch.empty(nb, dtype=torch.uint8, device=DEV)
    rc = lib.mrphy_signal_rfgr_mrx_bwd(code, Mck.data_ptr(), *p.k0_args(), *consts, rxd.data_ptr(), nRx, v.data_ptr(),
                                       w.data_ptr(), every, gMi.data_ptr(), grf.data_ptr(), ggr.data_ptr(),
                                       work.data_ptr(), nb, n, NM, nT, st)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(gMi, gMi_py) and torch.equal(grf[..., 0], grf_py) and torch.equal(ggr, ggr_py)
    del alive


# =============================================================================================
# 6. empty problems
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('empty', ['nT', 'nM'])
def test_signal_mrx_empty_problem(tag, empty):
    r"""test_signal_empty_problem with a coil axis of 3: ``sig`` is `(N, 2, 0, 3)`, or zeros `(N, 2, nRec, 3)` without
    spins; ``Mo`` is ``Mi``; the backward runs -- ``grad_Mi`` is the cotangent of ``Mo``, the pulse gradients are zeros."""
    nT, nM, every = (0, NM, 3) if empty == 'nT' else (32, 0, 5)
    P = _problem(tag, 'plain', 32, nM=nM)
    P['rf'], P['gr'] = P['rf'][:, :, :nT], P['gr'][:, :, :nT]
    rx = _rxn(tag, 3, nM=nM)
    Mi, rf, gr = (dev(P[k]).clone().requires_grad_(True) for k in ('M0', 'rf', 'gr'))
    sig, Mo = fused.signal_rfgr(Mi, rf, gr, dev(P['loc']), every=every, rx=dev(rx), return_Mo=True, **_kw(P, dev))
    nRec = len(_traj_ends(nT, every))
    assert sig.shape == (N, 2, nRec, 3) and sig.dtype == DT[tag] and Mo.shape == Mi.shape
    assert nRec == (0 if empty == 'nT' else 7)
    assert bool((sig == 0).all()) and torch.equal(Mo, Mi.detach())
    v = dev(_weights(tuple(Mo.shape), Mo.dtype))
    ((sig * dev(_weights(tuple(sig.shape), sig.dtype))).sum() + (Mo * v).sum()).backward()
    assert Mi.grad.shape == Mi.shape and torch.equal(Mi.grad, v)
    for g, x in ((rf.grad, rf), (gr.grad, gr)):
        assert g is not None and g.shape == x.shape and g.dtype == x.dtype and bool((g == 0).all())


# =============================================================================================
# 7. hipGraph capture
# =============================================================================================
def test_signal_mrx_hipgraph_capture():
    r"""One design iteration with 3 receive coils (signal_rfgr, the loss, backward) at 16^3 x 256 captured into a HIP
    graph as test_signal_hipgraph_capture does and replayed once: the eager bits."""
    n, nT, every = 16, 256, 16
    sp = synth.cube_spins(n, device=DEV)
    p = synth.pulse(nT, device=DEV)
    rf = (0.05 * p['rf']).clone().requires_grad_(True)
    gr = p['gr'].clone().requires_grad_(True)
    rx = dev(_rxn('f32', 3, nM=n ** 3, n=1)).reshape(sp['M0'].shape[:-1] + (2, 3))

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


# =============================================================================================
# 8. the `_mrx_` entry points with one coil: capacity 1, the one-coil entry points' bits
# =============================================================================================
@pytest.mark.parametrize('tag_mode', ['f64', 'f32-precise', 'f32-fast'])
def test_signal_mrx_entry_points_with_one_coil_are_the_one_coil_entry_points(tag_mode):
    r"""mrphy_signal_rfgr_mrx_fwd / _mrx_bwd at nRx = 1 against mrphy_signal_rfgr_fwd / _bwd through ctypes on the same
    device buffers (N = 1, nM = 100: a tail tile with masked lanes, nT = 48, every = 1, 3, 16, with checkpoints): all
    return 0, and ``sig``, ``Mo``, the checkpoints, ``grad_Mi``, ``grad_rf`` and ``grad_gr`` are the same bits.  Outputs
    start as NaN, so an element left unwritten fails the comparison."""
    from mrphy_amd import sims
    tag, mode = _mode(tag_mode)
    lib = mrphy_amd.require_library()
    n, nT, dt_ = 1, 48, DT[tag]
    P = _problem(tag, 'b1map', nT, N=n)
    rxd = dev(_rxn(tag, 1, n=n)).contiguous()              # (1, nM, 2, 1): the memory of a one-coil (1, nM, 2)
    kw = _kw(P, dev)
    new = lambda *s: torch.full(s, float('nan'), dtype=dt_, device=DEV)  # noqa: E731
    with mode:
        p = beffective._PulseOnSpins(dev(P['rf']), dev(P['gr']), dev(P['loc']), kw['Δf'], kw['b1Map'], kw['γ_beff'])
        cs = sims.relax_constants(kw['T1'], kw['T2'], kw['γ'], kw['dt'], 4, DEV)
        code, alive, consts, Mck, (_, ck) = _forward_prep(lib, p, *cs, dt_, DEV, True)
    Mi = dev(P['M0']).contiguous()
    st = _host.current_stream(DEV)
    nbb = lib.mrphy_blochsim_rfgr_bwd_workspace(code, n, NM, nT)
    for every in (1, 3, 16):
        nRec = len(_traj_ends(nT, every))
        nb = lib.mrphy_signal_rfgr_fwd_workspace(code, n, NM, nT, every)
        assert nb == lib.mrphy_signal_rfgr_mrx_fwd_workspace(code, n, NM, nT, every, 1)
        w, v = dev(_weights((n, 2, nRec), dt_)), dev(_weights((n, NM, 3), dt_))
        got = []
        for mrx in ((), (1,)):
            sig, Mo, Mck_ = new(n, 2, nRec, *mrx), new(n, NM, 3), torch.full_like(Mck, float('nan'))
            work = torch.empty(nb, dtype=torch.uint8, device=DEV)
            fwd = lib.mrphy_signal_rfgr_mrx_fwd if mrx else lib.mrphy_signal_rfgr_fwd
            rc = fwd(code, Mi.data_ptr(), *p.k0_args(), *consts, rxd.data_ptr(), *mrx, Mo.data_ptr(), Mck_.data_ptr(),
                     ck, sig.data_ptr(), every, work.data_ptr(), nb, n, NM, nT, 1, st)
            assert rc == 0, (every, mrx)
            gMi, grf, ggr = new(n, NM, 3), new(n, 2, nT, 1), new(n, 3, nT)
            work = torch.empty(nbb, dtype=torch.uint8, device=DEV)
            bwd = lib.mrphy_signal_rfgr_mrx_bwd if mrx else lib.mrphy_signal_rfgr_bwd
            rc = bwd(code, Mck_.data_ptr(), *p.k0_args(), *consts, rxd.data_ptr(), *mrx, v.data_ptr(), w.data_ptr(), every,
                     gMi.data_ptr(), grf.data_ptr(), ggr.data_ptr(), work.data_ptr(), nbb, n, NM, nT, st)
            assert rc == 0, (every, mrx)
            torch.cuda.synchronize()
            got.append((sig.reshape(n, 2, nRec), Mo, Mck_, gMi, grf, ggr))
        for a, b, nm in zip(*got, ('sig', 'Mo', 'Mck', 'grad_Mi', 'grad_rf', 'grad_gr')):
            assert torch.equal(a, b), (every, nm)
    del alive


# =============================================================================================
# 9. where the tile is flushed, at every capacity
# =============================================================================================
@pytest.mark.parametrize('tag_mode', ['f64', 'f32-precise', 'f32-fast'])
@pytest.mark.parametrize('nT', [40, 35])
def test_signal_flush_rule_at_every_capacity(tag_mode, nT):
    r"""N = 1, nM = 64 + 36, nRx = 1, 2, 3, 8 (the capacities 1, 2, 4, 8) x every = 1, 2, 5, 16, 17, forward only: at the
    small strides a tile of 16 / R records fills and is flushed during the pulse, before a step batch or inside it
    according to the capacity and the data type; nT = 35 adds the nT % 8 (fp64: nT % 4) tail loop.  ``sig[..., c]`` is the
    bits of the one-coil call for coil ``c``, and is held to ``_signal_of`` of ``blochsim_rfgr_traj``'s records (formed
    in fp64) at test_signal_forward's gates: assert_close and, in fp32, the elementwise (nM + 3) 2^-24 Σ|terms| bound."""
    tag, mode = _mode(tag_mode)
    n = 1
    P = _problem(tag, 'b1map', nT, N=n)
    rx = _rxn(tag, 8, n=n)
    kw = _kw(P, dev)
    args = (dev(P['M0']), dev(P['rf']), dev(P['gr']), dev(P['loc']))
    with mode, torch.no_grad():
        for every in (1, 2, 5, 16, 17):
            nRec = len(_traj_ends(nT, every))
            Mt = fused.blochsim_rfgr_traj(*args, every=every, **kw)
            ref = _signal_of(Mt.movedim(-2, 0).double(), dev(rx).double()).cpu()       # (1, 2, nRec, 8), fp64
            A64 = torch.stack([_sig64(Mt, rx[..., c])[1] for c in range(8)], dim=-1)
            one = [fused.signal_rfgr(*args, every=every, rx=dev(rx[..., c]), **kw) for c in range(8)]
            for nRx in (1, 2, 3, 8):
                sig = fused.signal_rfgr(*args, every=every, rx=dev(rx[..., :nRx]), **kw)
                assert sig.shape == (n, 2, nRec, nRx), (every, nRx)
                for c in range(nRx):
                    assert torch.equal(sig[..., c], one[c]), (every, nRx, c, 'sig vs the one-coil call')
                    assert_close(sig[..., c], ref[..., c], tag, f'sig vs _signal_of (every={every}, nRx={nRx}, coil {c})')
                if tag == 'f32':                     # the worst element of the nRx coils, as a fraction of its bound
                    ratio = float(((sig.double().cpu() - ref[..., :nRx]).abs()
                                   / ((NM + 3) * 2.0 ** -24 * A64[..., :nRx])).max())
                    record(f'signal.flush.{tag_mode}.nT{nT}.every{every}.nRx{nRx}.elementwise_over_bound', ratio, 1.0)
                    assert ratio <= 1.0, (every, nRx, ratio)
