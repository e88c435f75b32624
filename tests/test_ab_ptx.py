r"""``fused.ab_rfgr`` under parallel transmit on the device: Hargreaves' ``A, B`` of a pulse on 2 .. 8 transmit coils with
their ``b1Map`` (K2ab-mc) and the fused adjoint w.r.t. ``rf`` `(N ⊻ 1, xy, nT, nCoils)` and ``gr`` (K2abb-mc).

The forward is held bit for bit to the materialised route ``beffective.beff2ab(rfgr2beff(.))`` on the same step constants
and to ``blochsim_rfgr(Mi = 0)``; gradients at the project's gates (``util.assert_close``: fp64 max-abs 1e-9, fp32 relative
L2 1e-5) to autograd through the materialised route on the device and to the CPU oracle in fp64.  Shapes: N = 2, nM = 100
(one full wave and a ragged one with 36 valid lanes) unless a test says otherwise; 4 and 8 coils are
``test_fused_traj._problem``'s ``ptx4`` / ``ptx8``, 2, 3, 5 and 9 coils are drawn the same way (3 and 5 leave coils of the
capacity 4 / 8 builds zero-padded).  Coil counts above a data type's ``mrphy_ab_rfgr_mc_max_coils`` compose, and must
pass the same assertions."""
import functools

import pytest

from gpu_common import *  # noqa: F401,F403
from mrphy_amd import _host
from mrphy_amd.fused import _forward_prep
from test_ab_rfgr import (COMPOSED, LOSSES, _counted, _factors, _fused, _grads, _materialised, _mode, _tail, _weights,
                          _widened)
from test_fused_traj import _problem

pytestmark = pytest.mark.gpu

MODES = ['f64', 'f32-precise', 'f32-fast']
FWD, BWD = 'mrphy_ab_rfgr_fwd', 'mrphy_ab_rfgr_bwd'
FWD_MC, BWD_MC = 'mrphy_ab_rfgr_mc_fwd', 'mrphy_ab_rfgr_mc_bwd'
COUNTED = (FWD, BWD, FWD_MC, BWD_MC) + COMPOSED
WAVE = 64


def _ptx(tag, nC, nT, N=2, nM=100, batch1=False, relax=True):
    r"""The operands of ``test_fused_traj._problem`` with ``nC`` transmit coils: its own ``ptx4`` / ``ptx8``, other counts
    (and a batch-1 pulse) drawn by its recipe from a generator of their own."""
    if nC in (4, 8) and not batch1:
        P = _problem(tag, f'ptx{nC}', nT, N=N, nM=nM)
    else:
        P = _problem(tag, 'plain_batch1_pulse' if batch1 else 'plain', nT, N=N, nM=nM)
        gen = torch.Generator().manual_seed(977 + 10 * nC + nT)
        rnd = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64)  # noqa: E731
        P['rf'] = ((rnd(1 if batch1 else N, 2, nT, nC) * 2 - 1) * 1.5).to(DT[tag])
        P['b1'] = ((rnd(N, nM, 2, nC) * 2 - 1) * 0.7).to(DT[tag])
    if not relax:
        P['T1'] = P['T2'] = None
    return P


def _cap(tag):
    lib = mrphy_amd.require_library()
    return int(lib.mrphy_ab_rfgr_mc_max_coils(_host.dtype_code(DT[tag], DT[tag])))


def _consts(P):
    r"""``beff2ab``'s own four step constants, formed on the device by its expressions (``test_ab_rfgr``, test 5)."""
    from math import pi as π
    E1, E2 = (dev(x) for x in _factors(P))
    γ, dt = dev(P['γ']), dev(P['dt'])
    pad = lambda x: _host.pad_trailing(x, 2)  # noqa: E731
    return E1, E2, dict(γ2πdt=2 * π * pad(γ) * pad(dt), E1=pad(E1), E2=pad(E2), E1_1=pad(E1) - 1)


# =============================================================================================
# 1. forward bits
# =============================================================================================
@pytest.mark.parametrize('tag_mode', MODES)
@pytest.mark.parametrize('nC', [2, 3, 4, 5, 8])
@pytest.mark.parametrize('nT', [48, 50, 7])
def test_forward_bits(tag_mode, nC, nT, monkeypatch):
    r"""``A, B`` == ``beff2ab(rfgr2beff(.))`` on the same four constants, ``B`` == ``blochsim_rfgr(Mi = 0)``, with and
    without relaxation; one ``_mc_fwd`` per call up to the data type's capacity, the composed kernels above it; at
    nT = 48 a pulse gradient leaves ``A, B`` unchanged."""
    tag, mode = _mode(tag_mode)
    calls = _counted(monkeypatch, COUNTED)
    for relax in (True, False):
        P = _ptx(tag, nC, nT, relax=relax)
        E1, E2, consts = _consts(P)
        rf, gr, loc = dev(P['rf']), dev(P['gr']), dev(P['loc'])
        kw = dict(Δf=dev(P['df']), b1Map=dev(P['b1']), γ_beff=dev(P['γ']), T1=dev(P['T1']), T2=dev(P['T2']),
                  γ=dev(P['γ']), dt=dev(P['dt']))
        with mode, torch.no_grad():
            beff = beffective.rfgr2beff(rf, gr, loc, Δf=kw['Δf'], b1Map=kw['b1Map'], γ=kw['γ_beff'])
            A0, B0 = beffective.beff2ab(beff, E1=E1, E2=E2, γ=kw['γ'], dt=kw['dt'])
            calls.clear()
            A, B = _fused(P, rf, gr, T1=None, T2=None, consts=consts)
            n = dict(calls)
            Ap, Bp = fused.ab_rfgr(rf, gr, loc, **kw)
            Mo = fused.blochsim_rfgr(torch.zeros((2, 100, 3), dtype=DT[tag], device=DEV), rf, gr, loc, **kw)
        if nC <= _cap(tag):
            assert n == {FWD_MC: 1}, (relax, n)
        else:
            assert not n.get(FWD_MC) and not n.get(FWD) and n.get('mrphy_rfgr2beff_st') == 1, (relax, n)
        assert A.shape == (2, 100, 3, 3) and B.shape == (2, 100, 3) and A.dtype == B.dtype == DT[tag]
        assert torch.equal(A, A0) and torch.equal(B, B0), relax
        assert torch.equal(Bp, Mo), relax
        if relax:
            assert float(Bp.abs().max()) > 0
        else:
            assert torch.equal(B, torch.zeros_like(B))
        if nT == 48:
            with mode:
                Ag, Bg = fused.ab_rfgr(rf.clone().requires_grad_(True), gr.clone().requires_grad_(True), loc, **kw)
            assert torch.equal(Ag.detach(), Ap) and torch.equal(Bg.detach(), Bp), relax


# =============================================================================================
# 2. routes by call count
# =============================================================================================
ROUTE_CASES = ['fused', 'split', 'short', '9 coils', 'loc gradient', 'no b1Map']


@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('case', ROUTE_CASES)
def test_routes_by_call_count(tag, case, monkeypatch):
    r"""4 coils, nT = 48, pulse gradients: exactly one ``_mc_fwd`` and one ``_mc_bwd``, nothing composed; nT = 50: the split;
    nT = 7, 9 coils, a ``loc`` gradient, multi-coil ``rf`` without ``b1Map``: composed.  The one-coil entry points are never
    called."""
    nT = {'split': 50, 'short': 7}.get(case, 48)
    P = _ptx(tag, 9 if case == '9 coils' else 4, nT)
    calls = _counted(monkeypatch, COUNTED)
    rf, gr = dev(P['rf']).requires_grad_(True), dev(P['gr']).requires_grad_(True)
    loc = dev(P['loc']).requires_grad_(case == 'loc gradient')
    kw = dict(Δf=dev(P['df']), b1Map=None if case == 'no b1Map' else dev(P['b1']), γ_beff=dev(P['γ']), T1=dev(P['T1']),
              T2=dev(P['T2']), γ=dev(P['γ']), dt=dev(P['dt']))
    A, B = fused.ab_rfgr(rf, gr, loc, **kw)
    wA, wB = (dev(x) for x in _weights(2, 100, DT[tag]))
    ((A * wA).sum() + (B * wB).sum()).backward()
    n = {k: v for k, v in calls.items() if v}
    assert not n.get(FWD) and not n.get(BWD), n
    assert rf.grad.shape == P['rf'].shape and gr.grad.shape == P['gr'].shape
    if case == 'fused':
        assert n == {FWD_MC: 1, BWD_MC: 1}, n
    elif case == 'split':
        assert n.get(FWD_MC) == 1 and n.get(BWD_MC) == 1 and n.get('mrphy_beff2ab_save') == 1, n
    else:
        assert not n.get(FWD_MC) and not n.get(BWD_MC) and n.get('mrphy_beff2ab_save') == 1, n


# =============================================================================================
# 3. gradients
# =============================================================================================
GRAD_CASES = [(4, 48, False), (4, 16, False), (4, 50, False), (2, 48, False), (3, 48, False), (5, 48, False),
              (8, 48, False), (4, 48, True)]


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag_mode', MODES)
@pytest.mark.parametrize('nC,nT,batch1', GRAD_CASES, ids=[f'c{c}-nT{t_}' + ('-batch1' if b else '') for c, t_, b in GRAD_CASES])
def test_gradients(tag_mode, nC, nT, batch1, monkeypatch):
    r"""``grad_rf`` per coil and ``grad_gr`` of the six losses of ``test_ab_rfgr.LOSSES`` (a cotangent sent to the wrong
    column or coil differs by O(1)) against autograd through ``rfgr2beff`` -> ``beff2ab`` on the device and the oracle's
    autograd in fp64; the shapes of ``rf`` and ``gr`` (a batch-1 pulse gets the sum over N); a second run gives the same
    bits.  nT = 16 is one segment: nothing is fetched ahead."""
    tag, mode = _mode(tag_mode)
    P = _ptx(tag, nC, nT, batch1=batch1)
    calls = _counted(monkeypatch, COUNTED)
    for which in LOSSES:
        wA, wB = _weights(2, 100, DT[tag], which)
        with mode:
            calls.clear()
            fu = _grads(_fused, P, dev, wA, wB)
            n = {k: v for k, v in calls.items() if v}
            again = _grads(_fused, P, dev, wA, wB)
            mat = _grads(lambda P_, rf, gr: _materialised(P_, dev, rf, gr), P, dev, wA, wB)
        ora = _grads(lambda P_, rf, gr: _materialised(P_, lambda x: x, rf, gr), _widened(P), lambda x: x,
                     wA.double(), wB.double())
        if nC > _cap(tag):
            assert not n.get(FWD_MC) and not n.get(BWD_MC) and n.get('mrphy_beff2ab_save') == 1, (which, n)
        elif nT % 16 == 0:
            assert n == {FWD_MC: 1, BWD_MC: 1}, (which, n)
        else:
            assert n.get(FWD_MC) == 1 and n.get(BWD_MC) == 1 and n.get('mrphy_beff2ab_save') == 1, (which, n)
        assert fu['grad_rf'].shape == P['rf'].shape == (1 if batch1 else 2, 2, nT, nC)
        assert fu['grad_gr'].shape == P['gr'].shape
        for k in fu:
            assert bool(torch.isfinite(fu[k]).all()), (which, k)
            assert torch.equal(fu[k], again[k]), (which, k, 'second run')
            assert_close(fu[k], mat[k], tag, f'{which}: {k} vs the materialised route')
            assert_close(fu[k], ora[k], tag, f'{which}: {k} vs the fp64 oracle')
        for c in range(nC):
            assert_close(fu['grad_rf'][..., c], mat['grad_rf'][..., c], tag, f'{which}: grad_rf of coil {c} vs materialised')
            assert_close(fu['grad_rf'][..., c], ora['grad_rf'][..., c], tag, f'{which}: grad_rf of coil {c} vs the oracle')
            if which != 'B':
                assert float(fu['grad_rf'][..., c].abs().max()) > 0, (which, c)


# =============================================================================================
# 4. more tiles than persistent waves
# =============================================================================================
NT_TILES = 32


@functools.lru_cache(maxsize=None)
def _tiles_shape(tag):
    r"""``(P, nM)``: the cap on the adjoint's persistent waves, from the parallel-transmit workspace query (11 rows per
    wave at 4 coils), and nM = P 64 + 100."""
    lib = mrphy_amd.require_library()
    code = _host.dtype_code(DT[tag], DT[tag])
    waves = lambda nM: int(lib.mrphy_ab_rfgr_mc_bwd_workspace(code, 2, nM, NT_TILES, 4)) // (  # noqa: E731
        2 * 11 * NT_TILES * DT[tag].itemsize)
    P = waves(1 << 30)
    nM = P * WAVE + 100
    assert waves(nM) == P and -(-nM // WAVE) == P + 2
    return P, nM


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag_mode', MODES)
def test_more_tiles_than_persistent_waves(tag_mode):
    r"""The scheme of ``test_ab_rfgr.test_more_tiles_than_persistent_waves`` with 4 coils: waves 0 and 1 take a second
    tile, the second of them ragged.  FULL weights against the materialised route on the device, TAIL-ONLY weights (zero
    cotangent on every spin of the tiles ``< P``) against the fp64 oracle on the last 136 spins alone; twice the same
    bits."""
    tag, mode = _mode(tag_mode)
    P, nM = _tiles_shape(tag)
    Q = _ptx(tag, 4, NT_TILES, N=2, nM=nM)
    wA, wB = _weights(2, nM, DT[tag])
    mask = torch.ones(nM, dtype=DT[tag])
    mask[:P * WAVE] = 0
    tA, tB = wA * mask[None, :, None, None], wB * mask[None, :, None]
    Q64 = _tail(_widened(Q), nM)
    ora = _grads(lambda P_, rf, gr: _materialised(P_, lambda x: x, rf, gr), Q64, lambda x: x,
                 tA[:, nM - 136:].double(), tB[:, nM - 136:].double())
    with mode:
        full = _grads(_fused, Q, dev, wA, wB)
        mat = _grads(lambda P_, rf, gr: _materialised(P_, dev, rf, gr), Q, dev, wA, wB)
        tail = _grads(_fused, Q, dev, tA, tB)
        again = _grads(_fused, Q, dev, tA, tB)
    for k in ('A', 'B'):
        assert_close(full[k], mat[k], tag, f'{k} vs the materialised route')
        assert_close(full[k][:, nM - 136:], ora[k], tag, f'{k} on the last 136 spins vs the fp64 oracle')
    for k in ('grad_rf', 'grad_gr'):
        assert torch.equal(tail[k], again[k]), (k, 'second run')
        record(f'ab_ptx.tiles.{tag_mode}.full.{k}.vs_materialised',
               max_abs(full[k], mat[k]) if tag == 'f64' else rel_l2(full[k], mat[k]))
        record(f'ab_ptx.tiles.{tag_mode}.tail.{k}.vs_oracle64',
               max_abs(tail[k], ora[k]) if tag == 'f64' else rel_l2(tail[k], ora[k]))
        assert_close(full[k], mat[k], tag, f'FULL weights: {k} vs the materialised route')
        assert_close(tail[k], ora[k], tag, f'TAIL-ONLY weights: {k} vs the fp64 oracle on the last 136 spins')


# =============================================================================================
# 5. zero-field steps and spins with γ = 0, 4 coils
# =============================================================================================
@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', [('f64', 'precise'), ('f32', 'precise'), ('f32', 'fast')])
@pytest.mark.parametrize('kind', ['zero', 'gamma0'])
def test_zero_field_steps_and_gamma_zero_spins(tag, mode, kind, monkeypatch):
    r"""``cases.zero_field_case`` and 'gamma_split' with ``γ = 0`` on ``ZERO_SPINS``, both at ``nC = 4``, through the
    invariants of ``test_ab_operands`` (everything finite; ``A, B`` the materialised route's bits; the gradients at the gates
    against the column yardstick, which holds the zero-field limit -- on the zero-field steps alone and on the all-zero
    segment alone as well; twice the same bits) -- on the parallel-transmit kernels: the call counter says so.  The spin
    whose map is zero never rotates; the ``γ = 0`` spins' ``A`` is the relaxation diagonal with exactly zero
    off-diagonals."""
    from test_ab_operands import _case, _invariants, _relaxed_only
    calls = _counted(monkeypatch, COUNTED)
    v = _case(tag, kind, 4, 48)[0]
    with mrphy_amd.precision(mode):
        fu = _invariants(tag, mode, kind, 4, 48)
    assert calls[FWD_MC] >= 3 and calls[BWD_MC] == 2 and not calls[FWD] and not calls[BWD], dict(calls)
    for k in fu:
        assert bool(torch.isfinite(fu[k]).all()), k
    spins = ((1, 64),) if kind == 'zero' else cases.ZERO_SPINS
    for n, s in spins:
        A, B = _relaxed_only(v, n, s, 48)
        assert_close(fu['A'][n, s], A, tag, f'spin {(n, s)}: A')
        if kind == 'gamma0':
            assert float((fu['A'][n, s] - torch.diag(torch.diagonal(fu['A'][n, s]))).abs().max()) == 0.0, (n, s)
        else:
            assert max_abs(fu['B'][n, s, :2], B[:2]) == 0.0
        assert rel_l2(fu['B'][n, s], B) <= (1e-12 if tag == 'f64' else 1e-5)


# =============================================================================================
# 6. no Beff in memory
# =============================================================================================
def test_no_beff_in_memory(monkeypatch):
    r"""N = 1, nM = 4096, nT = 256, 4 coils, fp32, forward + backward: the allocator's peak rises by less than half of
    ``Beff``'s bytes (12 nM nT).  In fractions of ``Beff``: the checkpoints are exactly 0.25 (4 columns x 3 x nM x nT / 16);
    ``A, B`` and their cotangents 2 x 12 nM x 4 B = 0.03, the workspace of 64 waves x 11 rows x nT 0.06, the pulse gradients
    and their folds below 0.01 -- under 0.1 together.  The composed route on the same problem rises by more than all of
    ``Beff``."""
    nM, nT = 4096, 256
    P = _ptx('f32', 4, nT, N=1, nM=nM)
    wA, wB = (dev(x) for x in _weights(1, nM, torch.float32))
    Pd = {k: dev(x) for k, x in P.items()}
    beff_bytes = 12 * nM * nT
    calls = _counted(monkeypatch, COUNTED)
    kw = dict(Δf=Pd['df'], b1Map=Pd['b1'], γ_beff=Pd['γ'], T1=Pd['T1'], T2=Pd['T2'], γ=Pd['γ'], dt=Pd['dt'])

    def rise():
        rf, gr = Pd['rf'].clone().requires_grad_(True), Pd['gr'].clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        A, B = fused.ab_rfgr(rf, gr, Pd['loc'], **kw)
        ((A * wA).sum() + (B * wB).sum()).backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    fu = rise()
    assert dict(calls) == {FWD_MC: 1, BWD_MC: 1}, dict(calls)
    decide = fused._decide_ab_route
    monkeypatch.setattr(fused, '_decide_ab_route', lambda **facts: decide(**dict(facts, ptx_fused=False)))
    calls.clear()
    mat = rise()
    assert not calls[FWD_MC] and not calls[BWD_MC] and calls['mrphy_beff2ab_save'] == 1, dict(calls)
    record('ab_ptx.memory.fused_peak_over_beff_bytes', fu / beff_bytes, 0.5)
    record('ab_ptx.memory.composed_peak_over_beff_bytes', mat / beff_bytes)
    record('ab_ptx.memory.composed_over_fused', mat / fu)
    assert fu < 0.5 * beff_bytes < beff_bytes < mat, (fu, beff_bytes, mat)


# =============================================================================================
# 7. steadystate_rfgr with 4 coils
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_steadystate_rfgr_inherits_parallel_transmit(tag, monkeypatch):
    r"""``Mss`` against ``torch_steadystate`` of the fused ``A, B`` at the steady-state kernels' own gate; ``grad_rf,
    grad_gr`` against the same call with ``ab_rfgr`` composed (``ptx_fused`` forced to ``False``); one ``_mc_fwd`` and one
    ``_mc_bwd``."""
    from test_steadystate import _gate
    from test_steadystate_host import torch_steadystate
    P = _ptx(tag, 4, 48)
    gen = torch.Generator().manual_seed(4100)
    rnd = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64)  # noqa: E731
    # T1 in 0.05 .. 0.15 s and T2 in 0.02 .. 0.07 s with a rest of 5 ms: I - A F as well conditioned as in test_steadystate
    P['T1'], P['T2'] = (0.05 + 0.1 * rnd(2, 100)).to(DT[tag]), (0.02 + 0.05 * rnd(2, 100)).to(DT[tag])
    rest = dev(torch.tensor(5e-3, dtype=DT[tag]))
    w = dev(torch.sin(torch.arange(600, dtype=torch.float64) * 0.37 + 0.3).reshape(2, 100, 3).to(DT[tag]))
    kw = dict(Δf=dev(P['df']), b1Map=dev(P['b1']), γ_beff=dev(P['γ']), T1=dev(P['T1']), T2=dev(P['T2']), γ=dev(P['γ']),
              dt=dev(P['dt']))
    loc = dev(P['loc'])
    calls = _counted(monkeypatch, COUNTED)

    def run():
        rf, gr = dev(P['rf']).requires_grad_(True), dev(P['gr']).requires_grad_(True)
        Mss = fused.steadystate_rfgr(rf, gr, loc, rest=rest, **kw)
        (Mss * w).sum().backward()
        return Mss.detach(), rf.grad, gr.grad

    Mss, grf, ggr = run()
    assert {k: v for k, v in calls.items() if v} == {FWD_MC: 1, BWD_MC: 1}, dict(calls)
    with torch.no_grad():
        A, B = fused.ab_rfgr(dev(P['rf']), dev(P['gr']), loc, **{k: x for k, x in kw.items()})
    _gate(Mss, torch_steadystate(A.double().cpu(), B.double().cpu(), rest.double().cpu(), P['T1'].double(), P['T2'].double(),
                                 P['df'].double()), tag, 'Mss vs the torch solve on the fused A, B')
    decide = fused._decide_ab_route
    monkeypatch.setattr(fused, '_decide_ab_route', lambda **facts: decide(**dict(facts, ptx_fused=False)))
    calls.clear()
    Mss_c, grf_c, ggr_c = run()
    assert not calls[FWD_MC] and not calls[BWD_MC] and calls['mrphy_beff2ab_save'] == 1, dict(calls)
    assert grf.shape == P['rf'].shape and ggr.shape == P['gr'].shape and float(grf.abs().max()) > 0
    assert_close(Mss, Mss_c, tag, 'Mss vs the composed route')
    assert_close(grf, grf_c, tag, 'grad_rf vs the composed route')
    assert_close(ggr, ggr_c, tag, 'grad_gr vs the composed route')


# =============================================================================================
# 8. the entry points, called directly
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_direct_abi_call_with_one_coil(tag):
    r"""``nC = 1`` with a map through ``mrphy_ab_rfgr_mc_fwd`` / ``_mc_bwd`` (the capacity-2 builds, one coil zero-padded):
    ``A, B`` are the materialised route's bits (and the one-coil kernel's), the checkpoints the one-coil kernel's, the
    gradients within the gates of ``mrphy_ab_rfgr_bwd``'s.  Then ``N = 65536`` is refused with the NaN-filled outputs
    untouched, after which the process passes a normal call."""
    from mrphy_amd import sims
    lib = mrphy_amd.require_library()
    N, nM, nT, dt_ = 2, 100, 48, DT[tag]
    P = _problem(tag, 'b1map', nT)
    new = lambda *s: torch.full(s, float('nan'), dtype=dt_, device=DEV)  # noqa: E731
    p = beffective._PulseOnSpins(dev(P['rf']), dev(P['gr']), dev(P['loc']), dev(P['df']), dev(P['b1']), dev(P['γ']))
    assert p.nC == 1 and p.b1.shape == (N, nM, 2, 1)
    cs = sims.relax_constants(dev(P['T1']), dev(P['T2']), dev(P['γ']), dev(P['dt']), 4, DEV)
    code, alive, consts, _, _ = _forward_prep(lib, p, *cs, dt_, DEV, False)
    ck = int(lib.mrphy_blochsim_rfgr_ck_every())
    st = _host.current_stream(DEV)
    wA, wB = (dev(x) for x in _weights(N, nM, dt_))

    def mc():
        A, B, ABck = new(N, nM, 3, 3), new(N, nM, 3), new(nT // ck, 4, N * nM, 3)
        assert lib.mrphy_ab_rfgr_mc_fwd(code, *p.k0_args(), *consts, A.data_ptr(), B.data_ptr(), ABck.data_ptr(), ck,
                                        N, nM, nT, 1, st) == 0
        nbytes = int(lib.mrphy_ab_rfgr_mc_bwd_workspace(code, N, nM, nT, 1))
        work = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        grf, ggr = new(N, 2, nT, 1), new(N, 3, nT)
        assert lib.mrphy_ab_rfgr_mc_bwd(code, ABck.data_ptr(), *p.k0_args(), *consts, wA.data_ptr(), wB.data_ptr(),
                                        grf.data_ptr(), ggr.data_ptr(), work.data_ptr(), nbytes, N, nM, nT, 1, st) == 0
        return A, B, ABck, grf, ggr

    A, B, ABck, grf, ggr = mc()
    A1, B1, ABck1 = new(N, nM, 3, 3), new(N, nM, 3), new(nT // ck, 4, N * nM, 3)
    assert lib.mrphy_ab_rfgr_fwd(code, *p.k0_args(), *consts, A1.data_ptr(), B1.data_ptr(), ABck1.data_ptr(), ck,
                                 N, nM, nT, st) == 0
    nbytes1 = int(lib.mrphy_blochsim_rfgr_bwd_workspace(code, N, nM, nT))
    work1 = torch.empty(nbytes1, dtype=torch.uint8, device=DEV)
    grf1, ggr1 = new(N, 2, nT, 1), new(N, 3, nT)
    assert lib.mrphy_ab_rfgr_bwd(code, ABck1.data_ptr(), *p.k0_args(), *consts, wA.data_ptr(), wB.data_ptr(),
                                 grf1.data_ptr(), ggr1.data_ptr(), work1.data_ptr(), nbytes1, N, nM, nT, st) == 0
    with torch.no_grad():
        beff = beffective.rfgr2beff(dev(P['rf']), dev(P['gr']), dev(P['loc']), Δf=dev(P['df']), b1Map=dev(P['b1']),
                                    γ=dev(P['γ']))
        A0, B0 = beffective._Beff2AB.apply(beff, *cs, False)
    assert torch.equal(A, A0) and torch.equal(B, B0), 'the materialised route on the same constants'
    assert torch.equal(A, A1) and torch.equal(B, B1) and torch.equal(ABck, ABck1), 'the one-coil kernel'
    assert_close(grf, grf1, tag, 'grad_rf vs mrphy_ab_rfgr_bwd')
    assert_close(ggr, ggr1, tag, 'grad_gr vs mrphy_ab_rfgr_bwd')
    # N = 65536: more batch entries than a grid holds -- refused, outputs untouched
    A2, B2, g2 = new(1, 1, 3, 3), new(1, 1, 3), new(1, 2, nT, 1)
    assert lib.mrphy_ab_rfgr_mc_fwd(code, *p.k0_args(), *consts, A2.data_ptr(), B2.data_ptr(), None, 0,
                                    65536, 1, nT, 1, st) == -1
    assert lib.mrphy_ab_rfgr_mc_bwd(code, ABck.data_ptr(), *p.k0_args(), *consts, wA.data_ptr(), wB.data_ptr(),
                                    g2.data_ptr(), None, work1.data_ptr(), 1 << 50, 65536, 1, nT, 1, st) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(A2).all()) and bool(torch.isnan(B2).all()) and bool(torch.isnan(g2).all())
    A3, B3, _, grf3, ggr3 = mc()
    assert torch.equal(A3, A) and torch.equal(B3, B) and torch.equal(grf3, grf) and torch.equal(ggr3, ggr)
