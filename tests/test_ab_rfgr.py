r"""``fused.ab_rfgr`` on the device: Hargreaves' ``A, B`` of a pulse from ``rf`` and ``gr`` (K2ab) and the fused adjoint
w.r.t. the pulse (K2abb).

The forward is held bit for bit to the materialised route ``beffective.beff2ab(rfgr2beff(.))`` on the same step
constants and, through the public ``T1 / T2`` signature, to ``blochsim_rfgr`` column by column; values and gradients are
held at the project's gates (``util.assert_close``: fp64 max-abs 1e-9, fp32 relative L2 1e-5) to the fixture from the
live reference (``tests/golden/ab_rfgr_*.npz``), to the CPU oracle in fp64 and to autograd through the materialised
route.  Shapes: N = 2, nM = 100 (one full wave and a ragged one with 36 valid lanes) unless a test says otherwise;
operands: ``test_fused_traj._problem``.

More tiles than persistent waves (``test_more_tiles_than_persistent_waves``; the method of ``test_fused_tiles.py``):
N = 2, nT = 32, ``nM = P 64 + 100`` with ``P`` from the workspace query, so waves 0 and 1 take a second tile, the
second of them ragged.  With the TAIL-ONLY weights (zero cotangent on every spin of the tiles ``< P``) the pulse
gradients must equal, to the gate, the fp64 oracle's on the last 136 spins alone.  Oracle-side dry run of that
comparison on the CPU, one tile's spins left out of the sum (the oracle's tail gradients without the 36 spins of the
ragged tile, or without the 64 of tile ``P``, against those of all 100 with a cotangent): ``grad_rf`` and ``grad_gr``
move by 0.36 .. 0.85 in relative L2 over the two variants -- more than 3e4 times the fp32 gate -- and by 0.98 .. 8.1
in max abs, more than 9e8 times the fp64 gate.  With the FULL weights the yardstick is autograd through the materialised
route on the device (the oracle's autograd over 262 344 spins is minutes and gigabytes on the CPU).
"""
import collections
import functools
from math import pi as π

import pytest

from gpu_common import *  # noqa: F401,F403
from mrphy_amd import _host
from mrphy_amd.fused import _forward_prep
from test_ab_rfgr_host import fixture_inputs, oracle_ab
from test_fused_traj import _problem

pytestmark = pytest.mark.gpu

MODES = ['f64', 'f32-precise', 'f32-fast']
VARIANTS = ['plain', 'b1map', 'norelax', 'plain_batch1_pulse']
FWD, BWD = 'mrphy_ab_rfgr_fwd', 'mrphy_ab_rfgr_bwd'
COMPOSED = ('mrphy_rfgr2beff_st', 'mrphy_beff2ab', 'mrphy_beff2ab_save', 'mrphy_beff2ab_bwd')
WAVE = 64


def _mode(tag_mode):
    tag, _, mode = tag_mode.partition('-')
    return tag, mrphy_amd.precision(mode or 'precise')


def _wave(n, freq, phase):
    return torch.sin(torch.arange(n, dtype=torch.float64) * freq + phase)


def _weights(N, nM, dtype, which='both'):
    r"""``wA`` (N, nM, 3, 3), ``wB`` (N, nM, 3) of the loss ``(A wA).sum() + (B wB).sum()``: 'both', 'A' / 'B' (the other
    term's weights zero), 'col0' .. 'col2' (``wA`` on that column of A alone, ``wB`` zero)."""
    wA = _wave(N * nM * 9, 0.61, 1.0).reshape(N, nM, 3, 3)
    wB = _wave(N * nM * 3, 0.37, 0.3).reshape(N, nM, 3)
    if which == 'A' or which.startswith('col'):
        wB = torch.zeros_like(wB)
    if which == 'B':
        wA = torch.zeros_like(wA)
    if which.startswith('col'):
        keep = torch.zeros(3, dtype=torch.float64)
        keep[int(which[3:])] = 1
        wA = wA * keep
    return wA.to(dtype), wB.to(dtype)


def _factors(P):
    r"""``E1, E2`` of the problem as ``beff2ab`` takes them (the relaxation FACTORS; ones without relaxation), on the CPU in
    the data type; kept in ``P``, so that a widened copy of the problem (the oracle's) holds the same numbers."""
    if 'E1' not in P:
        if P['T1'] is None:
            P['E1'], P['E2'] = torch.ones((), dtype=P['loc'].dtype), torch.ones((), dtype=P['loc'].dtype)
        else:
            P['E1'], P['E2'] = torch.exp(-P['dt'][:, None] / P['T1']), torch.exp(-P['dt'][:, None] / P['T2'])
    return P['E1'], P['E2']


def _materialised(P, on, rf, gr):
    r"""``A, B`` by ``rfgr2beff`` + ``beff2ab`` (``on`` = ``dev``) or by the oracle (``on`` = identity)."""
    mod_b, mod_a = (beffective.rfgr2beff, beffective.beff2ab) if on is dev else (O.rfgr2beff, O.beff2ab)
    E1, E2 = _factors(P)
    beff = mod_b(rf, gr, on(P['loc']), Δf=on(P['df']), b1Map=on(P['b1']), γ=on(P['γ']))
    return mod_a(beff, E1=on(E1), E2=on(E2), γ=on(P['γ']), dt=on(P['dt']))


def _fused(P, rf, gr, **over):
    kw = dict(Δf=dev(P['df']), b1Map=dev(P['b1']), γ_beff=dev(P['γ']), T1=dev(P['T1']), T2=dev(P['T2']), γ=dev(P['γ']),
              dt=dev(P['dt']))
    kw.update(over)
    return fused.ab_rfgr(rf, gr, dev(P['loc']), **kw)


def _grads(run, P, on, wA, wB):
    r"""``A, B, grad_rf, grad_gr`` of the loss through ``run(P, rf, gr)`` on the device (``on`` = ``dev``) or the CPU."""
    rf, gr = on(P['rf']).clone().requires_grad_(True), on(P['gr']).clone().requires_grad_(True)
    A, B = run(P, rf, gr)
    ((A * on(wA).to(A.dtype)).sum() + (B * on(wB).to(B.dtype)).sum()).backward()
    return dict(A=A.detach(), B=B.detach(), grad_rf=rf.grad, grad_gr=gr.grad)


def _widened(P):
    _factors(P)
    return {k: (None if x is None else x.double()) for k, x in P.items()}


def _counted(monkeypatch, names=(FWD, BWD) + COMPOSED):
    lib = mrphy_amd.require_library()
    calls = collections.Counter()

    def wrap(name, fn):
        def counted(*a):
            calls[name] += 1
            return fn(*a)
        return counted
    for name in names:
        monkeypatch.setattr(lib, name, wrap(name, getattr(lib, name)))
    return calls


# =============================================================================================
# 5. forward bits vs the materialised route
# =============================================================================================
@pytest.mark.parametrize('tag_mode', MODES)
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('nT', [48, 50, 7])
def test_forward_is_the_materialised_route_bit_for_bit(tag_mode, variant, nT):
    r"""``A, B`` == ``beff2ab(rfgr2beff(.))`` with the same four constants: ``beff2ab``'s own ``2πγ·dt, E1, E2, E1 - 1``,
    formed once on the device by its expressions and handed to ``ab_rfgr`` as ``consts=`` (without relaxation: factors of
    one and a zero offset).  nT = 50 and 7 run the tail loop; every output element is written (NaN-free, right shape)."""
    tag, mode = _mode(tag_mode)
    P = _problem(tag, variant, nT)
    E1, E2 = (dev(x) for x in _factors(P))
    γ, dt = dev(P['γ']), dev(P['dt'])
    pad = lambda x: _host.pad_trailing(x, 2)  # noqa: E731  (beff2ab pads to the rank of (N, *Nd))
    consts = dict(γ2πdt=2 * π * pad(γ) * pad(dt), E1=pad(E1), E2=pad(E2), E1_1=pad(E1) - 1)
    with mode, torch.no_grad():
        beff = beffective.rfgr2beff(dev(P['rf']), dev(P['gr']), dev(P['loc']), Δf=dev(P['df']), b1Map=dev(P['b1']),
                                    γ=γ)
        A0, B0 = beffective.beff2ab(beff, E1=E1, E2=E2, γ=γ, dt=dt)
        A, B = _fused(P, dev(P['rf']), dev(P['gr']), T1=None, T2=None, consts=consts)
    assert A.shape == (2, 100, 3, 3) and B.shape == (2, 100, 3) and A.dtype == B.dtype == DT[tag]
    assert torch.equal(A, A0) and torch.equal(B, B0)


# =============================================================================================
# 6. forward bits vs the simulator, through the public T1 / T2 signature
# =============================================================================================
@pytest.mark.parametrize('tag_mode', MODES)
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('nT', [48, 50, 7])
def test_forward_is_the_simulator_column_by_column(tag_mode, variant, nT):
    r"""Without relaxation ``A[..., :, j]`` is ``blochsim_rfgr(Mi = e_j)`` bit for bit and ``B`` an exact zero; with
    relaxation ``B`` is ``blochsim_rfgr(Mi = 0)`` bit for bit -- the same ``T1, T2, γ, dt`` on both sides."""
    tag, mode = _mode(tag_mode)
    P = _problem(tag, variant, nT)
    kw = dict(Δf=dev(P['df']), b1Map=dev(P['b1']), γ_beff=dev(P['γ']), T1=dev(P['T1']), T2=dev(P['T2']), γ=dev(P['γ']),
              dt=dev(P['dt']))
    rf, gr, loc = dev(P['rf']), dev(P['gr']), dev(P['loc'])
    with mode, torch.no_grad():
        A, B = fused.ab_rfgr(rf, gr, loc, **kw)
        if variant == 'norelax':
            assert torch.equal(B, torch.zeros_like(B))
            for j in range(3):
                e = torch.zeros((2, 100, 3), dtype=DT[tag], device=DEV)
                e[..., j] = 1
                assert torch.equal(A[..., :, j], fused.blochsim_rfgr(e, rf, gr, loc, **kw)), j
        else:
            zero = torch.zeros((2, 100, 3), dtype=DT[tag], device=DEV)
            assert torch.equal(B, fused.blochsim_rfgr(zero, rf, gr, loc, **kw))
            assert float(B.abs().max()) > 0


# =============================================================================================
# 7. the fixture from the reference, and the oracle
# =============================================================================================
@pytest.mark.parametrize('tag_mode', MODES)
def test_against_the_reference_fixture_and_the_oracle(tag_mode, monkeypatch):
    tag, mode = _mode(tag_mode)
    G = golden(f'ab_rfgr_{tag}')
    Q = fixture_inputs(G)
    ora = oracle_ab(Q, torch.float64)
    calls = _counted(monkeypatch)
    rf, gr = dev(Q['rf']).requires_grad_(True), dev(Q['gr']).requires_grad_(True)
    γ, dt, E1 = dev(Q['γ']), dev(Q['dt']), dev(Q['E1'])
    with mode:
        A, B = fused.ab_rfgr(rf, gr, dev(Q['loc']), Δf=dev(Q['df']), b1Map=dev(Q['b1']), γ_beff=γ,
                             consts=dict(γ2πdt=2 * π * γ * dt, E1=E1, E2=dev(Q['E2']), E1_1=E1 - 1))
        ((A * dev(Q['wA'])).sum() + (B * dev(Q['wB'])).sum()).backward()
    assert calls[FWD] == 1 and calls[BWD] == 1 and not any(calls[n] for n in COMPOSED), dict(calls)
    got = dict(A=A.detach(), B=B.detach(), grad_rf=rf.grad, grad_gr=gr.grad)
    for k, x in got.items():
        record(f'ab_rfgr.{tag_mode}.fixture.{k}', max_abs(x, G[k]) if tag == 'f64' else rel_l2(x, G[k]))
        record(f'ab_rfgr.{tag_mode}.fixture.{k}.vs_oracle64', max_abs(x, ora[k]) if tag == 'f64' else rel_l2(x, ora[k]))
        assert_close(x, G[k], tag, f'{k} vs the reference fixture')
        assert_close(x, ora[k], tag, f'{k} vs the fp64 oracle')


# =============================================================================================
# 8. gradients
# =============================================================================================
LOSSES = ['both', 'A', 'B', 'col0', 'col1', 'col2']
ROUTE_CALLS = {16: 'fused', 48: 'fused', 50: 'split', 7: 'composed'}


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag_mode', MODES)
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('nT', [16, 48, 50, 7])
def test_gradients(tag_mode, variant, nT, monkeypatch):
    r"""``grad_rf, grad_gr`` of ``(A wA).sum() + (B wB).sum()``, of each term alone and of ``wA`` on a single column of A
    (a cotangent routed to the wrong column would be seen: the columns' gradients differ by O(1)), against autograd
    through ``rfgr2beff`` -> ``beff2ab`` on the device and the oracle's autograd in fp64; ``A, B`` likewise; a second run
    gives the same bits; a batch-1 pulse gets gradients of its own shape.  nT = 48 and 16 are one ``_fwd`` and one
    ``_bwd`` and nothing of the materialised route; 50 splits at 48; 7 is composed."""
    tag, mode = _mode(tag_mode)
    P = _problem(tag, variant, nT)
    calls = _counted(monkeypatch)
    for which in LOSSES:
        wA, wB = _weights(2, 100, DT[tag], which)
        with mode:
            calls.clear()
            fu = _grads(_fused, P, dev, wA, wB)
            n = dict(calls)
            again = _grads(_fused, P, dev, wA, wB)
            mat = _grads(lambda P_, rf, gr: _materialised(P_, dev, rf, gr), P, dev, wA, wB)
        ora = _grads(lambda P_, rf, gr: _materialised(P_, lambda x: x, rf, gr), _widened(P), lambda x: x,
                     wA.double(), wB.double())
        route = ROUTE_CALLS[nT]
        if route == 'fused':
            assert n == {FWD: 1, BWD: 1}, (which, n)
        elif route == 'split':
            assert n.get(FWD) == 1 and n.get(BWD) == 1 and n.get('mrphy_beff2ab_save') == 1, (which, n)
        else:
            assert not n.get(FWD) and not n.get(BWD) and n.get('mrphy_beff2ab_save') == 1, (which, n)
        assert fu['grad_rf'].shape == P['rf'].shape and fu['grad_gr'].shape == P['gr'].shape
        # (without relaxation B is an exact zero and so is the gradient of a loss on B alone)
        for k in fu:
            assert bool(torch.isfinite(fu[k]).all()), (which, k)
            assert torch.equal(fu[k], again[k]), (which, k, 'second run')
            assert_close(fu[k], mat[k], tag, f'{which}: {k} vs the materialised route')
            assert_close(fu[k], ora[k], tag, f'{which}: {k} vs the fp64 oracle')
        if which.startswith('col') or (which == 'both') or (which == 'B' and variant != 'norelax'):
            assert float(fu['grad_rf'].abs().max()) > 0, which          # (B is O(1e-5) after a few steps, and so is its gradient)


# =============================================================================================
# 9. more tiles than persistent waves
# =============================================================================================
NT_TILES = 32


@functools.lru_cache(maxsize=None)
def _tiles_shape(tag):
    r"""``(P, nM)``: the cap on the adjoint's persistent waves, from the workspace query, and nM = P 64 + 100."""
    lib = mrphy_amd.require_library()
    code = _host.dtype_code(DT[tag], DT[tag])
    waves = lambda nM: int(lib.mrphy_blochsim_rfgr_bwd_workspace(code, 2, nM, NT_TILES)) // (  # noqa: E731
        2 * 5 * NT_TILES * DT[tag].itemsize)
    P = waves(1 << 30)
    nM = P * WAVE + 100
    assert waves(nM) == P and -(-nM // WAVE) == P + 2
    return P, nM


def _tail(P_, nM, last=136):
    r"""The problem restricted to its last ``last`` spins."""
    return {k: (x[:, nM - last:] if k in ('M0', 'loc', 'df', 'b1', 'T1', 'T2', 'E1', 'E2') and x is not None else x)
            for k, x in P_.items()}


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag_mode', MODES)
@pytest.mark.parametrize('variant', ['plain', 'b1map'])
def test_more_tiles_than_persistent_waves(tag_mode, variant):
    r"""Module docstring: FULL weights against the materialised route on the device, TAIL-ONLY weights against the fp64
    oracle on the last 136 spins; ``A, B`` of those spins against the oracle too; twice the same bits."""
    tag, mode = _mode(tag_mode)
    P, nM = _tiles_shape(tag)
    Q = _problem(tag, variant, NT_TILES, N=2, nM=nM)
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
        record(f'ab_rfgr.tiles.{tag_mode}.{variant}.full.{k}.vs_materialised',
               max_abs(full[k], mat[k]) if tag == 'f64' else rel_l2(full[k], mat[k]))
        record(f'ab_rfgr.tiles.{tag_mode}.{variant}.tail.{k}.vs_oracle64',
               max_abs(tail[k], ora[k]) if tag == 'f64' else rel_l2(tail[k], ora[k]))
        assert_close(full[k], mat[k], tag, f'FULL weights: {k} vs the materialised route')
        assert_close(tail[k], ora[k], tag, f'TAIL-ONLY weights: {k} vs the fp64 oracle on the last 136 spins')


# =============================================================================================
# 10. dtype codes 2 / 4: fp32 data with fp64 constants
# =============================================================================================
@pytest.mark.parametrize('mode', ['precise', 'fast'])
def test_f32_data_with_f64_constants(mode, monkeypatch):
    r"""The step constants as fp64 tensors beside fp32 data: the fused kernels run under the codes MRPHY_F32P_C64 (4) /
    MRPHY_F32_C64 (2); values and gradients against the materialised route in the same mode.  That route rounds its
    constants to the data type (``beff2ab``), so the fp64 tensors hold ITS numbers -- ``2πγ·dt``, ``E1``, ``E2`` and the
    difference ``E1 - 1`` as it forms them in fp32, widened: both sides then integrate the same function, and what
    differs is the precision of the products with the constants.  (With constants formed in fp64 the two are not the
    same function to the gate: ``E1 - 1`` is about -4e-6, and its fp32 form carries a rounding error of 6e-8, 1.5 % of
    it, which ``B`` is proportional to.)"""
    P = _problem('f32', 'b1map', 48)
    E1, E2 = (dev(x) for x in _factors(P))
    γ, dt = dev(P['γ']), dev(P['dt'])
    pad = lambda x: _host.pad_trailing(x, 2)  # noqa: E731
    consts = {k: v.double() for k, v in dict(γ2πdt=2 * π * pad(γ) * pad(dt), E1=pad(E1), E2=pad(E2),
                                             E1_1=pad(E1) - 1).items()}
    lib = mrphy_amd.require_library()
    codes = []
    for name in (FWD, BWD):
        monkeypatch.setattr(lib, name, (lambda fn: lambda *a: (codes.append(a[0]), fn(*a))[1])(getattr(lib, name)))
    wA, wB = _weights(2, 100, torch.float32)
    with mrphy_amd.precision(mode):
        fu = _grads(lambda P_, rf, gr: _fused(P_, rf, gr, T1=None, T2=None, consts=consts), P, dev, wA, wB)
        mat = _grads(lambda P_, rf, gr: _materialised(P_, dev, rf, gr), P, dev, wA, wB)
    want = mrphy_amd._lib.F32P_C64 if mode == 'precise' else mrphy_amd._lib.F32_C64
    assert codes == [want, want], codes
    for k in fu:
        assert fu[k].dtype == torch.float32
        record(f'ab_rfgr.c64.{mode}.{k}.vs_materialised', rel_l2(fu[k], mat[k]), 1e-5)
        assert_close(fu[k], mat[k], 'f32', f'{k} vs the materialised route')


# =============================================================================================
# 11. empty problems
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('empty', ['nT', 'nM'])
def test_empty_problem(tag, empty):
    r"""No step: ``A = I``, ``B = 0`` and the backward gives zeros of the shapes of ``rf``, ``gr``; no spin: empty outputs,
    and the backward runs."""
    nT, nM = (0, 100) if empty == 'nT' else (48, 0)
    P = _problem(tag, 'b1map', nT, nM=nM)
    wA, wB = _weights(2, nM, DT[tag])
    got = _grads(_fused, P, dev, wA, wB)
    assert got['A'].shape == (2, nM, 3, 3) and got['B'].shape == (2, nM, 3)
    if empty == 'nT':
        assert torch.equal(got['A'], torch.eye(3, dtype=DT[tag], device=DEV).expand(2, nM, 3, 3))
        assert torch.equal(got['B'], torch.zeros_like(got['B']))
    for k in ('rf', 'gr'):
        assert got['grad_' + k].shape == P[k].shape and float(got['grad_' + k].abs().sum()) == 0.0


# =============================================================================================
# 12. no Beff in memory
# =============================================================================================
def test_no_beff_in_memory():
    r"""N = 1, nM = 4096, nT = 256, fp32, forward + backward: the allocator's peak rises by less than half of ``Beff``'s
    bytes (12 nM nT) -- the checkpoints are exactly a quarter of them, outputs, cotangents and the workspace small beside
    that -- where the materialised route rises by more than all of them."""
    nM, nT = 4096, 256
    P = _problem('f32', 'b1map', nT, N=1, nM=nM)
    wA, wB = (dev(x) for x in _weights(1, nM, torch.float32))
    Pd = {k: dev(x) for k, x in P.items()}
    beff_bytes = 12 * nM * nT

    def rise(run):
        rf, gr = Pd['rf'].clone().requires_grad_(True), Pd['gr'].clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        A, B = run(rf, gr)
        ((A * wA).sum() + (B * wB).sum()).backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    kw = dict(Δf=Pd['df'], b1Map=Pd['b1'], γ_beff=Pd['γ'], T1=Pd['T1'], T2=Pd['T2'], γ=Pd['γ'], dt=Pd['dt'])
    E1, E2 = (dev(x) for x in _factors(P))
    fu = rise(lambda rf, gr: fused.ab_rfgr(rf, gr, Pd['loc'], **kw))
    mat = rise(lambda rf, gr: beffective.beff2ab(
        beffective.rfgr2beff(rf, gr, Pd['loc'], Δf=Pd['df'], b1Map=Pd['b1'], γ=Pd['γ']), E1=E1, E2=E2, γ=Pd['γ'],
        dt=Pd['dt']))
    record('ab_rfgr.memory.fused_peak_over_beff_bytes', fu / beff_bytes, 0.5)
    record('ab_rfgr.memory.materialised_peak_over_beff_bytes', mat / beff_bytes)
    assert fu < 0.5 * beff_bytes, (fu, beff_bytes)
    assert mat > beff_bytes, (mat, beff_bytes)


# =============================================================================================
# 13. the two entry points, called directly
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_direct_abi_call(tag):
    r"""``mrphy_ab_rfgr_fwd`` with checkpoints and ``mrphy_ab_rfgr_bwd`` through ctypes (N = 2, nM = 100, nT = 48, a b1
    map, relaxation): plane ``j < 3`` of ``ABck`` is the ``Mck`` of ``mrphy_blochsim_rfgr_fwd`` for ``Mi = e_j`` with a zero
    offset, plane 3 the one for ``Mi = 0`` with the real offset, bit for bit; ``A, B`` and the gradients are the public
    function's bits.  Outputs start as NaN: an element left unwritten fails the comparison."""
    from mrphy_amd import sims
    lib = mrphy_amd.require_library()
    N, nM, nT, dt_ = 2, 100, 48, DT[tag]
    P = _problem(tag, 'b1map', nT)
    new = lambda *s: torch.full(s, float('nan'), dtype=dt_, device=DEV)  # noqa: E731
    p = beffective._PulseOnSpins(dev(P['rf']), dev(P['gr']), dev(P['loc']), dev(P['df']), dev(P['b1']), dev(P['γ']))
    cs = sims.relax_constants(dev(P['T1']), dev(P['T2']), dev(P['γ']), dev(P['dt']), 4, DEV)
    code, alive, consts, _, _ = _forward_prep(lib, p, *cs, dt_, DEV, False)
    ck = int(lib.mrphy_blochsim_rfgr_ck_every())
    st = _host.current_stream(DEV)
    A, B, ABck = new(N, nM, 3, 3), new(N, nM, 3), new(nT // ck, 4, N * nM, 3)
    assert lib.mrphy_ab_rfgr_fwd(code, *p.k0_args(), *consts, A.data_ptr(), B.data_ptr(), ABck.data_ptr(), ck,
                                 N, nM, nT, st) == 0
    zero_off = torch.zeros_like(alive[3].t)
    for j in range(4):
        Mi = torch.zeros((N, nM, 3), dtype=dt_, device=DEV)
        if j < 3:
            Mi[..., j] = 1
        off = consts[:-1] + ((zero_off if j < 3 else alive[3].t).data_ptr(),)
        Mo, Mck = new(N, nM, 3), new(nT // ck, N * nM, 3)
        assert lib.mrphy_blochsim_rfgr_fwd(code, Mi.data_ptr(), *p.k0_args(), *off, Mo.data_ptr(), Mck.data_ptr(), ck,
                                           N, nM, nT, 1, st) == 0
        assert torch.equal(ABck[:, j], Mck), j
        assert torch.equal(A[..., :, j] if j < 3 else B, Mo), j
    wA, wB = (dev(x) for x in _weights(N, nM, dt_))
    nbytes = int(lib.mrphy_blochsim_rfgr_bwd_workspace(code, N, nM, nT))
    work = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    grf, ggr = new(N, 2, nT, 1), new(N, 3, nT)
    assert lib.mrphy_ab_rfgr_bwd(code, ABck.data_ptr(), *p.k0_args(), *consts, wA.data_ptr(), wB.data_ptr(),
                                 grf.data_ptr(), ggr.data_ptr(), work.data_ptr(), nbytes, N, nM, nT, st) == 0
    pub = _grads(_fused, P, dev, wA.cpu(), wB.cpu())
    assert torch.equal(A, pub['A']) and torch.equal(B, pub['B'])
    assert torch.equal(grf[..., 0], pub['grad_rf']) and torch.equal(ggr, pub['grad_gr'])
    # a null cotangent is a zero one
    g2 = new(N, 2, nT, 1)
    assert lib.mrphy_ab_rfgr_bwd(code, ABck.data_ptr(), *p.k0_args(), *consts, wA.data_ptr(), None, g2.data_ptr(), None,
                                 work.data_ptr(), nbytes, N, nM, nT, st) == 0
    onlyA = _grads(_fused, P, dev, wA.cpu(), torch.zeros_like(wB).cpu())
    assert torch.equal(g2[..., 0], onlyA['grad_rf'])


# =============================================================================================
# 14. hipGraph capture
# =============================================================================================
def test_hipgraph_capture():
    r"""One design iteration on ``A, B`` (``ab_rfgr``, a loss, backward) at 16^3 x 256 captured into a HIP graph on one
    stream, as ``test_signal_mrx_hipgraph_capture`` does, and replayed once: the eager bits."""
    n, nT = 16, 256
    sp = synth.cube_spins(n, device=DEV)
    p = synth.pulse(nT, device=DEV)
    rf = (0.05 * p['rf']).clone().requires_grad_(True)
    gr = p['gr'].clone().requires_grad_(True)
    wA, wB = (dev(x).reshape(sp['M0'].shape[:-1] + s) for x, s in zip(_weights(1, n ** 3, torch.float32), ((3, 3), (3,))))

    def iteration():
        A, B = fused.ab_rfgr(rf, gr, sp['loc'], Δf=sp['Δf'], γ_beff=sp['γ'], T1=sp['T1'], T2=sp['T2'], γ=sp['γ'],
                             dt=p['dt'])
        return torch.autograd.grad((A * wA).sum() + (B * wB).sum(), (rf, gr))

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
    assert float(a0.abs().max()) > 0 and torch.equal(a0, a1) and torch.equal(b0, b1)
