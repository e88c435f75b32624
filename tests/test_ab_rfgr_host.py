r"""``fused.ab_rfgr`` without a GPU: the two entry points ``mrphy_ab_rfgr_fwd`` / ``_bwd`` are exported, declared and bound
alike and refuse bad arguments before any launch; the routing decision ``fused._decide_ab_route`` row by row; and the
fixtures ``tests/golden/ab_rfgr_f32.npz`` / ``_f64.npz`` (the live reference's ``rfgr2beff`` -> ``beff2ab`` with its own
autograd, ``tests/golden/make_golden_ab_rfgr.py``) against the CPU oracle's composition, which the GPU tests use as
their yardstick beside the fixture.

Two yardsticks for ``A, B`` and their pulse gradients live here.  ``oracle_ab`` / ``oracle_ab_beff2ab``: ``O.rfgr2beff`` ->
``O.beff2ab`` and autograd, what ``test_ab_rfgr.py`` uses -- right wherever no spin sits at zero field.
``oracle_ab_columns``: the same ``A, B`` column by column through the EXPLICIT simulator ``O.blochsim``, whose adjoint
holds the analytic zero-field limit -- what ``test_ab_operands.py`` uses, because its cases have dead time and spins at
the iso-centre, where autograd through ``F.normalize`` returns an exact 0 for gradients that are O(1)
(``test_columns_hold_the_zero_field_limit_that_beff2ab_misses``: finite differences decide)."""
import ctypes
import os
import re

import pytest
import torch

import bloch_oracle as O
import mrphy_amd
from mrphy_amd import _lib, fused
from mrphy_amd.fused import _decide_ab_route
from util import DT, FAKE, assert_close, fused_ops, golden, t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('mrphy_ab_rfgr_fwd', 'mrphy_ab_rfgr_bwd')
EINVAL = -1
SEG = 16                    # mrphy_blochsim_rfgr_ck_every()
CTYPE = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'size_t': ctypes.c_size_t, 'const void*': ctypes.c_void_p,
         'void*': ctypes.c_void_p}


def _declared(name):
    r"""(return type, [argument types]) of ``name`` as ``include/mrphy_hip.h`` declares it, as ctypes types."""
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mrphy_hip.h')).read(), flags=re.S)
    m = re.search(r'\b(\w+)\s+' + name + r'\s*\(([^)]*)\)\s*;', src)
    assert m, f'{name} is not declared in mrphy_hip.h'
    args = [re.sub(r'\s*\w+$', '', a.strip()).replace(' *', '*') for a in m.group(2).split(',')]
    return CTYPE[m.group(1)], [CTYPE[a] for a in args]


def test_symbols_are_exported_declared_and_bound_alike():
    raw = ctypes.CDLL(mrphy_amd.build())
    for name in NAMES:
        assert hasattr(raw, name), f'{name} is not exported'
        assert name in _lib.PROTOTYPES, f'{name} is not bound in _lib.py'
        res, args = _declared(name)
        assert (_lib.PROTOTYPES[name][0], list(_lib.PROTOTYPES[name][1])) == (res, args), name
    # the operands sit where the fused family's do: after dtype in the forward, after dtype and the checkpoints in the
    # adjoint, 22 arguments as mrphy_blochsim_rfgr_fwd takes them
    ops = _lib.PROTOTYPES['mrphy_blochsim_rfgr_fwd'][1][2:24]
    assert list(_lib.PROTOTYPES['mrphy_ab_rfgr_fwd'][1][1:23]) == list(ops)
    assert list(_lib.PROTOTYPES['mrphy_ab_rfgr_bwd'][1][2:24]) == list(ops)
    lib = mrphy_amd.require_library()
    assert lib.mrphy_abi_version() == _lib.ABI_VERSION == 5


def _calls(lib):
    r"""``fwd(ops, A, B, ABck, ck_every, N, nM, nT, dtype)`` and ``bwd(ops, ABck, work, work_bytes, N, nM, nT, dtype)`` with
    fake pointers (never dereferenced: no call here is valid on a problem that is not empty)."""
    fwd = lambda ops, A=FAKE, B=FAKE, ABck=None, ck=0, N=1, nM=64, nT=SEG, dtype=0: lib.mrphy_ab_rfgr_fwd(  # noqa: E731
        dtype, *ops, A, B, ABck, ck, N, nM, nT, None)
    bwd = lambda ops, ABck=FAKE, work=FAKE, wb=None, N=1, nM=64, nT=SEG, dtype=0, gA=FAKE, gB=FAKE: lib.mrphy_ab_rfgr_bwd(  # noqa: E731
        dtype, ABck, *ops, gA, gB, FAKE, FAKE, work,
        lib.mrphy_blochsim_rfgr_bwd_workspace(0, N, nM, nT) if wb is None else wb, N, nM, nT, None)
    return fwd, bwd


OPERAND_FAULTS = {
    'loc null': dict(loc=None),
    'g null': dict(g=None),
    'rf null': dict(rf=None),
    'gr null': dict(gr=None),
    'df without gamma': dict(df=FAKE),
    'E1 without E2': dict(E1=FAKE, E1m1=FAKE),
    'E2 without E1': dict(E2=FAKE, E1m1=FAKE),
    'E1 and E2 without E1m1': dict(E1=FAKE, E2=FAKE),
    'E1m1 alone': dict(E1m1=FAKE),
}


@pytest.mark.parametrize('what', list(OPERAND_FAULTS))
def test_entry_points_check_their_operands_as_the_fused_family_does(what):
    r"""The faults of ``test_fused_entry_points_check_their_operands_alike``, one operand at a time: MRPHY_EINVAL from
    both, with the adjoint's workspace whole and one byte short."""
    lib = mrphy_amd.require_library()
    fwd, bwd = _calls(lib)
    ops = fused_ops(**OPERAND_FAULTS[what])
    need = lib.mrphy_blochsim_rfgr_bwd_workspace(0, 1, 64, SEG)
    assert need > 0
    assert fwd(ops) == EINVAL
    assert bwd(ops, wb=need) == EINVAL and bwd(ops, wb=need - 1) == EINVAL


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = mrphy_amd.require_library()
    fwd, bwd = _calls(lib)
    ok = fused_ops()
    need = lib.mrphy_blochsim_rfgr_bwd_workspace(0, 1, 64, SEG)
    for dtype in (-1, 5, 17):
        assert fwd(ok, dtype=dtype) == EINVAL and bwd(ok, dtype=dtype) == EINVAL, ('unknown dtype', dtype)
    assert fwd(ok, A=None) == EINVAL and fwd(ok, B=None) == EINVAL, 'a null output'
    assert bwd(ok, ABck=None) == EINVAL and bwd(ok, work=None) == EINVAL, 'null checkpoints / workspace'
    assert fwd(ok, N=65536) == EINVAL and bwd(ok, N=65536) == EINVAL, 'N > 65535'
    assert fwd(ok, N=-1) == EINVAL and bwd(ok, nT=-SEG) == EINVAL, 'a negative size'
    for ck in (0, 4, 12, -8):
        assert fwd(ok, ABck=FAKE, ck=ck) == EINVAL, ('checkpoints every', ck)
    for nT in (1, 7, SEG + 8, 50):
        assert bwd(ok, nT=nT) == EINVAL, ('the adjoint takes whole segments', nT)
    assert bwd(ok, wb=need - 1) == EINVAL and bwd(ok, wb=0) == EINVAL, 'a short workspace'
    # ... the same with every other argument in order would be a launch: not made here


def test_empty_problems_are_a_success_whatever_the_operands_are():
    lib = mrphy_amd.require_library()
    fwd, bwd = _calls(lib)
    null = fused_ops(rf=None, gr=None, loc=None, g=None)
    assert fwd(null, A=None, B=None, nM=0) == 0 and fwd(null, A=None, B=None, N=0) == 0
    for kw in (dict(nM=0), dict(N=0), dict(nT=0)):
        assert bwd(null, ABck=None, work=None, wb=0, **kw) == 0, kw
    # the forward at nT == 0 with spins is NOT empty (it writes A = I, B = 0): it wants its outputs and loc, g -- but
    # no pulse
    assert fwd(fused_ops(rf=None, gr=None), A=None, nT=0) == EINVAL
    assert fwd(fused_ops(rf=None, gr=None, g=None), nT=0) == EINVAL


def test_python_wrapper_refuses_cpu_tensors():
    rf, gr, loc = torch.zeros(1, 2, SEG), torch.zeros(1, 3, SEG), torch.zeros(1, 5, 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.ab_rfgr(rf, gr, loc)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.ab_rfgr(rf.requires_grad_(True), gr, loc, T1=torch.ones(1, 5), T2=torch.ones(1, 5))
    assert 'ab_rfgr' in fused.__all__


# ---------------------------------------------------------------------------------------------
# the routing decision, row by row
# ---------------------------------------------------------------------------------------------
ONE = dict(seg=SEG, one_coil=True, pulse_grad=False, maps_grad=False, consts_grad=False)
ROUTES = [
    ('one coil, nT 48, no gradient', dict(ONE, nT=48), ('fused', False)),
    ('one coil, nT 50, no gradient', dict(ONE, nT=50), ('fused', False)),
    ('one coil, nT 7, no gradient', dict(ONE, nT=7), ('fused', False)),
    ('one coil, nT 48, pulse gradient', dict(ONE, nT=48, pulse_grad=True), ('fused', True)),
    ('one coil, nT 50, pulse gradient', dict(ONE, nT=50, pulse_grad=True), ('split', 48)),
    ('one coil, nT 8, pulse gradient', dict(ONE, nT=8, pulse_grad=True), ('composed', None)),
    ('a map gradient', dict(ONE, nT=48, maps_grad=True), ('composed', None)),
    ('a map gradient beside a pulse gradient', dict(ONE, nT=48, pulse_grad=True, maps_grad=True), ('composed', None)),
    ("a constants' gradient", dict(ONE, nT=48, consts_grad=True), ('composed', None)),
    ("a constants' gradient beside a pulse gradient, nT 50", dict(ONE, nT=50, pulse_grad=True, consts_grad=True),
     ('composed', None)),
    ('4 coils', dict(ONE, nT=48, one_coil=False), ('composed', None)),
    ('4 coils, pulse gradient, nT 50', dict(ONE, nT=50, one_coil=False, pulse_grad=True), ('composed', None)),
    ('one coil, nT 16, pulse gradient', dict(ONE, nT=16, pulse_grad=True), ('fused', True)),
    ('one coil, nT 17, pulse gradient', dict(ONE, nT=17, pulse_grad=True), ('split', 16)),
    ('one coil, nT 0, pulse gradient', dict(ONE, nT=0, pulse_grad=True), ('fused', True)),
]


@pytest.mark.parametrize('what, facts, route', ROUTES, ids=[r[0] for r in ROUTES])
def test_ab_route(what, facts, route):
    assert _decide_ab_route(**facts) == route


# ---------------------------------------------------------------------------------------------
# the fixture from the reference against the oracle's composition
# ---------------------------------------------------------------------------------------------
def oracle_ab(P, dtype=None):
    r"""``A, B, grad_rf, grad_gr`` of the loss ``(A wA).sum() + (B wB).sum()`` by the CPU oracle's ``rfgr2beff`` ->
    ``beff2ab`` and autograd, on the inputs ``P`` of a fixture (``in.*``), widened to ``dtype`` if given."""
    P = {k: (v if dtype is None else v.to(dtype)) for k, v in P.items()}
    rf, gr = P['rf'].clone().requires_grad_(True), P['gr'].clone().requires_grad_(True)
    beff = O.rfgr2beff(rf, gr, P['loc'], Δf=P['df'], b1Map=P['b1'], γ=P['γ'])
    A, B = O.beff2ab(beff, E1=P['E1'], E2=P['E2'], γ=P['γ'], dt=P['dt'])
    ((A * P['wA']).sum() + (B * P['wB']).sum()).backward()
    return dict(A=A.detach(), B=B.detach(), grad_rf=rf.grad, grad_gr=gr.grad)


def fixture_inputs(G):
    return {k[3:]: t(v) for k, v in G.items() if k.startswith('in.')}


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_oracle_composition_matches_the_reference_fixture(tag):
    G = golden(f'ab_rfgr_{tag}')
    P = fixture_inputs(G)
    assert P['rf'].shape == (2, 2, 48) and P['loc'].shape == (2, 100, 3) and P['b1'].shape == (2, 100, 2)
    assert all(v.dtype == DT[tag] for v in P.values())
    for dtype, who in ((None, 'the oracle in the data type'), (torch.float64, 'the oracle in fp64')):
        got = oracle_ab(P, dtype)
        for k in ('A', 'B', 'grad_rf', 'grad_gr'):
            assert got[k].shape == G[k].shape
            assert_close(got[k], G[k], tag, f'{who}: {k}')
    if tag == 'f32':
        # the generator's condition: the reference's own fp32 run is the function to a tenth of the gate
        assert max(float(G[f'distance_f32_vs_f64.{k}']) for k in ('A', 'B', 'grad_rf', 'grad_gr')) <= 1e-6


# ---------------------------------------------------------------------------------------------
# the column yardstick: A, B from the explicit adjoint, which holds the analytic zero-field limit
# ---------------------------------------------------------------------------------------------
def _wide(x, dtype=torch.float64):
    return None if x is None else x.detach().to(dtype)


def oracle_ab_columns(v, rf=None, gr=None, dtype=torch.float64):
    r"""``A, B`` of the operand dict ``v`` (keys as ``cases.fused_operand_variants``: ``rf, gr, loc, Δf, b1Map, γ_beff, T1,
    T2, γ, dt``, each in any form the simulators take) in fp64 from ``O.rfgr2beff`` and the EXPLICIT simulator:
    ``B = O.blochsim(0, beff, ...)`` and ``A[..., :, j] = O.blochsim(e_j, beff, ...) - B``, the four columns as four
    batch entries of one call.  Differentiable w.r.t. ``rf`` and ``gr`` when they are handed over as fp64 leaves.

    This is the yardstick of the GPU tests of ``fused.ab_rfgr`` / ``steadystate_rfgr`` (``test_ab_operands.py``), not
    ``O.beff2ab``: ``beff2ab`` is differentiated by autograd through ``F.normalize`` and returns an exact 0 for the field
    gradient of every step at which a spin sits at zero field, where the true value is the limit ``-γ2πdt (m x h̃)`` of
    ``O.explicit_backward`` (``test_columns_hold_the_zero_field_limit_that_beff2ab_misses``: finite differences side
    with the columns).  Their VALUES are the same function (``test_column_yardstick_is_beff2ab``: 1e-12).  ``dtype``: the
    same chain in another precision (fp32: what an all-fp32 evaluation of this very chain loses, the measure of the fp32
    margins of ``test_ab_operands.py``)."""
    P = {k: _wide(v.get(k), dtype) for k in ('loc', 'Δf', 'b1Map', 'γ_beff', 'T1', 'T2', 'γ', 'dt')}
    rf, gr = (_wide(v['rf'], dtype) if rf is None else rf), (_wide(v['gr'], dtype) if gr is None else gr)
    beff = O.rfgr2beff(rf, gr, P['loc'], Δf=P['Δf'], b1Map=P['b1Map'], γ=P['γ_beff'])
    lead = tuple(beff.shape[:-2])
    Mi = torch.zeros((4,) + lead + (3,), dtype=dtype)
    for j in range(3):
        Mi[j, ..., j] = 1
    # the columns as batch entries: whatever runs over the batch is repeated, whatever broadcasts over it stays
    rep = lambda x: x if x is None or x.ndim == 0 or x.shape[0] == 1 else torch.cat([x] * 4, 0)  # noqa: E731
    Mo = O.blochsim(Mi.reshape((4 * lead[0],) + lead[1:] + (3,)), torch.cat([beff] * 4, 0), T1=rep(P['T1']),
                    T2=rep(P['T2']), γ=rep(P['γ']), dt=rep(P['dt']))
    Mo = Mo.reshape((4,) + lead + (3,))
    return torch.stack([Mo[j] - Mo[3] for j in range(3)], dim=-1), Mo[3]


def oracle_ab_beff2ab(v, rf=None, gr=None):
    r"""The same ``A, B`` by ``O.rfgr2beff`` -> ``O.beff2ab`` (autograd): the yardstick of ``test_ab_rfgr.py``, right
    wherever no spin sits at zero field."""
    P = {k: _wide(v.get(k)) for k in ('loc', 'Δf', 'b1Map', 'γ_beff', 'T1', 'T2', 'γ', 'dt')}
    rf, gr = (_wide(v['rf']) if rf is None else rf), (_wide(v['gr']) if gr is None else gr)
    beff = O.rfgr2beff(rf, gr, P['loc'], Δf=P['Δf'], b1Map=P['b1Map'], γ=P['γ_beff'])
    k = beff.ndim - 2
    dt = O._rpad(P['dt'], k)
    one = torch.ones((), dtype=torch.float64)
    E1, E2 = (one, one) if P['T1'] is None else (torch.exp(-dt / O._rpad(P['T1'], k)), torch.exp(-dt / O._rpad(P['T2'], k)))
    return O.beff2ab(beff, E1=E1, E2=E2, γ=P['γ'], dt=P['dt'])


def ab_weights(v):
    r"""The cotangents of the operand tests, formed from the case's own ``w``: ``wB = w`` and ``wA = w[..., None] * (0.9,
    -0.6, 0.4)`` in the FORM of ``w`` -- a ``w`` that starts one element into its buffer gives a ``wA`` that does, a
    non-contiguous ``w`` a non-contiguous ``wA``."""
    w = v['w']
    wA = (w[..., None] * torch.tensor([0.9, -0.6, 0.4], dtype=w.dtype)).contiguous()
    if w.storage_offset():
        buf = torch.zeros(wA.numel() + w.storage_offset() + 3, dtype=w.dtype)
        buf[w.storage_offset():w.storage_offset() + wA.numel()].view(wA.shape).copy_(wA)
        wA = buf[w.storage_offset():w.storage_offset() + wA.numel()].view(wA.shape)
    elif not w.is_contiguous():
        wA = wA.movedim(-1, 0).contiguous().movedim(0, -1)
    return wA, w


def oracle_ab_grads(v, ab=oracle_ab_columns, wA=None, wB=None):
    r"""``A, B, grad_rf, grad_gr`` of ``(A wA).sum() + (B wB).sum()`` in fp64 through ``ab``; the gradients in the shapes of
    ``rf`` and ``gr`` as given."""
    if wA is None:
        wA, wB = ab_weights(v)
    rf, gr = _wide(v['rf']).clone().requires_grad_(True), _wide(v['gr']).clone().requires_grad_(True)
    A, B = ab(v, rf, gr)
    ((A * _wide(wA)).sum() + (B * _wide(wB)).sum()).backward()
    return dict(A=A.detach(), B=B.detach(), grad_rf=rf.grad, grad_gr=gr.grad)


def oracle_steadystate_columns(v, rest, T1, T2, df, dtype=torch.float64):
    r"""``Mss, grad_rf, grad_gr`` of ``(Mss w).sum()``: ``test_steadystate_host.torch_steadystate`` on the column
    yardstick's ``A, B`` of ``v`` (whose ``T1, T2`` the caller has set to those of the rest period), all in ``dtype``.
    ``T1, T2, df``: broadcastable against the spins ``(N, *Nd)`` from the left, as the simulators take them."""
    from test_steadystate_host import torch_steadystate
    rf, gr = _wide(v['rf'], dtype).clone().requires_grad_(True), _wide(v['gr'], dtype).clone().requires_grad_(True)
    A, B = oracle_ab_columns(v, rf, gr, dtype)
    k = B.ndim - 1
    pad = lambda x: None if x is None else O._rpad(_wide(x, dtype), k) if x.ndim else _wide(x, dtype)  # noqa: E731
    Mss = torch_steadystate(A, B, _wide(rest, dtype), pad(T1), pad(T2), pad(df))
    (Mss * _wide(v['w'], dtype)).sum().backward()
    return dict(Mss=Mss.detach(), grad_rf=rf.grad, grad_gr=gr.grad)


def zero_field_masks(v):
    r"""``(live_rf, live_gr)``, boolean `(N, nT)`, read from the case: the pulse samples at which autograd through
    ``F.normalize`` still gives the right ``grad_rf`` / ``grad_gr`` -- no spin of the batch entry sits at zero field there,
    except spins whose own factor on that gradient is an exact zero anyway (``b1Map = 0`` for ``rf``; ``loc = 0`` for
    ``gr``: the iso-centre spins on the pure-``gr`` samples of ``ZERO_RF_ONLY``)."""
    beff = O.rfgr2beff(_wide(v['rf']), _wide(v['gr']), _wide(v['loc']), Δf=_wide(v['Δf']), b1Map=_wide(v['b1Map']),
                       γ=_wide(v['γ_beff']))
    dead = (beff == 0).all(dim=-1)                                               # (N, nM, nT)
    loc0 = (_wide(v['loc']) == 0).all(dim=-1)[..., None]
    b10 = torch.zeros_like(loc0) if v['b1Map'] is None else (_wide(v['b1Map']).reshape(loc0.shape[:2] + (-1,)) == 0).all(-1)[..., None]
    return ~(dead & ~b10).any(dim=1), ~(dead & ~loc0).any(dim=1)


ZERO_FIELD_CASES = [(nC, nT) for nC in (0, 1) for nT in (48, 53)]
FD_SAMPLES = ((0, 2), (1, 15), (0, 17), (1, 46)) + ((1, 20), (1, 29))   # four inside ZERO_STEPS, two inside ZERO_SEGMENT


def _zero_case(nC, nT):
    import cases
    v, zero = cases.zero_field_case(torch.float64, nC, nT)
    gen = torch.Generator().manual_seed(4000 + 10 * nC + nT)
    N, nM = v['loc'].shape[:2]
    wA = torch.rand((N, nM, 3, 3), generator=gen, dtype=torch.float64) * 2 - 1
    wB = torch.rand((N, nM, 3), generator=gen, dtype=torch.float64) * 2 - 1
    return cases, v, zero, wA, wB


@pytest.mark.parametrize('nC,nT', ZERO_FIELD_CASES)
def test_column_yardstick_is_beff2ab(nC, nT):
    r"""On the zero-field case: ``A, B`` of the two yardsticks to 1e-12, and the gradients of a seeded ``(A wA).sum() + (B
    wB).sum()`` to 1e-9 on every pulse sample the case leaves live (:func:`zero_field_masks`)."""
    cases, v, zero, wA, wB = _zero_case(nC, nT)
    col, b2a = oracle_ab_grads(v, oracle_ab_columns, wA, wB), oracle_ab_grads(v, oracle_ab_beff2ab, wA, wB)
    for k in ('A', 'B'):
        assert float((col[k] - b2a[k]).abs().max()) <= 1e-12, k
    live_rf, live_gr = zero_field_masks(v)
    # the masks are the case's: dead time takes both out, the pure-gr samples only grad_rf -- and not even that in batch
    # entry 1 with a map, whose one iso-centre spin has b1Map = 0
    rf_only = torch.zeros_like(zero)
    rf_only[:1 if nC else 2, list(cases.ZERO_RF_ONLY)] = True
    assert torch.equal(live_gr, ~zero) and torch.equal(live_rf, ~zero & ~rf_only)
    assert int(live_rf.sum()) >= 40 and int(live_gr.sum()) > int(live_rf.sum())
    for k, live in (('grad_rf', live_rf), ('grad_gr', live_gr)):
        a, b = col[k].movedim(2, 1)[live], b2a[k].movedim(2, 1)[live]
        assert float(a.abs().max()) > 0.1
        assert float((a - b).abs().max()) <= 1e-9, k


@pytest.mark.parametrize('nC,nT', ZERO_FIELD_CASES)
def test_columns_hold_the_zero_field_limit_that_beff2ab_misses(nC, nT):
    r"""Central finite differences in fp64 (h = 1e-4 G, G/cm: the loss is smooth in ``γ2πdt b``, 0.1 rad per Gauss, so the
    truncation error is O(1e-11) and the rounding error O(1e-10)) on the five components of six dead pulse samples: within
    1e-6 relative of the column yardstick; ``O.beff2ab``'s autograd holds an exact zero there -- a distance of 1.

    Dry run (nC = 0 / 1; nT = 48, 53): over the dead samples the columns' ``grad_rf`` reaches 1.4, 3.2 / 1.1, 2.0 and
    ``grad_gr`` 7.9, 9.3 / 2.2, 9.8 in max abs where ``beff2ab`` gives 0; over the whole gradients the two yardsticks are
    0.43 .. 0.78 apart in relative L2.  A kernel held to ``beff2ab`` there would have to return zeros, more than 4e4 fp32
    gates (1e9 fp64 gates) away from the truth."""
    cases, v, zero, wA, wB = _zero_case(nC, nT)
    col, b2a = oracle_ab_grads(v, oracle_ab_columns, wA, wB), oracle_ab_grads(v, oracle_ab_beff2ab, wA, wB)
    h = 1e-4

    def loss(rf, gr):
        with torch.no_grad():
            A, B = oracle_ab_columns(v, rf, gr)
            return float((A * wA).sum() + (B * wB).sum())

    for n, t_ in FD_SAMPLES:
        assert bool(zero[n, t_]) and (t_ in cases.ZERO_STEPS or (n == 1 and t_ in cases.ZERO_SEGMENT))
        fd = []
        for name, ncomp in (('rf', 2), ('gr', 3)):
            for c in range(ncomp):
                x = {k: _wide(v[k]).clone() for k in ('rf', 'gr')}
                x[name][n, c, t_] = h
                up = loss(x['rf'], x['gr'])
                x[name][n, c, t_] = -h
                fd.append((up - loss(x['rf'], x['gr'])) / (2 * h))
        fd = torch.tensor(fd, dtype=torch.float64)
        want = torch.cat((col['grad_rf'][n, :, t_], col['grad_gr'][n, :, t_]))
        auto = torch.cat((b2a['grad_rf'][n, :, t_], b2a['grad_gr'][n, :, t_]))
        assert float(fd.norm()) > 0.1, (n, t_)
        assert float((fd - want).norm() / fd.norm()) <= 1e-6, (n, t_, fd, want)
        assert float(auto.abs().max()) == 0.0 and float((fd - auto).norm() / fd.norm()) > 0.5, (n, t_, auto)
    dead = zero
    assert float(b2a['grad_rf'].movedim(2, 1)[dead].abs().max()) == 0.0 == float(b2a['grad_gr'].movedim(2, 1)[dead].abs().max())
    assert float(col['grad_rf'].movedim(2, 1)[dead].abs().max()) > 0.1 < float(col['grad_gr'].movedim(2, 1)[dead].abs().max())
