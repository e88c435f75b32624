r"""``fused.ab_rfgr`` without a GPU: the two entry points ``mrphy_ab_rfgr_fwd`` / ``_bwd`` are exported, declared and bound
alike and refuse bad arguments before any launch; the routing decision ``fused._decide_ab_route`` row by row; and the
fixtures ``tests/golden/ab_rfgr_f32.npz`` / ``_f64.npz`` (the live reference's ``rfgr2beff`` -> ``beff2ab`` with its own
autograd, ``tests/golden/make_golden_ab_rfgr.py``) against the CPU oracle's composition, which the GPU tests use as
their yardstick beside the fixture."""
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
