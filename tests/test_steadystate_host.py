r"""``fused.ab_steadystate`` / ``fused.steadystate_rfgr`` without a GPU: the two entry points ``mrphy_ab_steadystate_fwd`` /
``_bwd`` are exported, declared and bound alike and refuse bad arguments before any launch; the Python layer refuses CPU
tensors and a call without relaxation; and the fixtures ``tests/golden/steadystate_f32.npz`` / ``_f64.npz`` (the live
reference iterated to its steady state, ``tests/golden/make_golden_steadystate.py``) against the CPU oracle's composition
``rfgr2beff`` -> ``beff2ab`` -> ``torch.linalg.solve``, which the GPU tests use as their yardstick beside the fixture."""
import ctypes
from math import pi as π

import pytest
import torch

import bloch_oracle as O
import mrphy_amd
from mrphy_amd import _lib, fused
from test_ab_rfgr_host import _declared, fixture_inputs
from util import FAKE, assert_close, golden

NAMES = ('mrphy_ab_steadystate_fwd', 'mrphy_ab_steadystate_bwd')
EINVAL, EALIGN = -1, -2
BC0 = (None, 0, 0)
BCF = (FAKE, 0, 0)


# ---------------------------------------------------------------------------------------------
# the yardstick: the rest period and the solve in plain torch (any device, differentiable)
# ---------------------------------------------------------------------------------------------
def rest_period(like, rest=None, T1=None, T2=None, df=None):
    r"""``F`` (..., 3, 3), ``f`` (..., 3) of ``sims.freeprec(M, rest, T1=T1, T2=T2, Δf=df)``, ``M⁻ = F M + f``, broadcast
    over the spins ``like.shape[:-1]`` (``like``: B); absent operands as ``freeprec`` treats them; ``rest`` `()` ⊻ `(N,)`,
    the others broadcastable to the spins."""
    shape = like.shape[:-1]
    one, o = like.new_ones(shape), like.new_zeros(shape)
    if rest is None:
        return torch.eye(3, dtype=like.dtype, device=like.device).expand(shape + (3, 3)), like.new_zeros(shape + (3,))
    rest = rest.reshape(rest.shape + (1,) * (len(shape) - rest.ndim)) if rest.ndim else rest
    φ = o if df is None else -2 * π * df * rest * one
    E1r, E2r = (one, one) if T1 is None else (torch.exp(-rest / T1) * one, torch.exp(-rest / T2) * one)
    f3 = o if T1 is None else -torch.expm1(-rest / T1) * one
    c, s = torch.cos(φ), torch.sin(φ)
    F = torch.stack((torch.stack((E2r * c, -E2r * s, o), -1), torch.stack((E2r * s, E2r * c, o), -1),
                     torch.stack((o, o, E1r), -1)), -2)
    return F, torch.stack((o, o, f3), -1)


def torch_steadystate(A, B, rest=None, T1=None, T2=None, df=None):
    r"""``Mss`` of ``(I - A F) Mss = A f + B`` by ``torch.linalg.solve``."""
    F, f = rest_period(B, rest, T1, T2, df)
    C = torch.eye(3, dtype=A.dtype, device=A.device) - A @ F
    return torch.linalg.solve(C, (A @ f[..., None])[..., 0] + B)


def oracle_steadystate(P, dtype=None):
    r"""``Mss, grad_rf, grad_gr`` of the loss ``(Mss w).sum()`` by the CPU oracle's ``rfgr2beff`` -> ``beff2ab``, the torch
    solve and autograd, on the inputs ``P`` of a fixture (``in.*``), widened to ``dtype`` if given."""
    P = {k: (v if dtype is None else v.to(dtype)) for k, v in P.items()}
    rf, gr = P['rf'].clone().requires_grad_(True), P['gr'].clone().requires_grad_(True)
    beff = O.rfgr2beff(rf, gr, P['loc'], Δf=P['df'], b1Map=P['b1'], γ=P['γ'])
    A, B = O.beff2ab(beff, E1=P['E1'], E2=P['E2'], γ=P['γ'], dt=P['dt'])
    Mss = torch_steadystate(A, B, P['rest'], P['T1'], P['T2'], P['df'])
    (Mss * P['w']).sum().backward()
    return dict(Mss=Mss.detach(), grad_rf=rf.grad, grad_gr=gr.grad)


# ---------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------
def test_symbols_are_exported_declared_and_bound_alike():
    raw = ctypes.CDLL(mrphy_amd.build())
    for name in NAMES:
        assert hasattr(raw, name), f'{name} is not exported'
        assert name in _lib.PROTOTYPES, f'{name} is not bound in _lib.py'
        res, args = _declared(name)
        assert (_lib.PROTOTYPES[name][0], list(_lib.PROTOTYPES[name][1])) == (res, args), name
    # rest, T1, T2, df sit where dur, T1, T2, df of mrphy_freeprec_fwd do: after the leading data pointers
    rest_ops = _lib.PROTOTYPES['mrphy_freeprec_fwd'][1][2:13]
    assert list(_lib.PROTOTYPES[NAMES[0]][1][3:14]) == list(rest_ops)
    assert list(_lib.PROTOTYPES[NAMES[1]][1][4:15]) == list(rest_ops)
    lib = mrphy_amd.require_library()
    assert lib.mrphy_abi_version() == _lib.ABI_VERSION == 5
    assert ('tu_ab_steady.hip', None) in _lib.UNITS


def _calls(lib):
    r"""``fwd(...)`` / ``bwd(...)`` with fake pointers (never dereferenced: no call here is valid on a problem that is not
    empty and well-formed enough to launch)."""
    def fwd(A=FAKE, B=FAKE, rest=FAKE, T1=BCF, T2=BCF, df=BCF, Mss=FAKE, N=2, nM=100, dtype=0):
        return lib.mrphy_ab_steadystate_fwd(dtype, A, B, rest, 0, *T1, *T2, *df, Mss, N, nM, None)

    def bwd(A=FAKE, B=FAKE, g=FAKE, rest=FAKE, T1=BCF, T2=BCF, df=BCF, gA=FAKE, gB=FAKE, gC=FAKE, N=2, nM=100, dtype=0):
        return lib.mrphy_ab_steadystate_bwd(dtype, A, B, g, rest, 0, *T1, *T2, *df, gA, gB, gC, N, nM, None)
    return fwd, bwd


OPERAND_FAULTS = {
    'A null': dict(A=None),
    'B null': dict(B=None),
    'T1 without a rest': dict(rest=None, df=BC0),
    'df without a rest': dict(rest=None, T1=BC0, T2=BC0),
    'T1, T2, df without a rest': dict(rest=None),
    'T1 without T2': dict(T2=BC0),
    'T2 without T1': dict(T1=BC0),
    'T2 without T1 nor df': dict(T1=BC0, df=BC0),
}


@pytest.mark.parametrize('what', list(OPERAND_FAULTS))
def test_entry_points_check_their_operands_alike(what):
    fwd, bwd = _calls(mrphy_amd.require_library())
    for dtype in (0, 1):
        assert fwd(dtype=dtype, **OPERAND_FAULTS[what]) == EINVAL
        assert bwd(dtype=dtype, **OPERAND_FAULTS[what]) == EINVAL


def test_entry_points_refuse_bad_arguments_before_any_launch():
    fwd, bwd = _calls(mrphy_amd.require_library())
    for dtype in (-1, 2, 3, 4, 5, 17):          # data types only: the codes mrphy_freeprec_* accept
        assert fwd(dtype=dtype) == EINVAL and bwd(dtype=dtype) == EINVAL, ('dtype', dtype)
    assert fwd(N=-1) == EINVAL and fwd(nM=-1) == EINVAL and bwd(N=-2) == EINVAL and bwd(nM=-100) == EINVAL
    assert fwd(Mss=None) == EINVAL, 'a null output'
    assert bwd(g=None) == EINVAL, 'a null cotangent'
    assert bwd(gA=None, gB=None, gC=None) == EINVAL, 'nothing to compute'
    for dtype, odd in ((0, FAKE + 2), (1, FAKE + 4)):
        for k in ('A', 'B', 'rest', 'Mss'):
            assert fwd(dtype=dtype, **{k: odd}) == EALIGN, (dtype, k)
        for k in ('T1', 'T2', 'df'):
            assert fwd(dtype=dtype, **{k: (odd, 0, 0)}) == EALIGN and bwd(dtype=dtype, **{k: (odd, 0, 0)}) == EALIGN
        for k in ('A', 'B', 'g', 'rest', 'gA', 'gB', 'gC'):
            assert bwd(dtype=dtype, **{k: odd}) == EALIGN, (dtype, k)
    # ... a call right in every argument would be a launch: not made here


def test_empty_problems_are_a_success_whatever_the_pointers_are():
    fwd, bwd = _calls(mrphy_amd.require_library())
    null = dict(A=None, B=None, rest=None, T1=BCF, T2=BC0, df=BCF)
    for size in (dict(nM=0), dict(N=0), dict(N=0, nM=0)):
        assert fwd(Mss=None, **null, **size) == 0, size
        assert bwd(g=None, gA=None, gB=None, gC=None, **null, **size) == 0, size
    assert fwd(nM=0, dtype=7) == EINVAL and bwd(N=0, nM=-1) == EINVAL    # ... but not whatever the dtype and sizes are


# ---------------------------------------------------------------------------------------------
# the Python layer
# ---------------------------------------------------------------------------------------------
def test_python_wrappers_refuse_cpu_tensors():
    A, B = torch.eye(3).expand(1, 5, 3, 3) * 0.9, torch.zeros(1, 5, 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.ab_steadystate(A, B)
    rf, gr, loc = torch.zeros(1, 2, 16), torch.zeros(1, 3, 16), torch.zeros(1, 5, 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.steadystate_rfgr(rf, gr, loc, rest=torch.tensor(5e-3), T1=torch.ones(1, 5), T2=torch.ones(1, 5))
    assert 'ab_steadystate' in fused.__all__ and 'steadystate_rfgr' in fused.__all__


def test_steadystate_rfgr_needs_relaxation():
    rf, gr, loc = torch.zeros(1, 2, 16), torch.zeros(1, 3, 16), torch.zeros(1, 5, 3)
    T = torch.ones(1, 5)
    for kw in (dict(rest=torch.tensor(5e-3), T2=T), dict(rest=torch.tensor(5e-3), T1=T), dict(T1=T, T2=T),
               dict(rest=torch.tensor(5e-3))):
        with pytest.raises(AssertionError, match='needs relaxation'):
            fused.steadystate_rfgr(rf, gr, loc, **kw)


# ---------------------------------------------------------------------------------------------
# the fixture from the reference against the oracle's composition
# ---------------------------------------------------------------------------------------------
def test_oracle_composition_matches_the_reference_fixture():
    G = golden('steadystate_f64')
    P = fixture_inputs(G)
    assert P['rf'].shape == (2, 2, 48) and P['loc'].shape == (2, 100, 3) and P['b1'].shape == (2, 100, 2)
    assert P['rest'].tolist() == [5e-3, 6.5e-3] and P['w'].shape == (2, 100, 3)
    assert 0.05 <= float(P['T1'].min()) and float(P['T1'].max()) <= 0.15
    assert 0.02 <= float(P['T2'].min()) and float(P['T2'].max()) <= 0.07
    assert all(v.dtype == torch.float64 for v in P.values())
    got = oracle_steadystate(P)
    for k in ('Mss', 'grad_rf', 'grad_gr'):
        assert got[k].shape == G[k].shape
        assert_close(got[k], G[k], 'f64', f'the oracle: {k}')
    assert float(G['kappa_max']) <= 100


def test_fp32_fixture_holds_the_distances_the_generator_printed():
    r"""``distance_f32_vs_f64.*``: the reference's all-fp32 closed form against its fp64 run on the same fp32 numbers
    (last run of the generator, its docstring) -- and they are what the stored fp32 outputs are from the fp64 oracle on
    the stored fp32 inputs."""
    G = golden('steadystate_f32')
    P = fixture_inputs(G)
    assert all(v.dtype == torch.float32 for v in P.values()) and G['Mss'].dtype == 'float32'
    printed = dict(Mss=3.246e-06, grad_rf=2.492e-06, grad_gr=3.554e-06)
    wide = oracle_steadystate(P, torch.float64)
    for k, d in printed.items():
        stored = float(G[f'distance_f32_vs_f64.{k}'])
        assert abs(stored - d) <= 5e-10, (k, stored, d)
        here = float((torch.from_numpy(G[k]).double() - wide[k]).norm() / wide[k].norm())
        assert abs(here - stored) <= 0.02 * stored, (k, here, stored)
    assert float(G['kappa_max']) <= 100
