r"""``fused.ab_train`` / ``fused.train_rfgr`` without a GPU: the two entry points ``mrphy_ab_train_fwd`` / ``_bwd`` are
exported, declared and bound alike and refuse bad arguments before any launch; the Python layer refuses CPU tensors and
an unknown or contradictory number of repetitions; the fixtures ``tests/golden/train_f32.npz`` / ``_f64.npz`` (the live
reference's ``freeprec`` -> ``rfgr2beff(rf e^{iφ_k})`` -> ``blochsim``, K times: ``tests/golden/make_golden_train.py``)
against the yardstick of the GPU tests -- the recursion in plain torch (:func:`torch_train`) on the CPU oracle's
``rfgr2beff`` -> ``beff2ab`` --; and two identities of that yardstick which the GPU tests reuse as known answers."""
import ctypes
from math import pi as π

import pytest
import torch

import bloch_oracle as O
import mrphy_amd
from mrphy_amd import _lib, fused
from test_ab_rfgr_host import _declared, fixture_inputs
from test_steadystate_host import rest_period, torch_steadystate
from util import FAKE, assert_close, golden

NAMES = ('mrphy_ab_train_fwd', 'mrphy_ab_train_bwd')
EINVAL, EALIGN = -1, -2
BC0 = (None, 0, 0)
BCF = (FAKE, 0, 0)


# ---------------------------------------------------------------------------------------------
# the yardstick: the recursion in plain torch (any device, differentiable)
# ---------------------------------------------------------------------------------------------
def rz(M, φ):
    r"""``Rz(φ) M``: ``M`` (..., 3), ``φ`` broadcastable to ``M.shape[:-1]``."""
    c, s = torch.cos(φ), torch.sin(φ)
    return torch.stack((c * M[..., 0] - s * M[..., 1], s * M[..., 0] + c * M[..., 1], M[..., 2] + 0 * c), -1)


def torch_train(A, B, K, Mi=None, phase=None, rest=None, T1=None, T2=None, df=None):
    r"""``Mt`` `(N, *Nd, K, 3)`: from ``M_0 = Mi`` (default ``(0, 0, 1)``), ``M⁻ = F M_k + f`` (``rest_period``), then
    ``M_{k+1} = Rz(φ_k) [A Rz(-φ_k) M⁻ + B]``, ``Rz`` applied explicitly, K times in a loop.  ``phase`` `(N ⊻ 1, K)` or
    ``None`` (zeros); the rest's operands as ``rest_period`` takes them."""
    F, f = rest_period(B, rest, T1, T2, df)
    M = torch.zeros_like(B)
    M[..., 2] = 1
    if Mi is not None:
        M = Mi.expand(B.shape)
    out = []
    for k in range(K):
        Mm = (F @ M[..., None])[..., 0] + f
        if phase is None:
            M = (A @ Mm[..., None])[..., 0] + B
        else:
            φ = phase[:, k].reshape((-1,) + (1,) * (B.ndim - 2))
            M = rz((A @ rz(Mm, -φ)[..., None])[..., 0] + B, φ)
        out.append(M)
    if not out:
        return B.new_zeros(B.shape[:-1] + (0, 3))
    return torch.stack(out, dim=-2)


def oracle_train(P, dtype=None):
    r"""``Mt, grad_rf, grad_gr, grad_T1`` of the loss ``(Mt w).sum()`` (``w`` time-major) by the CPU oracle's ``rfgr2beff``
    -> ``beff2ab`` of the pulse as it is, :func:`torch_train` and autograd, on the inputs ``P`` of a fixture (``in.*``),
    widened to ``dtype`` if given.  ``T1`` is shared by the pulse (``E1 = exp(-dt/T1)``) and the rest."""
    P = {k: (v if dtype is None else v.to(dtype)) for k, v in P.items()}
    rf, gr, T1 = (P[k].clone().requires_grad_(True) for k in ('rf', 'gr', 'T1'))
    beff = O.rfgr2beff(rf, gr, P['loc'], Δf=P['df'], b1Map=P['b1'], γ=P['γ'])
    A, B = O.beff2ab(beff, E1=torch.exp(-P['dt'][:, None] / T1), E2=torch.exp(-P['dt'][:, None] / P['T2']), γ=P['γ'],
                     dt=P['dt'])
    Mt = torch_train(A, B, P['phase'].shape[1], None, P['phase'], P['rest'], T1, P['T2'], P['df'])
    (Mt.movedim(-2, 0) * P['w']).sum().backward()
    return dict(Mt=Mt.detach(), grad_rf=rf.grad, grad_gr=gr.grad, grad_T1=T1.grad)


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
    # rest, T1, T2, df sit where mrphy_ab_steadystate_* have them
    assert list(_lib.PROTOTYPES[NAMES[0]][1][:15]) == list(_lib.PROTOTYPES['mrphy_ab_steadystate_fwd'][1][:15])
    assert list(_lib.PROTOTYPES[NAMES[1]][1][:16]) == list(_lib.PROTOTYPES['mrphy_ab_steadystate_bwd'][1][:16])
    lib = mrphy_amd.require_library()
    assert lib.mrphy_abi_version() == _lib.ABI_VERSION == 5
    assert ('tu_ab_train.hip', None) in _lib.UNITS


def _calls(lib):
    r"""``fwd(...)`` / ``bwd(...)`` with fake pointers (never dereferenced: no call here is valid on a problem that is not
    empty and well-formed enough to launch)."""
    def fwd(A=FAKE, B=FAKE, rest=FAKE, T1=BCF, T2=BCF, df=BCF, Mi=BCF, cs=FAKE, Mt=FAKE, N=2, nM=100, K=5, dtype=0):
        return lib.mrphy_ab_train_fwd(dtype, A, B, rest, 0, *T1, *T2, *df, *Mi, cs, 0, Mt, N, nM, K, None)

    def bwd(A=FAKE, B=FAKE, g=FAKE, rest=FAKE, T1=BCF, T2=BCF, df=BCF, Mi=BCF, cs=FAKE, Mt=FAKE, gA=FAKE, gB=FAKE,
            gC=FAKE, gMi=FAKE, gphi=FAKE, N=2, nM=100, K=5, dtype=0):
        return lib.mrphy_ab_train_bwd(dtype, A, B, g, rest, 0, *T1, *T2, *df, *Mi, cs, 0, Mt, gA, gB, gC, gMi, gphi,
                                      N, nM, K, None)
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
    for dtype in (-1, 2, 3, 4, 5, 17):          # data types only, as mrphy_ab_steadystate_*
        assert fwd(dtype=dtype) == EINVAL and bwd(dtype=dtype) == EINVAL, ('dtype', dtype)
    assert fwd(N=-1) == EINVAL and fwd(nM=-1) == EINVAL and bwd(N=-2) == EINVAL and bwd(nM=-100) == EINVAL
    assert fwd(K=-1) == EINVAL and bwd(K=-3) == EINVAL, 'a negative number of repetitions'
    assert fwd(N=65536) == EINVAL and bwd(N=65536) == EINVAL, 'N > 65535: the batch entry is blockIdx.y'
    assert fwd(Mt=None) == EINVAL, 'a null output'
    assert bwd(g=None) == EINVAL, 'a null cotangent'
    assert bwd(Mt=None) == EINVAL, 'no records'
    assert bwd(gA=None, gB=None, gC=None, gMi=None, gphi=None) == EINVAL, 'nothing to compute'
    for dtype, odd in ((0, FAKE + 2), (1, FAKE + 4)):
        for k in ('A', 'B', 'rest', 'Mt'):
            assert fwd(dtype=dtype, **{k: odd}) == EALIGN, (dtype, k)
        for k in ('T1', 'T2', 'df', 'Mi'):
            assert fwd(dtype=dtype, **{k: (odd, 0, 0)}) == EALIGN and bwd(dtype=dtype, **{k: (odd, 0, 0)}) == EALIGN
        for k in ('A', 'B', 'g', 'rest', 'Mt', 'gA', 'gB', 'gC', 'gMi', 'gphi'):
            assert bwd(dtype=dtype, **{k: odd}) == EALIGN, (dtype, k)
        # the phase table is fp64 whatever the data type
        assert fwd(dtype=dtype, cs=FAKE + 4) == EALIGN and bwd(dtype=dtype, cs=FAKE + 4) == EALIGN
    # ... a call right in every argument would be a launch: not made here


def test_empty_problems_are_a_success_whatever_the_pointers_are():
    fwd, bwd = _calls(mrphy_amd.require_library())
    null = dict(A=None, B=None, rest=None, T1=BCF, T2=BC0, df=BCF, Mi=BC0, cs=None)
    for size in (dict(nM=0), dict(N=0), dict(K=0), dict(N=0, nM=0, K=0)):
        assert fwd(Mt=None, **null, **size) == 0, size
        assert bwd(g=None, Mt=None, gA=None, gB=None, gC=None, gMi=None, gphi=None, **null, **size) == 0, size
    assert fwd(K=0, dtype=7) == EINVAL and bwd(N=0, nM=-1) == EINVAL and fwd(N=0, K=-1) == EINVAL


# ---------------------------------------------------------------------------------------------
# the Python layer
# ---------------------------------------------------------------------------------------------
def test_python_wrappers_refuse_cpu_tensors():
    A, B = torch.eye(3).expand(1, 5, 3, 3) * 0.9, torch.zeros(1, 5, 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.ab_train(A, B, n=4)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.ab_train(A, B, phase=torch.zeros(1, 4))
    rf, gr, loc = torch.zeros(1, 2, 16), torch.zeros(1, 3, 16), torch.zeros(1, 5, 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.train_rfgr(rf, gr, loc, n=4, rest=torch.tensor(5e-3), T1=torch.ones(1, 5), T2=torch.ones(1, 5))
    assert 'ab_train' in fused.__all__ and 'train_rfgr' in fused.__all__


def test_python_wrapper_wants_one_number_of_repetitions():
    A, B = torch.eye(3).expand(2, 5, 3, 3) * 0.9, torch.zeros(2, 5, 3)
    with pytest.raises(ValueError, match='give `n`'):
        fused.ab_train(A, B)
    with pytest.raises(ValueError, match='disagrees'):
        fused.ab_train(A, B, n=3, phase=torch.zeros(2, 4))
    with pytest.raises(ValueError, match='must be'):
        fused.ab_train(A, B, phase=torch.zeros(3, 4))          # neither N nor 1 rows
    for n in (True, 2.0, -1, '3'):
        with pytest.raises(ValueError, match='int >= 0'):
            fused.ab_train(A, B, n=n)


# ---------------------------------------------------------------------------------------------
# the fixture from the reference against the yardstick on the oracle's A, B
# ---------------------------------------------------------------------------------------------
OUTPUTS = ('Mt', 'grad_rf', 'grad_gr', 'grad_T1')


def test_yardstick_on_the_oracle_matches_the_reference_fixture():
    G = golden('train_f64')
    P = fixture_inputs(G)
    assert P['rf'].shape == (2, 2, 48) and P['loc'].shape == (2, 100, 3) and P['b1'].shape == (2, 100, 2)
    assert P['rest'].tolist() == [5e-3, 6.5e-3] and P['phase'].shape == (2, 40) and P['w'].shape == (40, 2, 100, 3)
    assert 0.01 <= float(P['T1'].min()) and float(P['T1'].max()) <= 0.02
    assert 0.005 <= float(P['T2'].min()) and float(P['T2'].max()) <= 0.01
    k = torch.arange(40, dtype=torch.float64)
    for n, φ in enumerate((117 * π / 180 * k * (k + 1) / 2, 0.7 * k)):        # the schedules, modulo 2π
        assert float((torch.exp(1j * P['phase'][n]) - torch.exp(1j * φ)).abs().max()) <= 1e-12
    assert all(v.dtype == torch.float64 for v in P.values())
    got = oracle_train(P)
    for k in OUTPUTS:
        assert tuple(got[k].shape) == G[k].shape, k
        assert_close(got[k], G[k], 'f64', f'the yardstick: {k}')
    assert G['Mt'].shape == (2, 100, 40, 3) and float(torch.from_numpy(G['grad_T1']).abs().max()) > 0


def test_fp32_fixture_holds_the_distances_the_generator_printed():
    r"""``distance_f32_vs_f64.*``: the reference's all-fp32 run against its fp64 run on the same fp32 numbers (last run of
    the generator, its docstring) -- and they are what the stored fp32 outputs are from the fp64 yardstick on the stored
    fp32 inputs."""
    G = golden('train_f32')
    P = fixture_inputs(G)
    assert all(v.dtype == torch.float32 for v in P.values()) and G['Mt'].dtype == 'float32'
    printed = dict(Mt=1.391e-06, grad_rf=1.667e-06, grad_gr=1.356e-06, grad_T1=2.188e-06)
    wide = oracle_train(P, torch.float64)
    for k, d in printed.items():
        stored = float(G[f'distance_f32_vs_f64.{k}'])
        assert abs(stored - d) <= 5e-10, (k, stored, d)
        here = float((torch.from_numpy(G[k]).double() - wide[k]).norm() / wide[k].norm())
        assert abs(here - stored) <= 0.02 * stored, (k, here, stored)


# ---------------------------------------------------------------------------------------------
# two identities of the yardstick: the known answers of the GPU tests
# ---------------------------------------------------------------------------------------------
def identity_problem():
    r"""``A, B`` of the ``steadystate_f64`` pulse by the CPU oracle with T1 in [10, 20] ms, T2 in [5, 10] ms (seeded),
    and the rest's operands: ``dict(A, B, rest, T1, T2, df)`` in fp64."""
    P = fixture_inputs(golden('steadystate_f64'))
    gen = torch.Generator().manual_seed(96)
    rnd = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64)  # noqa: E731
    T1, T2 = 0.01 + 0.01 * rnd(2, 100), 0.005 + 0.005 * rnd(2, 100)
    beff = O.rfgr2beff(P['rf'], P['gr'], P['loc'], Δf=P['df'], b1Map=P['b1'], γ=P['γ'])
    A, B = O.beff2ab(beff, E1=torch.exp(-P['dt'][:, None] / T1), E2=torch.exp(-P['dt'][:, None] / T2), γ=P['γ'],
                     dt=P['dt'])
    return dict(A=A, B=B, rest=P['rest'], T1=T1, T2=T2, df=P['df'])


def test_zero_phase_train_converges_to_the_steady_state():
    r"""(a) Zero phase, K = 96: the last record is ``torch_steadystate`` to 1e-9 (the contraction is at most
    ``exp(-5 ms / 20 ms)`` = 0.78 per repetition: 0.78^96 = 4e-11)."""
    Q = identity_problem()
    Mt = torch_train(Q['A'], Q['B'], 96, None, None, Q['rest'], Q['T1'], Q['T2'], Q['df'])
    Mss = torch_steadystate(Q['A'], Q['B'], Q['rest'], Q['T1'], Q['T2'], Q['df'])
    assert Mt.shape == (2, 100, 96, 3)
    assert float((Mt[..., -1, :] - Mss).abs().max()) <= 1e-9
    assert float((Mt[..., 0, :] - Mss).abs().max()) > 1e-2


def test_linear_phase_is_an_off_resonance_in_the_rest():
    r"""(b) ``φ_k = kψ``: the records rotated back by ``-φ_k`` are the zero-phase train with
    ``Δf' = Δf + ψ / (2π rest)`` -- to 1e-12; the other sign is O(1) away."""
    Q = identity_problem()
    K, ψ = 24, 0.7
    φ = (ψ * torch.arange(K, dtype=torch.float64)).expand(2, K)
    Mt = torch_train(Q['A'], Q['B'], K, None, φ, Q['rest'], Q['T1'], Q['T2'], Q['df'])
    back = rz(Mt, -φ[:, None, :])
    for sign, close in ((1, True), (-1, False)):
        df = Q['df'] + sign * ψ / (2 * π * Q['rest'][:, None])
        want = torch_train(Q['A'], Q['B'], K, None, None, Q['rest'], Q['T1'], Q['T2'], df)
        d = float((back - want).abs().max())
        assert (d <= 1e-12) if close else (d > 0.1), (sign, d)
