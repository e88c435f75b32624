r"""``fused.ab_sequence`` / ``fused.sequence_rfgr`` without a GPU: the three entry points ``mrphy_ab_sequence_*`` are
exported, declared and bound alike and refuse bad arguments before any launch; the Python layer refuses CPU tensors, a
schedule outside the bank and contradictory lengths -- the schedule before anything else; the fixtures
``tests/golden/sequence_f32.npz`` / ``_f64.npz`` (the live reference, ``tests/golden/make_golden_sequence.py``) against
the yardstick of the GPU tests -- the recursion in plain torch (:func:`torch_sequence`) on the CPU oracle's ``rfgr2beff``
-> ``beff2ab`` per bank entry --; and two identities of that yardstick."""
import ctypes
import itertools

import pytest
import torch

import bloch_oracle as O
import mrphy_amd
from mrphy_amd import _lib, fused
from test_ab_rfgr_host import _declared, fixture_inputs
from test_ab_train_host import rz, torch_train
from test_steadystate_host import rest_period
from util import FAKE, assert_close, golden

NAMES = ('mrphy_ab_sequence_bwd_workspace', 'mrphy_ab_sequence_fwd', 'mrphy_ab_sequence_bwd')
EINVAL, EALIGN, ENOSPC = -1, -2, -3
BC0 = (None, 0, 0)
BCF = (FAKE, 0, 0)


# ---------------------------------------------------------------------------------------------
# the yardstick: the recursion in plain torch (any device, differentiable)
# ---------------------------------------------------------------------------------------------
def torch_sequence(A, B, K, pulse=None, Mi=None, phase=None, rest=None, T1=None, T2=None, df=None):
    r"""``Mt`` `(N, *Nd, K, 3)`: ``test_ab_train_host.torch_train`` with ``rest_period(B, rest[:, k], ...)`` and
    ``A[pulse[k]], B[pulse[k]]`` per repetition.  ``A`` `(P, N, *Nd, 3, 3)`; ``pulse`` a sequence of ``K`` ints or ``None``
    (zeros); ``rest`` `(N ⊻ 1, K)` or ``None``."""
    M = torch.zeros_like(B[0])
    M[..., 2] = 1
    if Mi is not None:
        M = Mi.expand(B[0].shape)
    out = []
    for k in range(K):
        p = 0 if pulse is None else int(pulse[k])
        F, f = rest_period(B[p], None if rest is None else rest[:, k], T1, T2, df)
        Mm = (F @ M[..., None])[..., 0] + f
        if phase is None:
            M = (A[p] @ Mm[..., None])[..., 0] + B[p]
        else:
            φ = phase[:, k].reshape((-1,) + (1,) * (B.ndim - 3))
            M = rz((A[p] @ rz(Mm, -φ)[..., None])[..., 0] + B[p], φ)
        out.append(M)
    if not out:
        return B.new_zeros(B.shape[1:-1] + (0, 3))
    return torch.stack(out, dim=-2)


def oracle_bank(P, rf, gr, T1):
    r"""``A, B`` of the bank by the CPU oracle's ``rfgr2beff`` -> ``beff2ab``, entry by entry."""
    E2 = torch.exp(-P['dt'][:, None] / P['T2'])
    AB = [O.beff2ab(O.rfgr2beff(rf[p], gr, P['loc'], Δf=P['df'], b1Map=P['b1'], γ=P['γ']),
                    E1=torch.exp(-P['dt'][:, None] / T1), E2=E2, γ=P['γ'], dt=P['dt']) for p in range(rf.shape[0])]
    return torch.stack([a for a, _ in AB]), torch.stack([b for _, b in AB])


def oracle_sequence(P, dtype=None):
    r"""``Mt, grad_rf, grad_gr, grad_T1, grad_rest`` of the loss ``(Mt w).sum()`` by the CPU oracle's bank,
    :func:`torch_sequence` and autograd, on the inputs ``P`` of a fixture, widened to ``dtype`` if given."""
    P = {k: (v if dtype is None or k == 'pulse' else v.to(dtype)) for k, v in P.items()}
    rf, gr, T1, rest = (P[k].clone().requires_grad_(True) for k in ('rf', 'gr', 'T1', 'rest'))
    A, B = oracle_bank(P, rf, gr, T1)
    Mt = torch_sequence(A, B, P['phase'].shape[1], P['pulse'].tolist(), None, P['phase'], rest, T1, P['T2'], P['df'])
    (Mt.movedim(-2, 0) * P['w']).sum().backward()
    return dict(Mt=Mt.detach(), grad_rf=rf.grad, grad_gr=gr.grad, grad_T1=T1.grad, grad_rest=rest.grad)


def _seeded(P_, N, nM, K, seed=5):
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64)  # noqa: E731
    Q = torch.linalg.qr(torch.randn((P_, N, nM, 3, 3), generator=gen, dtype=torch.float64))[0]
    return dict(A=0.97 * Q, B=torch.randn((P_, N, nM, 3), generator=gen, dtype=torch.float64),
                Mi=torch.randn((N, nM, 3), generator=gen, dtype=torch.float64),
                phase=2 * torch.randn((N, K), generator=gen, dtype=torch.float64), rest=2e-3 + 8e-3 * rnd(N, K),
                T1=0.05 + 0.1 * rnd(N, nM), T2=0.02 + 0.05 * rnd(N, nM), df=(rnd(N, nM) * 2 - 1) * 200)


def test_yardstick_without_a_schedule_is_the_train_exactly():
    Q = _seeded(1, 2, 7, 6)
    const = Q['rest'][:, 0].clone()
    want = torch_train(Q['A'][0], Q['B'][0], 6, Q['Mi'], Q['phase'], const, Q['T1'], Q['T2'], Q['df'])
    got = torch_sequence(Q['A'], Q['B'], 6, None, Q['Mi'], Q['phase'], const[:, None].expand(2, 6), Q['T1'], Q['T2'],
                         Q['df'])
    assert torch.equal(got, want)
    assert torch.equal(torch_sequence(Q['A'], Q['B'], 6, [0] * 6, Q['Mi'], Q['phase'], const[:, None].expand(2, 6),
                                      Q['T1'], Q['T2'], Q['df']), want)


def test_yardstick_split_anywhere_is_two_chained_calls():
    K, pulse = 6, [0, 2, 2, 1, 0, 2]
    Q = _seeded(3, 2, 7, K)
    ops = (Q['T1'], Q['T2'], Q['df'])
    whole = torch_sequence(Q['A'], Q['B'], K, pulse, Q['Mi'], Q['phase'], Q['rest'], *ops)
    assert whole.shape == (2, 7, K, 3)
    for k in range(K + 1):
        head = torch_sequence(Q['A'], Q['B'], k, pulse[:k], Q['Mi'], Q['phase'][:, :k], Q['rest'][:, :k], *ops)
        Mi = head[..., -1, :] if k else Q['Mi']
        tail = torch_sequence(Q['A'], Q['B'], K - k, pulse[k:], Mi, Q['phase'][:, k:], Q['rest'][:, k:], *ops)
        assert float((torch.cat((head, tail), dim=-2) - whole).abs().max()) <= 1e-14, k


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
    # T1 .. cs_sn sit in the order mrphy_ab_train_* have them: 14 arguments after (rest, rest_sn) there, (rs, rs_sn) here
    train_f, train_b = (_lib.PROTOTYPES[f'mrphy_ab_train_{w}'][1] for w in ('fwd', 'bwd'))
    assert list(_lib.PROTOTYPES[NAMES[1]][1][5:21]) == list(train_f[3:19])
    assert list(_lib.PROTOTYPES[NAMES[2]][1][6:22]) == list(train_b[4:20])
    lib = mrphy_amd.require_library()
    assert lib.mrphy_abi_version() == _lib.ABI_VERSION == 5
    assert ('tu_ab_sequence.hip', None) in _lib.UNITS
    q = lib.mrphy_ab_sequence_bwd_workspace
    assert q(0, 3, 2, 100) == q(1, 3, 2, 100) == 3 * 12 * 200 * 8, 'fp64 (P, 12, rows) whatever the data type'
    assert q(5, 3, 2, 100) == 0 and q(0, 0, 2, 100) == 0 and q(0, 3, 0, 100) == 0 and q(0, 3, 2, -1) == 0


def _calls(lib):
    r"""``fwd(...)`` / ``bwd(...)`` with fake pointers (never dereferenced: no call here is valid on a problem that is not
    empty and well-formed enough to launch)."""
    def fwd(A=FAKE, B=FAKE, P=3, pulse=FAKE, rs=FAKE, T1=BCF, T2=BCF, df=BCF, Mi=BCF, cs=FAKE, Mt=FAKE, N=2, nM=100, K=5,
            dtype=0):
        return lib.mrphy_ab_sequence_fwd(dtype, A, B, P, pulse, rs, 0, *T1, *T2, *df, *Mi, cs, 0, Mt, N, nM, K, None)

    def bwd(A=FAKE, B=FAKE, P=3, pulse=FAKE, g=FAKE, rs=FAKE, T1=BCF, T2=BCF, df=BCF, Mi=BCF, cs=FAKE, Mt=FAKE, gA=FAKE,
            gB=FAKE, gC=FAKE, grest=FAKE, gMi=FAKE, gphi=FAKE, work=FAKE, wb=None, N=2, nM=100, K=5, dtype=0):
        wb = lib.mrphy_ab_sequence_bwd_workspace(0, max(P, 1), max(N, 1), max(nM, 1)) if wb is None else wb
        return lib.mrphy_ab_sequence_bwd(dtype, A, B, P, pulse, g, rs, 0, *T1, *T2, *df, *Mi, cs, 0, Mt, gA, gB, gC,
                                         grest, gMi, gphi, work, wb, N, nM, K, None)
    return fwd, bwd


OPERAND_FAULTS = {
    'A null': dict(A=None),
    'B null': dict(B=None),
    'T1 without a rest': dict(rs=None, df=BC0),
    'df without a rest': dict(rs=None, T1=BC0, T2=BC0),
    'T1, T2, df without a rest': dict(rs=None),
    'T1 without T2': dict(T2=BC0),
    'T2 without T1': dict(T1=BC0),
    'T2 without T1 nor df': dict(T1=BC0, df=BC0),
    'no pulse in the bank': dict(P=0),
    'a negative bank': dict(P=-2),
    'no schedule for a bank of 3': dict(pulse=None),
}


@pytest.mark.parametrize('what', list(OPERAND_FAULTS))
def test_entry_points_check_their_operands_alike(what):
    fwd, bwd = _calls(mrphy_amd.require_library())
    for dtype in (0, 1):
        assert fwd(dtype=dtype, **OPERAND_FAULTS[what]) == EINVAL
        assert bwd(dtype=dtype, **OPERAND_FAULTS[what]) == EINVAL


def test_entry_points_refuse_bad_arguments_before_any_launch():
    fwd, bwd = _calls(mrphy_amd.require_library())
    for dtype in (-1, 2, 3, 4, 5, 17):          # data types only, as mrphy_ab_train_*
        assert fwd(dtype=dtype) == EINVAL and bwd(dtype=dtype) == EINVAL, ('dtype', dtype)
    assert fwd(N=-1) == EINVAL and fwd(nM=-1) == EINVAL and bwd(N=-2) == EINVAL and bwd(nM=-100) == EINVAL
    assert fwd(K=-1) == EINVAL and bwd(K=-3) == EINVAL, 'a negative number of repetitions'
    assert fwd(N=65536) == EINVAL and bwd(N=65536) == EINVAL, 'N > 65535: the batch entry is blockIdx.y'
    assert fwd(Mt=None) == EINVAL, 'a null output'
    assert bwd(g=None) == EINVAL, 'a null cotangent'
    assert bwd(Mt=None) == EINVAL, 'no records'
    assert bwd(gA=None, gB=None, gC=None, grest=None, gMi=None, gphi=None) == EINVAL, 'nothing to compute'
    for dtype in (0, 1):
        assert bwd(dtype=dtype, work=None) == EINVAL, 'the bank gradients need the workspace'
        assert bwd(dtype=dtype, wb=3 * 12 * 200 * 8 - 8) == ENOSPC, 'a short workspace'
        assert bwd(dtype=dtype, wb=0) == ENOSPC
    for dtype, odd in ((0, FAKE + 2), (1, FAKE + 4)):
        for k in ('A', 'B', 'Mt'):
            assert fwd(dtype=dtype, **{k: odd}) == EALIGN, (dtype, k)
        for k in ('T1', 'T2', 'df', 'Mi'):
            assert fwd(dtype=dtype, **{k: (odd, 0, 0)}) == EALIGN and bwd(dtype=dtype, **{k: (odd, 0, 0)}) == EALIGN
        for k in ('A', 'B', 'g', 'Mt', 'gA', 'gB', 'gC', 'grest', 'gMi', 'gphi'):
            assert bwd(dtype=dtype, **{k: odd}) == EALIGN, (dtype, k)
        # the three tables and the workspace have their own element sizes whatever the data type
        for k in ('rs', 'cs'):
            assert fwd(dtype=dtype, **{k: FAKE + 4}) == EALIGN and bwd(dtype=dtype, **{k: FAKE + 4}) == EALIGN, k
        assert fwd(dtype=dtype, pulse=FAKE + 2) == EALIGN and bwd(dtype=dtype, pulse=FAKE + 2) == EALIGN
        assert bwd(dtype=dtype, work=FAKE + 4) == EALIGN
    # a null pointer is reported before a misaligned one
    assert fwd(pulse=None, A=FAKE + 2) == EINVAL and bwd(pulse=None, rs=FAKE + 4) == EINVAL
    # ... a call right in every argument would be a launch: not made here


def test_empty_problems_are_a_success_whatever_the_pointers_are():
    fwd, bwd = _calls(mrphy_amd.require_library())
    null = dict(A=None, B=None, pulse=None, rs=None, T1=BCF, T2=BC0, df=BCF, Mi=BC0, cs=None)
    for size in (dict(nM=0), dict(N=0), dict(K=0), dict(N=0, nM=0, K=0)):
        assert fwd(Mt=None, **null, **size) == 0, size
        assert bwd(g=None, Mt=None, gA=None, gB=None, gC=None, grest=None, gMi=None, gphi=None, work=None, wb=0, **null,
                   **size) == 0, size
    assert fwd(K=0, dtype=7) == EINVAL and bwd(N=0, nM=-1) == EINVAL and fwd(N=0, K=-1) == EINVAL
    assert fwd(K=0, P=0) == EINVAL and bwd(nM=0, P=-1) == EINVAL, 'a bank holds at least one pulse'


# ---------------------------------------------------------------------------------------------
# the Python layer
# ---------------------------------------------------------------------------------------------
def _cpu_bank(P=3, N=2, nM=5):
    return (torch.eye(3).expand(P, N, nM, 3, 3) * 0.9).contiguous(), torch.zeros(P, N, nM, 3)


def test_python_wrappers_refuse_cpu_tensors():
    A, B = _cpu_bank()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.ab_sequence(A, B, pulse=[0, 1, 2, 1])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.ab_sequence(A[:1], B[:1], n=4)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.ab_sequence(A, B, pulse=torch.tensor([0, 2], dtype=torch.int32), rest=torch.full((2, 2), 5e-3))
    rf, gr, loc = torch.zeros(3, 2, 2, 16), torch.zeros(1, 2, 3, 16), torch.zeros(2, 5, 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.sequence_rfgr(rf, gr, loc, pulse=[0, 1, 2, 2], rest=torch.tensor(5e-3), T1=torch.ones(2, 5),
                            T2=torch.ones(2, 5))
    assert 'ab_sequence' in fused.__all__ and 'sequence_rfgr' in fused.__all__


@pytest.mark.parametrize('pulse, k', [([0, 1, 3], 2), ([0, -1, 1], 1), (torch.tensor([2, 0, 5, 7]), 2),
                                      ([0, 1.0, 1], 1), ([True, 0], 0), (torch.tensor([0.0, 1.0]), 0)],
                         ids=['past-the-bank', 'negative', 'tensor-past-the-bank', 'float-entry', 'bool-entry',
                              'float-tensor'])
def test_schedule_is_checked_on_the_host_before_the_device(pulse, k):
    r"""On CPU tensors: the schedule's ``ValueError`` names the repetition and comes before the 'no CPU fallback' error."""
    A, B = _cpu_bank()
    with pytest.raises(ValueError, match=f'repetition {k}'):
        fused.ab_sequence(A, B, pulse=pulse)
    rf, gr, loc = torch.zeros(3, 2, 2, 16), torch.zeros(1, 2, 3, 16), torch.zeros(2, 5, 3)
    with pytest.raises(ValueError, match=f'repetition {k}'):
        fused.sequence_rfgr(rf, gr, loc, pulse=pulse)


def test_schedule_is_required_with_more_than_one_pulse():
    A, B = _cpu_bank()
    with pytest.raises(ValueError, match='`pulse` is required'):
        fused.ab_sequence(A, B, n=4)
    with pytest.raises(ValueError, match=r'must be \(K,\)'):
        fused.ab_sequence(A, B, pulse=torch.zeros(2, 2, dtype=torch.int64))


def test_python_wrapper_wants_one_number_of_repetitions():
    A, B = _cpu_bank()
    with pytest.raises(ValueError, match='give `n`'):
        fused.ab_sequence(A[:1], B[:1])
    with pytest.raises(ValueError, match='disagrees'):
        fused.ab_sequence(A, B, n=3, pulse=[0, 1, 2, 0])
    with pytest.raises(ValueError, match='disagrees'):
        fused.ab_sequence(A, B, pulse=[0, 1, 2], phase=torch.zeros(2, 4))
    with pytest.raises(ValueError, match='disagrees'):
        fused.ab_sequence(A[:1], B[:1], n=3, phase=torch.zeros(2, 4))
    with pytest.raises(ValueError, match='must be'):
        fused.ab_sequence(A, B, pulse=[0] * 4, phase=torch.zeros(3, 4))          # neither N nor 1 rows
    for n in (True, 2.0, -1, '3'):
        with pytest.raises(ValueError, match='int >= 0'):
            fused.ab_sequence(A, B, n=n, pulse=[0])


@pytest.mark.parametrize('shape', [(3,), (2, 3), (3, 4), (2, 4, 1), (4, 2)])
def test_rest_of_a_wrong_shape_is_refused(shape):
    r"""N = 2, K = 4: `()`, `(1,)`, `(2,)`, `(1, 4)`, `(2, 4)` are the forms; anything else is a ``ValueError``."""
    A, B = _cpu_bank()
    with pytest.raises(ValueError, match='`rest`'):
        fused.ab_sequence(A, B, pulse=[0, 1, 2, 0], rest=torch.full(shape, 5e-3))


@pytest.mark.parametrize('shape', [(2, 1), (1, 1)])
def test_a_rest_table_of_one_column_is_refused_unless_K_is_1(shape):
    r"""N = 2, K = 4: a 2-d ``rest`` is a table `(N ⊻ 1, K)`, so `(N, 1)` and `(1, 1)` -- durations that do not change,
    written with a column axis -- are a ``ValueError``; the spellings of a constant rest are `()`, `(1,)` and `(N,)`.
    At ``K = 1`` the same two shapes ARE the table and pass the check (the call then goes on to ask for device
    tensors)."""
    A, B = _cpu_bank()
    with pytest.raises(ValueError, match='`rest`'):
        fused.ab_sequence(A, B, pulse=[0, 1, 2, 0], rest=torch.full(shape, 5e-3))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.ab_sequence(A, B, pulse=[1], rest=torch.full(shape, 5e-3))


# ---------------------------------------------------------------------------------------------
# the fixture from the reference against the yardstick on the oracle's A, B
# ---------------------------------------------------------------------------------------------
OUTPUTS = ('Mt', 'grad_rf', 'grad_gr', 'grad_T1', 'grad_rest')


def test_yardstick_on_the_oracle_matches_the_reference_fixture():
    from math import pi as π
    G = golden('sequence_f64')
    P = fixture_inputs(G)
    K = 24
    assert P['rf'].shape == (3, 2, 2, 48) and P['gr'].shape == (2, 3, 48) and P['loc'].shape == (2, 100, 3)
    assert torch.equal(P['rf'][1], 0.5 * P['rf'][0]) and torch.equal(P['rf'][2], 1.6 * P['rf'][0])
    pulse = P['pulse'].tolist()
    assert len(pulse) == K and set(pulse) == {0, 1, 2} and P['pulse'].dtype == torch.int64
    runs = [len(list(g)) for _, g in itertools.groupby(pulse)]
    assert 1 in runs and 2 in runs and max(runs) == 2, 'single repetitions and runs of two'
    assert len(runs) > 3, 'returns to entries played before'
    rest = P['rest']
    assert rest.shape == (2, K) and torch.equal(rest[:, 5], rest[:, 4]) and float(rest[:, 9].abs().max()) == 0
    others = rest[:, [k for k in range(K) if k != 9]]
    assert 2e-3 <= float(others.min()) and float(others.max()) <= 8e-3
    assert P['phase'].shape == (2, K) and P['w'].shape == (K, 2, 100, 3)
    assert 0.01 <= float(P['T1'].min()) and float(P['T1'].max()) <= 0.02
    assert 0.005 <= float(P['T2'].min()) and float(P['T2'].max()) <= 0.01
    k = torch.arange(K, dtype=torch.float64)
    for n, φ in enumerate((117 * π / 180 * k * (k + 1) / 2, 0.7 * k)):        # the schedules, modulo 2π
        assert float((torch.exp(1j * P['phase'][n]) - torch.exp(1j * φ)).abs().max()) <= 1e-12
    assert all(v.dtype == torch.float64 for k, v in P.items() if k != 'pulse')
    got = oracle_sequence(P)
    for k in OUTPUTS:
        assert tuple(got[k].shape) == G[k].shape, k
        assert_close(got[k], G[k], 'f64', f'the yardstick: {k}')
    assert G['Mt'].shape == (2, 100, K, 3) and G['grad_rest'].shape == (2, K)
    # (the first rest acts on the equilibrium (0, 0, 1), which it leaves alone: its duration has no effect)
    assert float(torch.from_numpy(G['grad_T1']).abs().max()) > 0 and float(torch.from_numpy(G['grad_rest'][:, 1:]).abs().min()) > 0


def test_fp32_fixture_holds_the_distances_the_generator_printed():
    r"""``distance_f32_vs_f64.*``: the reference's all-fp32 run against its fp64 run on the same fp32 numbers (last run of
    the generator, its docstring) -- and they are what the stored fp32 outputs are from the fp64 yardstick on the stored
    fp32 inputs, to 2 %."""
    G = golden('sequence_f32')
    P = fixture_inputs(G)
    assert all(v.dtype == torch.float32 for k, v in P.items() if k != 'pulse') and G['Mt'].dtype == 'float32'
    printed = dict(Mt=1.599e-06, grad_rf=1.854e-06, grad_gr=2.368e-06, grad_T1=1.991e-06, grad_rest=2.033e-06)
    wide = oracle_sequence(P, torch.float64)
    for k, d in printed.items():
        stored = float(G[f'distance_f32_vs_f64.{k}'])
        assert abs(stored - d) <= 5e-10, (k, stored, d)
        here = float((torch.from_numpy(G[k]).double() - wide[k]).norm() / wide[k].norm())
        assert abs(here - stored) <= 0.02 * stored, (k, here, stored)
