r"""``fused.sequence_steadystate`` / ``fused.sequence_steadystate_rfgr`` without a GPU: the yardstick of the GPU tests --
the period composed by ``test_ab_sequence_host.torch_sequence`` on the start vectors ``0, e_x, e_y, e_z`` and solved by
``torch.linalg.solve``, fp64 torch on the CPU -- and three identities of it; the entry points
``mrphy_sequence_steadystate_*`` are exported, declared and bound alike and refuse bad arguments before any launch; the
Python layer refuses CPU tensors, a bad schedule, ``K = 0``, an ``Mi`` and a ``rest`` of the wrong shape, all before the
device is touched."""
import ctypes

import pytest
import torch

import mrphy_amd
from mrphy_amd import _lib, fused
from test_ab_sequence_host import _cpu_bank, _seeded, torch_sequence
from test_train_signal_host import _declared
from util import FAKE

NAMES = ('mrphy_sequence_steadystate_fwd', 'mrphy_sequence_steadystate_bwd')
EINVAL, EALIGN, ENOSPC = -1, -2, -3
BC0 = (None, 0, 0)
BCF = (FAKE, 0, 0)


# ---------------------------------------------------------------------------------------------
# the yardstick (any device, differentiable)
# ---------------------------------------------------------------------------------------------
def torch_period(A, B, K, pulse=None, phase=None, rest=None, T1=None, T2=None, df=None):
    r"""``Ā`` `(N, *Nd, 3, 3)` and ``b̄`` `(N, *Nd, 3)` of the period: the last record of ``torch_sequence`` started at
    ``0`` is ``b̄``, started at ``e_j`` it is ``Ā e_j + b̄``.  Operands as ``torch_sequence`` takes them."""
    def last(Mi):
        return torch_sequence(A, B, K, pulse, Mi, phase, rest, T1, T2, df)[..., -1, :]
    zero = torch.zeros_like(B[0])
    b = last(zero)
    cols = []
    for j in range(3):
        e = zero.clone()
        e[..., j] = 1
        cols.append(last(e) - b)
    return torch.stack(cols, dim=-1), b


def torch_steadystate(A, B, K, pulse=None, phase=None, rest=None, T1=None, T2=None, df=None):
    r"""``Mss = (I - Ā)⁻¹ b̄`` `(N, *Nd, 3)` by ``torch.linalg.solve``: the state right after the last repetition."""
    Abar, b = torch_period(A, B, K, pulse, phase, rest, T1, T2, df)
    eye = torch.eye(3, dtype=b.dtype, device=b.device)
    return torch.linalg.solve(eye - Abar, b[..., None])[..., 0]


K11, PULSE11 = 11, [0, 2, 2, 0, 0, 2, 0, 2, 2, 2, 0]           # repeats; entry 1 is never played


def _ops(Q, sel=slice(None)):
    return Q['phase'][:, sel], Q['rest'][:, sel], Q['T1'], Q['T2'], Q['df']


def test_yardstick_is_a_fixed_point_of_the_period():
    Q = _seeded(3, 2, 5, K11)
    Mss = torch_steadystate(Q['A'], Q['B'], K11, PULSE11, *_ops(Q))
    assert Mss.shape == (2, 5, 3) and bool(torch.isfinite(Mss).all()) and float(Mss.abs().max()) > 0.1
    again = torch_sequence(Q['A'], Q['B'], K11, PULSE11, Mss, *_ops(Q))[..., -1, :]
    assert float((again - Mss).abs().max()) <= 1e-12
    Abar, _ = torch_period(Q['A'], Q['B'], K11, PULSE11, *_ops(Q))
    cond = torch.linalg.cond(torch.eye(3, dtype=torch.float64) - Abar)
    assert float(cond.max()) <= 1.8, 'the conditioning the GPU tests count on at K = 11'


def test_yardstick_of_the_doubled_period_is_the_same_state():
    Q = _seeded(3, 2, 5, K11)
    one = torch_steadystate(Q['A'], Q['B'], K11, PULSE11, *_ops(Q))
    two = torch_steadystate(Q['A'], Q['B'], 2 * K11, PULSE11 * 2, Q['phase'].repeat(1, 2), Q['rest'].repeat(1, 2),
                            Q['T1'], Q['T2'], Q['df'])
    assert float((two - one).abs().max()) <= 1e-12


def test_yardstick_of_the_shifted_period_is_one_repetition_on():
    r"""The period that starts at repetition 1 and ends with repetition 0 has the steady state ``Φ_0(Mss)``."""
    Q = _seeded(3, 2, 5, K11)
    Mss = torch_steadystate(Q['A'], Q['B'], K11, PULSE11, *_ops(Q))
    roll = lambda x: torch.roll(x, -1, dims=1)  # noqa: E731
    shifted = torch_steadystate(Q['A'], Q['B'], K11, PULSE11[1:] + PULSE11[:1], roll(Q['phase']), roll(Q['rest']),
                                Q['T1'], Q['T2'], Q['df'])
    on = torch_sequence(Q['A'], Q['B'], 1, PULSE11[:1], Mss, *_ops(Q, slice(0, 1)))[..., 0, :]
    assert float((shifted - on).abs().max()) <= 1e-12
    assert float((shifted - Mss).abs().max()) > 1e-3, 'the shift moves the state'


def test_the_lambda_sweep_is_autograd_through_the_solve():
    r"""What the adjoint computes: with ``λ = (I - Ā)⁻ᵀ g``, the gradient of ``(Mss g).sum()`` w.r.t. every operand is the
    gradient of ``(M_K λ).sum()`` of one period started at the constant ``Mi = Mss``; its ``grad_Mi`` is ``λ - g``; the
    entry never played gets exact zeros."""
    Q = _seeded(3, 2, 5, K11)
    names = ('A', 'B', 'phase', 'rest', 'T1', 'T2', 'df')
    g = torch.sin(torch.arange(30, dtype=torch.float64) * 0.37 + 0.3).reshape(2, 5, 3)

    def leaves():
        return {k: Q[k].clone().requires_grad_(True) for k in names}
    L = leaves()
    Mss = torch_steadystate(L['A'], L['B'], K11, PULSE11, *(L[k] for k in names[2:]))
    (Mss * g).sum().backward()
    with torch.no_grad():
        Abar, _ = torch_period(Q['A'], Q['B'], K11, PULSE11, *_ops(Q))
        lam = torch.linalg.solve((torch.eye(3, dtype=torch.float64) - Abar).transpose(-1, -2), g[..., None])[..., 0]
    S = leaves()
    Mi = Mss.detach().clone().requires_grad_(True)
    last = torch_sequence(S['A'], S['B'], K11, PULSE11, Mi, *(S[k] for k in names[2:]))[..., -1, :]
    (last * lam).sum().backward()
    for k in names:
        want = L[k].grad
        assert float((S[k].grad - want).abs().max()) <= 1e-13 * max(1.0, float(want.abs().max())), k
    assert float((Mi.grad - (lam - g)).abs().max()) <= 1e-13
    for k in ('A', 'B'):
        assert torch.equal(L[k].grad[1], torch.zeros_like(L[k].grad[1])) and float(L[k].grad[0].abs().min()) > 0


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
    # A .. df_sm and cs, cs_sn sit where mrphy_ab_sequence_* have them, without the three arguments of Mi between
    seq_f, seq_b = (list(_lib.PROTOTYPES[f'mrphy_ab_sequence_{w}'][1]) for w in ('fwd', 'bwd'))
    fwd, bwd = (list(_lib.PROTOTYPES[n][1]) for n in NAMES)
    assert fwd[:16] == seq_f[:16] and fwd[16:18] == seq_f[19:21]
    assert bwd[:17] == seq_b[:17] and bwd[17:19] == seq_b[20:22]
    # the outputs and the workspaces of the adjoint as mrphy_sequence_signal_bwd ends, without grad_Mi and grad_rx
    sig_b = list(_lib.PROTOTYPES['mrphy_sequence_signal_bwd'][1])
    assert bwd[-8:] == sig_b[-8:] and len(bwd) == 19 + 3 + 5 + 8
    lib = mrphy_amd.require_library()
    assert lib.mrphy_abi_version() == _lib.ABI_VERSION == 5
    assert ('tu_sequence_steady.hip', None) in _lib.UNITS
    assert 'sequence_steadystate' in fused.__all__ and 'sequence_steadystate_rfgr' in fused.__all__


def _calls(lib):
    r"""``fwd(...)`` / ``bwd(...)`` with fake pointers (never dereferenced: no call here is valid on a problem that has
    spins and is well-formed enough to launch).  ``wb=None`` / ``bb=None``: the workspaces the queries ask for."""
    def fwd(A=FAKE, B=FAKE, P=3, pulse=FAKE, rs=FAKE, T1=BCF, T2=BCF, df=BCF, cs=FAKE, Mss=FAKE, per=FAKE, ck=FAKE, N=2,
            nM=100, K=5, dtype=0):
        return lib.mrphy_sequence_steadystate_fwd(dtype, A, B, P, pulse, rs, 0, *T1, *T2, *df, cs, 0, Mss, per, ck, N, nM,
                                                  K, None)

    def bwd(A=FAKE, B=FAKE, P=3, pulse=FAKE, g=FAKE, rs=FAKE, T1=BCF, T2=BCF, df=BCF, cs=FAKE, per=FAKE, ck=FAKE,
            lam=FAKE, gA=FAKE, gB=FAKE, gC=FAKE, grest=FAKE, gphi=FAKE, work=FAKE, wb=None, bank=FAKE, bb=None, N=2,
            nM=100, K=5, dtype=0):
        nQ = (gphi is not None) + (grest is not None)
        wb = lib.mrphy_sequence_signal_workspace(dtype, N, nM, K, max(nQ, 1)) if wb is None else wb
        bb = lib.mrphy_sequence_signal_bank_workspace(0, max(P, 1), max(N, 1), max(nM, 1)) if bb is None else bb
        return lib.mrphy_sequence_steadystate_bwd(dtype, A, B, P, pulse, g, rs, 0, *T1, *T2, *df, cs, 0, per, ck, lam,
                                                  gA, gB, gC, grest, gphi, work, wb, bank, bb, N, nM, K, None)
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
    'a bank past the grid': dict(P=65536),
    'no schedule for a bank of 3': dict(pulse=None),
    'a period without a repetition': dict(K=0),
}


@pytest.mark.parametrize('what', list(OPERAND_FAULTS))
def test_entry_points_check_their_operands_alike(what):
    fwd, bwd = _calls(mrphy_amd.require_library())
    for dtype in (0, 1):
        assert fwd(dtype=dtype, **OPERAND_FAULTS[what]) == EINVAL
        assert bwd(dtype=dtype, **OPERAND_FAULTS[what]) == EINVAL


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = mrphy_amd.require_library()
    fwd, bwd = _calls(lib)
    for dtype in (-1, 2, 3, 4, 5, 17):          # data types only, as mrphy_ab_sequence_*
        assert fwd(dtype=dtype) == EINVAL and bwd(dtype=dtype, wb=1 << 30) == EINVAL, ('dtype', dtype)
    assert fwd(N=-1) == EINVAL and fwd(nM=-1) == EINVAL and bwd(N=-2) == EINVAL and bwd(nM=-100) == EINVAL
    assert fwd(K=-1) == EINVAL and bwd(K=-3) == EINVAL, 'a negative number of repetitions'
    assert fwd(N=65536) == EINVAL and bwd(N=65536) == EINVAL, 'N > 65535: the batch entry is blockIdx.y'
    assert fwd(Mss=None) == EINVAL, 'a null output'
    assert bwd(g=None) == EINVAL, 'no cotangent'
    assert bwd(per=None) == EINVAL and bwd(ck=None) == EINVAL and bwd(lam=None) == EINVAL, 'what the forward left; λ'
    assert bwd(gA=None, gB=None, gC=None, grest=None, gphi=None) == EINVAL, 'nothing to compute'
    assert bwd(work=None) == EINVAL and bwd(work=None, gphi=None) == EINVAL and bwd(work=None, grest=None) == EINVAL, \
        'the sums over the spins need their workspace'
    assert bwd(bank=None) == EINVAL and bwd(bank=None, gA=None) == EINVAL and bwd(bank=None, gB=None) == EINVAL, \
        'the bank gradients need their workspace'
    two, one = (lib.mrphy_sequence_signal_workspace(0, 2, 100, 5, q) for q in (2, 1))
    assert bwd(wb=two - 1) == ENOSPC and bwd(wb=one) == ENOSPC, 'a phase and a rest row'
    assert bwd(grest=None, wb=one - 1) == ENOSPC and bwd(gphi=None, wb=one - 1) == ENOSPC and bwd(gphi=None, wb=0) == ENOSPC
    for dtype in (0, 1):
        assert bwd(dtype=dtype, bb=3 * 12 * 200 * 8 - 8) == ENOSPC and bwd(dtype=dtype, bb=0) == ENOSPC, 'a short bank'
    for dtype, odd in ((0, FAKE + 2), (1, FAKE + 4)):
        for k in ('A', 'B', 'Mss'):
            assert fwd(dtype=dtype, **{k: odd}) == EALIGN, (dtype, k)
        for k in ('T1', 'T2', 'df'):
            assert fwd(dtype=dtype, **{k: (odd, 0, 0)}) == EALIGN and bwd(dtype=dtype, **{k: (odd, 0, 0)}) == EALIGN
        for k in ('A', 'B', 'g', 'lam', 'gA', 'gB'):
            assert bwd(dtype=dtype, **{k: odd}) == EALIGN, (dtype, k)
        # the tables, what the forward leaves, the workspaces and the fp64 gradients have their own element sizes
        for k in ('rs', 'cs', 'per', 'ck'):
            assert fwd(dtype=dtype, **{k: FAKE + 4}) == EALIGN and bwd(dtype=dtype, **{k: FAKE + 4}) == EALIGN, k
        assert fwd(dtype=dtype, pulse=FAKE + 2) == EALIGN and bwd(dtype=dtype, pulse=FAKE + 2) == EALIGN
        for k in ('gC', 'grest', 'gphi', 'work', 'bank'):
            assert bwd(dtype=dtype, **{k: FAKE + 4}) == EALIGN, (dtype, k)
    # a null pointer is reported before a misaligned one, a misaligned pointer before a short bank
    assert fwd(pulse=None, A=FAKE + 2) == EINVAL and bwd(pulse=None, rs=FAKE + 4) == EINVAL
    assert fwd(Mss=None, A=FAKE + 2) == EINVAL and bwd(ck=None, rs=FAKE + 4) == EINVAL
    assert bwd(rs=FAKE + 4, bb=0) == EALIGN
    # ... a call right in every argument would be a launch: not made here


def test_problems_without_spins_are_a_success_whatever_the_pointers_are():
    fwd, bwd = _calls(mrphy_amd.require_library())
    null = dict(A=None, B=None, pulse=None, rs=None, T1=BCF, T2=BC0, df=BCF, cs=None)
    for size in (dict(nM=0), dict(N=0), dict(N=0, nM=0), dict(nM=0, K=0), dict(N=0, K=0)):
        assert fwd(Mss=None, per=None, ck=None, **null, **size) == 0, size
        assert bwd(g=None, per=None, ck=None, lam=None, gA=None, gB=None, gC=None, grest=None, gphi=None, work=None,
                   wb=0, bank=None, bb=0, **null, **size) == 0, size
    assert fwd(nM=0, dtype=7) == EINVAL and bwd(N=0, nM=-1) == EINVAL and fwd(N=0, K=-1) == EINVAL
    assert fwd(nM=0, P=0) == EINVAL and bwd(nM=0, P=-1) == EINVAL, 'a bank holds at least one pulse'
    assert fwd(K=0, **null) == EINVAL and bwd(K=0, **null) == EINVAL, 'spins, but no repetition: not an empty problem'


# ---------------------------------------------------------------------------------------------
# the Python layer
# ---------------------------------------------------------------------------------------------
RFGR = dict(rest=torch.tensor(5e-3), T1=torch.ones(2, 5), T2=torch.ones(2, 5))


def _cpu_pulses():
    return torch.zeros(3, 2, 2, 16), torch.zeros(1, 2, 3, 16), torch.zeros(2, 5, 3)


def test_python_wrappers_refuse_cpu_tensors():
    A, B = _cpu_bank()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.sequence_steadystate(A, B, pulse=[0, 1, 2, 1])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.sequence_steadystate(A[:1], B[:1], n=4)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.sequence_steadystate(A, B, pulse=torch.tensor([0, 2], dtype=torch.int32), rest=torch.full((2, 2), 5e-3))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.sequence_steadystate_rfgr(*_cpu_pulses(), pulse=[0, 1, 2, 2], **RFGR)


@pytest.mark.parametrize('pulse, k', [([0, 1, 3], 2), ([0, -1, 1], 1), (torch.tensor([2, 0, 5, 7]), 2),
                                      ([0, 1.0, 1], 1), ([True, 0], 0), (torch.tensor([0.0, 1.0]), 0)],
                         ids=['past-the-bank', 'negative', 'tensor-past-the-bank', 'float-entry', 'bool-entry',
                              'float-tensor'])
def test_schedule_is_checked_on_the_host_before_the_device(pulse, k):
    r"""On CPU tensors: the schedule's ``ValueError`` is ``ab_sequence``'s, names the repetition and comes before the
    'no CPU fallback' error."""
    A, B = _cpu_bank()
    with pytest.raises(ValueError) as want:
        fused.ab_sequence(A, B, pulse=pulse)
    with pytest.raises(ValueError, match=f'repetition {k}') as got:
        fused.sequence_steadystate(A, B, pulse=pulse)
    assert str(got.value) == str(want.value)
    with pytest.raises(ValueError, match=f'repetition {k}') as got:
        fused.sequence_steadystate_rfgr(*_cpu_pulses(), pulse=pulse, **RFGR)
    assert str(got.value) == str(want.value)


def test_python_wrapper_checks_the_schedule_the_length_and_the_rest():
    A, B = _cpu_bank()
    with pytest.raises(ValueError, match='`pulse` is required'):
        fused.sequence_steadystate(A, B, n=4)
    with pytest.raises(ValueError, match=r'must be \(K,\)'):
        fused.sequence_steadystate(A, B, pulse=torch.zeros(2, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match='give `n`'):
        fused.sequence_steadystate(A[:1], B[:1])
    with pytest.raises(ValueError, match='disagrees'):
        fused.sequence_steadystate(A, B, n=3, pulse=[0, 1, 2, 0])
    with pytest.raises(ValueError, match='disagrees'):
        fused.sequence_steadystate(A, B, pulse=[0, 1, 2], phase=torch.zeros(2, 4))
    with pytest.raises(ValueError, match='must be'):
        fused.sequence_steadystate(A, B, pulse=[0] * 4, phase=torch.zeros(3, 4))          # neither N nor 1 rows
    for n in (True, 2.0, -1, '3'):
        with pytest.raises(ValueError, match='int >= 0'):
            fused.sequence_steadystate(A, B, n=n, pulse=[0])
    for shape in ((3,), (2, 3), (3, 4), (2, 4, 1), (4, 2), (2, 1), (1, 1)):           # N = 2, K = 4
        with pytest.raises(ValueError, match='`rest`'):
            fused.sequence_steadystate(A, B, pulse=[0, 1, 2, 0], rest=torch.full(shape, 5e-3))


def test_a_period_needs_a_repetition_and_has_no_initial_state():
    A, B = _cpu_bank()
    for given in (dict(pulse=[]), dict(n=0, pulse=[]), dict(pulse=torch.zeros(0, dtype=torch.int64)),
                  dict(pulse=[], phase=torch.zeros(2, 0))):
        with pytest.raises(ValueError, match='needs a repetition'):
            fused.sequence_steadystate(A, B, **given)
    with pytest.raises(ValueError, match='needs a repetition'):
        fused.sequence_steadystate(A[:1], B[:1], n=0)
    with pytest.raises(ValueError, match='needs a repetition'):
        fused.sequence_steadystate_rfgr(*_cpu_pulses(), pulse=[], **RFGR)
    with pytest.raises(TypeError, match='Mi'):
        fused.sequence_steadystate(A, B, pulse=[0, 1], Mi=torch.zeros(2, 5, 3))
    with pytest.raises(TypeError, match='Mi'):
        fused.sequence_steadystate_rfgr(*_cpu_pulses(), pulse=[0, 1], Mi=torch.zeros(2, 5, 3), **RFGR)


@pytest.mark.parametrize('missing', ['rest', 'T1', 'T2'])
def test_rfgr_requires_the_relaxation_of_the_rest(missing):
    kw = {k: v for k, v in RFGR.items() if k != missing}
    with pytest.raises(AssertionError, match='needs relaxation'):
        fused.sequence_steadystate_rfgr(*_cpu_pulses(), pulse=[0, 1, 2], **kw)
