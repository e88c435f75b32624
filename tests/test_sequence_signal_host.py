r"""``fused.sequence_signal`` / ``fused.sequence_signal_rfgr`` without a GPU: the entry points ``mrphy_sequence_signal_*``
are exported, declared and bound alike and refuse bad arguments before any launch; the two workspace queries equal
their documented products; the Python layer refuses CPU tensors and a bad schedule -- the schedule first, with
``ab_sequence``'s messages --; and the yardstick of the GPU tests, ``test_ab_sequence_host.torch_sequence`` followed by
``test_train_signal_host.torch_signal``, against ``fused._signal_of`` on CPU tensors."""
import ctypes

import pytest
import torch

import mrphy_amd
from mrphy_amd import _lib, fused
from test_ab_sequence_host import _cpu_bank, _seeded, torch_sequence
from test_train_signal_host import MAX_WAVES, _declared, torch_signal
from util import FAKE

NAMES = ('mrphy_sequence_signal_workspace', 'mrphy_sequence_signal_bank_workspace', 'mrphy_sequence_signal_fwd',
         'mrphy_sequence_signal_bwd')
EINVAL, EALIGN, ENOSPC = -1, -2, -3
BC0 = (None, 0, 0)
BCF = (FAKE, 0, 0)


# ---------------------------------------------------------------------------------------------
# the yardstick
# ---------------------------------------------------------------------------------------------
def test_yardstick_composition_is_signal_of_the_records():
    r"""``torch_signal(torch_sequence(.))`` against ``fused._signal_of`` on the time-major records, on the CPU: no map,
    one coil, an array -- and the last record is what ``Mlast`` is compared with."""
    K, pulse = 6, [0, 2, 2, 1, 0, 2]
    Q = _seeded(3, 2, 7, K)
    Mt = torch_sequence(Q['A'], Q['B'], K, pulse, Q['Mi'], Q['phase'], Q['rest'], Q['T1'], Q['T2'], Q['df'])
    assert Mt.shape == (2, 7, K, 3)
    gen = torch.Generator().manual_seed(6)
    for rx in (None, torch.randn((2, 7, 2), generator=gen, dtype=torch.float64),
               torch.randn((1, 7, 2, 3), generator=gen, dtype=torch.float64)):
        a, b = torch_signal(Mt, rx), fused._signal_of(Mt.movedim(-2, 0), rx)
        assert a.shape == b.shape == ((2, 2, K) if rx is None or rx.ndim == 3 else (2, 2, K, 3))
        assert float((a - b).abs().max()) <= 1e-13 * float(b.abs().max())
    # a one-hot map picks one spin's records
    rx = torch.zeros((2, 7, 2), dtype=torch.float64)
    rx[:, 4, 0] = 1
    assert torch.equal(torch_signal(Mt, rx), Mt[:, 4, :, :2].movedim(-1, 1))


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
    # A .. cs_sn sit where mrphy_ab_sequence_* have them (the adjoint: after its two cotangents), rx .. where
    # mrphy_train_signal_* have them
    seq_f, seq_b = (list(_lib.PROTOTYPES[f'mrphy_ab_sequence_{w}'][1]) for w in ('fwd', 'bwd'))
    trs_f, trs_b = (list(_lib.PROTOTYPES[f'mrphy_train_signal_{w}'][1]) for w in ('fwd', 'bwd'))
    fwd, bwd = (list(_lib.PROTOTYPES[n][1]) for n in NAMES[2:])
    assert fwd[:21] == seq_f[:21] and fwd[21:] == trs_f[19:]
    assert bwd[:5] == seq_b[:5] and bwd[7:23] == seq_b[6:22] and bwd[23:26] == trs_b[21:24]
    lib = mrphy_amd.require_library()
    assert lib.mrphy_abi_version() == _lib.ABI_VERSION == 5
    assert ('tu_sequence_signal.hip', None) in _lib.UNITS
    assert 'sequence_signal' in fused.__all__ and 'sequence_signal_rfgr' in fused.__all__


def _calls(lib):
    r"""``fwd(...)`` / ``bwd(...)`` with fake pointers (never dereferenced: no call here is valid on a problem that is not
    empty and well-formed enough to launch).  ``wb=None`` / ``bb=None``: the workspaces the queries ask for."""
    def fwd(A=FAKE, B=FAKE, P=3, pulse=FAKE, rs=FAKE, T1=BCF, T2=BCF, df=BCF, Mi=BCF, cs=FAKE, rx=FAKE, nRx=1, sig=FAKE,
            Ml=FAKE, ck=FAKE, work=FAKE, wb=None, N=2, nM=100, K=5, dtype=0):
        wb = lib.mrphy_sequence_signal_workspace(dtype, N, nM, K, 2 * max(nRx, 1)) if wb is None else wb
        return lib.mrphy_sequence_signal_fwd(dtype, A, B, P, pulse, rs, 0, *T1, *T2, *df, *Mi, cs, 0, rx, nRx, sig, Ml,
                                             ck, work, wb, N, nM, K, None)

    def bwd(A=FAKE, B=FAKE, P=3, pulse=FAKE, gs=FAKE, gl=FAKE, rs=FAKE, T1=BCF, T2=BCF, df=BCF, Mi=BCF, cs=FAKE, rx=FAKE,
            nRx=1, ck=FAKE, gA=FAKE, gB=FAKE, gC=FAKE, grest=FAKE, gMi=FAKE, gphi=FAKE, grx=FAKE, work=FAKE, wb=None,
            bank=FAKE, bb=None, N=2, nM=100, K=5, dtype=0):
        nQ = (gphi is not None) + (grest is not None)
        wb = lib.mrphy_sequence_signal_workspace(dtype, N, nM, K, max(nQ, 1)) if wb is None else wb
        bb = lib.mrphy_sequence_signal_bank_workspace(0, max(P, 1), max(N, 1), max(nM, 1)) if bb is None else bb
        return lib.mrphy_sequence_signal_bwd(dtype, A, B, P, pulse, gs, gl, rs, 0, *T1, *T2, *df, *Mi, cs, 0, rx, nRx, ck,
                                             gA, gB, gC, grest, gMi, gphi, grx, work, wb, bank, bb, N, nM, K, None)
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
    'no coil': dict(nRx=0),
    'a negative coil count': dict(nRx=-1),
    'no map for two coils': dict(rx=None, nRx=2),
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
        assert fwd(dtype=dtype, wb=1 << 30) == EINVAL and bwd(dtype=dtype, wb=1 << 30) == EINVAL, ('dtype', dtype)
    assert fwd(N=-1) == EINVAL and fwd(nM=-1) == EINVAL and bwd(N=-2) == EINVAL and bwd(nM=-100) == EINVAL
    assert fwd(K=-1) == EINVAL and bwd(K=-3) == EINVAL, 'a negative number of repetitions'
    assert fwd(N=65536) == EINVAL and bwd(N=65536) == EINVAL, 'N > 65535: the batch entry is blockIdx.y'
    for dtype in (0, 1):
        over = lib.mrphy_train_signal_max_rx(dtype) + 1
        assert fwd(dtype=dtype, nRx=over) == EINVAL and bwd(dtype=dtype, nRx=over) == EINVAL, 'coils over the limit'
    assert fwd(sig=None) == EINVAL, 'a null output'
    assert fwd(work=None) == EINVAL, 'no workspace'
    assert bwd(gs=None, gl=None) == EINVAL, 'no cotangent'
    assert bwd(ck=None) == EINVAL, 'no checkpoints'
    assert bwd(gA=None, gB=None, gC=None, grest=None, gMi=None, gphi=None, grx=None) == EINVAL, 'nothing to compute'
    assert bwd(work=None) == EINVAL and bwd(work=None, gphi=None) == EINVAL and bwd(work=None, grest=None) == EINVAL, \
        'the sums over the spins need their workspace'
    assert bwd(bank=None) == EINVAL and bwd(bank=None, gA=None) == EINVAL and bwd(bank=None, gB=None) == EINVAL, \
        'the bank gradients need their workspace'
    # a short workspace
    for nRx in (1, 3, 8):
        need = lib.mrphy_sequence_signal_workspace(0, 2, 100, 5, 2 * nRx)
        assert fwd(nRx=nRx, wb=need - 1) == ENOSPC and fwd(nRx=nRx, wb=0) == ENOSPC, nRx
    two, one = (lib.mrphy_sequence_signal_workspace(0, 2, 100, 5, q) for q in (2, 1))
    assert bwd(wb=two - 1) == ENOSPC and bwd(wb=one) == ENOSPC, 'a phase and a rest row'
    assert bwd(grest=None, wb=one - 1) == ENOSPC and bwd(gphi=None, wb=one - 1) == ENOSPC and bwd(gphi=None, wb=0) == ENOSPC
    for dtype in (0, 1):
        assert bwd(dtype=dtype, bb=3 * 12 * 200 * 8 - 8) == ENOSPC and bwd(dtype=dtype, bb=0) == ENOSPC, 'a short bank'
    for dtype, odd in ((0, FAKE + 2), (1, FAKE + 4)):
        for k in ('A', 'B', 'rx', 'sig', 'Ml'):
            assert fwd(dtype=dtype, **{k: odd}) == EALIGN, (dtype, k)
        for k in ('T1', 'T2', 'df', 'Mi'):
            assert fwd(dtype=dtype, **{k: (odd, 0, 0)}) == EALIGN and bwd(dtype=dtype, **{k: (odd, 0, 0)}) == EALIGN
        for k in ('A', 'B', 'gl', 'rx', 'gA', 'gB', 'gMi', 'grx'):
            assert bwd(dtype=dtype, **{k: odd}) == EALIGN, (dtype, k)
        # the tables, the checkpoints, the workspaces, the cotangent table and the fp64 gradients have their own
        # element sizes whatever the data type
        for k in ('rs', 'cs', 'ck', 'work'):
            assert fwd(dtype=dtype, **{k: FAKE + 4}) == EALIGN and bwd(dtype=dtype, **{k: FAKE + 4}) == EALIGN, k
        assert fwd(dtype=dtype, pulse=FAKE + 2) == EALIGN and bwd(dtype=dtype, pulse=FAKE + 2) == EALIGN
        for k in ('gs', 'gC', 'grest', 'gphi', 'bank'):
            assert bwd(dtype=dtype, **{k: FAKE + 4}) == EALIGN, (dtype, k)
    # a null pointer is reported before a misaligned one
    assert fwd(pulse=None, A=FAKE + 2) == EINVAL and bwd(pulse=None, rs=FAKE + 4) == EINVAL
    assert fwd(sig=None, A=FAKE + 2) == EINVAL and bwd(ck=None, rs=FAKE + 4) == EINVAL
    # ... a call right in every argument would be a launch: not made here


def test_empty_problems_are_a_success_whatever_the_pointers_are():
    fwd, bwd = _calls(mrphy_amd.require_library())
    null = dict(A=None, B=None, pulse=None, rs=None, T1=BCF, T2=BC0, df=BCF, Mi=BC0, cs=None, rx=None, nRx=7, work=None,
                wb=0)
    for size in (dict(nM=0), dict(N=0), dict(K=0), dict(N=0, nM=0, K=0)):
        assert fwd(sig=None, Ml=None, ck=None, **null, **size) == 0, size
        assert bwd(gs=None, gl=None, ck=None, gA=None, gB=None, gC=None, grest=None, gMi=None, gphi=None, grx=None,
                   bank=None, bb=0, **null, **size) == 0, size
    assert fwd(K=0, dtype=7) == EINVAL and bwd(N=0, nM=-1) == EINVAL and fwd(N=0, K=-1) == EINVAL
    assert fwd(K=0, P=0) == EINVAL and bwd(nM=0, P=-1) == EINVAL, 'a bank holds at least one pulse'


def test_workspace_queries_are_their_documented_products():
    r"""``Pw = min(ceil(nM / 64), 2048)`` partial rows of `(N, rows, K)` fp64 sums, whatever ``nM``; the bank's
    `(P, 12, N nM)` fp64 whatever the data type."""
    lib = mrphy_amd.require_library()
    q, b = lib.mrphy_sequence_signal_workspace, lib.mrphy_sequence_signal_bank_workspace
    for dtype in (0, 1):
        for N, nM, K, rows in ((1, 1, 1, 2), (2, 100, 7, 2), (3, 64 * 5 + 1, 19, 16), (2, 64 * MAX_WAVES, 3, 1),
                               (2, 64 * MAX_WAVES + 100, 19, 2), (1, 64 ** 3, 256, 16)):
            Pw = min(-(-nM // 64), MAX_WAVES)
            assert q(dtype, N, nM, K, rows) == Pw * N * rows * K * 8, (N, nM, K, rows)
            assert q(dtype, N, nM, K, rows) == lib.mrphy_train_signal_workspace(dtype, N, nM, K, rows)
        for bad in ((0, 5, 5, 2), (2, 0, 5, 2), (2, 5, 0, 2), (2, 5, 5, 0), (-1, 5, 5, 2)):
            assert q(dtype, *bad) == 0, bad
        assert b(dtype, 3, 2, 100) == 3 * 12 * 200 * 8 and b(dtype, 1, 1, 64 ** 3) == 12 * 64 ** 3 * 8
        assert b(dtype, 3, 2, 100) == lib.mrphy_ab_sequence_bwd_workspace(dtype, 3, 2, 100)
        assert b(dtype, 0, 2, 100) == 0 and b(dtype, 3, 0, 100) == 0 and b(dtype, 3, 2, -1) == 0
    assert q(2, 2, 100, 7, 2) == 0 and b(5, 3, 2, 100) == 0, 'data types only'


# ---------------------------------------------------------------------------------------------
# the Python layer
# ---------------------------------------------------------------------------------------------
def test_python_wrappers_refuse_cpu_tensors():
    A, B = _cpu_bank()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.sequence_signal(A, B, pulse=[0, 1, 2, 1])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.sequence_signal(A[:1], B[:1], n=4, rx=torch.ones(1, 5, 2), demod=True, return_last=True)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.sequence_signal(A, B, pulse=torch.tensor([0, 2], dtype=torch.int32), rest=torch.full((2, 2), 5e-3),
                              rx=torch.ones(2, 5, 2, 3))
    rf, gr, loc = torch.zeros(3, 2, 2, 16), torch.zeros(1, 2, 3, 16), torch.zeros(2, 5, 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.sequence_signal_rfgr(rf, gr, loc, pulse=[0, 1, 2, 2], rest=torch.tensor(5e-3), T1=torch.ones(2, 5),
                                   T2=torch.ones(2, 5))


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
        fused.sequence_signal(A, B, pulse=pulse)
    assert str(got.value) == str(want.value)
    rf, gr, loc = torch.zeros(3, 2, 2, 16), torch.zeros(1, 2, 3, 16), torch.zeros(2, 5, 3)
    with pytest.raises(ValueError, match=f'repetition {k}') as got:
        fused.sequence_signal_rfgr(rf, gr, loc, pulse=pulse)
    assert str(got.value) == str(want.value)


def test_python_wrapper_checks_the_schedule_the_length_the_rest_and_the_receive_map():
    A, B = _cpu_bank()
    with pytest.raises(ValueError, match='`pulse` is required'):
        fused.sequence_signal(A, B, n=4)
    with pytest.raises(ValueError, match=r'must be \(K,\)'):
        fused.sequence_signal(A, B, pulse=torch.zeros(2, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match='give `n`'):
        fused.sequence_signal(A[:1], B[:1])
    with pytest.raises(ValueError, match='disagrees'):
        fused.sequence_signal(A, B, n=3, pulse=[0, 1, 2, 0])
    with pytest.raises(ValueError, match='disagrees'):
        fused.sequence_signal(A, B, pulse=[0, 1, 2], phase=torch.zeros(2, 4))
    with pytest.raises(ValueError, match='must be'):
        fused.sequence_signal(A, B, pulse=[0] * 4, phase=torch.zeros(3, 4))          # neither N nor 1 rows
    for n in (True, 2.0, -1, '3'):
        with pytest.raises(ValueError, match='int >= 0'):
            fused.sequence_signal(A, B, n=n, pulse=[0])
    for shape in ((3,), (2, 3), (3, 4), (2, 4, 1), (4, 2), (2, 1), (1, 1)):           # N = 2, K = 4
        with pytest.raises(ValueError, match='`rest`'):
            fused.sequence_signal(A, B, pulse=[0, 1, 2, 0], rest=torch.full(shape, 5e-3))
    for rx in (torch.ones(2, 5), torch.ones(2, 5, 3), torch.ones(2, 4, 2), torch.ones(2, 5, 2, 3, 1), torch.ones(3, 5, 2),
               torch.ones(2, 5, 2, 0)):
        with pytest.raises(ValueError, match='`rx`'):
            fused.sequence_signal(A, B, pulse=[0, 1, 2], rx=rx)
