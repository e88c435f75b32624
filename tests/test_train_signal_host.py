r"""``fused.train_signal`` / ``fused.train_signal_rfgr`` without a GPU: the entry points ``mrphy_train_signal_*`` are
exported, declared and bound alike and refuse bad arguments before any launch; the workspace query is
``P · N · rows · K · 8``; the Python layer refuses CPU tensors, a contradictory number of repetitions and an ``rx`` of the
wrong rank; and the yardstick of the GPU tests -- ``test_ab_train_host.torch_train`` followed by the complex sum
:func:`torch_signal` -- against ``fused._signal_of`` and on identity (b) of ``test_ab_train_host`` carried to the sum."""
import ctypes
import os
import re
from math import pi as π

import pytest
import torch

import mrphy_amd
from mrphy_amd import _lib, fused
from test_ab_rfgr_host import CTYPE
from test_ab_train_host import identity_problem, torch_train
from util import FAKE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('mrphy_train_signal_ck_every', 'mrphy_train_signal_max_rx', 'mrphy_train_signal_workspace',
         'mrphy_train_signal_fwd', 'mrphy_train_signal_bwd')
EINVAL, EALIGN, ENOSPC = -1, -2, -3
BC0 = (None, 0, 0)
BCF = (FAKE, 0, 0)
MAX_WAVES = 2048            # geom.hpp: TRS_MAX_WAVES, the cap on the partial rows P


# ---------------------------------------------------------------------------------------------
# the yardstick: the complex product with rx and the sum over the spins, in plain torch
# ---------------------------------------------------------------------------------------------
def torch_signal(Mt, rx=None):
    r"""``sig`` `(N, xy, K)` -- `(N, xy, K, nRx)` for ``rx`` `(N ⊻ 1, *Nd, xy, nRx)` -- of ``Mt`` `(N, *Nd, K, 3)`:
    ``(rx_re + i rx_im)(Mx + i My)`` summed over ``*Nd``, written with complex numbers."""
    N, K = Mt.shape[0], Mt.shape[-2]
    m = torch.complex(Mt[..., 0], Mt[..., 1]).reshape(N, -1, K)                      # (N, nM, K)
    if rx is None:
        s = m.sum(1)
        return torch.stack((s.real, s.imag), dim=1)
    coils = rx.ndim == Mt.ndim
    r = rx if coils else rx[..., None]
    r = r.expand((N,) + tuple(r.shape[1:]))
    r = torch.complex(r[..., 0, :], r[..., 1, :]).reshape(N, -1, r.shape[-1])         # (N, nM, nRx)
    s = (m[..., None] * r[:, :, None, :]).sum(1)                                     # (N, K, nRx)
    s = torch.stack((s.real, s.imag), dim=1)
    return s if coils else s[..., 0]


def demodulated(sig, phase):
    r"""Sample ``k`` times ``exp(-iφ_k)``: ``sig`` `(N, xy, K[, nRx])`, ``phase`` `(N ⊻ 1, K)`, in fp64."""
    φ = phase.double().reshape(phase.shape + (1,) * (sig.ndim - 3))
    z = torch.complex(sig[:, 0].double(), sig[:, 1].double()) * torch.exp(-1j * φ)
    return torch.stack((z.real, z.imag), dim=1)


def test_yardstick_sum_is_signal_of():
    r"""``torch_signal`` against ``fused._signal_of`` (time-major ``Mt``) on the CPU: no map, one coil, an array."""
    gen = torch.Generator().manual_seed(5)
    Mt = torch.randn((2, 4, 5, 7, 3), generator=gen, dtype=torch.float64)           # (N, 4, 5, K, 3)
    for rx in (None, torch.randn((2, 4, 5, 2), generator=gen, dtype=torch.float64),
               torch.randn((2, 4, 5, 2, 3), generator=gen, dtype=torch.float64)):
        a, b = torch_signal(Mt, rx), fused._signal_of(Mt.movedim(-2, 0), rx)
        assert a.shape == b.shape == ((2, 2, 7) if rx is None or rx.ndim == 4 else (2, 2, 7, 3))
        assert float((a - b).abs().max()) <= 1e-13 * float(b.abs().max())


# ---------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------
def _declared(name):
    r"""``test_ab_rfgr_host._declared`` that also reads a ``(void)`` argument list."""
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mrphy_hip.h')).read(), flags=re.S)
    m = re.search(r'\b(\w+)\s+' + name + r'\s*\(([^)]*)\)\s*;', src)
    assert m, f'{name} is not declared in mrphy_hip.h'
    if m.group(2).strip() == 'void':
        return CTYPE[m.group(1)], []
    args = [re.sub(r'\s*\w+$', '', a.strip()).replace(' *', '*') for a in m.group(2).split(',')]
    return CTYPE[m.group(1)], [CTYPE[a] for a in args]


def test_symbols_are_exported_declared_and_bound_alike():
    raw = ctypes.CDLL(mrphy_amd.build())
    for name in NAMES:
        assert hasattr(raw, name), f'{name} is not exported'
        assert name in _lib.PROTOTYPES, f'{name} is not bound in _lib.py'
        res, args = _declared(name)
        assert (_lib.PROTOTYPES[name][0], list(_lib.PROTOTYPES[name][1])) == (res, args), name
    # A .. cs_sn sit where mrphy_ab_train_* have them (the adjoint: after its two cotangents)
    assert list(_lib.PROTOTYPES[NAMES[3]][1][:19]) == list(_lib.PROTOTYPES['mrphy_ab_train_fwd'][1][:19])
    assert list(_lib.PROTOTYPES[NAMES[4]][1][5:21]) == list(_lib.PROTOTYPES['mrphy_ab_train_bwd'][1][4:20])
    lib = mrphy_amd.require_library()
    assert lib.mrphy_abi_version() == _lib.ABI_VERSION == 5
    assert ('tu_train_signal.hip', None) in _lib.UNITS
    assert 'train_signal' in fused.__all__ and 'train_signal_rfgr' in fused.__all__
    assert lib.mrphy_train_signal_ck_every() >= 1
    assert lib.mrphy_train_signal_max_rx(0) == 8 and lib.mrphy_train_signal_max_rx(1) in (4, 8)
    for code in (-1, 2, 3, 4, 9):
        assert lib.mrphy_train_signal_max_rx(code) == 0, code


def _calls(lib):
    r"""``fwd(...)`` / ``bwd(...)`` with fake pointers (never dereferenced: no call here is valid on a problem that is not
    empty and well-formed enough to launch).  ``wb=None``: the workspace the query asks for."""
    def fwd(A=FAKE, B=FAKE, rest=FAKE, T1=BCF, T2=BCF, df=BCF, Mi=BCF, cs=FAKE, rx=FAKE, nRx=1, sig=FAKE, Ml=FAKE,
            ck=FAKE, work=FAKE, wb=None, N=2, nM=100, K=5, dtype=0):
        wb = lib.mrphy_train_signal_workspace(dtype, N, nM, K, 2 * max(nRx, 1)) if wb is None else wb
        return lib.mrphy_train_signal_fwd(dtype, A, B, rest, 0, *T1, *T2, *df, *Mi, cs, 0, rx, nRx, sig, Ml, ck,
                                          work, wb, N, nM, K, None)

    def bwd(A=FAKE, B=FAKE, gs=FAKE, gl=FAKE, rest=FAKE, T1=BCF, T2=BCF, df=BCF, Mi=BCF, cs=FAKE, rx=FAKE, nRx=1,
            ck=FAKE, gA=FAKE, gB=FAKE, gC=FAKE, gMi=FAKE, gphi=FAKE, grx=FAKE, work=FAKE, wb=None, N=2, nM=100, K=5,
            dtype=0):
        wb = lib.mrphy_train_signal_workspace(dtype, N, nM, K, 1) if wb is None else wb
        return lib.mrphy_train_signal_bwd(dtype, A, B, gs, gl, rest, 0, *T1, *T2, *df, *Mi, cs, 0, rx, nRx, ck,
                                          gA, gB, gC, gMi, gphi, grx, work, wb, N, nM, K, None)
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
    for dtype in (-1, 2, 3, 4, 5, 17):          # data types only, as mrphy_ab_train_*
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
    assert bwd(gA=None, gB=None, gC=None, gMi=None, gphi=None, grx=None) == EINVAL, 'nothing to compute'
    assert bwd(work=None) == EINVAL, 'the phase gradient needs the workspace'
    # a short workspace
    for nRx in (1, 3, 8):
        need = lib.mrphy_train_signal_workspace(0, 2, 100, 5, 2 * nRx)
        assert fwd(nRx=nRx, wb=need - 1) == ENOSPC and fwd(nRx=nRx, wb=0) == ENOSPC, nRx
    assert bwd(wb=lib.mrphy_train_signal_workspace(0, 2, 100, 5, 1) - 1) == ENOSPC
    for dtype, odd in ((0, FAKE + 2), (1, FAKE + 4)):
        for k in ('A', 'B', 'rest', 'rx', 'sig', 'Ml'):
            assert fwd(dtype=dtype, **{k: odd}) == EALIGN, (dtype, k)
        for k in ('T1', 'T2', 'df', 'Mi'):
            assert fwd(dtype=dtype, **{k: (odd, 0, 0)}) == EALIGN and bwd(dtype=dtype, **{k: (odd, 0, 0)}) == EALIGN
        for k in ('A', 'B', 'gl', 'rest', 'rx', 'gA', 'gB', 'gC', 'gMi', 'gphi', 'grx'):
            assert bwd(dtype=dtype, **{k: odd}) == EALIGN, (dtype, k)
        # the phase table, the checkpoints, the workspace and the cotangent table are fp64 whatever the data type
        for k in ('cs', 'ck', 'work'):
            assert fwd(dtype=dtype, **{k: FAKE + 4}) == EALIGN and bwd(dtype=dtype, **{k: FAKE + 4}) == EALIGN, k
        assert bwd(dtype=dtype, gs=FAKE + 4) == EALIGN
    # ... a call right in every argument would be a launch: not made here


def test_empty_problems_are_a_success_whatever_the_pointers_are():
    fwd, bwd = _calls(mrphy_amd.require_library())
    null = dict(A=None, B=None, rest=None, T1=BCF, T2=BC0, df=BCF, Mi=BC0, cs=None, rx=None, nRx=7, work=None, wb=0)
    for size in (dict(nM=0), dict(N=0), dict(K=0), dict(N=0, nM=0, K=0)):
        assert fwd(sig=None, Ml=None, ck=None, **null, **size) == 0, size
        assert bwd(gs=None, gl=None, ck=None, gA=None, gB=None, gC=None, gMi=None, gphi=None, grx=None, **null,
                   **size) == 0, size
    assert fwd(K=0, dtype=7) == EINVAL and bwd(N=0, nM=-1) == EINVAL and fwd(N=0, K=-1) == EINVAL


def test_workspace_query_is_P_N_rows_K_doubles():
    r"""``P = min(ceil(nM / 64), 2048)`` partial rows of `(N, rows, K)` fp64 sums, whatever ``nM``."""
    lib = mrphy_amd.require_library()
    for dtype in (0, 1):
        for N, nM, K, rows in ((1, 1, 1, 2), (2, 100, 7, 2), (3, 64 * 5 + 1, 19, 16), (2, 64 * MAX_WAVES, 3, 1),
                               (2, 64 * MAX_WAVES + 100, 19, 6), (1, 64 ** 3, 256, 16)):
            P = min(-(-nM // 64), MAX_WAVES)
            assert lib.mrphy_train_signal_workspace(dtype, N, nM, K, rows) == P * N * rows * K * 8, (N, nM, K, rows)
        for bad in ((0, 5, 5, 2), (2, 0, 5, 2), (2, 5, 0, 2), (2, 5, 5, 0), (-1, 5, 5, 2)):
            assert lib.mrphy_train_signal_workspace(dtype, *bad) == 0, bad
    assert lib.mrphy_train_signal_workspace(2, 2, 100, 7, 2) == 0, 'data types only'


# ---------------------------------------------------------------------------------------------
# the Python layer
# ---------------------------------------------------------------------------------------------
def test_python_wrappers_refuse_cpu_tensors():
    A, B = torch.eye(3).expand(1, 5, 3, 3) * 0.9, torch.zeros(1, 5, 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.train_signal(A, B, n=4)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.train_signal(A, B, phase=torch.zeros(1, 4), rx=torch.ones(1, 5, 2), demod=True, return_last=True)
    rf, gr, loc = torch.zeros(1, 2, 16), torch.zeros(1, 3, 16), torch.zeros(1, 5, 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.train_signal_rfgr(rf, gr, loc, n=4, rest=torch.tensor(5e-3), T1=torch.ones(1, 5), T2=torch.ones(1, 5))


def test_python_wrapper_wants_one_number_of_repetitions_and_a_receive_map_of_its_rank():
    A, B = torch.eye(3).expand(2, 5, 3, 3) * 0.9, torch.zeros(2, 5, 3)
    with pytest.raises(ValueError, match='give `n`'):
        fused.train_signal(A, B)
    with pytest.raises(ValueError, match='disagrees'):
        fused.train_signal(A, B, n=3, phase=torch.zeros(2, 4))
    with pytest.raises(ValueError, match='must be'):
        fused.train_signal(A, B, phase=torch.zeros(3, 4))          # neither N nor 1 rows
    for n in (True, 2.0, -1, '3'):
        with pytest.raises(ValueError, match='int >= 0'):
            fused.train_signal(A, B, n=n)
    for rx in (torch.ones(2, 5), torch.ones(2, 5, 3), torch.ones(2, 4, 2), torch.ones(2, 5, 2, 3, 1), torch.ones(3, 5, 2),
               torch.ones(2, 5, 2, 0)):
        with pytest.raises(ValueError, match='`rx`'):
            fused.train_signal(A, B, n=3, rx=rx)


# ---------------------------------------------------------------------------------------------
# an identity of the yardstick: a known answer of the GPU tests
# ---------------------------------------------------------------------------------------------
def test_demodulated_linear_phase_signal_is_the_shifted_off_resonance_signal():
    r"""Identity (b) of ``test_ab_train_host`` carried to the sum: ``φ_k = kψ``, the signal times ``exp(-iφ_k)`` is the
    zero-phase train's with ``Δf' = Δf + ψ / (2π rest)`` -- with a complex receive map too; the other sign is O(1) away."""
    Q = identity_problem()
    K, ψ = 24, 0.7
    φ = (ψ * torch.arange(K, dtype=torch.float64)).expand(2, K)
    rx = torch.randn((2, 100, 2, 3), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    Mt = torch_train(Q['A'], Q['B'], K, None, φ, Q['rest'], Q['T1'], Q['T2'], Q['df'])
    for r in (None, rx[..., 0], rx):
        back = demodulated(torch_signal(Mt, r), φ)
        for sign, close in ((1, True), (-1, False)):
            df = Q['df'] + sign * ψ / (2 * π * Q['rest'][:, None])
            want = torch_signal(torch_train(Q['A'], Q['B'], K, None, None, Q['rest'], Q['T1'], Q['T2'], df), r)
            d = float((back - want).abs().max()) / float(want.abs().max())
            assert (d <= 1e-12) if close else (d > 0.05), (sign, d)
