r"""``fused.signal_rfgr`` (K2s and the signal mode of K2b) on every operand form ``test_fused_operands.py`` feeds the other
fused kernels -- ``cases.fused_operand_variants``, each with a receive map ``rx`` in a spelling of its own (batch-1, absent,
stride-0, three coils on a ``*Nd`` grid, one weight per plane, fp64 on the CPU, a permuted view, off the 16-B grid) --
and on steps of exactly zero field (``cases.zero_field_case``).

Per case and record stride, with the loss ``<w_s, sig> + <w, Mo>``: (1) a spelling changes no bit -- ``sig``, ``Mo`` and
the three gradients as given against the same numbers materialised over ``(N, nM)``; (2) ``Mo`` == ``blochsim_rfgr`` bit
for bit; (3) ``sig`` against S64, the fp64 product-and-sum of ``blochsim_rfgr_traj``'s own records: the gate, and in fp32
the elementwise bound ``(nM + 3) 2^-24 Σ (|rx_re M_a| + |rx_im M_b|)`` of ``test_signal.py``, which holds for any order
of summation; (4) ``sig``, ``Mo`` and the gradients within the gates (``tests/util.py``) of the CPU oracle run in fp64 on
the operands as given, and the gradients within them of the two-kernel route (``rfgr2beff`` + ``sims.blochsim``, which
shares no code with K2b); (5) a second run gives the same bits.

The signal loss is a trajectory loss with the cotangent ``(rx_re w0 + rx_im w1, rx_re w1 - rx_im w0, 0)`` per record
(summed over the receive coils) plus ``w`` on the last record: that is what the oracle and the two-kernel route are
given (``test_fused_operands._run(..., cot=)``).  ``precision('fast')`` is held to (1), (2), (3), (5) and to the
two-kernel route in the same mode; its distance to the oracle goes to the ledger (``sigops.*``) unasserted, as
``fusedops.*`` does."""
from math import prod

import pytest

from gpu_common import *  # noqa: F401,F403
from mrphy_amd.fused import _signal_composed, _traj_ends
from test_fused_operands import MODES, VARIANTS, _run, _same_bits
from test_signal import _sig64
from util import ATOL64, REL32

pytestmark = pytest.mark.gpu

EVERYS = (1, 5, 16)             # the EV1 build; a compare per step; one reduction per checkpoint segment
GRADS = ('grad_Mi', 'grad_rf', 'grad_gr')
NAMES = ('sig', 'Mo') + GRADS


def _over_gate(a, b, tag, what):
    r"""``assert_close`` that returns the distance over its gate (fp64: max abs / 1e-9; fp32: relative L2 / 1e-5)."""
    assert a.shape == b.shape, (what, a.shape, b.shape)
    r = max_abs(a, b) / ATOL64 if tag == 'f64' else rel_l2(a, b) / REL32
    assert r <= 1.0, f'{what}: {r:.3e} of the {"max-abs 1e-9" if tag == "f64" else "relative-L2 1e-5"} gate'
    return r


def _rx_coils(v, dtype):
    r"""The receive map as the kernels take it, in fp64 on the CPU: `(N, nM, 2, nRx)` of the values rounded to ``dtype``
    (``None``: the weight ``(1, 0)``), and whether ``rx`` has a coil axis."""
    N, Nd = v['M0'].shape[0], tuple(v['M0'].shape[1:-1])
    rx = v.get('rx')
    if rx is None:
        r = torch.zeros((N, prod(Nd), 2, 1), dtype=torch.float64)
        r[:, :, 0] = 1
        return r, False
    coils = rx.ndim == v['M0'].ndim + 1
    r = rx.to(dtype).double().expand((N,) + Nd + tuple(rx.shape[1 + len(Nd):]))
    return r.reshape(N, -1, 2, rx.shape[-1] if coils else 1), coils


def _sig_weights(shape):
    n = 1
    for d in shape:
        n *= d
    return torch.cos(torch.arange(n, dtype=torch.float64) * 0.37 + 0.2).reshape(shape)


def _traj_cotangent(v, r, ws):
    r"""The cotangent of the trajectory `(N, *Nd, nRec, 3)` that ``<ws, sig> + <w, Mo>`` is (module docstring), fp64."""
    N, nM, nRx = r.shape[0], r.shape[1], r.shape[3]
    w4 = ws.reshape(N, 2, -1, nRx)
    rr, ri = r[:, :, 0], r[:, :, 1]
    ein = lambda a, b: torch.einsum('nsc,njc->nsj', a, b)  # noqa: E731
    cot = torch.zeros((N, nM, w4.shape[2], 3), dtype=torch.float64)
    cot[..., 0] = ein(rr, w4[:, 0]) + ein(ri, w4[:, 1])
    cot[..., 1] = ein(rr, w4[:, 1]) - ein(ri, w4[:, 0])
    cot[:, :, -1] += v['w'].double().reshape(N, nM, 3)
    return cot.reshape(tuple(v['M0'].shape[:-1]) + (w4.shape[2], 3))


def _signal(v, every, ws, rx_on_cpu=False, composed=False):
    r"""``sig, Mo, grad_Mi, grad_rf, grad_gr`` of ``<ws, sig> + <w, Mo>`` through ``fused.signal_rfgr`` (``composed``:
    through ``fused._signal_composed``), the operands AS GIVEN (``test_fused_operands._run``); ``rx_on_cpu``: the
    receive map stays where and what it is."""
    leaf = lambda x: place(x).detach().requires_grad_(True)  # noqa: E731
    Mi, rf, gr = leaf(v['M0']), leaf(v['rf']), leaf(v['gr'])
    rx = v.get('rx') if rx_on_cpu else place(v.get('rx'))
    kw = dict(Δf=place(v['Δf']), b1Map=place(v['b1Map']), γ_beff=place(v['γ_beff']), T1=place(v['T1']),
              T2=place(v['T2']), γ=place(v['γ']), dt=place(v['dt']))
    if composed:
        sig, Mo = _signal_composed(Mi, rf, gr, place(v['loc']), every, rx, dict(kw, consts=None))
    else:
        sig, Mo = fused.signal_rfgr(Mi, rf, gr, place(v['loc']), every=every, rx=rx, return_Mo=True, **kw)
    torch.autograd.backward([sig, Mo], [dev(ws.to(sig.dtype)), place(v['w'])])
    return dict(sig=sig.detach(), Mo=Mo.detach(), grad_Mi=Mi.grad, grad_rf=rf.grad, grad_gr=gr.grad)


def _f64(v):
    return {k: (x.double() if isinstance(x, torch.Tensor) else x) for k, x in v.items()}


def _invariants(v, tag, mode, every, key, Mo_ref, dense=None, zero=None, rx_on_cpu=False, composed=False):
    r"""Invariants (1)-(5) of the module docstring for one case and one record stride; returns the results.  ``Mo_ref``:
    ``blochsim_rfgr``'s.  ``zero``: `(N, nT)` mask of the zero-field steps -- the pulse gradients are compared on those
    steps alone as well, and on batch entry 1's all-zero segment alone.  ``composed``: a case the signal kernels do not
    cover -- ``sig`` and ``Mo`` must be the composed route's bits."""
    dtype = DT[tag]
    nT = v['rf'].shape[2]
    nRec = len(_traj_ends(nT, every))
    r, coils = _rx_coils(v, dtype)
    N, nM, nRx = r.shape[0], r.shape[1], r.shape[3]
    ws = _sig_weights((N, 2, nRec) + ((nRx,) if coils else ())).to(dtype).double()   # the numbers the kernels get
    cot = _traj_cotangent(v, r, ws)
    led = f'sigops.{key}.{tag}.{mode}.every{every}'

    fu = _signal(v, every, ws, rx_on_cpu)
    assert fu['sig'].shape == ws.shape and fu['sig'].dtype == dtype, (key, fu['sig'].shape)
    for k in NAMES:
        assert bool(torch.isfinite(fu[k]).all()), (key, k)
    if dense is not None:                                                      # (1) the spelling changes nothing
        fd = _signal(dense, every, ws)
        for k in ('sig', 'Mo', 'grad_Mi'):
            _same_bits(fu[k].reshape(fd[k].shape), fd[k], f'{key}: {k}, as given vs dense')
        for k in ('grad_rf', 'grad_gr'):
            if fu[k].shape == fd[k].shape:
                _same_bits(fu[k], fd[k], f'{key}: {k}, as given vs dense')
            else:                                                              # a batch-1 pulse, expanded in `dense`
                assert_close(fu[k], fd[k].sum(0, keepdim=True), tag, f'{key}: {k} vs dense summed over N')
    if composed:
        co = _signal(v, every, ws, rx_on_cpu, composed=True)
        for k in ('sig', 'Mo'):
            _same_bits(fu[k], co[k], f'{key}: {k} vs the composed route')
        for k in GRADS:
            assert_close(fu[k], co[k], tag, f'{key}: {k} vs the composed route')
    _same_bits(fu['Mo'], Mo_ref, f'{key}: Mo vs blochsim_rfgr (every={every})')    # (2)
    tr = _run('fused', v, every, cot=cot.to(dtype))                            # (3) S64 of the trajectory's own records
    Mt = tr['out'].reshape(N, nM, nRec, 3)
    s4 = fu['sig'].reshape(N, 2, nRec, nRx)
    worst = 0.0
    for c in range(nRx):
        S64, A64 = _sig64(Mt, None if v.get('rx') is None else r[..., c])
        worst = max(worst, _over_gate(s4[..., c], S64, tag, f'{key}: sig (coil {c}) vs S64 (every={every})'))
        if tag == 'f32':
            ratio = float(((s4[..., c].double().cpu() - S64).abs() / ((nM + 3) * 2.0 ** -24 * A64)).max())
            record(f'{led}.coil{c}.elementwise_over_bound', ratio, 1.0)
            assert ratio <= 1.0, (key, every, c, ratio)
    record(f'{led}.sig_vs_S64.over_gate', worst, 1.0)
    two = _run('two', v, every, cot=cot.to(dtype))                             # (4) the yardsticks
    _same_bits(tr['out'], two['out'], f'{key}: the trajectory, fused vs two-kernel')
    record(f'{led}.grads_vs_two_kernel.over_gate',
           max(_over_gate(fu[k], two[k], tag, f'{key}: {k} vs two-kernel (every={every})') for k in GRADS), 1.0)
    ora = _run('oracle', _f64(v), every, cot=cot)
    Mt_o = ora['out'].reshape(N, nM, nRec, 3)
    ora['sig'] = torch.stack([_sig64(Mt_o, None if v.get('rx') is None else r[..., c])[0] for c in range(nRx)],
                             dim=-1).reshape(ws.shape)
    ora['Mo'] = ora['out'][..., -1, :]
    sl = lambda x: x.movedim(2, 1)[zero.to(x.device)]                          # noqa: E731
    seg = list(cases.ZERO_SEGMENT)
    if mode == 'precise':
        record(f'{led}.vs_oracle.over_gate',
               max(_over_gate(fu[k], ora[k], tag, f'{key}: {k} vs oracle (every={every})') for k in NAMES), 1.0)
        if zero is not None:
            worst = 0.0
            for k in ('grad_rf', 'grad_gr'):
                assert float(sl(ora[k]).abs().max()) > 0.1 and float(ora[k][1, :, seg].abs().max()) > 0.1, (key, k)
                worst = max(worst,
                            _over_gate(sl(fu[k]), sl(ora[k]), tag, f'{key}: {k} on the zero-field steps vs oracle'),
                            _over_gate(fu[k][1, :, seg], ora[k][1, :, seg], tag, f'{key}: {k} on the all-zero segment'))
            record(f'{led}.zero_steps.vs_oracle.over_gate', worst, 1.0)
    else:
        record(f'{led}.worst_rel_l2_vs_oracle', max(rel_l2(fu[k], ora[k]) for k in NAMES),
               note='largest of sig, Mo, grad_Mi, grad_rf, grad_gr; not asserted')
        if zero is not None:
            record(f'{led}.zero_steps.worst_rel_l2_vs_oracle',
                   max(rel_l2(sl(fu[k]), sl(ora[k])) for k in ('grad_rf', 'grad_gr')), note='not asserted')
    again = _signal(v, every, ws, rx_on_cpu)                                   # (5) determinism
    for k in NAMES:
        _same_bits(fu[k], again[k], f'{key}: {k}, second run')
    return fu


def _forms_arrive(name, given):
    r"""The spellings under test reach ``signal_rfgr`` as such."""
    rx = given['rx']
    if name == 'compact_mixed':
        assert rx.shape[0] == 1 and given['M0'].shape[0] == 2
    if name == 'scalars':
        assert rx is None
    if name == 'expanded':
        assert place(rx).stride(1) == 0 and rx.shape[1] == cases.FUSED_NM
    if name == 'cube':
        assert tuple(rx.shape) == (2,) + cases.FUSED_ND + (2, 3)
    if name == 'cube_planes':
        assert tuple(rx.shape) == (1, 5, 1, 1, 2)
    if name == 'gamma_split':
        assert rx.device.type == 'cpu' and rx.dtype == torch.float64
    if name == 'views':
        assert not place(rx).is_contiguous()
    if name == 'offset':
        assert place(rx).is_contiguous() and place(rx).data_ptr() % 16 != 0


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('nC', (0, 1))
@pytest.mark.parametrize('name,nT', [(n, 48) for n in VARIANTS] + [(n, 53) for n in cases.FUSED_NT53])
def test_signal_operand_spellings(tag, mode, nC, name, nT):
    r"""One problem, many spellings (module docstring) through K2s and the signal mode of K2b; nT = 48: three checkpoint
    segments, nT = 53: the fused part plus five composed steps."""
    given, dense = cases.fused_operand_variants(DT[tag], nC, nT)[name]
    key = f'c{nC}.nT{nT}.{name}'
    _forms_arrive(name, given)
    with mrphy_amd.precision(mode):
        Mo_ref = _run('fused', given)['out']
        for every in EVERYS:
            _invariants(given, tag, mode, every, key, Mo_ref, dense, rx_on_cpu=name == 'gamma_split')


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
def test_signal_parallel_transmit_is_the_composed_route(tag, mode):
    r"""nC = 4, three receive coils on the ``*Nd`` grid: outside the signal kernels' coverage -- ``sig`` and ``Mo`` are the
    composed route's bits, the gradients within the gates of it, of the two-kernel route and of the oracle."""
    given, dense = cases.fused_operand_variants(DT[tag], 4, 48)['cube']
    with mrphy_amd.precision(mode):
        Mo_ref = _run('fused', given)['out']
        _invariants(given, tag, mode, 5, 'c4.nT48.cube', Mo_ref, dense, composed=True)


def _zero_rx(dtype, seed=37):
    r"""A dense receive map `(N, nM, 2)` whose weights on the two ``cases.ZERO_SPINS`` are of magnitude >= 0.5."""
    gen = torch.Generator(device='cpu').manual_seed(seed)
    rx = torch.rand((cases.FUSED_N, cases.FUSED_NM, 2), generator=gen, dtype=torch.float64) * 2 - 1
    for n, s in cases.ZERO_SPINS:
        rx[n, s] = torch.tensor([0.5 + 0.25 * n, -0.75])
    return rx.to(dtype)


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('nC', (0, 1))
@pytest.mark.parametrize('nT', [48, 53])
def test_signal_zero_field_steps(tag, mode, nC, nT):
    r"""Dead time and spins at the iso-centre through the signal mode of K2b, which injects a sample's cotangent on those
    very steps: ``every`` 1 and 5 put records on zero-field steps, 16 on the ends of the segments (batch entry 1's
    all-zero one included); nT = 53 through the split route.  The yardstick is the explicit adjoint, as in
    ``test_fused_operands.py::test_zero_field_steps``; the pulse gradients are held to the gates on the zero-field steps
    alone, and on batch entry 1's all-zero segment alone, where the yardstick is O(1) (asserted: > 0.1)."""
    v, zero = cases.zero_field_case(DT[tag], nC, nT)
    v['rx'] = _zero_rx(DT[tag])
    assert all(float(v['rx'][n, s].abs().min()) >= 0.5 for n, s in cases.ZERO_SPINS)
    key = f'c{nC}.nT{nT}.zero_field'
    with mrphy_amd.precision(mode):
        Mo_ref = _run('fused', v)['out']
        for every in EVERYS:
            _invariants(v, tag, mode, every, key, Mo_ref, zero=zero)
