r"""More spin tiles than persistent waves, in every mode of the fused adjoint.  K2b launches ``min(tiles, cap)`` waves; a
wave that takes tiles ``w, w + P, ...`` re-initialises its record cursor for each and adds a later tile's row sums into
its workspace row ``(w N + n)`` by read-modify-write.  Here N = 2, nT = 32 (two checkpoint segments) and
``nM = P 64 + 100`` with ``P`` read from the workspace query: waves 0 and 1 take a second tile, wave 1's is ragged (36
valid lanes), and batch entry 1 addresses a row with ``w > 0`` on a later tile.

Entry points: ``blochsim_rfgr`` (``INJ == 0``), ``blochsim_rfgr_traj`` at ``every`` 1, 5 (``INJ == 1``) and 16
(``INJ == 2``), ``signal_rfgr`` with ``rx`` and ``return_Mo`` at ``every`` 1, 5, 16 (``INJ == 3``); the operands of
``test_fused_traj._problem``, 'plain' and 'b1map', fp64 and fp32, fp32 also in ``precision('fast')`` (bit checks only; its
distances go to the ledger unasserted).

Two losses each.  FULL weights: the read-modify-write -- a dropped, doubled or unmasked tile moves ``grad_rf`` /
``grad_gr`` by about ``sqrt(36 / nM)`` = 1.5e-2 relative.  TAIL-ONLY weights: the cotangent (for the signal, ``rx`` too) is
zero on every spin of the tiles ``< P``, so the pulse gradients must equal, to the gate, the oracle's on the last 136
spins alone (36 of them before tile ``P``, with a zero cotangent: they add exact zeros) -- a wrong value on a second
tile is not diluted by 131 072 right ones.  Oracle-side dry run of that comparison on the CPU, one tile's spins left out
of the sum (the oracle's tail gradients without the 36 spins of the ragged tile, or without the 64 of tile ``P``, against
those of all 100): ``grad_rf`` and ``grad_gr`` move by 0.35 .. 1.14 in relative L2 over the entry points, strides and
variants -- 3.5e4 .. 1.1e5 times the fp32 gate -- and by 0.46 .. 16.6 in max abs, more than 4e8 times the fp64 gate.

The yardstick is the CPU oracle run in fp64 on the operands as given (fp32 operands widened), never the composed route
``_traj_by_segments``, which runs plain K2b itself.  The oracle's own fp32 run of these problems is 4e-7 .. 9e-7 (relative
L2) from its fp64 run for ``sig``, ``Mo`` and the three gradients at every stride: the 1e-5 gate leaves the kernels more
than 10x that.  ``Mo``, ``Mt`` and ``sig`` are held bit for bit to what the small-problem tests pin them to: prefix runs
of ``blochsim_rfgr``, and S64 (``test_signal._sig64``) with its elementwise bound."""
import functools

import pytest

from gpu_common import *  # noqa: F401,F403
from mrphy_amd import _host
from mrphy_amd.fused import _signal_of, _traj_ends
from test_fused_traj import _problem, _kw, _oracle_traj
from test_signal import _rx, _sig64
from util import ATOL64, REL32

pytestmark = pytest.mark.gpu

N, NT, WAVE = 2, 32, 64
ENTRIES = [('Mo', None), ('traj', 1), ('traj', 5), ('traj', 16), ('sig', 1), ('sig', 5), ('sig', 16)]
MODES = [('f64', 'precise'), ('f32', 'precise'), ('f32', 'fast')]


def _adjoint_waves(tag, nM):
    r"""The adjoint's wave count for ``nM`` spins, from the workspace query (``(P N 5 nT)`` elements)."""
    lib = mrphy_amd.require_library()
    code = _host.dtype_code(DT[tag], DT[tag])
    return int(lib.mrphy_blochsim_rfgr_bwd_workspace(code, N, nM, NT)) // (N * 5 * NT * DT[tag].itemsize)


def _signal_waves(tag, nM, every):
    r"""The signal forward's wave count, from its workspace query (``(P N 2 nRec)`` elements)."""
    lib = mrphy_amd.require_library()
    code = _host.dtype_code(DT[tag], DT[tag])
    nRec = len(_traj_ends(NT, every))
    return int(lib.mrphy_signal_rfgr_fwd_workspace(code, N, nM, NT, every)) // (N * 2 * nRec * DT[tag].itemsize)


@functools.lru_cache(maxsize=None)
def _shape(tag):
    r"""``(P, nM)``: the cap on the adjoint's waves (the count for far more tiles than any cap) and nM = P 64 + 100."""
    P = _adjoint_waves(tag, 1 << 30)
    nM = P * WAVE + 100
    assert _adjoint_waves(tag, nM) == P and -(-nM // WAVE) == P + 2 > P, (P, nM)   # two waves take a second tile
    return P, nM


@functools.lru_cache(maxsize=None)
def _setup(tag, variant):
    r"""The problem (CPU, the data dtype), its receive map and the same numbers in fp64."""
    P, nM = _shape(tag)
    Q = _problem(tag, variant, NT, N=N, nM=nM)
    rx = _rx(tag, 'coil', nM=nM, n=N)
    Q64 = {k: (None if x is None else x.double()) for k, x in Q.items()}
    return Q, rx, Q64, rx.double()


@functools.lru_cache(maxsize=4)
def _wave(n, phase):
    return torch.sin(torch.arange(n, dtype=torch.float64) * 0.61 + phase)


def _weights(tag, entry, every, loss):
    r"""``(w_out, w_sig, rx_mask)`` in fp64: the cotangent of ``Mo`` / ``Mt``, of ``sig`` (``None`` unless the signal), and
    the factor on ``rx`` -- for the tail-only loss the first two (``w_sig`` aside) and ``rx`` are zero on the spins of
    the tiles ``< P``."""
    P, nM = _shape(tag)
    nRec = len(_traj_ends(NT, every)) if every else 1
    shape = (N, nM, nRec, 3) if entry == 'traj' else (N, nM, 3)
    w = _wave(N * nM * nRec * 3 if entry == 'traj' else N * nM * 3, 1.0).reshape(shape)
    mask = torch.ones(nM, dtype=torch.float64)
    if loss == 'tail':
        mask[:P * WAVE] = 0
    w = w * mask.reshape((1, nM) + (1,) * (w.ndim - 2))
    ws = _wave(N * 2 * nRec, 0.3).reshape(N, 2, nRec) if entry == 'sig' else None
    rounded = lambda x: None if x is None else x.to(DT[tag]).double()      # noqa: E731  (the numbers the kernels get)
    return rounded(w), rounded(ws), mask


def _oracle_run(Q64, rx64, entry, every, w, ws, spins):
    r"""``out, [sig,] grad_Mi, grad_rf, grad_gr`` of the loss by the CPU oracle in fp64 on the spins ``spins`` (a slice)."""
    R = {k: (x[:, spins] if k in ('M0', 'loc', 'df', 'b1', 'T1', 'T2') and x is not None else x) for k, x in Q64.items()}
    Mi, r, g = (R[k].clone().requires_grad_(True) for k in ('M0', 'rf', 'gr'))
    ends = [NT] if entry == 'Mo' else _traj_ends(NT, every)
    Mt = _oracle_traj(Mi, r, g, R, ends)                                   # (N, nM, nRec, 3)
    got = {}
    if entry == 'sig':
        got['sig'] = _signal_of(Mt.movedim(-2, 0), rx64[:, spins])
        out = Mt[..., -1, :]
        loss = (got['sig'] * ws).sum() + (out * w[:, spins]).sum()
    else:
        out = Mt if entry == 'traj' else Mt[..., -1, :]
        loss = (out * w[:, spins]).sum()
    loss.backward()
    got.update(out=out, grad_Mi=Mi.grad, grad_rf=r.grad, grad_gr=g.grad)
    return {k: x.detach() for k, x in got.items()}


@functools.lru_cache(maxsize=4)
def _oracle(tag, variant, entry, every, loss):
    r"""The yardstick of one case, once: the whole problem for the full loss; for the tail-only loss the last 136 spins
    alone."""
    _, _, Q64, rx64 = _setup(tag, variant)
    P, nM = _shape(tag)
    w, ws, mask = _weights(tag, entry, every, loss)
    with mrphy_amd.constants_on('cpu'):
        if loss == 'full':
            return _oracle_run(Q64, rx64, entry, every, w, ws, slice(None))
        return _oracle_run(Q64, rx64 * mask[None, :, None], entry, every, w, ws, slice(nM - 136, nM))


def _gpu_run(Q, rx, entry, every, w, ws, mask):
    dtype = Q['M0'].dtype
    Mi, r, g = (dev(Q[k]).clone().requires_grad_(True) for k in ('M0', 'rf', 'gr'))
    kw, loc = _kw(Q, dev), dev(Q['loc'])
    got = {}
    if entry == 'sig':
        rxd = dev((rx.double() * mask[None, :, None]).to(dtype))
        got['sig'], out = fused.signal_rfgr(Mi, r, g, loc, every=every, rx=rxd, return_Mo=True, **kw)
        loss = (got['sig'] * dev(ws.to(dtype))).sum() + (out * dev(w.to(dtype))).sum()
    else:
        out = (fused.blochsim_rfgr_traj(Mi, r, g, loc, every=every, **kw) if entry == 'traj' else
               fused.blochsim_rfgr(Mi, r, g, loc, **kw))
        loss = (out * dev(w.to(dtype))).sum()
    loss.backward()
    got.update(out=out, grad_Mi=Mi.grad, grad_rf=r.grad, grad_gr=g.grad)
    return {k: x.detach() for k, x in got.items()}


def _over_gate(a, b, tag):
    assert a.shape == b.shape, (a.shape, b.shape)
    return max_abs(a, b) / ATOL64 if tag == 'f64' else rel_l2(a, b) / REL32


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('variant', ['plain', 'b1map'])
@pytest.mark.parametrize('entry,every', ENTRIES)
def test_adjoint_wave_takes_a_second_tile(tag, mode, variant, entry, every):
    r"""Module docstring: N = 2, nM = P 64 + 100, nT = 32; the full and the tail-only loss through one entry point."""
    P, nM = _shape(tag)
    t0 = P * WAVE                                                  # the first spin of the tiles >= P
    Q, rx, _, _ = _setup(tag, variant)
    led = f'tiles.{tag}.{mode}.{variant}.{entry}' + (f'.every{every}' if every else '')
    args = (dev(Q['M0']), dev(Q['rf']), dev(Q['gr']), dev(Q['loc']))
    ends = [NT] if entry == 'Mo' else _traj_ends(NT, every)
    with mrphy_amd.precision(mode):
        kw = _kw(Q, dev)
        with torch.no_grad():                                      # what the small-problem tests pin the outputs to
            pre = torch.stack([fused.blochsim_rfgr(args[0], args[1][:, :, :e], args[2][:, :, :e], args[3], **kw)
                               for e in ends], dim=-2)
            Mt = fused.blochsim_rfgr_traj(*args, every=every, **kw) if entry == 'sig' else None
        for loss in ('full', 'tail'):
            w, ws, mask = _weights(tag, entry, every, loss)
            fu = _gpu_run(Q, rx, entry, every, w, ws, mask)
            for k, x in fu.items():
                assert bool(torch.isfinite(x).all()), (loss, k)
            # the outputs, bit for bit
            if entry == 'traj':
                assert max_abs(fu['out'], pre) == 0.0, (loss, 'Mt vs prefix runs')
            else:
                assert max_abs(fu['out'], pre[..., -1, :]) == 0.0, (loss, 'Mo vs blochsim_rfgr')
            if entry == 'sig':
                assert max_abs(Mt, pre) == 0.0, 'the trajectory S64 is formed of vs prefix runs'
                S64, A64 = _sig64(Mt, rx.double() * mask[None, :, None])
                d = record(f'{led}.{loss}.sig_vs_S64.over_gate', _over_gate(fu['sig'], S64, tag), 1.0)
                assert d <= 1.0, (loss, 'sig vs S64', d)
                if tag == 'f32':
                    ratio = float(((fu['sig'].double().cpu() - S64).abs() / ((nM + 3) * 2.0 ** -24 * A64)).max())
                    record(f'{led}.{loss}.sig.elementwise_over_bound', ratio, 1.0)
                    assert ratio <= 1.0, (loss, ratio)
            # the yardstick
            ora = _oracle(tag, variant, entry, every, loss)
            if loss == 'full':
                pairs = {k: (fu[k], ora[k]) for k in fu}
                pairs['grad_Mi on the tiles >= P'] = (fu['grad_Mi'][:, t0:], ora['grad_Mi'][:, t0:])
            else:
                full_gMi = torch.zeros(fu['grad_Mi'].shape, dtype=torch.float64)
                full_gMi[:, t0:] = ora['grad_Mi'][:, 36:]
                assert float(ora['grad_Mi'][:, :36].abs().max()) == 0.0
                pairs = {'grad_rf': (fu['grad_rf'], ora['grad_rf']), 'grad_gr': (fu['grad_gr'], ora['grad_gr']),
                         'grad_Mi': (fu['grad_Mi'], full_gMi),
                         'grad_Mi on the tiles >= P': (fu['grad_Mi'][:, t0:], ora['grad_Mi'][:, 36:]),
                         'out on the tiles >= P': (fu['out'][:, t0:], ora['out'][:, 36:])}
                if entry == 'sig':
                    pairs['sig'] = (fu['sig'], ora['sig'])
            dist = {k: _over_gate(a, b, tag) for k, (a, b) in pairs.items()}
            if mode == 'precise':
                record(f'{led}.{loss}.vs_oracle.over_gate', max(dist.values()), 1.0,
                       note=', '.join(f'{k} {x:.3f}' for k, x in dist.items()))
                for k, x in dist.items():
                    assert x <= 1.0, f'{led}.{loss}: {k} is {x:.3e} of the gate from the oracle'
            else:
                record(f'{led}.{loss}.vs_oracle.over_precise_gate', max(dist.values()),
                       note='not asserted: ' + ', '.join(f'{k} {x:.3f}' for k, x in dist.items()))
            again = _gpu_run(Q, rx, entry, every, w, ws, mask)
            for k in fu:
                assert max_abs(fu[k], again[k]) == 0.0, (loss, k, 'second run')


@pytest.mark.parametrize('every', [1, 16])
def test_signal_forward_second_tile_two_batch_entries(every):
    r"""``test_signal.py::test_signal_second_tile_per_wave`` with a second batch entry: N = 2, nM = P_s 64 + 100 with
    ``P_s`` the signal forward's cap on its waves (from its workspace query), nT = 32, fp32, with rx -- a wave adds its
    second tile into the workspace row ``(w N + n)``.  Relative L2 <= 1e-5 against S64, as there; twice the same bits."""
    tag = 'f32'
    Ps = _signal_waves(tag, 1 << 30, every)
    nM = Ps * WAVE + 100
    assert _signal_waves(tag, nM, every) == Ps and -(-nM // WAVE) > Ps, (Ps, nM)
    Q = _problem(tag, 'plain', NT, N=N, nM=nM)
    rx = _rx(tag, 'coil', nM=nM, n=N)
    kw = _kw(Q, dev)
    args = (dev(Q['M0']), dev(Q['rf']), dev(Q['gr']), dev(Q['loc']))
    with torch.no_grad():
        sig = fused.signal_rfgr(*args, every=every, rx=dev(rx), **kw)
        again = fused.signal_rfgr(*args, every=every, rx=dev(rx), **kw)
        S64, _ = _sig64(fused.blochsim_rfgr_traj(*args, every=every, **kw), rx)
    assert sig.shape == (N, 2, NT // every)
    d = record(f'tiles.signal_fwd.N2.every{every}.vs_S64', rel_l2(sig, S64), 1e-5)
    assert d <= 1e-5, d
    assert torch.equal(sig, again)
