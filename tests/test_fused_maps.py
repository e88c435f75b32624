r"""The MAPS builds of K2b / K2bt (``mrphy_blochsim_rfgr_maps_bwd``): gradients of ``fused.blochsim_rfgr`` and
``fused.blochsim_rfgr_traj`` w.r.t. the spin-side operands ``loc``, ``Δf`` and ``b1Map`` of one transmit coil through the
fused adjoint -- against the two-kernel route (``rfgr2beff`` + ``blochsim`` on the GPU, which writes ``Beff`` and
``grad_Beff``), the per-segment composition and the CPU oracle's autograd; the pulse gradients' bits; operand forms;
dtype codes; more tiles than persistent waves; the route taken and the memory it needs; fallbacks; empty problems.

Gates (``util.assert_close``): fp64 max-abs 1e-9, fp32 relative L2 1e-5 -- what ``test_signal_fallbacks`` and
``test_traj_fallback_matches_oracle`` hold the composed route's map gradients to on these shapes."""
import collections
import functools

import pytest

from gpu_common import *  # noqa: F401,F403
from mrphy_amd import _lib as L
from mrphy_amd.fused import _traj_by_segments, _traj_ends
from test_fused_traj import _problem, _kw, _oracle_traj, _weights

pytestmark = pytest.mark.gpu

N, NM = 2, 100
ALL = ('M0', 'rf', 'gr', 'loc', 'df', 'b1')
NAMES = {'M0': 'grad_Mi', 'rf': 'grad_rf', 'gr': 'grad_gr', 'loc': 'grad_loc', 'df': 'grad_Δf', 'b1': 'grad_b1Map'}
MAPS_BWD = 'mrphy_blochsim_rfgr_maps_bwd'


def _run(kind, P, on, every=None, needs=ALL):
    r"""``{'out': M, 'M0': grad_Mi, 'rf': .., 'gr': .., 'loc': .., 'df': .., 'b1': ..}`` (``None`` where no gradient was
    asked for or the operand is absent) of the loss ``(M·w).sum()``; ``M`` is ``Mo`` (``every = None``) or the trajectory
    `(N, *Nd, nRec, 3)`.  kind: 'fused' -- the functions under test; 'two' -- rfgr2beff + blochsim, per record segment
    over slices of one ``Beff``; 'segments' -- ``_traj_by_segments``; 'oracle' -- the CPU oracle."""
    Q = {k: (None if P[k] is None else on(P[k]).clone().requires_grad_(k in needs)) for k in ALL}
    Q.update({k: (None if P[k] is None else on(P[k])) for k in ('T1', 'T2', 'γ', 'dt')})
    kw = _kw(Q, lambda x: x)
    nT = P['gr'].shape[2]
    ends = [nT] if every is None else _traj_ends(nT, every)
    if kind == 'oracle':
        Mt = _oracle_traj(Q['M0'], Q['rf'], Q['gr'], Q, ends)
    elif kind == 'two':
        beff = beffective.rfgr2beff(Q['rf'], Q['gr'], Q['loc'], Δf=Q['df'], b1Map=Q['b1'], γ=Q['γ'])
        out, M, t0 = [], Q['M0'], 0
        for e in ends:
            M = sims.blochsim(M, beff[..., t0:e, :], T1=Q['T1'], T2=Q['T2'], γ=Q['γ'], dt=Q['dt'])
            out.append(M)
            t0 = e
        Mt = torch.stack(out, dim=-2)
    elif kind == 'segments':
        Mt = _traj_by_segments(Q['M0'], Q['rf'], Q['gr'], Q['loc'], ends, kw).movedim(0, -2)
    elif every is None:
        Mt = fused.blochsim_rfgr(Q['M0'], Q['rf'], Q['gr'], Q['loc'], **kw)
    else:
        Mt = fused.blochsim_rfgr_traj(Q['M0'], Q['rf'], Q['gr'], Q['loc'], every=every, **kw)
    if every is None and kind != 'fused':
        Mt = Mt[..., 0, :]
    (Mt * on(_weights(tuple(Mt.shape), Mt.dtype))).sum().backward()
    res = {k: (None if Q[k] is None else Q[k].grad) for k in ALL}
    res['out'] = Mt.detach()
    return res


def _compare(got, want, tag, what, keys=ALL):
    for k in ('out',) + tuple(keys):
        a, b = got[k], want[k]
        assert (a is None) == (b is None), (what, k)
        if a is not None:
            assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape)
            assert_close(a, b, tag, f'{NAMES.get(k, k)} vs {what}')


def _same_bits(got, want, keys, what):
    for k in keys:
        if want[k] is not None:
            assert got[k] is not None and torch.equal(got[k], want[k]), (what, k)


@functools.lru_cache(maxsize=None)
def _oracle(tag, variant, nT, every, seed=23):
    with mrphy_amd.constants_on('cpu'):
        return _run('oracle', _problem(tag, variant, nT, seed=seed), lambda x: x, every)


# =============================================================================================
# 1. values and gradients, blochsim_rfgr
# =============================================================================================
@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('variant', ['b1map', 'plain', 'norelax', 'plain_batch1_pulse'])
@pytest.mark.parametrize('nT', [16, 48, 50])
def test_maps_gradients(tag, variant, nT):
    r"""Loss (Mo·w).sum() with Mi, rf, gr, loc, Δf, b1Map all requiring gradients: ``Mo`` is the bits of the call without
    map gradients; all six gradients == the two-kernel route == the oracle; with whole segments grad_Mi, grad_rf,
    grad_gr are the BITS of the call that asks for them alone (the plain K2b); twice the same bits; each map alone leaves
    the others' ``.grad`` at None and gives the same bits.  nT = 16: one segment; 48: three; 50: fused part + composed
    tail, autograd adds the parts' map gradients."""
    P = _problem(tag, variant, nT)
    got = _run('fused', P, dev)
    pulse = _run('fused', P, dev, needs=('M0', 'rf', 'gr'))
    assert torch.equal(got['out'], pulse['out']), 'Mo changed with the map gradients'
    assert (got['b1'] is None) == (variant != 'b1map') and got['loc'] is not None and got['df'] is not None
    assert all(pulse[k] is None for k in ('loc', 'df', 'b1'))
    _compare(got, _run('two', P, dev), tag, 'two-kernel route')
    _compare(got, _oracle(tag, variant, nT, None), tag, 'oracle')
    if nT % 16 == 0:
        _same_bits(got, pulse, ('M0', 'rf', 'gr'), 'pulse gradients with and without map gradients')
    _same_bits(_run('fused', P, dev), got, ALL, 'twice')
    for k in ('loc', 'df', 'b1'):
        if P[k] is None:
            continue
        one = _run('fused', P, dev, needs=(k,))
        assert all(one[j] is None for j in ALL if j != k), k
        assert one[k].shape == P[k].shape and one[k].dtype == P[k].dtype
        if nT % 16 == 0:
            assert torch.equal(one[k], got[k]), k
        else:
            assert_close(one[k], got[k], tag, f'{NAMES[k]} alone')


# =============================================================================================
# 2. trajectory
# =============================================================================================
@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('variant', ['b1map', 'plain'])
@pytest.mark.parametrize('nT,every', [(48, 1), (48, 3), (48, 16), (48, 40), (48, 48), (50, 3), (50, 16)])
def test_maps_trajectory_gradients(tag, variant, nT, every):
    r"""Loss (Mt·w).sum(): every < 16 is mode 1 (a record per step at every = 1, on and off the segment boundary at 3),
    every >= 16 mode 2 (on the boundary, off it, one record), nT = 50 the split.  ``Mt`` is the bits of the call
    without map gradients; all gradients == ``_traj_by_segments`` == the two-kernel route == the oracle."""
    P = _problem(tag, variant, nT)
    got = _run('fused', P, dev, every)
    pulse = _run('fused', P, dev, every, needs=('M0', 'rf', 'gr'))
    assert got['out'].shape == (N, NM, len(_traj_ends(nT, every)), 3)
    assert torch.equal(got['out'], pulse['out']), 'Mt changed with the map gradients'
    if nT % 16 == 0:
        _same_bits(got, pulse, ('M0', 'rf', 'gr'), 'pulse gradients with and without map gradients')
    _compare(got, _run('segments', P, dev, every), tag, f'segment loop (every={every})')
    _compare(got, _run('two', P, dev, every), tag, f'two-kernel route (every={every})')
    _compare(got, _oracle(tag, variant, nT, every), tag, f'oracle (every={every})')
    _same_bits(_run('fused', P, dev, every), got, ALL, 'twice')


# =============================================================================================
# 3. operand forms
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('df_form', ['full', 'batch1', 'per_batch'])
@pytest.mark.parametrize('b1_form', ['xy', 'coil1', 'batch1'])
def test_maps_operand_forms(tag, df_form, b1_form):
    r"""``Nd = (5, 5, 4)``; ``Δf`` as `(N, *Nd)`, `(1, *Nd)`, `(N, 1)`; ``b1Map`` as `(N, *Nd, xy)`, `(N, *Nd, xy, 1)`,
    `(1, *Nd, xy)`: each gradient has its operand's own shape and dtype and matches the two-kernel route, for ``Mo``
    and for a trajectory in each mode."""
    Nd = (5, 5, 4)
    P = _problem(tag, 'b1map', 48, seed=31)
    for k, tail in (('M0', (3,)), ('loc', (3,)), ('df', ()), ('b1', (2,)), ('T1', ()), ('T2', ())):
        P[k] = P[k].reshape((N,) + Nd + tail)
    P['df'] = {'full': P['df'], 'batch1': P['df'][:1], 'per_batch': P['df'][:, 0, 0, :1].reshape(N, 1)}[df_form]
    P['b1'] = {'xy': P['b1'], 'coil1': P['b1'][..., None], 'batch1': P['b1'][:1]}[b1_form]
    for every in (None, 5, 16):
        got = _run('fused', P, dev, every)
        for k in ALL:
            assert got[k].shape == P[k].shape and got[k].dtype == P[k].dtype, (k, every)
        _compare(got, _run('two', P, dev, every), tag, f'two-kernel route (every={every})')


# =============================================================================================
# 4. dtype codes
# =============================================================================================
@pytest.mark.parametrize('mode,wide', [('fast', False), ('fast', True), ('precise', False), ('precise', True)])
@pytest.mark.parametrize('every', [5, 16])
def test_maps_gradients_dtype_codes(mode, wide, every):
    r"""fp32 data through dtype codes 0 / 2 (fast; fp32 / fp64 constants) and 3 / 4 (precise: the sweep carries t = E h),
    with relaxation and a b1 map, against the two-kernel route in the same mode; code 3 also against the oracle."""
    from mrphy_amd import _host
    P = _problem('f32', 'b1map', 48, seed=5)
    if wide:
        P['T1'], P['T2'], P['γ'], P['dt'] = (P[k].double() for k in ('T1', 'T2', 'γ', 'dt'))
    with mrphy_amd.precision(mode):
        code = _host.dtype_code(torch.float32, torch.float64 if wide else torch.float32)
        assert code == {('fast', False): 0, ('fast', True): 2, ('precise', False): 3, ('precise', True): 4}[mode, wide]
        if code == 3:
            with mrphy_amd.constants_on('cpu'):
                got = _run('fused', P, dev, every)
                _compare(got, _run('two', P, dev, every), 'f32', f'two-kernel route (code 3, every={every})')
                _compare(got, _oracle('f32', 'b1map', 48, every, seed=5), 'f32', f'oracle (code 3, every={every})')
        else:
            got = _run('fused', P, dev, every)
            _compare(got, _run('two', P, dev, every), 'f32', f'two-kernel route (code {code}, every={every})')
        for k in ALL:
            assert got[k].dtype == torch.float32 and got[k].shape == P[k].shape


# =============================================================================================
# 5. more tiles than persistent waves
# =============================================================================================
def test_maps_second_tile_per_wave():
    r"""N = 1, nM = 2048·64 + 100, nT = 32, fp32, b1 map: more spin tiles than K2b has persistent waves (2048), so wave 0
    takes tile 0 and then the last, ragged one -- the running sums are reset and the outputs written per tile.  All map
    gradients against the two-kernel route, relative L2 <= 1e-5, over all spins and separately over the first tile and
    the last: a tile that inherited another's sums is off at order 1."""
    nM, nT = 2048 * 64 + 100, 32
    P = _problem('f32', 'b1map', nT, N=1, nM=nM)
    got = _run('fused', P, dev, needs=('loc', 'df', 'b1'))
    two = _run('two', P, dev, needs=('loc', 'df', 'b1'))
    for k in ('loc', 'df', 'b1'):
        for name, sl in (('all', slice(None)), ('first_tile', slice(0, 64)), ('last_tile', slice(2048 * 64, nM))):
            d = record(f'fused_maps.tiles2048.{k}.{name}.vs_two_kernel', rel_l2(got[k][:, sl], two[k][:, sl]), 1e-5)
            assert d <= 1e-5, (k, name, d)
    again = _run('fused', P, dev, needs=('loc', 'df', 'b1'))
    _same_bits(again, got, ('loc', 'df', 'b1'), 'twice')


# =============================================================================================
# 6. the route taken and what it needs
# =============================================================================================
OLD_BWD = ('mrphy_blochsim_rfgr_bwd', 'mrphy_blochsim_rfgr_traj_bwd')
COMPOSED = tuple(n for n in L.PROTOTYPES if n.startswith(('mrphy_rfgr2beff', 'mrphy_blochsim_fwd'))
                 and not n.endswith('workspace'))


def _counted(monkeypatch):
    lib = mrphy_amd.require_library()
    calls = collections.Counter()

    def wrap(name, fn):
        def counted(*a):
            calls[name] += 1
            return fn(*a)
        return counted
    for name in (MAPS_BWD,) + OLD_BWD + COMPOSED:
        monkeypatch.setattr(lib, name, wrap(name, getattr(lib, name)))
    return calls


def test_maps_gradient_is_one_fused_launch(monkeypatch):
    r"""nT = 48 with ``Δf`` requiring a gradient: ``blochsim_rfgr`` and ``blochsim_rfgr_traj(every = 5)`` each call
    ``mrphy_blochsim_rfgr_maps_bwd`` exactly once and neither K0 nor the blochsim forward; with only ``rf`` requiring a
    gradient they call the entry points they called before and not the new one."""
    P = _problem('f32', 'b1map', 48)
    assert len(COMPOSED) >= 4
    calls = _counted(monkeypatch)
    for every, old in ((None, OLD_BWD[0]), (5, OLD_BWD[1])):
        calls.clear()
        _run('fused', P, dev, every, needs=('df',))
        assert calls[MAPS_BWD] == 1 and not any(calls[n] for n in OLD_BWD + COMPOSED), (every, dict(calls))
        calls.clear()
        _run('fused', P, dev, every, needs=('rf',))
        assert calls[old] == 1 and sum(calls.values()) == 1, (every, dict(calls))


def test_maps_gradients_materialise_no_beff():
    r"""N = 1, nM = 4096, nT = 256, fp32, ``loc``, ``Δf``, ``b1Map`` and ``rf`` requiring gradients, forward + backward:
    the allocator's peak rises by less than a quarter of ``Beff``'s bytes (nM·nT·12) -- the checkpoints are 1/16 of
    them, the workspace and the per-spin outputs smaller still; the two-kernel route holds Beff, the history and
    grad_Beff, more than twice all of them."""
    nM, nT = 4096, 256
    P = _problem('f32', 'b1map', nT, N=1, nM=nM)
    kw = _kw(P, dev)
    Mi = dev(P['M0'])
    rf, gr = dev(P['rf']).requires_grad_(True), dev(P['gr'])
    loc = dev(P['loc']).requires_grad_(True)
    kw['Δf'], kw['b1Map'] = kw['Δf'].requires_grad_(True), kw['b1Map'].requires_grad_(True)
    beff_bytes = nM * nT * 12
    leaves = (rf, loc, kw['Δf'], kw['b1Map'])

    def rise(fn):
        for x in leaves:
            x.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn().sum().backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, [x.grad.clone() for x in leaves]

    def two():
        b = beffective.rfgr2beff(rf, gr, loc, Δf=kw['Δf'], b1Map=kw['b1Map'], γ=kw['γ_beff'])
        return sims.blochsim(Mi, b, T1=kw['T1'], T2=kw['T2'], γ=kw['γ'], dt=kw['dt'])
    fused_rise, g = rise(lambda: fused.blochsim_rfgr(Mi, rf, gr, loc, **kw))
    two_rise, g2 = rise(two)
    record('fused_maps.mem.rise_over_beff', fused_rise / beff_bytes, 0.25,
           note=f'fused {fused_rise} B, two-kernel route {two_rise} B, Beff {beff_bytes} B')
    assert fused_rise < 0.25 * beff_bytes, (fused_rise, beff_bytes)
    assert two_rise > 2 * beff_bytes, (two_rise, beff_bytes)
    for a, b, nm in zip(g, g2, ('grad_rf', 'grad_loc', 'grad_Δf', 'grad_b1Map')):
        assert_close(a, b, 'f32', nm)


# =============================================================================================
# 7. fallbacks unchanged
# =============================================================================================
@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('case', ['ptx4_b1', 'nT8_df'])
def test_maps_fallbacks_stay_composed(case, monkeypatch):
    r"""A 4-coil parallel-transmit ``b1Map`` gradient and a ``Δf`` gradient at nT = 8 (no whole segment) go through the
    composed route as before: the new entry point is not called, and values and gradients match the oracle."""
    tag = 'f32'
    variant, nT, needs = ('ptx4', 48, ('M0', 'rf', 'gr', 'b1')) if case == 'ptx4_b1' else ('b1map', 8, ('M0', 'rf', 'gr', 'df'))
    P = _problem(tag, variant, nT, seed=77)
    calls = _counted(monkeypatch)
    for every in (None, 5):
        calls.clear()
        got = _run('fused', P, dev, every, needs=needs)
        assert calls[MAPS_BWD] == 0 and calls['mrphy_rfgr2beff_st'] >= 1, (case, dict(calls))
        _compare(got, _run('oracle', P, lambda x: x, every, needs=needs), tag, f'oracle ({case}, every={every})')


# =============================================================================================
# 8. empty problems
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('empty', ['nT', 'nM'])
def test_maps_empty_problem(tag, empty):
    r"""No step (nT = 0) or no spin (nM = 0) with map gradients wanted: the backward runs and the gradients are zeros of
    the operands' shapes and dtypes (``grad_Mi`` the cotangent of ``Mo``; zero for a trajectory without a record)."""
    nT, nM, every = (0, 100, 3) if empty == 'nT' else (32, 0, 5)
    P = _problem(tag, 'b1map', 32, nM=nM)
    P['rf'], P['gr'] = P['rf'][:, :, :nT], P['gr'][:, :, :nT]
    for ev in (None, every):
        got = _run('fused', P, dev, ev)
        for k in ALL:
            assert got[k] is not None and got[k].shape == P[k].shape and got[k].dtype == P[k].dtype, (k, ev)
            if k != 'M0':
                assert bool((got[k] == 0).all()), (k, ev)
        w = dev(_weights(tuple(got['out'].shape), DT[tag]))
        assert torch.equal(got['M0'], w if ev is None else torch.zeros_like(got['M0'])), ev
