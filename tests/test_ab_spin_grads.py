r"""``fused.ab_rfgr``'s gradients w.r.t. ``loc, Δf, b1Map, γ_beff`` and ``T1, T2, γ, dt`` through K2abb's MAPS and CONSTS builds
(``mrphy_ab_rfgr_maps_bwd`` / ``mrphy_ab_rfgr_consts_bwd``), and ``fused.steadystate_rfgr`` on top of them.

Yardsticks.  (a) ``test_ab_spin_grads_host.oracle_ab_spin_grads``: the fp64 CPU column chain with every operand a leaf
(finite differences hold it: ``test_ab_spin_grads_host.py``); for fp32 data it integrates with the fp32 relaxation
factors the kernels are handed, differentiated as ``exp(-dt / T)`` (``straight_through_times``: the reason is
``test_ab_operands.py``'s -- ``B`` is proportional to ``E1 - 1``, whose fp32 form is off by up to 1.5 %).  (b) today's
composed route on the GPU (``rfgr2beff`` + ``beff2ab``, which writes ``Beff``, the columns' history and ``grad_Beff``):
``ab_rfgr`` with the fused builds switched off.  (c) the column identity ``A[..., j] = blochsim_rfgr(e_j) - B``, ``B =
blochsim_rfgr(0)``, differentiated through K2b's CONSTS build.

Gates: the project's.  A gradient with a spin axis (``loc, b1Map``, a per-spin ``Δf, γ_beff, T1, T2, γ``) and the pulse
gradients: ``util.assert_close`` -- fp64 max-abs 1e-9, fp32 relative L2 1e-5.  A gradient summed over the spins (a 0-dim or
per-batch ``Δf, T1, T2, γ, γ_beff, dt``) is an ill-conditioned sum, so, as ``test_fused_consts._gate_sum``: ``|got - want|
<= gate · Σ_s |g_s|`` per element, ``g_s`` the oracle's per-spin terms in fp64, gate 1e-9 / 1e-5.  (``dt`` is always such
a sum: ``dL/ddt`` is O(1e5), no absolute 1e-9 can be asked of it.)  fp32: where the chain (a) evaluated wholly in fp32 on
the CPU lies further than a third of 1e-5 from itself in fp64, the gate of that gradient on that case is three times that
distance (``test_ab_operands.py``'s margin); the distance is measured where the test runs and goes to the ledger
(``abspin.*.chain_f32_vs_f64``).  CPU dry run of that distance (relative L2; per-spin terms for the summed operands), the
six 2-D variants of ``cases.fused_operand_variants``, nC in {0, 1}, nT = 48, with relaxation: ``rf`` 5.2e-7 .. 1.2e-6,
``gr`` 4.3e-7 .. 1.3e-6, ``loc`` 5.8e-7 .. 9.7e-7, ``Δf`` 5.1e-7 .. 9.9e-7, ``b1Map`` 5.7e-7 .. 9.7e-7, ``γ_beff`` 5.2e-7
.. 1.0e-6, ``T1`` 4.8e-7 .. 1.1e-6, ``T2`` 5.4e-7 .. 1.2e-6, ``γ`` 6.2e-7 .. 1.0e-6, ``dt`` 6.2e-7 .. 1.0e-6; the
zero-field case 7.7e-7 .. 1.8e-6 (``gr``); 'gamma_split' at nT = 16, 50, 7 and without relaxation 2.0e-7 .. 1.3e-6 -- a
tenth of the gate, so the margin does not come into play on these cases.  ``precision('fast')`` gets the bit checks and
ledger entries only."""
import functools

import pytest

from gpu_common import *  # noqa: F401,F403
from mrphy_amd import _host
from test_ab_rfgr import _counted
from test_ab_rfgr_host import ab_weights
from test_ab_spin_grads_host import fold_like, oracle_ab_spin_grads
from test_fused_operands import _same_bits
from test_steadystate import _gate as _ss_gate
from test_steadystate_host import torch_steadystate

pytestmark = pytest.mark.gpu

MODES = [('f64', 'precise'), ('f32', 'precise'), ('f32', 'fast')]
LEAVES = ('rf', 'gr', 'loc', 'Δf', 'b1Map', 'γ_beff', 'T1', 'T2', 'γ', 'dt')
PER_SPIN = ('Δf', 'γ_beff', 'T1', 'T2', 'γ', 'dt')        # what the oracle returns per spin, folded to the operand's shape
TWO_D = ('compact_mixed', 'scalars', 'expanded', 'gamma_split', 'views', 'offset')
TOL = {'f64': 1e-9, 'f32': 1e-5}
FWD, BWD, MAPS_BWD, CONSTS_BWD = ('mrphy_ab_rfgr_fwd', 'mrphy_ab_rfgr_bwd', 'mrphy_ab_rfgr_maps_bwd',
                                  'mrphy_ab_rfgr_consts_bwd')
COMPOSED = ('mrphy_rfgr2beff_st', 'mrphy_beff2ab', 'mrphy_beff2ab_save', 'mrphy_beff2ab_bwd', 'mrphy_beff2ab_bwd_consts')


# ---------------------------------------------------------------------------------------------
# cases, oracle (once per case, never modified), runs
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(tag, name, nC, nT, relax=True):
    r"""The operands as given: a 2-D variant of the zoo, 'zero' (``cases.zero_field_case``) or 'gamma0' ('gamma_split'
    with the step constant ``γ = 0`` for the spins of ``ZERO_SPINS``)."""
    if name == 'zero':
        v = dict(cases.zero_field_case(DT[tag], nC, nT)[0])
    else:
        v = dict(cases.fused_operand_variants(DT[tag], nC, nT)['gamma_split' if name == 'gamma0' else name][0])
    if name == 'gamma0':
        v['γ'] = v['γ'].clone()
        for n, s in cases.ZERO_SPINS:
            v['γ'][n, s] = 0
    if not relax:
        v['T1'] = v['T2'] = None
    return v


def _factors(v, tag):
    r"""The fp32 ``E1, E2`` the kernels are handed (formed on the CPU: ``host_constants``), or ``None``."""
    if tag == 'f64' or v['T1'] is None:
        return None
    c = cases.reference_constants(v['T1'], v['T2'], v['γ'], v['dt'], 2)
    return c['E1'], c['E2']


@functools.lru_cache(maxsize=None)
def _oracle(tag, name, nC, nT, relax=True):
    r"""``(the yardstick (a), {operand: the chain's own fp32-vs-fp64 distance} or None)``."""
    v = _case(tag, name, nC, nT, relax)
    wide = oracle_ab_spin_grads(v, factors=_factors(v, tag))
    if tag == 'f64':
        return wide, None
    hi, lo = oracle_ab_spin_grads(v), oracle_ab_spin_grads(v, dtype=torch.float32)
    return wide, {k: rel_l2(lo[k], hi[k]) for k in hi}


def _run(route, v, wrt=LEAVES, monkeypatch=None):
    r"""``A, B`` and the gradients of the operands named in ``wrt`` for the cotangents ``ab_weights(v)``.  ``route``: 'fused'
    (``fused.ab_rfgr``), 'composed' (the same call with K2abb's MAPS / CONSTS builds switched off: today's route) or 'k2b'
    (the column identity through ``fused.blochsim_rfgr``).  The operands go in AS GIVEN (``place``), leaves that are
    detached aliases."""
    Q = {k: (None if v[k] is None else place(v[k]).detach().requires_grad_(k in wrt)) for k in LEAVES}
    kw = dict(Δf=Q['Δf'], b1Map=Q['b1Map'], γ_beff=Q['γ_beff'], T1=Q['T1'], T2=Q['T2'], γ=Q['γ'], dt=Q['dt'])
    if route == 'k2b':
        lead = tuple(v['loc'].shape[:-1])
        e = torch.eye(3, dtype=v['loc'].dtype, device=DEV)
        B = fused.blochsim_rfgr(torch.zeros(lead + (3,), dtype=v['loc'].dtype, device=DEV), Q['rf'], Q['gr'], Q['loc'], **kw)
        A = torch.stack([fused.blochsim_rfgr(e[j].expand(lead + (3,)).contiguous(), Q['rf'], Q['gr'], Q['loc'], **kw) - B
                         for j in range(3)], dim=-1)
    elif route == 'composed':
        with monkeypatch.context() as m:
            m.setattr(fused, '_ab_spin_fused', lambda *a: False)
            A, B = fused.ab_rfgr(Q['rf'], Q['gr'], Q['loc'], **kw)
    else:
        A, B = fused.ab_rfgr(Q['rf'], Q['gr'], Q['loc'], **kw)
    res = dict(A=A.detach(), B=B.detach())
    if wrt:
        wA, wB = ab_weights(v)
        torch.autograd.backward([A, B], [place(wA), place(wB)])
        res.update({k: Q[k].grad for k in wrt if Q[k] is not None})
    return res


def _want(ora, v, k):
    r"""``(the oracle's gradient in the operand's own shape, Σ_s|g_s| in that shape or None for a gradient with a spin
    axis)``."""
    if k not in PER_SPIN:
        return ora[k].reshape(v[k].shape), None
    ref = fold_like(ora[k], v[k])
    summed = v[k].numel() < ora[k].shape[1]          # no spin axis: every element is a sum over nM spins
    return ref, fold_like(ora[k].abs(), v[k]) if summed else None


def _check(key, got, ora, d32, v, tag, mode, wrt=LEAVES, gate=True):
    r"""Every gradient of ``wrt`` in its operand's shape and dtype, finite, within the gates of the module docstring."""
    for k in wrt:
        if v[k] is None:
            continue
        g = got[k]
        if g is None:                                # γ_beff without a Δf: the field does not depend on it
            assert k == 'γ_beff' and v['Δf'] is None, (key, k)
            continue
        assert g.shape == v[k].shape and g.dtype == v[k].dtype and bool(torch.isfinite(g).all()), (key, k, g.shape)
        ref, scale = _want(ora, v, k)
        tol = TOL[tag]
        if d32 is not None:
            record(f'abspin.{key}.{k}.chain_f32_vs_f64', d32[k], note='the oracle chain in fp32 against itself in fp64, CPU')
            if d32[k] > tol / 3:
                tol = 3 * d32[k]
        if scale is not None:
            d = float(((g.detach().double().cpu() - ref).abs() / scale.clamp_min(1e-300)).max())
            what = '|got - want| / sum|g_s|'
        else:
            d = max_abs(g, ref) if tag == 'f64' else rel_l2(g, ref)
            what = 'max abs' if tag == 'f64' else 'relative L2'
        record(f'abspin.{key}.{k}', d, tol if (gate and mode == 'precise') else None, note=what)
        if gate and mode == 'precise':
            assert d <= tol, f'{key}: grad {k}: {what} {d:.3e} > {tol:.1e}'


# =============================================================================================
# 1. values
# =============================================================================================
@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('relax', [True, False], ids=['relax', 'norelax'])
@pytest.mark.parametrize('nC', [0, 1])
@pytest.mark.parametrize('nT', [16, 48, 50, 7])
def test_values(tag, mode, relax, nC, nT, monkeypatch):
    r"""Every operand requires grad; one segment, three, the split route (48 fused + 2 composed steps) and the composed
    route (7 steps), with and without a ``b1Map`` and relaxation.  The fused call against the three yardsticks of the
    module docstring; the composed route and the column identity against each other's values as well."""
    v = _case(tag, 'gamma_split', nC, nT, relax)
    ora, d32 = _oracle(tag, 'gamma_split', nC, nT, relax)
    key = f'values.{tag}.{mode}.c{nC}.nT{nT}.{"relax" if relax else "norelax"}'
    with mrphy_amd.precision(mode):
        fu = _run('fused', v)                       # on the constants the oracle is handed (host_constants)
        # the GPU yardsticks on the constants of the device, all three routes alike: in fp32 B is proportional to
        # E1 - 1, which another exp() moves by a per cent (module docstring)
        with mrphy_amd.constants_on('native'):
            fun = _run('fused', v)
            co = _run('composed', v, monkeypatch=monkeypatch)
            kb = _run('k2b', v)
    for k in ('A', 'B'):
        assert_close(fun[k], co[k], tag, f'{key}: {k} vs the composed route')
        if mode == 'precise':
            assert_close(fun[k], kb[k], tag, f'{key}: {k} vs the column identity')
            assert_close(fu[k], ora[k], tag, f'{key}: {k} vs the oracle')
    _check(key + '.vs_oracle', fu, ora, d32, v, tag, mode)
    # (b), (c): the other GPU routes as yardsticks, by the same gates, their per-spin terms taken from the oracle
    for name, other in (('vs_composed', co), ('vs_k2b', kb)):
        for k in LEAVES:
            if v[k] is None or fun[k] is None:
                continue
            assert other[k] is not None and other[k].shape == fun[k].shape, (key, name, k)
            _, scale = _want(ora, v, k)
            if scale is not None:
                d = float(((fun[k] - other[k]).abs().double().cpu() / scale.clamp_min(1e-300)).max())
            else:
                d = max_abs(fun[k], other[k]) if tag == 'f64' else rel_l2(fun[k], other[k])
            record(f'abspin.{key}.{name}.{k}', d, TOL[tag] if mode == 'precise' else None)
            if mode == 'precise':
                assert d <= TOL[tag], f'{key}: grad {k} {name}: {d:.3e}'


# =============================================================================================
# 2. bits
# =============================================================================================
@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('nC', [0, 1])
@pytest.mark.parametrize('nT', [48, 50])
def test_bits(tag, mode, nC, nT):
    r"""``A, B`` are the bits of the call without these gradients; over whole segments ``grad_rf`` / ``grad_gr`` are the
    pulse-only call's (the plain K2abb's); each operand alone gets the bits it has in the full set (over whole segments:
    one K2abb build against another; nT = 50 adds a composed tail, see below); a second run gives the same bits."""
    v = _case(tag, 'gamma_split', nC, nT)
    with mrphy_amd.precision(mode):
        full, again = _run('fused', v), _run('fused', v)
        none, pulse = _run('fused', v, wrt=()), _run('fused', v, wrt=('rf', 'gr'))
        for k in full:
            if full[k] is not None:
                _same_bits(full[k], again[k], f'{k}, second run')
        for k in ('A', 'B'):
            if nT % 16 == 0:
                _same_bits(full[k], none[k], f'{k}, with and without gradients')
            else:                                   # the split joins two parts by 3x3 products: other roundings
                assert_close(full[k], none[k], tag, f'{k}, the split route vs one sweep')
            _same_bits(full[k], pulse[k], f'{k}, every gradient vs the pulse gradient alone')
        if nT % 16 == 0:
            for k in ('rf', 'gr'):
                _same_bits(full[k], pulse[k], f'grad {k}: every gradient vs the pulse gradient alone')
        for k in LEAVES[2:]:
            if v[k] is None:
                continue
            one = _run('fused', v, wrt=(k,))
            _same_bits(one['A'], full['A'], f'A with grad {k} alone')
            if nT % 16 == 0:
                _same_bits(one[k], full[k], f'grad {k} alone vs in the full set')
            else:
                # the tail of the split route is rfgr2beff + beff2ab, whose adjoint runs another build when the
                # constants' gradients are wanted too (mrphy_beff2ab_bwd_consts for mrphy_beff2ab_bwd).  Measured:
                # grad_loc alone differs from the full set's in the last place (1.1e-16 fp64, 6.0e-8 fp32) at nT = 50
                # and in no bit at nT = 48 -- presumably from there; across the join the property is the gate's
                record(f'abspin.bits.{tag}.{mode}.c{nC}.nT{nT}.{k}.alone_vs_full.max_abs', max_abs(one[k], full[k]))
                assert_close(one[k], full[k], tag, f'grad {k} alone vs in the full set, across the split')


# =============================================================================================
# 3. route and memory
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('wrt,name', [(('Δf', 'T1'), CONSTS_BWD), (('Δf', 'loc'), MAPS_BWD), (('rf',), BWD),
                                      (('rf', 'gr', 'b1Map', 'γ'), CONSTS_BWD)])
def test_one_forward_and_one_adjoint_call(tag, wrt, name, monkeypatch):
    r"""nT = 48: exactly one ``mrphy_ab_rfgr_fwd`` and one call of the cheapest adjoint that serves what is wanted; nothing
    of ``rfgr2beff`` + ``beff2ab``."""
    v = _case(tag, 'gamma_split', 1, 48)
    calls = _counted(monkeypatch, (FWD, BWD, MAPS_BWD, CONSTS_BWD) + COMPOSED)
    got = _run('fused', v, wrt=wrt)
    assert all(got[k] is not None for k in wrt)
    assert dict(calls) == {FWD: 1, name: 1}, dict(calls)


def test_split_route_calls(monkeypatch):
    r"""nT = 50: the 48 fused steps are one forward and one CONSTS adjoint; the two composed steps are the tail's."""
    v = _case('f32', 'gamma_split', 1, 50)
    calls = _counted(monkeypatch, (FWD, BWD, MAPS_BWD, CONSTS_BWD) + COMPOSED)
    _run('fused', v, wrt=('Δf', 'T1'))
    assert calls[FWD] == 1 and calls[CONSTS_BWD] == 1 and calls[BWD] == calls[MAPS_BWD] == 0, dict(calls)
    assert calls['mrphy_rfgr2beff_st'] == 1, dict(calls)


def test_peak_memory_stays_below_one_beff():
    r"""N = 1, nM = 4096, nT = 256, fp32, every spin-side gradient wanted: the allocator's peak over forward + backward,
    above what the operands hold, stays below the bytes of ONE ``Beff`` (``N nM nT 3 4``) -- the tensor the composed route
    cannot avoid, beside its history and ``grad_Beff``.  The checkpoints are a quarter of it."""
    N, nM, nT = 1, 4096, 256
    gen = torch.Generator().manual_seed(77)
    u = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64)  # noqa: E731
    leaf = lambda x: x.float().to(DEV).requires_grad_(True)  # noqa: E731
    rf, gr, loc = leaf((u(N, 2, nT) * 2 - 1) * 3), leaf(u(N, 3, nT) * 2 - 1), leaf((u(N, nM, 3) * 2 - 1) * 6)
    kw = dict(Δf=leaf((u(N, nM) * 2 - 1) * 200), b1Map=leaf(u(N, nM, 2) * 2 - 1), T1=leaf(0.5 + u(N, nM)),
              T2=leaf(0.02 + 0.1 * u(N, nM)))
    wA, wB = (u(N, nM, 3, 3) * 2 - 1).float().to(DEV), (u(N, nM, 3) * 2 - 1).float().to(DEV)

    def once():
        A, B = fused.ab_rfgr(rf, gr, loc, **kw)
        torch.autograd.backward([A, B], [wA, wB])
    once()                                          # (the constants' caches, the gradients' buffers)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    once()
    torch.cuda.synchronize()
    peak, beff = torch.cuda.max_memory_allocated() - base, N * nM * nT * 3 * 4
    record('abspin.memory.peak_over_one_beff', peak / beff, 1.0, note=f'{peak} B over {beff} B')
    assert peak < beff, (peak, beff)
    assert all(x.grad is not None and bool(torch.isfinite(x.grad).all()) for x in (rf, gr, loc, *kw.values()))


# =============================================================================================
# 4. operand forms
# =============================================================================================
FORMS = [(nC, n) for nC in (0, 1) for n in TWO_D + ('zero', 'gamma0')]


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('nC,name', FORMS, ids=[f'c{c}-{n}' for c, n in FORMS])
def test_operand_forms(tag, mode, nC, name):
    r"""Broadcast, 0-dim and stride-0 operands, permuted views, buffers off the 16-byte grid, ``γ_beff != γ``, a batch
    ``dt``, dead time with spins at the iso-centre, spins with ``γ = 0`` (``dL/dγ`` is right there because the sweep sums
    the raw ``dL/db``): every gradient in its operand's own shape and dtype, finite, within the gates."""
    v = _case(tag, name, nC, 48)
    ora, d32 = _oracle(tag, name, nC, 48)
    if name == 'expanded':
        assert all(0 in place(v[k]).stride() for k in ('loc', 'Δf', 'γ_beff', 'T1', 'T2', 'γ'))
    if name == 'offset':
        assert place(v['loc']).data_ptr() % 16 != 0
    with mrphy_amd.precision(mode):
        fu = _run('fused', v)
    _check(f'forms.{tag}.{mode}.c{nC}.{name}', fu, ora, d32, v, tag, mode)
    if name == 'gamma0':
        for n, s in cases.ZERO_SPINS:               # a spin that never rotates still has a gradient w.r.t. its γ
            assert float(ora['γ'][n, s].abs()) > 0 and bool(torch.isfinite(fu['γ'][n, s]))
            if mode == 'precise':
                assert abs(float(fu['γ'][n, s]) - float(ora['γ'][n, s])) <= (1e-9 if tag == 'f64' else
                                                                             1e-5 * float(ora['γ'].abs().max()))


# =============================================================================================
# 5. more tiles than persistent waves
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_second_tile_per_wave(tag):
    r"""N = 2, nT = 32, ``nM = P 64 + 100`` with ``P`` from the workspace query: waves 0 and 1 take a second tile, wave 1's
    ragged.  The per-spin gradients of the spins past tile ``P`` alone against the oracle on those spins (spins are
    independent): a running sum that is not reset per tile carries tile 0's into them, an unmasked ragged lane writes
    past the batch entry."""
    N, nT = 2, 32
    lib = mrphy_amd.require_library()
    code = _host.dtype_code(DT[tag], DT[tag])
    P = int(lib.mrphy_blochsim_rfgr_bwd_workspace(code, N, 1 << 30, nT)) // (N * 5 * nT * DT[tag].itemsize)
    nM = P * 64 + 100
    gen = torch.Generator().manual_seed(91)
    u = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64)  # noqa: E731
    c = lambda x: x.to(DT[tag])  # noqa: E731
    v = dict(rf=c((u(N, 2, nT) * 2 - 1) * 3), gr=c(u(N, 3, nT) * 2 - 1), loc=c((u(N, nM, 3) * 2 - 1) * 6),
             Δf=c((u(N, nM) * 2 - 1) * 200), b1Map=c(u(N, nM, 2) * 2 - 1), γ_beff=c(4257.6 * (0.9 + 0.2 * u(N, nM))),
             T1=c(0.5 + u(N, nM)), T2=c(0.02 + 0.1 * u(N, nM)), γ=c(4257.6 * (0.9 + 0.2 * u(N, nM))),
             dt=torch.tensor([4e-6], dtype=DT[tag]), w=c(u(N, nM, 3) * 2 - 1))
    tail = slice(P * 64, nM)
    sub = {k: (x if k in ('rf', 'gr', 'dt') else x[:, tail].contiguous()) for k, x in v.items()}
    with mrphy_amd.constants_on('cpu'):
        fu = _run('fused', v, wrt=LEAVES[2:])
        again = _run('fused', v, wrt=LEAVES[2:])
    ora = oracle_ab_spin_grads(sub, factors=_factors(sub, tag))
    for k in ('loc', 'Δf', 'b1Map', 'γ_beff', 'T1', 'T2', 'γ'):
        _same_bits(fu[k], again[k], f'grad {k}, second run')
        got, ref = fu[k][:, tail], ora[k].reshape(fu[k][:, tail].shape)
        d = record(f'abspin.tiles.{tag}.{k}', max_abs(got, ref) if tag == 'f64' else rel_l2(got, ref), TOL[tag])
        assert d <= TOL[tag], (k, d)
        assert bool(torch.isfinite(fu[k]).all()), k
    for k in ('A', 'B'):
        assert_close(fu[k][:, tail], ora[k], tag, f'{k} past tile P')


# =============================================================================================
# 6. dtype codes
# =============================================================================================
@pytest.mark.parametrize('mode', ['fast', 'precise'])
@pytest.mark.parametrize('wide', [False, True])
def test_dtype_codes(mode, wide, monkeypatch):
    r"""fp32 data through dtype codes 0 / 2 (fast) and 3 / 4 (precise: all four columns carry ``t = E h``, which the sums
    take as it is and one ``adj_const_finish`` divides out), per-spin constants, with relaxation and a map, against the
    composed route in the same mode; code 3 also against the oracle.  A missing or doubled ``E`` shows at order 1."""
    v = dict(_case('f32', 'views', 1, 48))
    if wide:
        for k in ('T1', 'T2', 'γ', 'dt'):
            v[k] = v[k].double()
    with mrphy_amd.precision(mode), mrphy_amd.constants_on('native'):
        code = _host.dtype_code(torch.float32, torch.float64 if wide else torch.float32)
        assert code == {('fast', False): 0, ('fast', True): 2, ('precise', False): 3, ('precise', True): 4}[mode, wide]
        fu = _run('fused', v)
        co = _run('composed', v, monkeypatch=monkeypatch)
    ora, _ = _oracle('f32', 'views', 1, 48)
    for k in LEAVES:
        assert fu[k].dtype == v[k].dtype and fu[k].shape == co[k].shape == v[k].shape, k
        _, scale = _want(ora, v, k)
        if scale is not None:
            d = float(((fu[k] - co[k]).abs().double().cpu() / scale.clamp_min(1e-300)).max())
        else:
            d = rel_l2(fu[k], co[k])
        record(f'abspin.code{code}.{k}.vs_composed', d, 1e-5)
        assert d <= 1e-5, (code, k, d)
    if code == 3:
        with mrphy_amd.constants_on('cpu'), mrphy_amd.precision(mode):
            fu = _run('fused', v)
        _check('code3.vs_oracle', fu, ora, None, v, 'f32', 'precise')


# =============================================================================================
# 7. the steady state end to end
# =============================================================================================
SS_WRT = ('rf', 'gr', 'T1', 'T2', 'Δf', 'b1Map')


@functools.lru_cache(maxsize=None)
def _ss_case(tag):
    r"""'views' with a map, ``T1`` in 0.05 .. 0.15 s and ``T2`` in 0.02 .. 0.07 s per spin (as ``test_ab_operands._ss_case``
    draws them: ``I - A F`` well conditioned), a rest per batch entry and a ``Δf_rest`` per spin."""
    v = dict(_case(tag, 'views', 1, 48))
    gen = torch.Generator().manual_seed(5100)
    rnd = lambda s: torch.rand(tuple(s), generator=gen, dtype=torch.float64)  # noqa: E731
    v.update(T1=(0.05 + 0.1 * rnd(v['T1'].shape)).to(DT[tag]), T2=(0.02 + 0.05 * rnd(v['T2'].shape)).to(DT[tag]))
    return v, torch.tensor([5e-3, 6.5e-3], dtype=DT[tag]), ((rnd(v['loc'].shape[:-1]) * 2 - 1) * 200).to(DT[tag])


@functools.lru_cache(maxsize=None)
def _ss_oracle(tag):
    v, rest, df_rest = _ss_case(tag)

    def chain(dtype):
        w = lambda x: x.detach().to(dtype)  # noqa: E731

        def loss(A, B, Q):
            Mss = torch_steadystate(A, B, w(rest), Q['T1'], Q['T2'], w(df_rest))
            return (Mss * w(v['w'])).sum(), Mss
        return oracle_ab_spin_grads(v, dtype=dtype, loss=loss)
    wide = chain(torch.float64)
    if tag == 'f64':
        return wide, None
    low = chain(torch.float32)
    return wide, {k: rel_l2(low[k], wide[k]) for k in SS_WRT + ('extra',)}


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
def test_steadystate_end_to_end(tag, mode):
    r"""``steadystate_rfgr`` with ``rf, gr, T1, T2, Δf, b1Map`` requiring grad, nT = 48, a rest per batch entry and a
    ``Δf_rest``: ``Mss`` and the six gradients against ``torch_steadystate`` on the fp64 column chain; ``T1`` and ``T2``,
    shared by the pulse and the rest, receive the sum of both paths (the oracle's leaves feed both).  fp64:
    ``test_steadystate._gate``.  fp32: three times the same chain's fp32-vs-fp64 distance on the CPU (``Mss`` inherits the
    rounding of an fp32 ``A`` amplified by the conditioning of ``I - A F``); CPU dry run of that distance (relative L2):
    ``Mss`` 8.4e-6, ``rf`` 1.1e-5, ``gr`` 1.8e-5, ``T1`` 1.2e-5, ``T2`` 1.1e-5, ``Δf`` 2.3e-5, ``b1Map`` 1.5e-5; the run's
    own figures go to the ledger."""
    v, rest, df_rest = _ss_case(tag)
    wide, d32 = _ss_oracle(tag)

    def steady():
        Q = {k: (place(v[k]).detach().requires_grad_(k in SS_WRT)) for k in LEAVES}
        Mss = fused.steadystate_rfgr(Q['rf'], Q['gr'], Q['loc'], rest=dev(rest), T1=Q['T1'], T2=Q['T2'], Δf=Q['Δf'],
                                     b1Map=Q['b1Map'], γ_beff=Q['γ_beff'], γ=Q['γ'], dt=Q['dt'], Δf_rest=dev(df_rest))
        torch.autograd.backward([Mss], [place(v['w'])])
        return dict(extra=Mss.detach(), **{k: Q[k].grad for k in SS_WRT})
    key = f'abspin.ss.{tag}.{mode}'
    with mrphy_amd.precision(mode):
        got, again = steady(), steady()
    for k in SS_WRT + ('extra',):
        _same_bits(got[k], again[k], f'{key}: {k}, second run')
        ref = wide[k].reshape(got[k].shape)
        if tag == 'f64':
            _ss_gate(got[k], ref, tag, 'Mss' if k == 'extra' else 'grad_' + k)
            continue
        record(f'{key}.{k}.chain_f32_vs_f64', d32[k], note='the oracle chain in fp32 against itself in fp64, CPU')
        d = record(f'{key}.{k}.vs_oracle64', rel_l2(got[k], ref), 3 * d32[k] if mode == 'precise' else None)
        if mode == 'precise':
            assert d <= 3 * d32[k], f'{key} {k}: {d:.3e} > 3 x {d32[k]:.3e}, the oracle chain\'s own fp32 distance'
