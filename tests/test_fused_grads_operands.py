r"""The MAPS and CONSTS builds of K2b / K2bt / K2bs -- the gradients of ``fused.blochsim_rfgr``, ``blochsim_rfgr_traj`` and
``signal_rfgr`` w.r.t. ``loc, Δf, b1Map`` and w.r.t. ``T1, T2, γ, dt, γ_beff`` -- on every operand form the host code accepts
(``cases.fused_operand_variants``: broadcast shapes, 0-dim and stride-0 leaves, a general ``*Nd`` grid, permuted views,
buffers off the 16-byte grid), on steps of exactly zero field and with spins whose ``γ`` is 0.

Per case and function, two calls: one with ``Mi, rf, gr, loc, Δf, b1Map`` as leaves, one with ``T1, T2, γ, dt, γ_beff`` (the
signal call: without ``γ_beff``, which counts with the maps there), every leaf in the form it is given in.  Each gradient has
its operand's shape and dtype; equals the two-kernel route's (``rfgr2beff`` + ``sims.blochsim``; ``slowsims.blochsim`` for
the constants) and the fp64 CPU oracle's; ``out`` keeps the bits of the call without gradients (``sig`` where the signal
kernel forms it: with map gradients, and in the tail of a split length, ``signal_rfgr`` documents the product and the sum
in torch -- there ``sig`` is held to the gate, and to the bits of the pulse-gradient call, which takes the same route); a
second run gives the same bits; whole segments take the one fused entry point the functions document, counted.

Yardsticks (``test_fused_consts_host.oracle_fused``, pinned by ``test_slow_oracle_at_zero_field``): the EXPLICIT adjoint
for ``Mi, rf, gr, loc, Δf, b1Map`` -- it holds the analytic zero-field limit --, the slow autograd form for ``T1, T2, γ,
dt, γ_beff``, from which nothing but those is taken.  Gates: the pulse and the maps ``util.assert_close`` (fp64 max-abs
1e-9, fp32 relative L2 1e-5: ``test_fused_maps.py``); the constants relative L2 <= 1e-9 / 2e-5 (``test_fused_consts.py``)
where the operand has one entry per spin, and where it is shared over spins (0-dim, `(1, 1)`, `(N, 1)`, a plane of a
grid) each entry by ``test_fused_consts._gate_sum``'s rule ``|got - want| <= gate · Σ_s |g_s|`` over the spins ``s`` it is
summed over, the per-spin terms ``g_s`` from the fp64 oracle on the dense spelling.  All under ``constants_on('native')``,
as ``test_fused_consts.py`` runs.
"""
import functools

import pytest

from gpu_common import *  # noqa: F401,F403
from test_ab_operands import _case
from test_fused_consts import CONSTS_BWD, MAPS_BWD, SIG_CONSTS_BWD, TOL, _counted
from test_fused_consts_host import CONST_LEAVES, FIELD_LEAVES, oracle_fused, zero_field_maps_case
from test_fused_operands import VARIANTS, _cotangent, _same_bits
from test_signal_operands import _rx_coils, _sig_weights, _traj_cotangent
from mrphy_amd.fused import _traj_ends

pytestmark = pytest.mark.gpu

EVERY = 5
FNS = ('Mo', 'traj', 'sig')
KEYS = FIELD_LEAVES + CONST_LEAVES
SIG_CONSTS = ('T1', 'T2', 'γ', 'dt')         # the signal call's fused constants; its γ_beff goes with the maps


# ---------------------------------------------------------------------------------------------
# cotangents, runs, oracles
# ---------------------------------------------------------------------------------------------
def _ends(fn, nT):
    return [nT] if fn == 'Mo' else _traj_ends(nT, EVERY)


def _cots(fn, v, dtype):
    r"""``(ws, cot)``: the signal's own cotangent (``None`` otherwise) and the cotangent of the trajectory
    `(N, *Nd, nRec, 3)` that the loss is, on the CPU in ``dtype`` -- ``w`` on ``Mo``; ``test_fused_operands._cotangent`` on the
    trajectory; for the signal ``<ws, sig> + <w, Mo>`` as ``test_signal_operands._traj_cotangent`` writes it."""
    nT = v['rf'].shape[2]
    if fn == 'Mo':
        return None, v['w'].unsqueeze(-2)
    if fn == 'traj':
        return None, _cotangent(v, EVERY, nT)
    r, coils = _rx_coils(v, dtype)
    ws = _sig_weights((r.shape[0], 2, len(_ends(fn, nT))) + ((r.shape[3],) if coils else ())).to(dtype).double()
    return ws, _traj_cotangent(v, r, ws).to(dtype)


def _run(route, fn, v, needs, rx_on_cpu=False):
    r"""``{'out': .., <leaf>: gradient}``; ``route`` 'fused' (the function ``fn`` names; ``out`` is ``Mo``, the trajectory
    or ``(sig, Mo)``), 'two' (``rfgr2beff`` + ``sims.blochsim`` -- ``slowsims.blochsim`` when a constant is a leaf -- per
    record segment over slices of one ``Beff``, the loss as a trajectory loss; ``out`` the trajectory) or 'plain' (the
    function under ``no_grad``).  The operands go in AS GIVEN (``place``); a leaf is a detached alias of that form."""
    dtype = v['loc'].dtype
    Q = {k: (None if v.get(k) is None else place(v[k]).detach().requires_grad_(True) if k in needs and route != 'plain'
             else place(v[k])) for k in KEYS}
    nT = v['rf'].shape[2]
    kw = dict(Δf=Q['Δf'], b1Map=Q['b1Map'], γ_beff=Q['γ_beff'], T1=Q['T1'], T2=Q['T2'], γ=Q['γ'], dt=Q['dt'])
    ws, cot = _cots(fn, v, dtype)
    if route == 'two':
        step = slowsims.blochsim if any(k in CONST_LEAVES[:4] for k in needs) else sims.blochsim
        beff = beffective.rfgr2beff(Q['rf'], Q['gr'], Q['loc'], Δf=Q['Δf'], b1Map=Q['b1Map'], γ=Q['γ_beff'])
        recs, M, t0 = [], Q['M0'], 0
        for e in _ends(fn, nT):
            M = step(M, beff[..., t0:e, :], T1=Q['T1'], T2=Q['T2'], γ=Q['γ'], dt=Q['dt'])
            recs.append(M)
            t0 = e
        out = torch.stack(recs, dim=-2)
        torch.autograd.backward([out], [place(cot)])
    else:
        with torch.set_grad_enabled(route != 'plain'):
            if fn == 'Mo':
                out = fused.blochsim_rfgr(Q['M0'], Q['rf'], Q['gr'], Q['loc'], **kw)
            elif fn == 'traj':
                out = fused.blochsim_rfgr_traj(Q['M0'], Q['rf'], Q['gr'], Q['loc'], every=EVERY, **kw)
            else:
                rx = v.get('rx') if rx_on_cpu else place(v.get('rx'))
                out = fused.signal_rfgr(Q['M0'], Q['rf'], Q['gr'], Q['loc'], every=EVERY, rx=rx, return_Mo=True, **kw)
        if route == 'plain':
            return {'out': out}
        if fn == 'sig':
            torch.autograd.backward(list(out), [dev(ws.to(dtype)), place(v['w'])])
        else:
            torch.autograd.backward([out], [place(cot if fn == 'traj' else v['w'])])
    res = {k: Q[k].grad for k in needs if Q[k] is not None}
    res['out'] = tuple(o.detach() for o in out) if isinstance(out, tuple) else out.detach()
    return res


def _per_spin(v):
    r"""The dense spelling with ``dt`` per spin as well: every constant a leaf `(N, nM)`, whose gradients are the per-spin
    terms ``g_s`` of any summed form."""
    d = cases.fused_dense(v)
    N, nM = d['loc'].shape[:2]
    return dict(d, dt=d['dt'][:, None].expand(N, nM).contiguous())


@functools.lru_cache(maxsize=None)
def _oracles(tag, kind, nC, nT, name, fn):
    r"""``(explicit, terms)``: the explicit oracle's ``out`` and gradients w.r.t. ``Mi, rf, gr, loc, Δf, b1Map`` on the
    operands as given, and the slow-form oracle's per-spin gradients `(N, *Nd)` w.r.t. ``T1, T2, γ, dt, γ_beff``."""
    v = _problem(tag, kind, nC, nT, name)
    _, cot = _cots(fn, v, DT[tag])
    ends = _ends(fn, nT)
    expl = oracle_fused(v, 'explicit', FIELD_LEAVES, ends, cot)
    d = _per_spin(v)
    slow = oracle_fused(d, 'slow', CONST_LEAVES, ends, cot.reshape(tuple(d['loc'].shape[:-1]) + tuple(cot.shape[-2:])))
    lead = tuple(v['loc'].shape[:-1])
    return expl, {k: slow[k].reshape(lead) for k in CONST_LEAVES}


def _problem(tag, kind, nC, nT, name=None):
    if kind == 'zero':
        return zero_field_maps_case(DT[tag], nC, nT)[0]
    return _case(tag, kind, nC, nT, name)[0]


def _hold_const(key, k, got, like, gs, tag, ref=None):
    r"""One constant's gradient ``got`` against the per-spin fp64 terms ``gs`` `(N, *Nd)` (module docstring), or against
    ``ref`` (the two-kernel route's) on the same scale."""
    assert got is not None and got.shape == like.shape and got.dtype == like.dtype, (key, k, got, like.shape)
    assert bool(torch.isfinite(got).all()), (key, k)
    shp = (tuple(like.shape) + (gs.ndim - like.ndim) * (1,)) if like.ndim else (1,) * gs.ndim
    want = (gs.sum_to_size(shp) if ref is None else ref.detach().double().cpu().reshape(shp))
    scale = gs.abs().sum_to_size(shp)
    g = got.detach().double().cpu().reshape(shp)
    shared = any(a == 1 and b > 1 for a, b in zip(shp[1:], gs.shape[1:]))
    if shared:
        d = float(((g - want).abs() / scale.clamp(min=1e-300)).max())
    else:
        d = rel_l2(g, want)
    record(f'fusedgrads.{key}.{k}.{"vs_oracle" if ref is None else "vs_two_kernel"}', d, TOL[tag],
           note='max |got - want| / sum_s |g_s|' if shared else 'relative L2')
    assert d <= TOL[tag], (key, k, 'shared' if shared else 'per spin', d)


def _check(tag, kind, nC, nT, name, fn, monkeypatch=None):
    r"""The module docstring's checks for one case and one function; returns ``(maps call, constants call, oracles)``."""
    v = _problem(tag, kind, nC, nT, name)
    key = f'{tag}.c{nC}.nT{nT}.{name or kind}.{fn}'
    cpu_rx = name == 'gamma_split' or kind == 'gamma0'          # that variant's fp64 rx is meant to stay on the CPU
    run = lambda route, needs: _run(route, fn, v, needs, cpu_rx)  # noqa: E731
    cneeds = SIG_CONSTS if fn == 'sig' else CONST_LEAVES
    calls = _counted(monkeypatch) if monkeypatch is not None else None
    with mrphy_amd.constants_on('native'):
        plain = run('plain', ())
        if calls is not None:
            calls.clear()
        gm = run('fused', FIELD_LEAVES)
        n_maps = dict(calls) if calls is not None else None
        if calls is not None:
            calls.clear()
        gc = run('fused', cneeds)
        n_consts = dict(calls) if calls is not None else None
        if fn == 'sig':       # γ_beff beside a Δf is a map gradient: the signal call composes it
            gc['γ_beff'] = run('fused', ('γ_beff',))['γ_beff']
        gm2, gc2 = run('fused', FIELD_LEAVES), run('fused', cneeds)
        pulse = run('fused', FIELD_LEAVES[:3]) if fn == 'sig' and nT % 16 else None
        tm, tc = run('two', FIELD_LEAVES), run('two', CONST_LEAVES)
    if n_maps is not None and nT % 16 == 0 and nC <= 1:
        composed = [n for n in n_maps if n.startswith(('mrphy_rfgr2beff', 'mrphy_blochsim_fwd'))]
        assert n_maps.get(MAPS_BWD) == 1 and not composed and not n_maps.get(SIG_CONSTS_BWD), (key, n_maps)
        want = SIG_CONSTS_BWD if fn == 'sig' else CONSTS_BWD
        assert n_consts.get(want, 0) >= 1 and sum(n_consts.values()) == n_consts[want], (key, n_consts)
    outs = lambda r: r['out'] if isinstance(r['out'], tuple) else (r['out'],)  # noqa: E731
    for which, g, g2 in (('maps', gm, gm2), ('consts', gc, gc2)):
        for i, (a, b) in enumerate(zip(outs(g), outs(plain))):
            if fn == 'sig' and i == 0 and (which == 'maps' or nT % 16):
                # composed -- with the constants: the records of the split route's tail --: the product and the sum in
                # torch, not K2s: the kernel's sum to the gate, and the bits of the pulse-gradient call, which takes the
                # same route
                assert_close(a, b, tag, f'{key}: sig of the composed route vs the signal kernel')
                if which == 'consts':
                    _same_bits(a, pulse['out'][0], f'{key}: sig with the consts gradients vs with the pulse gradients')
            else:
                _same_bits(a, b, f'{key}: out with the {which} gradients vs without')
        for k in g2:
            if k != 'out':
                _same_bits(g[k], g2[k], f'{key}: grad {k}, second run')
    expl, terms = _oracles(tag, kind, nC, nT, name, fn)
    out = outs(gm)[-1] if fn != 'traj' else outs(gm)[0][..., -1, :]
    assert_close(out, expl['out'][..., -1, :], tag, f'{key}: the final state vs oracle')
    for k in FIELD_LEAVES:
        if v.get(k) is None:
            assert k not in gm
            continue
        assert gm[k] is not None and gm[k].shape == v[k].shape and gm[k].dtype == v[k].dtype, (key, k)
        assert bool(torch.isfinite(gm[k]).all()), (key, k)
        record(f'fusedgrads.{key}.{k}.vs_oracle', max_abs(gm[k], expl[k]) if tag == 'f64' else rel_l2(gm[k], expl[k]),
               1e-9 if tag == 'f64' else 1e-5)
        assert_close(gm[k], tm[k], tag, f'{key}: grad {k} vs two-kernel route')
        assert_close(gm[k], expl[k], tag, f'{key}: grad {k} vs oracle')
    for k in CONST_LEAVES:
        if kind == 'zero' and k == 'γ_beff':
            continue
        _hold_const(key, k, gc[k], v[k], terms[k], tag)
        _hold_const(key, k, gc[k], v[k], terms[k], tag, ref=tc[k])
    return gm, gc, (expl, terms)


# =============================================================================================
# (a) spellings
# =============================================================================================
SPELLINGS = [(nC, n, 48) for nC in (0, 1) for n in VARIANTS] + [(nC, n, 53) for nC in (0, 1) for n in cases.FUSED_NT53]


@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('fn', FNS)
@pytest.mark.parametrize('nC,name,nT', SPELLINGS, ids=[f'c{c}-{n}-{t_}' for c, n, t_ in SPELLINGS])
def test_operand_spellings(tag, fn, nC, name, nT, monkeypatch):
    r"""One problem, many spellings, each gradient in the form of its operand (module docstring).  nT = 48: one fused
    launch per call; nT = 53: the fused part plus five composed steps, autograd adds the parts' gradients."""
    given = _case(tag, 'zoo', nC, nT, name)[0]
    if name == 'views':        # the forms under test arrive as such
        assert not any(place(given[k]).is_contiguous() for k in ('M0', 'loc', 'Δf', 'rf', 'gr', 'w'))
    if name == 'offset':
        assert all(place(given[k]).is_contiguous() and place(given[k]).data_ptr() % 16 != 0
                   for k in ('M0', 'loc', 'rf', 'gr', 'w'))
    if name == 'expanded':
        assert all(0 in place(given[k]).stride() for k in ('loc', 'Δf', 'γ_beff', 'T1', 'T2', 'γ'))
    _check(tag, 'zoo', nC, nT, name, fn, monkeypatch)


# =============================================================================================
# (b) zero field
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('fn', FNS)
@pytest.mark.parametrize('nC', [0, 1])
@pytest.mark.parametrize('nT', [48, 53])
def test_zero_field_steps(tag, fn, nC, nT):
    r"""``cases.zero_field_case`` with ``Δf`` an exact-zero `(N, nM)` leaf: dead time, spins at the iso-centre, a spin whose
    ``b1Map`` is 0.  The pulse and the maps against the EXPLICIT oracle, ``T1, T2, γ, dt`` against the slow form; ``γ_beff``
    beside the zero ``Δf`` gets an exact zero.  The case discriminates: on the final-state loss the slow form's ``grad_loc``
    / ``grad_Δf`` are 0.014 .. 0.099 / 0.42 .. 0.46 in relative L2 from the explicit oracle's (CPU dry run in fp64 over nC =
    0, 1 and nT = 48, 53; ``grad_b1Map``: 0.035, 0.013) -- more than 1e3 gates --, so a kernel that returned the autograd
    zeros of the dead steps would miss by that much, and one held to the slow form could not pass."""
    gm, gc, _ = _check(tag, 'zero', nC, nT, None, fn)
    g = gc['γ_beff']
    v = _problem(tag, 'zero', nC, nT)
    assert g is not None and g.shape == v['γ_beff'].shape and float(g.abs().max()) == 0.0, g
    # once, on the CPU: the two oracle forms part ways here
    d = _slow_vs_explicit(nC, nT)
    assert all(x > 1e3 * 1e-5 for x in d.values()), d


@functools.lru_cache(maxsize=None)
def _slow_vs_explicit(nC, nT):
    v = zero_field_maps_case(torch.float64, nC, nT)[0]
    slow, expl = (oracle_fused(v, sim, ('loc', 'Δf')) for sim in ('slow', 'explicit'))
    return {k: rel_l2(slow[k], expl[k]) for k in ('loc', 'Δf')}


# =============================================================================================
# (c) spins with γ = 0 in the CONSTS builds
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('fn', FNS)
def test_gamma_zero_spins(tag, fn):
    r"""Per-spin ``γ`` `(N, nM)` with ``γ[0, 7] = γ[1, 64] = 0`` (padding spins; mid-wave and the first lane of the second
    tile), ``γ_beff`` separate and live, relaxation on, a b1 map.  ``bloch_math.hpp: adj_const_accumulate`` records that
    such a spin once poisoned K3's summed ``γ`` gradient with ``0/0``; the fused CONSTS builds copied that arithmetic.
    Every gradient is finite; ``grad_γ`` at the two spins is the slow-form oracle's ``Σ_t dL/db · B`` -- not zero: CPU dry
    run in fp64, |grad_γ| at the two spins is 0.019, 0.042 (``Mo``), 0.010, 0.079 (trajectory), 0.056, 0.060 (signal) of
    the largest element of ``grad_γ``, which the comparison is scaled by, so a kernel that skipped them (or wrote zeros)
    would miss the fp32 gate of 2e-5 by a factor of 500 and more, the fp64 gate by 1e7 --;
    the summed forms (``T1, T2`` `(N, 1)`, ``dt`` `(1,)`) are not disturbed."""
    gm, gc, (expl, terms) = _check(tag, 'gamma0', 1, 48, None, fn)
    for r in (gm, gc):
        assert all(bool(torch.isfinite(x).all()) for k, x in r.items() if k != 'out'), fn
    want, got = terms['γ'], gc['γ'].detach().double().cpu()
    top = float(want.abs().max())
    for n, s in cases.ZERO_SPINS:
        assert abs(float(want[n, s])) > 100 * TOL[tag] * top, (n, s, float(want[n, s]), top)
        d = record(f'fusedgrads.{tag}.gamma0.{fn}.grad_γ.spin{n}_{s}.over_max', abs(float(got[n, s] - want[n, s])) / top, TOL[tag])
        assert d <= TOL[tag], (n, s, float(got[n, s]), float(want[n, s]))
