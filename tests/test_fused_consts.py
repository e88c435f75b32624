r"""The CONSTS builds of K2b / K2bt / K2bs (``mrphy_blochsim_rfgr_consts_bwd``, ``mrphy_signal_rfgr_consts_bwd``): gradients
of ``fused.blochsim_rfgr``, ``blochsim_rfgr_traj`` and ``signal_rfgr`` w.r.t. ``T1, T2, γ, dt, γ_beff`` (or the entries of
``consts=``) through the fused adjoint -- against the CPU oracle's autograd (``O.rfgr2beff`` + ``O.blochsim_slow``) and
the two-kernel GPU route (``rfgr2beff`` + ``slowsims.blochsim``, which writes ``Beff``, the history and ``grad_Beff``);
the bits of everything the other builds already return; dtype codes; more tiles than persistent waves; the route taken
and the memory it needs; fallbacks; empty problems.

Gates.  The constants' gradients in per-spin and per-batch form (``T1, T2 (N, nM)``, ``γ`` and ``γ_beff`` as separate
`(N, nM)` tensors, ``dt (N, 1)``): relative L2 <= 1e-9 in fp64 and <= 2e-5 in fp32, the gates of
``test_slowsims_blochsim_differentiates_T1_T2_gamma_dt``, under ``constants_on('native')`` as that test sets it (the
oracle differentiates through ``torch.exp``).  The fully summed scalars -- a 0-dim ``γ`` shared with ``γ_beff`` and a
one-entry ``dt``, what ``test_fused_traj._kw`` passes -- are ill-conditioned sums (Σ|g_s| / |Σ g_s| up to 400 on these
operands; the oracle's own fp32 result misses 2e-5 relative by up to 3.4e-5), so for them: shape, dtype and
``|got − want| <= gate · Σ_s|g_s|``, ``want`` and the per-spin ``g_s`` from the oracle in fp64.  ``Mi, rf, gr`` and the maps
keep ``util.assert_close`` (fp64 max-abs 1e-9, fp32 relative L2 1e-5).  Every distance goes to the ledger."""
import collections
import functools

import pytest

from gpu_common import *  # noqa: F401,F403
from mrphy_amd import _lib as L
from mrphy_amd.fused import _signal_composed, _signal_of, _traj_ends
from test_fused_traj import _problem, _weights
from test_signal_mrx import _rxn

pytestmark = pytest.mark.gpu

N, NM = 2, 100
PULSE, MAPS, CONSTS = ('M0', 'rf', 'gr'), ('loc', 'df', 'b1'), ('T1', 'T2', 'γ', 'dt', 'γb')
ALL = PULSE + MAPS + CONSTS
MIX_A, MIX_B = PULSE + CONSTS, ALL
TOL = {'f64': 1e-9, 'f32': 2e-5}
CONSTS_BWD, SIG_CONSTS_BWD, MAPS_BWD = ('mrphy_blochsim_rfgr_consts_bwd', 'mrphy_signal_rfgr_consts_bwd',
                                        'mrphy_blochsim_rfgr_maps_bwd')


def _operands(P, on, needs, form, dtype=None):
    r"""The operands of ``P`` (``test_fused_traj._problem``) on a device, leaves where ``needs`` says.  form 'shared':
    ``γ`` 0-dim and ``γ_beff`` THE SAME tensor (its ``.grad`` is the sum of both), ``dt`` one entry -- what ``_kw`` passes;
    'perspin': ``γ`` and ``γ_beff`` separate `(N, nM)` tensors, ``dt`` `(N, 1)`; 'spinwise': ``dt`` `(N, nM)` as well (the
    oracle only: the per-spin terms of the summed scalars)."""
    cast = (lambda x: x) if dtype is None else (lambda x: x.to(dtype))
    leaf = lambda k, x: None if x is None else on(cast(x)).clone().requires_grad_(k in needs)  # noqa: E731
    n, nM = P['M0'].shape[:2]
    Q = {k: leaf(k, P[k]) for k in PULSE + MAPS + ('T1', 'T2')}
    if form == 'shared':
        Q['γ'], Q['dt'] = leaf('γ', P['γ']), leaf('dt', P['dt'])
        Q['γb'] = Q['γ']
    else:
        Q['γ'], Q['γb'] = leaf('γ', P['γ'].expand(n, nM)), leaf('γb', P['γ'].expand(n, nM))
        Q['dt'] = leaf('dt', P['dt'].expand(n, nM if form == 'spinwise' else 1))
    return Q


def _run(kind, P, on, every=None, needs=ALL, form='shared', sig=None, dtype=None, consts=False):
    r"""``{'out': .., <leaf>: its gradient or None}``.  Loss ``(M·w).sum()``, ``M`` the final state (``every = None``) or
    the trajectory `(N, nM, nRec, 3)`; with ``sig = (rx, terms)`` the signal's ``(sig·w).sum() + (Mo·v).sum()``, ``terms``
    'both' / 'sig' / 'Mo', and ``'out'`` is ``(sig, Mo)``.  kind: 'fused' -- the functions under test; 'two' -- rfgr2beff
    + slowsims.blochsim per record segment over slices of one ``Beff`` (the signal: ``_signal_composed``); 'oracle'.
    ``consts``: hand ``consts=dict(γ2πdt, E1, E2, E1_1)`` leaves over instead of ``T1, T2, γ, dt`` (gradients under the keys
    'g', 'E1', 'E2', 'E1_1'; 'two' is ``sims.blochsim_consts``)."""
    Q = _operands(P, on, needs, form, dtype)
    nT = P['gr'].shape[2]
    ends = [nT] if every is None else _traj_ends(nT, every)
    kw = dict(Δf=Q['df'], b1Map=Q['b1'], γ_beff=Q['γb'], T1=Q['T1'], T2=Q['T2'], γ=Q['γ'], dt=Q['dt'])
    ckeys = CONSTS
    if consts:
        c = sims.relax_constants(Q['T1'], Q['T2'], Q['γ'], Q['dt'], 4, DEV)
        for k, v in zip(('g', 'E1', 'E2', 'E1_1'), c):
            Q[k] = None if v is None else v.detach().to(DEV).clone().requires_grad_(True)
        cd = dict(γ2πdt=Q['g'], E1=Q['E1'], E2=Q['E2'], E1_1=Q['E1_1'])
        kw = dict(Δf=Q['df'], b1Map=Q['b1'], γ_beff=Q['γb'].detach(), consts=cd)
        ckeys = ('g', 'E1', 'E2', 'E1_1')
    if kind == 'fused':
        if sig is not None:
            out = fused.signal_rfgr(Q['M0'], Q['rf'], Q['gr'], Q['loc'], every=every, rx=on(sig[0]), return_Mo=True, **kw)
        elif every is None:
            out = fused.blochsim_rfgr(Q['M0'], Q['rf'], Q['gr'], Q['loc'], **kw)
        else:
            out = fused.blochsim_rfgr_traj(Q['M0'], Q['rf'], Q['gr'], Q['loc'], every=every, **kw)
    elif kind == 'two' and sig is not None:
        out = _signal_composed(Q['M0'], Q['rf'], Q['gr'], Q['loc'], every, on(sig[0]), dict(kw, consts=kw.get('consts')))
    else:
        r2b, step = (O.rfgr2beff, O.blochsim_slow) if kind == 'oracle' else (beffective.rfgr2beff, slowsims.blochsim)
        beff = r2b(Q['rf'], Q['gr'], Q['loc'], Δf=Q['df'], b1Map=Q['b1'], γ=Q['γb'])
        outs, M, t0 = [], Q['M0'], 0
        for e in ends:
            if consts:
                M = sims.blochsim_consts(M, beff[..., t0:e, :], **cd)
            else:
                M = step(M, beff[..., t0:e, :], T1=Q['T1'], T2=Q['T2'], γ=Q['γ'], dt=Q['dt'])
            outs.append(M)
            t0 = e
        out = outs[0] if every is None else torch.stack(outs, dim=-2)
        if sig is not None:
            out = (_signal_of(torch.stack(outs), sig[0]), outs[-1])
    if sig is None:
        (out * on(_weights(tuple(out.shape), out.dtype))).sum().backward()
        res = {'out': out.detach()}
    else:
        s, Mo = out
        loss = 0
        if sig[1] in ('both', 'sig'):
            loss = loss + (s * on(_weights(tuple(s.shape), s.dtype))).sum()
        if sig[1] in ('both', 'Mo'):
            loss = loss + (Mo * on(_weights(tuple(Mo.shape), Mo.dtype)) * 0.5).sum()
        loss.backward()
        res = {'out': (s.detach(), Mo.detach())}
    res.update({k: (None if Q.get(k) is None else Q[k].grad) for k in PULSE + MAPS + ckeys})
    return res


@functools.lru_cache(maxsize=None)
def _oracle(tag, variant, nT, every, form, sig=None, seed=23):
    r"""The oracle's gradients of every operand, once per problem; ``form`` 'perspin' in the data's own dtype, 'spinwise'
    in fp64 (the values rounded to the data's dtype)."""
    P = _problem(tag, variant, nT, seed=seed)
    s = None if sig is None else (None if sig[0] == 0 else _rxn(tag, sig[0]).double() if form == 'spinwise'
                                  else _rxn(tag, sig[0]), sig[1])
    with mrphy_amd.constants_on('native'):
        return _run('oracle', P, lambda x: x, every, form=form, sig=s, dtype=torch.float64 if form == 'spinwise' else None)


def _gate(key, got, want, tag):
    assert got is not None and got.shape == want.shape and got.dtype == want.dtype, (key, got, want.shape)
    d = record(f'fused_consts.{key}', rel_l2(got, want), TOL[tag])
    assert d <= TOL[tag], (key, d)


def _gate_sum(key, got, ref, gs64, tag, like):
    r"""A fully summed scalar: ``|got − ref| <= gate · Σ_s|g_s|`` with the fp64 oracle's per-spin terms ``g_s``."""
    assert got is not None and got.shape == like.shape and got.dtype == like.dtype, (key, got, like.shape)
    scale = float(gs64.abs().sum())
    d = record(f'fused_consts.{key}', abs(float(got.sum()) - float(ref.sum())) / scale, TOL[tag],
               note=f'|got - want| / sum|g_s|; sum|g_s| / |sum g_s| = {scale / max(abs(float(gs64.sum())), 1e-300):.1f}')
    assert d <= TOL[tag], (key, d)


def _check(tag, variant, nT, every, P, needs, got_s, got_p, two_s, two_p, okey, what=''):
    r"""``got_s`` / ``got_p``: the fused results in the 'shared' and the 'perspin' form; against the two-kernel route in the
    same forms and against the oracle."""
    op, o64 = _oracle(tag, variant, nT, every, 'perspin', okey), _oracle(tag, variant, nT, every, 'spinwise', okey)
    relax = P['T1'] is not None
    k0 = f'{what}{tag}.{variant}.nT{nT}.every{every}'
    outs = lambda r: r['out'] if isinstance(r['out'], tuple) else (r['out'],)  # noqa: E731
    for got, two, form in ((got_s, two_s, 'shared'), (got_p, two_p, 'perspin')):
        for a, b, c in zip(outs(got), outs(two), outs(op)):
            assert_close(a, b, tag, f'{k0} output vs two-kernel route')
            assert_close(a, c, tag, f'{k0} output vs oracle')
        for k in PULSE + MAPS:
            if k not in needs or P[k] is None:
                assert got[k] is None, (k, form)
                continue
            assert got[k].shape == P[k].shape and got[k].dtype == P[k].dtype, (k, form)
            assert_close(got[k], two[k], tag, f'{k0} grad {k} vs two-kernel route ({form})')
            assert_close(got[k], op[k], tag, f'{k0} grad {k} vs oracle ({form})')
    for k in ('T1', 'T2'):
        for got, two, form in ((got_s, two_s, 'shared'), (got_p, two_p, 'perspin')):
            if not relax:
                assert got[k] is None
                continue
            _gate(f'{k0}.{k}.{form}.vs_oracle', got[k], op[k], tag)
            _gate(f'{k0}.{k}.{form}.vs_two_kernel', got[k], two[k], tag)
    for k in ('γ', 'γb', 'dt'):                     # per-spin / per-batch forms
        _gate(f'{k0}.{k}.perspin.vs_oracle', got_p[k], op[k], tag)
        _gate(f'{k0}.{k}.perspin.vs_two_kernel', got_p[k], two_p[k], tag)
    # the summed scalars: γ shared with γ_beff, one-entry dt
    g_γ, g_dt = o64['γ'] + o64['γb'], o64['dt']
    for k, gs in (('γ', g_γ), ('dt', g_dt)):
        _gate_sum(f'{k0}.{k}.shared.vs_oracle', got_s[k], gs, gs, tag, P[k])
        _gate_sum(f'{k0}.{k}.shared.vs_two_kernel', got_s[k], two_s[k], gs, tag, P[k])


def _bits(a, b, keys, what):
    for k in keys:
        if b[k] is not None:
            assert a[k] is not None and torch.equal(a[k], b[k]), (what, k)


def _same_out(a, b, what):
    oa, ob = (x['out'] if isinstance(x['out'], tuple) else (x['out'],) for x in (a, b))
    assert all(torch.equal(x, y) for x, y in zip(oa, ob)), what


def _full_check(tag, variant, nT, every):
    P = _problem(tag, variant, nT)
    with mrphy_amd.constants_on('native'):
        res = {(mix, form): _run('fused', P, dev, every, needs=needs, form=form)
               for mix, needs in (('A', MIX_A), ('B', MIX_B)) for form in ('shared', 'perspin')}
        two = {form: _run('two', P, dev, every, form=form) for form in ('shared', 'perspin')}
        assert P['T1'] is None or res['A', 'shared']['T1'] is not None, 'T1.grad is None: no gradient w.r.t. the constants'
        for mix, needs in (('A', MIX_A), ('B', MIX_B)):
            _check(tag, variant, nT, every, P, needs, res[mix, 'shared'], res[mix, 'perspin'], two['shared'], two['perspin'],
                   None, what=f'mix{mix}.')
        full = res['B', 'shared']
        pulse = _run('fused', P, dev, every, needs=PULSE)
        _same_out(full, pulse, 'the output changed with the constants\' gradients')
        _same_out(res['A', 'perspin'], pulse, 'the output changed with the constants\' gradients (per-spin forms)')
        assert all(pulse[k] is None for k in MAPS + CONSTS)
        if P['T1'] is None:
            assert full['T1'] is None and full['T2'] is None and full['γ'] is not None and full['dt'] is not None
        if nT % 16 == 0:
            _bits(full, pulse, PULSE, 'pulse gradients: the plain K2b')
            _bits(res['A', 'shared'], pulse, PULSE, 'pulse gradients: the plain K2b (mix A)')
            _bits(full, _run('fused', P, dev, every, needs=PULSE + MAPS), PULSE + MAPS, 'map gradients: the MAPS build')
            _bits(full, res['A', 'shared'], CONSTS, 'the constants with and without the maps')
            for k in ('T1', 'T2', 'γ', 'dt', 'γb'):
                if P.get(k, 0) is None:
                    continue
                one = _run('fused', P, dev, every, needs=(k,), form='perspin')
                assert all(one[j] is None for j in ALL if j != k), k
                assert torch.equal(one[k], res['B', 'perspin'][k]), k
        _bits(_run('fused', P, dev, every), full, ALL, 'twice')


# =============================================================================================
# 1. blochsim_rfgr
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('variant', ['plain', 'b1map', 'norelax', 'plain_batch1_pulse'])
@pytest.mark.parametrize('nT', [16, 48, 50])
def test_consts_gradients(tag, variant, nT):
    r"""Loss (Mo·w).sum().  Mix A: Mi, rf, gr, T1, T2, γ, dt, γ_beff require grad; mix B: loc, Δf, b1Map as well.  Every
    gradient against both yardsticks (module docstring); ``Mo`` is the bits of the call with the constants detached; with
    whole segments grad_Mi / rf / gr are the bits of the plain K2b, the map gradients the bits of the MAPS build, each
    constant alone the bits it has in the full set; twice the same bits; without relaxation ``T1`` / ``T2`` are absent
    and ``γ``, ``dt`` still get gradients.  nT = 50: fused part + composed tail.  Fails without the CONSTS builds:
    ``T1.grad is None``."""
    _full_check(tag, variant, nT, None)


# =============================================================================================
# 2. trajectory
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('variant', ['b1map', 'plain'])
@pytest.mark.parametrize('nT,every', [(48, 1), (48, 3), (48, 16), (48, 40), (48, 48), (50, 3)])
def test_consts_trajectory_gradients(tag, variant, nT, every):
    r"""Loss (Mt·w).sum(): modes 1 (every < 16) and 2, records on and off the segment boundaries, one record, the split;
    the assertions of ``test_consts_gradients``."""
    _full_check(tag, variant, nT, every)


# =============================================================================================
# 3. signal
# =============================================================================================
def _cap(tag):
    return int(mrphy_amd.require_library().mrphy_signal_rfgr_max_rx(L.F64 if tag == 'f64' else L.F32))


SIG_NEEDS = PULSE + ('T1', 'T2', 'dt')


@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('nrx', [0, 1, 3, 'cap+1'])
@pytest.mark.parametrize('nT,every', [(48, 1), (48, 3), (48, 16), (48, 40), (48, 48), (50, 3)])
def test_consts_signal_gradients(tag, nrx, nT, every, monkeypatch):
    r"""``signal_rfgr`` with a b1 map, ``rx`` None / 1 / 3 / max_rx + 1 coils, loss (sig·w).sum() + (Mo·v).sum() and each
    term alone; Mi, rf, gr, T1, T2, dt require grad (a ``γ`` shared with ``γ_beff`` beside a ``Δf`` is a map gradient: the
    composed route).  Against ``_signal_composed`` and the oracle; ``sig`` and ``Mo`` are the bits of the call without the
    constants' gradients, and with whole segments grad_Mi / rf / gr the bits of ``mrphy_signal_rfgr(_mrx)_bwd``."""
    nrx = _cap(tag) + 1 if nrx == 'cap+1' else nrx
    P = _problem(tag, 'b1map', nT)
    rx = None if nrx == 0 else _rxn(tag, nrx)
    calls = _counted(monkeypatch)
    with mrphy_amd.constants_on('native'):
        for terms in ('both', 'sig', 'Mo'):
            calls.clear()
            got_s, got_p = (_run('fused', P, dev, every, needs=SIG_NEEDS, form=f, sig=(rx, terms)) for f in ('shared', 'perspin'))
            if nT % 16 == 0:
                blocks = 1 if terms == 'Mo' else max(1, -(-nrx // _cap(tag)))      # (Mo is the first block's)
                assert calls[SIG_CONSTS_BWD] == 2 * blocks and not any(calls[n] for n in COMPOSED), dict(calls)
            two_s, two_p = (_run('two', P, dev, every, needs=SIG_NEEDS, form=f, sig=(rx, terms)) for f in ('shared', 'perspin'))
            pulse = _run('fused', P, dev, every, needs=PULSE, sig=(rx, terms))
            _same_out(got_s, pulse, 'sig, Mo changed with the constants\' gradients')
            if nT % 16 == 0:
                _bits(got_s, pulse, PULSE, 'pulse gradients: mrphy_signal_rfgr(_mrx)_bwd')
            op, o64 = (_oracle(tag, 'b1map', nT, every, f, (nrx, terms)) for f in ('perspin', 'spinwise'))
            k0 = f'signal.{tag}.rx{nrx}.{terms}.nT{nT}.every{every}'
            for got, two in ((got_s, two_s), (got_p, two_p)):
                for a, b, c in zip(got['out'], two['out'], op['out']):
                    assert_close(a, b, tag, f'{k0} output vs composed')
                    assert_close(a, c, tag, f'{k0} output vs oracle')
                for k in PULSE:
                    assert_close(got[k], two[k], tag, f'{k0} grad {k} vs composed')
                    assert_close(got[k], op[k], tag, f'{k0} grad {k} vs oracle')
                for k in ('T1', 'T2'):
                    _gate(f'{k0}.{k}.vs_oracle', got[k], op[k], tag)
                    _gate(f'{k0}.{k}.vs_composed', got[k], two[k], tag)
                assert got['γ'] is None and got['γb'] is None
            _gate(f'{k0}.dt.perbatch.vs_oracle', got_p['dt'], op['dt'], tag)
            _gate(f'{k0}.dt.perbatch.vs_composed', got_p['dt'], two_p['dt'], tag)
            _gate_sum(f'{k0}.dt.shared.vs_oracle', got_s['dt'], o64['dt'], o64['dt'], tag, P['dt'])
            _gate_sum(f'{k0}.dt.shared.vs_composed', got_s['dt'], two_s['dt'], o64['dt'], tag, P['dt'])


# =============================================================================================
# 4. consts= dict
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('variant', ['b1map', 'norelax'])
@pytest.mark.parametrize('every', [None, 5, 16])
def test_consts_dict_gradients(tag, variant, every):
    r"""``consts=dict(γ2πdt, E1, E2, E1_1)`` with every entry requiring grad: the gradients equal those of
    ``sims.blochsim_consts`` on ``rfgr2beff`` (K3's GC builds) under the gates, ``Mi, rf, gr`` under ``assert_close``."""
    P = _problem(tag, variant, 48, seed=31)
    got = _run('fused', P, dev, every, needs=PULSE, consts=True)
    two = _run('two', P, dev, every, needs=PULSE, consts=True)
    _same_out(got, _run('fused', P, dev, every, needs=PULSE), 'the output changed with consts=')
    for k in PULSE:
        assert_close(got[k], two[k], tag, f'grad {k} vs blochsim_consts')
    for k in ('g', 'E1', 'E2', 'E1_1'):
        if variant == 'norelax' and k != 'g':
            assert got[k] is None
            continue
        _gate(f'dict.{tag}.{variant}.every{every}.{k}.vs_blochsim_consts', got[k], two[k], tag)


# =============================================================================================
# 5. dtype codes
# =============================================================================================
@pytest.mark.parametrize('mode,wide', [('fast', False), ('fast', True), ('precise', False), ('precise', True)])
@pytest.mark.parametrize('every', [5, 16])
def test_consts_gradients_dtype_codes(mode, wide, every):
    r"""fp32 data through dtype codes 0 / 2 (fast) and 3 / 4 (precise: the sweep carries t = E h, which the constants'
    sums take as it is and divide out once), with relaxation and a b1 map, per-spin forms, against the two-kernel route
    in the same mode; code 3 also against the oracle.  A missing or doubled E shows at order 1."""
    from mrphy_amd import _host
    P = _problem('f32', 'b1map', 48, seed=5)
    if wide:
        P['T1'], P['T2'], P['γ'], P['dt'] = (P[k].double() for k in ('T1', 'T2', 'γ', 'dt'))
    keys = ('T1', 'T2', 'γ', 'γb', 'dt')
    with mrphy_amd.precision(mode), mrphy_amd.constants_on('native'):
        code = _host.dtype_code(torch.float32, torch.float64 if wide else torch.float32)
        assert code == {('fast', False): 0, ('fast', True): 2, ('precise', False): 3, ('precise', True): 4}[mode, wide]
        got = _run('fused', P, dev, every, form='perspin')
        two = _run('two', P, dev, every, form='perspin')
        for k in PULSE + MAPS:
            assert_close(got[k], two[k], 'f32', f'grad {k} vs two-kernel route (code {code})')
        for k in keys:
            _gate(f'code{code}.every{every}.{k}.vs_two_kernel', got[k].float(), two[k].float(), 'f32')
            assert got[k].dtype == P['T1'].dtype
        if code == 3:
            op = _oracle('f32', 'b1map', 48, every, 'perspin', None, 5)
            for k in keys:
                _gate(f'code3.every{every}.{k}.vs_oracle', got[k], op[k], 'f32')


# =============================================================================================
# 6. more tiles than persistent waves
# =============================================================================================
def test_consts_second_tile_per_wave():
    r"""N = 1, nM = 2048·64 + 100, nT = 32, fp32, per-spin ``T1, T2, γ``: wave 0 takes tile 0 and then the last, ragged one
    -- the sums are reset and the outputs written per tile.  Against the two-kernel route, relative L2 <= 2e-5, over all
    spins and over the first and the last tile separately; twice the same bits."""
    nM, nT = 2048 * 64 + 100, 32
    P = _problem('f32', 'b1map', nT, N=1, nM=nM)
    needs = ('T1', 'T2', 'γ')
    got = _run('fused', P, dev, needs=needs, form='perspin')
    two = _run('two', P, dev, needs=needs, form='perspin')
    for k in needs:
        for name, sl in (('all', slice(None)), ('first_tile', slice(0, 64)), ('last_tile', slice(2048 * 64, nM))):
            _gate(f'tiles2048.{k}.{name}.vs_two_kernel', got[k][:, sl], two[k][:, sl], 'f32')
    _bits(_run('fused', P, dev, needs=needs, form='perspin'), got, needs, 'twice')


# =============================================================================================
# 7. the route taken
# =============================================================================================
OLD_BWD = ('mrphy_blochsim_rfgr_bwd', 'mrphy_blochsim_rfgr_traj_bwd', 'mrphy_signal_rfgr_bwd', 'mrphy_signal_rfgr_mrx_bwd')
NEW_BWD = (CONSTS_BWD, SIG_CONSTS_BWD)
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
    for name in NEW_BWD + (MAPS_BWD,) + OLD_BWD + COMPOSED:
        monkeypatch.setattr(lib, name, wrap(name, getattr(lib, name)))
    return calls


def test_consts_gradient_is_one_fused_launch(monkeypatch):
    r"""nT = 48 with ``T1`` requiring grad: each of the three functions calls its new entry point exactly once and neither
    K0 nor the blochsim forward; with only ``rf`` requiring grad each calls exactly what it called before."""
    P = _problem('f32', 'b1map', 48)
    assert len(COMPOSED) >= 4
    calls = _counted(monkeypatch)
    rx3 = _rxn('f32', 3)
    for every, sig, new, old in ((None, None, CONSTS_BWD, OLD_BWD[0]), (5, None, CONSTS_BWD, OLD_BWD[1]),
                                 (5, (None, 'both'), SIG_CONSTS_BWD, OLD_BWD[2]), (5, (rx3, 'both'), SIG_CONSTS_BWD, OLD_BWD[3])):
        calls.clear()
        g = _run('fused', P, dev, every, needs=('T1',), sig=sig)
        assert g['T1'] is not None and calls[new] == 1 and sum(calls.values()) == 1, (every, dict(calls))
        calls.clear()
        _run('fused', P, dev, every, needs=('rf',), sig=sig)
        assert calls[old] == 1 and sum(calls.values()) == 1, (every, dict(calls))


@pytest.mark.parametrize('case', ['ptx4', 'nT8'])
def test_consts_fallbacks_stay_composed(case, monkeypatch):
    r"""A 4-coil parallel-transmit case and nT = 8 (no whole segment) never call the new entry points and still give the
    constants' gradients, which match the oracle."""
    tag = 'f32'
    variant, nT = ('ptx4', 48) if case == 'ptx4' else ('b1map', 8)
    P = _problem(tag, variant, nT, seed=77)
    needs = PULSE + ('T1', 'T2', 'γ', 'γb', 'dt')
    calls = _counted(monkeypatch)
    with mrphy_amd.constants_on('native'):
        for every in (None, 5):
            calls.clear()
            got = _run('fused', P, dev, every, needs=needs, form='perspin')
            assert not any(calls[n] for n in NEW_BWD) and calls['mrphy_rfgr2beff_st'] >= 1, (case, dict(calls))
            op = _run('oracle', P, lambda x: x, every, needs=needs, form='perspin')
            assert_close(got['out'], op['out'], tag, f'{case} output vs oracle')
            for k in PULSE:
                assert_close(got[k], op[k], tag, f'{case} grad {k} vs oracle')
            for k in ('T1', 'T2', 'γ', 'γb', 'dt'):
                _gate(f'fallback.{case}.every{every}.{k}.vs_oracle', got[k], op[k], tag)


# =============================================================================================
# 8. memory
# =============================================================================================
def test_consts_gradients_materialise_no_beff():
    r"""N = 1, nM = 4096, nT = 256, fp32, ``T1``, ``T2`` and ``rf`` requiring grad, forward + backward: the allocator's peak
    rises by less than a quarter of ``Beff``'s bytes (nM·nT·12) -- ``test_maps_gradients_materialise_no_beff``'s bound: the
    checkpoints are 1/16 of them and the per-spin outputs <= 10 / (3 nT) of them; the two-kernel route holds Beff, the
    history and grad_Beff."""
    nM, nT = 4096, 256
    P = _problem('f32', 'b1map', nT, N=1, nM=nM)
    Q = _operands(P, dev, ('rf', 'T1', 'T2'), 'shared')
    kw = dict(Δf=Q['df'], b1Map=Q['b1'], γ_beff=Q['γb'], T1=Q['T1'], T2=Q['T2'], γ=Q['γ'], dt=Q['dt'])
    beff_bytes = nM * nT * 12
    leaves = (Q['rf'], Q['T1'], Q['T2'])

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
        b = beffective.rfgr2beff(Q['rf'], Q['gr'], Q['loc'], Δf=Q['df'], b1Map=Q['b1'], γ=Q['γb'])
        return slowsims.blochsim(Q['M0'], b, T1=Q['T1'], T2=Q['T2'], γ=Q['γ'], dt=Q['dt'])
    fused_rise, g = rise(lambda: fused.blochsim_rfgr(Q['M0'], Q['rf'], Q['gr'], Q['loc'], **kw))
    two_rise, g2 = rise(two)
    record('fused_consts.mem.rise_over_beff', fused_rise / beff_bytes, 0.25,
           note=f'fused {fused_rise} B, two-kernel route {two_rise} B, Beff {beff_bytes} B')
    assert fused_rise < 0.25 * beff_bytes, (fused_rise, beff_bytes)
    assert two_rise > 2 * beff_bytes, (two_rise, beff_bytes)
    assert_close(g[0], g2[0], 'f32', 'grad_rf')
    for a, b, nm in zip(g[1:], g2[1:], ('T1', 'T2')):
        _gate(f'mem.{nm}.vs_two_kernel', a, b, 'f32')


# =============================================================================================
# 9. empty problems
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('empty', ['nT', 'nM'])
def test_consts_empty_problem(tag, empty):
    r"""No step (nT = 0) or no spin (nM = 0) with the constants' gradients wanted: the backward runs, and the gradients
    are zeros of the operands' shapes and dtypes -- in the three functions."""
    nT, nM, every = (0, 100, 3) if empty == 'nT' else (32, 0, 5)
    P = _problem(tag, 'b1map', 32, nM=nM)
    P['rf'], P['gr'] = P['rf'][:, :, :nT], P['gr'][:, :, :nT]
    rx = _rxn(tag, 3, nM=nM)
    for ev, sig in ((None, None), (every, None), (every, (None, 'both')), (every, (rx, 'both'))):
        for form in ('shared', 'perspin'):
            keys = ('T1', 'T2', 'dt') + (() if sig else ('γ',))
            got = _run('fused', P, dev, ev, needs=PULSE + keys, form=form, sig=sig)
            Q = _operands(P, lambda x: x, (), form)
            for k in keys:
                assert got[k] is not None and got[k].shape == Q[k].shape and got[k].dtype == Q[k].dtype, (k, ev, form)
                assert bool((got[k] == 0).all()), (k, ev, form)
