r"""The fused kernels (K2, K2b, the pTx K2b, the trajectory builds) on every operand form the host code accepts -- broadcast
shapes, 0-dim and stride-0 operands, a general ``*Nd`` grid, views, unaligned buffers (``cases.fused_operand_variants``) --
on steps of exactly zero field (``cases.zero_field_case``) and at the batch-size limit ``N = 65535``.

Four invariants per case: (1) a spelling changes no bit -- the operands as given against the same numbers materialised
over ``(N, nM)``; (2) fused == rfgr2beff + blochsim (``Mo`` and ``grad_Mi`` bit for bit; at a split length in precise
fp32, ``grad_Mi`` against the two-kernel route cut at the same step, see ``_invariants``); (3) both within the project's gates
(``tests/util.py``) of the CPU oracle on the operands as given, and of the reference's own recorded outputs
(``golden/fusedops_*.npz``) where the reference accepts the form; (4) a second run gives the same bits.  ``precision('fast')`` is held to (1), (2) and (4); its
distance to the oracle goes to the ledger (``fusedops.*``) -- the project has no small-problem bound for it.
``fused.signal_rfgr`` on the same cases, each with a receive map: ``test_signal_operands.py``.
"""
import pytest

from gpu_common import *  # noqa: F401,F403
from mrphy_amd.fused import _traj_ends

pytestmark = pytest.mark.gpu

MODES = [('f64', 'precise'), ('f32', 'precise'), ('f32', 'fast')]
VARIANTS = ['compact_mixed', 'scalars', 'expanded', 'cube', 'cube_planes', 'gamma_split', 'views', 'offset']
NAMES = ('out', 'grad_Mi', 'grad_rf', 'grad_gr')
EVERY = 5


def _cotangent(v, every, nT):
    r"""The loss cotangent: ``w`` as given for ``Mo``; for the trajectory ``w`` times a factor per record."""
    if every is None:
        return v['w']
    nRec = len(_traj_ends(nT, every))
    c = torch.cos(torch.arange(nRec, dtype=torch.float64) * 0.7 + 0.3).to(v['w'].dtype)
    return v['w'].unsqueeze(-2) * c[:, None]


def _run(route, v, every=None, consts=None, sim=None, cut=None, cot=None):
    r"""``out, grad_Mi, grad_rf, grad_gr`` of ``<cotangent, out>``; ``out`` is ``Mo`` (``every = None``) or the trajectory
    `(N, *Nd, nRec, 3)`.  ``route``: 'fused' (``fused.blochsim_rfgr[_traj]``), 'two' (``rfgr2beff`` + ``sims.blochsim``,
    one call per record segment for a trajectory; with ``cut``, ``Mo`` by two such calls, steps ``[0, cut)`` and
    ``[cut, nT)``) or 'oracle' (the same composition on the CPU).  ``cot``: the cotangent of ``out`` in place of
    :func:`_cotangent` (CPU; ``test_signal_operands.py``).  The operands go in AS GIVEN: ``place`` keeps their
    strides and offsets, and the leaves are detached aliases, not copies."""
    on = (lambda x: x) if route == 'oracle' else place
    leaf = lambda x: on(x).detach().requires_grad_(True)  # noqa: E731
    Mi, rf, gr = leaf(v['M0']), leaf(v['rf']), leaf(v['gr'])
    nT = rf.shape[2]
    loc, pk = on(v['loc']), dict(Δf=on(v['Δf']), b1Map=on(v['b1Map']))
    rk = dict(T1=on(v['T1']), T2=on(v['T2']), γ=on(v['γ']), dt=on(v['dt']))
    if route == 'fused':
        ck = dict(consts=consts) if consts is not None else rk
        out = (fused.blochsim_rfgr(Mi, rf, gr, loc, γ_beff=on(v['γ_beff']), **pk, **ck) if every is None else
               fused.blochsim_rfgr_traj(Mi, rf, gr, loc, every=every, γ_beff=on(v['γ_beff']), **pk, **ck))
    else:
        if route == 'oracle':
            mk, step = O.rfgr2beff, lambda M, b: O.blochsim(M, b, **rk)                            # noqa: E731
        elif consts is not None:
            mk, step = beffective.rfgr2beff, lambda M, b: sims.blochsim_consts(M, b, **consts)     # noqa: E731
        else:
            mk, step = beffective.rfgr2beff, lambda M, b: (sim or sims.blochsim)(M, b, **rk)       # noqa: E731
        beff = mk(rf, gr, loc, γ=on(v['γ_beff']), **pk)
        if every is None and cut is not None:
            out = step(step(Mi, beff[..., :cut, :]), beff[..., cut:, :])
        elif every is None:
            out = step(Mi, beff)
        else:
            recs, M, t0 = [], Mi, 0
            for e in _traj_ends(nT, every):
                M = step(M, beff[..., t0:e, :])
                recs.append(M)
                t0 = e
            out = torch.stack(recs, dim=-2)
    torch.autograd.backward([out], [on(_cotangent(v, every, nT) if cot is None else cot)])
    return dict(out=out.detach(), grad_Mi=Mi.grad, grad_rf=rf.grad, grad_gr=gr.grad)


def _same_bits(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert max_abs(a, b) == 0.0, f'{what}: differs by {max_abs(a, b):.3e}'


def _invariants(v, tag, mode, every, key, dense=None, zero=None):
    r"""Invariants (1)-(4) of the module docstring for one case and one entry point; returns the fused results.
    ``zero``: `(N, nT)` mask of the zero-field steps -- the pulse gradients are compared on those steps alone as well, so
    that a wrong value there is not diluted by the live ones."""
    fu = _run('fused', v, every)
    for k in NAMES:
        assert bool(torch.isfinite(fu[k]).all()), (key, k)
    if dense is not None:                                                      # (1) the spelling changes nothing
        fd = _run('fused', dense, every)
        flat = (lambda x: x.reshape(fd['out'].shape))
        _same_bits(flat(fu['out']), fd['out'], f'{key}: out, as given vs dense')
        _same_bits(fu['grad_Mi'].reshape(fd['grad_Mi'].shape), fd['grad_Mi'], f'{key}: grad_Mi, as given vs dense')
        for k in ('grad_rf', 'grad_gr'):
            if fu[k].shape == fd[k].shape:
                _same_bits(fu[k], fd[k], f'{key}: {k}, as given vs dense')
            else:                                                              # a batch-1 pulse, expanded in `dense`
                assert_close(fu[k], fd[k].sum(0, keepdim=True), tag, f'{key}: {k} vs dense summed over N')
    two = _run('two', v, every)                                                # (2) fused == two-kernel
    _same_bits(fu['out'], two['out'], f'{key}: out, fused vs two-kernel')
    if every is None:
        nT = v['rf'].shape[2]
        n1 = nT - nT % 16
        if n1 != nT and tag == 'f32' and mode == 'precise':
            # A split length in the precise fp32 build: that adjoint carries t = E h (bloch_math.hpp: AdjMode) and
            # divides E out once where a sweep ends.  The split route ends one sweep at step n1 and begins another
            # (h / E, then E (h / E)), one sweep over all nT steps does not: the same number, one more rounding.  So
            # the bits are those of the two-kernel route cut at the same step, and one sweep is held to the gate below.
            cut = _run('two', v, cut=n1)
            _same_bits(fu['out'], cut['out'], f'{key}: out, fused vs two-kernel cut at {n1}')
            _same_bits(fu['grad_Mi'], cut['grad_Mi'], f'{key}: grad_Mi, fused vs two-kernel cut at {n1}')
        else:
            _same_bits(fu['grad_Mi'], two['grad_Mi'], f'{key}: grad_Mi, fused vs two-kernel')
    for k in NAMES[1:]:
        # (the trajectory's grad_Mi too: the precise K2bt carries t = E h and takes a record's cotangent in scaled by E,
        # autograd over the segment loop adds it to h -- the same number, another rounding)
        assert_close(fu[k], two[k], tag, f'{key}: {k}, fused vs two-kernel')
    ora = _run('oracle', v, every)                                             # (3) the yardstick
    sl = lambda x: x.movedim(2, 1)[zero.to(x.device)]                          # noqa: E731
    for route, got in (('fused', fu), ('two', two)):
        for k in NAMES:
            assert got[k].shape == ora[k].shape, (key, route, k)
            if mode == 'precise':
                assert_close(got[k], ora[k], tag, f'{key}: {route} {k} vs oracle')
        if zero is not None and mode == 'precise':
            for k in ('grad_rf', 'grad_gr'):
                assert_close(sl(got[k]), sl(ora[k]), tag, f'{key}: {route} {k} on the zero-field steps vs oracle')
                seg = list(cases.ZERO_SEGMENT)
                assert_close(got[k][1, :, seg], ora[k][1, :, seg], tag, f'{key}: {route} {k} on the all-zero segment')
    if mode == 'fast':
        record(f'fusedops.{key}.fast.{"Mo" if every is None else "traj"}.worst_rel_l2_vs_oracle',
               max(rel_l2(fu[k], ora[k]) for k in NAMES), note='largest of out, grad_Mi, grad_rf, grad_gr; not asserted')
        if zero is not None:
            record(f'fusedops.{key}.fast.{"Mo" if every is None else "traj"}.zero_steps.worst_rel_l2_vs_oracle',
                   max(rel_l2(sl(fu[k]), sl(ora[k])) for k in ('grad_rf', 'grad_gr')), note='not asserted')
    again = _run('fused', v, every)                                            # (4) determinism
    for k in NAMES:
        _same_bits(fu[k], again[k], f'{key}: {k}, second run')
    return fu


def _against_golden(v, tag, key):
    r"""Both HIP routes with the constants of the reference's run against what the reference gave (where it gave
    anything: ``make_golden.py: fusedops_reference``)."""
    G = golden(f'fusedops_{tag}')
    if f'{key}.Mo' not in G:
        assert '.cube' in key and not key.startswith('c0.'), key      # b1Map on a general *Nd grid: IndexError there
        return
    for route in ('fused', 'two'):
        got = _run(route, v, consts=gconsts(G, f'{key}.'))
        for k, gk in (('out', 'Mo'), ('grad_Mi', 'grad_Mi'), ('grad_rf', 'grad_rf'), ('grad_gr', 'grad_gr')):
            if f'{key}.{gk}' in G:
                assert_close(got[k], G[f'{key}.{gk}'], tag, f'{key}: {route} {gk} vs the reference')


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('nC', cases.FUSED_COILS)
@pytest.mark.parametrize('name,nT', [(n, 48) for n in VARIANTS] + [(n, 53) for n in cases.FUSED_NT53])
def test_operand_spellings(tag, mode, nC, name, nT):
    r"""One problem, many spellings (module docstring); nT = 48: three checkpoint segments through the fused adjoint,
    nT = 53: the fused part plus five composed steps."""
    given, dense = cases.fused_operand_variants(DT[tag], nC, nT)[name]
    key = f'c{nC}.nT{nT}.{name}'
    if name == 'views':        # the forms under test arrive as such
        assert not any(place(given[k]).is_contiguous() for k in ('M0', 'loc', 'Δf', 'rf', 'gr', 'w'))
    if name == 'offset':
        assert all(place(given[k]).is_contiguous() and place(given[k]).data_ptr() % 16 != 0
                   for k in ('M0', 'loc', 'rf', 'gr', 'w'))
    if name == 'expanded':
        assert all(0 in place(given[k]).stride() for k in ('loc', 'Δf', 'γ_beff', 'T1', 'T2', 'γ'))
    with mrphy_amd.precision(mode):
        Mo = _invariants(given, tag, mode, None, key, dense)
        Mt = _invariants(given, tag, mode, EVERY, key, dense)
        _same_bits(Mt['out'][..., -1, :], Mo['out'], f'{key}: last record vs blochsim_rfgr')
        if name == 'gamma_split':
            # the same problem through consts=: the constants formed in their broadcast shapes, as the host forms them
            c = {k: x.to(DEV) for k, x in cases.reference_constants(
                given['T1'], given['T2'], given['γ'], given['dt'], given['loc'].ndim + 1).items()}
            for route in ('fused', 'two'):
                got, want = _run(route, given, consts=c), _run(route, given)
                for k in NAMES:
                    _same_bits(got[k], want[k], f'{key}: {route} {k}, consts= vs T1, T2, γ, dt')
        if mode == 'precise':
            _against_golden(given, tag, key)


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('nC', cases.FUSED_COILS)
@pytest.mark.parametrize('nT', [48, 53])
def test_zero_field_steps(tag, mode, nC, nT):
    r"""Dead time and spins at the iso-centre through K2b, the pTx K2b and K2bt (``every`` 1, 5: per-step injection; 16:
    per-segment), nT = 53 through the split route.  The yardstick is the explicit adjoint, the analytic limit
    ``-γ2πdt (m x h̃)`` at zero field (``test_oracle_golden.py::test_zero_field_adjoint_yardsticks_agree``: finite
    differences confirm it; autograd through the reference's ``slowsims`` form returns 0 there).  The pulse gradients
    are held to the gates on the zero-field steps alone, and on batch entry 1's all-zero segment alone, too."""
    v, zero = cases.zero_field_case(DT[tag], nC, nT)
    key = f'c{nC}.nT{nT}.zero_field'
    with mrphy_amd.precision(mode):
        Mo = _invariants(v, tag, mode, None, key, zero=zero)
        for every in (1, EVERY, 16):
            Mt = _invariants(v, tag, mode, every, key, zero=zero)
            _same_bits(Mt['out'][..., -1, :], Mo['out'], f'{key}: last record (every={every}) vs blochsim_rfgr')
        if nC:      # b1Map = 0 and loc = 0: that spin only relaxes -- nT times  Mxy *= E2, Mz = Mz E1 - (E1 - 1)
            c = cases.reference_constants(v['T1'], v['T2'], v['γ'], v['dt'], 4)
            e1, e2, e1m1 = (float(c[k][1, 64, 0, 0]) for k in ('E1', 'E2', 'E1_1'))
            m = v['M0'][1, 64].double().clone()
            for _ in range(nT):
                m = torch.stack((m[0] * e2, m[1] * e2, m[2] * e1 - e1m1))
            assert_close(Mo['out'][1, 64], m, tag, 'the spin that never rotates: pure relaxation')
        # the product's slowsims.blochsim follows sims (the analytic values), not the reference's autograd zeros
        ora, slow = _run('oracle', v), _run('two', v, sim=slowsims.blochsim)
        if mode == 'precise':
            for k in NAMES:
                assert_close(slow[k], ora[k], tag, f'{key}: slowsims.blochsim {k} vs oracle')
            for k in ('grad_rf', 'grad_gr'):
                assert_close(slow[k].movedim(2, 1)[zero.to(DEV)], ora[k].movedim(2, 1)[zero], tag,
                             f'{key}: slowsims.blochsim {k} on the zero-field steps')
                assert float(ora[k].movedim(2, 1)[zero].abs().max()) > 0.1          # O(1): nothing like zero
            _against_golden(v, tag, key)


# ---------------------------------------------------------------------------------------------
# The batch-size limit N <= 65535 (a grid dimension of K0, K2, K2b and the mask kernels)
# ---------------------------------------------------------------------------------------------
def _batch_problem(N, dtype, nT=16):
    gen = torch.Generator().manual_seed(57)
    u = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64)         # noqa: E731
    c = lambda x: x.to(dtype)                                                 # noqa: E731
    return dict(M0=c(u(N, 1, 3) * 2 - 1), rf=c((u(N, 2, nT) * 2 - 1) * 3), gr=c(u(N, 3, nT) * 2 - 1),
                loc=c((u(N, 1, 3) * 2 - 1) * 6), Δf=c((u(N, 1) * 2 - 1) * 200), b1Map=None,
                γ_beff=torch.tensor(cases.γH_val, dtype=dtype), T1=c(0.5 + u(N, 1)), T2=c(0.02 + 0.1 * u(N, 1)),
                γ=torch.tensor(cases.γH_val, dtype=dtype), dt=torch.tensor([cases.dt0_val], dtype=dtype),
                w=c(u(N, 1, 3) * 2 - 1))


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_batch_size_limit_65535(tag):
    r"""``N = 65535`` (the largest batch the grids take), one spin each, one checkpoint segment: forward and gradients
    through both routes against the oracle."""
    v = _batch_problem(65535, DT[tag])
    fu, two, ora = _run('fused', v), _run('two', v), _run('oracle', v)
    _same_bits(fu['out'], two['out'], 'Mo, fused vs two-kernel')
    _same_bits(fu['grad_Mi'], two['grad_Mi'], 'grad_Mi, fused vs two-kernel')
    for route, got in (('fused', fu), ('two', two)):
        for k in NAMES:
            assert got[k].shape == ora[k].shape, (route, k)
            assert_close(got[k], ora[k], tag, f'N = 65535: {route} {k} vs oracle')
            # ... and entry by entry (the project's elementwise gate for pulse gradients, tests/util.py): one batch
            # entry's gradient is a few numbers among 65535 times as many, which a norm over all of them would hide
            if tag == 'f32' and k in ('grad_rf', 'grad_gr'):
                elementwise(f'fusedops.N65535.{route}.{k}', got[k], ora[k], ELEM32_GRAD, scale=True, comp_axis=1)


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_batch_size_beyond_limit_is_refused_before_any_launch(tag):
    r"""``N = 65536``: ``fused.blochsim_rfgr`` and ``rfgr2beff`` raise the library's ``RuntimeError`` naming the entry
    point; through the C ABI the call returns MRPHY_EINVAL with its output buffer untouched (nothing was launched); the
    process then passes a normal call."""
    from mrphy_amd import _host
    lib = mrphy_amd.require_library()
    v = {k: (place(x) if isinstance(x, torch.Tensor) else x) for k, x in _batch_problem(65536, DT[tag]).items()}
    kw = dict(Δf=v['Δf'], γ_beff=v['γ_beff'], T1=v['T1'], T2=v['T2'], γ=v['γ'], dt=v['dt'])
    with pytest.raises(RuntimeError, match='mrphy_blochsim_rfgr_fwd.*invalid argument'):
        fused.blochsim_rfgr(v['M0'], v['rf'], v['gr'], v['loc'], **kw)
    with pytest.raises(RuntimeError, match='mrphy_blochsim_rfgr_fwd.*invalid argument'):
        fused.blochsim_rfgr(v['M0'], v['rf'].requires_grad_(True), v['gr'], v['loc'], **kw)
    v['rf'].requires_grad_(False)
    with pytest.raises(RuntimeError, match='mrphy_rfgr2beff.*invalid argument'):
        beffective.rfgr2beff(v['rf'], v['gr'], v['loc'], Δf=v['Δf'], γ=v['γ_beff'])
    # the C ABI: EINVAL, and not one element of the outputs written
    P = beffective._PulseOnSpins(v['rf'], v['gr'], v['loc'], v['Δf'], None, v['γ_beff'])
    g, E1, E2, E1_1 = sims.relax_constants(v['T1'], v['T2'], v['γ'], v['dt'], 4, DEV)
    code, bg, e1, e2, e1m1 = sims._prep_constants(g, E1, E2, E1_1, P.N, P.Nd, DT[tag], DEV)
    Mo = torch.full_like(v['M0'], float('nan'))
    Mck = torch.full((1, P.N * P.nM, 3), float('nan'), dtype=DT[tag], device=DEV)
    beff = torch.full((P.N, 1, P.nT, 3), float('nan'), dtype=DT[tag], device=DEV)
    rc = lib.mrphy_blochsim_rfgr_fwd(code, v['M0'].data_ptr(), *P.k0_args(), *bg.args, *e1.args, *e2.args,
                                     e1m1.t.data_ptr(), Mo.data_ptr(), Mck.data_ptr(), 16, P.N, P.nM, P.nT, P.nC,
                                     _host.current_stream(DEV))
    assert rc != 0 and lib.mrphy_error_string(rc) == b'mrphy: invalid argument', rc
    rc = lib.mrphy_rfgr2beff_st(beffective._code(DT[tag]), *P.k0_args(), beff.data_ptr(), P.N, P.nM, P.nT, P.nC, -1,
                                _host.current_stream(DEV))
    assert rc != 0 and lib.mrphy_error_string(rc) == b'mrphy: invalid argument'
    torch.cuda.synchronize()
    assert bool(torch.isnan(Mo).all()) and bool(torch.isnan(Mck).all()) and bool(torch.isnan(beff).all())
    # ... and the process goes on
    given, _ = cases.fused_operand_variants(DT[tag], 0)['compact_mixed']
    with mrphy_amd.constants_on('cpu'):
        fu, ora = _run('fused', given), _run('oracle', given)
    for k in NAMES:
        assert_close(fu[k], ora[k], tag, f'a normal call after the refused one: {k}')
