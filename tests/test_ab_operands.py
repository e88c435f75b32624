r"""``fused.ab_rfgr`` (K2ab / K2abb, under parallel transmit K2ab-mc / K2abb-mc, its split and composed routes) and ``fused.steadystate_rfgr`` / ``ab_steadystate`` on every
operand form the host code accepts -- ``cases.fused_operand_variants``: broadcast shapes, 0-dim and stride-0 operands, a
general ``*Nd`` grid, permuted views, buffers off the 16-byte grid, ``γ_beff != γ``, a batch ``dt``, non-contiguous and
unaligned cotangents --, on steps of exactly zero field (``cases.zero_field_case``), with spins whose ``γ`` is 0, and at
the batch-size limit ``N = 65535``.

Four invariants per case: (1) a spelling changes no bit -- the operands as given against the same numbers materialised
over ``(N, nM)``; (2) the routes agree -- ``B`` is ``blochsim_rfgr(Mi = 0)`` bit for bit, ``A, B`` are the materialised
route's (``rfgr2beff`` + ``beff2ab``'s kernels) bit for bit on the same four step constants, its gradients to the gate;
(3) ``A, B, grad_rf, grad_gr`` within the project's gates (``util.assert_close``: fp64 max-abs 1e-9, fp32 relative L2
1e-5) of the fp64 CPU oracle on the operands as given; (4) a second run gives the same bits.  ``precision('fast')`` is held
to (1), (2) and (4); its distance to the oracle goes to the ledger (``abops.*``).

The yardstick of (3) is ``test_ab_rfgr_host.oracle_ab_columns`` -- the EXPLICIT adjoint, column by column --, not
``O.beff2ab``'s autograd, which returns an exact 0 for the pulse gradient of every sample at which a spin sits at zero
field (``test_ab_rfgr_host.py::test_columns_hold_the_zero_field_limit_that_beff2ab_misses``).  In fp32 the oracle
integrates with the relaxation factors the kernels are handed (:func:`_for_oracle`): ``B`` is proportional to ``E1 - 1``,
about -4e-6, whose fp32 form carries a rounding error of up to 6e-8, 1.5 % of it; both sides then integrate the same
function, as ``test_ab_rfgr.py`` arranges by widening its ``E1, E2``.

The steady state end to end (``test_steadystate_end_to_end``): ``test_steadystate_host.torch_steadystate`` on the column
oracle's ``A, B`` in fp64.  fp64: ``test_steadystate._gate``.  fp32: three times the distance of the SAME chain evaluated
in fp32 on the CPU from itself in fp64 -- ``Mss`` inherits the rounding of an fp32 ``A`` and of the fp32 ``E1 - 1``,
amplified by the conditioning of ``I - A F``; the margin is the one ``test_against_the_reference_fixture`` uses for the same
reason.  CPU dry run of that distance (relative L2; ``Mss``, ``grad_rf``, ``grad_gr``), per case as ``rest0`` /
``restN_dfrest``: see ``SS_DRY_RUN`` below; the run's own figures go to the ledger (``abops.ss.*.oracle_f32_vs_f64``).
"""
import functools

import pytest

from gpu_common import *  # noqa: F401,F403
from mrphy_amd import _host
from mrphy_amd.fused import _forward_prep
from test_ab_ptx import BWD_MC, COUNTED, FWD_MC, _cap
from test_ab_rfgr import _counted
from test_ab_rfgr_host import ab_weights, oracle_ab_grads, oracle_steadystate_columns
from test_fused_operands import VARIANTS, _batch_problem, _same_bits
from test_steadystate import _gate as _ss_gate, _kernel_problem, _run as _ss_run
from test_steadystate_host import torch_steadystate

pytestmark = pytest.mark.gpu

MODES = [('f64', 'precise'), ('f32', 'precise'), ('f32', 'fast')]
NAMES = ('A', 'B', 'grad_rf', 'grad_gr')
FWD = 'mrphy_ab_rfgr_fwd'
# the oracle chain in fp32 against itself in fp64 on the CPU (relative L2 of Mss, grad_rf, grad_gr), nC = 1, nT = 48:
# what the fp32 gate of the end-to-end steady state is three times of.  The test measures it where it runs (an fp32 chain
# on another host rounds differently: 6.0e-6 .. 1.9e-5 on the MI355X host, where the kernels' own distance is 0.57 of the
# bound and below, except `zero_field.rest0.grad_gr`: 3.04e-5 against 3 x 1.10e-5, 0.92 of it).
SS_DRY_RUN = {
    'cube':        {'rest0': (8.8e-06, 9.8e-06, 1.1e-05), 'restN_dfrest': (8.0e-06, 6.6e-06, 6.8e-06)},
    'cube_planes': {'rest0': (1.0e-05, 1.4e-05, 1.7e-05), 'restN_dfrest': (8.4e-06, 7.6e-06, 1.2e-05)},
    'views':       {'rest0': (9.3e-06, 1.2e-05, 2.0e-05), 'restN_dfrest': (8.6e-06, 8.4e-06, 8.3e-06)},
    'zero_field':  {'rest0': (8.2e-06, 1.7e-05, 8.5e-06), 'restN_dfrest': (6.9e-06, 1.2e-05, 1.0e-05)},
}


# ---------------------------------------------------------------------------------------------
# cases, oracle (once per case, never modified), runs
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(tag, kind, nC, nT, name=None):
    r"""``(operands as given, dense spelling or None, zero-field mask or None)``; kind 'zoo' (a variant of the operand
    zoo), 'zero' (the zero-field case) or 'gamma0' ('gamma_split' with ``γ = 0`` for the two spins of ``ZERO_SPINS``: the
    per-spin STEP constant, not ``γ_beff`` -- their field is live)."""
    if kind == 'zero':
        v, zero = cases.zero_field_case(DT[tag], nC, nT)
        return v, None, zero
    given, dense = cases.fused_operand_variants(DT[tag], nC, nT)[name if kind == 'zoo' else 'gamma_split']
    if kind == 'gamma0':
        γ = given['γ'].clone()
        for n, s in cases.ZERO_SPINS:
            γ[n, s] = 0
        return dict(given, γ=γ), None, None
    return given, dense, None


def _step_constants(v):
    r"""``γ2πdt, E1, E1_1, E2`` of the case in its data type, formed on the CPU in their broadcast shapes
    (``cases.reference_constants``): what ``ab_rfgr`` forms itself under ``constants_on('cpu')``."""
    return cases.reference_constants(v['T1'], v['T2'], v['γ'], v['dt'], v['loc'].ndim + 1)


def _for_oracle(v, tag):
    r"""The operands the fp64 oracle gets.  fp64: as given.  fp32: ``T1, T2`` replaced by the fp64 times whose factors
    ``exp(-dt / T)`` ARE the fp32 ``E1, E2`` the kernels are handed (module docstring) -- to 1e-16 relative, so ``E1 - 1``
    to 3e-11."""
    if tag == 'f64' or v['T1'] is None:
        return v
    lead = v['loc'].ndim - 1
    c = cases.reference_constants(v['T1'], v['T2'], v['γ'], v['dt'], lead)
    dt = v['dt'].double().reshape(tuple(v['dt'].shape) + (lead - v['dt'].ndim) * (1,))
    return dict(v, T1=-dt / torch.log(c['E1'].double()), T2=-dt / torch.log(c['E2'].double()))


@functools.lru_cache(maxsize=None)
def _oracle(tag, kind, nC, nT, name=None):
    return oracle_ab_grads(_for_oracle(_case(tag, kind, nC, nT, name)[0], tag))


def _run(route, v, consts=None, grads=True):
    r"""``A, B`` and, with ``grads``, ``grad_rf, grad_gr`` for the cotangents ``test_ab_rfgr_host.ab_weights`` (in the
    form of the case's ``w``), handed over by ``torch.autograd.backward([A, B], [wA, wB])``.  ``route``: 'fused'
    (``fused.ab_rfgr``; with ``consts`` through ``consts=``) or 'mat' (``rfgr2beff`` + ``beff2ab``'s kernels on
    ``consts``).  The operands go in AS GIVEN: ``place`` keeps strides and offsets; ``rf`` and ``gr`` are leaves that are
    detached aliases, not copies."""
    leaf = lambda x: place(x).detach().requires_grad_(grads)  # noqa: E731
    rf, gr, loc = leaf(v['rf']), leaf(v['gr']), place(v['loc'])
    pk = dict(Δf=place(v['Δf']), b1Map=place(v['b1Map']))
    if route == 'fused':
        ck = dict(consts=consts) if consts is not None else dict(T1=place(v['T1']), T2=place(v['T2']), γ=place(v['γ']),
                                                                 dt=place(v['dt']))
        A, B = fused.ab_rfgr(rf, gr, loc, γ_beff=place(v['γ_beff']), **pk, **ck)
    else:
        beff = beffective.rfgr2beff(rf, gr, loc, γ=place(v['γ_beff']), **pk)
        A, B = beffective._Beff2AB.apply(beff, consts['γ2πdt'], consts['E1'], consts['E2'], consts['E1_1'], grads)
    res = dict(A=A.detach(), B=B.detach())
    if grads:
        wA, wB = ab_weights(v)
        torch.autograd.backward([A, B], [place(wA), place(wB)])
        res.update(grad_rf=rf.grad, grad_gr=gr.grad)
    return res


def _relaxed_only(v, n, s, nT):
    r"""``A = diag(E2ⁿ, E2ⁿ, E1ⁿ)``, ``B = (0, 0, 1 - E1ⁿ)`` of a spin that never rotates, stepped in fp64 with the case's own
    step constants (2-D cases)."""
    c = cases.reference_constants(v['T1'], v['T2'], v['γ'], v['dt'], 2)
    at = lambda x: float(x.expand(v['loc'].shape[:2])[n, s])  # noqa: E731
    e1, e2, e1m1 = at(c['E1']), at(c['E2']), at(c['E1_1'])
    a1 = a2 = 1.0
    b = 0.0
    for _ in range(nT):
        a1, a2, b = a1 * e1, a2 * e2, b * e1 - e1m1
    return torch.diag(torch.tensor([a2, a2, a1], dtype=torch.float64)), torch.tensor([0.0, 0.0, b], dtype=torch.float64)


def _expected_route(tag, nC, nT):
    r"""The route of ``ab_rfgr`` with a pulse gradient for ``nC > 1`` coils with their map, written out from
    ``fused._decide_ab_route``'s rules and ``ab_rfgr``'s docstring (segments of 16 steps; the capacity of K2ab-mc /
    K2abb-mc is 8 coils in fp32 and 4 in fp64): 'composed' above the capacity, 'fused' on whole segments, 'split' for a
    ragged length of more than one segment."""
    table = {(True, True): 'fused', (True, False): 'split', (False, True): 'composed', (False, False): 'composed'}
    return table[(2 <= nC <= _cap(tag), nT % 16 == 0)] if nT > 16 else 'composed'


def _assert_route(n, route, key):
    r"""The calls ``n`` of one ``ab_rfgr`` forward + backward under parallel transmit are those of ``route``; the
    one-coil entry points are never called."""
    n = {k: c for k, c in n.items() if c}
    assert not n.get('mrphy_ab_rfgr_fwd') and not n.get('mrphy_ab_rfgr_bwd'), (key, n)
    if route == 'fused':
        assert n == {FWD_MC: 1, BWD_MC: 1}, (key, n)
    elif route == 'split':
        assert n.get(FWD_MC) == 1 and n.get(BWD_MC) == 1 and n.get('mrphy_beff2ab_save') == 1, (key, n)
    else:
        assert not n.get(FWD_MC) and not n.get(BWD_MC) and n.get('mrphy_beff2ab_save') == 1, (key, n)


def _invariants(tag, mode, kind, nC, nT, name=None, calls=None):
    r"""Invariants (1)-(4) of the module docstring for one case; returns the fused results.  ``calls``: the counter of
    ``test_ab_rfgr._counted`` over ``test_ab_ptx.COUNTED``; under parallel transmit the first run's route is asserted
    by its call counts (:func:`_expected_route`)."""
    v, dense, zero = _case(tag, kind, nC, nT, name)
    key = f'c{nC}.nT{nT}.{name or kind}'
    lead = tuple(v['loc'].shape[:-1])
    if calls is not None:
        calls.clear()
    fu = _run('fused', v)
    if calls is not None and nC > 1:
        _assert_route(dict(calls), _expected_route(tag, nC, nT), key)
    assert fu['A'].shape == lead + (3, 3) and fu['B'].shape == lead + (3,), (key, fu['A'].shape, fu['B'].shape)
    assert fu['grad_rf'].shape == v['rf'].shape and fu['grad_gr'].shape == v['gr'].shape, key
    for k in NAMES:
        assert fu[k].dtype == DT[tag] and bool(torch.isfinite(fu[k]).all()), (key, k)
    if dense is not None:                                                      # (1) the spelling changes nothing
        fd = _run('fused', dense)
        for k in ('A', 'B'):
            _same_bits(fu[k].reshape(fd[k].shape), fd[k], f'{key}: {k}, as given vs dense')
        for k in ('grad_rf', 'grad_gr'):
            if fu[k].shape == fd[k].shape:
                _same_bits(fu[k], fd[k], f'{key}: {k}, as given vs dense')
            else:                                                              # a batch-1 pulse, expanded in `dense`
                assert_close(fu[k], fd[k].sum(0, keepdim=True), tag, f'{key}: {k} vs dense summed over N')
    # (2) the routes
    kw = dict(Δf=place(v['Δf']), b1Map=place(v['b1Map']), γ_beff=place(v['γ_beff']), T1=place(v['T1']),
              T2=place(v['T2']), γ=place(v['γ']), dt=place(v['dt']))
    with torch.no_grad():
        Mo = fused.blochsim_rfgr(torch.zeros(lead + (3,), dtype=DT[tag], device=DEV), place(v['rf']), place(v['gr']),
                                 place(v['loc']), **kw)
    # the forward alone is one K2ab over all nT steps (K2ab-mc under parallel transmit up to its capacity, the composed
    # kernels above it), whatever nT is; with
    # a pulse gradient a ragged length is split and joined by two 3x3 products: the same numbers, other roundings
    f0 = _run('fused', v, grads=False)
    _same_bits(f0['B'], Mo, f'{key}: B vs blochsim_rfgr(Mi = 0)')
    c = {k: x.to(DEV) for k, x in _step_constants(v).items()}
    mat = _run('mat', v, consts=c)
    fc = _run('fused', v, consts=c, grads=False)
    for k in ('A', 'B'):
        _same_bits(fc[k], mat[k], f'{key}: {k}, consts= vs the materialised route on the same constants')
        _same_bits(fc[k], f0[k], f'{key}: {k}, consts= vs T1, T2, γ, dt')
        if nT % 16 == 0:
            _same_bits(fu[k], f0[k], f'{key}: {k}, with and without a pulse gradient')
        else:
            assert_close(fu[k], f0[k], tag, f'{key}: {k}, the split route vs one sweep')
    for k in ('grad_rf', 'grad_gr'):
        assert mat[k].shape == fu[k].shape, (key, k)
        assert_close(fu[k], mat[k], tag, f'{key}: {k}, fused vs the materialised route')
    ora = _oracle(tag, kind, nC, nT, name)                                     # (3) the yardstick
    sl = lambda x: x.movedim(2, 1)[zero.to(x.device)]                          # noqa: E731
    seg = list(cases.ZERO_SEGMENT)
    for route, got in (('fused', fu), ('materialised', mat)):
        for k in NAMES:
            assert got[k].shape == ora[k].shape, (key, route, k)
            d = max_abs(got[k], ora[k]) if tag == 'f64' else rel_l2(got[k], ora[k])
            record(f'abops.{key}.{tag}.{mode}.{route}.{k}.vs_oracle', d, None if mode == 'fast' else 1e-9 if tag == 'f64' else 1e-5)
            if mode == 'precise':
                assert_close(got[k], ora[k], tag, f'{key}: {route} {k} vs oracle')
        if zero is not None:
            for k in ('grad_rf', 'grad_gr'):
                # the yardstick's own values there are O(1): the comparison is not with nothing
                assert float(sl(ora[k]).abs().max()) > 0.1 and float(ora[k][1][:, seg].abs().max()) > 0.1, (key, k)
                record(f'abops.{key}.{tag}.{mode}.{route}.{k}.zero_steps.rel_l2_vs_oracle', rel_l2(sl(got[k]), sl(ora[k])))
                if mode == 'precise':
                    assert_close(sl(got[k]), sl(ora[k]), tag, f'{key}: {route} {k} on the zero-field steps vs oracle')
                    assert_close(got[k][1][:, seg], ora[k][1][:, seg], tag, f'{key}: {route} {k} on the all-zero segment')
    again = _run('fused', v)                                                   # (4) determinism
    for k in NAMES:
        _same_bits(fu[k], again[k], f'{key}: {k}, second run')
    return fu


# =============================================================================================
# (a) spellings
# =============================================================================================
SPELLINGS = ([(nC, n, 48) for nC in (0, 1) for n in VARIANTS] + [(nC, n, 53) for nC in (0, 1) for n in cases.FUSED_NT53] +
             [(4, n, 48) for n in VARIANTS] + [(4, n, 53) for n in cases.FUSED_NT53] +
             [(nC, n, 48) for nC in (2, 8) for n in ('compact_mixed', 'views', 'offset')])


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('nC,name,nT', SPELLINGS, ids=[f'c{c}-{n}-{t_}' for c, n, t_ in SPELLINGS])
def test_operand_spellings(tag, mode, nC, name, nT, monkeypatch):
    r"""One problem, many spellings (module docstring).  nT = 48: K2ab and three checkpoint segments through K2abb; nT = 53:
    the split route, 48 fused steps joined with 5 composed ones (``A2 @ A1``, ``A2 @ B1 + B2`` on the operands' own
    ``*Nd``).  nC = 2, 4, 8 with their map: the parallel-transmit kernels K2ab-mc / K2abb-mc on the same zoo -- 4 coils on
    all eight variants and on the split, 2 and 8 coils on 'compact_mixed' (a batch-shared ``b1Map`` under a batch-1
    pulse), 'views' and 'offset'; 8 coils are the fp32 adjoint build that reads the map from LDS, and in fp64, above
    that type's capacity of 4, the composed route.  The route each of them took is asserted by call counts."""
    given = _case(tag, 'zoo', nC, nT, name)[0]
    wA, wB = ab_weights(given)
    if name == 'views':        # the forms under test arrive as such
        assert not any(place(x).is_contiguous() for x in (given['loc'], given['Δf'], given['rf'], given['gr'], wA, wB))
    if name == 'offset':
        assert all(place(x).is_contiguous() and place(x).data_ptr() % 16 != 0
                   for x in (given['loc'], given['rf'], given['gr'], wA, wB))
    if name == 'expanded':
        assert all(0 in place(given[k]).stride() for k in ('loc', 'Δf', 'γ_beff', 'T1', 'T2', 'γ'))
    calls = _counted(monkeypatch, COUNTED)
    with mrphy_amd.precision(mode):
        _invariants(tag, mode, 'zoo', nC, nT, name, calls=calls)


# =============================================================================================
# (b) zero field
# =============================================================================================
@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('nC', [0, 1])
@pytest.mark.parametrize('nT', [48, 53])
def test_zero_field_steps(tag, mode, nC, nT):
    r"""Dead time and spins at the iso-centre through K2abb's four adjoint columns (nT = 53: through the split).  The pulse
    gradients are held to the gates on the zero-field steps alone and on batch entry 1's all-zero segment alone as well,
    for the fused and the materialised route both.  CPU dry run (fp64, these cotangents; nC = 0 / 1): on the zero-field
    steps the yardstick's ``grad_rf`` reaches 1.2, 0.91 / 0.97, 0.84 and its ``grad_gr`` 5.4, 6.9 / 3.8, 5.4 in max abs (nT =
    48, 53), on the segment 0.62, 0.77 / 0.78, 0.30 and 3.4, 6.9 / 2.1, 5.3 -- ``O.beff2ab``'s autograd gives an exact 0
    there and is 0.54 .. 0.73 in relative L2 from the yardstick over the whole gradient: a kernel returning zeros on those
    steps misses the fp32 gate by a factor of 5e4.  With a map, spin 64 of entry 1 never rotates: pure relaxation."""
    v = _case(tag, 'zero', nC, nT)[0]
    with mrphy_amd.precision(mode):
        fu = _invariants(tag, mode, 'zero', nC, nT)
    if nC:
        A, B = _relaxed_only(v, 1, 64, nT)
        assert_close(fu['A'][1, 64], A, tag, 'the spin that never rotates: A')
        assert max_abs(fu['B'][1, 64, :2], B[:2]) == 0.0
        assert rel_l2(fu['B'][1, 64], B) <= (1e-12 if tag == 'f64' else 1e-5), rel_l2(fu['B'][1, 64], B)


# =============================================================================================
# (c) spins with γ = 0
# =============================================================================================
@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('nC', [0, 1])
@pytest.mark.parametrize('nT', [48, 53])
def test_gamma_zero_spins(tag, mode, nC, nT):
    r"""``γ[0, 7] = γ[1, 64] = 0`` on 'gamma_split' (mid-wave; the first lane of the second tile): padding spins.  Their
    field is live (``γ_beff`` is a separate operand), their rotation angle ``2πγ dt |B|`` an exact zero beside a unit
    vector that is not: every output and gradient stays finite (the ``0/0`` that ``bloch_math.hpp: adj_const_accumulate``
    records for K3 would make every pulse sample of the batch entry NaN, the gradients being sums over the spins), those
    spins' ``A`` is the relaxation diagonal, and the pulse gradients are the oracle's, to which these spins contribute an
    exact zero (the factor ``γ2πdt`` of ``O.explicit_backward``).  CPU dry run in fp64 (nC = 0, 1; nT = 48, 53): with a
    live ``γ`` those spins' ``A`` has off-diagonal elements of 0.048 .. 0.99 (asserted here: exactly 0), and a kernel that
    let them contribute to the pulse gradients as live spins would move ``grad_rf`` by 0.049 .. 0.087 and ``grad_gr`` by
    0.050 .. 0.13 in relative L2, 5e3 fp32 gates."""
    v = _case(tag, 'gamma0', nC, nT)[0]
    with mrphy_amd.precision(mode):
        fu = _invariants(tag, mode, 'gamma0', nC, nT)
    for n, s in cases.ZERO_SPINS:
        A, B = _relaxed_only(v, n, s, nT)
        assert_close(fu['A'][n, s], A, tag, f'spin {(n, s)} with γ = 0: A')
        assert float((fu['A'][n, s] - torch.diag(torch.diagonal(fu['A'][n, s]))).abs().max()) == 0.0, (n, s)
        assert rel_l2(fu['B'][n, s], B) <= (1e-12 if tag == 'f64' else 1e-5)


# =============================================================================================
# (d) the steady state end to end
# =============================================================================================
SS_CASES = ['cube', 'cube_planes', 'views', 'zero_field']
SS_FORMS = ['rest0', 'restN_dfrest']


@functools.lru_cache(maxsize=None)
def _ss_case(tag, name, form):
    r"""The case with ``T1`` in 0.05 .. 0.15 s and ``T2`` in 0.02 .. 0.07 s in the forms it has them in (drawn as
    ``test_steadystate._kernel_problem`` draws them), ``rest`` `()` = 5e-3 s or `(N,)` = (5e-3, 6.5e-3), ``Δf_rest`` absent
    or one value per spin: ``I - A F`` as well conditioned as in that module."""
    v = _case(tag, 'zero', 1, 48)[0] if name == 'zero_field' else _case(tag, 'zoo', 1, 48, name)[0]
    gen = torch.Generator().manual_seed(5000 + SS_CASES.index(name))
    rnd = lambda s: torch.rand(tuple(s), generator=gen, dtype=torch.float64)  # noqa: E731
    v = dict(v, T1=(0.05 + 0.1 * rnd(v['T1'].shape)).to(DT[tag]), T2=(0.02 + 0.05 * rnd(v['T2'].shape)).to(DT[tag]))
    df_rest = ((rnd(v['loc'].shape[:-1]) * 2 - 1) * 200).to(DT[tag])
    if form == 'rest0':
        return v, torch.tensor(5e-3, dtype=DT[tag]), None
    return v, torch.tensor([5e-3, 6.5e-3], dtype=DT[tag]), df_rest


@functools.lru_cache(maxsize=None)
def _ss_oracle(tag, name, form):
    r"""The fp64 chain; for fp32 data also the relative L2 distance of the same chain in fp32 from it, and the fp64 chain
    whose pulse relaxes with the fp32 factors the kernels are handed (:func:`_for_oracle`; for the ledger: what of the
    distance is the kernels' own arithmetic)."""
    v, rest, df_rest = _ss_case(tag, name, form)
    df = v['Δf'] if df_rest is None else df_rest
    wide = oracle_steadystate_columns(v, rest, v['T1'], v['T2'], df)
    if tag == 'f64':
        return wide, None, None
    low = oracle_steadystate_columns(v, rest, v['T1'], v['T2'], df, dtype=torch.float32)
    same = oracle_steadystate_columns(_for_oracle(v, tag), rest, v['T1'], v['T2'], df)
    return wide, {k: rel_l2(low[k], wide[k]) for k in wide}, same


def _steady(v, rest, df_rest):
    leaf = lambda x: place(x).detach().requires_grad_(True)  # noqa: E731
    rf, gr = leaf(v['rf']), leaf(v['gr'])
    Mss = fused.steadystate_rfgr(rf, gr, place(v['loc']), rest=dev(rest), T1=place(v['T1']), T2=place(v['T2']),
                                 Δf=place(v['Δf']), b1Map=place(v['b1Map']), γ_beff=place(v['γ_beff']), γ=place(v['γ']),
                                 dt=place(v['dt']), Δf_rest=dev(df_rest))
    torch.autograd.backward([Mss], [place(v['w'])])
    return dict(Mss=Mss.detach(), grad_rf=rf.grad, grad_gr=gr.grad)


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('name', SS_CASES)
@pytest.mark.parametrize('form', SS_FORMS)
def test_steadystate_end_to_end(tag, mode, name, form):
    r"""``steadystate_rfgr`` on a ``*Nd`` grid, on views (a non-contiguous cotangent) and through dead time, one transmit
    coil with a map, nT = 48: ``Mss`` and the gradients w.r.t. ``rf`` and ``gr`` against the module docstring's chain;
    shapes and dtype of the operands as given; twice the same bits."""
    v, rest, df_rest = _ss_case(tag, name, form)
    wide, d32, same = _ss_oracle(tag, name, form)
    key = f'abops.ss.{name}.{form}.{tag}.{mode}'
    with mrphy_amd.precision(mode):
        got, again = _steady(v, rest, df_rest), _steady(v, rest, df_rest)
    assert got['Mss'].shape == v['loc'].shape and got['Mss'].dtype == DT[tag]
    for k in got:
        assert got[k].shape == wide[k].shape and bool(torch.isfinite(got[k]).all()), (key, k)
        _same_bits(got[k], again[k], f'{key}: {k}, second run')
        if tag == 'f64':
            _ss_gate(got[k], wide[k], tag, k)
            continue
        bound = 3 * d32[k]
        record(f'{key}.{k}.oracle_f32_vs_f64', d32[k], note='the oracle chain in fp32 against itself in fp64, CPU')
        record(f'{key}.{k}.vs_oracle64_on_the_kernels_factors', rel_l2(got[k], same[k]), note='not asserted')
        d = record(f'{key}.{k}.vs_oracle64', rel_l2(got[k], wide[k]), bound if mode == 'precise' else None)
        print(f'{key} {k}: {d:.3e} from the fp64 chain; the chain in fp32: {d32[k]:.3e}')
        if mode == 'precise':
            assert d <= bound, f'{key} {k}: {d:.3e} > 3 x {d32[k]:.3e}, the oracle chain\'s own fp32 distance'


@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('form', ['permuted', 'offset', 'cotangent'])
def test_ab_steadystate_views(tag, form):
    r"""``ab_steadystate`` alone: ``A`` and ``B`` as permuted views, one element into a larger buffer, and a non-contiguous
    ``grad_Mss`` -- ``Mss`` and the gradients w.r.t. ``A, B, rest, T1, T2, Δf`` against the call on contiguous copies, at
    ``test_steadystate._gate``; the gradients in the shapes of their operands."""
    P, _ = _kernel_problem(2, 100, tag)
    ref = _ss_run(P)
    A, B, w = P['A'], P['B'], P['w']
    if form == 'permuted':
        A, B = A.permute(2, 3, 0, 1).contiguous().permute(2, 3, 0, 1), B.permute(2, 0, 1).contiguous().permute(1, 2, 0)
        assert not place(A).is_contiguous() and not place(B).is_contiguous()
    elif form == 'offset':
        A, B = cases._after(A), cases._after(B)
        assert place(A).data_ptr() % 16 != 0 and place(B).data_ptr() % 16 != 0
    else:
        w = w.transpose(1, 2).contiguous().transpose(1, 2)
        assert not place(w).is_contiguous()
    L = dict(A=place(A).detach().requires_grad_(True), B=place(B).detach().requires_grad_(True))
    L.update({k: dev(P[k]).clone().requires_grad_(True) for k in ('rest', 'T1', 'T2', 'df')})
    Mss = fused.ab_steadystate(L['A'], L['B'], rest=L['rest'], T1=L['T1'], T2=L['T2'], Δf=L['df'])
    torch.autograd.backward([Mss], [place(w)])
    _ss_gate(Mss.detach(), ref['Mss'], tag, 'Mss')
    for k, x in L.items():
        assert x.grad is not None and x.grad.shape == x.shape, k
        _ss_gate(x.grad, ref['grad_' + k], tag, 'grad_' + k)


# =============================================================================================
# (e) the batch-size limit N <= 65535
# =============================================================================================
@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_batch_size_limit_65535(tag):
    r"""``N = 65535``, one spin each, one checkpoint segment: ``A, B`` and the pulse gradients against the column oracle --
    the fp32 pulse gradients entry by entry too (``test_fused_operands.test_batch_size_limit_65535``: one batch entry's
    gradient is a few numbers among 65535 times as many) --, and ``ab_steadystate`` on that ``A, B``."""
    v = _batch_problem(65535, DT[tag])
    fu, ora = _run('fused', v), oracle_ab_grads(_for_oracle(v, tag))
    for k in NAMES:
        assert fu[k].shape == ora[k].shape, k
        assert_close(fu[k], ora[k], tag, f'N = 65535: {k} vs oracle')
        if tag == 'f32' and k in ('grad_rf', 'grad_gr'):
            elementwise(f'abops.N65535.{k}', fu[k], ora[k], ELEM32_GRAD, scale=True, comp_axis=1)
    rest = torch.tensor(5e-3, dtype=DT[tag])
    with torch.no_grad():
        Mss = fused.ab_steadystate(fu['A'], fu['B'], rest=dev(rest), T1=place(v['T1']), T2=place(v['T2']))
    want = torch_steadystate(fu['A'].double().cpu(), fu['B'].double().cpu(), rest.double(), v['T1'].double(), v['T2'].double())
    _ss_gate(Mss, want, tag, 'Mss at N = 65535')


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_batch_size_beyond_limit_is_refused_before_any_launch(tag):
    r"""``N = 65536``: ``fused.ab_rfgr`` raises the library's ``RuntimeError`` naming the entry point, with and without a
    pulse gradient; through the C ABI both entry points return MRPHY_EINVAL with their NaN-filled outputs untouched
    (nothing was launched); the process then passes a normal call."""
    lib = mrphy_amd.require_library()
    v = {k: (place(x) if isinstance(x, torch.Tensor) else x) for k, x in _batch_problem(65536, DT[tag]).items()}
    kw = dict(Δf=v['Δf'], γ_beff=v['γ_beff'], T1=v['T1'], T2=v['T2'], γ=v['γ'], dt=v['dt'])
    with pytest.raises(RuntimeError, match=FWD + '.*invalid argument'):
        fused.ab_rfgr(v['rf'], v['gr'], v['loc'], **kw)
    with pytest.raises(RuntimeError, match=FWD + '.*invalid argument'):
        fused.ab_rfgr(v['rf'].requires_grad_(True), v['gr'], v['loc'], **kw)
    v['rf'].requires_grad_(False)
    p = beffective._PulseOnSpins(v['rf'], v['gr'], v['loc'], v['Δf'], None, v['γ_beff'])
    cs = sims.relax_constants(v['T1'], v['T2'], v['γ'], v['dt'], 4, DEV)
    code, alive, consts, _, _ = _forward_prep(lib, p, *cs, DT[tag], DEV, False)
    new = lambda *s: torch.full(s, float('nan'), dtype=DT[tag], device=DEV)  # noqa: E731
    A, B, ABck = new(p.N, 1, 3, 3), new(p.N, 1, 3), new(1, 4, p.N, 3)
    grf, ggr, work = new(p.N, 2, p.nT, 1), new(p.N, 3, p.nT), torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    st = _host.current_stream(DEV)
    rc = lib.mrphy_ab_rfgr_fwd(code, *p.k0_args(), *consts, A.data_ptr(), B.data_ptr(), ABck.data_ptr(), 16, p.N, p.nM,
                               p.nT, st)
    assert rc != 0 and lib.mrphy_error_string(rc) == b'mrphy: invalid argument', rc
    rc = lib.mrphy_ab_rfgr_bwd(code, ABck.data_ptr(), *p.k0_args(), *consts, A.data_ptr(), B.data_ptr(), grf.data_ptr(),
                               ggr.data_ptr(), work.data_ptr(), work.numel(), p.N, p.nM, p.nT, st)
    assert rc != 0 and lib.mrphy_error_string(rc) == b'mrphy: invalid argument', rc
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(x).all()) for x in (A, B, ABck, grf, ggr)) and int(work.sum()) == 0
    del alive
    # ... and the process goes on
    given = _case(tag, 'zoo', 0, 48, 'compact_mixed')[0]
    with mrphy_amd.constants_on('cpu'):
        fu = _run('fused', given)
    ora = _oracle(tag, 'zoo', 0, 48, 'compact_mixed')
    for k in NAMES:
        assert_close(fu[k], ora[k], tag, f'a normal call after the refused one: {k}')
