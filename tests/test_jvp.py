r"""K2j: ``fused.blochsim_rfgr_jvp`` and ``fused.sensitivity_rfgr`` on the GPU -- each tangent group against the CPU oracle's
forward-mode derivative (``test_jvp_host.oracle_jvp``, pinned there to the reference's), ``Mo`` against ``blochsim_rfgr``
bit for bit, the direction capacity and its blocks, exact linearity, the branches of ``S'``, ``C'``, the dot-product
identity with the fused adjoint, operand forms, and the sensitivity maps.

Distances are taken per group and per direction, relative to that direction's own norm: the groups' tangents differ by
four orders of magnitude (``|dMo| / |Mo|`` from 1.5 for ``loc`` to 1e-4 for ``T1`` on this kind of problem), and a combined
norm would hide a wrong ``Δf`` or ``T1`` path.  Gates: fp64 ``max_abs <= ATOL64 · max(1, max|want|)``; fp32 precise
``REL32``, the fused adjoint's gate (the oracle's own fp32 tangent lies a tenth of it from its fp64 one at ``nT <= 48``);
the fast mode's distances go to the ledger unasserted."""
import functools

import pytest

from gpu_common import *  # noqa: F401,F403
from test_jvp_host import GROUPS, oracle_jvp
from util import ATOL64, REL32

pytestmark = pytest.mark.gpu

VARIANTS = ['plain', 'b1map', 'norelax', 'b1map_norelax']
MODES = [('f64', 'precise'), ('f32', 'precise'), ('f32', 'fast')]
SCALE = dict(Mi=1.0, rf=3.0, gr=1.0, loc=6.0, Δf=200.0, b1Map=1.0, T1=1.0, T2=0.1)
KW = dict(Δf='Δf', b1Map='b1Map', γ_beff='γ', T1='T1', T2='T2', γ='γ', dt='dt')


@functools.lru_cache(maxsize=None)
def _problem(variant, nT, seed=41, N=2, nM=130):
    r"""``test_fused_traj._problem``'s operands in fp64 (CPU), by the names of ``GROUPS``: a pulse per batch entry; nM = 130:
    two full tiles and a ragged one of 2 lanes."""
    gen = torch.Generator().manual_seed(seed + nT)
    rnd = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64)  # noqa: E731
    P = dict(Mi=rnd(N, nM, 3), rf=(rnd(N, 2, nT) * 2 - 1) * 3, gr=rnd(N, 3, nT) * 2 - 1, loc=(rnd(N, nM, 3) * 2 - 1) * 6,
             Δf=(rnd(N, nM) * 2 - 1) * 200, b1Map=rnd(N, nM, 2) * 2 - 1, T1=0.5 + rnd(N, nM), T2=0.02 + 0.1 * rnd(N, nM))
    if not variant.startswith('b1map'):
        P['b1Map'] = None
    if variant.endswith('norelax'):
        P['T1'] = P['T2'] = None
    P['γ'], P['dt'] = torch.tensor(4257.6, dtype=torch.float64), torch.tensor([4e-6], dtype=torch.float64)
    return P


def _groups(P):
    return tuple(k for k in GROUPS if P[k] is not None)


def _directions(P, n, seed=7):
    r"""``n`` seeded directions per group present: ``{group: (n, *operand shape)}`` in fp64."""
    gen = torch.Generator().manual_seed(seed)
    return {k: (torch.rand((n,) + tuple(P[k].shape), generator=gen, dtype=torch.float64) * 2 - 1) * SCALE[k] for k in _groups(P)}


def _cast(P, tag):
    return {k: (None if v is None else v.to(DT[tag])) for k, v in P.items()}


def _args(P, on=dev):
    return (on(P['Mi']), on(P['rf']), on(P['gr']), on(P['loc'])), {k: on(P[v]) for k, v in KW.items()}


def _jvp(P, tangents, mode='precise', on=dev, **more):
    a, kw = _args(P, on)
    with mrphy_amd.precision(mode):
        Mo, dMo = fused.blochsim_rfgr_jvp(*a, tangents={k: on(v) for k, v in tangents.items()}, **kw, **more)
    assert not Mo.requires_grad and not dMo.requires_grad
    return Mo, dMo


def _forward(P, mode='precise'):
    a, kw = _args(P)
    with mrphy_amd.precision(mode), torch.no_grad():
        return fused.blochsim_rfgr(*a, **kw)


def _gate(key, tag, mode, got, want):
    r"""The gate of the module docstring on one direction of one group; every distance goes to the ledger."""
    assert got.shape == want.shape, (key, got.shape, want.shape)
    if tag == 'f64':
        bound = ATOL64 * max(1.0, float(want.abs().max()))
        d = record(f'jvp.{key}.f64.max_abs', max_abs(got, want), bound)
        print(f'{key} f64 max_abs {d:.3e} (bound {bound:.1e})')
        assert d <= bound, (key, d, bound)
    else:
        d = record(f'jvp.{key}.f32.{mode}.rel_l2', rel_l2(got, want), REL32 if mode == 'precise' else None)
        print(f'{key} f32 {mode} rel_l2 {d:.3e}')
        if mode == 'precise':
            assert d <= REL32, (key, d)


# ---------------------------------------------------------------------------------------------
# 1. each group alone; Mo's bits
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nT', [1, 7, 8, 9, 41, 48])
@pytest.mark.parametrize('variant', VARIANTS)
def test_each_group_alone_against_the_oracle(variant, nT):
    P64 = _problem(variant, nT)
    V64 = _directions(P64, 1)
    for tag in ('f64', 'f32'):
        P, V = _cast(P64, tag), _cast(V64, tag)
        want = {k: oracle_jvp(P, {k: V[k][0]}) for k in _groups(P)}          # on the operands as given, widened
        for mode in [m for t_, m in MODES if t_ == tag]:
            Mo_static = _forward(P, mode)
            for k in _groups(P):
                Mo, dMo = _jvp(P, {k: V[k]}, mode)
                assert dMo.shape == (1, 2, 130, 3) and dMo.dtype == DT[tag]
                assert torch.equal(Mo, Mo_static), (variant, nT, tag, mode, k, 'Mo is blochsim_rfgr\'s, bit for bit')
                _gate(f'{variant}.nT{nT}.{k}', tag, mode, dMo[0].cpu(), want[k][1])
            if mode == 'precise':                                               # (the primal itself, once per mode)
                assert_close(Mo.cpu(), want[k][0], tag, 'Mo')


@pytest.mark.parametrize('mode', ['precise', 'fast'])
def test_fp64_constants_beside_fp32_data(mode):
    r"""``T1, T2, γ, dt`` in fp64 beside fp32 data: the dtype codes ``MRPHY_F32P_C64`` / ``MRPHY_F32_C64``, whose step forms its
    products with the constants in fp64.  ``Mo``'s bits and the gate of case 1, all groups."""
    P = _cast(_problem('b1map', 9), 'f32')
    P.update({k: _problem('b1map', 9)[k] for k in ('T1', 'T2', 'γ', 'dt')})
    V = _cast(_directions(P, 1, seed=23), 'f32')
    Mo_static = _forward(P, mode)
    for k in _groups(P):
        Mo, dMo = _jvp(P, {k: V[k]}, mode)
        assert Mo.dtype == dMo.dtype == torch.float32 and torch.equal(Mo, Mo_static)
        _gate(f'c64.{k}', 'f32', mode, dMo[0].cpu(), oracle_jvp(P, {k: V[k][0]})[1])


# ---------------------------------------------------------------------------------------------
# 2. all groups at once
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag, mode', MODES)
def test_all_groups_at_once_is_the_sum_of_the_groups(tag, mode):
    P = _cast(_problem('b1map', 41), tag)
    V = _cast(_directions(P, 1, seed=9), tag)
    _, both = _jvp(P, V, mode)
    parts = sum(_jvp(P, {k: V[k]}, mode)[1].double() for k in V)
    _, want = oracle_jvp(P, {k: v[0] for k, v in V.items()})
    _gate('all_groups.vs_sum', tag, mode, both[0].cpu().double(), parts[0].cpu())
    _gate('all_groups.vs_oracle', tag, mode, both[0].cpu(), want)


# ---------------------------------------------------------------------------------------------
# 3. the direction capacity and its blocks
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag, mode', MODES)
@pytest.mark.parametrize('variant', ['b1map', 'norelax'])
def test_every_direction_has_the_bits_of_its_own_call(variant, tag, mode):
    r"""D = 1, 2, 3, 4, 5, 9 of nine seeded directions (all groups in each): a partially filled capacity, a full one, one
    block + 1, two blocks + 1.  Cross-talk between direction registers, the blocks' order or a capacity that rounds
    differently would show."""
    P = _cast(_problem(variant, 9), tag)
    V = _cast(_directions(P, 9, seed=11), tag)
    alone = [_jvp(P, {k: v[d:d + 1] for k, v in V.items()}, mode)[1][0] for d in range(9)]
    Mo1 = _forward(P, mode)
    for D in (1, 2, 3, 4, 5, 9):
        Mo, dMo = _jvp(P, {k: v[:D] for k, v in V.items()}, mode)
        assert dMo.shape[0] == D and torch.equal(Mo, Mo1)
        for d in range(D):
            assert torch.equal(dMo[d], alone[d]), (variant, tag, mode, D, d)
    # ... and whichever directions ride along: direction 3 beside 7, 8 and beside zeros
    pick = lambda idx: {k: v[idx] for k, v in V.items()}  # noqa: E731
    assert torch.equal(_jvp(P, pick([7, 3, 8]), mode)[1][1], alone[3])
    assert torch.equal(_jvp(P, {k: torch.stack([v[3], 0 * v[3]]) for k, v in V.items()}, mode)[1][0], alone[3])


# ---------------------------------------------------------------------------------------------
# 4. exact linearity
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag, mode', MODES)
@pytest.mark.parametrize('variant', ['b1map', 'plain'])
def test_the_tangent_is_exactly_linear(variant, tag, mode):
    r"""Zero tangents give exact zeros (no primal term, such as the ``E1 - 1`` offset, leaks in); ``2v`` gives ``2 dMo(v)`` and
    ``-v`` gives ``-dMo(v)`` bit for bit: scaling by a power of two commutes with every FMA."""
    P = _cast(_problem(variant, 9), tag)
    V = _cast(_directions(P, 1, seed=13), tag)
    _, zero = _jvp(P, {k: torch.zeros_like(v) for k, v in V.items()}, mode)
    assert float(zero.abs().max()) == 0.0
    _, one = _jvp(P, V, mode)
    assert float(one.abs().min()) > 0
    _, both = _jvp(P, {k: torch.cat([2 * v, -v, 0.25 * v]) for k, v in V.items()}, mode)
    assert torch.equal(both[0], 2 * one[0]) and torch.equal(both[1], -one[0]) and torch.equal(both[2], 0.25 * one[0])
    for k in V:                                                             # group by group too
        _, a = _jvp(P, {k: V[k]}, mode)
        _, b = _jvp(P, {k: torch.cat([-2 * V[k], 0 * V[k]])}, mode)
        assert torch.equal(b[0], -2 * a[0]) and float(b[1].abs().max()) == 0.0, k


# ---------------------------------------------------------------------------------------------
# 5. the branches of S', C' within one wave
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_zero_field_steps_and_large_angles_within_one_wave(tag):
    r"""Two all-zero steps (``rf = gr = 0``) with ``Δf = 0`` on every other spin: ``x = 0`` there, the derivative
    polynomials at their constant terms with a tangent field that is not zero.  One step with an 8 G/cm gradient: at
    ``dt = 4 us`` spins beyond 3.7 cm along it turn by more than π and take the closed forms of the cold path, the rest of
    the same wave do not.

    The yardstick on the ``x = 0`` spins.  The oracle, as the reference, turns ``M`` by the angle ``|b|`` about ``b / |b|``: a
    parametrisation that is singular at ``b = 0`` although the step itself is smooth there (``m - S b×m + C b×(b×m)``, with
    the derivative ``-b'×m``).  At ``b = 0`` exactly autograd differentiates ``norm`` by its subgradient 0 and the clamped
    axis by nothing, so the oracle's tangent of such a step is ``m'`` alone, whatever ``b'`` is -- measured on this problem:
    0.52 absolute from K2j in the ``rf`` group on exactly those spins, 0 on the others; K2b's adjoint, which the dot-product
    identity below ties to K2j, has the smooth derivative too.  The oracle's tangent is therefore taken in the limit: on
    those spins it runs at ``Δf = 1e-6 Hz`` (``|b| = 2.5e-11`` rad, above its clamp), the kernels at ``Δf = 0`` exactly.  The
    function's tangent moves by about ``2π dt nT · 1e-6 = 2e-10`` of its size between the two points: measured in fp64
    0.01 - 0.19 of the gate (``loc`` 1.04e-9 against 6.6e-9, ``Mi`` 3.0e-10 against 1.6e-9), nothing in fp32.  Gates and
    cases are those of case 1."""
    P64 = dict(_problem('b1map', 9, seed=43))
    P64['rf'], P64['gr'], P64['Δf'] = P64['rf'].clone(), P64['gr'].clone(), P64['Δf'].clone()
    P64['rf'][:, :, [2, 6]] = 0
    P64['gr'][:, :, [2, 6]] = 0
    P64['Δf'][:, ::2] = 0
    P64['gr'][:, :, 4] = torch.tensor([8.0, 0.0, 0.0], dtype=torch.float64)
    γ2πdt = 2 * torch.pi * 4257.6 * 4e-6
    φ = (γ2πdt * 8.0 * P64['loc'][..., 0]).abs()
    assert 10 < int((φ > torch.pi).sum()) < φ.numel() - 10, 'both branches within the waves'
    V64 = _directions(P64, 1, seed=15)
    P, V = _cast(P64, tag), _cast(V64, tag)
    Por = dict(P, Δf=P['Δf'].double().clone())                              # the oracle's own copy: P stays at Δf = 0
    Por['Δf'][:, ::2] = 1e-6                                                # the oracle's side of the limit (docstring)
    assert float(P['Δf'][:, ::2].abs().max()) == 0.0 and float(Por['Δf'][:, ::2].min()) == 1e-6
    Mo_static = _forward(P)
    for k in _groups(P):
        Mo, dMo = _jvp(P, {k: V[k]})
        assert torch.equal(Mo, Mo_static)
        _gate(f'branches.{k}', tag, 'precise', dMo[0].cpu(), oracle_jvp(Por, {k: V[k][0]})[1])


# ---------------------------------------------------------------------------------------------
# 6. the dot-product identity with the fused adjoint
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('group', [('Mi', 'rf', 'gr'), ('loc', 'Δf', 'b1Map'), ('T1', 'T2')])
def test_dot_product_identity_with_the_fused_adjoint(group):
    r"""``<w, J v> = <J^T w, v>`` in fp64 at nT = 48 (whole 16-step segments), one group of operands at a time: K2b, its MAPS
    build, its CONSTS build.  Both sides are library code: a consistency check on top of the oracle comparisons."""
    P = _problem('b1map', 48)
    V = _directions(P, 1, seed=17)
    w = torch.sin(torch.arange(2 * 130 * 3, dtype=torch.float64) * 0.61 + 1).reshape(2, 130, 3)
    _, dMo = _jvp(P, {k: V[k] for k in group})
    lhs = float((dev(w) * dMo[0]).sum())
    leaf = {k: _leaf(P[k], DEV) for k in group}
    a, kw = _args({**P, **leaf}, on=lambda x: x if x is None or x.is_cuda else x.to(DEV))
    fused.blochsim_rfgr(*a, **kw).backward(dev(w))
    rhs = sum(float((leaf[k].grad * dev(V[k][0])).sum()) for k in group)
    d = record(f'jvp.dot_product.{"_".join(group)}', abs(lhs - rhs) / abs(rhs), 1e-9)
    print(group, lhs, rhs, d)
    assert d <= 1e-9, (group, lhs, rhs)


# ---------------------------------------------------------------------------------------------
# 7. operand forms
# ---------------------------------------------------------------------------------------------
def test_tangents_broadcast_as_views_and_as_constants_tangents():
    P = _problem('b1map', 9)
    N, nM, nT = 2, 130, 9
    V = _directions(P, 3, seed=19)
    # a tangent shared by the batch: (D, 1, ...) against its dense copy
    shared = {k: v[:, :1] for k, v in V.items()}
    _, a = _jvp(P, shared)
    _, b = _jvp(P, {k: v.expand(V[k].shape).contiguous() for k, v in shared.items()})
    assert torch.equal(a, b)
    # non-contiguous views: a transpose, a slice of a larger buffer, an expanded constant
    def views(k, v):
        if k in ('Mi', 'loc', 'b1Map'):
            return v.transpose(1, 2).contiguous().transpose(1, 2)
        if k in ('rf', 'gr'):
            big = torch.zeros(v.shape[:-1] + (nT + 5,), dtype=v.dtype)
            big[..., 2:2 + nT] = v
            return big[..., 2:2 + nT]
        return v[:, :, :1].expand(v.shape)
    Vv = {k: views(k, v) for k, v in V.items()}
    assert not any(v.is_contiguous() for v in Vv.values())
    _, a = _jvp(P, Vv, on=place)
    _, b = _jvp(P, {k: v.contiguous() for k, v in Vv.items()})
    assert torch.equal(a, b)
    # dT1 per spin beside a 0-dim T1, T2
    P0 = dict(P, T1=torch.tensor(0.8, dtype=torch.float64), T2=torch.tensor(0.07, dtype=torch.float64))
    Pd = dict(P, T1=torch.full((N, nM), 0.8, dtype=torch.float64), T2=torch.full((N, nM), 0.07, dtype=torch.float64))
    _, a = _jvp(P0, dict(T1=V['T1'], T2=V['T2']))
    _, b = _jvp(Pd, dict(T1=V['T1'], T2=V['T2']))
    assert torch.equal(a, b) and float(a.abs().max()) > 0
    # consts= with the constants' own tangents
    E1, E2 = torch.exp(-P['dt'] / P['T1']), torch.exp(-P['dt'] / P['T2'])
    consts = dict(γ2πdt=dev(2 * torch.pi * P['γ'] * P['dt']), E1=dev(E1), E2=dev(E2), E1_1=dev(E1 - 1))
    dE = dict(E1=V['T1'] * 1e-5, E2=V['T2'] * 1e-3, E1_1=V['T1'] * 1e-5)
    Pc = dict(P, T1=None, T2=None)
    Mo, a = _jvp(Pc, dE, consts=consts)
    _, b = _jvp(Pc, {k: place(v.transpose(1, 2).contiguous().transpose(1, 2)) for k, v in dE.items()}, on=lambda x: x if x is None or x.is_cuda else dev(x), consts=consts)
    assert torch.equal(a, b) and float(a.abs().max()) > 0
    args, kw = _args(Pc)
    with torch.no_grad():
        assert torch.equal(Mo, fused.blochsim_rfgr(*args, **{k: v for k, v in kw.items() if k not in ('T1', 'T2', 'γ', 'dt')}, consts=consts))
    want = oracle_jvp(P, dict(T1=V['T1'][0] * 1e-5 * P['T1'] ** 2 / (P['dt'] * E1)))[1]     # dE1 = E1 dt / T1^2 dT1, inverted
    only1 = _jvp(Pc, dict(E1=dE['E1'], E1_1=dE['E1_1']), consts=consts)[1]
    _gate('consts.E1', 'f64', 'precise', only1[0].cpu(), want)


@pytest.mark.parametrize('nM', [1, 64, 65])
def test_tile_edges_and_the_empty_problem(nM):
    P = {k: (v[:, :nM] if k in ('Mi', 'loc', 'Δf', 'b1Map', 'T1', 'T2') and v is not None else v)
         for k, v in _problem('b1map', 9).items()}
    V = {k: v[0:2, :, :nM] if k in ('Mi', 'loc', 'Δf', 'b1Map', 'T1', 'T2') else v[0:2] for k, v in _directions(_problem('b1map', 9), 2, seed=21).items()}
    Mo, dMo = _jvp(P, V)
    assert torch.equal(Mo, _forward(P))
    for d in range(2):
        _gate(f'nM{nM}.dir{d}', 'f64', 'precise', dMo[d].cpu(), oracle_jvp(P, {k: v[d] for k, v in V.items()})[1])
    if nM == 1:                                                             # N nM = 0: empty outputs, no launch error
        P0 = {k: (v[:, :0] if k in ('Mi', 'loc', 'Δf', 'b1Map', 'T1', 'T2') else v) for k, v in P.items()}
        Mo, dMo = _jvp(P0, {k: (v[:, :, :0] if k in ('Mi', 'loc', 'Δf', 'b1Map', 'T1', 'T2') else v) for k, v in V.items()})
        assert Mo.shape == (2, 0, 3) and dMo.shape == (2, 2, 0, 3)


# ---------------------------------------------------------------------------------------------
# 8. sensitivity_rfgr
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', ['plain', 'b1map'])
def test_sensitivity_maps(variant):
    P = _problem(variant, 41)
    a, kw = _args(P)
    Mo, S = fused.sensitivity_rfgr(*a, **kw)
    assert tuple(S) == ('Δf', 'rf', 'T1', 'T2') and all(v.shape == (2, 130, 3) for v in S.values())
    one = lambda i: torch.eye(4, dtype=torch.float64)[:, i]  # noqa: E731
    tangents = dict(Δf=one(0).reshape(4, 1, 1), rf=one(1).reshape(4, 1, 1, 1) * P['rf'], T1=one(2).reshape(4, 1, 1),
                    T2=one(3).reshape(4, 1, 1))
    Mo2, dMo = _jvp(P, tangents)
    assert torch.equal(Mo, Mo2) and all(torch.equal(S[k], dMo[i]) for i, k in enumerate(S))
    # the Δf map against a central difference of blochsim_rfgr at Δf ± 0.01 Hz: 1e-6 is the difference's own budget (third
    # derivative and cancellation at this step)
    h = 0.01
    with torch.no_grad():
        up = fused.blochsim_rfgr(*a, **dict(kw, Δf=kw['Δf'] + h))
        dn = fused.blochsim_rfgr(*a, **dict(kw, Δf=kw['Δf'] - h))
    d = record(f'jvp.sensitivity.{variant}.df_vs_central_difference', rel_l2(S['Δf'], (up - dn) / (2 * h)), 1e-6)
    print('Δf map vs central difference', d)
    assert d <= 1e-6, d
    # 'rf' alone, and without relaxation
    Mo3, S3 = fused.sensitivity_rfgr(*a, wrt=('rf',), **dict(kw, T1=None, T2=None))
    assert tuple(S3) == ('rf',) and float(S3['rf'].abs().max()) > 0
