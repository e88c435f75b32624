r"""``fused.ab_rfgr``'s gradients w.r.t. the spin-side operands without a GPU: the two entry points
``mrphy_ab_rfgr_maps_bwd`` / ``mrphy_ab_rfgr_consts_bwd`` (K2abb's MAPS and CONSTS builds) are exported, declared and bound
alike and refuse bad arguments before any launch; the rows ``fused._decide_ab_route`` gains with ``spin_fused``; and the
yardstick of ``test_ab_spin_grads.py``, :func:`oracle_ab_spin_grads`, against finite differences.

The yardstick is the fp64 column chain of ``test_ab_rfgr_host.oracle_ab_columns`` -- ``B = sim(0)``, ``A[..., j] =
sim(e_j) - B`` on ``O.rfgr2beff``'s field, the four columns as batch entries -- with every operand a leaf, in two passes:
the EXPLICIT simulator ``O.blochsim`` for the operands the field is made of (``rf, gr, loc, Δf, b1Map, γ_beff``: its
adjoint holds the zero-field limit that autograd through ``F.normalize`` misses), and ``O.blochsim_slow``, whose Jacobian
autograd supplies, for ``T1, T2, γ, dt`` (a step of zero field does not depend on ``γ2πdt``, so nothing is missed there).
The constants are per-spin leaves `(N, nM)` -- the per-spin terms ``g_s`` that the gate of a summed operand is scaled
by -- and :func:`fold_like` sums them to the shape an operand was given in."""
import ctypes

import pytest
import torch

import bloch_oracle as O
import cases
import mrphy_amd
from mrphy_amd import _lib
from mrphy_amd.fused import _decide_ab_route
from test_ab_rfgr_host import _declared, ab_weights, oracle_ab_columns
from util import FAKE, fused_ops

NAMES = ('mrphy_ab_rfgr_maps_bwd', 'mrphy_ab_rfgr_consts_bwd')
EINVAL = -1
SEG = 16
FIELD = ('rf', 'gr', 'loc', 'Δf', 'b1Map', 'γ_beff')
CONSTS = ('T1', 'T2', 'γ', 'dt')


def test_symbols_are_exported_declared_and_bound_alike():
    raw = ctypes.CDLL(mrphy_amd.build())
    for name in NAMES:
        assert hasattr(raw, name), f'{name} is not exported'
        assert name in _lib.PROTOTYPES, f'{name} is not bound in _lib.py'
        res, args = _declared(name)
        assert (_lib.PROTOTYPES[name][0], list(_lib.PROTOTYPES[name][1])) == (res, args), name
    # mrphy_ab_rfgr_bwd's arguments with the per-spin outputs between grad_gr and the workspace: three, then four
    plain = list(_lib.PROTOTYPES['mrphy_ab_rfgr_bwd'][1])
    vp = ctypes.c_void_p
    assert list(_lib.PROTOTYPES[NAMES[0]][1]) == plain[:28] + [vp] * 3 + plain[28:]
    assert list(_lib.PROTOTYPES[NAMES[1]][1]) == plain[:28] + [vp] * 4 + plain[28:]
    for unit in ('tu_ab_rfgr_maps_bwd.hip', 'tu_ab_rfgr_consts_bwd.hip'):
        assert sorted(m for f, m in _lib.UNITS if f == unit) == sorted(m for f, m in _lib.UNITS if f == 'tu_ab_rfgr_bwd.hip')
    assert mrphy_amd.require_library().mrphy_abi_version() == _lib.ABI_VERSION == 5


def _calls(lib):
    r"""The two adjoints with fake pointers (never dereferenced: no call here is valid on a problem that is not empty);
    ``spin``: the per-spin outputs ``grad_loc, grad_Bz, grad_b1[, grad_consts]``."""
    def make(name, nspin):
        def call(ops, ABck=FAKE, work=FAKE, wb=None, N=1, nM=64, nT=SEG, dtype=0, spin=None):
            spin = [FAKE, FAKE, None, FAKE][:nspin] if spin is None else spin
            return getattr(lib, name)(dtype, ABck, *ops, FAKE, FAKE, FAKE, FAKE, *spin, work,
                                      lib.mrphy_blochsim_rfgr_bwd_workspace(0, N, nM, nT) if wb is None else wb,
                                      N, nM, nT, None)
        return call
    return make(NAMES[0], 3), make(NAMES[1], 4)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = mrphy_amd.require_library()
    ok = fused_ops()
    need = lib.mrphy_blochsim_rfgr_bwd_workspace(0, 1, 64, SEG)
    assert need > 0
    for bwd in _calls(lib):
        for dtype in (-1, 5, 17):
            assert bwd(ok, dtype=dtype) == EINVAL, ('unknown dtype', dtype)
        assert bwd(ok, ABck=None) == EINVAL and bwd(ok, work=None) == EINVAL, 'null checkpoints / workspace'
        assert bwd(ok, N=65536) == EINVAL, 'N > 65535'
        assert bwd(ok, nT=-SEG) == EINVAL, 'a negative size'
        for nT in (1, 7, SEG + 8, 50):
            assert bwd(ok, nT=nT) == EINVAL, ('the adjoint takes whole segments', nT)
        assert bwd(ok, wb=need - 1) == EINVAL and bwd(ok, wb=0) == EINVAL, 'a short workspace'
    # a grad_b1 needs a b1 map to differentiate -- a mode argument: refused on an empty problem too
    maps, consts = _calls(lib)
    assert maps(ok, spin=[None, None, FAKE]) == EINVAL and consts(ok, spin=[None, None, FAKE, None]) == EINVAL
    assert maps(ok, spin=[None, None, FAKE], nM=0) == EINVAL and consts(ok, spin=[None, None, FAKE, None], nT=0) == EINVAL
    for what in (dict(loc=None), dict(g=None), dict(rf=None), dict(gr=None), dict(df=FAKE), dict(E1=FAKE, E1m1=FAKE),
                 dict(E1m1=FAKE)):
        assert maps(fused_ops(**what)) == EINVAL and consts(fused_ops(**what)) == EINVAL, what


def test_empty_problems_are_a_success_whatever_the_operands_are():
    lib = mrphy_amd.require_library()
    null = fused_ops(rf=None, gr=None, loc=None, g=None)
    for bwd, spin in zip(_calls(lib), ([None] * 3, [None] * 4)):
        for kw in (dict(nM=0), dict(N=0), dict(nT=0)):
            assert bwd(null, ABck=None, work=None, wb=0, spin=spin, **kw) == 0, kw


# ---------------------------------------------------------------------------------------------
# the routing decision: the rows `spin_fused` adds (test_ab_rfgr_host.py::test_ab_route pins the default's)
# ---------------------------------------------------------------------------------------------
ONE = dict(seg=SEG, one_coil=True, pulse_grad=False, maps_grad=False, consts_grad=False, spin_fused=True)
ROUTES = [
    ('no gradient', dict(ONE, nT=48), ('fused', False)),
    ('a pulse gradient, nT 50', dict(ONE, nT=50, pulse_grad=True), ('split', 48)),
    ('a map gradient, nT 48', dict(ONE, nT=48, maps_grad=True), ('fused', True)),
    ('a map gradient, nT 16', dict(ONE, nT=16, maps_grad=True), ('fused', True)),
    ('a map gradient beside a pulse gradient', dict(ONE, nT=48, pulse_grad=True, maps_grad=True), ('fused', True)),
    ("a constants' gradient, nT 48", dict(ONE, nT=48, consts_grad=True), ('fused', True)),
    ('maps and constants, nT 50', dict(ONE, nT=50, maps_grad=True, consts_grad=True), ('split', 48)),
    ("a constants' gradient beside a pulse gradient, nT 17", dict(ONE, nT=17, pulse_grad=True, consts_grad=True),
     ('split', 16)),
    ('a map gradient, nT 7', dict(ONE, nT=7, maps_grad=True), ('composed', None)),
    ("a constants' gradient, nT 15", dict(ONE, nT=15, consts_grad=True), ('composed', None)),
    ('a map gradient, nT 0', dict(ONE, nT=0, maps_grad=True), ('fused', True)),
    ('4 coils, a map gradient', dict(ONE, nT=48, one_coil=False, maps_grad=True), ('composed', None)),
    ("4 coils, a constants' gradient, nT 50", dict(ONE, nT=50, one_coil=False, consts_grad=True), ('composed', None)),
    ('a build that was left out', dict(ONE, nT=48, consts_grad=True, spin_fused=False), ('composed', None)),
    ('a build that was left out, pulse gradient, nT 50',
     dict(ONE, nT=50, pulse_grad=True, maps_grad=True, spin_fused=False), ('composed', None)),
]


@pytest.mark.parametrize('what, facts, route', ROUTES, ids=[r[0] for r in ROUTES])
def test_ab_route_with_spin_gradients(what, facts, route):
    assert _decide_ab_route(**facts) == route


# ---------------------------------------------------------------------------------------------
# the yardstick
# ---------------------------------------------------------------------------------------------
def fold_like(g, like):
    r"""The per-spin gradient ``g`` `(N, nM[, k])` summed to the shape of the operand ``like`` as it was given (2-D
    spins): the axes summed that the operand broadcasts along, a 0-dim operand over all of them."""
    if like.ndim == 0:
        return g.sum()
    shape = tuple(like.shape) + (1,) * (g.ndim - like.ndim)   # right-padded, as the simulators pad the constants
    assert len(shape) == g.ndim, (g.shape, like.shape)
    dims = [i for i, (a, b) in enumerate(zip(g.shape, shape)) if b == 1 and a != 1]
    return (g.sum(dim=dims, keepdim=True) if dims else g).reshape(like.shape)


def straight_through_times(T, dt, E):
    r"""Relaxation times whose factor ``exp(-dt / T')`` IS ``E`` (the factor a kernel was handed, e.g. rounded to fp32) in
    value and ``exp(-dt / T)`` in its derivatives w.r.t. ``T`` and ``dt``: ``T' = -dt / log(exp(-dt / T) + (E - exp(-dt /
    T)).detach())``."""
    e = torch.exp(-dt / T)
    return -dt / torch.log(e + (E - e).detach())


def oracle_ab_spin_grads(v, wA=None, wB=None, dtype=torch.float64, factors=None, loss=None):
    r"""``A, B`` of the operand dict ``v`` (keys as ``cases.fused_operand_variants``; 2-D spins `(N, nM)`) and the gradients
    of ``(A wA).sum() + (B wB).sum()`` w.r.t. every operand (module docstring): ``rf, gr, loc, b1Map`` in the shapes given,
    ``Δf, γ_beff, T1, T2, γ, dt`` per spin `(N, nM)` (:func:`fold_like` sums them to an operand's own shape).  ``factors =
    (E1, E2)``: integrate with these relaxation factors (:func:`straight_through_times`).  ``loss(A, B, Q)``: another
    scalar of ``A, B`` and the pass's operands ``Q`` (the leaves ``T1, T2`` among them, for a rest period that shares
    them); it returns ``(scalar, extra)``, and ``extra`` (e.g. the steady state) comes back under ``'extra'``."""
    if wA is None and loss is None:
        wA, wB = ab_weights(v)
    N, nM = v['loc'].shape[:2]
    wide = lambda x: x.detach().to(dtype)  # noqa: E731
    per_spin = lambda x: wide(x).reshape(tuple(x.shape) + (2 - x.ndim) * (1,)).expand(N, nM).clone()  # noqa: E731
    L = {k: wide(v[k]).clone() for k in ('rf', 'gr', 'loc')}
    L['b1Map'] = None if v['b1Map'] is None else wide(v['b1Map']).clone()
    for k in ('Δf', 'γ_beff', 'T1', 'T2', 'γ'):
        L[k] = None if v[k] is None else per_spin(v[k])
    L['dt'] = per_spin(v['dt'].reshape(-1, 1) if v['dt'].ndim == 1 else v['dt'])
    out = {}
    for names, sim in ((FIELD, O.blochsim), (CONSTS, O.blochsim_slow)):
        Q = {k: (x.clone().requires_grad_(True) if k in names and x is not None else x) for k, x in L.items()}
        beff = O.rfgr2beff(Q['rf'], Q['gr'], Q['loc'], Δf=Q['Δf'], b1Map=Q['b1Map'], γ=Q['γ_beff'])
        Mi = torch.zeros((4, N, nM, 3), dtype=dtype)
        for j in range(3):
            Mi[j, ..., j] = 1
        T1, T2 = Q['T1'], Q['T2']
        if factors is not None and T1 is not None:
            T1, T2 = (straight_through_times(T, Q['dt'], wide(E).expand(N, nM)) for T, E in zip((T1, T2), factors))
        rep = lambda x: None if x is None else torch.cat([x] * 4, 0)  # noqa: E731
        Mo = sim(Mi.reshape(4 * N, nM, 3), torch.cat([beff] * 4, 0), T1=rep(T1), T2=rep(T2), γ=rep(Q['γ']),
                 dt=rep(Q['dt'])).reshape(4, N, nM, 3)
        A, B = torch.stack([Mo[j] - Mo[3] for j in range(3)], dim=-1), Mo[3]
        if loss is None:
            ((A * wide(wA)).sum() + (B * wide(wB)).sum()).backward()
        else:
            val, extra = loss(A, B, Q)
            val.backward()
            out.update(extra=extra.detach())
        out.update(A=A.detach(), B=B.detach())
        # (an operand nothing depends on -- γ_beff without a Δf -- has no gradient: an exact zero)
        out.update({k: torch.zeros_like(Q[k]) if Q[k].grad is None else Q[k].grad for k in names if Q[k] is not None})
    return out


def _dense_case(nC, nT=16, relax=True):
    v = dict(cases.fused_operand_variants(torch.float64, nC, nT)['gamma_split'][1])
    if not relax:
        v['T1'] = v['T2'] = None
    return v


@pytest.mark.parametrize('nC', [0, 1])
def test_leaf_chain_is_the_column_yardstick(nC):
    r"""The values of the chain with leaves are ``oracle_ab_columns``' (1e-12), and its pulse gradients are the same
    function's (the explicit pass)."""
    v = _dense_case(nC, 48)
    A, B = oracle_ab_columns(v)
    got = oracle_ab_spin_grads(v)
    assert float((got['A'] - A).abs().max()) <= 1e-12 and float((got['B'] - B).abs().max()) <= 1e-12
    from test_ab_rfgr_host import oracle_ab_grads
    ref = oracle_ab_grads(v)
    for k in ('rf', 'gr'):
        assert float((got[k] - ref['grad_' + k]).abs().max()) <= 1e-9, k


FD_AT = ((0, 3), (1, 64), (1, 139))


@pytest.mark.parametrize('nC', [0, 1])
@pytest.mark.parametrize('relax', [True, False])
def test_yardstick_against_finite_differences(nC, relax):
    r"""Central differences in fp64 on three spins (mid-wave, the first lane of the second tile, the last spin) for every
    spin-side operand.  Spins are independent, so a per-spin operand is differenced on its own spin's share of the
    loss, which is O(1): with a relative step of 1e-4 (absolute 1e-4 cm on ``loc``, 1e-2 Hz on ``Δf``) the truncation
    error is O(h²) = 1e-8 relative and the rounding error 2e-16 / h = 2e-12 absolute.  Bound: 1e-6 relative to the
    larger of the difference and a thousandth of the largest gradient element of that operand."""
    v = _dense_case(nC, 16, relax)
    wA, wB = ab_weights(v)
    got = oracle_ab_spin_grads(v, wA, wB)

    def loss(at, **moved):
        with torch.no_grad():
            A, B = oracle_ab_columns(dict(v, **moved))
            return float((A[at] * wA[at]).sum() + (B[at] * wB[at]).sum())

    names = ['loc', 'Δf', 'γ_beff', 'γ'] + (['b1Map'] if nC else []) + (['T1', 'T2'] if relax else [])
    for k in names:
        x0 = v[k].clone()
        assert tuple(x0.shape[:2]) == (2, 140), k
        for n, s in FD_AT:
            for c in range(x0.shape[2] if x0.ndim >= 3 else 1):
                at = (n, s, c) + (0,) * (x0.ndim - 3) if x0.ndim >= 3 else (n, s)      # (b1Map: a coil axis of 1)
                h = 1e-4 if k == 'loc' else 1e-2 if k == 'Δf' else 1e-4 * abs(float(x0[at]))
                up, dn = x0.clone(), x0.clone()
                up[at] += h
                dn[at] -= h
                fd = (loss((n, s), **{k: up}) - loss((n, s), **{k: dn})) / (2 * h)
                g = float(got[k][at])
                scale = max(abs(fd), float(got[k].abs().max()) * 1e-3)
                assert abs(fd - g) <= 1e-6 * scale, (k, at, fd, g)
    # dt: one value for the batch entry; the yardstick's per-spin terms summed
    for n in (0, 1):
        dt = v['dt'].reshape(-1).expand(2).clone()
        h = 1e-6 * float(dt[n])
        up, dn = dt.clone(), dt.clone()
        up[n] += h
        dn[n] -= h
        fd = (loss(n, dt=up) - loss(n, dt=dn)) / (2 * h)
        g = float(got['dt'][n].sum())
        assert abs(fd - g) <= 1e-6 * float(got['dt'][n].abs().sum()), ('dt', n, fd, g)
    if not relax:
        assert 'T1' not in got and 'T2' not in got
