r"""``fused.blochsim_rfgr_moving`` (K2v / K2vb): spins at constant velocity, forward and adjoint w.r.t. ``Mi``, ``rf``, ``gr``.

The yardstick is the CPU oracle (``bloch_oracle``) run in fp64 on the operands as given (fp32 operands widened): its
``rfgr2beff`` at the static ``loc``, with ``(gr_t . vel dt)(step0 + t + 1/2)`` added to the z component here, then its
``blochsim`` -- never the library's own composed route.  Gates: ``util.ATOL64`` elementwise in fp64, ``util.REL32``
(relative L2) in fp32 precise; the fast mode's distances go to the ledger unasserted.

Problem: N = 2 with a pulse per entry, nM = 343 (7^3: five full tiles and a ragged one of 23 lanes), nT = 48; velocities
seeded uniform with ``|vel dt| <= 0.02 cm`` per step.  On this problem the oracle's ``Mo`` moves by 0.14 (relative L2) and
its gradients by 0.14 .. 0.26 against the static result (CPU dry run, every variant), so a kernel that ignores ``vel``, uses ``t`` for ``t + 1/2`` or drops
``step0`` is four orders above the gate.  The loss weights are those of the existing fused tests
(``test_fused_traj._weights``); the static ``blochsim_rfgr`` on the same problem at ``vel = 0`` is recorded next to every
gated distance (``...static_vs_oracle``), so that a distance near the gate can be told from the oracle's own fp32 loss."""
import functools
from math import pi as π

import pytest

from gpu_common import *  # noqa: F401,F403
from test_fused_traj import _problem, _kw, _weights
from test_fused_tiles import _shape
from util import ATOL64, REL32

pytestmark = pytest.mark.gpu

N, NM, NT, WAVE = 2, 343, 48, 64
DT_STEP = 4e-6                                                   # test_fused_traj._problem's dt
VARIANTS = ['plain', 'b1map', 'norelax', 'b1map_norelax']
MODES = [('f64', 'precise'), ('f32', 'precise'), ('f32', 'fast')]


@functools.lru_cache(maxsize=None)
def _prob(tag, variant, nT, nM=NM):
    r"""``test_fused_traj._problem``'s operands (CPU, the data dtype; read-only) and seeded velocities ``vel`` (N, nM, 3)."""
    Q = dict(_problem(tag, 'b1map' if variant.startswith('b1map') else 'plain', nT, N=N, nM=nM))
    if variant.endswith('norelax'):
        Q['T1'] = Q['T2'] = None
    gen = torch.Generator().manual_seed(101 + nT)
    Q['vel'] = ((torch.rand(N, nM, 3, generator=gen, dtype=torch.float64) * 2 - 1) * (0.02 / DT_STEP)).to(DT[tag])
    return Q


def _wide(Q):
    return {k: (None if x is None else x.double()) for k, x in Q.items()}


def _oracle_Mo(Q64, Mi, rf, gr, vel, step0=0, loc=None, df='own'):
    r"""The yardstick's forward in fp64 (module docstring); differentiable w.r.t. every tensor argument."""
    loc = Q64['loc'] if loc is None else loc
    df = Q64['df'] if isinstance(df, str) else df
    be = O.rfgr2beff(rf, gr, loc, Δf=df, b1Map=Q64['b1'], γ=Q64['γ'])
    nT, lead = gr.shape[2], tuple(loc.shape[:-1])
    w = (vel * Q64['dt']).expand(loc.shape)
    τ = torch.arange(nT, dtype=torch.float64) + (step0 + 0.5)
    z = torch.einsum('nsi,nit->nst', w.reshape(lead[0], -1, 3), gr.expand(lead[0], 3, nT)) * τ
    be = be + torch.nn.functional.pad(z.reshape(lead + (nT, 1)), (2, 0))
    return O.blochsim(Mi, be, T1=Q64['T1'], T2=Q64['T2'], γ=Q64['γ'], dt=Q64['dt'])


def _oracle_run(Q, w, vel=None, spins=slice(None), step0=0):
    r"""``Mo, grad_Mi, grad_rf, grad_gr`` of ``sum(Mo w)`` by the oracle on the spins ``spins``; ``vel = None``: the problem's."""
    Q64 = _wide(Q)
    Q64 = {k: (x[:, spins] if k in ('M0', 'loc', 'df', 'b1', 'T1', 'T2', 'vel') and x is not None else x)
           for k, x in Q64.items()}
    Mi, r, g = (Q64[k].clone().requires_grad_(True) for k in ('M0', 'rf', 'gr'))
    with mrphy_amd.constants_on('cpu'):
        Mo = _oracle_Mo(Q64, Mi, r, g, Q64['vel'] if vel is None else vel.double()[:, spins], step0)
        (Mo * w.double()[:, spins]).sum().backward()
    return dict(Mo=Mo.detach(), grad_Mi=Mi.grad, grad_rf=r.grad, grad_gr=g.grad)


@functools.lru_cache(maxsize=None)
def _oracle(tag, variant, nT, static=False):
    Q = _prob(tag, variant, nT)
    return _oracle_run(Q, _weights((N, NM, 3), DT[tag]), vel=torch.zeros_like(Q['vel']) if static else None)


def _gpu_run(Q, w, vel='own', step0=0, sl=slice(None), Mi=None, **over):
    r"""The same four through ``fused.blochsim_rfgr_moving``; ``vel = None`` runs the static ``fused.blochsim_rfgr``; ``sl``: the
    steps played; ``w = None``: the forward alone."""
    Mi = dev(Q['M0']).clone().requires_grad_(True) if Mi is None else Mi
    r, g = (dev(Q[k]).clone().requires_grad_(True) for k in ('rf', 'gr'))
    kw = dict(_kw(Q, dev), **over)
    if vel is None:
        Mo = fused.blochsim_rfgr(Mi, r[:, :, sl], g[:, :, sl], dev(Q['loc']), **kw)
    else:
        v = dev(Q['vel']) if isinstance(vel, str) else vel
        Mo = fused.blochsim_rfgr_moving(Mi, r[:, :, sl], g[:, :, sl], dev(Q['loc']), v, step0=step0, **kw)
    if w is None:
        return dict(Mo=Mo, rf=r, gr=g)
    (Mo * dev(w)).sum().backward()
    return dict(Mo=Mo.detach(), grad_Mi=Mi.grad, grad_rf=r.grad, grad_gr=g.grad)


def _over_gate(a, b, tag):
    assert a.shape == b.shape, (a.shape, b.shape)
    return max_abs(a, b) / ATOL64 if tag == 'f64' else rel_l2(a, b) / REL32


def _gate(led, got, want, tag, mode, keys=None):
    r"""Every distance to the ledger, in units of the gate; asserted in the precise modes."""
    dist = {k: _over_gate(got[k], want[k], tag) for k in (keys or want)}
    note = ', '.join(f'{k} {x:.3f}' for k, x in dist.items())
    if mode == 'precise':
        record(f'{led}.over_gate', max(dist.values()), 1.0, note=note)
        for k, x in dist.items():
            assert x <= 1.0, f'{led}: {k} is {x:.3e} of the gate from the yardstick'
    else:
        record(f'{led}.over_precise_gate', max(dist.values()), note='not asserted: ' + note)
    return dist


# ---------------------------------------------------------------------------------------------
# 1. vel = 0: blochsim_rfgr's bits
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('variant', VARIANTS)
def test_zero_velocity_gives_the_static_bits(tag, mode, variant):
    r"""``fma(0, tau, loc)`` is ``loc`` and every other expression is K2's / K2b's: ``Mo`` at nT = 0, 5, 37, 48 (no step, a
    tail only, batches and a tail, whole segments) and the three gradients at nT = 48 are ``blochsim_rfgr``'s bits."""
    with mrphy_amd.precision(mode):
        for nT in (0, 5, 37, NT):
            Q = _prob(tag, variant, nT)
            zero = torch.zeros_like(dev(Q['vel']))
            with torch.no_grad():
                mv, st = _gpu_run(Q, None, vel=zero)['Mo'], _gpu_run(Q, None, vel=None)['Mo']
            assert torch.equal(mv, st), (nT, 'Mo')
            if nT == 0:
                assert torch.equal(mv, dev(Q['M0']))
        w = _weights((N, NM, 3), DT[tag])
        mv, st = _gpu_run(Q, w, vel=zero), _gpu_run(Q, w, vel=None)
        for k in st:
            assert torch.equal(mv[k], st[k]), k


# ---------------------------------------------------------------------------------------------
# 2. the oracle, at the velocities of the module docstring
# ---------------------------------------------------------------------------------------------
@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('variant', VARIANTS)
def test_oracle_parity(tag, mode, variant):
    r"""``Mo`` at nT = 37 and 48 and the three gradients at nT = 48 against the oracle; the static call at ``vel = 0``
    against the static oracle is recorded beside them (module docstring), and so is how far motion moves the result."""
    led = f'moving.{tag}.{mode}.{variant}'
    w = _weights((N, NM, 3), DT[tag])
    with mrphy_amd.precision(mode):
        Q = _prob(tag, variant, 37)
        with torch.no_grad():
            Mo = _gpu_run(Q, None)['Mo']
        _gate(f'{led}.nT37', dict(Mo=Mo), _oracle(tag, variant, 37), tag, mode, keys=['Mo'])
        Q = _prob(tag, variant, NT)
        ora, ora0 = _oracle(tag, variant, NT), _oracle(tag, variant, NT, static=True)
        st = _gpu_run(Q, w, vel=None)
        record(f'{led}.nT48.static_vs_oracle.over_gate', max(_over_gate(st[k], ora0[k], tag) for k in ora0),
               note=', '.join(f'{k} {_over_gate(st[k], ora0[k], tag):.3f}' for k in ora0))
        record(f'{led}.nT48.oracle_moving_vs_static.rel_l2', max(rel_l2(ora[k], ora0[k]) for k in ('Mo', 'grad_rf', 'grad_gr')),
               note=', '.join(f'{k} {rel_l2(ora[k], ora0[k]):.3f}' for k in ora))
        got = _gpu_run(Q, w)
        for k, x in got.items():
            assert bool(torch.isfinite(x).all()), k
        _gate(f'{led}.nT48', got, ora, tag, mode)


# ---------------------------------------------------------------------------------------------
# 3. known answer
# ---------------------------------------------------------------------------------------------
@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('b1map', [False, True])
def test_bipolar_gradient_known_answer(b1map):
    r"""``rf = 0``, no relaxation, no off-resonance, fp64, a bipolar gradient (+G for 24 steps, -G for 24; a G per batch
    entry): its zeroth moment is zero, so static spins return to ``Mi``; moving spins are rotated about z by the closed
    form ``-2 pi gamma dt (m1 . vel dt)``, ``m1 = sum_t gr_t (t + 1/2)``.  Both within ``ATOL64``."""
    Q = dict(_prob('f64', 'b1map_norelax' if b1map else 'norelax', NT))
    G = torch.tensor([[0.7, -0.4, 1.1], [-0.9, 0.5, 0.3]], dtype=torch.float64)
    sign = torch.cat((torch.ones(NT // 2), -torch.ones(NT // 2))).double()
    Q['gr'], Q['rf'], Q['df'] = G[:, :, None] * sign, torch.zeros(N, 2, NT, dtype=torch.float64), None
    with torch.no_grad():
        still = _gpu_run(Q, None, vel=torch.zeros_like(dev(Q['vel'])))['Mo']
        moved = _gpu_run(Q, None)['Mo']
    d0 = record(f'moving.known_answer.b1map{int(b1map)}.static.max_abs', max_abs(still, Q['M0']), ATOL64)
    τ = torch.arange(NT, dtype=torch.float64) + 0.5
    m0, m1 = Q['gr'].sum(-1), (Q['gr'] * τ).sum(-1)                                  # (N, 3)
    assert float(m0.abs().max()) == 0.0
    φ = -2 * π * Q['γ'] * Q['dt'] * ((m1[:, None, :] * (Q['vel'] * Q['dt'])).sum(-1))     # (N, nM)
    Mx, My, Mz = Q['M0'].unbind(-1)
    want = torch.stack((Mx * torch.cos(φ) - My * torch.sin(φ), Mx * torch.sin(φ) + My * torch.cos(φ), Mz), dim=-1)
    assert rel_l2(want, Q['M0']) > 0.1                                               # the phases are not small
    d1 = record(f'moving.known_answer.b1map{int(b1map)}.moving.max_abs', max_abs(moved, want), ATOL64)
    assert d0 <= ATOL64 and d1 <= ATOL64, (d0, d1)


# ---------------------------------------------------------------------------------------------
# 4. step0
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('variant', VARIANTS)
def test_chained_calls_through_step0(tag, mode, variant):
    r"""Steps 0 .. 31, then steps 32 .. 47 with ``step0 = 32``: ``Mo`` is the single 48-step call's bit for bit (with and
    without checkpoints), and the gradients through the chain are the single call's within the gate.  A second call that
    forgets ``step0`` is not."""
    Q, w = _prob(tag, variant, NT), _weights((N, NM, 3), DT[tag])
    with mrphy_amd.precision(mode):
        with torch.no_grad():
            one = _gpu_run(Q, None)['Mo']
            M1 = _gpu_run(Q, None, sl=slice(0, 32))['Mo']
            two = _gpu_run(Q, None, sl=slice(32, NT), step0=32, Mi=M1)['Mo']
            wrong = _gpu_run(Q, None, sl=slice(32, NT), step0=0, Mi=M1)['Mo']
        assert torch.equal(one, two)
        assert rel_l2(wrong, one) > 1e-2
        single = _gpu_run(Q, w)
        # the chain with gradients: one graph over both calls
        Mi, r, g = (dev(Q[k]).clone().requires_grad_(True) for k in ('M0', 'rf', 'gr'))
        kw, loc, vel = _kw(Q, dev), dev(Q['loc']), dev(Q['vel'])
        M1 = fused.blochsim_rfgr_moving(Mi, r[:, :, :32], g[:, :, :32], loc, vel, **kw)
        M2 = fused.blochsim_rfgr_moving(M1, r[:, :, 32:], g[:, :, 32:], loc, vel, step0=32, **kw)
        assert torch.equal(M2.detach(), single['Mo'])
        (M2 * dev(w)).sum().backward()
        chain = dict(Mo=M2.detach(), grad_Mi=Mi.grad, grad_rf=r.grad, grad_gr=g.grad)
    dist = {k: _over_gate(chain[k], single[k].cpu(), tag) for k in single}
    record(f'moving.{tag}.{mode}.{variant}.chain_vs_single.over_gate', max(dist.values()), 1.0)
    assert max(dist.values()) <= 1.0, dist


# ---------------------------------------------------------------------------------------------
# 5. more tiles than persistent waves
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tile_weights(tag, loss):
    P, nM = _shape(tag)
    w = torch.sin(torch.arange(N * nM * 3, dtype=torch.float64) * 0.61 + 1.0).reshape(N, nM, 3)
    if loss == 'tail':
        w[:, :P * WAVE] = 0
    return w.to(DT[tag])


@functools.lru_cache(maxsize=None)
def _tile_oracle(tag, variant, loss):
    P, nM = _shape(tag)
    Q = _prob(tag, variant, 32, nM)
    return _oracle_run(Q, _tile_weights(tag, loss), spins=slice(None) if loss == 'full' else slice(nM - 136, nM))


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('variant', ['plain', 'b1map'])
def test_adjoint_wave_takes_a_second_tile(tag, mode, variant):
    r"""``tests/test_fused_tiles.py``'s shape for K2vb: N = 2, nT = 32, nM = P 64 + 100 with ``P`` the adjoint's cap on its
    persistent waves (from the workspace query), so waves 0 and 1 take a second tile (the last one ragged) and add its row
    sums into their workspace rows by read-modify-write.  Full weights: everything against the oracle.  Tail-only weights
    (zero on the tiles ``< P``): ``grad_rf`` / ``grad_gr`` against the oracle on the last 136 spins alone -- a wrong position
    on a second tile is not diluted by 131 072 right ones."""
    P, nM = _shape(tag)
    t0 = P * WAVE
    Q = _prob(tag, variant, 32, nM)
    with mrphy_amd.precision(mode):
        for loss in ('full', 'tail'):
            got, ora = _gpu_run(Q, _tile_weights(tag, loss)), _tile_oracle(tag, variant, loss)
            led = f'moving.tiles.{tag}.{mode}.{variant}.{loss}'
            if loss == 'full':
                _gate(led, got, ora, tag, mode)
            else:
                assert float(ora['grad_Mi'][:, :36].abs().max()) == 0.0
                assert float(got['grad_Mi'][:, :t0].abs().max()) == 0.0
                _gate(led, dict(got, tail_Mo=got['Mo'][:, t0:], tail_grad_Mi=got['grad_Mi'][:, t0:]),
                      dict(grad_rf=ora['grad_rf'], grad_gr=ora['grad_gr'], tail_Mo=ora['Mo'][:, 36:],
                           tail_grad_Mi=ora['grad_Mi'][:, 36:]), tag, mode)


# ---------------------------------------------------------------------------------------------
# 6. routes
# ---------------------------------------------------------------------------------------------
@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('variant', ['plain', 'b1map_norelax'])
def test_split_route(tag, mode, variant):
    r"""nT = 40 with a pulse gradient: 32 fused steps, then 8 composed at ``step0 = 32``."""
    Q, w = _prob(tag, variant, 40), _weights((N, NM, 3), DT[tag])
    with mrphy_amd.precision(mode):
        got = _gpu_run(Q, w)
    _gate(f'moving.split.{tag}.{mode}.{variant}', got, _oracle_run(Q, w), tag, mode)


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
def test_composed_route_spin_side_gradients(tag, mode):
    r"""Gradients w.r.t. ``vel``, ``loc`` and ``Δf`` (the composed route) against the oracle's autograd."""
    Q, w = _prob(tag, 'b1map', NT), _weights((N, NM, 3), DT[tag])
    Q64 = _wide(Q)
    leaves = {k: Q64[k].clone().requires_grad_(True) for k in ('vel', 'loc', 'df', 'rf')}
    with mrphy_amd.constants_on('cpu'):
        Mo = _oracle_Mo(Q64, Q64['M0'], leaves['rf'], Q64['gr'], leaves['vel'], loc=leaves['loc'], df=leaves['df'])
        (Mo * w.double()).sum().backward()
    want = dict(Mo=Mo.detach(), **{'grad_' + k: x.grad for k, x in leaves.items()})
    gl = {k: dev(Q[k]).clone().requires_grad_(True) for k in leaves}
    with mrphy_amd.precision(mode):
        kw = dict(_kw(Q, dev), Δf=gl['df'])
        Mo = fused.blochsim_rfgr_moving(dev(Q['M0']), gl['rf'], dev(Q['gr']), gl['loc'], gl['vel'], **kw)
        (Mo * dev(w)).sum().backward()
    got = dict(Mo=Mo.detach(), **{'grad_' + k: x.grad for k, x in gl.items()})
    _gate(f'moving.composed.{tag}.{mode}.spin_side', got, want, tag, mode)


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
def test_composed_route_two_transmit_coils(tag, mode):
    r"""Parallel transmit is composed: two coils with their ``b1Map``, forward and pulse gradients against the oracle."""
    Q, w = dict(_prob(tag, 'plain', NT)), _weights((N, NM, 3), DT[tag])
    gen = torch.Generator().manual_seed(7)
    Q['rf'] = ((torch.rand(N, 2, NT, 2, generator=gen, dtype=torch.float64) * 2 - 1) * 1.5).to(DT[tag])
    Q['b1'] = ((torch.rand(N, NM, 2, 2, generator=gen, dtype=torch.float64) * 2 - 1) * 0.7).to(DT[tag])
    with mrphy_amd.precision(mode):
        got = _gpu_run(Q, w)
    assert got['grad_rf'].shape == Q['rf'].shape
    _gate(f'moving.composed.{tag}.{mode}.two_coils', got, _oracle_run(Q, w), tag, mode)


# ---------------------------------------------------------------------------------------------
# 7. operand forms
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('variant', ['plain', 'b1map'])
def test_velocity_operand_forms(tag, mode, variant):
    r"""``vel`` as `(1, *Nd, 3)` against N = 2, as a stride-0 expanded view of that, as a permuted view, and the whole call
    with ``Nd = (7, 7, 7)``: each gives the bits of the contiguous `(N, nM, 3)` call, forward and backward."""
    Q, w = _prob(tag, variant, NT), _weights((N, NM, 3), DT[tag])
    one = Q['vel'][:1].clone()
    with mrphy_amd.precision(mode):
        ref1 = _gpu_run(Q, w, vel=dev(one.expand(N, NM, 3).contiguous()))
        for name, v in (('one', one), ('expanded', one.expand(N, NM, 3))):
            x = place(v)
            assert x.stride() == v.stride()
            got = _gpu_run(Q, w, vel=x)
            for k in ref1:
                assert torch.equal(got[k], ref1[k]), (name, k)
        ref = _gpu_run(Q, w)
        perm = Q['vel'].permute(2, 0, 1).contiguous().permute(1, 2, 0)
        assert not perm.is_contiguous() and torch.equal(perm, Q['vel'])
        x = place(perm)
        assert x.stride() == perm.stride()
        got = _gpu_run(Q, w, vel=x)
        for k in ref:
            assert torch.equal(got[k], ref[k]), ('permuted', k)
        # Nd = (7, 7, 7)
        cube = lambda x, *tail: None if x is None else dev(x).reshape((N, 7, 7, 7) + tail)  # noqa: E731
        Mi, r, g = dev(Q['M0']).reshape(N, 7, 7, 7, 3).clone().requires_grad_(True), dev(Q['rf']).clone().requires_grad_(True), \
            dev(Q['gr']).clone().requires_grad_(True)
        kw = dict(_kw(Q, dev), Δf=cube(Q['df']), b1Map=cube(Q['b1'], 2), T1=cube(Q['T1']), T2=cube(Q['T2']))
        Mo = fused.blochsim_rfgr_moving(Mi, r, g, cube(Q['loc'], 3), cube(Q['vel'], 3), **kw)
        assert Mo.shape == (N, 7, 7, 7, 3)
        (Mo * dev(w).reshape(Mo.shape)).sum().backward()
        for k, x in (('Mo', Mo.detach()), ('grad_Mi', Mi.grad), ('grad_rf', r.grad), ('grad_gr', g.grad)):
            assert torch.equal(x.reshape(ref[k].shape), ref[k]), ('Nd = (7, 7, 7)', k)


# ---------------------------------------------------------------------------------------------
# 8. determinism
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,mode', MODES)
def test_two_identical_calls_give_identical_bits(tag, mode):
    Q, w = _prob(tag, 'b1map', NT), _weights((N, NM, 3), DT[tag])
    with mrphy_amd.precision(mode):
        a, b = _gpu_run(Q, w), _gpu_run(Q, w)
    for k in a:
        assert torch.equal(a[k], b[k]), k
