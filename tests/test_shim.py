r"""``fused.blochsim_rfgr_shim`` (K2sh / K2shb): extra Bz field channels, forward and adjoint w.r.t. ``Mi``, ``rf``, ``gr``, ``sh``.

The yardstick is the CPU oracle (``bloch_oracle``) run in fp64 on the operands as given (fp32 operands widened): its
``rfgr2beff`` at ``loc``, with ``einsum('nmk,nkt->nmt', shMap, sh)`` added to the z component here, then its ``blochsim`` --
never the library's own composed route.  Gates: ``util.ATOL64`` elementwise in fp64, ``util.REL32`` (relative L2) in fp32
precise; the fast mode's distances go to the ledger unasserted.

Problem: ``test_fused_traj._problem`` with N = 2 and a pulse per entry, nM = 343 (7^3: five full tiles and a ragged one of
23 lanes), nT = 48; ``sh`` seeded uniform in +-1, ``shMap`` seeded uniform in +-2 G per unit; nS = 1, 3, 5, 8 (one below the
smallest capacity, one inside each capacity, the largest full) are the first nS of nine seeded channels.  CPU dry run of
the oracle on exactly this problem: the channels move ``Mo`` by 0.38 .. 0.84 (relative L2) and the gradients by 0.36 .. 1.7
against the static result; dropping only the last channel moves ``Mo`` by 0.20 .. 0.48 and ``grad_sh`` by 0.27 .. 1.26 -- so
a kernel that ignores a channel, reads a wrong row of ``sh`` or skips a coefficient row is at least four orders above
either gate.  The loss weights are those of the existing fused tests (``test_fused_traj._weights``); the static
``blochsim_rfgr`` on the same problem is recorded next to every gated distance (``...static_vs_oracle``), so that a distance
near the gate can be told from the oracle's own fp32 loss."""
import collections
import functools
from math import pi as π

import pytest

from gpu_common import *  # noqa: F401,F403
from mrphy_amd import _host
from test_fused_traj import _problem, _kw, _weights
from test_moving import _prob as _moving_prob, _over_gate, _gate
from util import ATOL64, REL32  # noqa: F401

pytestmark = pytest.mark.gpu

N, NM, NT, WAVE = 2, 343, 48, 64
NCH = 9                                                          # channels drawn: the capacity and one more
VARIANTS = ['plain', 'b1map', 'norelax', 'b1map_norelax']
MODES = [('f64', 'precise'), ('f32', 'precise'), ('f32', 'fast')]
GRADS = ('grad_Mi', 'grad_rf', 'grad_gr', 'grad_sh')


@functools.lru_cache(maxsize=None)
def _prob(tag, variant, nT, nM=NM):
    r"""``test_fused_traj._problem``'s operands (CPU, the data dtype; read-only) and nine seeded channels: ``sh`` (N, 9, nT) in
    +-1, ``map`` (N, nM, 9) in +-2."""
    Q = dict(_problem(tag, 'b1map' if variant.startswith('b1map') else 'plain', nT, N=N, nM=nM))
    if variant.endswith('norelax'):
        Q['T1'] = Q['T2'] = None
    gen = torch.Generator().manual_seed(211 + nT)
    Q['sh'] = (torch.rand(N, NCH, nT, generator=gen, dtype=torch.float64) * 2 - 1).to(DT[tag])
    Q['map'] = ((torch.rand(N, nM, NCH, generator=gen, dtype=torch.float64) * 2 - 1) * 2).to(DT[tag])
    return Q


def _wide(Q):
    return {k: (None if x is None else x.double()) for k, x in Q.items()}


def _oracle_Mo(Q64, Mi, rf, gr, sh, shMap, loc=None):
    r"""The yardstick's forward in fp64 (module docstring); differentiable w.r.t. every tensor argument."""
    loc = Q64['loc'] if loc is None else loc
    be = O.rfgr2beff(rf, gr, loc, Δf=Q64['df'], b1Map=Q64['b1'], γ=Q64['γ'])
    if sh is not None:
        z = torch.einsum('nmk,nkt->nmt', shMap, sh)
        be = be + torch.nn.functional.pad(z.unsqueeze(-1), (2, 0))
    return O.blochsim(Mi, be, T1=Q64['T1'], T2=Q64['T2'], γ=Q64['γ'], dt=Q64['dt'])


def _oracle_run(Q, w, nS, spins=slice(None)):
    r"""``Mo, grad_Mi, grad_rf, grad_gr, grad_sh`` of ``sum(Mo w)`` by the oracle on the spins ``spins`` with the first ``nS``
    channels; ``nS = 0``: the static problem (no ``grad_sh``)."""
    Q64 = _wide(Q)
    Q64 = {k: (x[:, spins] if k in ('M0', 'loc', 'df', 'b1', 'T1', 'T2', 'map') and x is not None else x)
           for k, x in Q64.items()}
    Mi, r, g = (Q64[k].clone().requires_grad_(True) for k in ('M0', 'rf', 'gr'))
    s = Q64['sh'][:, :nS].clone().requires_grad_(True) if nS else None
    with mrphy_amd.constants_on('cpu'):
        Mo = _oracle_Mo(Q64, Mi, r, g, s, Q64['map'][..., :nS])
        (Mo * w.double()[:, spins]).sum().backward()
    out = dict(Mo=Mo.detach(), grad_Mi=Mi.grad, grad_rf=r.grad, grad_gr=g.grad)
    return dict(out, grad_sh=s.grad) if nS else out


@functools.lru_cache(maxsize=None)
def _oracle(tag, variant, nT, nS):
    return _oracle_run(_prob(tag, variant, nT), _weights((N, NM, 3), DT[tag]), nS)


def _gpu_run(Q, w, nS, sh=None, shMap=None, **over):
    r"""The same five through ``fused.blochsim_rfgr_shim`` with the first ``nS`` channels, or with ``sh`` / ``shMap`` as given
    (device tensors; an ``sh`` that requires grad is the leaf itself, passed in the form it has); ``nS = None`` runs the static
    ``fused.blochsim_rfgr``; ``w = None``: the forward alone."""
    Mi, r, g = (dev(Q[k]).clone().requires_grad_(True) for k in ('M0', 'rf', 'gr'))
    kw = dict(_kw(Q, dev), **over)
    if nS is None:
        s = None
        Mo = fused.blochsim_rfgr(Mi, r, g, dev(Q['loc']), **kw)
    else:
        # a leaf handed in (requires_grad) goes to the call as it is, in its own strides; anything else is copied to one
        s = sh if sh is not None and sh.requires_grad else \
            (dev(Q['sh'][:, :nS]) if sh is None else sh).clone().requires_grad_(True)
        m = dev(Q['map'][..., :nS].contiguous()) if shMap is None else shMap
        Mo = fused.blochsim_rfgr_shim(Mi, r, g, dev(Q['loc']), s, m, **kw)
    if w is None:
        return dict(Mo=Mo)
    (Mo * dev(w)).sum().backward()
    out = dict(Mo=Mo.detach(), grad_Mi=Mi.grad, grad_rf=r.grad, grad_gr=g.grad)
    return out if s is None else dict(out, grad_sh=s.grad)


# ---------------------------------------------------------------------------------------------
# 1. zero channels: blochsim_rfgr's bits
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('nS', [3, 8])
def test_zero_channels_give_the_static_bits(tag, mode, variant, nS):
    r"""``fma(0, m, Bz)`` and ``fma(s, 0, Bz)`` are ``Bz`` and every other expression is K2's / K2b's: with zero waveforms and
    a map, and with waveforms and a zero map, ``Mo`` at nT = 0, 5, 37, 48 (no step, a tail only, batches and a tail, whole
    segments) and ``grad_Mi``, ``grad_rf``, ``grad_gr`` at nT = 48 are ``blochsim_rfgr``'s bits."""
    with mrphy_amd.precision(mode):
        for nT in (0, 5, 37, NT):
            Q = _prob(tag, variant, nT)
            zero_sh = dict(sh=torch.zeros_like(dev(Q['sh'][:, :nS])))
            zero_map = dict(shMap=torch.zeros_like(dev(Q['map'][..., :nS].contiguous())))
            with torch.no_grad():
                st = _gpu_run(Q, None, None)['Mo']
                for name, z in (('sh = 0', zero_sh), ('shMap = 0', zero_map)):
                    assert torch.equal(_gpu_run(Q, None, nS, **z)['Mo'], st), (nT, name, 'Mo')
            if nT == 0:
                assert torch.equal(st, dev(Q['M0']))
        w = _weights((N, NM, 3), DT[tag])
        st = _gpu_run(Q, w, None)
        for name, z in (('sh = 0', zero_sh), ('shMap = 0', zero_map)):
            got = _gpu_run(Q, w, nS, **z)
            for k in st:
                assert torch.equal(got[k], st[k]), (name, k)
            assert got['grad_sh'].shape == (N, nS, NT)
        assert float(got['grad_sh'].abs().max()) == 0.0              # a zero map: no gradient w.r.t. its waveform


# ---------------------------------------------------------------------------------------------
# 2. all-zero channels appended: no bit changes, across capacities
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('variant', VARIANTS)
def test_zero_padding_across_capacities(tag, mode, variant):
    r"""nS = 3 with 0, 1, 2 and 5 all-zero channels appended (capacities 4, 4, 8, 8) and nS = 1 with 0 and 1 appended
    (capacity 2 both): ``Mo``, ``grad_Mi``, ``grad_rf``, ``grad_gr`` and the real channels' ``grad_sh`` rows keep their bits."""
    Q, w = _prob(tag, variant, NT), _weights((N, NM, 3), DT[tag])
    with mrphy_amd.precision(mode):
        for nS, pads in ((3, (1, 2, 5)), (1, (1,))):
            ref = _gpu_run(Q, w, nS)
            assert float(ref['grad_sh'].abs().min()) > 0.0
            for pad in pads:
                sh = torch.cat((dev(Q['sh'][:, :nS]), torch.zeros(N, pad, NT, dtype=DT[tag], device=DEV)), dim=1)
                m = torch.cat((dev(Q['map'][..., :nS]), torch.zeros(N, NM, pad, dtype=DT[tag], device=DEV)), dim=2)
                got = _gpu_run(Q, w, nS + pad, sh=sh, shMap=m.contiguous())
                assert got['grad_sh'].shape == (N, nS + pad, NT)
                for k in ('Mo', 'grad_Mi', 'grad_rf', 'grad_gr'):
                    assert torch.equal(got[k], ref[k]), (nS, pad, k)
                assert torch.equal(got['grad_sh'][:, :nS], ref['grad_sh']), (nS, pad, 'grad_sh')


# ---------------------------------------------------------------------------------------------
# 3. the oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('nS', [1, 3, 5, 8])
def test_oracle_parity(tag, mode, variant, nS):
    r"""``Mo`` at nT = 37 and 48 and the four gradients at nT = 48 against the oracle; the static call against the static
    oracle is recorded beside them (module docstring), and so is how far the channels move the result."""
    led = f'shim.{tag}.{mode}.{variant}.nS{nS}'
    w = _weights((N, NM, 3), DT[tag])
    with mrphy_amd.precision(mode):
        Q = _prob(tag, variant, 37)
        with torch.no_grad():
            Mo = _gpu_run(Q, None, nS)['Mo']
        _gate(f'{led}.nT37', dict(Mo=Mo), _oracle(tag, variant, 37, nS), tag, mode, keys=['Mo'])
        Q = _prob(tag, variant, NT)
        ora, ora0 = _oracle(tag, variant, NT, nS), _oracle(tag, variant, NT, 0)
        st = _gpu_run(Q, w, None)
        record(f'{led}.nT48.static_vs_oracle.over_gate', max(_over_gate(st[k], ora0[k], tag) for k in ora0),
               note=', '.join(f'{k} {_over_gate(st[k], ora0[k], tag):.3f}' for k in ora0))
        record(f'{led}.nT48.oracle_shim_vs_static.rel_l2', max(rel_l2(ora[k], ora0[k]) for k in ('Mo', 'grad_rf', 'grad_gr')),
               note=', '.join(f'{k} {rel_l2(ora[k], ora0[k]):.3f}' for k in ora0))
        got = _gpu_run(Q, w, nS)
        assert got['grad_sh'].shape == Q['sh'][:, :nS].shape
        for k, x in got.items():
            assert bool(torch.isfinite(x).all()), k
        _gate(f'{led}.nT48', got, ora, tag, mode)


# ---------------------------------------------------------------------------------------------
# 4. known answer
# ---------------------------------------------------------------------------------------------
@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('b1map', [False, True])
@pytest.mark.parametrize('nS', [3, 8])
def test_precession_known_answer(b1map, nS):
    r"""``rf = 0``, no relaxation, fp64: the transverse magnetisation is rotated about z by
    ``-2 pi gamma dt (m0 . loc + sum_k (sum_t sh[k, t]) shMap[k] + nT df / gamma_beff)``, ``m0 = sum_t gr_t``, within
    ``ATOL64``; the channels' share of that phase is not small."""
    Q = dict(_prob('f64', 'b1map_norelax' if b1map else 'norelax', NT))
    Q['rf'] = torch.zeros(N, 2, NT, dtype=torch.float64)
    with torch.no_grad():
        got = _gpu_run(Q, None, nS)['Mo']
    m0, a = Q['gr'].sum(-1), Q['sh'][:, :nS].sum(-1)                                 # (N, 3), (N, nS)
    φ_lin = (m0[:, None, :] * Q['loc']).sum(-1) + NT * Q['df'] / Q['γ']
    φ_ch = (a[:, None, :] * Q['map'][..., :nS]).sum(-1)
    k = -2 * π * Q['γ'] * Q['dt']
    Mx, My, Mz = Q['M0'].unbind(-1)
    rot = lambda φ: torch.stack((Mx * torch.cos(φ) - My * torch.sin(φ), Mx * torch.sin(φ) + My * torch.cos(φ), Mz), -1)  # noqa: E731
    want = rot(k * (φ_lin + φ_ch))
    assert rel_l2(want, rot(k * φ_lin)) > 0.1                                        # the channels' phases are not small
    d = record(f'shim.known_answer.b1map{int(b1map)}.nS{nS}.max_abs', max_abs(got, want), ATOL64)
    assert d <= ATOL64, d


# ---------------------------------------------------------------------------------------------
# 5. two identities against the other fused kernels
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('variant', ['plain', 'b1map'])
def test_three_motion_channels_are_the_moving_call(tag, mode, variant):
    r"""nS = 3 with ``shMap = vel dt`` and ``sh[k, t] = gr[k, t] (t + 1/2)`` is ``blochsim_rfgr_moving``: ``Mo``, ``grad_Mi``,
    ``grad_rf`` and -- ``sh`` formed from ``gr`` in torch, so that autograd adds both paths -- ``grad_gr``, within the gates (the
    two round ``gr_t . pos_t`` differently)."""
    Q, w = _moving_prob(tag, variant, NT), _weights((N, NM, 3), DT[tag])
    kw, loc, vel = _kw(Q, dev), dev(Q['loc']), dev(Q['vel'])
    τ = (torch.arange(NT, dtype=torch.float64) + 0.5).to(DT[tag]).to(DEV)
    res = {}
    with mrphy_amd.precision(mode):
        for name in ('moving', 'shim'):
            Mi, r, g = (dev(Q[k]).clone().requires_grad_(True) for k in ('M0', 'rf', 'gr'))
            if name == 'moving':
                Mo = fused.blochsim_rfgr_moving(Mi, r, g, loc, vel, **kw)
            else:
                Mo = fused.blochsim_rfgr_shim(Mi, r, g, loc, g * τ, vel * dev(Q['dt']), **kw)
            (Mo * dev(w)).sum().backward()
            res[name] = dict(Mo=Mo.detach(), grad_Mi=Mi.grad, grad_rf=r.grad, grad_gr=g.grad)
    _gate(f'shim.identity.moving.{tag}.{mode}.{variant}', res['shim'], {k: x.cpu() for k, x in res['moving'].items()},
          tag, mode)


@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('variant', ['plain', 'b1map'])
def test_three_linear_channels_are_an_added_gradient(tag, mode, variant):
    r"""nS = 3 with ``shMap = loc`` and waveforms ``h`` is ``blochsim_rfgr(gr + h)``, whose ``grad_gr`` is then ``grad_sh`` (and
    ``grad_gr``), within the gates."""
    Q, w = _prob(tag, variant, NT), _weights((N, NM, 3), DT[tag])
    h = dev(Q['sh'][:, :3])
    with mrphy_amd.precision(mode):
        got = _gpu_run(Q, w, 3, sh=h, shMap=dev(Q['loc']))
        Q2 = dict(Q, gr=(Q['gr'].double() + Q['sh'][:, :3].double()).to(DT[tag]))
        ref = {k: x.cpu() for k, x in _gpu_run(Q2, w, None).items()}
    _gate(f'shim.identity.linear.{tag}.{mode}.{variant}', got, dict(ref, grad_sh=ref['grad_gr']), tag, mode)


# ---------------------------------------------------------------------------------------------
# 6. more tiles than persistent waves
# ---------------------------------------------------------------------------------------------
def _adjoint_waves(tag, nM, nS, nT=32):
    r"""K2shb's wave count for ``nM`` spins, from its workspace query (``(P, N, 5 + nS, nT)`` elements)."""
    lib = mrphy_amd.require_library()
    code = _host.dtype_code(DT[tag], DT[tag])
    return int(lib.mrphy_blochsim_rfgr_shim_bwd_workspace(code, N, nM, nT, nS)) // (N * (5 + nS) * nT * DT[tag].itemsize)


@functools.lru_cache(maxsize=None)
def _shape(tag, nS):
    P = _adjoint_waves(tag, 1 << 30, nS)
    nM = P * WAVE + 100
    assert _adjoint_waves(tag, nM, nS) == P and -(-nM // WAVE) == P + 2 > P, (P, nM)   # two waves take a second tile
    return P, nM


@functools.lru_cache(maxsize=None)
def _tile_weights(tag, nS, loss):
    P, nM = _shape(tag, nS)
    w = torch.sin(torch.arange(N * nM * 3, dtype=torch.float64) * 0.61 + 1.0).reshape(N, nM, 3)
    if loss == 'tail':
        w[:, :P * WAVE] = 0
    return w.to(DT[tag])


@functools.lru_cache(maxsize=None)
def _tile_oracle(tag, nS, loss):
    P, nM = _shape(tag, nS)
    Q = _prob(tag, 'b1map', 32, nM)
    return _oracle_run(Q, _tile_weights(tag, nS, loss), nS, spins=slice(None) if loss == 'full' else slice(nM - 136, nM))


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('nS', [3, 8])
def test_adjoint_wave_takes_a_second_tile(tag, mode, nS):
    r"""``test_moving.test_adjoint_wave_takes_a_second_tile``'s construction for K2shb: N = 2, nT = 32, nM = P 64 + 100 with
    ``P`` the cap on its persistent waves (from the new workspace query), so waves 0 and 1 take a second tile (the last one
    ragged) and add its sums into their workspace rows by read-modify-write.  Full weights: everything against the
    oracle.  Tail-only weights (zero on the tiles ``< P``): ``grad_rf``, ``grad_gr``, ``grad_sh`` against the oracle on the last
    136 spins alone -- a wrong coefficient row on a second tile is not diluted by 131 072 right ones."""
    P, nM = _shape(tag, nS)
    t0 = P * WAVE
    Q = _prob(tag, 'b1map', 32, nM)
    with mrphy_amd.precision(mode):
        for loss in ('full', 'tail'):
            got, ora = _gpu_run(Q, _tile_weights(tag, nS, loss), nS), _tile_oracle(tag, nS, loss)
            led = f'shim.tiles.{tag}.{mode}.nS{nS}.{loss}'
            if loss == 'full':
                _gate(led, got, ora, tag, mode)
            else:
                assert float(ora['grad_Mi'][:, :36].abs().max()) == 0.0
                assert float(got['grad_Mi'][:, :t0].abs().max()) == 0.0
                _gate(led, dict(got, tail_Mo=got['Mo'][:, t0:], tail_grad_Mi=got['grad_Mi'][:, t0:]),
                      dict(grad_rf=ora['grad_rf'], grad_gr=ora['grad_gr'], grad_sh=ora['grad_sh'], tail_Mo=ora['Mo'][:, 36:],
                           tail_grad_Mi=ora['grad_Mi'][:, 36:]), tag, mode)


# ---------------------------------------------------------------------------------------------
# 7. routes
# ---------------------------------------------------------------------------------------------
SHIM_ENTRIES = ('mrphy_blochsim_rfgr_shim_fwd', 'mrphy_blochsim_rfgr_shim_bwd')


def _counted(monkeypatch):
    lib = mrphy_amd.require_library()
    calls = collections.Counter()

    def wrap(name, fn):
        def counted(*a):
            calls[name] += 1
            return fn(*a)
        return counted
    for name in SHIM_ENTRIES:
        monkeypatch.setattr(lib, name, wrap(name, getattr(lib, name)))
    return calls


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('variant', ['plain', 'b1map_norelax'])
def test_split_route(tag, mode, variant, monkeypatch):
    r"""nT = 40 with a pulse gradient: 32 fused steps (one forward and one adjoint launch), then 8 composed."""
    Q, w = _prob(tag, variant, 40), _weights((N, NM, 3), DT[tag])
    calls = _counted(monkeypatch)
    with mrphy_amd.precision(mode):
        got = _gpu_run(Q, w, 5)
    assert dict(calls) == {n: 1 for n in SHIM_ENTRIES}, dict(calls)
    _gate(f'shim.split.{tag}.{mode}.{variant}', got, _oracle_run(Q, w, 5), tag, mode)


def test_fused_route_calls_each_entry_point_once(monkeypatch):
    Q, w = _prob('f32', 'b1map', NT), _weights((N, NM, 3), DT['f32'])
    calls = _counted(monkeypatch)
    for nS in (1, 3, 5, 8):
        calls.clear()
        _gpu_run(Q, w, nS)
        assert dict(calls) == {n: 1 for n in SHIM_ENTRIES}, (nS, dict(calls))
        calls.clear()
        with torch.no_grad():
            _gpu_run(Q, None, nS)
        assert dict(calls) == {SHIM_ENTRIES[0]: 1}, (nS, dict(calls))


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
def test_composed_route_spin_side_gradients(tag, mode, monkeypatch):
    r"""Gradients w.r.t. ``shMap`` and ``loc`` (the composed route; ``sh`` and ``rf`` beside them) against the oracle's autograd;
    no ``_shim_`` entry point is called."""
    Q, w = _prob(tag, 'b1map', NT), _weights((N, NM, 3), DT[tag])
    Q = dict(Q, sh=Q['sh'][:, :3], map=Q['map'][..., :3].contiguous())
    Q64 = _wide(Q)
    leaves = {k: Q64[k].clone().requires_grad_(True) for k in ('map', 'loc', 'sh', 'rf')}
    with mrphy_amd.constants_on('cpu'):
        Mo = _oracle_Mo(Q64, Q64['M0'], leaves['rf'], Q64['gr'], leaves['sh'], leaves['map'], loc=leaves['loc'])
        (Mo * w.double()).sum().backward()
    want = dict(Mo=Mo.detach(), **{'grad_' + k: x.grad for k, x in leaves.items()})
    gl = {k: dev(Q[k]).clone().requires_grad_(True) for k in leaves}
    calls = _counted(monkeypatch)
    with mrphy_amd.precision(mode):
        Mo = fused.blochsim_rfgr_shim(dev(Q['M0']), gl['rf'], dev(Q['gr']), gl['loc'], gl['sh'], gl['map'], **_kw(Q, dev))
        (Mo * dev(w)).sum().backward()
    assert not calls, dict(calls)
    got = dict(Mo=Mo.detach(), **{'grad_' + k: x.grad for k, x in gl.items()})
    _gate(f'shim.composed.{tag}.{mode}.spin_side', got, want, tag, mode)


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
def test_composed_route_two_transmit_coils(tag, mode, monkeypatch):
    r"""Parallel transmit is composed: two coils with their ``b1Map``, forward and the four gradients against the oracle."""
    Q, w = dict(_prob(tag, 'plain', NT)), _weights((N, NM, 3), DT[tag])
    gen = torch.Generator().manual_seed(7)
    Q['rf'] = ((torch.rand(N, 2, NT, 2, generator=gen, dtype=torch.float64) * 2 - 1) * 1.5).to(DT[tag])
    Q['b1'] = ((torch.rand(N, NM, 2, 2, generator=gen, dtype=torch.float64) * 2 - 1) * 0.7).to(DT[tag])
    calls = _counted(monkeypatch)
    with mrphy_amd.precision(mode):
        got = _gpu_run(Q, w, 3)
    assert not calls, dict(calls)
    assert got['grad_rf'].shape == Q['rf'].shape
    _gate(f'shim.composed.{tag}.{mode}.two_coils', got, _oracle_run(Q, w, 3), tag, mode)


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
def test_composed_route_more_channels_than_the_capacity(tag, mode, monkeypatch):
    lib = mrphy_amd.require_library()
    nS = int(lib.mrphy_blochsim_rfgr_shim_max_channels(_host.dtype_code(DT[tag], DT[tag]))) + 1
    assert nS <= NCH
    Q, w = _prob(tag, 'b1map', NT), _weights((N, NM, 3), DT[tag])
    calls = _counted(monkeypatch)
    with mrphy_amd.precision(mode):
        got = _gpu_run(Q, w, nS)
    assert not calls, dict(calls)
    _gate(f'shim.composed.{tag}.{mode}.over_capacity', got, _oracle_run(Q, w, nS), tag, mode)


# ---------------------------------------------------------------------------------------------
# 8. operand forms
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('variant', ['plain', 'b1map'])
def test_channel_operand_forms(tag, mode, variant):
    r"""``sh`` as `(1, nS, nT)` against N = 2 and as a stride-0 expanded view of that; ``shMap`` as `(1, *Nd, nS)`, as an expanded
    view of that and as a permuted view; and the whole call with ``Nd = (7, 7, 7)``: each gives the bits of the contiguous
    call, forward and backward (``grad_sh`` of a shared waveform set: the batch entries' rows added)."""
    nS = 5
    Q, w = _prob(tag, variant, NT), _weights((N, NM, 3), DT[tag])
    sh1, m1 = Q['sh'][:1, :nS].clone(), Q['map'][:1, :, :nS].clone()
    mfull = Q['map'][..., :nS].contiguous()
    with mrphy_amd.precision(mode):
        ref = _gpu_run(Q, w, nS, sh=dev(sh1.expand(N, nS, NT).contiguous()))
        for name, v in (('one', sh1), ('expanded', sh1.expand(N, nS, NT))):
            x = place(v).requires_grad_(True)                        # the leaf the call gets: no copy in between
            assert x.stride() == v.stride() and (name == 'one' or x.stride(0) == 0)
            got = _gpu_run(Q, w, nS, sh=x)
            assert got['grad_sh'] is x.grad and x.stride() == v.stride()
            assert got['grad_sh'].shape == v.shape
            for k in ('Mo', 'grad_Mi', 'grad_rf', 'grad_gr'):
                assert torch.equal(got[k], ref[k]), ('sh', name, k)
            if name == 'expanded':
                assert torch.equal(got['grad_sh'], ref['grad_sh']), ('sh', name)
            else:
                assert torch.equal(got['grad_sh'], ref['grad_sh'].sum(0, keepdim=True)), ('sh', name)
        ref = _gpu_run(Q, w, nS, shMap=dev(m1.expand(N, NM, nS).contiguous()))
        for name, v in (('one', m1), ('expanded', m1.expand(N, NM, nS))):
            x = place(v)
            assert x.stride() == v.stride()
            got = _gpu_run(Q, w, nS, shMap=x)
            for k in ref:
                assert torch.equal(got[k], ref[k]), ('shMap', name, k)
        ref = _gpu_run(Q, w, nS)
        perm = mfull.permute(2, 0, 1).contiguous().permute(1, 2, 0)
        assert not perm.is_contiguous() and torch.equal(perm, mfull)
        x = place(perm)
        assert x.stride() == perm.stride()
        got = _gpu_run(Q, w, nS, shMap=x)
        for k in ref:
            assert torch.equal(got[k], ref[k]), ('shMap permuted', k)
        # Nd = (7, 7, 7)
        cube = lambda x, *tail: None if x is None else dev(x).reshape((N, 7, 7, 7) + tail)  # noqa: E731
        Mi, r, g, s = (dev(Q[k]).clone().requires_grad_(True) for k in ('M0', 'rf', 'gr', 'sh'))
        Mi = dev(Q['M0']).reshape(N, 7, 7, 7, 3).clone().requires_grad_(True)
        s = dev(Q['sh'][:, :nS]).clone().requires_grad_(True)
        kw = dict(_kw(Q, dev), Δf=cube(Q['df']), b1Map=cube(Q['b1'], 2), T1=cube(Q['T1']), T2=cube(Q['T2']))
        Mo = fused.blochsim_rfgr_shim(Mi, r, g, cube(Q['loc'], 3), s, cube(mfull, nS), **kw)
        assert Mo.shape == (N, 7, 7, 7, 3)
        (Mo * dev(w).reshape(Mo.shape)).sum().backward()
        for k, x in (('Mo', Mo.detach()), ('grad_Mi', Mi.grad), ('grad_rf', r.grad), ('grad_gr', g.grad), ('grad_sh', s.grad)):
            assert torch.equal(x.reshape(ref[k].shape), ref[k]), ('Nd = (7, 7, 7)', k)


# ---------------------------------------------------------------------------------------------
# 9. determinism
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('nS', [3, 8])
def test_two_identical_calls_give_identical_bits(tag, mode, nS):
    Q, w = _prob(tag, 'b1map', NT), _weights((N, NM, 3), DT[tag])
    with mrphy_amd.precision(mode):
        a, b = _gpu_run(Q, w, nS), _gpu_run(Q, w, nS)
    assert set(a) == {'Mo', *GRADS}
    for k in a:
        assert torch.equal(a[k], b[k]), k
