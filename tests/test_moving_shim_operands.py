r"""``fused.blochsim_rfgr_moving`` (K2v / K2vb) and ``fused.blochsim_rfgr_shim`` (K2sh / K2shb) on every operand form the host
code accepts (``cases.moving_shim_variants``: the zoo of ``test_fused_operands.py``, each variant with ``vel``, ``sh``, ``shMap`` in a
spelling of its own and nS = 2, 4, 6, 7 channels on a per-entry and on a shared ``sh``), on steps of exactly zero field
(``cases.moving_shim_zero_field``) and with spins whose ``γ`` is 0.

The yardstick is ``test_moving_shim_cases_host.oracle_run``: ``bloch_oracle`` in fp64 on the operands as given (fp32 widened),
never the library's composed route; ``test_moving_shim_cases_host.py`` shows on the CPU that the new operands and the
per-entry ``dt`` move it by far more than a gate.  Gates: ``util.ATOL64`` elementwise in fp64, ``util.REL32`` relative L2 in fp32
precise, through ``test_moving._gate``; the fast mode's distances go to the ledger unasserted; bit identities hold in all three
modes.  Ledger keys: ``movshim.*``."""
import collections
import functools

import pytest

from gpu_common import *  # noqa: F401,F403
from test_moving import _gate
from test_moving_shim_cases_host import CALLS, CASES, GRADS, oracle_run

pytestmark = pytest.mark.gpu

MODES = [('f64', 'precise'), ('f32', 'precise'), ('f32', 'fast')]
ENTRIES = {'moving': ('mrphy_blochsim_rfgr_moving_fwd', 'mrphy_blochsim_rfgr_moving_bwd'),
           'shim': ('mrphy_blochsim_rfgr_shim_fwd', 'mrphy_blochsim_rfgr_shim_bwd')}
LEAVES = {'grad_Mi': 'M0', 'grad_rf': 'rf', 'grad_gr': 'gr', 'grad_sh': 'sh'}


def _counted(monkeypatch):
    r"""``test_shim._counted`` over the four entry points of the two calls."""
    lib = mrphy_amd.require_library()
    calls = collections.Counter()

    def wrap(name, fn):
        def counted(*a):
            calls[name] += 1
            return fn(*a)
        return counted
    for name in ENTRIES['moving'] + ENTRIES['shim']:
        monkeypatch.setattr(lib, name, wrap(name, getattr(lib, name)))
    return calls


def _run(v, call, **over):
    r"""``(results, leaves)`` of ``<w, Mo>`` through the call: ``Mo`` and the gradient of every leaf (``Mi``, ``rf``, ``gr``; ``sh``).
    The operands go in AS GIVEN: ``place`` keeps their strides and offsets, and the leaves are detached aliases of that, not
    copies -- what receives ``.grad`` is what was handed in."""
    leaf = lambda x: place(x).detach().requires_grad_(True)  # noqa: E731
    L = dict(M0=leaf(v['M0']), rf=leaf(v['rf']), gr=leaf(v['gr']))
    kw = dict({k: place(v[k]) for k in ('Δf', 'b1Map', 'γ_beff', 'T1', 'T2', 'γ', 'dt')}, **over)
    if call == 'moving':
        Mo = fused.blochsim_rfgr_moving(L['M0'], L['rf'], L['gr'], place(v['loc']), place(v['vel']), **kw)
    else:
        L['sh'] = leaf(v['sh'])
        Mo = fused.blochsim_rfgr_shim(L['M0'], L['rf'], L['gr'], place(v['loc']), L['sh'], place(v['shMap']), **kw)
    torch.autograd.backward([Mo], [place(v['w'])])
    return dict(Mo=Mo.detach(), **{g: L[LEAVES[g]].grad for g in GRADS[call]}), L


def _same_bits(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert max_abs(a, b) == 0.0, f'{what}: differs by {max_abs(a, b):.3e}'


@functools.lru_cache(maxsize=None)
def _zoo(tag, nC, nT):
    return cases.moving_shim_variants(DT[tag], nC, nT)


@functools.lru_cache(maxsize=None)
def _oracle(tag, call, nC, nT, name):
    return oracle_run(_zoo(tag, nC, nT)[name][0], call)


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('nC', [0, 1])
@pytest.mark.parametrize('name,nT', CASES)
@pytest.mark.parametrize('call', CALLS)
def test_operand_spellings(call, name, nT, nC, tag, mode, monkeypatch):
    r"""One problem, many spellings; nT = 48: three checkpoint segments through the fused adjoint; nT = 53: the split route,
    48 fused steps and 5 composed ones (``fused.py``: the tail of a split length never reaches a ``_moving_`` / ``_shim_`` entry
    point, so each is called once there too, as ``test_shim.test_split_route`` counts them)."""
    given, dense = _zoo(tag, nC, nT)[name]
    key = f'movshim.{call}.{tag}.{mode}.c{nC}.nT{nT}.{name}'
    new = ('vel',) if call == 'moving' else ('sh', 'shMap')
    if name == 'views':        # the forms under test arrive as such
        assert not any(place(given[k]).is_contiguous() for k in ('M0', 'loc', 'rf', 'gr', 'w') + new)
    if name == 'offset':
        assert all(place(given[k]).is_contiguous() and place(given[k]).data_ptr() % 16 != 0 for k in ('M0', 'rf', 'gr') + new)
    if name in ('expanded', 'scalars'):
        assert all(0 in place(given[k]).stride() for k in new if k != 'sh' or name == 'expanded')
    if name == 'gamma_split':
        assert all(given[k].dtype == torch.float64 for k in new)
    calls = _counted(monkeypatch)
    with mrphy_amd.precision(mode):
        fu, L = _run(given, call)
        assert dict(calls) == {n: 1 for n in ENTRIES[call]}, (key, dict(calls))
        for g in GRADS[call]:                          # the leaf handed in got the gradient, in its own form
            k = LEAVES[g]
            assert fu[g] is L[k].grad and fu[g] is not None, (key, g)
            assert L[k].stride() == given[k].stride() and L[k].storage_offset() == given[k].storage_offset(), (key, k)
            assert fu[g].shape == given[k].shape and fu[g].dtype == given[k].dtype, (key, g, fu[g].shape, fu[g].dtype)
            assert bool(torch.isfinite(fu[g]).all()), (key, g)
        assert fu['Mo'].shape == given['M0'].shape and fu['Mo'].dtype == DT[tag]
        fd, _ = _run(dense, call)                      # (1) the spelling changes nothing
        _same_bits(fu['Mo'].reshape(fd['Mo'].shape), fd['Mo'], f'{key}: Mo, as given vs dense')
        _same_bits(fu['grad_Mi'].reshape(fd['grad_Mi'].shape), fd['grad_Mi'], f'{key}: grad_Mi, as given vs dense')
        for g in GRADS[call][1:]:
            if fu[g].shape == fd[g].shape:
                _same_bits(fu[g], fd[g], f'{key}: {g}, as given vs dense')
            else:                                      # a batch-1 leaf, expanded in `dense`
                assert fu[g].shape[0] == 1
                _gate(f'{key}.{g}.vs_dense_summed', {g: fu[g]}, {g: fd[g].sum(0, keepdim=True).cpu()}, tag, mode)
        _gate(key, fu, _oracle(tag, call, nC, nT, name), tag, mode)      # (3) the yardstick
        again, _ = _run(given, call)                   # (4) determinism
        for k in fu:
            _same_bits(fu[k], again[k], f'{key}: {k}, second run')


@functools.lru_cache(maxsize=None)
def _zero(tag, nC):
    return cases.moving_shim_zero_field(DT[tag], nC)


@functools.lru_cache(maxsize=None)
def _zero_oracle(tag, call, nC):
    return oracle_run(_zero(tag, nC)[0], call)


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('nC', [0, 1])
@pytest.mark.parametrize('call', CALLS)
def test_zero_field_steps(call, nC, tag, mode):
    r"""Dead time and spins at rest at the iso-centre through K2vb / K2shb (``test_fused_operands.test_zero_field_steps`` for K2b):
    the yardstick's explicit adjoint holds the analytic limit ``-γ2πdt (m x h̃)`` at zero field, which is not zero
    (``test_moving_shim_cases_host.py``: the dead steps carry more than half of ``grad_gr``'s and ``grad_sh``'s norm).  The pulse
    gradients -- ``grad_sh`` comes out of a dot product in LDS against rows that hold that limit -- are held to the gates on the
    zero-field steps alone and on batch entry 1's all-zero segment alone, too."""
    v, zero = _zero(tag, nC)
    key = f'movshim.{call}.{tag}.{mode}.c{nC}.zero_field'
    with mrphy_amd.precision(mode):
        fu, _ = _run(v, call)
    ora = _zero_oracle(tag, call, nC)
    for k, x in fu.items():
        assert bool(torch.isfinite(x).all()), (key, k)
    _gate(key, fu, ora, tag, mode)
    pulse = GRADS[call][1:]
    sl = lambda x: x.movedim(2, 1)[zero.to(x.device)]  # noqa: E731
    seg = list(cases.ZERO_SEGMENT)
    _gate(f'{key}.zero_steps', {k: sl(fu[k]) for k in pulse}, {k: sl(ora[k]) for k in pulse}, tag, mode)
    _gate(f'{key}.zero_segment', {k: fu[k][1][:, seg] for k in pulse}, {k: ora[k][1][:, seg] for k in pulse}, tag, mode)
    for k in ('grad_gr',) + (('grad_sh',) if call == 'shim' else ()):
        assert float(sl(ora[k]).abs().max()) > 1e-3 * float(ora[k].abs().max()), k      # nothing like zero


@functools.lru_cache(maxsize=None)
def _gamma0(tag, nC):
    v = dict(_zoo(tag, nC, 48)['gamma_split'][0])
    γ = v['γ'].clone()
    for n, s in cases.ZERO_SPINS:
        γ[n, s] = 0
    return dict(v, γ=γ)


@functools.lru_cache(maxsize=None)
def _gamma0_oracle(tag, call, nC, masked):
    v = _gamma0(tag, nC)
    if masked:                      # the pulse gradients of the other spins alone: a zero cotangent for the two
        w = v['w'].clone()
        for n, s in cases.ZERO_SPINS:
            w[n, s] = 0
        return oracle_run(v, call, cot=w)
    return oracle_run(v, call)


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('call', CALLS)
def test_gamma_zero_spins(call, tag, mode):
    r"""``test_fused_grads_operands.test_gamma_zero_spins``'s construction: 'gamma_split' (per-spin ``γ`` and ``γ_beff``, fp64
    ``vel`` / ``sh`` / ``shMap``, a b1 map) with ``γ[0, 7] = γ[1, 64] = 0`` -- the STEP constant; the spins' field, motion and channels
    are live.  Such a spin turns by ``0·|B|``: it only relaxes (``Mo`` the closed form, ``grad_Mi = E^nT w``), and adds exact
    zeros to ``grad_rf``, ``grad_gr``, ``grad_sh`` -- which are then the yardstick's with a zero cotangent for the two spins.
    Everything is finite and within the gates."""
    v = _gamma0(tag, 1)
    key = f'movshim.{call}.{tag}.{mode}.gamma0'
    with mrphy_amd.precision(mode):
        fu, _ = _run(v, call)
    for k, x in fu.items():
        assert bool(torch.isfinite(x).all()), (key, k)
    _gate(key, fu, _gamma0_oracle(tag, call, 1, False), tag, mode)
    pulse = GRADS[call][1:]
    masked = _gamma0_oracle(tag, call, 1, True)
    _gate(f'{key}.other_spins_alone', {k: fu[k] for k in pulse}, {k: masked[k] for k in pulse}, tag, mode)
    c = cases.reference_constants(v['T1'], v['T2'], v['γ'], v['dt'], 4)
    for n, s in cases.ZERO_SPINS:
        e1, e2, e1m1 = (float(c[k][n, 0, 0, 0]) for k in ('E1', 'E2', 'E1_1'))
        m, h = v['M0'][n, s].double().clone(), v['w'][n, s].double().clone()
        for _ in range(48):
            m = torch.stack((m[0] * e2, m[1] * e2, m[2] * e1 - e1m1))
            h = torch.stack((h[0] * e2, h[1] * e2, h[2] * e1))
        if mode == 'precise':
            assert_close(fu['Mo'][n, s], m, tag, f'{key}: spin {(n, s)} only relaxes: Mo')
            assert_close(fu['grad_Mi'][n, s], h, tag, f'{key}: spin {(n, s)} only relaxes: grad_Mi')
