r"""``fused.blochsim_rfgr_moving`` (K2v / K2vb) and ``fused.blochsim_rfgr_shim`` (K2sh / K2shb) on what a caller may ask of them:
any subset of the gradients, a cotangent in any form, the smallest shapes, a pulse that starts millions of steps into
a sequence (``step0``), fp16 / bf16 operands.

The problem is ``test_moving._prob`` / ``test_shim._prob``, variant ``b1map`` (N = 2, nM = 343, nT = 48), unless stated otherwise;
the yardstick is ``test_moving_shim_cases_host.oracle_run``: ``bloch_oracle`` in fp64 on the operands as given, never the
library's composed route.  Gates: ``util.ATOL64`` elementwise in fp64, ``util.REL32`` relative L2 in fp32 precise, through
``test_moving._gate``; the fast mode's distances go to the ledger unasserted; bit identities hold in all three modes.  Ledger
keys: ``movshim.*``."""
import functools
import itertools

import pytest

from gpu_common import *  # noqa: F401,F403
from test_fused_traj import _problem, _kw, _weights
from test_moving import _prob as _moving_prob, _gate, _over_gate, DT_STEP
from test_moving_shim_cases_host import GRADS, oracle_run
from test_moving_shim_operands import ENTRIES, MODES, _counted, _same_bits
from test_shim import _prob as _shim_prob

pytestmark = pytest.mark.gpu

N, NM, NT = 2, 343, 48
LEAVES = {'moving': ('Mi', 'rf', 'gr'), 'shim': ('Mi', 'rf', 'gr', 'sh')}
CALLS_NS = [('moving', None), ('shim', 3), ('shim', 8)]
PER_SPIN = ('M0', 'loc', 'Δf', 'b1Map', 'T1', 'T2', 'vel', 'shMap', 'w')


def _prob(call, tag, nT=NT):
    return _moving_prob(tag, 'b1map', nT) if call == 'moving' else _shim_prob(tag, 'b1map', nT)


def _as_v(Q, w, nS=None, spins=None):
    r"""The problem under the keys of ``cases.moving_shim_variants``, for the yardstick; ``spins``: those spins alone."""
    v = dict(M0=Q['M0'], rf=Q['rf'], gr=Q['gr'], loc=Q['loc'], Δf=Q['df'], b1Map=Q['b1'], γ_beff=Q['γ'], T1=Q['T1'],
             T2=Q['T2'], γ=Q['γ'], dt=Q['dt'], vel=Q.get('vel'), w=w)
    if nS is not None:
        v.update(sh=Q['sh'][:, :nS], shMap=Q['map'][..., :nS])
    if spins is not None:
        v = {k: (x[:, spins] if k in PER_SPIN and x is not None else x) for k, x in v.items()}
    return {k: x for k, x in v.items() if x is not None or k in ('Δf', 'b1Map', 'T1', 'T2')}


def _forward(call, Q, T, nS=None, step0=0, on=dev, shape=None):
    r"""The call on the tensors ``T`` (``Mi``, ``rf``, ``gr``; ``sh``) and the rest of ``Q``; ``shape``: the spins on a grid ``(N, *Nd)``."""
    grid = (lambda x, *tail: x) if shape is None else \
        (lambda x, *tail: None if x is None else x.reshape(tuple(shape) + tail))
    kw = _kw(Q, on)
    kw.update(Δf=grid(kw['Δf']), b1Map=grid(kw['b1Map'], 2), T1=grid(kw['T1']), T2=grid(kw['T2']))
    loc = grid(on(Q['loc']), 3)
    if call == 'moving':
        return fused.blochsim_rfgr_moving(T['Mi'], T['rf'], T['gr'], loc, grid(on(Q['vel']), 3), step0=step0, **kw)
    return fused.blochsim_rfgr_shim(T['Mi'], T['rf'], T['gr'], loc, T['sh'], grid(on(Q['map'][..., :nS].contiguous()), nS), **kw)


def _tensors(call, Q, want, nS=None, on=dev, shape=None):
    r"""Fresh device copies of the possible leaves; those in ``want`` require grad."""
    T = dict(Mi=on(Q['M0']).clone(), rf=on(Q['rf']).clone(), gr=on(Q['gr']).clone())
    if shape is not None:
        T['Mi'] = T['Mi'].reshape(tuple(shape) + (3,)).clone()
    if call == 'shim':
        T['sh'] = on(Q['sh'][:, :nS]).clone()
    for k in want:
        T[k].requires_grad_(True)
    return T


def _go(call, Q, want, cot, nS=None, step0=0, shape=None):
    r"""``Mo`` and ``grad_<leaf>`` (``None`` where not asked for) of ``<cot, Mo>``; ``cot`` a device tensor in the form it has, or a
    function of ``Mo`` returning the loss."""
    T = _tensors(call, Q, want, nS, shape=shape)
    Mo = _forward(call, Q, T, nS, step0, shape=shape)
    if callable(cot):
        cot(Mo).backward()
    else:
        torch.autograd.backward([Mo], [cot])
    return dict(Mo=Mo.detach(), **{'grad_' + k: T[k].grad for k in LEAVES[call]})


# ---------------------------------------------------------------------------------------------
# 1. partial requests
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('call,nS', CALLS_NS)
def test_every_subset_of_the_gradients(call, nS, tag, mode, monkeypatch):
    r"""Every non-empty subset of the leaves: what is asked for is the all-leaves call's bits, what is not asked for is
    ``None``, one adjoint launch serves it (NULL ``grad_Mi`` / ``grad_rf`` / ``grad_gr`` outputs; K2shb's ``lead`` buffer holds
    ``grad_gr`` and ``grad_sh`` when either is wanted).  No leaf under ``enable_grad``: the forward alone, nothing kept."""
    Q, leaves = _prob(call, tag), LEAVES[call]
    w = dev(_weights((N, NM, 3), DT[tag]))
    fwd, bwd = ENTRIES[call]
    calls = _counted(monkeypatch)
    with mrphy_amd.precision(mode):
        full = _go(call, Q, leaves, w, nS)
        assert dict(calls) == {fwd: 1, bwd: 1}, dict(calls)
        assert all(full['grad_' + k] is not None and float(full['grad_' + k].abs().max()) > 0 for k in leaves)
        for r in range(1, len(leaves)):
            for want in itertools.combinations(leaves, r):
                calls.clear()
                got = _go(call, Q, want, w, nS)
                assert dict(calls) == {fwd: 1, bwd: 1}, (want, dict(calls))
                _same_bits(got['Mo'], full['Mo'], f'{want}: Mo')
                for k in leaves:
                    if k in want:
                        _same_bits(got['grad_' + k], full['grad_' + k], f'{want}: grad_{k}')
                    else:
                        assert got['grad_' + k] is None, (want, k)
        calls.clear()
        with torch.enable_grad():
            Mo = _forward(call, Q, _tensors(call, Q, (), nS), nS)
        assert dict(calls) == {fwd: 1}, dict(calls)
        assert not Mo.requires_grad and Mo.grad_fn is None
        _same_bits(Mo, full['Mo'], 'no leaf: Mo')


@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('nS', [3, 8])
def test_shim_backward_returns_each_gradient_in_its_leafs_form(nS, tag, mode):
    r"""``BlochSimRfGrShimHIP.backward`` called as autograd calls it, its return values looked at BEFORE autograd's engine has
    them: the engine sums a gradient that is too large over the axes it can and casts one of another dtype, so a backward
    that forgot to fold ``grad_sh`` of a batch-1 ``sh`` over N, or returned it in the data dtype for an fp64 ``sh``, gives the
    right ``.grad`` all the same.  The shapes and dtypes asserted here are the Function's own."""
    Q = _prob('shim', tag)
    w = dev(_weights((N, NM, 3), DT[tag]))
    with mrphy_amd.precision(mode):
        for sh in (Q['sh'][:1, :nS].clone(), Q['sh'][:, :nS].double()):
            T = _tensors('shim', Q, ('Mi', 'rf', 'gr'), nS)
            T['sh'] = dev(sh).requires_grad_(True)
            Mo = _forward('shim', Q, T, nS)
            ctx = Mo.grad_fn
            assert type(ctx).__name__.startswith('BlochSimRfGrShimHIP'), type(ctx)
            out = dict(zip(fused.BlochSimRfGrShimHIP.ARGS, fused.BlochSimRfGrShimHIP.backward(ctx, w)))
            for k in LEAVES['shim']:
                assert out[k].shape == T[k].shape and out[k].dtype == T[k].dtype and out[k].device == T[k].device, \
                    (k, out[k].shape, out[k].dtype)
            assert all(out[k] is None for k in fused.BlochSimRfGrShimHIP.ARGS if k not in LEAVES['shim'])
            Mo.backward(w)
            for k in LEAVES['shim']:
                _same_bits(out[k], T[k].grad, f'backward called by hand vs .grad: {k}')


# ---------------------------------------------------------------------------------------------
# 2. cotangent forms
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('call,nS', CALLS_NS)
def test_cotangent_forms_give_the_same_bits(call, nS, tag, mode):
    r"""The same numbers ``w`` as a contiguous cotangent, as the transpose of `(N, 3, nM)`, one element into a larger buffer,
    in fp64 multiplied into ``Mo``, and on a `(N, 7, 7, 7, 3)` grid: one set of bits.  ``Mo.sum().backward()`` hands the
    backward a stride-0 cotangent: the bits of a contiguous tensor of ones."""
    Q, leaves = _prob(call, tag), LEAVES[call]
    w = _weights((N, NM, 3), DT[tag])
    wT = w.transpose(1, 2).contiguous().transpose(1, 2)
    assert not wT.is_contiguous() and torch.equal(wT, w)
    with mrphy_amd.precision(mode):
        ref = _go(call, Q, leaves, dev(w), nS)
        forms = {
            'transposed': _go(call, Q, leaves, place(wT), nS),
            'after': _go(call, Q, leaves, place(cases._after(w)), nS),
            'fp64 product': _go(call, Q, leaves, lambda Mo: (Mo * dev(w.double())).sum(), nS),
            'product': _go(call, Q, leaves, lambda Mo: (Mo * dev(w)).sum(), nS),
            'grid': _go(call, Q, leaves, dev(w).reshape(N, 7, 7, 7, 3), nS, shape=(N, 7, 7, 7)),
        }
        assert place(wT).stride() == wT.stride() and place(cases._after(w)).storage_offset() == 1
        for name, got in forms.items():
            for k in ref:
                assert got[k].dtype == ref[k].dtype, (name, k)
                _same_bits(got[k].reshape(ref[k].shape), ref[k], f'{name}: {k}')
        ones = _go(call, Q, leaves, torch.ones(N, NM, 3, dtype=DT[tag], device=DEV), nS)
        summed = _go(call, Q, leaves, lambda Mo: Mo.sum(), nS)
        for k in ones:
            _same_bits(summed[k], ones[k], f'Mo.sum(): {k}')
            assert float(ones[k].abs().max()) > 0


@functools.lru_cache(maxsize=None)
def _one_spin_oracle(call, tag, nS, spin):
    return oracle_run(_as_v(_prob(call, tag), _weights((N, NM, 3), DT[tag]), nS, slice(spin, spin + 1)), call)


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('call,nS', CALLS_NS)
@pytest.mark.parametrize('spin', [342, 64])
def test_one_hot_cotangent(spin, call, nS, tag, mode):
    r"""A cotangent that is ``w`` on one spin (of both batch entries) and zero elsewhere -- spin 342, the last lane of the
    ragged tile, and spin 64, the first lane of the second tile: the pulse gradients are that ONE spin's, against the
    yardstick run on that spin alone (nothing to hide a wrong lane behind), and ``grad_Mi`` is exactly zero elsewhere."""
    Q, leaves = _prob(call, tag), LEAVES[call]
    w = _weights((N, NM, 3), DT[tag])
    hot = torch.zeros_like(w)
    hot[:, spin] = w[:, spin]
    with mrphy_amd.precision(mode):
        got = _go(call, Q, leaves, dev(hot), nS)
    ora = _one_spin_oracle(call, tag, nS, spin)
    rest = torch.ones(NM, dtype=torch.bool)
    rest[spin] = False
    assert float(got['grad_Mi'][:, rest.to(DEV)].abs().max()) == 0.0
    pulse = GRADS[call][1:]
    _gate(f'movshim.{call}.{tag}.{mode}.nS{nS}.one_hot.spin{spin}',
          dict({k: got[k] for k in pulse}, Mo=got['Mo'][:, spin:spin + 1], grad_Mi=got['grad_Mi'][:, spin:spin + 1]),
          {k: ora[k] for k in pulse + ('Mo', 'grad_Mi')}, tag, mode)


# ---------------------------------------------------------------------------------------------
# 3. small shapes
# ---------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 16, False), (1, 63, 16, False), (1, 64, 32, False), (2, 65, 16, False), (3, 65, 48, True)]


@functools.lru_cache(maxsize=None)
def _small(tag, n, nM, nT, shared):
    r"""``test_fused_traj._problem`` (variant ``b1map``) at N = ``n`` with seeded ``vel``, four channels ``sh`` / ``map`` and weights;
    ``shared``: ``rf``, ``gr``, ``sh`` batch-1."""
    Q = dict(_problem(tag, 'b1map', nT, N=n, nM=nM))
    gen = torch.Generator().manual_seed(307 + 1000 * n + 10 * nM + nT)
    u = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64) * 2 - 1  # noqa: E731
    c = lambda x: x.to(DT[tag])  # noqa: E731
    Q.update(vel=c(u(n, nM, 3) * (0.02 / DT_STEP)), sh=c(u(1 if shared else n, 4, nT)), map=c(u(n, nM, 4) * 2))
    if shared:
        Q.update(rf=Q['rf'][:1].clone(), gr=Q['gr'][:1].clone())
    return Q, c(u(n, nM, 3))


@functools.lru_cache(maxsize=None)
def _small_oracle(call, tag, shape, nS):
    Q, w = _small(tag, *shape)
    return oracle_run(_as_v(Q, w, nS), call)


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('call,nS', [('moving', None), ('shim', 2), ('shim', 4)])
@pytest.mark.parametrize('shape', SHAPES)
def test_small_shapes(shape, call, nS, tag, mode, monkeypatch):
    r"""N = 1; one spin; 63, 64, 65 spins (a ragged tile, a full one, one lane of a second); nT = 16, one segment, where the
    adjoint's ``first`` and ``seg > 0`` never change; N = 3 beside a shared pulse and shared waveforms, whose gradients keep
    the shape `(1, ...)`; the full capacities nS = 2 and 4.  Forward and every gradient against the yardstick."""
    n, nM, nT, shared = shape
    Q, w = _small(tag, *shape)
    calls = _counted(monkeypatch)
    with mrphy_amd.precision(mode):
        got = _go(call, Q, LEAVES[call], dev(w), nS)
    assert dict(calls) == {e: 1 for e in ENTRIES[call]}, dict(calls)
    assert got['Mo'].shape == got['grad_Mi'].shape == (n, nM, 3)
    nP = 1 if shared else n
    assert got['grad_rf'].shape == (nP, 2, nT) and got['grad_gr'].shape == (nP, 3, nT)
    assert call == 'moving' or got['grad_sh'].shape == (nP, nS, nT)
    for k, x in got.items():
        assert bool(torch.isfinite(x).all()), k
    _gate(f'movshim.{call}.{tag}.{mode}.nS{nS}.shape{n}x{nM}x{nT}', got, _small_oracle(call, tag, shape, nS), tag, mode)


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('call,nS', [('moving', None), ('shim', 2), ('shim', 4)])
def test_fewer_steps_than_a_segment_are_composed(call, nS, tag, mode, monkeypatch):
    r"""(2, 65, 8) with gradients: no ``_moving_`` / ``_shim_`` entry point is called; everything against the yardstick."""
    shape = (2, 65, 8, False)
    Q, w = _small(tag, *shape)
    calls = _counted(monkeypatch)
    with mrphy_amd.precision(mode):
        got = _go(call, Q, LEAVES[call], dev(w), nS)
    assert not calls, dict(calls)
    _gate(f'movshim.{call}.{tag}.{mode}.nS{nS}.shape2x65x8.composed', got, _small_oracle(call, tag, shape, nS), tag, mode)


@pytest.mark.parametrize('tag,mode', MODES)
@pytest.mark.parametrize('call,nS', [('moving', None), ('shim', 2), ('shim', 4)])
@pytest.mark.parametrize('nM,nT', [(0, 16), (65, 0)])
def test_empty_problems_with_gradients(nM, nT, call, nS, tag, mode):
    r"""No spin, or no step: ``Mo`` is ``Mi``, ``grad_Mi`` the cotangent, the pulse gradients zeros of the leaves' shapes."""
    Q, w = _small(tag, 2, nM, nT, False)
    with mrphy_amd.precision(mode):
        got = _go(call, Q, LEAVES[call], dev(w), nS)
    torch.cuda.synchronize()
    assert torch.equal(got['Mo'], dev(Q['M0'])) and torch.equal(got['grad_Mi'], dev(w))
    assert got['grad_rf'].shape == (2, 2, nT) and got['grad_gr'].shape == (2, 3, nT)
    assert call == 'moving' or got['grad_sh'].shape == (2, nS, nT)
    for k in GRADS[call][1:]:
        assert got[k].dtype == DT[tag] and float(got[k].abs().sum()) == 0.0, k


# ---------------------------------------------------------------------------------------------
# 4. step0 in the millions (fp32) and beyond 2^32 (fp64)
# ---------------------------------------------------------------------------------------------
BIG = {'f32': 2 ** 23 - 49, 'f64': 2 ** 40 + 12345}


@functools.lru_cache(maxsize=None)
def _late(tag):
    r"""``test_moving._prob`` with ``vel = u 2 / (B dt)``, ``u`` seeded in +-1: by step ``B`` each spin has moved up to 2 cm."""
    Q = dict(_moving_prob(tag, 'b1map', NT))
    gen = torch.Generator().manual_seed(401)
    u = torch.rand(N, NM, 3, generator=gen, dtype=torch.float64) * 2 - 1
    Q['vel'] = (u * 2 / (BIG[tag] * DT_STEP)).to(DT[tag])
    return Q


@functools.lru_cache(maxsize=None)
def _late_oracle(tag, step0, static=False):
    Q, w = _late(tag), _weights((N, NM, 3), DT[tag])
    if static:
        Q = dict(Q, vel=torch.zeros_like(Q['vel']))
    return oracle_run(_as_v(Q, w), 'moving', step0=step0)


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag,mode', MODES)
def test_large_step0(tag, mode):
    r"""``step0 = B``: 2^23 - 49 in fp32, so that ``B + 48 = 2^23 - 1`` is the last value accepted; 2^40 + 12345 in fp64, which
    no 32-bit count holds.  ``Mo`` and the gradients against the yardstick at ``step0 = B``; the chain of 32 steps at ``B`` and
    16 at ``B + 32`` gives the single call's ``Mo`` bit for bit and its gradients within the gate; the call at ``step0 = 0`` is
    somewhere else.  CPU dry run of the yardstick on this problem: ``Mo`` and the gradients move by 0.47 .. 0.66 (relative L2)
    when ``step0`` is dropped or cut to its low 16 bits (0.52 .. 0.62 on 100 spins of this construction, in fp64 for the low 32
    bits too), so a count truncated anywhere between the call and ``step_mid`` is four orders above the gate.  An off-by-one
    or a missing 1/2 is NOT seen here -- either moves the result by 1e-7 or less at these velocities; that is
    ``test_moving.py``'s job, at velocities 1e5 times larger."""
    B, Q, w = BIG[tag], _late(tag), _weights((N, NM, 3), DT[tag])
    led = f'movshim.moving.{tag}.{mode}.step0_{"2p23" if tag == "f32" else "2p40"}'
    leaves = LEAVES['moving']
    ora, ora0 = _late_oracle(tag, B), _late_oracle(tag, 0, static=True)
    with mrphy_amd.precision(mode):
        st = _go('moving', dict(Q, vel=torch.zeros_like(Q['vel'])), leaves, dev(w))
        record(f'{led}.static_vs_oracle.over_gate', max(_over_gate(st[k], ora0[k], tag) for k in ora0),
               note=', '.join(f'{k} {_over_gate(st[k], ora0[k], tag):.3f}' for k in ora0))
        got = _go('moving', Q, leaves, dev(w), step0=B)
        _gate(led, got, ora, tag, mode)
        early = _go('moving', Q, leaves, dev(w), step0=0)
        for k in ('Mo', 'grad_rf', 'grad_gr'):
            assert rel_l2(early[k], got[k]) > 0.1, (k, rel_l2(early[k], got[k]))
        # the chain: one graph over both calls
        T = _tensors('moving', Q, leaves)
        kw, loc, vel = _kw(Q, dev), dev(Q['loc']), dev(Q['vel'])
        M1 = fused.blochsim_rfgr_moving(T['Mi'], T['rf'][:, :, :32], T['gr'][:, :, :32], loc, vel, step0=B, **kw)
        M2 = fused.blochsim_rfgr_moving(M1, T['rf'][:, :, 32:], T['gr'][:, :, 32:], loc, vel, step0=B + 32, **kw)
        _same_bits(M2.detach(), got['Mo'], 'the chain through step0: Mo')
        torch.autograd.backward([M2], [dev(w)])
        chain = dict(Mo=M2.detach(), grad_Mi=T['Mi'].grad, grad_rf=T['rf'].grad, grad_gr=T['gr'].grad)
    _gate(f'{led}.chain_vs_single', chain, {k: x.cpu() for k, x in got.items()}, tag, mode)
    _gate(f'{led}.chain', chain, ora, tag, mode)


# ---------------------------------------------------------------------------------------------
# 5. fp16 / bf16: half_via_float
# ---------------------------------------------------------------------------------------------
HALF = {'fp16': torch.float16, 'bf16': torch.bfloat16}


@pytest.mark.parametrize('half', list(HALF))
@pytest.mark.parametrize('call,nS', [('moving', None), ('shim', 5)])
def test_half_operands_are_computed_in_fp32(call, nS, half):
    r"""Every floating operand and the loss's weights in fp16 / bf16 -- the fp32 problem's values rounded to the half type --:
    ``Mo`` has the half dtype and is the fp32 call's on the widened values, rounded; the gradients arrive in the half dtype
    and are the fp32 gradients, rounded.  That is all ``half_via_float`` promises, and it involves no tolerance
    (``test_train_requests.test_half_operands_are_computed_in_fp32``)."""
    h = HALF[half]
    Q32 = _prob(call, 'f32')
    Qh = {k: (x.to(h) if isinstance(x, torch.Tensor) else x) for k, x in Q32.items()}
    Qf = {k: (x.float() if isinstance(x, torch.Tensor) else x) for k, x in Qh.items()}
    assert float(Qf['dt']) > 0 and bool(torch.isfinite(Qf['γ']))
    wh = _weights((N, NM, 3), torch.float32).to(h)
    got, ref = _go(call, Qh, LEAVES[call], dev(wh), nS), _go(call, Qf, LEAVES[call], dev(wh.float()), nS)
    assert set(got) == set(ref)
    for k in got:
        assert got[k].dtype == h and ref[k].dtype == torch.float32, (k, got[k].dtype, ref[k].dtype)
        assert got[k].shape == ref[k].shape and float(got[k].float().abs().max()) > 0, k
        assert bool(torch.isfinite(ref[k]).all()), k
        assert torch.equal(got[k], ref[k].to(h)), f'{call} {half}: {k} is not the fp32 result rounded'
