r"""``cases.moving_shim_variants`` / ``moving_shim_zero_field`` and the yardstick the GPU tests of
``fused.blochsim_rfgr_moving`` / ``_shim`` hold them to (``test_moving_shim_operands.py``, ``test_moving_shim_requests.py``),
without a GPU: these tests keep the GPU ones from passing vacuously.

The yardstick (:func:`oracle_run`) is ``bloch_oracle`` in fp64 on the operands as given (fp32 widened): ``rfgr2beff`` at ``loc``,
the moving term ``(gr_t . vel dt)(step0 + t + 1/2)`` or the channel term ``sum_k sh[k, t] shMap[k]`` added to z as
``test_moving._oracle_Mo`` / ``test_shim._oracle_Mo`` do, then ``blochsim`` -- for every broadcast form of the zoo (``dt`` `(N,)`
right-padded as the library pads it; a ``*Nd`` grid).

Observed on the seeded numbers, fp64, nC = 0, 1 and nT = 48, 53 (relative L2; the floors asserted are in brackets):
(a) as given against dense: at most 7.8e-16 [1e-12];
(b) ``vel`` zeroed moves ``Mo`` by 0.073 .. 0.35, ``grad_rf`` by 0.070 .. 0.58, ``grad_gr`` by 0.13 .. 0.69 [0.05]; the last channel
dropped moves them by 0.20 .. 0.97, 0.14 .. 0.73, 0.17 .. 1.3, the last channel zeroed moves ``grad_sh`` by 0.35 .. 1.1 [0.05];
(c) ``dt[0]`` for every batch entry in the moving term moves ``Mo`` by 0.015 .. 0.075 [1e-3];
(d) on the zero-field steps ``grad_gr`` has 0.64 .. 0.70 (moving) and 0.65 .. 0.72 (shim) of its full norm, ``grad_sh`` 0.64 .. 0.67
[1e-6].
"""
import functools

import pytest
import torch

import bloch_oracle as O
import cases
from util import rel_l2

VARIANTS = ['compact_mixed', 'scalars', 'expanded', 'cube', 'cube_planes', 'gamma_split', 'views', 'offset']
CASES = [(n, 48) for n in VARIANTS] + [(n, 53) for n in cases.FUSED_NT53]
CALLS = ('moving', 'shim')
GRADS = {'moving': ('grad_Mi', 'grad_rf', 'grad_gr'), 'shim': ('grad_Mi', 'grad_rf', 'grad_gr', 'grad_sh')}
F64 = torch.float64


def _wide(v):
    return {k: (x.double() if isinstance(x, torch.Tensor) else x) for k, x in v.items()}


def _rpad(x, ndim):
    return x.reshape(tuple(x.shape) + (ndim - x.ndim) * (1,))


def oracle_Mo(v64, call, Mi, rf, gr, sh=None, *, step0=0, dt_motion=None):
    r"""The yardstick's forward (module docstring) on fp64 operands ``v64`` (keys as ``cases.moving_shim_variants``);
    differentiable w.r.t. ``Mi``, ``rf``, ``gr``, ``sh``.  ``dt_motion``: the ``dt`` of the moving term, in place of the problem's."""
    loc = v64['loc']
    lead, N, nT = tuple(loc.shape[:-1]), loc.shape[0], gr.shape[2]
    be = O.rfgr2beff(rf, gr, loc, Δf=v64['Δf'], b1Map=v64['b1Map'], γ=v64['γ_beff'])
    if call == 'moving':
        dt = v64['dt'] if dt_motion is None else dt_motion
        w = (v64['vel'] * _rpad(dt, loc.ndim)).expand(loc.shape).reshape(N, -1, 3)
        τ = torch.arange(nT, dtype=F64) + (step0 + 0.5)
        z = torch.einsum('nsi,nit->nst', w, gr.expand(N, 3, nT)) * τ
    else:
        nS = sh.shape[1]
        m = v64['shMap'].expand(lead + (nS,)).reshape(N, -1, nS)
        z = torch.einsum('nmk,nkt->nmt', m, sh.expand(N, nS, nT))
    be = be + torch.nn.functional.pad(z.reshape(lead + (nT, 1)), (2, 0))
    return O.blochsim(Mi, be, T1=v64['T1'], T2=v64['T2'], γ=v64['γ'], dt=v64['dt'])


def oracle_run(v, call, *, cot=None, step0=0, dt_motion=None, **over):
    r"""``Mo, grad_Mi, grad_rf, grad_gr[, grad_sh]`` of ``<cot, Mo>`` (``cot``: ``v['w']``) by the yardstick, fp64, each gradient
    in the shape of its leaf as given; ``over`` replaces operands of ``v``."""
    v64 = _wide(dict(v, **over))
    leaf = lambda x: x.detach().requires_grad_(True)  # noqa: E731
    Mi, rf, gr = leaf(v64['M0']), leaf(v64['rf']), leaf(v64['gr'])
    sh = leaf(v64['sh']) if call == 'shim' else None
    Mo = oracle_Mo(v64, call, Mi, rf, gr, sh, step0=step0, dt_motion=None if dt_motion is None else dt_motion.double())
    torch.autograd.backward([Mo], [(v64['w'] if cot is None else cot.double()).expand(Mo.shape)])
    out = dict(Mo=Mo.detach(), grad_Mi=Mi.grad, grad_rf=rf.grad, grad_gr=gr.grad)
    return dict(out, grad_sh=sh.grad) if call == 'shim' else out


@functools.lru_cache(maxsize=None)
def _zoo(nC, nT):
    return cases.moving_shim_variants(F64, nC, nT)


def _fold(x, shape):
    r"""A dense gradient `(N, ...)` summed over the batch where the leaf as given is batch-1."""
    return x if tuple(x.shape) == tuple(shape) else x.sum(0, keepdim=True)


@pytest.mark.parametrize('nC', [0, 1])
@pytest.mark.parametrize('name,nT', CASES)
@pytest.mark.parametrize('call', CALLS)
def test_variants_mean_what_they_say(call, name, nT, nC):
    r"""(a) as given and dense agree; (b) the new operand matters; (c) so does the per-entry ``dt`` in the moving term."""
    v, d = _zoo(nC, nT)[name]
    assert v['nS'] == cases.MOVSHIM_NS[name] == v['sh'].shape[1] == v['shMap'].shape[-1]
    N, nM = d['loc'].shape[:2]
    assert d['vel'].shape == (N, nM, 3) and d['sh'].shape == (N, v['nS'], nT) and d['shMap'].shape == (N, nM, v['nS'])
    assert all(d[k].is_contiguous() and d[k].dtype == F64 for k in ('vel', 'sh', 'shMap'))
    step = (v['vel'].double() * float(v['dt'].max())).abs().max()
    # the amplitudes of the existing tests (a form with a handful of entries need not come near the bound)
    assert 0.25 * cases.MOVSHIM_STEP_CM < float(step) <= cases.MOVSHIM_STEP_CM
    assert 0.5 < float(v['sh'].abs().max()) <= 1 and 0.5 < float(v['shMap'].abs().max()) <= 2
    a, b = oracle_run(v, call), oracle_run(d, call)
    for k in ('Mo',) + GRADS[call]:                                            # (a)
        want = _fold(b[k], a[k].shape) if k in ('grad_rf', 'grad_gr', 'grad_sh') else b[k].reshape(a[k].shape)
        assert a[k].shape == want.shape and rel_l2(a[k], want) <= 1e-12, (k, rel_l2(a[k], want))
    if call == 'moving':                                                       # (b)
        off = oracle_run(v, call, vel=torch.zeros_like(v['vel']))
    else:
        off = oracle_run(v, call, sh=v['sh'][:, :-1], shMap=v['shMap'][..., :-1])
        sh0, m0 = v['sh'].clone(), v['shMap'].clone()
        sh0[:, -1], m0[..., -1] = 0, 0
        z = oracle_run(v, call, sh=sh0, shMap=m0)
        assert rel_l2(z['grad_sh'], a['grad_sh']) >= 0.05, rel_l2(z['grad_sh'], a['grad_sh'])
    for k in ('Mo', 'grad_rf', 'grad_gr'):
        assert rel_l2(off[k], a[k]) >= 0.05, (k, rel_l2(off[k], a[k]))
    if v['dt'].ndim == 1 and v['dt'].shape[0] > 1 and call == 'moving':       # (c)
        assert name in ('compact_mixed', 'cube')
        one = oracle_run(v, call, dt_motion=v['dt'][:1])
        assert rel_l2(one['Mo'], a['Mo']) >= 1e-3, rel_l2(one['Mo'], a['Mo'])
    else:
        assert name not in ('compact_mixed', 'cube') or call == 'shim'


@pytest.mark.parametrize('nC', [0, 1])
@pytest.mark.parametrize('call', CALLS)
def test_zero_field_gradients_are_not_zeros(call, nC):
    r"""(d) the limit the GPU tests hold on the dead steps is not a zero; the lanes at zero field are those of the static
    case."""
    v, zero = cases.moving_shim_zero_field(F64, nC)
    st, _ = cases.zero_field_case(F64, nC)
    for k, x in st.items():
        assert (x is None and v[k] is None) or torch.equal(x, v[k]), k
    for n, s in cases.ZERO_SPINS:
        assert float(v['vel'][n, s].abs().max()) == 0.0 and float(v['shMap'][n, s].abs().max()) == 0.0
    assert float(v['sh'].movedim(2, 1)[zero].abs().max()) == 0.0
    assert float(v['sh'][:, :, list(cases.ZERO_RF_ONLY)].abs().max()) == 0.0
    got = oracle_run(v, call)
    sl = lambda x: x.movedim(2, 1)[zero]  # noqa: E731
    for k in ('grad_gr',) + (('grad_sh',) if call == 'shim' else ()):
        assert bool(torch.isfinite(got[k]).all())
        assert float(sl(got[k]).norm()) > 1e-6 * float(got[k].norm()), (k, float(sl(got[k]).norm() / got[k].norm()))


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
@pytest.mark.parametrize('nC', [0, 1])
@pytest.mark.parametrize('nT', [48, 53])
def test_the_existing_generators_keep_their_bits(dtype, nC, nT):
    r"""``fused_operand_variants`` and ``zero_field_case`` return the same tensors (values, dtypes, shapes, strides, offsets)
    before and after the new functions are called: ``golden/fusedops_*.npz`` was recorded on them."""
    def snap():
        zoo = {f'{n}.{k}': x for n, (v, _) in cases.fused_operand_variants(dtype, nC, nT).items() for k, x in v.items()}
        return dict(zoo, **{f'zero.{k}': x for k, x in cases.zero_field_case(dtype, nC, nT)[0].items()})
    before = snap()
    cases.moving_shim_variants(dtype, nC, nT)
    cases.moving_shim_zero_field(dtype, nC, nT)
    after = snap()
    assert set(before) == set(after)
    for k, x in before.items():
        y = after[k]
        if x is None:
            assert y is None, k
            continue
        assert x.dtype == y.dtype and x.shape == y.shape and x.stride() == y.stride() and \
            x.storage_offset() == y.storage_offset() and torch.equal(x, y), k
    # ... and the variants carry those very operands
    for n, (v, _) in cases.moving_shim_variants(dtype, nC, nT).items():
        for k, x in cases.fused_operand_variants(dtype, nC, nT)[n][0].items():
            assert (x is None and v[k] is None) or (torch.equal(x, v[k]) and x.stride() == v[k].stride()), (n, k)
