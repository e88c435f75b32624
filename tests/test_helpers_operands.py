r"""The elementwise helper kernels (``csrc/k_aux.hpp``) and the no-grad 1-step kernel past one 256-thread block and on
every operand form: ``freeprec`` and its constant gradients, linear and one-tap ``interpT``, ``beff2uϕ`` / ``uϕrot`` and their
adjoints, ``blochsim_1step``, ``blochsim_ab``, mask extract / embed, ``cube_loc``.

Yardstick: the fp64 oracle (``oracle/bloch_oracle.py``) on the very numbers the kernel reads -- an operand the host layer
rounds to fp32 is rounded first, then cast up.  Gates: ``util.assert_close``'s (fp64 max-abs 1e-9, fp32 relative L2 1e-5);
the constant gradients relative L2 1e-9 / 1e-5 (``test_slowsims_freeprec_gradients_wrt_dur_T1_T2_df``); row by row where
one row would hide the others (the clamp of ``beff2uϕ``), the same numbers relative to the row's norm.  The worst distance
of every quantity goes to the ledger (``util.record``).  Shapes: ``cases.helper_rows`` -- all in bounds by construction."""
import pytest
from torch import tensor

from gpu_common import *  # noqa: F401,F403

pytestmark = pytest.mark.gpu

F64 = torch.float64
SHAPES = cases.helper_rows()
SHAPE_IDS = ['x'.join(str(d) for d in s) for s in SHAPES]
TOL = {'f64': 1e-9, 'f32': 1e-5}


class Worst:
    r"""Asserts every distance against its gate and keeps the worst per quantity; leaving the ``with`` block writes them to the ledger."""

    def __init__(self, prefix):
        self.prefix, self.seen = prefix, {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for k, (v, bound, where) in self.seen.items():
            record(f'{self.prefix}.{k}', v, bound, note=f'worst over the operand forms: {where}')
        return False

    def note(self, key, value, bound, where):
        if key not in self.seen or value > self.seen[key][0]:
            self.seen[key] = (value, bound, where)
        assert value <= bound, f'{self.prefix}.{key} [{where}]: {value:.3e} > {bound:.1e}'

    def close(self, key, got, want, tag, where):
        r"""``util.assert_close``'s gates: fp64 max-abs <= 1e-9, fp32 relative L2 <= 1e-5."""
        assert tuple(got.shape) == tuple(want.shape), (key, where, tuple(got.shape), tuple(want.shape))
        self.note(key, max_abs(got, want) if tag == 'f64' else rel_l2(got, want), TOL[tag], where)

    def rel(self, key, got, want, tag, where):
        r"""Relative L2 <= 1e-9 (fp64) / 1e-5 (fp32): the gates of the constant gradients."""
        assert tuple(got.shape) == tuple(want.shape), (key, where, tuple(got.shape), tuple(want.shape))
        self.note(key, rel_l2(got, want), TOL[tag], where)

    def rows(self, key, got, want, tag, where):
        r"""Row by row over the last axis: fp64 max-abs, fp32 L2, each relative to the yardstick row's norm (1 for a zero
        row) -- the gates of ``close`` per row."""
        assert tuple(got.shape) == tuple(want.shape), (key, where, tuple(got.shape), tuple(want.shape))
        a, b = got.detach().double().cpu().reshape(-1, got.shape[-1]), want.detach().double().cpu().reshape(-1, want.shape[-1])
        den = b.norm(dim=-1)
        den = torch.where(den > 0, den, torch.ones_like(den))
        d = ((a - b).abs().max(dim=-1).values if tag == 'f64' else (a - b).norm(dim=-1)) / den
        r = int(d.argmax())
        self.note(key, float(d[r]), TOL[tag], f'{where}, row {r}')


def _u(gen, *s):
    return torch.rand(s, generator=gen, dtype=F64)


def _leaf_as_given(x):
    r"""``x`` on the device in the form it has on the host (``place``), as a leaf that requires grad."""
    return place(x, DEV).requires_grad_(True)


def _up(x, dtype):
    r"""The numbers a kernel of data type ``dtype`` reads from an operand the host layer casts to it: rounded, then up."""
    return None if x is None else x.detach().to(dtype).double()


def _permuted(x):
    r"""The same values as a permuted view: ``xyz`` (the last axis) stored first."""
    return x.movedim(-1, 0).contiguous().movedim(0, -1)


def _swapped(x):
    r"""The same values as a view whose last two axes are stored swapped."""
    return x.transpose(-1, -2).contiguous().transpose(-1, -2)


# =============================================================================================
# freeprec
# =============================================================================================
FP_RANGE = {'T1': lambda u: 0.6 + u, 'T2': lambda u: 0.03 + 0.1 * u, 'Δf': lambda u: u * 200 - 100}
FP_SEED = {'T1': 51, 'T2': 52, 'Δf': 53}


def _freeprec_oracle(M, w, dur, T1, T2, Δf, dtype):
    r"""``Mo``, ``grad_Mi`` and the gradients w.r.t. the operands that are given, each in its operand's shape: autograd
    through the oracle's plain torch ops in fp64 on the rounded numbers."""
    leaf = lambda x: None if x is None else _up(x, dtype).requires_grad_(True)  # noqa: E731
    Mr, ops = leaf(M), {k: leaf(v) for k, v in (('dur', dur), ('T1', T1), ('T2', T2), ('Δf', Δf))}
    Mo = O.freeprec_slow(Mr, ops['dur'], T1=ops['T1'], T2=ops['T2'], Δf=ops['Δf'])
    (Mo * _up(w, dtype)).sum().backward()
    return Mo.detach(), Mr.grad, {k: (None if v is None else v.grad) for k, v in ops.items()}


def _freeprec_hip(M, w, dur, T1, T2, Δf):
    Mh = _leaf_as_given(M)
    ops = {k: (None if v is None else _leaf_as_given(v)) for k, v in (('dur', dur), ('T1', T1), ('T2', T2), ('Δf', Δf))}
    Mo = slowsims.freeprec(Mh, ops['dur'], T1=ops['T1'], T2=ops['T2'], Δf=ops['Δf'])
    assert Mo.grad_fn is not None and Mo.data_ptr() != Mh.data_ptr()
    (Mo * place(w, DEV)).sum().backward()
    with torch.no_grad():               # sims.freeprec: the same kernel, the same bits
        plain = sims.freeprec(Mh, ops['dur'], T1=ops['T1'], T2=ops['T2'], Δf=ops['Δf'])
    assert torch.equal(plain, Mo.detach())
    return Mo.detach(), Mh.grad, {k: (None if v is None else v.grad) for k, v in ops.items()}, ops


def _freeprec_check(W, tag, where, M, w, dur, T1, T2, Δf):
    dtype = DT[tag]
    Mo_o, gM_o, gc_o = _freeprec_oracle(M, w, dur, T1, T2, Δf, dtype)
    Mo_h, gM_h, gc_h, ops = _freeprec_hip(M, w, dur, T1, T2, Δf)
    assert Mo_h.dtype == dtype and gM_h.shape == M.shape
    W.close('Mo', Mo_h, Mo_o, tag, where)
    W.close('grad_Mi', gM_h, gM_o, tag, where)
    for k, want in gc_o.items():
        if want is None:
            assert gc_h[k] is None
            continue
        got = gc_h[k]
        assert got is not None and got.shape == ops[k].shape and got.dtype == ops[k].dtype, (where, k)
        W.rel(f'grad_{k}', got, want, tag, where)


def _freeprec_base(N, Nd, dtype, seed=61):
    r"""Dense per-spin operands, ``dur (N,)``, a permuted ``Mi`` view and a transposed cotangent."""
    gen = torch.Generator(device='cpu').manual_seed(seed + N + 10 * len(Nd))
    M = _permuted(_u(gen, N, *Nd, 3).to(dtype))
    w = _permuted(_u(gen, N, *Nd, 3).to(dtype))
    assert not M.is_contiguous() and not w.is_contiguous()
    ops = dict(dur=((2 + 4 * _u(gen, N)) * 1e-3).to(dtype), T1=FP_RANGE['T1'](_u(gen, N, *Nd)).to(dtype),
               T2=FP_RANGE['T2'](_u(gen, N, *Nd)).to(dtype), Δf=FP_RANGE['Δf'](_u(gen, N, *Nd)).to(dtype))
    return M, w, ops


@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_freeprec_rows_and_constant_forms(tag, shape):
    r"""``slowsims.freeprec`` / ``sims.freeprec``: forward, ``grad_Mi`` and the four constant gradients (each in the shape
    its operand was given in) with T1, T2, Δf in every form of ``cases.helper_constant_forms`` -- one operand at a time,
    the others per spin --, ``dur`` as ``()``, ``(1,)``, ``(N,)`` and fp64 beside fp32 data, relaxation only and
    precession only; ``Mi`` is a permuted view and the cotangent a transposed one throughout."""
    dtype, N, Nd = DT[tag], shape[0], tuple(shape[1:])
    M, w, base = _freeprec_base(N, Nd, dtype)
    with Worst(f'helpers.freeprec.{tag}.{"x".join(map(str, shape))}') as W:
        for which in ('T1', 'T2', 'Δf'):
            for name, c in cases.helper_constant_forms(N, Nd, dtype, fn=FP_RANGE[which], seed=FP_SEED[which]).items():
                _freeprec_check(W, tag, f'{which} as {name}', M, w, **dict(base, **{which: c}))
        durs = {'()': base['dur'][0].reshape(()), '(1,)': base['dur'][:1], '(N,)': base['dur'], 'f64': base['dur'].double() * 1.1}
        for name, dur in durs.items():
            _freeprec_check(W, tag, f'dur as {name}', M, w, **dict(base, dur=dur))
        _freeprec_check(W, tag, 'relaxation only', M, w, **dict(base, Δf=None))
        _freeprec_check(W, tag, 'precession only', M, w, **dict(base, T1=None, T2=None))


def test_freeprec_large_angle():
    r"""About 1000 cycles of precession: |Δf| <= 2e4 Hz, ``dur`` = (5e-2, 2e-2, 1e-2) s at shape (3, 171).  fp64: the
    standing gate.  fp32: the angle 2π Δf dur ~ 6e3 rad is held to half an ulp (~2e-4 rad) whatever the kernel does, so
    the gate is 3x the distance of THE ORACLE ITSELF run in fp32 from the fp64 oracle, computed here on the CPU and
    recorded (measured: the fp32 oracle 7.0e-5 forward, 6.4e-5 for ``grad_Mi``, the kernels the same to three digits -- both
    round the same angle; the small-angle cases sit at 1e-7)."""
    N, nM = 3, 171
    gen = torch.Generator(device='cpu').manual_seed(67)
    M64, w64 = _u(gen, N, nM, 3), _u(gen, N, nM, 3)
    ops64 = dict(dur=tensor([5e-2, 2e-2, 1e-2], dtype=F64), T1=0.6 + _u(gen, N, nM), T2=0.03 + 0.1 * _u(gen, N, nM),
                 Δf=(_u(gen, N, nM) * 2 - 1) * 2e4)
    for tag in ('f64', 'f32'):
        dtype = DT[tag]
        M, w, ops = M64.to(dtype), w64.to(dtype), {k: v.to(dtype) for k, v in ops64.items()}
        Mo_o, gM_o, _ = _freeprec_oracle(M, w, dtype=dtype, **ops)
        Mh = _leaf_as_given(M)
        Mo_h = sims.freeprec(Mh, dev(ops['dur']), T1=dev(ops['T1']), T2=dev(ops['T2']), Δf=dev(ops['Δf']))
        (Mo_h * dev(w)).sum().backward()
        if tag == 'f64':
            bound = {'Mo': 1e-9, 'grad_Mi': 1e-9}
            dist = {'Mo': max_abs(Mo_h, Mo_o), 'grad_Mi': max_abs(Mh.grad, gM_o)}
        else:
            Mr = M.clone().requires_grad_(True)                      # the oracle in fp32, CPU
            Mo_r = O.freeprec(Mr, ops['dur'], T1=ops['T1'], T2=ops['T2'], Δf=ops['Δf'])
            (Mo_r * w).sum().backward()
            own = {'Mo': rel_l2(Mo_r, Mo_o), 'grad_Mi': rel_l2(Mr.grad, gM_o)}
            for k, v in own.items():
                record(f'helpers.freeprec.large_angle.f32.oracle_in_fp32.{k}', v, note='the fp32 oracle against the fp64 oracle')
            bound = {k: 3 * v for k, v in own.items()}
            dist = {'Mo': rel_l2(Mo_h, Mo_o), 'grad_Mi': rel_l2(Mh.grad, gM_o)}
        for k in ('Mo', 'grad_Mi'):
            print(f'freeprec large angle {tag} {k}: {dist[k]:.3e} (gate {bound[k]:.3e})')
            record(f'helpers.freeprec.large_angle.{tag}.{k}', dist[k], bound[k])
            assert dist[k] <= bound[k], (tag, k, dist[k], bound[k])


@pytest.mark.parametrize('half', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
def test_freeprec_half_inputs_round_once(half):
    r"""bf16 / fp16 inputs: the result is the fp32 call on the upcast inputs, rounded once -- bit for bit."""
    N, nM = 3, 171
    gen = torch.Generator(device='cpu').manual_seed(71)
    M = _u(gen, N, nM, 3).to(half)
    ops = dict(T1=(0.6 + _u(gen, N, nM)).to(half), T2=(0.03 + 0.1 * _u(gen, N, 1)).to(half), Δf=(_u(gen, 1, nM) * 200 - 100).to(half))
    dur = tensor([2e-3, 3e-3, 5e-3]).to(half)
    for fn in (sims.freeprec, slowsims.freeprec):
        got = fn(dev(M), dev(dur), **{k: dev(v) for k, v in ops.items()})
        want = fn(dev(M).float(), dev(dur).float(), **{k: dev(v).float() for k, v in ops.items()})
        assert got.dtype == half and want.dtype == torch.float32
        assert torch.equal(got, want.to(half))


# =============================================================================================
# interpT: linear, and the empty result of every kernel-backed kind
# =============================================================================================
def _scipy_interpT(x, t_o, t_n, kind='linear'):
    r"""``Pulse.interpT`` on the host (``mobjs.py:203-217``): zero sample prepended, time on axis 2, cast back."""
    from scipy import interpolate
    x = x.numpy()
    x0 = np.concatenate([np.zeros_like(x[:, :, :1]), x], axis=2)
    if len(t_n) == 0:
        return np.zeros(x.shape[:2] + (0,) + x.shape[3:], dtype=x.dtype)
    return interpolate.interp1d(t_o, x0, axis=2, kind=kind, copy=False, assume_sorted=True)(t_n).astype(x.dtype)


def _dense_linear(nT, dt_o, dt_n):
    r"""The resampling as a dense fp64 matrix `(nTn, nT)` built from ``interp_grid`` (the prepended zero's column dropped)."""
    from mrphy_amd.interp import interp_grid
    lo, w, dx, n = interp_grid(nT, dt_o, dt_n)
    Wm = torch.zeros(n, nT + 1, dtype=F64)
    for j in range(n):
        Wm[j, lo[j] + 1] += w[j] / dx[j]
        Wm[j, lo[j]] += 1 - w[j] / dx[j]
    return Wm[:, 1:], n


@pytest.mark.parametrize('grid', cases.INTERP_GRIDS, ids=[f'{g[0]}to{g[3]}' for g in cases.INTERP_GRIDS])
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_interpT_linear_vs_scipy_and_dense_adjoint(tag, grid):
    r"""``interpT(kind='linear')`` on grids that cross a block on either side, single-coil and `(N, 2, nT, 3)` rf: the forward
    BIT-IDENTICAL to ``scipy.interpolate.interp1d`` applied as ``Pulse.interpT`` applies it (the kernel restates scipy's
    arithmetic with contraction off); the adjoint, with a non-contiguous cotangent, against the dense fp64 matrix of the
    grid; an empty result has shape `(N, C, 0)` and a zero gradient."""
    from mrphy_amd import interp
    nT, dt_o, dt_n, count = grid
    dtype = DT[tag]
    gen = torch.Generator(device='cpu').manual_seed(73 + nT)
    dt, dtn = tensor([dt_o], dtype=F64), tensor([dt_n], dtype=F64)
    t_o = np.arange(0, nT + 1) * dt.item()
    t_n = np.arange(1, t_o[-1] // dtn.item() + 1) * dtn.item()
    Wm, n = _dense_linear(nT, dt_o, dt_n)
    assert n == len(t_n) == count
    with Worst(f'helpers.interpT_linear.{tag}.{nT}to{count}') as W:
        for nC in (None, 3):
            rf = (_u(gen, 2, 2, nT, *((nC,) if nC else ())) * 2 - 1).to(dtype)
            gr = (_u(gen, 2, 3, nT) * 2 - 1).to(dtype)
            rf_h, gr_h = _leaf(rf, DEV), _leaf(gr, DEV)
            rf_n, gr_n, dt_out = interp.interpT(rf_h, gr_h, dev(dt), dev(dtn))
            assert rf_n.dtype == dtype and float(dt_out) == float(dtn.to(dtype))
            assert tuple(rf_n.shape) == (2, 2, count) + ((nC,) if nC else ()) and tuple(gr_n.shape) == (2, 3, count)
            assert np.array_equal(rf_n.detach().cpu().numpy(), _scipy_interpT(rf, t_o, t_n)), 'rf is not scipy, bit for bit'
            assert np.array_equal(gr_n.detach().cpu().numpy(), _scipy_interpT(gr, t_o, t_n)), 'gr is not scipy, bit for bit'
            # the adjoint: W^T applied to the cotangent; cotangents stored with the time axis first (not contiguous)
            w_rf = (_u(gen, *rf_n.shape) * 2 - 1).to(dtype).movedim(2, 0).contiguous().movedim(0, 2)
            w_gr = (_u(gen, *gr_n.shape) * 2 - 1).to(dtype).movedim(2, 0).contiguous().movedim(0, 2)
            assert count < 2 or not w_gr.is_contiguous()
            ((rf_n * place(w_rf, DEV)).sum() + (gr_n * place(w_gr, DEV)).sum()).backward()        # must not raise when empty
            want_gr = torch.einsum('jt,ncj->nct', Wm, w_gr.double())
            want_rf = (torch.einsum('jt,ncjk->nctk', Wm, w_rf.double()) if nC
                       else torch.einsum('jt,ncj->nct', Wm, w_rf.double()))
            assert rf_h.grad.shape == rf.shape and gr_h.grad.shape == gr.shape
            if count == 0:
                assert not rf_h.grad.any() and not gr_h.grad.any()
            W.close('grad_rf', rf_h.grad, want_rf, tag, f'nC = {nC}')
            W.close('grad_gr', gr_h.grad, want_gr, tag, f'nC = {nC}')


@pytest.mark.parametrize('code', [0, 1], ids=['f32', 'f64'])
def test_interp_adjoint_of_an_empty_result_takes_null_cotangent_and_grid(code):
    r"""The C ABI at ``nTn == 0``, adjoint direction: a null cotangent and a null grid are accepted and the gradient
    `(nch, nTo)` is zeroed, for the linear and the one-tap entry."""
    lib = mrphy_amd.require_library()
    dtype = torch.float64 if code == mrphy_amd._lib.F64 else torch.float32
    assert code in (mrphy_amd._lib.F32, mrphy_amd._lib.F64)
    nch, nTo = 5, 300
    st = torch.cuda.current_stream(DEV).cuda_stream
    for call in (lambda out: lib.mrphy_pulse_interp_linear(code, -1, None, out, None, None, None, nch, nTo, 0, st),
                 lambda out: lib.mrphy_pulse_interp_select(code, -1, None, out, None, nch, nTo, 0, st)):
        gy = torch.full((nch, nTo), 7.0, dtype=dtype, device=DEV)
        assert call(gy.data_ptr()) == 0
        assert not gy.any()
        assert call(None) == -1                                      # the gradient itself is still required


# =============================================================================================
# beff2uϕ / uϕrot and their adjoints
# =============================================================================================
G_RANGE = lambda u: 0.05 + 0.1 * u       # noqa: E731  γ2πdt around 2π·4257.6·4e-6 = 0.107


def _flat_rows(x, k=3):
    return x.detach().double().cpu().reshape(-1, k)


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_beff2uphi_tie_row_is_a_tie_on_the_device(tag):
    r"""What the special-row tests rely on: for ``b = (1e-12, 0, 0)`` as the data type holds it the kernel's norm IS
    ``eps`` as the data type holds it (``Φ = -|b| γ2πdt`` with ``γ2πdt = 1`` shows it), and ``U = (1, 0, 0)``."""
    dtype = DT[tag]
    b = cases.beff_special_row('tie', dtype).reshape(1, 1, 3)
    U, Φ = beffective.beff2uϕ(dev(b), torch.ones((), dtype=dtype, device=DEV))
    assert float(Φ) == -float(tensor(cases.BEFF_EPS, dtype=dtype)) and U.cpu().flatten().tolist() == [1., 0., 0.]


@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_beff2uphi_rows_forms_and_special_rows(tag, shape):
    r"""``beff2uϕ`` and its adjoint with ``γ2πdt`` in every constant form (fp64 beside fp32 data: the ``<float, double>``
    build), a permuted field and permuted cotangents, special rows (exact zero, |b| = 3e-13, |b| = 1e-12 exactly,
    |b| = 2e-12, an ordinary one) at flat rows 0, 255, 256 and the last, the kinds rotating from form to form.  ``U``, ``Φ``
    against the oracle; ``grad_beff`` ROW BY ROW against ``cases.beff2uphi_grad_closed`` (the tiny rows' gradients are of order
    1e11 and would hide every other row in a whole-tensor norm); ``grad_γ2πdt`` in the shape it was given in."""
    dtype, N, Nd = DT[tag], shape[0], tuple(shape[1:])
    gen = torch.Generator(device='cpu').manual_seed(79 + N + len(Nd))
    forms = cases.helper_constant_forms(N, Nd, dtype, fn=G_RANGE, seed=83)
    seen = set()
    with Worst(f'helpers.beff2uphi.{tag}.{"x".join(map(str, shape))}') as W:
        for shift, (name, g) in enumerate(forms.items()):
            b = ((_u(gen, N, *Nd, 3) * 2 - 1) * 10).to(dtype)
            planted = cases.plant_special_rows(b, shift)
            seen.update(planted.values())
            b = _permuted(b)
            gU = _permuted((_u(gen, N, *Nd, 3) * 2 - 1).to(dtype))
            gΦ = (0.3 + 1.7 * _u(gen, *Nd, N)).to(dtype).movedim(-1, 0)
            assert not b.is_contiguous() and not gU.is_contiguous() and (N == 1 or not gΦ.is_contiguous())
            wide = g.dtype == F64                                    # fp64 constants are read as fp64
            g_read = g.double() if wide else _up(g, dtype)
            gd = cases.helper_dense(g_read, N, Nd)
            U_o, Φ_o = O.beff2uphi(b.double(), gd)
            gb_o, gg_o = cases.beff2uphi_grad_closed(b.reshape(-1, 3), gd.reshape(-1), gU.reshape(-1, 3), gΦ.reshape(-1), dtype)
            lead = 1 + len(Nd)
            gshape = tuple(g.shape[:lead]) + (1,) * (lead - min(g.ndim, lead))
            gg_o = gg_o.reshape((N,) + Nd).sum_to_size(gshape).reshape(g.shape)
            b_h, g_h = _leaf_as_given(b), _leaf_as_given(g)
            U_h, Φ_h = beffective.beff2uϕ(b_h, g_h)
            assert U_h.dtype == Φ_h.dtype == dtype and Φ_h.shape == b.shape[:-1]
            ((U_h * place(gU, DEV)).sum() + (Φ_h * place(gΦ, DEV)).sum()).backward()
            where = f'γ2πdt as {name}, special rows {planted}'
            W.rows('U', U_h, U_o, tag, where)
            W.close('U_whole', U_h, U_o, tag, where)
            W.close('Phi', Φ_h, Φ_o, tag, where)
            assert torch.isfinite(b_h.grad).all() and b_h.grad.shape == b.shape
            W.rows('grad_beff', b_h.grad, gb_o.reshape(b.shape), tag, where)
            assert g_h.grad.shape == g.shape and g_h.grad.dtype == g.dtype
            W.rel('grad_g', g_h.grad, gg_o, tag, where)
    assert seen == set(cases.HELPER_SPECIAL)


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_beff2uphi_dim_1(tag):
    r"""``beff2uϕ(dim=1)`` on a `(N, xyz, nM)` field: ``U`` comes back in that layout, ``Φ`` `(N, nM)`, gradients too."""
    dtype, N, nM = DT[tag], 3, 171
    gen = torch.Generator(device='cpu').manual_seed(89)
    b = ((_u(gen, N, 3, nM) * 2 - 1) * 10).to(dtype)
    g = G_RANGE(_u(gen, N, 1)).to(dtype)
    gU, gΦ = (_u(gen, N, 3, nM) * 2 - 1).to(dtype), (0.3 + _u(gen, N, nM)).to(dtype)
    b_o = _up(b, dtype).clone().requires_grad_(True)
    U_o, Φ_o = O.beff2uphi(b_o, g.double(), dim=1)
    ((U_o * gU.double()).sum() + (Φ_o * gΦ.double()).sum()).backward()
    b_h = _leaf(b, DEV)
    U_h, Φ_h = beffective.beff2uϕ(b_h, dev(g), dim=1)
    assert U_h.shape == (N, 3, nM) and Φ_h.shape == (N, nM)
    ((U_h * dev(gU)).sum() + (Φ_h * dev(gΦ)).sum()).backward()
    with Worst(f'helpers.beff2uphi_dim1.{tag}') as W:
        W.close('U', U_h, U_o, tag, 'dim=1')
        W.close('Phi', Φ_h, Φ_o, tag, 'dim=1')
        W.rows('grad_beff', b_h.grad.movedim(1, -1), b_o.grad.movedim(1, -1), tag, 'dim=1')


def _phi_forms(N, Nd, dtype, gen):
    one = (1,) * len(Nd)
    mk = lambda *s: ((_u(gen, *s) * 2 - 1) * 3).to(dtype)  # noqa: E731
    return {'(N, *Nd)': mk(N, *Nd), '(1, *Nd)': mk(1, *Nd), '(N, 1)': mk(N, *one)}


@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_uphirot_rows_nV_and_gradients(tag, shape):
    r"""``utils.uϕrot`` and its adjoint: ``nV`` absent, 1, 4, 5 (so that ``i / nV`` is not a shift), a NON-UNIT ``U`` (the
    formula holds for any ``U``; |U| = 1 hides errors in the ``(1 - c)`` terms), ``Φ`` per spin, per spin of one entry and
    per batch entry, ``Vi`` and the cotangent as views; gradients w.r.t. ``U``, ``Φ``, ``Vi`` each alone (the kernel's
    null-pointer branches) and all together, against autograd through the oracle."""
    dtype, N, Nd = DT[tag], shape[0], tuple(shape[1:])
    gen = torch.Generator(device='cpu').manual_seed(97 + N + len(Nd))
    with Worst(f'helpers.uphirot.{tag}.{"x".join(map(str, shape))}') as W:
        for nV, (pname, Φ) in zip((None, 1, 4, 5), list(_phi_forms(N, Nd, dtype, gen).items()) * 2):
            tail = (3,) if nV is None else (3, nV)
            U = _permuted(((_u(gen, N, *Nd, 3) * 2 - 1) * 1.5).to(dtype))
            Vi = _swapped((_u(gen, N, *Nd, *tail) * 2 - 1).to(dtype)) if nV else _permuted((_u(gen, N, *Nd, 3) * 2 - 1).to(dtype))
            G = (_u(gen, *tail[::-1], *Nd[::-1], N) * 2 - 1).to(dtype).permute(*range(len(tail) + len(Nd), -1, -1))
            assert G.shape == Vi.shape and not G.is_contiguous()
            ins_o = [_up(x, dtype).clone().requires_grad_(True) for x in (U, Φ, Vi)]
            Vo_o = O.uphirot(*ins_o)
            (Vo_o * G.double()).sum().backward()
            where = f'nV = {nV}, Φ as {pname}'
            for need in ((0, 1, 2), (0,), (1,), (2,)):
                ins_h = [(_leaf_as_given(x) if i in need else place(x, DEV)) for i, x in enumerate((U, Φ, Vi))]
                Vo_h = utils.uϕrot(*ins_h)
                assert Vo_h.shape == Vi.shape and Vo_h.dtype == dtype
                (Vo_h * place(G, DEV)).sum().backward()
                W.close('Vo', Vo_h, Vo_o, tag, where)
                for i, nm in enumerate(('U', 'Phi', 'Vi')):
                    if i in need:
                        W.close(f'grad_{nm}', ins_h[i].grad, ins_o[i].grad, tag, f'{where}, grads of {need}')
                    else:
                        assert ins_h[i].grad is None


@pytest.mark.parametrize('nV', [None, 4])
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_uphirot_broadcasts_U_over_the_batch_or_raises(tag, nV):
    r"""A ``U`` `(1, nM, 3)` against ``Vi`` `(N, nM, 3[, nV])`: broadcast as the reference does (``U.expand_as(Vi)``) --
    every row is written and ``grad_U`` comes back `(1, nM, 3)`, summed over the batch; a leading shape that cannot
    broadcast raises, it never returns unwritten rows."""
    dtype, N, nM = DT[tag], 3, 171
    gen = torch.Generator(device='cpu').manual_seed(101)
    tail = (3,) if nV is None else (3, nV)
    U, Φ = ((_u(gen, 1, nM, 3) * 2 - 1) * 1.5).to(dtype), ((_u(gen, 1, nM) * 2 - 1) * 3).to(dtype)
    Vi, G = (_u(gen, N, nM, *tail) * 2 - 1).to(dtype), (_u(gen, N, nM, *tail) * 2 - 1).to(dtype)
    ins_o = [_up(x, dtype).clone().requires_grad_(True) for x in (U, Φ, Vi)]
    Vo_o = O.uphirot(*ins_o)
    (Vo_o * G.double()).sum().backward()
    ins_h = [_leaf(x, DEV) for x in (U, Φ, Vi)]
    Vo_h = utils.uϕrot(*ins_h)
    (Vo_h * dev(G)).sum().backward()
    with Worst(f'helpers.uphirot_broadcast.{tag}.nV{nV}') as W:
        W.close('Vo', Vo_h, Vo_o, tag, 'U (1, nM, 3)')
        W.rows('Vo_rows', Vo_h.reshape(N * nM, -1), Vo_o.reshape(N * nM, -1), tag, 'U (1, nM, 3)')
        for nm, h, o in zip(('U', 'Phi', 'Vi'), ins_h, ins_o):
            W.close(f'grad_{nm}', h.grad, o.grad, tag, 'U (1, nM, 3)')
    with pytest.raises(RuntimeError):
        utils.uϕrot(dev(U.expand(2, nM, 3).contiguous()), dev(Φ), dev(Vi))


# =============================================================================================
# blochsim_1step, the no-grad kernel
# =============================================================================================
DT0 = cases.dt0_val
E_FN = {'E1': lambda u: torch.exp(-DT0 * 200 / (0.5 + u)), 'E2': lambda u: torch.exp(-DT0 * 200 / (0.02 + 0.1 * u))}


@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_onestep_nograd_rows_and_constant_forms(tag, shape):
    r"""``slowsims.blochsim_1step`` without a graph (``mrphy_blochsim_1step``) against the oracle, with γ2πdt, E1 (and E1 - 1,
    which travels with E1's strides) and E2 in every constant form, one at a time; zero-field rows at the block edges;
    the same bits as the grad path (``mrphy_blochsim_fwd``, nT = 1)."""
    dtype, N, Nd = DT[tag], shape[0], tuple(shape[1:])
    gen = torch.Generator(device='cpu').manual_seed(103 + N + len(Nd))
    M = _u(gen, N, *Nd, 3).to(dtype)
    b = ((_u(gen, N, *Nd, 3) * 2 - 1) * 10).to(dtype)
    for p in cases.helper_special_positions(b.view(-1, 3).shape[0]):
        b.view(-1, 3)[p] = 0
    dense = dict(g=G_RANGE(_u(gen, N, *Nd)).to(dtype), E1=E_FN['E1'](_u(gen, N, *Nd)).to(dtype), E2=E_FN['E2'](_u(gen, N, *Nd)).to(dtype))
    dense['E1_1'] = dense['E1'] - 1

    def variants():
        for name, c in cases.helper_constant_forms(N, Nd, dtype, fn=G_RANGE, seed=107).items():
            yield f'γ2πdt as {name}', dict(dense, g=c)
        e1 = cases.helper_constant_forms(N, Nd, dtype, fn=E_FN['E1'], seed=109)
        e1m1 = cases.helper_constant_forms(N, Nd, dtype, fn=lambda u: E_FN['E1'](u).to(dtype).double() - 1, seed=109)
        for name in e1:
            m1 = e1m1[name] if e1[name].dtype == dtype else e1[name] - 1      # the same form; fp64: the fp64 difference
            yield f'E1, E1_1 as {name}', dict(dense, E1=e1[name], E1_1=m1)
        yield 'E1 expanded, E1_1 dense', dict(dense, E1=e1['expanded'], E1_1=(e1['expanded'] - 1).contiguous())
        for name, c in cases.helper_constant_forms(N, Nd, dtype, fn=E_FN['E2'], seed=113).items():
            yield f'E2 as {name}', dict(dense, E2=c)
    with Worst(f'helpers.onestep_nograd.{tag}.{"x".join(map(str, shape))}') as W:
        for where, c in variants():
            read = {k: cases.helper_dense(v.double() if v.dtype == F64 else _up(v, dtype), N, Nd) for k, v in c.items()}
            want, _ = O.blochsim_1step(M.double().clone(), None, b.double(), read['E1'], read['E1_1'], read['E2'], read['g'])
            ch = {k: place(v, DEV) for k, v in c.items()}
            Md, bd = dev(M), dev(b)
            with torch.no_grad():
                got, old = slowsims.blochsim_1step(Md, Md, bd, ch['E1'], ch['E1_1'], ch['E2'], ch['g'])
            assert old is Md and got.grad_fn is None and got.dtype == dtype
            W.close('M_new', got, want, tag, where)
            Mg = Md.clone().requires_grad_(True)
            via_grad, _ = slowsims.blochsim_1step(Mg, Mg, bd, ch['E1'], ch['E1_1'], ch['E2'], ch['g'])
            assert via_grad.grad_fn is not None and torch.equal(via_grad.detach(), got), where


# =============================================================================================
# blochsim_ab
# =============================================================================================
@pytest.mark.parametrize('shape', SHAPES[:4], ids=SHAPE_IDS[:4])
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_blochsim_ab_rows_views_and_gradient_subsets(tag, shape):
    r"""``slowsims.blochsim_ab`` at 255, 256, 257 and 513 rows: ``A`` as a ``transpose(-1, -2)`` view of its stored transpose
    and, with fp32 ``M``, fp64 ``A`` and ``B``; every subset of {``M``, ``A``, ``B``} requiring grad, a non-contiguous
    cotangent.  ``grad_A`` is one product per entry: ``g[..., :, None] * M[..., None, :]`` in the data type, bit for bit;
    ``grad_B`` is the cotangent; ``Mo`` and ``grad_M`` go to the gates."""
    dtype, N, nM = DT[tag], shape[0], shape[1]
    gen = torch.Generator(device='cpu').manual_seed(127 + N * nM)
    M = (_u(gen, N, nM, 3) * 2 - 1).to(dtype)
    g = _permuted((_u(gen, N, nM, 3) * 2 - 1).to(dtype))
    kinds = {'transposed view': dtype, 'fp64 A, B': F64} if tag == 'f32' else {'transposed view': dtype}
    with Worst(f'helpers.blochsim_ab.{tag}.{N}x{nM}') as W:
        for kind, adt in kinds.items():
            A = _swapped((_u(gen, N, nM, 3, 3) * 2 - 1).to(adt))
            B = (_u(gen, N, nM, 3) * 2 - 1).to(adt)
            assert not A.is_contiguous()
            ins_o = [_up(x, dtype).requires_grad_(True) for x in (M, A, B)]
            Mo_o = O.blochsim_ab(*ins_o)
            (Mo_o * g.double()).sum().backward()
            gA_bits = (g[..., :, None] * M[..., None, :])
            for need in ((), (0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)):
                ins_h = [(_leaf_as_given(x) if i in need else place(x, DEV)) for i, x in enumerate((M, A, B))]
                Mo_h = slowsims.blochsim_ab(*ins_h)
                where = f'{kind}, grads of {need}'
                W.close('Mo', Mo_h, Mo_o, tag, where)
                if not need:
                    assert Mo_h.grad_fn is None
                    continue
                (Mo_h * place(g, DEV)).sum().backward()
                for i in range(3):
                    assert (ins_h[i].grad is not None) == (i in need), where
                if 0 in need:
                    W.close('grad_M', ins_h[0].grad, ins_o[0].grad, tag, where)
                if 1 in need:
                    assert ins_h[1].grad.dtype == adt and torch.equal(ins_h[1].grad.cpu(), gA_bits.to(adt)), where
                if 2 in need:
                    assert torch.equal(ins_h[2].grad.cpu(), g.to(adt)), where


# =============================================================================================
# mask extract / embed, cube_loc
# =============================================================================================
MASK_NDS = ((300,), (17, 19), (3, 4, 5, 2))
TAILS = ((), (3,), (2, 3))                   # K = 1, 3, 6


def _payload(shape, dtype, a):
    n = int(np.prod(shape)) if shape else 1
    k = torch.arange(n, dtype=torch.int64)
    v = ((k * a + 11) % 2039 - 1019).reshape(shape)
    if dtype.is_complex:
        return torch.complex((v / 64).float(), (v.flip(0) / 32).float())
    return v.to(dtype) if not dtype.is_floating_point else (v.to(F64) / 64).to(dtype)


@pytest.mark.parametrize('Nd', MASK_NDS, ids=['rank1', 'rank2', 'rank4'])
def test_masks_ranks_tails_and_payloads(Nd):
    r"""``masks.extract`` / ``masks.embed`` at mask ranks 1, 2 and 4, trailing sizes K = 1, 3, 6 (the kernels' index runs over
    voxel x K: past one block at every rank), N = 2: ``extract`` of float32, float64, int32, int64 and complex64 payloads (elements move as raw 4- and 8-byte
    words) and of a permuted ``v``; ``embed`` fresh (NaN outside) and into ``out=``; ``extract`` into ``out_=``; the
    gradients -- everything bit-exact against ``O.mask_extract`` / ``O.mask_embed``.  A 2-byte payload raises."""
    N = 2
    mask = cases.helper_mask(Nd)
    ix = masks.MaskIndex(dev(mask))
    nM = int(mask.sum())
    assert ix.nM == nM and ix.nV * 6 > cases.HELPER_BLOCK
    for tail in TAILS:
        for dtype in (torch.float32, torch.float64, torch.int32, torch.int64, torch.complex64):
            v = _payload((N,) + Nd + tail, dtype, 37)
            want = O.mask_extract(v, mask)
            got = masks.extract(dev(v), ix)
            assert got.dtype == dtype and got.shape == (N, nM) + tail and torch.equal(got.cpu(), want), (tail, dtype)
            if tail:                                                  # a permuted view: the trailing axes stored first
                vp = v.movedim(-1, 0).contiguous().movedim(0, -1)
                assert not vp.is_contiguous() and torch.equal(masks.extract(place(vp, DEV), ix).cpu(), want)
            out_ = torch.zeros((N, nM) + tail, dtype=dtype, device=DEV)
            assert masks.extract(dev(v), ix, out_=out_).data_ptr() == out_.data_ptr() and torch.equal(out_.cpu(), want)
        for dtype in (torch.float32, torch.float64):
            v_ = _payload((N, nM) + tail, dtype, 41)
            fresh = masks.embed(dev(v_), ix)
            assert np.array_equal(fresh.cpu().numpy(), O.mask_embed(v_, mask).numpy(), equal_nan=True), (tail, dtype)
            base = _payload((N,) + Nd + tail, dtype, 13)
            out = dev(base).clone()
            assert masks.embed(dev(v_), dev(mask), out=out).data_ptr() == out.data_ptr()
            assert torch.equal(out.cpu(), O.mask_embed(v_, mask, out=base.clone())), (tail, dtype)
            # extract and embed are each other's adjoints
            w_, w = _payload((N, nM) + tail, dtype, 17), _payload((N,) + Nd + tail, dtype, 19)
            vg = _leaf(_payload((N,) + Nd + tail, dtype, 37), DEV)
            (masks.extract(vg, ix) * dev(w_)).sum().backward()
            vo = _payload((N,) + Nd + tail, dtype, 37).requires_grad_(True)
            (O.mask_extract(vo, mask) * w_).sum().backward()
            assert torch.equal(vg.grad.cpu(), vo.grad), (tail, dtype)
            vg_ = _leaf(v_, DEV)
            torch.nan_to_num(masks.embed(vg_, ix) * dev(w)).sum().backward()
            assert torch.equal(vg_.grad.cpu(), O.mask_extract(w, mask)), (tail, dtype)
    with pytest.raises(RuntimeError, match='element size 2'):
        masks.extract(dev(_payload((N,) + Nd, torch.float16, 37)), ix)


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_cube_loc_past_one_block(tag):
    r"""``masks.cube_loc`` with more spins than one block (7 x 8 x 9 voxels, N = 2): bit-exact against the oracle."""
    dtype, Nd = DT[tag], (7, 8, 9)
    mask = cases.helper_mask(Nd)
    assert int(mask.sum()) > cases.HELPER_BLOCK
    fov = tensor([[24., 20., 7.5], [3., 30., 12.]], dtype=dtype)
    ofst = tensor([[0., 0.5, -1.25], [2., 0., 0.125]], dtype=dtype)
    assert torch.equal(masks.cube_loc(dev(mask), dev(fov), dev(ofst)).cpu(), O.cube_loc(mask, fov, ofst))
