r"""The helper kernels without a GPU: the oracle-side facts that ``tests/test_helpers_operands.py`` relies on (the closed
form of the ``beff2uϕ`` adjoint around its clamp, ``O.uphirot`` for a non-unit axis, the sample counts of the resampling
grids, the constant-form generator) and the return codes of the helpers' C entry points BEFORE any launch -- every
pointer here is fake and never dereferenced."""
import numpy as np
import pytest
import torch
from torch import tensor

import bloch_oracle as O
import cases
import mrphy_amd
from util import FAKE

EINVAL = -1
F64 = torch.float64


def _lib():
    return mrphy_amd.require_library()


# ---------------------------------------------------------------------------------------------
# oracle checks
# ---------------------------------------------------------------------------------------------
def _special_field(dtype, shape=(3, 171)):
    gen = torch.Generator(device='cpu').manual_seed(5)
    rnd = lambda *s: torch.rand(s, generator=gen, dtype=F64) * 2 - 1  # noqa: E731
    b = (rnd(*shape, 3) * 10).to(dtype)
    kinds = {}
    flat = b.view(-1, 3)
    for i, kind in enumerate(cases.HELPER_SPECIAL * 2):              # every kind twice, first rows and around the block edge
        p = (i if i < 5 else cases.HELPER_BLOCK - 3 + i - 5)
        flat[p] = cases.beff_special_row(kind, dtype)
        kinds[p] = kind
    g = (0.05 + 0.1 * torch.rand(shape, generator=gen, dtype=F64)).to(dtype)
    return b, g, rnd(*shape, 3).to(dtype), (0.3 + 1.7 * torch.rand(shape, generator=gen, dtype=F64)).to(dtype), kinds


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
def test_beff2uphi_closed_form_is_torch_autograd_below_at_and_above_the_clamp(dtype):
    r"""``cases.beff2uphi_grad_closed`` (fp64 arithmetic, the clamp decided as the data type decides it) against torch's
    autograd through ``O.beff2uphi`` IN the data type, row by row relative to the row's norm: exact zero, |b| = 3e-13,
    the tie |b| = 1e-12, |b| = 2e-12 and ordinary rows.  At the tie ``clamp_min``'s backward passes the gradient (``>=``):
    the x component of ``grad_b`` is the Φ branch alone, about -gΦ γ2πdt, where the clamped branch would give
    ``gU_x / eps`` ~ 1e11 (in fp32 torch loses the Φ term to the rounding of two 1e12-sized terms and returns 0.0 there)."""
    b, g, gU, gΦ, kinds = _special_field(dtype)
    bl = b.clone().requires_grad_(True)
    gl = g.clone().requires_grad_(True)
    U, Φ = O.beff2uphi(bl, gl)
    ((U * gU).sum() + (Φ * gΦ).sum()).backward()
    gb, gg = cases.beff2uphi_grad_closed(b.reshape(-1, 3), g.reshape(-1), gU.reshape(-1, 3), gΦ.reshape(-1), dtype)
    want = bl.grad.double().reshape(-1, 3)
    den = want.norm(dim=-1)
    den = torch.where(den > 0, den, torch.ones_like(den))
    d = (gb - want).norm(dim=-1) / den
    tol = 1e-12 if dtype == torch.float64 else 2e-6     # the data type's own rounding of torch's three-term sum
    assert float(d.max()) <= tol, (int(d.argmax()), float(d.max()))
    assert float(((gg - gl.grad.double().reshape(-1)).abs() / (1e-30 + gg.abs())).max()) <= (1e-12 if dtype == torch.float64 else 1e-6)
    ties = [p for p, k in kinds.items() if k == 'tie']
    assert len(ties) == 2
    for p in ties:
        x_free = float(gb[p, 0])
        assert abs(x_free + float(gΦ.reshape(-1)[p].double() * g.reshape(-1)[p].double())) <= 1e-3 * abs(x_free)
        assert abs(float(gU.reshape(-1, 3)[p, 0])) > 1e-3           # so the clamped branch would be ~1e9 or more away
        if dtype == torch.float64:
            assert abs(float(want[p, 0]) - x_free) <= 1e-2          # torch: the Φ branch (plus 1e12-sized cancellation noise)
        else:
            assert abs(float(want[p, 0])) < 1e6 < 1e-4 * float(den[p])       # torch fp32: the clamp passed the gradient too
    # ... and away from the special rows the closed form is the ordinary F.normalize / norm backward
    plain = torch.ones(b.reshape(-1, 3).shape[0], dtype=torch.bool)
    plain[list(kinds)] = False
    assert float(d[plain].max()) <= (1e-13 if dtype == torch.float64 else 2e-6)


def test_oracle_uphirot_with_a_non_unit_axis_against_finite_differences():
    r"""``O.uphirot`` is the formula ``c V + (1 - c)(U·V) U + s U x V`` for ANY ``U`` (the reference never normalises inside
    ``uϕrot``): its autograd gradients w.r.t. ``U``, ``Φ``, ``Vi`` agree with central differences in fp64, `(…, 3)` and
    `(…, 3, nV)`, and a ``U`` `(1, nM, 3)` broadcasts over the batch of ``Vi``."""
    gen = torch.Generator(device='cpu').manual_seed(7)
    rnd = lambda *s: torch.rand(s, generator=gen, dtype=F64) * 2 - 1  # noqa: E731
    for tail, lead_u in (((3,), (2, 5)), ((3, 4), (2, 5)), ((3, 5), (1, 5))):
        U, Φ, V, G = rnd(*lead_u, 3) * 1.5, rnd(*lead_u) * 3, rnd(2, 5, *tail), rnd(2, 5, *tail)
        assert float((U.norm(dim=-1) - 1).abs().min()) > 1e-3
        ins = [x.clone().requires_grad_(True) for x in (U, Φ, V)]
        (O.uphirot(*ins) * G).sum().backward()
        f = lambda *a: float((O.uphirot(*a) * G).sum())  # noqa: E731
        h = 1e-6
        for i, x in enumerate((U, Φ, V)):
            fd = torch.zeros_like(x)
            for j in range(x.numel()):
                e = torch.zeros_like(x).reshape(-1)
                e[j] = h
                e = e.reshape(x.shape)
                args_p = [x + e if k == i else y for k, y in enumerate((U, Φ, V))]
                args_m = [x - e if k == i else y for k, y in enumerate((U, Φ, V))]
                fd.reshape(-1)[j] = (f(*args_p) - f(*args_m)) / (2 * h)
            assert float((fd - ins[i].grad).abs().max()) <= 1e-7, (tail, i)


def test_interp_grid_sample_counts_of_the_helper_grids():
    r"""The new sample counts ``cases.INTERP_GRIDS`` states, by the reference's own float64 ``//`` (``mobjs.py:211-212``)."""
    from mrphy_amd.interp import interp_grid, interp_select
    for nT, dt_o, dt_n, count in cases.INTERP_GRIDS:
        lo, w, dx, n = interp_grid(nT, dt_o, dt_n)
        assert n == count == len(lo) == len(w) == len(dx), (nT, n)
        assert interp_select(nT, dt_o, dt_n, 'nearest')[1] == count
        if n:
            assert lo.min() >= 0 and lo.max() <= nT - 1 and np.all(np.diff(lo) >= 0) and np.all(w <= dx) and np.all(w > 0)
    lo, w, dx, _ = interp_grid(600, 4e-6, 8e-6)
    assert np.array_equal(w, dx)                                     # weights exactly 1 and exactly 0
    lo, _, _, _ = interp_grid(257, 4e-6, 1.5e-6)
    assert np.bincount(lo).max() == 3                                # up to 3 outputs per source interval
    lo, _, _, _ = interp_grid(300, 4e-6, 1.3e-5)
    assert 300 - len(np.unique(lo)) == 208                           # source samples that are no interval's upper end


def test_helper_constant_forms_hold_what_they_say():
    r"""Every form broadcasts over ``(N, *Nd)``; the views are views (stride 0, transposed, offset); two calls with one seed
    share shapes and strides, as E1 and E1 - 1 must."""
    for shape in cases.helper_rows():
        N, Nd = shape[0], tuple(shape[1:])
        a = cases.helper_constant_forms(N, Nd, torch.float32, seed=3)
        b = cases.helper_constant_forms(N, Nd, torch.float32, fn=lambda u: u - 1, seed=3)
        assert a['f64'].dtype == F64 and a['scalar'].ndim == 0 and a['after'].storage_offset() == 1
        assert 0 in a['expanded'].stride() and a['expanded'].shape == (N,) + Nd
        if len(Nd) == 1:
            assert a['transposed'].shape == (N, Nd[0]) and a['transposed'].stride() == (1, N)
        else:
            assert a['planes'].shape == (N, Nd[0], 1, 1) and a['in_plane'].shape == (1, 1) + Nd[1:]
        for k in a:
            assert a[k].shape == b[k].shape and a[k].stride() == b[k].stride() and a[k].dtype == b[k].dtype
            d = cases.helper_dense(a[k], N, Nd)
            assert d.shape == (N,) + Nd and d.dtype == F64
            assert torch.allclose(cases.helper_dense(b[k], N, Nd), d - 1, atol=1e-6)
    rows = [int(np.prod(s)) for s in cases.helper_rows()]
    assert rows == [255, 256, 257, 513, 280]
    assert cases.helper_special_positions(513) == (0, 255, 256, 512) and cases.helper_special_positions(255) == (0, 254)


# ---------------------------------------------------------------------------------------------
# C ABI: return codes before any launch
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [0, 1])
def test_interp_entries_reject_bad_arguments_on_the_host(dtype):
    r"""More channels than a grid's y extent takes (65535) in either direction: MRPHY_EINVAL.  An empty result
    (``nTn == 0``) forward, and an empty source (``nTo == 0``) in the adjoint direction: 0, nothing to do, whatever the
    pointers.  The adjoint of an empty result still needs the gradient it zeroes: MRPHY_EINVAL for a null ``out`` -- but
    no longer for a null cotangent or a null grid (that call launches, so it is made with real memory in
    ``test_helpers_operands.py::test_interp_adjoint_of_an_empty_result_takes_null_cotangent_and_grid``)."""
    lib = _lib()
    lin = lambda d, y, out, grid, nch, nTo, nTn: lib.mrphy_pulse_interp_linear(  # noqa: E731
        dtype, d, y, out, grid, grid, grid, nch, nTo, nTn, None)
    sel = lambda d, y, out, grid, nch, nTo, nTn: lib.mrphy_pulse_interp_select(  # noqa: E731
        dtype, d, y, out, grid, nch, nTo, nTn, None)
    for fn in (lin, sel):
        for d in (1, -1):
            assert fn(d, FAKE, FAKE, FAKE, 65536, 8, 8) == EINVAL
            assert fn(d, FAKE, FAKE, FAKE, -1, 8, 8) == EINVAL
            assert fn(d, FAKE, FAKE, FAKE, 0, 8, 8) == 0
            assert fn(d, FAKE, None, FAKE, 4, 8, 8) == EINVAL
            assert fn(d, None, FAKE, FAKE, 4, 8, 8) == EINVAL        # with samples to resample, y is required
            assert fn(d, FAKE, FAKE, None, 4, 8, 8) == EINVAL        # ... and so is the grid
        assert fn(1, None, None, None, 4, 8, 0) == 0                 # forward to an empty result
        assert fn(-1, None, None, None, 4, 0, 8) == 0                # adjoint onto an empty source
        assert fn(-1, None, None, None, 4, 8, 0) == EINVAL           # adjoint of an empty result: `out` is written
        assert fn(-1, FAKE, None, FAKE, 4, 8, 0) == EINVAL
    assert lib.mrphy_pulse_interp_linear(7, 1, FAKE, FAKE, FAKE, FAKE, FAKE, 4, 8, 8, None) == EINVAL
    assert lib.mrphy_pulse_interp_select(7, 1, FAKE, FAKE, FAKE, 4, 8, 8, None) == EINVAL


def test_mask_and_cube_loc_entries_reject_a_batch_beyond_the_grid():
    r"""``N`` is the grid's y extent: more than 65535 batch entries is MRPHY_EINVAL for extract, embed and cube_loc, as is
    an element size other than 4 or 8 bytes; empty problems return 0."""
    lib = _lib()
    ext = lambda eb=4, N=2, nV=64, nM=32, K=3: lib.mrphy_mask_extract(eb, FAKE, FAKE, FAKE, N, nV, nM, K, None)  # noqa: E731
    emb = lambda eb=4, N=2, nV=64, nM=32, K=3: lib.mrphy_mask_embed(eb, FAKE, FAKE, FAKE, N, nV, nM, K, 0, 0, None)  # noqa: E731
    loc = lambda dt=0, N=2, nM=32, n=(4, 4, 4): lib.mrphy_cube_loc(dt, FAKE, FAKE, FAKE, FAKE, N, nM, *n, None)  # noqa: E731
    for fn in (ext, emb):
        assert fn(N=65536) == EINVAL
        assert fn(eb=2) == EINVAL and fn(eb=16) == EINVAL
        assert fn(nM=65, nV=64) == EINVAL
        assert fn(N=0) == 0 and fn(K=0) == 0
    assert ext(nM=0) == 0
    assert loc(N=65536) == EINVAL and loc(dt=7) == EINVAL and loc(nM=65) == EINVAL and loc(n=(4, 0, 4)) == EINVAL
    assert loc(N=0) == 0 and loc(nM=0) == 0


def test_masks_refuse_a_two_byte_payload_by_its_element_size():
    r"""The payload check of ``masks.extract`` comes before any device work: a 2-byte dtype is refused by its element
    size; a 4-byte integer payload passes that check (and then meets the refusal of CPU tensors)."""
    mask = torch.ones(1, 4, dtype=torch.bool)
    for half in (torch.float16, torch.bfloat16, torch.int16):
        with pytest.raises(RuntimeError, match='element size 2'):
            mrphy_amd.masks.extract(torch.zeros(1, 4, dtype=half), mask)
    for word in (torch.int32, torch.int64, torch.complex64, torch.float32):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            mrphy_amd.masks.extract(torch.zeros(1, 4, dtype=word), mask)
