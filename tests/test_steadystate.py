r"""``fused.ab_steadystate`` (Kss / Kssb: ``mrphy_ab_steadystate_fwd`` / ``_bwd``) and ``fused.steadystate_rfgr`` on the
device.

What is claimed where.  The kernels compute in fp64 and round once, so ALONE they are held tight: against the fp64
torch solve on the CPU of the same numbers, fp64 max abs 1e-9 and fp32 relative L2 1e-6 (ten fp32 unit roundoffs), values
and every gradient (§1, §2).  End to end in fp32 the result inherits the rounding of ``A`` amplified by the conditioning of
``I - A F`` (``fused.steadystate_rfgr``'s docstring), so the project's 1e-5 gate is applied where nothing is amplified --
the fixed-point property, §4 -- and the distance to the fp64 fixture is held to three times what the reference's own
all-fp32 route loses on the same numbers (§5; recorded in the parity ledger).
"""
import functools
from math import pi as π

import pytest

from gpu_common import *  # noqa: F401,F403
from test_ab_rfgr_host import fixture_inputs
from test_fused_traj import _problem
from test_steadystate_host import oracle_steadystate, torch_steadystate

pytestmark = pytest.mark.gpu

MODES = ['f64', 'f32-precise', 'f32-fast']
CONSTS = ('rest', 'T1', 'T2', 'df')


def _mode(tag_mode):
    tag, _, mode = tag_mode.partition('-')
    return tag, mrphy_amd.precision(mode or 'precise')


def _gate(got, want, tag, what):
    r"""The kernel-alone gates: fp64 max abs <= 1e-9 -- a gradient (``what`` names a ``grad_*``) in units of the largest
    |element| of the yardstick --, fp32 relative L2 <= 1e-6 (ten fp32 unit roundoffs: one rounding of an fp64 result)."""
    want = torch.as_tensor(want).detach().double().cpu()
    assert tuple(got.shape) == tuple(want.shape), (what, tuple(got.shape), tuple(want.shape))
    assert bool(torch.isfinite(got).all()), what
    if tag == 'f64':
        scale = float(want.abs().max()) if 'grad' in what and want.numel() else 1.0
        scale = scale if scale > 0 else 1.0
        d = max_abs(got, want) / scale
        assert d <= 1e-9, f'{what}: max abs over scale {d:.3e} > 1e-9'
    else:
        d = rel_l2(got, want)
        assert d <= 1e-6, f'{what}: rel-L2 {d:.3e} > 1e-6'


@functools.lru_cache(maxsize=None)
def _kernel_problem(N, nM, tag):
    r"""Seeded ``A = 0.97 Q`` (``Q`` orthogonal), ``B``, the rest's operands and the weights ``w`` in the data type, on the
    CPU; and the fp64 yardstick of the same numbers: ``Mss`` and the gradients of ``(Mss w).sum()`` by autograd through
    ``torch.linalg.solve``.  Computed once per shape, never modified."""
    gen = torch.Generator().manual_seed(1000 * N + nM)
    rnd = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64)  # noqa: E731
    Q = torch.linalg.qr(torch.randn((N, nM, 3, 3), generator=gen, dtype=torch.float64))[0]
    P = dict(A=0.97 * Q, B=torch.randn((N, nM, 3), generator=gen, dtype=torch.float64),
             rest=torch.tensor([5e-3, 6.5e-3], dtype=torch.float64)[:N], T1=0.05 + 0.1 * rnd(N, nM),
             T2=0.02 + 0.05 * rnd(N, nM), df=(rnd(N, nM) * 2 - 1) * 200,
             w=torch.sin(torch.arange(N * nM * 3, dtype=torch.float64) * 0.37 + 0.3).reshape(N, nM, 3))
    P = {k: v.to(DT[tag]) for k, v in P.items()}
    return P, _yardstick(P)


def _yardstick(P, use=CONSTS):
    L = {k: P[k].double().clone().requires_grad_(True) for k in ('A', 'B') + tuple(use)}
    Mss = torch_steadystate(L['A'], L['B'], **{k: L[k] for k in use})
    (Mss * P['w'].double()).sum().backward()
    # (a rest without relaxation or precession changes nothing: autograd leaves its gradient None, the kernel writes 0)
    out = {'grad_' + k: (torch.zeros_like(x) if x.grad is None else x.grad) for k, x in L.items()}
    out['Mss'] = Mss.detach()
    return out


def _run(P, use=CONSTS, over=None, leaves=None, loss=None):
    r"""``Mss`` and the gradients of ``(Mss w).sum()`` w.r.t. ``A, B`` and the operands ``use`` through
    ``fused.ab_steadystate`` on the device; ``over``: tensors that replace operands (operand forms); ``leaves``: the
    names of the operands that require grad (all of them by default; the others' gradients come back ``None``);
    ``loss``: a callable that is handed ``Mss`` and runs the backward pass itself, instead of ``(Mss w).sum()``."""
    wanted = lambda k: leaves is None or k in leaves  # noqa: E731
    L = {k: dev(P[k]).clone().requires_grad_(wanted(k)) for k in ('A', 'B') + tuple(use)}
    for k, x in (over or {}).items():
        L[k] = x.requires_grad_(wanted(k))
    kw = {('Δf' if k == 'df' else k): L[k] for k in use}
    Mss = fused.ab_steadystate(L['A'], L['B'], **kw)
    if loss is not None:
        loss(Mss)
    elif Mss.requires_grad:
        (Mss * dev(P['w']).reshape(Mss.shape)).sum().backward()
    out = {'grad_' + k: x.grad for k, x in L.items()}
    out['Mss'] = Mss.detach()
    return out


# =============================================================================================
# 1. the kernels alone, tight
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('N, nM', [(1, 1), (2, 100), (2, 200)], ids=['rows1', 'rows200', 'rows400'])
def test_kernels_alone_against_the_fp64_solve(tag, N, nM):
    r"""1, 200 and 400 rows: 400 spans two 256-thread blocks, the second ragged, and the boundary between the two batch
    entries (row 200) falls inside the first.  ``Mss`` and the gradients w.r.t. ``A, B, rest, T1, T2, Δf`` against the CPU's
    fp64 solve and autograd on the same numbers."""
    P, want = _kernel_problem(N, nM, tag)
    got = _run(P)
    assert got['Mss'].dtype == DT[tag] and set(got) == set(want)
    for k in want:
        _gate(got[k], want[k], tag, k)
    assert float(got['grad_T1'].abs().max()) > 0 and float(got['grad_df'].abs().max()) > 0


@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('use', [(), ('rest',), ('rest', 'df'), ('rest', 'T1', 'T2')], ids=['norest', 'rest', 'rest-df', 'rest-T'])
def test_absent_operands(tag, use):
    r"""``rest=None`` is ``(I - A)^-1 B``; a rest without relaxation, without precession or without both is what
    ``sims.freeprec`` makes of the same absences.  The absent operands get no gradient; the others the yardstick's."""
    P, _ = _kernel_problem(2, 200, tag)
    want = _yardstick(P, use)
    got = _run(P, use)
    assert set(got) == set(want)
    for k in want:
        _gate(got[k], want[k], tag, f'{use}: {k}')
    if not use:
        A, B = P['A'].double(), P['B'].double()
        direct = torch.linalg.solve(torch.eye(3, dtype=torch.float64) - A, B)
        _gate(got['Mss'], direct, tag, 'Mss vs (I - A)^-1 B')


# =============================================================================================
# 2. operand forms
# =============================================================================================
def _form(full, form):
    r"""``(operand on the device in that form, its fully materialised (N, nM) values on the CPU)`` from ``full`` (N, nM)."""
    N, nM = full.shape
    if form == '0dim':
        x = full[0, 0].clone()
    elif form == '11':
        x = full[:1, :1].clone()
    elif form == 'N1':
        x = full[:, :1].clone()
    elif form == 'NnM':
        x = full.clone()
    else:
        assert form == 'expanded'
        x = full[:1].clone().expand(N, nM)                 # strides (0, 1): a (1, nM) row seen as (N, nM)
    return place(x), x.expand(N, nM).contiguous()


@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('form', ['0dim', '11', 'N1', 'NnM', 'expanded'])
def test_operand_forms(tag, form):
    r"""``T1``, ``T2`` in every broadcast form, ``rest`` as `()` and `(N,)`, ``Δf`` absent and `(N, nM)`: the result is the
    fully materialised call's bit for bit; each gradient has its operand's own shape and is the materialised call's
    gradient summed over the broadcast axes."""
    P, _ = _kernel_problem(2, 200, tag)
    N, nM = 2, 200
    for rest_form in ('0dim', 'N'):
        for with_df in (False, True):
            use = ('rest', 'T1', 'T2') + (('df',) if with_df else ())
            T1, T1m = _form(P['T1'], form)
            T2, T2m = _form(P['T2'], form)
            rest = P['rest'][0].clone() if rest_form == '0dim' else P['rest'].clone()
            mat = _run(dict(P, T1=T1m, T2=T2m, rest=rest.expand(N).contiguous()), use)
            got = _run(P, use, over=dict(T1=T1, T2=T2, rest=dev(rest)))
            what = (form, rest_form, with_df)
            assert torch.equal(got['Mss'], mat['Mss']), what
            assert torch.equal(got['grad_A'], mat['grad_A']) and torch.equal(got['grad_B'], mat['grad_B']), what
            for k, x in (('T1', T1), ('T2', T2), ('rest', rest)):
                g = got['grad_' + k]
                assert g.shape == x.shape and g.dtype == x.dtype, (what, k, g.shape)
                shp = tuple(x.shape) + (1,) * (mat['grad_' + k].ndim - x.ndim) if x.ndim else (1,) * mat['grad_' + k].ndim
                want = mat['grad_' + k].double().cpu().sum_to_size(shp).reshape(x.shape)
                _gate(g, want, tag, f'{what}: grad_{k}')
            if with_df:
                assert torch.equal(got['grad_df'], mat['grad_df']), what


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_two_spatial_dimensions(tag):
    r"""``Nd = (10, 10)``: ``T1`` `(N, 10, 10)`, ``T2`` `(1, 10, 1)`, ``Δf`` `(N, 10, 10)`, ``rest`` `(N,)` -- the bits of the
    flat `(N, 100)` call, gradients in the operands' shapes."""
    P, _ = _kernel_problem(2, 100, tag)
    T2row = P['T2'].reshape(2, 10, 10)[:1, :, :1].clone()
    flat = _run(dict(P, T2=T2row.expand(2, 10, 10).reshape(2, 100).contiguous()))
    Q = dict(P, A=P['A'].reshape(2, 10, 10, 3, 3), B=P['B'].reshape(2, 10, 10, 3), T1=P['T1'].reshape(2, 10, 10),
             T2=T2row, df=P['df'].reshape(2, 10, 10))
    got = _run(Q)
    assert got['Mss'].shape == (2, 10, 10, 3) and torch.equal(got['Mss'].reshape(2, 100, 3), flat['Mss'])
    for k in ('A', 'B', 'T1', 'df'):
        assert got['grad_' + k].shape == Q[k].shape and torch.equal(got['grad_' + k].reshape(flat['grad_' + k].shape),
                                                                    flat['grad_' + k]), k
    assert got['grad_T2'].shape == (1, 10, 1) and got['grad_rest'].shape == (2,)
    _gate(got['grad_T2'], flat['grad_T2'].double().cpu().reshape(2, 10, 10).sum_to_size(1, 10, 1), tag, 'grad_T2')
    _gate(got['grad_rest'], flat['grad_rest'], tag, 'grad_rest')          # (summed over the spins in another order)


# =============================================================================================
# 3. a known answer: the spoiled gradient echo (Ernst)
# =============================================================================================
def test_spoiled_steady_state_is_the_ernst_formula():
    r"""A one-step hard pulse about x of 0.5 G and of 3 G (the two batch entries) without relaxation during the pulse
    (``consts``: ``E1 = E2 = 1``, ``E1_1 = 0``), T2 = 50 us and a rest of 5 ms -- the transverse state is spoiled to
    ``e^-100`` -- and T1 from 50 ms to 1 s over the spins: ``Mz = m cos α``, ``|Mxy| = m sin α`` with
    ``m = (1 - E1r) / (1 - E1r cos α)``, ``α = 2πγ dt |rf|``, to 1e-12 in fp64."""
    N, nM, d = 2, 100, torch.float64
    γ, dt_ = 4257.6, 4e-6
    amp = torch.tensor([0.5, 3.0], dtype=d)
    rf = torch.zeros((N, 2, 1), dtype=d)
    rf[:, 0, 0] = amp
    T1 = torch.linspace(0.05, 1.0, nM, dtype=d).expand(N, nM).contiguous()
    rest = torch.tensor(5e-3, dtype=d)
    one = torch.ones((), dtype=d)
    consts = dict(γ2πdt=dev(2 * π * γ * dt_ * one), E1=dev(one), E2=dev(one), E1_1=dev(0 * one))
    loc = torch.zeros((N, nM, 3), dtype=d)
    with torch.no_grad():
        Mss = fused.steadystate_rfgr(dev(rf), dev(torch.zeros((N, 3, 1), dtype=d)), dev(loc), rest=dev(rest),
                                     T1=dev(T1), T2=dev(torch.tensor(50e-6, dtype=d)), γ_beff=dev(γ * one),
                                     consts=consts).cpu()
    α = (2 * π * γ * dt_ * amp)[:, None]
    E1r = torch.exp(-rest / T1)
    m = (1 - E1r) / (1 - E1r * torch.cos(α))
    assert float((Mss[..., 2] - m * torch.cos(α)).abs().max()) <= 1e-12
    assert float((Mss[..., :2].norm(dim=-1) - m * torch.sin(α)).abs().max()) <= 1e-12
    assert float(Mss[..., 0].abs().max()) <= 1e-12           # about x: the transverse state lies along y


# =============================================================================================
# 4. the fixed point: nothing amplified
# =============================================================================================
REST = (5e-3, 6.5e-3)


def _pulse_kw(P):
    return dict(Δf=dev(P['df']), b1Map=dev(P['b1']), γ_beff=dev(P['γ']), T1=dev(P['T1']), T2=dev(P['T2']), γ=dev(P['γ']),
                dt=dev(P['dt']))


@pytest.mark.parametrize('tag_mode', MODES)
@pytest.mark.parametrize('nT', [48, 50, 7])
def test_steady_state_is_the_fixed_point_of_the_simulators(tag_mode, nT):
    r"""``blochsim_rfgr(sims.freeprec(Mss, rest, ...), rf, gr, ...)`` returns ``Mss`` at the project's simulator gates; with a
    pulse gradient asked for, nT = 48 is the fused route with checkpoints, 50 the split one, 7 the composed one."""
    tag, mode = _mode(tag_mode)
    P = _problem(tag, 'b1map', nT)
    rest = dev(torch.tensor(REST, dtype=DT[tag]))
    rf, gr, loc = dev(P['rf']).requires_grad_(True), dev(P['gr']).requires_grad_(True), dev(P['loc'])
    kw = _pulse_kw(P)
    with mode:
        Mss = fused.steadystate_rfgr(rf, gr, loc, rest=rest, **kw)
        assert Mss.requires_grad and Mss.shape == (2, 100, 3) and Mss.dtype == DT[tag]
        with torch.no_grad():
            before = sims.freeprec(Mss.detach(), rest, T1=kw['T1'], T2=kw['T2'], Δf=kw['Δf'])
            after = fused.blochsim_rfgr(before, rf.detach(), gr.detach(), loc, **kw)
    assert bool(torch.isfinite(Mss).all()) and float(Mss.detach().norm()) > 0
    record(f'steadystate.{tag_mode}.nT{nT}.fixed_point', max_abs(after, Mss) if tag == 'f64' else rel_l2(after, Mss))
    assert_close(after, Mss, tag, 'one more period')


# =============================================================================================
# 5. the fixture from the reference
# =============================================================================================
def _fixture_run(Q, wrap=True):
    rf, gr = dev(Q['rf']).requires_grad_(True), dev(Q['gr']).requires_grad_(True)
    γ, dt, E1 = dev(Q['γ']), dev(Q['dt']), dev(Q['E1'])
    pulse = dict(Δf=dev(Q['df']), b1Map=dev(Q['b1']), γ_beff=γ,
                 consts=dict(γ2πdt=2 * π * γ * dt, E1=E1, E2=dev(Q['E2']), E1_1=E1 - 1))
    rest = dict(rest=dev(Q['rest']), T1=dev(Q['T1']), T2=dev(Q['T2']))
    if wrap:
        Mss = fused.steadystate_rfgr(rf, gr, dev(Q['loc']), **pulse, **rest)
    else:
        Mss = fused.ab_steadystate(*fused.ab_rfgr(rf, gr, dev(Q['loc']), **pulse), Δf=pulse['Δf'], **rest)
    (Mss * dev(Q['w'])).sum().backward()
    return dict(Mss=Mss.detach(), grad_rf=rf.grad, grad_gr=gr.grad)


@pytest.mark.parametrize('tag_mode', MODES)
def test_against_the_reference_fixture(tag_mode):
    r"""fp64: ``Mss`` (the reference iterated to its steady state) and ``grad_rf``, ``grad_gr`` at the project's gate.  fp32:
    the distances to the fp64 fixture go to the ledger and are held to 3 x ``distance_f32_vs_f64.*``, what the reference's
    own all-fp32 route loses on the same numbers (kappa <= 45 here; two fp32 routes round differently under it).
    ``steadystate_rfgr`` is ``ab_steadystate(*ab_rfgr(.))`` bit for bit."""
    tag, mode = _mode(tag_mode)
    G, G64 = golden(f'steadystate_{tag}'), golden('steadystate_f64')
    Q = fixture_inputs(G)
    with mode:
        got = _fixture_run(Q)
        parts = _fixture_run(Q, wrap=False)
    for k in got:
        assert torch.equal(got[k], parts[k]), k
    if tag == 'f64':
        for k in got:
            record(f'steadystate.f64.fixture.{k}', max_abs(got[k], G[k]))
            assert_close(got[k], G[k], 'f64', f'{k} vs the reference fixture')
        return
    wide = oracle_steadystate(Q, torch.float64)
    for k in got:
        bound = 3 * float(G[f'distance_f32_vs_f64.{k}'])
        record(f'steadystate.{tag_mode}.fixture.{k}.vs_oracle64_on_the_same_numbers', rel_l2(got[k], wide[k]))
        record(f'steadystate.{tag_mode}.fixture.{k}.reference_f32_vs_fixture64', rel_l2(G[k], G64[k]))
        d = record(f'steadystate.{tag_mode}.fixture.{k}.vs_fixture64', rel_l2(got[k], G64[k]), bound)
        print(f'{tag_mode} {k}: {d:.3e} from the fp64 fixture, bound {bound:.3e}')
    for k in got:
        d, bound = rel_l2(got[k], G64[k]), 3 * float(G[f'distance_f32_vs_f64.{k}'])
        assert d <= bound, f'{k}: {d:.3e} from the fp64 fixture > 3 x the reference\'s own fp32 distance = {bound:.3e}'


# =============================================================================================
# 6. a rest that precesses differently from the pulse
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_df_rest(tag):
    r"""``Δf_rest`` changes the rest period only: the result is the explicit composition with the two ``Δf`` bit for bit and
    differs from the default's; the gradient w.r.t. a ``Δf`` used in both places is the sum of the two paths'."""
    P = _problem(tag, 'b1map', 48)
    rest = dev(torch.tensor(REST, dtype=DT[tag]))
    rf, gr, loc = dev(P['rf']), dev(P['gr']), dev(P['loc'])
    kw = _pulse_kw(P)
    other = dev((P['df'] * 0.5 + 30).to(DT[tag]))
    w = dev(torch.sin(torch.arange(600, dtype=torch.float64) * 0.37 + 0.3).reshape(2, 100, 3).to(DT[tag]))
    with torch.no_grad():
        plain = fused.steadystate_rfgr(rf, gr, loc, rest=rest, **kw)
        same = fused.steadystate_rfgr(rf, gr, loc, rest=rest, Δf_rest=kw['Δf'], **kw)
        got = fused.steadystate_rfgr(rf, gr, loc, rest=rest, Δf_rest=other, **kw)
        A, B = fused.ab_rfgr(rf, gr, loc, **kw)
        want = fused.ab_steadystate(A, B, rest=rest, T1=kw['T1'], T2=kw['T2'], Δf=other)
    assert torch.equal(plain, same) and torch.equal(got, want) and not torch.equal(got, plain)
    _gate(got, torch_steadystate(A.double().cpu(), B.double().cpu(), rest.double().cpu(), P['T1'].double(), P['T2'].double(),
                                 other.double().cpu()), tag, 'Mss vs the torch solve')

    def grads(both):
        a, b = kw['Δf'].clone().requires_grad_(True), kw['Δf'].clone().requires_grad_(True)
        Mss = fused.steadystate_rfgr(rf, gr, loc, rest=rest, **dict(kw, Δf=a), **({} if both else dict(Δf_rest=b)))
        (Mss * w).sum().backward()
        return a.grad, b.grad
    g_both, none = grads(True)
    g_pulse, g_rest = grads(False)
    assert none is None and float(g_pulse.abs().max()) > 0 and float(g_rest.abs().max()) > 0
    _gate(g_both, g_pulse.double() + g_rest.double(), tag, 'grad_Δf through both paths')


# =============================================================================================
# 7. determinism   8. empty problems   9. capture
# =============================================================================================
@pytest.mark.parametrize('tag_mode', MODES)
def test_two_runs_give_the_same_bits(tag_mode):
    tag, mode = _mode(tag_mode)
    P, _ = _kernel_problem(2, 200, tag)
    Q = fixture_inputs(golden(f'steadystate_{tag}'))
    with mode:
        k1, k2 = _run(P), _run(P)
        f1, f2 = _fixture_run(Q), _fixture_run(Q)
    for a, b in ((k1, k2), (f1, f2)):
        for k in a:
            assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_empty_problem(tag):
    r"""No spin: correctly shaped empties, forward and backward, from the kernel's function and through the pulse."""
    P, _ = _kernel_problem(2, 100, tag)
    E = {k: (v[:, :0] if v.ndim > 1 else v) for k, v in P.items()}
    got = _run(E)
    assert got['Mss'].shape == (2, 0, 3) and got['grad_A'].shape == (2, 0, 3, 3) and got['grad_B'].shape == (2, 0, 3)
    assert got['grad_T1'].shape == got['grad_T2'].shape == got['grad_df'].shape == (2, 0)
    assert got['grad_rest'].shape == (2,) and float(got['grad_rest'].abs().sum()) == 0.0
    Q = _problem(tag, 'b1map', 48, nM=0)
    rf, gr = dev(Q['rf']).requires_grad_(True), dev(Q['gr']).requires_grad_(True)
    Mss = fused.steadystate_rfgr(rf, gr, dev(Q['loc']), rest=dev(torch.tensor(REST, dtype=DT[tag])), **_pulse_kw(Q))
    assert Mss.shape == (2, 0, 3) and Mss.dtype == DT[tag]
    Mss.sum().backward()
    assert rf.grad.shape == Q['rf'].shape and gr.grad.shape == Q['gr'].shape
    assert float(rf.grad.abs().sum()) == 0.0 and float(gr.grad.abs().sum()) == 0.0


def test_hipgraph_capture():
    r"""One design iteration on the steady state (``steadystate_rfgr``, a loss, backward) at 16^3 x 256 captured into a HIP
    graph on one stream, as ``test_ab_rfgr.test_hipgraph_capture`` does, and replayed once: the eager bits."""
    n, nT = 16, 256
    sp = synth.cube_spins(n, device=DEV)
    p = synth.pulse(nT, device=DEV)
    rf = (0.05 * p['rf']).clone().requires_grad_(True)
    gr = p['gr'].clone().requires_grad_(True)
    rest = torch.tensor(5e-3, dtype=torch.float32, device=DEV)
    w = dev(torch.sin(torch.arange(n ** 3 * 3, dtype=torch.float64) * 0.37 + 0.3).float()).reshape(sp['M0'].shape)

    def iteration():
        Mss = fused.steadystate_rfgr(rf, gr, sp['loc'], rest=rest, Δf=sp['Δf'], γ_beff=sp['γ'], T1=sp['T1'], T2=sp['T2'],
                                     γ=sp['γ'], dt=p['dt'])
        return torch.autograd.grad((Mss * w).sum(), (rf, gr)) + (Mss.detach(),)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            a0, b0, m0 = iteration()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a1, b1, m1 = iteration()
    g.replay()
    torch.cuda.synchronize()
    assert float(a0.abs().max()) > 0 and bool(torch.isfinite(m0).all())
    assert torch.equal(a0, a1) and torch.equal(b0, b1) and torch.equal(m0, m1)
