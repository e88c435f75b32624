r"""K2 / K2b: the fused rf,gr -> Mo forward and adjoint (what ``install()`` binds to ``SpinArray.applypulse``), parallel transmit, checkpoints,
BASELINE configs[4] forward + backward, hipGraph capture.

Regrouped by component in round 5 from ``test_hip_parity.py`` / ``test_hip_round{2,3,4}.py`` (no assertion changed; each test keeps its name).
"""
import pytest

from gpu_common import *  # noqa: F401,F403

pytestmark = pytest.mark.gpu


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('variant', ['b1map', 'plain_batch1_pulse', 'norelax', 'ptx4', 'ptx8_batch1_pulse'])
def test_fused_adjoint(tag, variant):
    r"""Gradients w.r.t. Mi, rf, gr through the fused kernels (checkpoints every 16 steps, segment
    recompute, deterministic spin reduction) == the two-kernel path == the oracle."""
    dt_ = DT[tag]
    gen = torch.Generator().manual_seed(23)
    rnd = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64)  # noqa: E731
    N, nM, nT = 2, 100, 48                       # ragged tile (100 = 64 + 36), 3 checkpoint segments
    Np = 1 if variant.endswith('batch1_pulse') else N
    nC = {'ptx4': 4, 'ptx8_batch1_pulse': 8}.get(variant, 0)      # parallel transmit: own kernel
    M0 = rnd(N, nM, 3).to(dt_)
    rf, gr = ((rnd(Np, 2, nT) * 2 - 1) * 3).to(dt_), ((rnd(Np, 3, nT) * 2 - 1)).to(dt_)
    loc, df = ((rnd(N, nM, 3) * 2 - 1) * 6).to(dt_), ((rnd(N, nM) * 2 - 1) * 200).to(dt_)
    b1 = (rnd(N, nM, 2) * 2 - 1).to(dt_) if variant == 'b1map' else None
    if nC:
        rf = ((rnd(Np, 2, nT, nC) * 2 - 1) * 1.5).to(dt_)
        b1 = ((rnd(N, nM, 2, nC) * 2 - 1) * 0.7).to(dt_)
    T1, T2 = (0.5 + rnd(N, nM)).to(dt_), (0.02 + 0.1 * rnd(N, nM)).to(dt_)
    if variant == 'norelax':
        T1 = T2 = None
    γ, dt = torch.tensor(4257.6, dtype=dt_), torch.tensor([4e-6], dtype=dt_)
    w = torch.sin(torch.arange(N * nM * 3, dtype=torch.float64) * 0.61 + 1).reshape(N, nM, 3).to(dt_)

    def run(kind):
        on = (lambda x: x) if kind == 'oracle' else dev
        Mi, r, g = on(M0).clone().requires_grad_(True), on(rf).clone().requires_grad_(True), \
            on(gr).clone().requires_grad_(True)
        kw = dict(T1=None if T1 is None else on(T1), T2=None if T2 is None else on(T2), γ=on(γ), dt=on(dt))
        if kind == 'oracle':
            be = O.rfgr2beff(r, g, loc, Δf=df, b1Map=b1, γ=γ)
            Mo = O.blochsim(Mi, be, **kw)
        elif kind == 'two':
            be = beffective.rfgr2beff(r, g, dev(loc), Δf=dev(df), b1Map=dev(b1), γ=dev(γ))
            Mo = sims.blochsim(Mi, be, **kw)
        else:
            Mo = fused.blochsim_rfgr(Mi, r, g, dev(loc), Δf=dev(df), b1Map=dev(b1), γ_beff=dev(γ), **kw)
        (Mo * on(w)).sum().backward()
        return Mo.detach(), Mi.grad, r.grad, g.grad
    fu, two, ora = run('fused'), run('two'), run('oracle')
    assert max_abs(fu[0], two[0]) == 0.0                       # forward: bit-identical
    names = ('Mo', 'grad_Mi', 'grad_rf', 'grad_gr')
    for a, b, c, nm in zip(fu, two, ora, names):
        assert a.shape == c.shape, nm
        assert_close(a, c, tag, f'fused {nm} vs oracle')
        assert_close(a, b, tag, f'fused {nm} vs two-kernel')
    assert max_abs(fu[1], two[1]) == 0.0                       # same states, same adjoint arithmetic
    again = run('fused')
    for a, b in zip(fu, again):
        assert max_abs(a, b) == 0.0                            # deterministic reduction
    # the lazy handle takes the same route under autograd
    r2, g2 = dev(rf).clone().requires_grad_(True), dev(gr).clone().requires_grad_(True)
    lz = beffective.rfgr2beff(r2, g2, dev(loc), Δf=dev(df), b1Map=dev(b1), γ=dev(γ), lazy=True)
    kw = dict(T1=dev(T1), T2=dev(T2), γ=dev(γ), dt=dev(dt))
    (sims.blochsim(dev(M0), lz, **kw) * dev(w)).sum().backward()
    assert max_abs(r2.grad, fu[2]) == 0.0 and max_abs(g2.grad, fu[3]) == 0.0


def test_ptx_adjoint_wave_takes_a_second_tile():
    r"""More spin tiles (2050) than the pTx adjoint has persistent waves (2048): waves 0 and 1 take a second tile and
    add its sums to the workspace rows of their first (`first == false`, `old[c]` in k_bloch_rfgr_bwd_mc) -- the plain
    kernel and the per-step injection of the trajectory (every = 1).  fp32 precise, 2 coils, one segment, a ragged last
    tile.  Against the two-kernel route with test_fused_adjoint's gates: grad_Mi bit for bit (the trajectory's, whose
    records enter the t-state rounded, to the fp32 gate), the pulse gradients to the fp32 gate; twice the same bits."""
    N, nM, nT, nC = 1, 2048 * 64 + 100, 16, 2
    gen = torch.Generator().manual_seed(31)
    rnd = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64).float()  # noqa: E731
    M0, loc, df = dev(rnd(N, nM, 3)), dev((rnd(N, nM, 3) * 2 - 1) * 6), dev((rnd(N, nM) * 2 - 1) * 200)
    rf, gr = dev((rnd(N, 2, nT, nC) * 2 - 1) * 1.5), dev(rnd(N, 3, nT) * 2 - 1)
    b1 = dev((rnd(N, nM, 2, nC) * 2 - 1) * 0.7)
    kw = dict(T1=dev(0.5 + rnd(N, nM)), T2=dev(0.02 + 0.1 * rnd(N, nM)), γ=dev(torch.tensor(4257.6)),
              dt=dev(torch.tensor([4e-6])))
    w = dev(torch.sin(torch.arange(N * nM * nT * 3, dtype=torch.float64) * 0.61 + 1).float().reshape(N, nM, nT, 3))

    def run(kind, traj):
        Mi, r, g = (x.clone().requires_grad_(True) for x in (M0, rf, gr))
        if kind == 'two':
            be = beffective.rfgr2beff(r, g, loc, Δf=df, b1Map=b1, γ=kw['γ'])
            if traj:                                           # M after every step: one-step runs of K1
                Ms, M = [], Mi
                for t in range(nT):
                    M = sims.blochsim(M, be[:, :, t:t + 1], **kw)
                    Ms.append(M)
                out = torch.stack(Ms, dim=-2)
            else:
                out = sims.blochsim(Mi, be, **kw)
        elif traj:
            out = fused.blochsim_rfgr_traj(Mi, r, g, loc, every=1, Δf=df, b1Map=b1, γ_beff=kw['γ'], **kw)
        else:
            out = fused.blochsim_rfgr(Mi, r, g, loc, Δf=df, b1Map=b1, γ_beff=kw['γ'], **kw)
        (out * (w if traj else w[..., -1, :])).sum().backward()
        return Mi.grad, r.grad, g.grad

    with mrphy_amd.precision('precise'):
        for traj in (False, True):
            fu, two, again = run('fused', traj), run('two', traj), run('fused', traj)
            if traj:
                assert_close(fu[0], two[0], 'f32', 'trajectory grad_Mi vs two-kernel')
            else:
                assert max_abs(fu[0], two[0]) == 0.0           # same states, same adjoint arithmetic
            assert_close(fu[1], two[1], 'f32', f'grad_rf vs two-kernel (traj={traj})')
            assert_close(fu[2], two[2], 'f32', f'grad_gr vs two-kernel (traj={traj})')
            for a, b in zip(fu, again):
                assert max_abs(a, b) == 0.0                    # deterministic reduction over two tiles per row


@pytest.mark.usefixtures('host_constants')
def test_config5_interpT_forward_backward():
    r"""64^3 x 2048 after interpT (configs[4]): fine pulse = the reference's own interpT output
    (golden), forward + backward to rf/gr on the 4096-spin subset."""
    G, I = golden('big_cfg4_f32'), golden('interp_f32')
    assert I['rf'].shape == (1, 2, 2048) and int(I['quirk_nT']) == 255
    pulse = dict(rf=t(I['rf']), gr=t(I['gr']), dt=t(I['dt']))
    idx, sp, _ = cases.big_subset(4, torch.float32, 4096)
    spd = to_dev(sp, DEV)
    rf, gr = dev(pulse['rf']).requires_grad_(True), dev(pulse['gr']).requires_grad_(True)
    beff = beffective.rfgr2beff(rf, gr, spd['loc'], Δf=spd['Δf'], γ=spd['γ'])
    Mo = sims.blochsim_consts(spd['M0'], beff, **gconsts(G))
    Mo.sum().backward()
    print(f'cfg5 rel-L2 vs sims: Mo {rel_l2(Mo, G["Mo_sims"]):.2e}, grad_rf '
          f'{rel_l2(rf.grad, G["grad_rf"]):.2e}, grad_gr {rel_l2(gr.grad, G["grad_gr"]):.2e}; '
          f'reference sims-vs-slowsims Mo {rel_l2(G["Mo_sims"], G["Mo_slow"]):.2e}')
    # the same through the fused kernels (no Beff, no history, no grad_Beff in HBM)
    rff, grf_ = dev(pulse['rf']).requires_grad_(True), dev(pulse['gr']).requires_grad_(True)
    Mof = fused.blochsim_rfgr(spd['M0'], rff, grf_, spd['loc'], Δf=spd['Δf'], γ_beff=spd['γ'],
                              consts=gconsts(G))
    Mof.sum().backward()
    assert max_abs(Mof, Mo) == 0.0
    print(f'cfg5 fused adjoint vs two-kernel: grad_rf {rel_l2(rff.grad, rf.grad):.2e}, grad_gr '
          f'{rel_l2(grf_.grad, gr.grad):.2e}; vs reference: grad_rf {rel_l2(rff.grad, G["grad_rf"]):.2e}, '
          f'grad_gr {rel_l2(grf_.grad, G["grad_gr"]):.2e}')
    assert rel_l2(rff.grad, rf.grad) < 1e-5 and rel_l2(grf_.grad, gr.grad) < 1e-5
    ref_noise = rel_l2(G['Mo_sims'], G['Mo_slow'])
    bo = O.rfgr2beff(pulse['rf'], pulse['gr'], sp['loc'], Δf=sp['Δf'], γ=sp['γ'])
    exact = O.blochsim_f64_arith(sp['M0'], bo, consts=gconsts(G, device='cpu'))
    e_hip, e_sims, e_slow = rel_l2(Mo, exact), rel_l2(G['Mo_sims'], exact), rel_l2(G['Mo_slow'], exact)
    print(f'cfg5 rel-L2 vs exact arithmetic: HIP {e_hip:.2e}, reference sims {e_sims:.2e}, '
          f'slowsims {e_slow:.2e}; beff max abs diff vs oracle {max_abs(beff, bo):.2e}')
    assert rel_l2(Mo, G['Mo_sims']) <= 1e-5 + e_sims
    assert e_hip <= 1e-5
    for k, v in (('HIP', e_hip), ('reference_sims', e_sims), ('reference_slowsims', e_slow)):
        record(f'cfg5.Mo.{k}.vs_exact', v, 1e-5 if k == 'HIP' else None)
    budget = angle_budget(bo, G['const.γ2πdt'])          # per spin: 2^-23 x total rotation angle (tests/util.py)
    elementwise('cfg5.Mo.HIP.vs_exact', Mo, exact, row_bound=budget, bulk=True)
    e_ref_el = elementwise('cfg5.Mo.reference_sims.vs_exact', G['Mo_sims'], exact)
    elementwise('cfg5.Mo.reference_slowsims.vs_exact', G['Mo_slow'], exact)
    elementwise('cfg5.Mo.HIP.vs_reference_sims', Mo, G['Mo_sims'], float(budget.max()) + e_ref_el)
    # gradients: ALL 4096 subset spins, both routes, hard 1e-5 against exact differentiation on the
    # same fp32 field and constants; the reference's golden gradients measured by the same yardstick
    # (round 2 asserted 2e-4 on 256 spins; with the fp32 adjoint HIP was 1.2e-5 / 4.4e-6 / 2.9e-5 from
    # exact on grad_M0 / grad_rf / grad_gr, the reference 3.8e-6 / 2.1e-5 on grad_rf / grad_gr)
    got, ex = _assert_grads_1e5('cfg5_grad', sp, pulse, G,
                                ref=dict(grf=G['grad_rf'], ggr=G['grad_gr'], Mo=G['Mo_sims']))
    assert max_abs(got['two']['grf'], rf.grad) == 0.0 and max_abs(got['two']['ggr'], gr.grad) == 0.0


@pytest.mark.usefixtures('host_constants')
def test_pulse_design_loop_descends():
    r"""examples/pulse_design.py: interpT -> fused forward -> loss -> fused adjoint -> Adam, a few
    iterations at 16^3 x 128: gradients flow to the coarse pulse and the loss goes down."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples',
                        'pulse_design.py')
    spec = importlib.util.spec_from_file_location('pulse_design_example', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    losses = mod.design(n=16, nT=128, iters=12, verbose=False)
    assert all(l == l for l in losses) and losses[-1] < 0.95 * losses[0], losses   # 0.865 measured


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('nT,nC', [(53, 1), (100, 1), (37, 4), (16, 1), (9, 1)])
def test_fused_adjoint_any_pulse_length(tag, nT, nC):
    r"""Pulse lengths that are not a whole number of 16-step checkpoint segments: the fused part +
    composed tail must give the forward of a single pass bit for bit and the oracle's gradients."""
    dt_ = DT[tag]
    g = torch.Generator().manual_seed(1000 + nT)
    rnd = lambda *s: torch.rand(s, generator=g, dtype=torch.float64)  # noqa: E731
    N, nM = 2, 90
    M0 = (rnd(N, nM, 3) * 2 - 1).to(dt_)
    rf = (((rnd(N, 2, nT, nC) if nC > 1 else rnd(N, 2, nT)) * 2 - 1) * 1.5).to(dt_)
    gr, loc = (rnd(N, 3, nT) * 2 - 1).to(dt_), ((rnd(N, nM, 3) * 2 - 1) * 6).to(dt_)
    b1 = ((rnd(N, nM, 2, nC) * 2 - 1) * 0.7).to(dt_) if nC > 1 else None
    df = ((rnd(N, nM) * 2 - 1) * 200).to(dt_)
    T1, T2 = (0.5 + rnd(N, nM)).to(dt_), (0.02 + 0.1 * rnd(N, nM)).to(dt_)
    γ, dt = torch.tensor(4257.6, dtype=dt_), torch.tensor([4e-6], dtype=dt_)
    w = (rnd(N, nM, 3) * 2 - 1).to(dt_)

    def run(kind):
        on = (lambda x: x) if kind == 'oracle' else (lambda x: None if x is None else dev(x))
        Mi, r, q = (on(x).clone().requires_grad_(True) for x in (M0, rf, gr))
        kw = dict(T1=on(T1), T2=on(T2), γ=on(γ), dt=on(dt))
        if kind == 'oracle':
            Mo = O.blochsim(Mi, O.rfgr2beff(r, q, loc, Δf=df, b1Map=b1, γ=γ), **kw)
        else:
            Mo = fused.blochsim_rfgr(Mi, r, q, on(loc), Δf=on(df), b1Map=on(b1), γ_beff=on(γ), **kw)
        (Mo * on(w)).sum().backward()
        return Mo.detach(), Mi.grad, r.grad, q.grad
    fu, ora = run('fused'), run('oracle')
    with torch.no_grad():
        single = fused.blochsim_rfgr(dev(M0), dev(rf), dev(gr), dev(loc), Δf=dev(df), b1Map=None if b1 is None else dev(b1),
                                     γ_beff=dev(γ), T1=dev(T1), T2=dev(T2), γ=dev(γ), dt=dev(dt))
    assert max_abs(fu[0], single) == 0.0
    for a, b, nm in zip(fu, ora, ('Mo', 'grad_Mi', 'grad_rf', 'grad_gr')):
        assert a.shape == b.shape
        assert_close(a, b, tag, f'{nm} (nT={nT}, nC={nC})')


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('nT', [16, 24, 1000, 1024])
def test_checkpoint_buffer_contract_guard_banded(nT):
    r"""include/mrphy_hip.h: K2 writes nCk = ceil(nT / ck_every) checkpoints of (rows, 3) -- not one
    element more.  Called through the C ABI with guard bands around exactly that many slots."""
    from mrphy_amd import _host
    lib = mrphy_amd.require_library()
    sp, p = _small_problem(nT, n=9)
    P = beffective._PulseOnSpins(p['rf'], p['gr'], sp['loc'], sp['Δf'], None, sp['γ'])
    g, E1, E2, E1_1 = sims.relax_constants(sp['T1'], sp['T2'], sp['γ'], p['dt'], 4, DEV)
    code, bg, e1, e2, e1m1 = sims._prep_constants(g, E1, E2, E1_1, P.N, P.Nd, torch.float32, DEV)
    ck = int(lib.mrphy_blochsim_rfgr_ck_every())
    rows, nck = P.N * P.nM, -(-nT // ck)
    guard = 4096
    buf = torch.full((guard + nck * rows * 3 + guard,), float('nan'), device=DEV)
    Mck = buf[guard:guard + nck * rows * 3]
    Mo = torch.empty_like(sp['M0'])
    rc = lib.mrphy_blochsim_rfgr_fwd(code, sp['M0'].data_ptr(), *P.k0_args(), *bg.args, *e1.args, *e2.args,
                                     e1m1.t.data_ptr(), Mo.data_ptr(), Mck.data_ptr(), ck,
                                     P.N, P.nM, nT, P.nC, _host.current_stream(DEV))
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[-guard:]).all(), 'checkpoint overrun'
    assert torch.isfinite(Mck).all(), 'a checkpoint slot was not written'
    assert torch.equal(Mck[:rows * 3].reshape(rows, 3), sp['M0'].reshape(rows, 3))   # slot 0 = Mi
    assert mrphy_amd.fused.BlochSimRfGrHIP is not None


# ---------------------------------------------------------------------------------------------
# beff2ab: the fused adjoint (one backward sweep for the four columns)
# ---------------------------------------------------------------------------------------------
@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('N,nM,nT', [(1, 70, 37), (2, 130, 64), (1, 64, 16)])
def test_beff2ab_fused_adjoint_vs_oracle_autograd(tag, N, nM, nT):
    r"""d(A, B)/d(beff) through ``mrphy_beff2ab_save`` + ``mrphy_beff2ab_bwd`` against autograd over the
    oracle's time loop (= the reference's, ``beffective.py:88-100``), with random weights on every
    entry of A and B; tiles that are not full, batches, pulse lengths off the chunk size."""
    dt_ = DT[tag]
    g = torch.Generator().manual_seed(1000 * N + nM + nT)
    beff = ((torch.rand((N, nM, nT, 3), generator=g, dtype=torch.float64) * 2 - 1) * 3).to(dt_)
    beff[:, 3, 5] = 0                                       # a zero-field step
    E1 = (0.9 + 0.1 * torch.rand((N, nM), generator=g, dtype=torch.float64)).to(dt_)
    E2 = (0.8 + 0.2 * torch.rand((N, nM), generator=g, dtype=torch.float64)).to(dt_)
    γ, dt = torch.tensor(4257.6, dtype=dt_), torch.tensor(4e-6, dtype=dt_)
    wA = torch.rand((N, nM, 3, 3), generator=g, dtype=torch.float64).to(dt_) - 0.5
    wB = torch.rand((N, nM, 3), generator=g, dtype=torch.float64).to(dt_) - 0.5
    b_o = _leaf(beff)
    A_o, B_o = O.beff2ab(b_o, E1=E1, E2=E2, γ=γ, dt=dt)
    ((A_o * wA).sum() + (B_o * wB).sum()).backward()
    b_h = _leaf(beff, DEV)
    A_h, B_h = beffective.beff2ab(b_h, E1=dev(E1), E2=dev(E2), γ=dev(γ), dt=dev(dt))
    assert A_h.grad_fn is not None
    with torch.no_grad():                                   # same forward numbers without history
        A_p, B_p = beffective.beff2ab(b_h, E1=dev(E1), E2=dev(E2), γ=dev(γ), dt=dev(dt))
    assert torch.equal(A_p, A_h.detach()) and torch.equal(B_p, B_h.detach())
    ((A_h * dev(wA)).sum() + (B_h * dev(wB)).sum()).backward()
    assert_close(A_h, A_o, tag, 'A')
    assert_close(B_h, B_o, tag, 'B')
    nz = (beff != 0).any(dim=-1)
    if tag == 'f64':
        assert_close(b_h.grad.cpu()[nz], b_o.grad[nz], tag, 'd(A,B)/dbeff')
    else:       # the fp32 oracle's own gradient noise is of the same order: compare with fp64 truth
        b_d = _leaf(beff.double())
        A_d, B_d = O.beff2ab(b_d, E1=E1.double(), E2=E2.double(), γ=γ.double(), dt=dt.double())
        ((A_d * wA.double()).sum() + (B_d * wB.double()).sum()).backward()
        e_hip, e_ref = rel_l2(b_h.grad.cpu()[nz], b_d.grad[nz]), rel_l2(b_o.grad[nz], b_d.grad[nz])
        assert e_hip <= max(1e-5, 1.5 * e_ref), (e_hip, e_ref)
    # only one of the two outputs used: the other's gradient is a zero / absent tensor
    b2 = _leaf(beff, DEV)
    beffective.beff2ab(b2, E1=dev(E1), E2=dev(E2), γ=dev(γ), dt=dev(dt))[1].sum().backward()
    b3 = _leaf(beff)
    O.beff2ab(b3, E1=E1, E2=E2, γ=γ, dt=dt)[1].sum().backward()
    if tag == 'f64':
        assert_close(b2.grad.cpu()[nz], b3.grad[nz], tag, 'd(B)/dbeff')


    # (round 4: slowsims.freeprec and beff2ab supply their constants' gradients too: test_hip_round4.py)


def test_config5_all_spins_gradients_vs_c_restatement():
    r"""BASELINE configs[4] at its real size -- all 262 144 spins x 2048 steps, the reference's own
    interpT output as the fine pulse -- forward + backward through both routes (rfgr2beff + blochsim
    with history + adjoints; fused K2 + K2b), in the product's DEFAULT constants mode, against
    ``oracle/bloch_c.c``: fp64 integration and differentiation of the same function on the same fp32
    field with the very constants the run used.  Bound: 1e-5 relative L2 on ``Mo, grad_M0, grad_rf,
    grad_gr`` (the reference tests gradient equality at atol 1e-4 in fp32, tests/test_sims.py:15,104-105)."""
    import bloch_c as C
    from mrphy_amd import fused
    I = golden('interp_f32')
    n, nT = 64, 2048
    pulse = dict(rf=t(I['rf']), gr=t(I['gr']), dt=t(I['dt']))
    spd = synth.cube_spins(n, dtype=torch.float32, device=DEV, seed_M0=2004)
    sp = {k: v.cpu() for k, v in spd.items()}
    with mrphy_amd.constants_on(None):            # default mode: exp in fp64, rounded once
        g, E1, E2, E1_1 = sims.relax_constants(spd['T1'], spd['T2'], spd['γ'], dev(pulse['dt']), 4, DEV)
    consts = dict(γ2πdt=g, E1=E1, E1_1=E1_1, E2=E2)
    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
    cc = C.constants_from(g, E1, E2, E1_1, N=1, nM=n ** 3)
    Mo_e, gM0_e, grf_e, ggr_e = C.blochsim_rfgr_grad(sp['M0'], pulse['rf'], pulse['gr'], sp['loc'],
                                                     Δf=sp['Δf'], γ_beff=sp['γ'], consts=cc, field_f32=True)
    ex = dict(Mo=Mo_e, gM0=gM0_e, grf=grf_e, ggr=ggr_e)
    assert mrphy_amd.precision.get() == 'precise'
    for route in ('two', 'fused'):
        rf, gr = dev(pulse['rf']).requires_grad_(True), dev(pulse['gr']).requires_grad_(True)
        M0 = spd['M0'].clone().requires_grad_(True)
        if route == 'two':
            Mo = sims.blochsim_consts(M0, beffective.rfgr2beff(rf, gr, spd['loc'], Δf=spd['Δf'], γ=spd['γ']),
                                      **consts)
        else:
            Mo = fused.blochsim_rfgr(M0, rf, gr, spd['loc'], Δf=spd['Δf'], γ_beff=spd['γ'], consts=consts)
        Mo.sum().backward()
        got = dict(Mo=Mo, gM0=M0.grad, grf=rf.grad, ggr=gr.grad)
        for k in ('Mo', 'gM0', 'grf', 'ggr'):
            e = record(f'cfg5_all_spins.{route}.{k}.vs_exact', rel_l2(got[k], ex[k]), 1e-5)
            assert e <= 1e-5, (route, k, e)
        del Mo, got
        torch.cuda.empty_cache()


def test_hipgraph_capture_of_a_design_iteration():
    r"""A whole multi-scale design iteration -- interpT, fused forward with checkpoints, loss, fused
    adjoint, interpT adjoint -- captured into a HIP graph (``torch.cuda.CUDAGraph``) and replayed:
    the launches go to torch's current stream through the C ABI, allocate through torch and never
    synchronise, so stream capture sees all of them.  Replayed gradients are bit-identical to eager
    ones, also after the static inputs are updated in place (what an optimiser does)."""
    from mrphy_amd import fused, interp
    n, nT = 16, 256
    sp = synth.cube_spins(n, device=DEV)
    p = synth.pulse(nT // 2, device=DEV, dt=8e-6)
    dt_fine = torch.tensor([4e-6], device=DEV)
    rf = (0.05 * p['rf']).clone().requires_grad_(True)
    gr = p['gr'].clone().requires_grad_(True)

    def iteration():
        rf_f, gr_f, dt_f = interp.interpT(rf, gr, p['dt'], dt_fine)
        Mo = fused.blochsim_rfgr(sp['M0'], rf_f, gr_f, sp['loc'], Δf=sp['Δf'], γ_beff=sp['γ'],
                                 T1=sp['T1'], T2=sp['T2'], γ=sp['γ'], dt=dt_f)
        return torch.autograd.grad((Mo ** 2).sum(), (rf, gr))

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            a0, b0 = iteration()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a1, b1 = iteration()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(a0, a1) and torch.equal(b0, b1)
    with torch.no_grad():
        rf.mul_(1.25)
        gr.add_(0.01)
    g.replay()
    torch.cuda.synchronize()
    a2, b2 = iteration()
    assert torch.equal(a1, a2) and torch.equal(b1, b2) and not torch.equal(a0, a2)


@pytest.mark.parametrize('nC', [1, 2])
def test_applypulse_bound_method_is_the_fused_kernel(nC):
    r"""``mobjs.SpinArray.applypulse`` as ``install()`` binds it (``mrphy_amd._spinarray_applypulse``), on
    stand-ins for a device-resident ``SpinArray`` and a CPU ``Pulse`` (the reference's default: pulses are built
    on the CPU and moved by ``pulse2beff``, ``mobjs.py:651``): spatial ``loc / Δf / b1Map`` gathered through the
    mask as at ``mobjs.py:425-433``, ``doRelax`` off and on, ``doEmbed``, ``doUpdate`` -- each result BIT-IDENTICAL
    to ``rfgr2beff`` + ``sims.blochsim`` on the same arguments (what the reference's method composes,
    ``mobjs.py:435-446``), and the gradient to the pulse equal to the composed route's."""
    gen = torch.Generator().manual_seed(77 + nC)
    rnd = lambda *s: torch.rand(s, generator=gen)  # noqa: E731
    Nd, nT = (6, 5, 7), 48
    mask = (rnd(1, *Nd) > 0.3).to(DEV)
    nM = int(mask.sum())
    M_ = dev(rnd(1, nM, 3) * 2 - 1)
    T1_, T2_ = dev(0.5 + rnd(1, nM)), dev(0.02 + 0.1 * rnd(1, nM))
    γ_ = dev(torch.full((1, nM), 4257.6))
    arr = SpinArrayStandIn(mask, M_, T1_, T2_, γ_)
    rf = ((rnd(1, 2, nT, nC) if nC > 1 else rnd(1, 2, nT)) * 2 - 1) * 0.8
    pulse = PulseStandIn(rf, rnd(1, 3, nT) * 2 - 1, dt=torch.tensor(4e-6))            # on the CPU
    loc = dev((rnd(1, *Nd, 3) * 2 - 1) * 8)                  # spatial layout: gathered through the mask
    df = dev((rnd(1, *Nd) * 2 - 1) * 200)
    b1 = dev(rnd(1, *Nd, 2, nC) * 2 - 1) if nC > 1 else dev(rnd(1, *Nd, 2) * 2 - 1)
    loc_, df_, b1_ = (arr.extract(x) for x in (loc, df, b1))

    def composed(relax, rfd=None, grd=None):
        rfd = dev(pulse.rf) if rfd is None else rfd
        grd = dev(pulse.gr) if grd is None else grd
        beff = beffective.rfgr2beff(rfd, grd, loc_, Δf=df_, b1Map=b1_, γ=γ_)
        kw = dict(T1=T1_, T2=T2_) if relax else dict(T1=None, T2=None)
        return sims.blochsim(M_, beff, γ=γ_, dt=pulse.dt, **kw)
    with torch.no_grad():
        for relax in (True, False):
            got = mrphy_amd._spinarray_applypulse(arr, pulse, loc=loc, Δf=df, b1Map=b1, doRelax=relax)
            assert got.shape == (1, nM, 3) and torch.equal(got, composed(relax))
        got = mrphy_amd._spinarray_applypulse(arr, pulse, loc_=loc_, Δf_=df_, b1Map_=b1_, doEmbed=True, doUpdate=True)
        want = composed(True)
        assert arr.M_ is not M_ and torch.equal(arr.M_, want)            # doUpdate
        assert got.shape == (1, *Nd, 3) and torch.equal(arr.extract(got), want)   # doEmbed
        arr.M_ = M_
    with pytest.raises(AssertionError):
        mrphy_amd._spinarray_applypulse(arr, pulse, loc=loc, loc_=loc_)
    # gradient to the pulse: fused adjoint (nT % 16 == 0) vs the composed route
    pg = PulseStandIn(dev(pulse.rf).requires_grad_(True), dev(pulse.gr).requires_grad_(True), dt=dev(pulse.dt),
                      device=DEV)
    pg.rf, pg.gr = pg.rf.detach().requires_grad_(True), pg.gr.detach().requires_grad_(True)
    mrphy_amd._spinarray_applypulse(arr, pg, loc_=loc_, Δf_=df_, b1Map_=b1_).sum().backward()
    r2, g2 = dev(pulse.rf).requires_grad_(True), dev(pulse.gr).requires_grad_(True)
    composed(True, r2, g2).sum().backward()
    assert rel_l2(pg.rf.grad, r2.grad) < 2e-6 and rel_l2(pg.gr.grad, g2.grad) < 2e-6


def test_fp64_fused_with_many_coils_takes_the_composed_route():
    r"""fp64 with more than 8 transmit coils: no fused register build exists (it would spill); the host composes
    rfgr2beff + blochsim, the C ABI falls back to its generic build -- the same bits either way."""
    from mrphy_amd import fused, _lib, _host
    f64 = torch.float64
    nC, nT, n = 12, 32, 6
    sp, p, kw = _problem(n, nT, dtype=f64)
    g = torch.Generator(device='cpu').manual_seed(5)
    rf = torch.randn((1, 2, nT, nC), generator=g, dtype=f64).to(DEV) * 0.05
    b1 = torch.randn((1, n ** 3, 2, nC), generator=g, dtype=f64).to(DEV)
    with torch.no_grad():
        beff = beffective.rfgr2beff(rf, p['gr'], sp['loc'], Δf=sp['Δf'], b1Map=b1, γ=sp['γ'])
        want = sims.blochsim(sp['M0'], beff, **kw)
        got = fused.blochsim_rfgr(sp['M0'], rf, p['gr'], sp['loc'], Δf=sp['Δf'], b1Map=b1, γ_beff=sp['γ'], **kw)
        assert torch.equal(got, want)
        # ... and the entry point itself (generic build behind the same C ABI)
        lib = _lib.require_library()
        ps = beffective._PulseOnSpins(rf, p['gr'], sp['loc'], sp['Δf'], b1, sp['γ'])
        γ2πdt, E1, E2, E1_1 = sims.relax_constants(sp['T1'], sp['T2'], sp['γ'], p['dt'], 4, DEV)
        code, gg, e1, e2, e1m1 = sims._prep_constants(γ2πdt, E1, E2, E1_1, ps.N, ps.Nd, f64, DEV)
        Mo = torch.empty_like(want)
        rc = lib.mrphy_blochsim_rfgr_fwd(code, sp['M0'].contiguous().data_ptr(), *ps.k0_args(), *gg.args, *e1.args,
                                         *e2.args, e1m1.t.data_ptr(), Mo.data_ptr(), None, 0, ps.N, ps.nM, ps.nT,
                                         ps.nC, _host.current_stream(DEV))
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(Mo, want)
