r"""K1 / K1h / K3: ``sims.blochsim`` forward and explicit adjoint over a materialised ``Beff``, the 1-step form and its
helpers (a5, a7, a8): known answers, golden gradients, the broadcast zoo, ragged / empty / unaligned inputs, the BASELINE config subsets, whole configs and
the headline workload against exact arithmetic (relative L2 AND elementwise), fuzzing.

Regrouped by component in round 5 from ``test_hip_parity.py`` / ``test_hip_round{2,3,4}.py`` (no assertion changed; each test keeps its name).
"""
import pytest

from gpu_common import *  # noqa: F401,F403

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore_hist_policy():
    r"""Several tests (and every case of the gradient fuzzers) change how the internal history is cut into parts
    (``mrphy_amd._hist.set_policy``): whatever a test leaves behind, the next one starts from the default."""
    from mrphy_amd import _hist
    old = dict(_hist.policy)
    yield
    _hist.policy.clear()
    _hist.policy.update(old)


@pytest.mark.usefixtures('host_constants')
def test_native_library_is_loaded():
    lib = mrphy_amd.require_library()
    assert lib.mrphy_arch() == b'gfx950'
    assert 'gfx950' in torch.cuda.get_device_properties(0).gcnArchName


# ---------------------------------------------------------------------------------------------
@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_ref3_known_answers(tag):
    r"""The reference's 3-spin case (tests/test_slowsims.py:33-84) end to end on the device."""
    G, c = golden(f'ref3_{tag}'), to_dev(cases.ref_case(3, DT[tag]), DEV)
    beff = beffective.rfgr2beff(c['rf'], c['gr'], c['loc'], Δf=c['Δf'], b1Map=c['b1Map'], γ=c['γ'])
    beff_nodim = beffective.rfgr2beff(c['rf'][..., 0], c['gr'], c['loc'], Δf=c['Δf'],
                                      b1Map=c['b1Map'][..., 0], γ=c['γ'])
    assert max_abs(beff, beff_nodim) == 0.0                    # test_sims.py:68-69,101-102
    assert_close(beff, G['beff'], tag, 'beff')
    kw = dict(γ=c['γ'], dt=c['dt'])
    Mo = sims.blochsim_consts(c['M0'], beff, **gconsts(G))          # the reference run's constants
    Mo_nr = sims.blochsim_consts(c['M0'], beff, **gconsts(G, relax=False))
    assert_close(Mo, G['Mo_sims'], tag, 'Mo')
    assert_close(Mo_nr, G['Mo_sims_norelax'], tag, 'Mo norelax')
    assert_close(Mo, G['Mo_slow'], tag, 'Mo vs slowsims')
    # the public signatures (constants formed by this box's torch) against this box's oracle
    cc = cases.ref_case(3, DT[tag])
    ob = O.rfgr2beff(cc['rf'], cc['gr'], cc['loc'], Δf=cc['Δf'], b1Map=cc['b1Map'], γ=cc['γ'])
    for rk in (dict(T1=c['T1'], T2=c['T2']), {}):
        ork = {k: v.cpu() for k, v in rk.items()}
        want = O.blochsim(cc['M0'], ob, **ork, γ=cc['γ'], dt=cc['dt'])
        assert_close(sims.blochsim(c['M0'], beff, **rk, **kw), want, tag, 'sims.blochsim API')
        assert_close(slowsims.blochsim(c['M0'], beff, **rk, **kw), want, tag, 'slowsims.blochsim API')
    # fp32: the reference's own fp32 run is this far from the fp64 known answer
    tol = 1e-9 if tag == 'f64' else 2 * max(max_abs(G['Mo_sims'], MO0_RELAX), 1e-5)
    assert max_abs(Mo, MO0_RELAX) < tol and max_abs(Mo_nr, MO0_NORELAX) < tol
    # 512 x blochsim_1step (test_slowsims.py:65-69)
    k1 = {k: v.reshape(v.shape[:2]) for k, v in gconsts(G).items()}
    M, tmp = c['M0'].clone(), c['M0'].clone()
    for i in range(beff.shape[-2]):
        M, tmp = slowsims.blochsim_1step(M, tmp, beff[..., i, :], k1['E1'], k1['E1_1'], k1['E2'],
                                         k1['γ2πdt'])
    assert_close(M, G['Mo_1step'], tag, '512 x 1step')
    # fused rf,gr -> Mo gives the same as the two kernels
    Mf = fused.blochsim_rfgr(c['M0'], c['rf'], c['gr'], c['loc'], Δf=c['Δf'], b1Map=c['b1Map'],
                             γ_beff=c['γ'], consts=gconsts(G))
    assert max_abs(Mf, Mo) == 0.0
    # gradient chain to rf and gr (test_slowsims.py:86-96)
    rf, gr = c['rf'].clone().requires_grad_(True), c['gr'].clone().requires_grad_(True)
    b2 = beffective.rfgr2beff(rf, gr, c['loc'], Δf=c['Δf'], b1Map=c['b1Map'], γ=c['γ'])
    sims.blochsim_consts(c['M0'], b2, **gconsts(G)).sum().backward()
    assert_close(rf.grad, G['grad_rf'], tag, 'grad_rf')
    assert_close(gr.grad, G['grad_gr'], tag, 'grad_gr')


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_ref512_gradients(tag):
    r"""The reference's differential test (tests/test_sims.py:36-143): Mo, grad_M0, grad_beff."""
    G, c = golden(f'ref512_{tag}'), to_dev(cases.ref_case(512, DT[tag], seed=1234), DEV)
    beff = beffective.rfgr2beff(c['rf'], c['gr'], c['loc'], Δf=c['Δf'], b1Map=c['b1Map'], γ=c['γ'])
    rows = G['rows'].tolist()
    assert_close(beff[:, rows], G['beff_rows'], tag, 'beff rows')
    for relax in (True, False):
        sfx = '' if relax else '_norelax'
        M0 = c['M0'].clone().requires_grad_(True)
        B = beff.clone().requires_grad_(True)
        B_before = B.detach().clone()
        Mo = sims.blochsim_consts(M0, B, **gconsts(G, relax=relax))
        Mo.sum().backward(retain_graph=True)
        assert max_abs(B, B_before) == 0.0 and max_abs(M0, c['M0']) == 0.0   # inputs untouched
        for ref in ('sims', 'slow'):
            assert_close(Mo, G[f'Mo_{ref}{sfx}'], tag, f'Mo vs {ref}{sfx}')
            assert_close(M0.grad, G[f'gM0_{ref}{sfx}'], tag, f'gM0 vs {ref}{sfx}')
            assert_close(B.grad[:, rows], G[f'gB_rows_{ref}{sfx}'], tag, f'gB vs {ref}{sfx}')
            assert_close(B.grad.sum(1), G[f'gB_sum_{ref}{sfx}'], tag, f'gB sum vs {ref}{sfx}')
            if tag == 'f32':
                # ... and ELEMENTWISE, the reference's own fp32 gate on this very case: atol = 1e-4
                # (/root/reference tests/test_sims.py:15,101-105) -- on top of the relative L2 above
                for nm, got, want in (('Mo', Mo, G[f'Mo_{ref}{sfx}']), ('gM0', M0.grad, G[f'gM0_{ref}{sfx}']),
                                      ('gB_rows', B.grad[:, rows], G[f'gB_rows_{ref}{sfx}'])):
                    elementwise(f'ref512_f32.{nm}.vs_reference_{ref}{sfx}', got, want, ATOL32_REFERENCE)
        # a second backward through the same graph gives the same answer (the reference's
        # would not: it overwrites its saved tensors, sims.py:239-264)
        g1 = (M0.grad.clone(), B.grad.clone())
        M0.grad = B.grad = None
        Mo.sum().backward()
        assert max_abs(M0.grad, g1[0]) == 0.0 and max_abs(B.grad, g1[1]) == 0.0
        # only one of the two gradients requested
        M1 = c['M0'].clone().requires_grad_(True)
        sims.blochsim_consts(M1, beff, **gconsts(G, relax=relax)).sum().backward()
        assert max_abs(M1.grad, g1[0]) == 0.0


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_broadcast_zoo(tag):
    r"""T1/T2/γ as 0-dim, (1,1), (N,nM), stride-0 expanded; dt (N,)."""
    G = golden(f'bcast_{tag}')
    M0, Beff, variants = cases.bcast_variants(DT[tag])
    for name, kw in variants.items():
        kd = {k: dev(v) for k, v in kw.items()}
        if name == 'expanded':       # stride-0 views on the device, as mobjs keeps T1_/T2_/γ_
            N_, nM_ = M0.shape[:2]
            kd.update(T1=dev(kw['T1'][:, :1].contiguous()).expand(N_, nM_),
                      T2=dev(kw['T2'][:1, :1].contiguous()).expand(N_, nM_),
                      γ=dev(kw['γ'][:1, :1].contiguous()).expand(N_, nM_))
            assert kd['γ'].stride() == (0, 0) and kd['T1'].stride() == (1, 0)
        w = torch.sin(torch.arange(M0.numel(), dtype=torch.float64) * 0.61 + 1).reshape(M0.shape)
        wd = w.to(device=DEV, dtype=DT[tag])
        # (a) golden: the reference's outputs, with the constants of the reference run
        Mi, B = dev(M0).requires_grad_(True), dev(Beff).requires_grad_(True)
        Mo = sims.blochsim_consts(Mi, B, **gconsts(G, f'{name}.'))
        (Mo * wd).sum().backward()
        assert_close(Mo, G[f'{name}.Mo'], tag, f'{name}.Mo')
        assert_close(B.grad, G[f'{name}.gB'], tag, f'{name}.gB')
        if f'{name}.gMi' in G:      # where the reference's grad_Mi is valid (sims.py:267)
            assert_close(Mi.grad, G[f'{name}.gMi'], tag, f'{name}.gMi golden')
        # (b) the public signature with every broadcast form, against this box's oracle (whose
        # explicit adjoint is pinned to the reference) -- incl. per-spin γ and per-batch dt
        Mi1, B1 = dev(M0).requires_grad_(True), dev(Beff).requires_grad_(True)
        Mo1 = sims.blochsim(Mi1, B1, **kd)
        (Mo1 * wd).sum().backward()
        Mi2, B2 = M0.clone().requires_grad_(True), Beff.clone().requires_grad_(True)
        Mo2 = O.blochsim(Mi2, B2, **kw)
        (Mo2 * w.to(DT[tag])).sum().backward()
        assert_close(Mo1, Mo2, tag, f'{name}.Mo API')
        assert_close(B1.grad, B2.grad, tag, f'{name}.gB API')
        assert_close(Mi1.grad, Mi2.grad, tag, f'{name}.gMi API')


@pytest.mark.usefixtures('host_constants')
def test_fp32_data_with_fp64_default_constants():
    r"""Direct call with the fp64 defaults γH, dt0 and fp32 data: the reference promotes the
    constant products to fp64; dtype code MRPHY_F32_C64 reproduces that."""
    M0, Beff, variants = cases.bcast_variants(torch.float32)
    kw = variants['per_spin']
    ref = O.blochsim(M0, Beff, T1=kw['T1'], T2=kw['T2'])          # γ=γH, dt=dt0: fp64 0-dim
    out = sims.blochsim(dev(M0), dev(Beff), T1=dev(kw['T1']), T2=dev(kw['T2']))
    assert out.dtype == torch.float32
    assert rel_l2(out, ref) < 1e-6
    # and it is NOT what all-fp32 constants give bit for bit (the promotion is really there)
    ref64 = O.blochsim_f64_arith(M0, Beff, T1=kw['T1'], T2=kw['T2'])
    assert rel_l2(out, ref64) < 1e-6


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_onestep_and_helpers(tag):
    G, U = golden(f'onestep_{tag}'), golden(f'uphi_{tag}')
    c = to_dev(cases.onestep_case(DT[tag]), DEV)
    Min = c['M'].clone()
    Mn, Mold = slowsims.blochsim_1step(Min, Min.clone(), c['b'], c['E1'], c['E1_1'], c['E2'], c['γ2πdt'])
    assert Mold is Min and max_abs(Min, c['M']) == 0.0
    assert_close(Mn, G['M_new'], tag, '1step')
    Mz, _ = slowsims.blochsim_1step(Min, Min, torch.zeros_like(c['b']), c['E1'], c['E1_1'],
                                    c['E2'], c['γ2πdt'])
    assert_close(Mz, G['M_new_zero_b'], tag, '1step zero field')
    u, p = beffective.beff2uϕ(c['b'], c['γ2πdt'])
    assert_close(u, U['U'], tag, 'U')
    assert_close(p, U['Phi'], tag, 'Phi')
    V34 = torch.stack([c['M'], c['M'].flip(-1), c['M'] * 2, -c['M']], dim=-1)
    assert_close(utils.uϕrot(u, p, c['M']), U['rot3'], tag, 'uϕrot (…,3)')
    assert_close(utils.uϕrot(u, p, V34), U['rot34'], tag, 'uϕrot (…,3,nV)')


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_mobjs_call_shapes(tag):
    r"""Replay exactly what mrphy.mobjs.SpinCube.applypulse hands to rfgr2beff and blochsim
    (shapes, STRIDES and dtypes recorded from the reference's object layer on the
    tests/test_mobjs.py:98-131 case) and compare with what the reference returned."""
    G = golden(f'mobjs_{tag}')
    meta = json.loads(str(G['meta']))
    dt_ = DT[tag]

    def rebuild(name, info, src):
        x = t(src, dt_, DEV)
        shape, stride = tuple(info['shape']), tuple(info['stride'])
        if tuple(x.shape) != shape:
            x = x.expand(shape)
        if 0 in stride and x.stride() != stride:               # stride-0 compact attributes
            keep = tuple(slice(0, 1) if s == 0 and n > 1 else slice(None) for s, n in zip(stride, shape))
            x = x[keep].expand(shape)
        assert x.shape == shape
        return x
    mb, ms = meta['rfgr2beff'], meta['blochsim']
    loc = rebuild('loc', mb['loc'], G['loc_'])
    beff = beffective.rfgr2beff(t(G['rf'], dt_, DEV), t(G['gr'], dt_, DEV), loc,
                                Δf=rebuild('Δf', mb['Δf'], G['Δf_']), b1Map=None,
                                γ=rebuild('γ', mb['γ'], G['γ_']))
    assert tuple(beff.shape) == tuple(ms['Beff']['shape'])
    kw = dict(γ=rebuild('γ', ms['γ'], G['γ_']), dt=t(G['dt'], dt_, DEV))
    kr = dict(T1=rebuild('T1', ms['T1'], G['T1_']), T2=rebuild('T2', ms['T2'], G['T2_']))
    assert meta['blochsim_norelax']['T1'] is None
    M0 = t(G['M0_'], dt_, DEV)
    M_ = sims.blochsim_consts(M0, beff, **gconsts(G))
    # the exact call mobjs makes (its shapes and strides), constants formed on this box
    M_api = sims.blochsim(M0, beff, **kr, **kw)
    # constants formed on this box vs the fixture's: exp() may differ by an ulp of E (2^-24 for E in
    # [1/2, 1)) on some spins, applied nT times -- hence the bound nT * 2^-24 (3.1e-5 at nT = 512)
    nT_ = beff.shape[-2]
    d_api = record(f'mobjs_replay.{tag}.api_constants_vs_fixture_constants', rel_l2(M_api, M_),
                   1e-9 if tag == 'f64' else nT_ * 2.0 ** -24)
    assert d_api <= (1e-9 if tag == 'f64' else nT_ * 2.0 ** -24)
    mask = t(G['mask']).to(DEV)
    M = torch.full((1, 3, 3, 3, 3), float('nan'), dtype=dt_, device=DEV)
    M[mask.expand(1, 3, 3, 3)] = M_.reshape(-1, 3)              # SpinArray.embed (mobjs.py:512-530)
    ref = t(G['M_embed'])
    assert torch.equal(torch.isnan(M.cpu()), torch.isnan(ref))
    assert_close(torch.nan_to_num(M), torch.nan_to_num(ref), tag, 'applypulse(doEmbed)')
    # the known answer is an fp64 result; in fp32 the reference's own output (the fixture's M_embed)
    # is e_ref away from it: ours may be 1e-5 (north star, |M| <= 1) further, not more
    e_ref = max(max_abs(ref[0:1, 1, :, 1, :], MO0_RELAX), max_abs(ref[0:1, :, 1, 1, :], MO0_RELAX))
    tol = 1e-9 if tag == 'f64' else e_ref + 1e-5
    e_ours = max(max_abs(M[0:1, 1, :, 1, :], MO0_RELAX), max_abs(M[0:1, :, 1, 1, :], MO0_RELAX))
    record(f'mobjs_replay.{tag}.known_answer_max_abs', e_ours, tol,
           note=f'reference fp output of the same call: {e_ref:.3e}')
    assert e_ours <= tol                                         # test_mobjs.py:125-126
    Mnr = sims.blochsim_consts(M0, beff, **gconsts(G, relax=False))
    assert_close(Mnr, G['M_compact_norelax'], tag, 'applypulse(doRelax=False)')
    assert_close(sims.blochsim(M0, beff, T1=None, T2=None, **kw), Mnr, tag, 'no-relax API')
    # the lazy handle: same call sequence, fused kernel, no Beff tensor
    lz = beffective.rfgr2beff(t(G['rf'], dt_, DEV), t(G['gr'], dt_, DEV), loc,
                              Δf=rebuild('Δf', mb['Δf'], G['Δf_']), γ=rebuild('γ', mb['γ'], G['γ_']),
                              lazy=True)
    assert isinstance(lz, beffective.LazyBeff) and tuple(lz.shape) == tuple(beff.shape)
    assert lz.to(DEV) is lz and lz.ndim == 4
    Ml = sims.blochsim(M0, lz, **kr, **kw)
    assert max_abs(Ml, M_api) == 0.0
    assert max_abs(lz[..., 0, :], beff[..., 0, :]) == 0.0       # any other use materialises it


# ---------------------------------------------------------------------------------------------
# Edge cases: empty, ragged, unaligned, non-contiguous, single step, large angles
# ---------------------------------------------------------------------------------------------
@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('N,nM,nT', [(1, 1, 1), (1, 63, 17), (2, 65, 16), (3, 130, 35),
                                     (1, 200, 64), (2, 64, 13), (1, 129, 4)])
def test_ragged_shapes(tag, N, nM, nT):
    r"""nM not a multiple of 64 (partial waves, tiles straddling batch entries), nT not a
    multiple of the 16-step chunk nor of 4 (unaligned rows: scalar path), N > 1."""
    dt_ = DT[tag]
    gen = torch.Generator().manual_seed(N * 1000 + nM * 10 + nT)
    rnd = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64)  # noqa: E731
    M0 = rnd(N, nM, 3).to(dt_)
    rf, gr = (rnd(N, 2, nT) * 2 - 1).to(dt_), (rnd(N, 3, nT) * 2 - 1).to(dt_)
    loc, df = ((rnd(N, nM, 3) * 2 - 1) * 6).to(dt_), ((rnd(N, nM) * 2 - 1) * 200).to(dt_)
    T1, T2 = (0.5 + rnd(N, nM)).to(dt_), (0.02 + 0.1 * rnd(N, nM)).to(dt_)
    γ, dt = torch.tensor(4257.6, dtype=dt_), torch.tensor([4e-6], dtype=dt_)
    bo = O.rfgr2beff(rf, gr, loc, Δf=df, γ=γ)
    Mi_o, B_o = M0.clone().requires_grad_(True), bo.clone().requires_grad_(True)
    Mo_o = O.blochsim(Mi_o, B_o, T1=T1, T2=T2, γ=γ, dt=dt)
    Mo_o.sum().backward()
    bh = beffective.rfgr2beff(dev(rf), dev(gr), dev(loc), Δf=dev(df), γ=dev(γ))
    assert_close(bh, bo, tag, 'beff')
    Mi_h, B_h = dev(M0).requires_grad_(True), dev(bo).requires_grad_(True)
    Mo_h = sims.blochsim(Mi_h, B_h, T1=dev(T1), T2=dev(T2), γ=dev(γ), dt=dev(dt))
    Mo_h.sum().backward()
    assert_close(Mo_h, Mo_o, tag, 'Mo')
    assert_close(Mi_h.grad, Mi_o.grad, tag, 'gMi')
    assert_close(B_h.grad, B_o.grad, tag, 'gB')
    Mf = fused.blochsim_rfgr(dev(M0), dev(rf), dev(gr), dev(loc), Δf=dev(df), γ_beff=dev(γ),
                             T1=dev(T1), T2=dev(T2), γ=dev(γ), dt=dev(dt))
    assert max_abs(Mf, sims.blochsim(dev(M0), bh, T1=dev(T1), T2=dev(T2), γ=dev(γ), dt=dev(dt))) == 0.0


@pytest.mark.usefixtures('host_constants')
def test_empty_inputs():
    for N, nM, nT in ((1, 0, 8), (0, 5, 8), (1, 5, 0)):
        M0 = torch.rand(N, nM, 3, device=DEV)
        B = torch.rand(N, nM, nT, 3, device=DEV)
        Mo = sims.blochsim(M0, B, T1=torch.ones(1, 1, device=DEV), T2=torch.ones(1, 1, device=DEV))
        assert Mo.shape == M0.shape
        if nT == 0:
            assert max_abs(Mo, M0) == 0.0            # no steps: unchanged
        b = beffective.rfgr2beff(torch.rand(N, 2, nT, device=DEV), torch.rand(N, 3, nT, device=DEV),
                                 torch.rand(N, nM, 3, device=DEV))
        assert b.shape == (N, nM, nT, 3)


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_unaligned_and_noncontiguous_inputs(tag):
    dt_ = DT[tag]
    gen = torch.Generator().manual_seed(5)
    N, nM, nT = 1, 70, 32
    M0 = torch.rand((N, nM, 3), generator=gen, dtype=torch.float64).to(dt_)
    B = ((torch.rand((N, nM, nT, 3), generator=gen, dtype=torch.float64) * 2 - 1) * 5).to(dt_)
    kw = dict(T1=torch.tensor([[1.]], dtype=dt_), T2=torch.tensor([[0.04]], dtype=dt_),
              γ=torch.tensor(4257.6, dtype=dt_), dt=torch.tensor(4e-6, dtype=dt_))
    ref = O.blochsim(M0, B, **kw)
    kd = {k: dev(v) for k, v in kw.items()}
    # Beff at an odd element offset inside a larger buffer: rows not 16-B aligned
    buf = torch.zeros(B.numel() + 1, dtype=dt_, device=DEV)
    buf[1:] = dev(B).reshape(-1)
    Bu = buf[1:].view(B.shape)
    assert Bu.data_ptr() % 16 != 0
    assert_close(sims.blochsim(dev(M0), Bu, **kd), ref, tag, 'unaligned Beff')
    # non-contiguous views (time-major storage, permuted to the API layout)
    Bt = dev(B).permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
    assert not Bt.is_contiguous()
    Mt = dev(M0).transpose(1, 2).contiguous().transpose(1, 2)
    assert_close(sims.blochsim(Mt, Bt, **kd), ref, tag, 'non-contiguous')
    # general *Nd (non-compact) layout (N, nx, ny, 3): flattened internally
    M3, B3 = dev(M0).reshape(1, 7, 10, 3), dev(B).reshape(1, 7, 10, nT, 3)
    out = sims.blochsim(M3, B3, **kd)
    assert out.shape == (1, 7, 10, 3)
    assert_close(out.reshape(1, 70, 3), ref, tag, 'general Nd')
    T1m = (0.5 + torch.rand((1, 7, 10), generator=gen, dtype=torch.float64)).to(dt_)
    T2m = (0.02 + 0.1 * torch.rand((1, 7, 10), generator=gen, dtype=torch.float64)).to(dt_)
    refm = O.blochsim(M0.reshape(1, 7, 10, 3), B.reshape(1, 7, 10, nT, 3), T1=T1m, T2=T2m,
                      γ=kw['γ'], dt=kw['dt'])
    assert_close(sims.blochsim(M3, B3, T1=dev(T1m), T2=dev(T2m), γ=kd['γ'], dt=kd['dt']), refm,
                 tag, 'general Nd, per-spin T1/T2')


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_large_rotation_angles(tag):
    r"""|B| up to ~150 G => phi up to ~16 rad per step: the general (sincos) branch of the
    rotation coefficients, mixed within one wave with tiny and zero fields."""
    dt_ = DT[tag]
    gen = torch.Generator().manual_seed(17)
    N, nM, nT = 1, 128, 48
    M0 = torch.rand((N, nM, 3), generator=gen, dtype=torch.float64).to(dt_)
    B = ((torch.rand((N, nM, nT, 3), generator=gen, dtype=torch.float64) * 2 - 1) * 100).to(dt_)
    B[:, ::3] *= 1e-3          # small-angle lanes next to large-angle lanes
    B[:, 5] = 0
    B[:, 64:, :16] *= 0.02     # a whole wave below the polynomial threshold for some steps
    kw = dict(T1=torch.tensor([[1.]], dtype=dt_), T2=torch.tensor([[0.04]], dtype=dt_),
              γ=torch.tensor(4257.6, dtype=dt_), dt=torch.tensor(4e-6, dtype=dt_))
    Mi_o, B_o = M0.clone().requires_grad_(True), B.clone().requires_grad_(True)
    Mo_o = O.blochsim(Mi_o, B_o, **kw)
    Mo_o.sum().backward()
    Mi_h, B_h = dev(M0).requires_grad_(True), dev(B).requires_grad_(True)
    Mo_h = sims.blochsim(Mi_h, B_h, **{k: dev(v) for k, v in kw.items()})
    Mo_h.sum().backward()
    assert_close(Mo_h, Mo_o, tag, 'Mo')
    assert_close(Mi_h.grad, Mi_o.grad, tag, 'gMi')
    if tag == 'f64':
        assert_close(B_h.grad, B_o.grad, tag, 'gB')
    else:   # the fp32 reference adjoint divides by phi and cancels; compare with fp64 truth
        Mi_d, B_d = M0.double().requires_grad_(True), B.double().requires_grad_(True)
        O.blochsim(Mi_d, B_d, **{k: v.double() for k, v in kw.items()}).sum().backward()
        e_hip, e_ref = rel_l2(B_h.grad, B_d.grad), rel_l2(B_o.grad, B_d.grad)
        assert e_hip <= max(1e-5, 1.5 * e_ref), (e_hip, e_ref)


@pytest.mark.usefixtures('host_constants')
def test_config1_subset_vs_reference():
    r"""64^3 x 1024 (BASELINE configs[1]): seeded 4096-spin subset vs the reference's rows."""
    G = golden('big_cfg1_f32')
    idx, sp, p, beff, Mo, Mf = _run_subset(1, G)
    assert np.array_equal(idx.numpy(), G['idx']) and max_abs(sp['M0'], G['M0']) == 0.0
    bo = O.rfgr2beff(p['rf'], p['gr'], sp['loc'], Δf=sp['Δf'], γ=sp['γ'])
    print(f'cfg1 beff: max abs diff vs oracle {max_abs(beff, bo):.2e}; fused vs K0+K1 '
          f'{max_abs(Mf, Mo):.2e}')
    assert max_abs(Mf, Mo) == 0.0
    e_sims, e_slow = rel_l2(Mo, G['Mo_sims']), rel_l2(Mo, G['Mo_slow'])
    print(f'cfg1 rel-L2: vs sims {e_sims:.2e}, vs slowsims {e_slow:.2e}, '
          f'reference sims-vs-slowsims {rel_l2(G["Mo_sims"], G["Mo_slow"]):.2e}')
    record('cfg1.Mo.vs_reference_sims', e_sims, 1e-5)
    record('cfg1.Mo.vs_reference_slowsims', e_slow, 1e-5)
    record('cfg1.reference_sims_vs_slowsims', rel_l2(G['Mo_sims'], G['Mo_slow']))
    assert e_sims <= 1e-5 and e_slow <= 1e-5
    # elementwise, the worst of the 4096 spins, against both of the reference's fp32 implementations (which differ from
    # each other by `cfg1.reference_sims_vs_slowsims.max_abs`) and against exact arithmetic
    elementwise('cfg1.Mo.vs_reference_sims', Mo, G['Mo_sims'], ATOL32_REFERENCE)
    elementwise('cfg1.Mo.vs_reference_slowsims', Mo, G['Mo_slow'], ATOL32_REFERENCE)
    elementwise('cfg1.reference_sims_vs_slowsims', G['Mo_sims'], G['Mo_slow'])
    exact = O.blochsim_f64_arith(sp['M0'], bo, consts=gconsts(G, device='cpu'))
    elementwise('cfg1.Mo.HIP.vs_exact', Mo, exact, row_bound=angle_budget(bo, G['const.γ2πdt']), bulk=True)
    elementwise('cfg1.Mo.reference_sims.vs_exact', G['Mo_sims'], exact)


@pytest.mark.usefixtures('host_constants')
def test_config2_subset_vs_reference():
    r"""128^3 x 4096 (configs[2], the headline): 4096-spin subset.  At nT = 4096 the
    reference's own two fp32 implementations differ by more than 1e-5 on this workload
    (stored in the fixture), so -- as SURVEY §8c prescribes -- the bar is the error against
    exact (fp64) arithmetic on the SAME fp32-rounded constants: not worse than the
    reference's own."""
    G = golden('big_cfg2_f32')
    idx, sp, p, beff, Mo, Mf = _run_subset(2, G)
    assert np.array_equal(idx.numpy(), G['idx'])
    bo = O.rfgr2beff(p['rf'], p['gr'], sp['loc'], Δf=sp['Δf'], γ=sp['γ'])
    print(f'cfg2 beff: max abs diff vs oracle {max_abs(beff, bo):.2e}; fused vs K0+K1 '
          f'{max_abs(Mf, Mo):.2e}')
    assert max_abs(Mf, Mo) == 0.0
    assert rel_l2(beff, bo) < 1e-6
    exact = O.blochsim_f64_arith(sp['M0'], bo, consts=gconsts(G, device='cpu'))
    e_hip = rel_l2(Mo, exact)
    e_sims, e_slow = rel_l2(G['Mo_sims'], exact), rel_l2(G['Mo_slow'], exact)
    print(f'cfg2 rel-L2 vs exact arithmetic: HIP {e_hip:.2e}, reference sims {e_sims:.2e}, '
          f'slowsims {e_slow:.2e}; HIP vs sims {rel_l2(Mo, G["Mo_sims"]):.2e}')
    # the north star's 1e-5, hard, at the headline length: precise step (the default) -- 4.8e-6
    # measured, where the reference's own fp32 runs are 2.6e-5 / 2.9e-5 from exact arithmetic
    assert mrphy_amd.precision.get() == 'precise'
    assert e_hip <= 1e-5
    # against the reference's fp32 run the distance is the REFERENCE's own noise: bounded by it
    assert rel_l2(Mo, G['Mo_sims']) <= 1e-5 + e_sims
    with mrphy_amd.precision('fast'):            # the all-fp32 step: not worse than the reference
        Mo_f = sims.blochsim_consts(dev(sp['M0']), dev(beff), **gconsts(G))
    e_fast = rel_l2(Mo_f, exact)
    print(f'cfg2 fast step: {e_fast:.2e} from exact')
    assert e_hip < 0.5 * e_fast and e_fast <= max(1e-5, min(e_sims, e_slow))
    for k, v in (('HIP', e_hip), ('reference_sims', e_sims), ('reference_slowsims', e_slow),
                 ('HIP_fast_step', e_fast)):
        record(f'cfg2.Mo.{k}.vs_exact', v, 1e-5 if k == 'HIP' else None)
    record('cfg2.Mo.HIP.vs_reference_sims', rel_l2(Mo, G['Mo_sims']), 1e-5 + e_sims)
    budget = angle_budget(bo, G['const.γ2πdt'])          # per spin: 2^-23 x total rotation angle (tests/util.py)
    elementwise('cfg2.Mo.HIP.vs_exact', Mo, exact, row_bound=budget, bulk=True)
    e_ref_el = elementwise('cfg2.Mo.reference_sims.vs_exact', G['Mo_sims'], exact)
    elementwise('cfg2.Mo.reference_slowsims.vs_exact', G['Mo_slow'], exact)
    elementwise('cfg2.Mo.HIP_fast_step.vs_exact', Mo_f, exact)
    elementwise('cfg2.Mo.HIP.vs_reference_sims', Mo, G['Mo_sims'], float(budget.max()) + e_ref_el)


@pytest.mark.usefixtures('host_constants')
def test_config2_subset_gradients_at_headline_length():
    r"""The backward half at the headline length (128^3 x 4096 subset, 4096 spins x 4096 steps):
    ``grad_M0, grad_rf, grad_gr`` of ``sum(Mo)`` from both routes within 1e-5 of exact
    differentiation (oracle/bloch_c.c; the reference tests gradient equality in
    tests/test_sims.py:104-105 and tests/test_slowsims.py:86-96, at atol 1e-4 in fp32)."""
    G = golden('big_cfg2_f32')
    idx, sp, p = cases.big_subset(2, torch.float32, 4096)
    assert np.array_equal(idx.numpy(), G['idx'])
    _assert_grads_1e5('cfg2_grad', sp, p, G)


@pytest.mark.usefixtures('host_constants')
def test_full_size_config1_properties():
    r"""The whole 64^3 x 1024 cube on the device (Beff = 3.2 GB): size-independent properties.
    (i) rows of the full run == the subset run (spins independent, order preserved);
    (ii) fused kernel == rfgr2beff + blochsim, bit for bit;
    (iii) without relaxation |M| is conserved;  (iv) without relaxation the map is linear in M."""
    n, nT = 64, 1024
    sp = synth.cube_spins(n, dtype=torch.float32, device=DEV, seed_M0=2001)
    p = synth.pulse(nT, dtype=torch.float32, device=DEV)
    beff = beffective.rfgr2beff(p['rf'], p['gr'], sp['loc'], Δf=sp['Δf'], γ=sp['γ'])
    kw = dict(γ=sp['γ'], dt=p['dt'])
    Mo = sims.blochsim(sp['M0'], beff, T1=sp['T1'], T2=sp['T2'], **kw)
    Mf = fused.blochsim_rfgr(sp['M0'], p['rf'], p['gr'], sp['loc'], Δf=sp['Δf'], γ_beff=sp['γ'],
                             T1=sp['T1'], T2=sp['T2'], **kw)
    assert max_abs(Mf, Mo) == 0.0
    G = golden('big_cfg1_f32')
    idx = torch.from_numpy(G['idx']).to(DEV)
    assert max_abs(sp['M0'][:, idx], G['M0']) == 0.0
    # rows of the full run == a run on those rows alone (same constants: this box's)
    sub = {k: (v[:, idx] if v.shape[1] > 1 else v) for k, v in sp.items()}
    Ms = fused.blochsim_rfgr(sub['M0'], p['rf'], p['gr'], sub['loc'], Δf=sub['Δf'], γ_beff=sub['γ'],
                             T1=sub['T1'], T2=sub['T2'], **kw)
    assert max_abs(Mo[:, idx], Ms) == 0.0
    # and they are the reference's rows up to the constants: this run formed its own (default mode:
    # exp rounded once), the reference run used its CPU's expf -- an ulp of E (2^-24) on some spins,
    # applied nT times, plus the 1e-5 of the arithmetic
    d_rows = record('cfg1_full.rows_default_constants_vs_reference_sims', rel_l2(Mo[:, idx], G['Mo_sims']),
                    1e-5 + nT * 2.0 ** -24)
    assert d_rows <= 1e-5 + nT * 2.0 ** -24
    Mn = sims.blochsim(sp['M0'], beff, **kw)
    nrm0, nrm1 = sp['M0'].norm(dim=-1), Mn.norm(dim=-1)
    drift = (nrm1 - nrm0).abs() / nrm0
    # fp32 round-off only; the reference's own two implementations drift by 4.1e-5 / 6.7e-5 (max)
    # and 2.3e-6 (mean) on the 4096-spin subset of this workload
    print(f'|M| drift without relaxation over {nT} steps: max {float(drift.max()):.2e}, '
          f'mean {float(drift.mean()):.2e}')
    record('cfg1_full.norm_drift_no_relax.max', float(drift.max()), 2e-4,
           note="the reference's two fp32 implementations drift by 4.1e-5 / 6.7e-5 (max) on the subset")
    record('cfg1_full.norm_drift_no_relax.mean', float(drift.mean()), 1e-5)
    assert float(drift.max()) < 2e-4 and float(drift.mean()) < 1e-5
    M2 = torch.rand_like(sp['M0'])
    lin = sims.blochsim(0.5 * sp['M0'] - 2.0 * M2, beff, **kw)
    assert rel_l2(lin, 0.5 * Mn - 2.0 * sims.blochsim(M2, beff, **kw)) < 1e-5   # fp32 round-off of 1024 steps
    del beff
    torch.cuda.empty_cache()


@pytest.mark.usefixtures('host_constants')
def test_constants_modes():
    r"""The three ways the per-spin constants are formed (mrphy_amd/_host.py: constants_on) on the
    config-1 subset: the default -- exp evaluated in fp64, rounded once: device-independent bits --,
    torch's own fp32 exp on the device ('native', the reference's literal behaviour there) and on the
    CPU (what the golden run used).  The kernels are the same; results differ only through 1-ulp
    differences of E on some spins, applied nT times: bounded by nT * 2^-24, measured far below."""
    G = golden('big_cfg1_f32')
    idx, sp, p = cases.big_subset(1, torch.float32, 4096)
    spd, pd = to_dev(sp, DEV), to_dev(p, DEV)
    beff = beffective.rfgr2beff(pd['rf'], pd['gr'], spd['loc'], Δf=spd['Δf'], γ=spd['γ'])
    kw = dict(T1=spd['T1'], T2=spd['T2'], γ=spd['γ'], dt=pd['dt'])
    nT = beff.shape[-2]
    ulp = 2.0 ** -24
    with mrphy_amd.constants_on(None):                          # the default
        M_def = sims.blochsim(spd['M0'], beff, **kw)
        _, E1_def, E2_def, _ = sims.relax_constants(spd['T1'], spd['T2'], spd['γ'], pd['dt'], 4, DEV)
        # the same constants formed on the host: same bits (fp64 exp, one rounding)
        _, E1_h, E2_h, _ = sims.relax_constants(sp['T1'], sp['T2'], sp['γ'], p['dt'], 4, torch.device('cpu'))
    with mrphy_amd.constants_on('native'):
        M_nat = sims.blochsim(spd['M0'], beff, **kw)
        E2_nat = torch.exp(-pd['dt'] / spd['T2'])
    M_host = sims.blochsim(spd['M0'], beff, **kw)              # autouse fixture: torch's CPU exp
    E2_cpu = torch.exp(-p['dt'] / sp['T2'])
    assert torch.equal(E1_def.cpu(), E1_h) and torch.equal(E2_def.cpu(), E2_h)   # device-independent
    f_nat = float((E2_nat.cpu() != E2_cpu).double().mean())
    f_def = float((E2_def.cpu().reshape(-1) != E2_cpu.reshape(-1)).double().mean())
    record('constants.frac_spins_E2_differs.native_device_exp_vs_cpu_exp', f_nat)
    record('constants.frac_spins_E2_differs.rounded_once_vs_cpu_exp', f_def)
    assert max_abs(E2_nat, E2_cpu) <= 2 * ulp and max_abs(E2_def.reshape(-1), E2_cpu.reshape(-1)) <= ulp
    for name, M in (('default_rounded_once', M_def), ('native_device_exp', M_nat)):
        d = record(f'constants.cfg1.Mo.{name}.vs_cpu_exp_constants', rel_l2(M, M_host), nT * ulp)
        assert d <= nT * ulp
        d = record(f'constants.cfg1.Mo.{name}.vs_reference_sims', rel_l2(M, G['Mo_sims']), 1e-5 + nT * ulp)
        assert d <= 1e-5 + nT * ulp
    record('constants.cfg1.Mo.cpu_exp_constants.vs_reference_sims', rel_l2(M_host, G['Mo_sims']),
           note="this box's CPU exp vs the exp of the CPU that produced the golden rows: two CPUs differ "
                "too (the golden comparisons at 1e-5 use the constants stored with the fixture)")
    print(f'constants: E2 differs from the CPU exp on {100 * f_nat:.1f}% (device exp) / {100 * f_def:.1f}% '
          f'(rounded once) of spins; Mo rel-L2 vs CPU-constant run {rel_l2(M_nat, M_host):.2e} / '
          f'{rel_l2(M_def, M_host):.2e} at nT = {nT}')
    # the default is not further from the reference's golden rows than the device exp was
    assert rel_l2(M_def, G['Mo_sims']) <= rel_l2(M_nat, G['Mo_sims']) + 1e-6
    # the same through the PUBLIC signature (sims.blochsim(T1=, T2=): the kernels form their own
    # constants) for the headline and for configs[4], next to the fixture-constant figures of the config tests.  The
    # bound is what those tests use -- 1e-5 plus the reference's own distance from exact arithmetic (beyond nT = 1024
    # the reference's fp32 runs are further than 1e-5 from exact themselves) -- plus nT ulps for the two exp()s.
    for cfg in (2, 4):
        Gc = golden(f'big_cfg{cfg}_f32')
        _, spc, pc = cases.big_subset(cfg, torch.float32, 4096)
        if cfg == 4:                  # configs[4]'s fine pulse is the reference's own interpT output (tests/test_fused.py)
            I = golden('interp_f32')
            pc = dict(rf=t(I['rf']), gr=t(I['gr']), dt=t(I['dt']))
        sd, pd_ = to_dev(spc, DEV), to_dev(pc, DEV)
        bc = beffective.rfgr2beff(pd_['rf'], pd_['gr'], sd['loc'], Δf=sd['Δf'], γ=sd['γ'])
        kwc = dict(T1=sd['T1'], T2=sd['T2'], γ=sd['γ'], dt=pd_['dt'])
        nTc = bc.shape[-2]
        exact = O.blochsim_f64_arith(spc['M0'], bc.cpu(), consts=gconsts(Gc, device='cpu'))
        e_ref = rel_l2(Gc['Mo_sims'], exact)
        fixture = rel_l2(sims.blochsim_consts(sd['M0'], bc, **gconsts(Gc)), Gc['Mo_sims'])
        record(f'constants.cfg{cfg}.Mo.fixture_constants.vs_reference_sims', fixture, 1e-5 + e_ref)
        for name, mode in (('default_rounded_once', None), ('native_device_exp', 'native')):
            with mrphy_amd.constants_on(mode):
                Mc = sims.blochsim(sd['M0'], bc, **kwc)
            d = record(f'constants.cfg{cfg}.Mo.{name}.vs_reference_sims', rel_l2(Mc, Gc['Mo_sims']),
                       1e-5 + e_ref + nTc * ulp, note='public signature sims.blochsim(Mi, Beff, T1=, T2=, γ=, dt=)')
            record(f'constants.cfg{cfg}.Mo.{name}.vs_exact_with_the_fixture_constants', rel_l2(Mc, exact))
            assert d <= 1e-5 + e_ref + nTc * ulp, (cfg, name, d)


@pytest.mark.usefixtures('host_constants')
def test_constant_cache_sees_inplace_updates():
    r"""The relaxation constants are cached per (tensor identity, version): an in-place change of
    T1/T2/dt must produce new constants, and a new tensor with the same values must hit nothing
    stale."""
    g = torch.Generator().manual_seed(8)
    N, nM, nT = 1, 130, 24
    M0 = torch.rand(N, nM, 3, generator=g)
    B = torch.randn(N, nM, nT, 3, generator=g) * 0.3
    T1, T2 = 0.5 + torch.rand(N, nM, generator=g), 0.02 + 0.1 * torch.rand(N, nM, generator=g)
    γ, dt = torch.tensor(4257.6), torch.tensor([4e-6])
    dT1, dT2, dγ, ddt = dev(T1), dev(T2), dev(γ), dev(dt)
    a = sims.blochsim(dev(M0), dev(B), T1=dT1, T2=dT2, γ=dγ, dt=ddt)
    assert torch.equal(a, sims.blochsim(dev(M0), dev(B), T1=dT1, T2=dT2, γ=dγ, dt=ddt))   # cached
    dT1.mul_(0.01)
    ddt.mul_(3.0)
    b = sims.blochsim(dev(M0), dev(B), T1=dT1, T2=dT2, γ=dγ, dt=ddt)
    want = O.blochsim(M0, B, T1=T1 * 0.01, T2=T2, γ=γ, dt=dt * 3.0)
    assert rel_l2(b, want) <= 1e-5 and rel_l2(a, want) > 1e-3
    c = fused.blochsim_rfgr(dev(M0), dev(torch.zeros(1, 2, nT)), dev(torch.zeros(1, 3, nT)),
                            dev(torch.zeros(N, nM, 3)), T1=dT1, T2=dT2, γ=dγ, dt=ddt)
    dT2.add_(0.05)
    d = fused.blochsim_rfgr(dev(M0), dev(torch.zeros(1, 2, nT)), dev(torch.zeros(1, 3, nT)),
                            dev(torch.zeros(N, nM, 3)), T1=dT1, T2=dT2, γ=dγ, dt=ddt)
    assert not torch.equal(c, d)


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('n,nT,bound', [(64, 1024, 1.0e-5), (64, 2048, 1.0e-5)])
def test_whole_config_vs_c_restatement(n, nT, bound):
    r"""EVERY spin of BASELINE configs[1] / [4]-sized problems (not a subset): the fp32 HIP result
    against oracle/bloch_c.c -- exact (fp64) arithmetic in the reference's axis/angle form -- on
    the same fp32 inputs and the same fp32 constants.  Bound: the north-star 1e-5 at both lengths
    (precise step; the reference's own fp32 run is 1.0e-5 from exact at nT = 2048)."""
    import bloch_c as C
    import os
    sp, p = synth.cube_spins(n, dtype=torch.float32, seed_M0=11), synth.pulse(nT, dtype=torch.float32)
    N, nM = 1, n ** 3
    # the fp32 constants, formed once on the CPU with the reference's expressions, for both sides
    g = 2 * np.pi * sp['γ'] * p['dt']
    E1, E2 = torch.exp(-p['dt'] / sp['T1']), torch.exp(-p['dt'] / sp['T2'])
    consts = dict(γ2πdt=g, E1=E1, E1_1=E1 - 1, E2=E2)
    Mo = fused.blochsim_rfgr(dev(sp['M0']), dev(p['rf']), dev(p['gr']), dev(sp['loc']), Δf=dev(sp['Δf']),
                             γ_beff=dev(sp['γ']), consts={k: dev(v) for k, v in consts.items()})
    beff = beffective.rfgr2beff(dev(p['rf']), dev(p['gr']), dev(sp['loc']), Δf=dev(sp['Δf']), γ=dev(sp['γ']))
    Mo2 = sims.blochsim_consts(dev(sp['M0']), beff, **{k: dev(v) for k, v in consts.items()})
    assert torch.equal(Mo, Mo2)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    cc = C.constants_from(g, E1, E2, E1 - 1, N=N, nM=nM)
    # like for like: exact arithmetic on the SAME fp32 field the kernels integrate (K0's output is
    # bit-identical to the reference's rfgr2beff) ...
    want = C.blochsim(sp['M0'], beff.cpu(), consts=cc)
    e = rel_l2(Mo, want)
    # ... and, for information, with the field itself formed in double from the fp32 inputs: this
    # adds the rounding of Beff to fp32, which the reference's materialised tensor has as well
    want_d = C.blochsim_rfgr(sp['M0'], p['rf'], p['gr'], sp['loc'], Δf=sp['Δf'], γ_beff=sp['γ'], consts=cc)
    print(f'{n}^3 x {nT}, all {nM} spins: rel-L2 vs fp64 C arithmetic on the same fp32 field {e:.2e} '
          f'(max abs {max_abs(Mo, want):.2e}); with the field in fp64 too: {rel_l2(Mo, want_d):.2e}')
    record(f'whole_{n}c_x{nT}.Mo.vs_exact_on_same_f32_field', e, bound)
    record(f'whole_{n}c_x{nT}.Mo.vs_exact_with_f64_field', rel_l2(Mo, want_d),
           note=f'exact-vs-exact (Beff rounded to fp32 or not): {rel_l2(want_d, want):.3e}')
    assert e <= bound
    # the worst of all n^3 spins, each against its own budget (2^-23 x its total rotation angle)
    elementwise(f'whole_{n}c_x{nT}.Mo.vs_exact_on_same_f32_field', Mo, want, row_bound=angle_budget(beff, g), bulk=True)


@pytest.mark.usefixtures('host_constants')
def test_fuzz_forward_vs_c_restatement():
    r"""40 random problems (fp64): batch 1-3, 1-200 spins, 1-70 steps, 1/2/5/8/9 coils, with and
    without b1Map / Δf / relaxation, scalar or per-spin constants, batch-1 or per-batch pulses.
    rfgr2beff + blochsim and the fused kernel against oracle/bloch_c.c, max-abs <= 1e-9."""
    import bloch_c as C
    # MRPHY_FUZZ_SEED / MRPHY_FUZZ_CASES: other seeds and more cases for a one-off campaign (with a seed
    # given, the coil counts also cover every capacity of the parallel-transmit kernels)
    g = torch.Generator().manual_seed(int(os.environ.get('MRPHY_FUZZ_SEED', 20261004)))
    campaign = 'MRPHY_FUZZ_SEED' in os.environ
    coils = (1, 1, 2, 5, 8, 9) if not campaign else (1, 1, 1, 2, 5, 8, 9, 12, 16, 17, 24, 32, 33, 40, 47, 64, 66)
    rnd = lambda *s: torch.rand(s, generator=g, dtype=torch.float64)  # noqa: E731
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))  # noqa: E731
    for case in range(int(os.environ.get('MRPHY_FUZZ_CASES', 40))):
        N, nM, nT = ri(1, 3), ri(1, 200), ri(1, 70)
        if campaign and ri(0, 1):
            nT = 16 * ri(1, 6)                      # the line-granular fp64 kernels (rows on 128-B lines)
        nC = coils[ri(0, len(coils) - 1)]
        Np = N if ri(0, 1) else 1
        has_b1 = bool(ri(0, 3))                     # multi-coil rf without a map: coils add
        rf = ((rnd(Np, 2, nT, nC) if (nC > 1 or ri(0, 1)) else rnd(Np, 2, nT)) * 2 - 1) * 1.2
        gr = (rnd(Np, 3, nT) * 2 - 1) * 2
        loc = (rnd(N, nM, 3) * 2 - 1) * 8
        b1 = None
        if has_b1:
            b1 = (rnd(N, nM, 2, nC) * 2 - 1) if rf.ndim == 4 else (rnd(N, nM, 2) * 2 - 1)
        df = ((rnd(N, nM) * 2 - 1) * 300) if ri(0, 1) else None
        relax = bool(ri(0, 2))
        per_spin = bool(ri(0, 1))
        T1 = (0.3 + rnd(N, nM)) if per_spin else torch.tensor([[0.8]], dtype=torch.float64)
        T2 = (0.01 + 0.1 * rnd(N, nM)) if per_spin else torch.tensor([[0.05]], dtype=torch.float64)
        γ = (4257.6 * (1 + 0.05 * rnd(N, nM))) if per_spin else torch.tensor(4257.6, dtype=torch.float64)
        dt = torch.tensor([4e-6 * (1 + case % 3)], dtype=torch.float64)
        M0 = rnd(N, nM, 3) * 2 - 1
        kw = dict(T1=T1, T2=T2) if relax else {}
        want = C.blochsim_rfgr(M0, rf, gr, loc, Δf=df, b1Map=b1, γ_beff=γ, γ=γ, dt=dt, **kw)
        d = lambda x: None if x is None else dev(x)  # noqa: E731
        kwd = {k: dev(v) for k, v in kw.items()}
        beff = beffective.rfgr2beff(d(rf), d(gr), d(loc), Δf=d(df), b1Map=d(b1), γ=d(γ))
        two = sims.blochsim(d(M0), beff, γ=d(γ), dt=d(dt), **kwd)
        fu = fused.blochsim_rfgr(d(M0), d(rf), d(gr), d(loc), Δf=d(df), b1Map=d(b1), γ_beff=d(γ),
                                 γ=d(γ), dt=d(dt), **kwd)
        tag = f'case {case}: N={N} nM={nM} nT={nT} nC={nC} Np={Np} b1={has_b1} df={df is not None} ' \
              f'relax={relax} per_spin={per_spin} rf.ndim={rf.ndim}'
        assert max_abs(two, want) <= 1e-9, tag
        assert max_abs(fu, want) <= 1e-9, tag


@pytest.mark.usefixtures('host_constants')
def test_fuzz_gradients_vs_oracle():
    r"""24 random problems (fp64): gradients of a weighted sum of Mo w.r.t. Mi, rf, gr through
    rfgr2beff + blochsim and through the fused route (fused adjoint when nT % 16 == 0 and <= 8
    coils, composed otherwise) against the torch oracle's autograd, max-abs <= 1e-9."""
    g = torch.Generator().manual_seed(int(os.environ.get('MRPHY_FUZZ_SEED', 424242)))
    campaign = 'MRPHY_FUZZ_SEED' in os.environ
    coils = (1, 1, 3, 8, 9) if not campaign else (1, 1, 1, 3, 4, 8, 9, 12, 13, 16, 17, 24, 32, 33, 40, 64, 66)
    rnd = lambda *s: torch.rand(s, generator=g, dtype=torch.float64)  # noqa: E731
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))  # noqa: E731
    import random
    from mrphy_amd import _hist
    prng = random.Random(6)                                   # round 6: every case also draws a way to cut the history
    for case in range(int(os.environ.get('MRPHY_FUZZ_CASES', 24))):
        _hist.set_policy(parts=prng.choice((1, 2, 3, 4, 8)), layout=prng.choice((0, 1)), min_bytes=0, min_tiles_per_part=1)
        N, nM = ri(1, 2), ri(1, 150)
        nT = (16, 32, 48, ri(1, 40))[ri(0, 3)]
        nC = coils[ri(0, len(coils) - 1)]
        Np = N if ri(0, 1) else 1
        has_b1 = nC > 1 or bool(ri(0, 1))
        rf = ((rnd(Np, 2, nT, nC) if (nC > 1 or ri(0, 1)) else rnd(Np, 2, nT)) * 2 - 1) * 1.2
        gr = (rnd(Np, 3, nT) * 2 - 1) * 2
        loc = (rnd(N, nM, 3) * 2 - 1) * 8
        b1 = ((rnd(N, nM, 2, nC) * 2 - 1) if rf.ndim == 4 else (rnd(N, nM, 2) * 2 - 1)) if has_b1 else None
        df = ((rnd(N, nM) * 2 - 1) * 300) if ri(0, 1) else None
        relax = bool(ri(0, 2))
        T1, T2 = 0.3 + rnd(N, nM), 0.01 + 0.1 * rnd(N, nM)
        γ, dt = torch.tensor(4257.6, dtype=torch.float64), torch.tensor([4e-6], dtype=torch.float64)
        M0, w = rnd(N, nM, 3) * 2 - 1, rnd(N, nM, 3) * 2 - 1
        kw = dict(T1=T1, T2=T2) if relax else {}

        def run(kind):
            on = (lambda x: x) if kind == 'oracle' else (lambda x: None if x is None else dev(x))
            Mi, r, q = (on(x).clone().requires_grad_(True) for x in (M0, rf, gr))
            kk = {k: on(v) for k, v in kw.items()}
            if kind == 'oracle':
                Mo = O.blochsim(Mi, O.rfgr2beff(r, q, loc, Δf=df, b1Map=b1, γ=γ), γ=γ, dt=dt, **kk)
            elif kind == 'two':
                be = beffective.rfgr2beff(r, q, on(loc), Δf=on(df), b1Map=on(b1), γ=on(γ))
                Mo = sims.blochsim(Mi, be, γ=on(γ), dt=on(dt), **kk)
            else:
                Mo = fused.blochsim_rfgr(Mi, r, q, on(loc), Δf=on(df), b1Map=on(b1), γ_beff=on(γ),
                                         γ=on(γ), dt=on(dt), **kk)
            (Mo * on(w)).sum().backward()
            return Mi.grad, r.grad, q.grad
        ora = run('oracle')
        tag = f'case {case}: N={N} nM={nM} nT={nT} nC={nC} Np={Np} b1={has_b1} df={df is not None} relax={relax}'
        for kind in ('two', 'fused'):
            for a, b, nm in zip(run(kind), ora, ('gMi', 'grf', 'ggr')):
                assert a.shape == b.shape and max_abs(a, b) <= 1e-9, f'{tag} {kind} {nm} {max_abs(a, b):.2e}'


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('hdt', [torch.bfloat16, torch.float16])
def test_half_inputs_are_computed_in_fp32(hdt):
    r"""fp16 / bf16 tensors (which the reference accepts): computed in fp32, returned in the
    caller's dtype, gradients flow through the casts."""
    g = torch.Generator().manual_seed(3)
    N, nM, nT = 1, 70, 32
    M0 = torch.rand(N, nM, 3, generator=g).to(hdt)
    rf, gr = (torch.rand(N, 2, nT, generator=g) - 0.5).to(hdt), (torch.rand(N, 3, nT, generator=g) - 0.5).to(hdt)
    loc = ((torch.rand(N, nM, 3, generator=g) - 0.5) * 8).to(hdt)
    T1, T2 = torch.tensor([[1.0]]), torch.tensor([[0.05]])
    r_, g_ = dev(rf).requires_grad_(True), dev(gr).requires_grad_(True)
    beff = beffective.rfgr2beff(r_, g_, dev(loc))
    assert beff.dtype == hdt and beff.shape == (N, nM, nT, 3)
    Mo = sims.blochsim(dev(M0), beff, T1=dev(T1), T2=dev(T2))
    assert Mo.dtype == hdt
    Mo.float().sum().backward()
    assert r_.grad.dtype == hdt and g_.grad.dtype == hdt and bool(torch.isfinite(r_.grad.float()).all())
    # the same numbers as the fp32 path on the upcast inputs, rounded once at the end
    b32 = beffective.rfgr2beff(dev(rf).float(), dev(gr).float(), dev(loc).float())
    assert torch.equal(beff, b32.to(hdt))
    want = sims.blochsim(dev(M0).float(), b32.to(hdt).float(), T1=dev(T1), T2=dev(T2)).to(hdt)
    assert torch.equal(Mo, want)
    Mf = fused.blochsim_rfgr(dev(M0), dev(rf), dev(gr), dev(loc), T1=dev(T1), T2=dev(T2))
    assert Mf.dtype == hdt
    M1, _ = slowsims.blochsim_1step(dev(M0), dev(M0), beff[:, :, 0], torch.tensor(0.99, device=DEV),
                                    torch.tensor(-0.01, device=DEV), torch.tensor(0.9, device=DEV),
                                    torch.tensor(0.107, device=DEV))
    assert M1.dtype == hdt


# ---------------------------------------------------------------------------------------------
# autograd through the 1-step form and its helpers
# ---------------------------------------------------------------------------------------------
@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_onestep_gradients_vs_oracle_autograd(tag):
    c = cases.onestep_case(DT[tag])
    w = torch.linspace(0.5, 1.5, c['M'].numel(), dtype=DT[tag]).reshape(c['M'].shape)
    # oracle: autograd over beff2uϕ / uϕrot / relaxation, as the reference
    M_o, b_o = _leaf(c['M']), _leaf(c['b'])
    Mn_o, _ = O.blochsim_1step(M_o, M_o, b_o, c['E1'], c['E1_1'], c['E2'], c['γ2πdt'])
    (Mn_o * w).sum().backward()
    M_h, b_h = _leaf(c['M'], DEV), _leaf(c['b'], DEV)
    Mn_h, Mold = slowsims.blochsim_1step(M_h, M_h, b_h, dev(c['E1']), dev(c['E1_1']), dev(c['E2']),
                                         dev(c['γ2πdt']))
    assert Mold is M_h and Mn_h.grad_fn is not None
    (Mn_h * dev(w)).sum().backward()
    assert_close(Mn_h, Mn_o, tag, '1step value (grad path)')
    assert_close(M_h.grad, M_o.grad, tag, 'd(1step)/dM')
    # d/db: rows with a field agree with the reference's autograd.  The zero-field row (0, 3) is
    # where the reference's two implementations differ: autograd through F.normalize's clamp gives
    # 0 there (slowsims), the explicit Jacobian gives the analytic limit -γ2πdt (m x E h)
    # (sims.py:229-259 with the forward's clamp) -- which is what the kernel returns.
    nz = (c['b'] != 0).any(dim=-1)
    assert int((~nz).sum()) == 1
    assert_close(b_h.grad.cpu()[nz], b_o.grad[nz], tag, 'd(1step)/db')
    m, E = c['M'][~nz].double(), torch.stack([c['E2'], c['E2'], c['E1']], -1)[~nz].double()
    lim = -c['γ2πdt'].double() * torch.cross(m, E * w[~nz].double(), dim=-1)
    assert_close(b_h.grad.cpu()[~nz], lim, tag, 'd(1step)/db at zero field = analytic limit')
    # the no-grad path (mrphy_blochsim_1step) and the grad path (mrphy_blochsim_fwd, nT = 1): same bits
    with torch.no_grad():
        Mn_p, _ = slowsims.blochsim_1step(M_h, M_h, b_h, dev(c['E1']), dev(c['E1_1']), dev(c['E2']),
                                          dev(c['γ2πdt']))
    assert Mn_p.grad_fn is None and torch.equal(Mn_p, Mn_h.detach())
    # chained steps: the reference's implicit-Jacobian use of 1step
    M_o2, M_h2 = _leaf(c['M']), _leaf(c['M'], DEV)
    a, bdev = M_o2, M_h2
    for _ in range(3):
        a, _old = O.blochsim_1step(a, a, c['b'], c['E1'], c['E1_1'], c['E2'], c['γ2πdt'])
        bdev, _old = slowsims.blochsim_1step(bdev, bdev, dev(c['b']), dev(c['E1']), dev(c['E1_1']),
                                             dev(c['E2']), dev(c['γ2πdt']))
    a.sum().backward()
    bdev.sum().backward()
    assert_close(M_h2.grad, M_o2.grad, tag, 'chained 1step dM')
    # the four constants are differentiable too (round 3), as under the reference's autograd
    co = {k: _leaf(c[k]) for k in ('E1', 'E1_1', 'E2', 'γ2πdt')}
    ch = {k: _leaf(c[k], DEV) for k in co}
    Mo_c, _ = O.blochsim_1step(c['M'].clone(), None, c['b'], co['E1'], co['E1_1'], co['E2'], co['γ2πdt'])
    (Mo_c * w).sum().backward()
    Mh_c, _ = slowsims.blochsim_1step(dev(c['M']), None, dev(c['b']), ch['E1'], ch['E1_1'], ch['E2'], ch['γ2πdt'])
    (Mh_c * dev(w)).sum().backward()
    for k in co:
        assert ch[k].grad is not None and ch[k].grad.shape == co[k].grad.shape, k
        assert_close(ch[k].grad, co[k].grad, tag, f'd(1step)/d{k}')


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_beff2uphi_uphirot_gradients_vs_oracle_autograd(tag):
    c = cases.onestep_case(DT[tag])
    dt_ = DT[tag]
    b0 = c['b'].clone()
    b0[0, 3] = torch.tensor([1., -2., .5], dtype=dt_)     # the zero-field row is tested on its own below
    g0 = c['γ2πdt']
    # beff2uϕ: d/d beff and d/d γ2πdt
    wU = torch.linspace(-1, 1, b0.numel(), dtype=dt_).reshape(b0.shape)
    wP = torch.linspace(0.3, 2, b0.numel() // 3, dtype=dt_).reshape(b0.shape[:-1])
    b_o, g_o = _leaf(b0), _leaf(g0)
    U_o, P_o = O.beff2uphi(b_o, g_o)
    ((U_o * wU).sum() + (P_o * wP).sum()).backward()
    b_h, g_h = _leaf(b0, DEV), _leaf(g0, DEV)
    U_h, P_h = beffective.beff2uϕ(b_h, g_h)
    assert U_h.grad_fn is not None and P_h.grad_fn is not None
    ((U_h * dev(wU)).sum() + (P_h * dev(wP)).sum()).backward()
    assert_close(b_h.grad, b_o.grad, tag, 'd(beff2uϕ)/dbeff')
    assert g_h.grad.shape == g0.shape
    assert_close(g_h.grad, g_o.grad, tag, 'd(beff2uϕ)/dγ2πdt')
    # zero field rows: torch gives gb = gU/eps there (F.normalize's clamp), no NaN
    bz = b0.clone()
    bz[:, 0] = 0
    bz_o, bz_h = _leaf(bz), _leaf(bz, DEV)
    O.beff2uphi(bz_o, g0)[1].sum().backward()
    beffective.beff2uϕ(bz_h, dev(g0))[1].sum().backward()
    assert torch.isfinite(bz_h.grad).all()
    assert_close(bz_h.grad, bz_o.grad, tag, 'd(Φ)/dbeff with a zero row')

    # uϕrot: (…,3) and (…,3,nV), gradients w.r.t. U, Φ and Vi
    U0, P0 = (x.detach() for x in O.beff2uphi(b0, g0))
    V3 = c['M']
    V34 = torch.stack([c['M'], c['M'].flip(-1), c['M'] * 2, -c['M']], dim=-1)
    for V in (V3, V34):
        w = torch.linspace(0.2, 1.7, V.numel(), dtype=dt_).reshape(V.shape)
        ins_o = [_leaf(U0), _leaf(P0), _leaf(V)]
        (O.uphirot(*ins_o) * w).sum().backward()
        ins_h = [_leaf(U0, DEV), _leaf(P0, DEV), _leaf(V, DEV)]
        out = utils.uϕrot(*ins_h)
        assert out.grad_fn is not None
        (out * dev(w)).sum().backward()
        for name, xh, xo in zip(('U', 'Φ', 'Vi'), ins_h, ins_o):
            assert xh.grad.shape == xo.grad.shape
            assert_close(xh.grad, xo.grad, tag, f'd(uϕrot {tuple(V.shape)})/d{name}')

    # the reference's own composition (slowsims.py:42-51) differentiated end to end on the device
    M_o, b_o = _leaf(c['M']), _leaf(b0)
    u, p = O.beff2uphi(b_o, g0)
    O.uphirot(u, p, M_o).sum().backward()
    M_h, b_h = _leaf(c['M'], DEV), _leaf(b0, DEV)
    u, p = beffective.beff2uϕ(b_h, dev(g0))
    utils.uϕrot(u, p, M_h).sum().backward()
    assert_close(M_h.grad, M_o.grad, tag, 'composition dM')
    assert_close(b_h.grad, b_o.grad, tag, 'composition db')


@pytest.mark.usefixtures('host_constants')
@pytest.mark.parametrize('nT', [24, 1000])
def test_no_grad_with_requires_grad_inputs(nT):
    sp, p = _small_problem(nT)
    kw = dict(Δf=sp['Δf'], γ_beff=sp['γ'], T1=sp['T1'], T2=sp['T2'], γ=sp['γ'], dt=p['dt'])
    plain = fused.blochsim_rfgr(sp['M0'], p['rf'], p['gr'], sp['loc'], **kw)
    rf, gr, M0 = (x.clone().requires_grad_(True) for x in (p['rf'], p['gr'], sp['M0']))
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    with torch.no_grad():
        out = fused.blochsim_rfgr(M0, rf, gr, sp['loc'], **kw)
        torch.cuda.synchronize()
        # nothing but the result may have been kept: no checkpoints (12 B x rows x ceil(nT/16))
        assert torch.cuda.memory_allocated() - base <= out.numel() * 4 + 4096
        assert out.grad_fn is None and torch.equal(out, plain)
        beff = beffective.rfgr2beff(rf, gr, sp['loc'], Δf=sp['Δf'], γ=sp['γ'])
        torch.cuda.synchronize()
        base2 = torch.cuda.memory_allocated()
        out2 = sims.blochsim(M0, beff, T1=sp['T1'], T2=sp['T2'], γ=sp['γ'], dt=p['dt'])
        torch.cuda.synchronize()
        # no 12 B/spin-step history under no_grad
        assert torch.cuda.memory_allocated() - base2 <= out2.numel() * 4 + 65536
        assert torch.equal(out2, plain)
    # and with grad enabled the same inputs give the same bits plus gradients
    out3 = fused.blochsim_rfgr(M0, rf, gr, sp['loc'], **kw)
    assert torch.equal(out3.detach(), plain)
    out3.sum().backward()
    assert rf.grad is not None and torch.isfinite(rf.grad).all()


@pytest.mark.usefixtures('host_constants')
def test_inference_mode_and_mismatched_constant_strides():
    sp, p = _small_problem(64)
    ref = fused.blochsim_rfgr(sp['M0'], p['rf'], p['gr'], sp['loc'], Δf=sp['Δf'], γ_beff=sp['γ'],
                              T1=sp['T1'], T2=sp['T2'], γ=sp['γ'], dt=p['dt'])
    with torch.inference_mode():
        T1, T2, γ, dt = (x.clone() for x in (sp['T1'], sp['T2'], sp['γ'], p['dt']))   # inference tensors
        out = fused.blochsim_rfgr(sp['M0'], p['rf'], p['gr'], sp['loc'], Δf=sp['Δf'], γ_beff=γ,
                                  T1=T1, T2=T2, γ=γ, dt=dt)
        beff = beffective.rfgr2beff(p['rf'], p['gr'], sp['loc'], Δf=sp['Δf'], γ=γ)
        out2 = sims.blochsim(sp['M0'], beff, T1=T1, T2=T2, γ=γ, dt=dt)
    assert torch.equal(out, ref) and torch.equal(out2, ref)
    # user-supplied constants whose E1 and E1_1 do not share strides (expanded vs contiguous)
    beff = beffective.rfgr2beff(p['rf'], p['gr'], sp['loc'], Δf=sp['Δf'], γ=sp['γ'])
    nM = sp['M0'].shape[1]
    e1s = torch.tensor(0.999, device=DEV)
    E1 = e1s.reshape(1, 1).expand(1, nM)                      # stride 0
    E1_1 = (E1 - 1).contiguous()                              # stride 1
    E2 = torch.full((1, nM), 0.99, device=DEV)
    g = torch.tensor(0.107, device=DEV)
    a = sims.blochsim_consts(sp['M0'], beff, γ2πdt=g, E1=E1, E1_1=E1_1, E2=E2)
    b = sims.blochsim_consts(sp['M0'], beff, γ2πdt=g, E1=E1.contiguous(), E1_1=E1_1, E2=E2)
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------
# the whole headline workload against exact arithmetic
# ---------------------------------------------------------------------------------------------
@pytest.mark.usefixtures('host_constants')
def test_headline_config_all_spins_vs_c_restatement():
    r"""BASELINE configs[2] in full: all 2 097 152 spins x 4096 steps, fused kernel (bit-identical to
    rfgr2beff + blochsim, asserted elsewhere and in bench.py) against ``oracle/bloch_c.c``: fp64
    integration of the SAME fp32 field the kernels integrate -- every step's field formed in single
    precision exactly as the reference forms its fp32 ``Beff`` tensor (``field_f32=True``) -- with the
    same fp32 constants.  The bound is the north star's 1e-5 relative L2 (the reference's own fp32
    runs are 2.6-2.9e-5 from exact arithmetic at this length).  The distance to an
    integration whose field is formed in fp64 too is recorded beside it (profiles/rNN_parity.json):
    that one contains the rounding of ``Beff`` to fp32, which the reference's tensor has as well and
    which no fp32 ``Beff`` can avoid -- on seeded M0 it alone moves Mo by 2-5e-5 (cfg2/cfg5 entries
    ``exact_on_f64_field_vs_exact_on_f32_field``), so it is reported, not asserted."""
    import bloch_c as C
    n, nT = 128, 4096
    nM = n ** 3
    spc, pc = synth.cube_spins(n, dtype=torch.float32), synth.pulse(nT, dtype=torch.float32)
    sp, p = to_dev(spc, DEV), to_dev(pc, DEV)
    g, E1, E2, E1_1 = sims.relax_constants(spc['T1'], spc['T2'], spc['γ'], pc['dt'], 4, DEV)
    consts = dict(γ2πdt=g, E1=E1, E1_1=E1_1, E2=E2)
    Mo = fused.blochsim_rfgr(sp['M0'], p['rf'], p['gr'], sp['loc'], Δf=sp['Δf'], γ_beff=sp['γ'],
                             consts=consts)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    cc = C.constants_from(g, E1, E2, E1_1, N=1, nM=nM)
    # like for like: exact (fp64) integration of the SAME fp32 field the kernels integrate (the
    # reference's Beff is an fp32 tensor; K0 / the fused field assembly reproduce it bit for bit)
    want = C.blochsim_rfgr(spc['M0'], pc['rf'], pc['gr'], spc['loc'], Δf=spc['Δf'], γ_beff=spc['γ'],
                           consts=cc, field_f32=True)
    err = rel_l2(Mo, want)
    with mrphy_amd.precision('fast'):
        Mo_fast = fused.blochsim_rfgr(sp['M0'], p['rf'], p['gr'], sp['loc'], Δf=sp['Δf'], γ_beff=sp['γ'],
                                      consts=consts)
    err_fast = rel_l2(Mo_fast, want)
    # for information: with the field itself formed in double (adds the rounding of Beff to fp32,
    # which the reference's materialised tensor has as well)
    want_d = C.blochsim_rfgr(spc['M0'], pc['rf'], pc['gr'], spc['loc'], Δf=spc['Δf'], γ_beff=spc['γ'],
                             consts=cc)
    print(f'headline, all {nM} spins x {nT}: rel-L2 vs exact arithmetic on the same fp32 field: '
          f'precise {err:.3e} (max abs {max_abs(Mo, want):.3e}), fast {err_fast:.3e}; '
          f'vs an fp64 field: {rel_l2(Mo, want_d):.3e}')
    assert Mo.shape == (1, nM, 3) and bool(torch.isfinite(Mo).all())
    assert mrphy_amd.precision.get() == 'precise'
    record('headline_all_spins.Mo.vs_exact_on_same_f32_field', err, 1e-5)
    record('headline_all_spins.Mo.fast_step.vs_exact_on_same_f32_field', err_fast)
    record('headline_all_spins.Mo.vs_exact_with_f64_field', rel_l2(Mo, want_d),
           note='includes the rounding of Beff to fp32 (the reference tensor has it too); exact-vs-exact: '
                f'{rel_l2(want_d, want):.3e}')
    assert err <= 1e-5, err                      # the north star, hard, on every spin of the headline
    # elementwise: the worst of the 2 097 152 spins (round 4 printed this number and asserted nothing on it)
    elementwise('headline_all_spins.Mo.vs_exact_on_same_f32_field', Mo, want, row_bound=angle_budget_of_cube(sp, p, g),
                bulk=True)
    elementwise('headline_all_spins.Mo.fast_step.vs_exact_on_same_f32_field', Mo_fast, want)       # recorded, not asserted
    elementwise('headline_all_spins.Mo.vs_exact_with_f64_field', Mo, want_d)                       # (includes Beff's rounding)
    assert err < 0.5 * err_fast
    # ... and against the integration whose field is formed in fp64 as well -- the yardstick of round 2,
    # which shares nothing with the kernels' field assembly: 8.9e-6 on this workload (M0 = z).  The like-for-like
    # yardstick above leans on oracle/bloch_c.c forming the fp32 field as the reference does; that half of the
    # argument is gated by test_k0_rows_equal_the_reference_beff (the reference's own Beff rows, bit for bit).
    assert rel_l2(Mo, want_d) <= 1e-5, rel_l2(Mo, want_d)


def test_slowsims_blochsim_differentiates_T1_T2_gamma_dt():
    r"""The reference's ``slowsims.blochsim`` forms ``E1, E2, γ2πdt`` with differentiable torch ops
    (``slowsims.py:86-98``): gradients w.r.t. ``T1, T2, γ, dt`` flow.  Here the adjoint sweep returns
    them (``mrphy_blochsim_bwd_consts``) -- per-spin ``T1``/``T2`` maps, a shared ``γ``, a one-entry
    ``dt`` -- against the oracle's autograd, with and without relaxation, fp64 (1e-9 relative) and fp32
    (1e-5); ``Mi`` / ``Beff`` gradients of the same call are unchanged by asking for the constants'."""
    import bloch_oracle as O
    for tag, dtype, tol in (('f64', torch.float64, 1e-9), ('f32', torch.float32, 2e-5)):
        n, nT = 5, 70                                   # 125 spins: tiles straddle; nT % 16 != 0
        sp = synth.cube_spins(n, dtype=dtype, seed_M0=3)
        p = synth.pulse(nT, dtype=dtype)
        beff = O.rfgr2beff(p['rf'], p['gr'], sp['loc'], Δf=sp['Δf'], γ=sp['γ'])
        w = torch.cos(torch.arange(sp['M0'].numel(), dtype=torch.float64) * 0.37).reshape(sp['M0'].shape).to(dtype)
        for relax in (True, False):
            leaf = lambda x, d=None: (x.clone() if d is None else x.to(d).clone()).requires_grad_(True)  # noqa: E731
            names = ('T1', 'T2', 'γ', 'dt') if relax else ('γ', 'dt')
            ref = {k: leaf(sp[k] if k in sp else p[k]) for k in names}
            got = {k: leaf(sp[k] if k in sp else p[k], DEV) for k in names}
            Mo_r, Bo_r = leaf(sp['M0']), leaf(beff)
            Mo_h, Bo_h = leaf(sp['M0'], DEV), leaf(beff, DEV)
            (O.blochsim_slow(Mo_r, Bo_r, **ref) * w).sum().backward()
            with mrphy_amd.constants_on('native'):      # the oracle differentiates through torch.exp
                out = slowsims.blochsim(Mo_h, Bo_h, **got)
            (out * dev(w)).sum().backward()
            for k in names:
                a, b = got[k].grad, ref[k].grad
                assert a is not None and a.shape == b.shape, (tag, relax, k)
                e = record(f'const_grads.{tag}.{"relax" if relax else "norelax"}.{k}', rel_l2(a, b), tol)
                assert e <= tol, (tag, relax, k, e)
            assert rel_l2(Mo_h.grad, Mo_r.grad) <= tol and rel_l2(Bo_h.grad, Bo_r.grad) <= tol
            # the same Mi / Beff gradients as the call that does not ask for the constants'
            M2, B2 = leaf(sp['M0'], DEV), leaf(beff, DEV)
            (slowsims.blochsim(M2, B2, **{k: v.detach() for k, v in got.items()}) * dev(w)).sum().backward()
            assert rel_l2(M2.grad, Mo_h.grad) <= 1e-6 and rel_l2(B2.grad, Bo_h.grad) <= 1e-6


def test_constants_that_require_grad_elsewhere():
    r"""``sims.blochsim`` keeps the reference's contract (``None`` for ``T1, T2, γ, dt``,
    ``sims.py:154,269``)."""
    sp = synth.cube_spins(4, dtype=torch.float32, device=DEV)
    p = synth.pulse(32, dtype=torch.float32, device=DEV)
    beff = beffective.rfgr2beff(p['rf'], p['gr'], sp['loc'], Δf=sp['Δf'], γ=sp['γ'])
    T1 = sp['T1'].clone().requires_grad_(True)
    kw = dict(T2=sp['T2'], γ=sp['γ'], dt=p['dt'])
    M0 = sp['M0'].clone().requires_grad_(True)
    b = sims.blochsim(M0, beff, T1=T1, **kw)           # the reference's own contract: T1.grad stays None
    b.sum().backward()
    assert T1.grad is None and M0.grad is not None
    with torch.no_grad():                              # nothing to differentiate: the plain kernels
        a = slowsims.blochsim(sp['M0'], beff, T1=T1, **kw)
    assert torch.equal(a, b.detach())


@pytest.mark.parametrize('mode', ['precise', 'fast'])
@pytest.mark.parametrize('nM', [64 * 8 * 3, 64 * 13 + 5, 64 * 7])
def test_k1_xcd_tile_order_is_the_same_arithmetic(mode, nM):
    r"""The history-saving K1 walks the spin tiles in XCD-contiguous order (block b -> tile (b % 8) * per_xcd + b / 8,
    grid padded to a multiple of 8), the no-history K1 in plain order (round 4, second half: K0's `sc1 nt` stores made
    the XCD-contiguous order of the no-history kernel unnecessary; DESIGN.md §3 "K1 right behind K0").  Every row must
    be integrated exactly once and exactly as on its own in both -- tile counts that are multiples of 8, not
    multiples of 8 (blocks past the last tile exit), and fewer than 8."""
    n, nT = 16, 64                                             # nT % 32 == 0: the line-granular kernel
    idx = torch.arange(nM)
    sp, p, kw = _problem(n, nT, idx=idx)
    with mrphy_amd.precision(mode), torch.no_grad():
        beff = beffective.rfgr2beff(p['rf'], p['gr'], sp['loc'], Δf=sp['Δf'], γ=sp['γ'])
        Mo = sims.blochsim(sp['M0'], beff, **kw)
        # the same rows alone (one tile each time: no tile order to speak of), and the fused kernel
        for lo in (0, 64 * 5, nM - 64):
            sl = slice(lo, lo + 64)
            part = sims.blochsim(sp['M0'][:, sl].contiguous(), beff[:, sl].contiguous(),
                                 T1=sp['T1'][:, sl], T2=sp['T2'][:, sl], γ=sp['γ'], dt=p['dt'])
            assert torch.equal(part, Mo[:, sl])
        from mrphy_amd import fused
        Mf = fused.blochsim_rfgr(sp['M0'], p['rf'], p['gr'], sp['loc'], Δf=sp['Δf'], γ_beff=sp['γ'], **kw)
        assert torch.equal(Mf, Mo)
    with mrphy_amd.precision(mode):
        Mh = sims.blochsim(sp['M0'].clone().requires_grad_(True), beff, **kw)       # history-saving twin
    assert torch.equal(Mh.detach(), Mo)


# (kind, relax, N, nM): every data type and step, with and without relaxation, at a ragged last tile, full tiles, a
# last tile of three rows (the mover's off0 / olim clamp for rows past the end, and the skipped stores), one ragged
# tile in a grid padded to 8 blocks (7 blocks leave at the top); and a batch of two with a tile across the batch
# boundary, where the row prologue's (n, s) split meets per-spin T1 / T2.
_LINE_CASES = [(kind, relax, 1, nM) for kind in ('f64', 'precise', 'fast') for relax in (True, False)
               for nM in (64 * 9 + 7, 64 * 8, 64 + 3, 5)] + [(kind, True, 2, 70) for kind in ('f64', 'precise', 'fast')]


@pytest.mark.parametrize('kind,relax,N,nM', _LINE_CASES, ids=lambda v: str(v))
def test_line_kernels_equal_the_chunked_ones(kind, relax, N, nM):
    r"""``blochsim`` (forward, forward with history, adjoint) runs line-granular kernels when the rows sit on 128-B
    lines and nT is whole periods (a line = 16 doubles / 32 floats, period 3 lines = 16 / 32 steps); the same values
    at an address off the 128-B grid run the chunked kernels.  Same step arithmetic: outputs and gradients bit for
    bit, in fp64 (round 4) and in fp32 with the precise and the fast step -- several periods, carries across all three
    piece boundaries.  The line kernels share one Beff mover and all kernels one row prologue (k_lines.hpp,
    k_common.hpp): the row counts are the mover's and the prologue's edge cases.  A backward in which Beff needs no
    gradient (the mover stores nothing) gives grad_Mi the same bits."""
    dtype = torch.float64 if kind == 'f64' else torch.float32
    nT = 80 if kind == 'f64' else 96                          # 5 / 3 periods
    sp, p, kw = _problem(16, nT, dtype=dtype, idx=torch.arange(N * nM))
    beff = beffective.rfgr2beff(p['rf'] * 40, p['gr'] * 3, sp['loc'], Δf=sp['Δf'], γ=sp['γ'])   # some steps beyond pi
    beff = beff.reshape(N, nM, nT, 3)
    M0 = sp['M0'].reshape(N, nM, 3)
    kw = dict(kw, T1=kw['T1'].reshape(N, nM), T2=kw['T2'].reshape(N, nM))
    if not relax:
        kw = dict(γ=kw['γ'], dt=kw['dt'])
    assert beff.data_ptr() % 128 == 0 and beff.is_contiguous()
    res = []
    with mrphy_amd.precision('fast' if kind == 'fast' else 'precise'):
        for b in (beff, _offset_copy(beff)):
            b = b.detach().requires_grad_(True)
            Mi = M0.clone().requires_grad_(True)
            with torch.no_grad():
                Mo_ng = sims.blochsim(Mi, b, **kw)            # no history
            Mo = sims.blochsim(Mi, b, **kw)                   # with history
            gMo = torch.cos(Mo.detach() * 3.0)
            gM, gB = torch.autograd.grad(Mo, (Mi, b), gMo)
            Mo2 = sims.blochsim(Mi, b.detach(), **kw)         # Beff needs no gradient: nothing is stored
            gM2, = torch.autograd.grad(Mo2, (Mi,), gMo)
            res.append((Mo_ng, Mo.detach(), gM, gB, gM2))
    names = ('Mo', 'Mo_hist', 'grad_Mi', 'grad_Beff', 'grad_Mi_alone')
    dist = {n_: float((a_.double() - b_.double()).abs().max()) for n_, a_, b_ in zip(names, *res)}
    print(f'line vs chunked kernels, max |difference| {kind} relax={relax} N={N} nM={nM}: {dist}')
    for n_, a_, b_ in zip(names, *res):
        assert torch.equal(a_, b_), (n_, dist)
    for r_ in res:
        assert torch.equal(r_[0], r_[1])                      # with history: the same output
        assert torch.equal(r_[2], r_[4])                      # ... and grad_Mi whether or not grad_Beff is wanted


def test_blochsim_constant_gradients_with_a_gamma_zero_spin():
    r"""a spin with γ2πdt == 0 used to put 0/0 into the γ / dt gradient of ``slowsims.blochsim``; the
    adjoint now accumulates dL/db . B directly (no division)."""
    import bloch_oracle as O
    from mrphy_amd import slowsims
    g = torch.Generator(device='cpu').manual_seed(13)
    f64 = torch.float64
    N, nM, nT = 1, 66, 16
    M = torch.rand((N, nM, 3), generator=g, dtype=f64)
    beff = torch.randn((N, nM, nT, 3), generator=g, dtype=f64) * 0.3
    γ = torch.full((N, nM), 4257.6, dtype=f64); γ[0, 5] = 0.0
    ops = dict(T1=torch.rand((N, nM), generator=g, dtype=f64) + 0.5, T2=torch.rand((N, nM), generator=g, dtype=f64) * 0.1 + 0.03,
               γ=γ, dt=torch.tensor([4e-6], dtype=f64))
    ref = _leafs(ops, ('T1', 'T2', 'γ', 'dt'), f64)
    O.blochsim_slow(M, beff, **ref).sum().backward()
    got = _leafs({k: v.to(DEV) for k, v in ops.items()}, ('T1', 'T2', 'γ', 'dt'), f64)
    slowsims.blochsim(M.to(DEV), beff.to(DEV), **got).sum().backward()
    for k in ('T1', 'T2', 'γ', 'dt'):
        assert bool(torch.isfinite(got[k].grad).all()), k
        assert float((got[k].grad.cpu() - ref[k].grad).abs().max()) <= 1e-9 * max(1.0, float(ref[k].grad.abs().max())), k


def test_underflowed_relaxation_is_refused_by_the_precise_adjoint():
    r"""with ``E2 == 0`` (T2 < dt/100 in fp32) the precise adjoint would divide 0 by 0.  The host says so
    (once per constants: the check is cached) -- for the materialised and the fused route; the fast step and the
    forward alone are unaffected.  ADVICE r4: it says so in ``backward``, where the division is; the forward of a
    graph-building call succeeds, as the reference's does."""
    from mrphy_amd import fused
    sp, p, kw = _problem(6, 32)
    kw = dict(kw, T2=torch.full_like(sp['T2'], 1e-9))
    beff = beffective.rfgr2beff(p['rf'], p['gr'], sp['loc'], Δf=sp['Δf'], γ=sp['γ'])
    with torch.no_grad():
        want = sims.blochsim(sp['M0'], beff, **kw)
        assert bool(torch.isfinite(want).all())
    Mi = sp['M0'].clone().requires_grad_(True)
    Mo = sims.blochsim(Mi, beff, **kw)                          # the forward succeeds (round 4 raised here) ...
    assert torch.equal(Mo.detach(), want)
    with pytest.raises(RuntimeError, match='exactly 0'):        # ... the adjoint refuses
        Mo.sum().backward()
    rf = p['rf'].clone().requires_grad_(True)
    Mf = fused.blochsim_rfgr(sp['M0'], rf, p['gr'], sp['loc'], Δf=sp['Δf'], γ_beff=sp['γ'], **kw)
    assert torch.equal(Mf.detach(), want)
    with pytest.raises(RuntimeError, match='exactly 0'):
        Mf.sum().backward()
    with mrphy_amd.precision('fast'):
        sims.blochsim(Mi, beff, **kw).sum().backward()
    assert bool(torch.isfinite(Mi.grad).all())


def test_fuzz_forward_fp32_vs_fp64_oracle():
    r"""60 random fp32 problems (the shapes of test_fuzz_forward_vs_c_restatement: batch 1-3, 1-200 spins, pulse lengths on and
    off the line grid up to 192 steps, 1-9 coils, with and without b1Map / Δf / relaxation): rfgr2beff + blochsim and the fused
    kernel agree bit for bit, and both are within the north star's 1e-5 (relative L2) of oracle/bloch_c.c run in fp64 on the same
    fp32 inputs -- field formed in fp64 too, so the bound includes the rounding of Beff to fp32."""
    import bloch_c as C
    from mrphy_amd import fused
    g = torch.Generator().manual_seed(int(os.environ.get('MRPHY_FUZZ_SEED', 20261005)))
    rnd = lambda *s: torch.rand(s, generator=g, dtype=torch.float64).float()  # noqa: E731
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))  # noqa: E731
    worst = 0.0
    for case in range(int(os.environ.get('MRPHY_FUZZ_CASES', 60))):
        N, nM = ri(1, 3), ri(1, 200)
        nT = (ri(1, 70), 32 * ri(1, 6), 16 * ri(1, 5))[ri(0, 2)]
        nC = (1, 1, 2, 5, 8, 9)[ri(0, 5)]
        Np = N if ri(0, 1) else 1
        has_b1 = bool(ri(0, 3))
        rf = ((rnd(Np, 2, nT, nC) if (nC > 1 or ri(0, 1)) else rnd(Np, 2, nT)) * 2 - 1) * 0.3
        gr = (rnd(Np, 3, nT) * 2 - 1) * 2
        loc = (rnd(N, nM, 3) * 2 - 1) * 8
        b1 = None
        if has_b1:
            b1 = (rnd(N, nM, 2, nC) * 2 - 1) if rf.ndim == 4 else (rnd(N, nM, 2) * 2 - 1)
        df = ((rnd(N, nM) * 2 - 1) * 300) if ri(0, 1) else None
        relax = bool(ri(0, 2))
        T1, T2 = 0.3 + rnd(N, nM), 0.01 + 0.1 * rnd(N, nM)
        γ, dt = torch.tensor(4257.6, dtype=torch.float32), torch.tensor([4e-6], dtype=torch.float32)
        M0 = rnd(N, nM, 3) * 2 - 1
        kw = dict(T1=T1, T2=T2) if relax else {}
        up = lambda x: None if x is None else x.double()  # noqa: E731
        want = C.blochsim_rfgr(up(M0), up(rf), up(gr), up(loc), Δf=up(df), b1Map=up(b1), γ_beff=up(γ), γ=up(γ), dt=up(dt),
                               **{k_: v.double() for k_, v in kw.items()})
        d = lambda x: None if x is None else x.to(DEV)  # noqa: E731
        kwd = {k_: v.to(DEV) for k_, v in kw.items()}
        beff = beffective.rfgr2beff(d(rf), d(gr), d(loc), Δf=d(df), b1Map=d(b1), γ=d(γ))
        two = sims.blochsim(d(M0), beff, γ=d(γ), dt=d(dt), **kwd)
        fu = fused.blochsim_rfgr(d(M0), d(rf), d(gr), d(loc), Δf=d(df), b1Map=d(b1), γ_beff=d(γ), γ=d(γ), dt=d(dt), **kwd)
        tag = f'case {case}: N={N} nM={nM} nT={nT} nC={nC} Np={Np} b1={has_b1} df={df is not None} relax={relax} rf.ndim={rf.ndim}'
        assert torch.equal(two, fu), tag
        rel = float((two.double().cpu() - want).norm() / want.norm())
        worst = max(worst, rel)
        assert rel <= 1e-5, tag + f' rel-L2 {rel:.3e}'
    print(f'fp32 fuzz: worst relative L2 {worst:.3e}')


def test_fuzz_gradients_fp32_vs_fp64_oracle():
    r"""30 random fp32 problems: gradients of a weighted sum of Mo w.r.t. Mi, rf, gr through rfgr2beff + blochsim and through the
    fused route against the torch oracle's autograd run in fp64 on the same fp32 inputs: relative L2 <= 3e-5 per gradient (the
    forward bound is 1e-5; a gradient sums nT x nM rounded contributions), the two routes' grad_Mi bit-identical when the fused
    adjoint runs (nT % 16 == 0, <= 8 coils)."""
    import bloch_oracle as O
    from mrphy_amd import fused
    g = torch.Generator().manual_seed(int(os.environ.get('MRPHY_FUZZ_SEED', 515151)))
    rnd = lambda *s: torch.rand(s, generator=g, dtype=torch.float64).float()  # noqa: E731
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))  # noqa: E731
    worst = {}
    import random
    from mrphy_amd import _hist
    prng = random.Random(66)                                  # round 6: every case also draws a way to cut the history
    for case in range(int(os.environ.get('MRPHY_FUZZ_CASES', 30))):
        _hist.set_policy(parts=prng.choice((1, 2, 3, 4, 8)), layout=prng.choice((0, 1)), min_bytes=0, min_tiles_per_part=1)
        N, nM = ri(1, 2), ri(8, 150)
        nT = (16, 32, 48, 96, ri(1, 60))[ri(0, 4)]
        nC = (1, 1, 1, 3, 8, 9)[ri(0, 5)]
        Np = N if ri(0, 1) else 1
        has_b1 = nC > 1 or bool(ri(0, 1))
        rf = ((rnd(Np, 2, nT, nC) if (nC > 1 or ri(0, 1)) else rnd(Np, 2, nT)) * 2 - 1) * 0.3
        gr = (rnd(Np, 3, nT) * 2 - 1) * 2
        loc = (rnd(N, nM, 3) * 2 - 1) * 8
        b1 = ((rnd(N, nM, 2, nC) * 2 - 1) if rf.ndim == 4 else (rnd(N, nM, 2) * 2 - 1)) if has_b1 else None
        df = ((rnd(N, nM) * 2 - 1) * 300) if ri(0, 1) else None
        relax = bool(ri(0, 2))
        T1, T2 = 0.3 + rnd(N, nM), 0.01 + 0.1 * rnd(N, nM)
        γ, dt = torch.tensor(4257.6, dtype=torch.float32), torch.tensor([4e-6], dtype=torch.float32)
        M0, w = rnd(N, nM, 3) * 2 - 1, rnd(N, nM, 3) * 2 - 1
        kw = dict(T1=T1, T2=T2) if relax else {}

        def run(kind):
            on = (lambda x: None if x is None else x.double()) if kind == 'oracle' else (lambda x: None if x is None else x.to(DEV))
            Mi, r, q = (on(x).clone().requires_grad_(True) for x in (M0, rf, gr))
            kk = {k_: on(v) for k_, v in kw.items()}
            if kind == 'oracle':
                Mo = O.blochsim(Mi, O.rfgr2beff(r, q, on(loc), Δf=on(df), b1Map=on(b1), γ=on(γ)), γ=on(γ), dt=on(dt), **kk)
            elif kind == 'two':
                Mo = sims.blochsim(Mi, beffective.rfgr2beff(r, q, on(loc), Δf=on(df), b1Map=on(b1), γ=on(γ)), γ=on(γ), dt=on(dt), **kk)
            else:
                Mo = fused.blochsim_rfgr(Mi, r, q, on(loc), Δf=on(df), b1Map=on(b1), γ_beff=on(γ), γ=on(γ), dt=on(dt), **kk)
            (Mo * on(w)).sum().backward()
            return Mi.grad, r.grad, q.grad
        ora = run('oracle')
        got = {kind: run(kind) for kind in ('two', 'fused')}
        tag = f'case {case}: N={N} nM={nM} nT={nT} nC={nC} Np={Np} b1={has_b1} df={df is not None} relax={relax}'
        if nT % 16 == 0 and nC <= 8:
            assert torch.equal(got['two'][0], got['fused'][0]), tag
        for kind, gs in got.items():
            for a, b, nm in zip(gs, ora, ('gMi', 'grf', 'ggr')):
                rel = float((a.double().cpu() - b).norm() / b.norm().clamp_min(1e-30))
                worst[nm] = max(worst.get(nm, 0.0), rel)
                assert a.shape == b.shape and rel <= 3e-5, f'{tag} {kind} {nm} rel-L2 {rel:.2e}'
    print('fp32 gradient fuzz: worst relative L2', {k_: f'{v:.2e}' for k_, v in worst.items()})


# ---------------------------------------------------------------------------------------------
# round 6: the history in separately allocated parts (ABI 5: mrphy_blochsim_fwd_parts / _bwd_parts)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,mode', [('f32', 'precise'), ('f32', 'fast'), ('f64', 'precise')])
@pytest.mark.parametrize('nM,nT', [(64 * 19 + 5, 64), (64 * 16, 96), (64 * 9 + 63, 48), (64 * 8, 35), (70, 7)])
def test_history_in_parts_is_the_same_arithmetic(tag, mode, nM, nT):
    r"""However the history (``sims.py:84-88``) is cut -- 1, 2, 3, 8 parts, tiles dealt in blocks or round-robin -- ``Mo``,
    ``grad_Mi``, ``grad_Beff`` and the constants' gradients are the one-part route's bit for bit: line-granular kernels
    (nT % 32 == 0 in fp32, % 16 in fp64), chunked kernels and their tails, ragged last tiles, fewer tiles than parts."""
    from mrphy_amd import _hist
    dtype = DT[tag]
    g = torch.Generator().manual_seed(nM * 131 + nT)
    Mi = torch.rand((1, nM, 3), generator=g, dtype=dtype).to(DEV)
    Beff = ((torch.rand((1, nM, nT, 3), generator=g, dtype=dtype) - 0.5) * 3).to(DEV)
    T1 = (0.5 + torch.rand((1, nM), generator=g, dtype=dtype)).to(DEV)
    T2 = (0.05 + 0.1 * torch.rand((1, nM), generator=g, dtype=dtype)).to(DEV)
    gMo = torch.rand((1, nM, 3), generator=g, dtype=dtype).to(DEV)
    old = dict(_hist.policy)

    def run(parts, layout, consts=False):
        _hist.set_policy(parts=parts, layout=layout, min_bytes=0)
        m, b = Mi.clone().requires_grad_(True), Beff.clone().requires_grad_(True)
        t1 = T1.clone().requires_grad_(consts)
        with mrphy_amd.precision(mode):
            if consts:
                Mo = slowsims.blochsim(m, b, T1=t1, T2=T2, γ=mrphy_amd.γH.to(DEV, dtype), dt=mrphy_amd.dt0.to(DEV, dtype))
            else:
                Mo = sims.blochsim(m, b, T1=t1, T2=T2)
            Mo.backward(gMo)
        return (Mo.detach(), m.grad, b.grad) + ((t1.grad,) if consts else ())

    try:
        want = run(1, _hist.BLOCKED)
        want_c = run(1, _hist.BLOCKED, consts=True)
        for parts in (2, 3, 8):
            for layout in (_hist.BLOCKED, _hist.INTERLEAVED):
                got = run(parts, layout)
                assert all(torch.equal(a, b) for a, b in zip(got, want)), (parts, layout)
        got_c = run(3, _hist.INTERLEAVED, consts=True)
        assert all(torch.equal(a, b) for a, b in zip(got_c, want_c))
    finally:
        _hist.policy.update(old)


def test_history_parts_allocation_and_second_backward():
    r"""The allocator's route draws the policy's number of parts, each an allocation of its own; a second backward
    (``retain_graph``) reads the same history and returns a fresh ``grad_Beff`` with the same bits -- never the storage an
    earlier backward returned (the reference overwrites its saved ``γBeff``, ``sims.py:239-264``; not replicated).  Below
    the policy's size threshold, or with fewer than eight tiles per part, the history is one part."""
    from mrphy_amd import _hist
    sp, p, kw = _problem(16, 64)
    nM = 16 ** 3
    code = mrphy_amd._lib.F32P
    old = dict(_hist.policy)
    try:
        assert _hist.policy['parts'] == 4 and _hist.n_parts_for(code, 1, nM, 64) == 1        # 3 MB: not worth cutting
        assert _hist.n_parts_for(code, 1, 64 ** 3, 2048) == 4
        _hist.set_policy(parts=2, min_bytes=0)
        assert _hist.n_parts_for(code, 1, nM, 64) == 2 and _hist.n_parts_for(code, 1, 64 * 15, 64) == 1
        h = _hist.allocate(code, 1, nM, 64, torch.float32, DEV)
        lib = mrphy_amd.require_library()
        assert len(h.parts) == 2
        assert all(q.numel() * 4 == lib.mrphy_blochsim_hist_part_bytes(code, 1, nM, 64, 2) for q in h.parts)
        assert h.parts[0].untyped_storage().data_ptr() != h.parts[1].untyped_storage().data_ptr()
        beff = beffective.rfgr2beff(p['rf'], p['gr'], sp['loc'], Δf=sp['Δf'], γ=sp['γ']).requires_grad_(True)
        Mo = sims.blochsim(sp['M0'], beff, **kw)
        (g1,) = torch.autograd.grad(Mo.sum(), beff, retain_graph=True)
        (g2,) = torch.autograd.grad(Mo.sum(), beff)
        assert g1.data_ptr() != g2.data_ptr() and torch.equal(g1, g2)
        _hist.set_policy(parts=1)
        (g3,) = torch.autograd.grad(sims.blochsim(sp['M0'], beff, **kw).sum(), beff)
        assert torch.equal(g1, g3)
        with pytest.raises(ValueError):
            _hist.set_policy(parts=9)
    finally:
        _hist.policy.update(old)


# ---------------------------------------------------------------------------------------------
# round 5: the gradient route's placement-probed workspace
# ---------------------------------------------------------------------------------------------
def test_grad_workspace_same_bits_guard_and_context():
    r"""``sims.blochsim(..., workspace=ws)`` / ``with ws:`` / ``rfgr2beff(..., out=ws.beff)``: history and ``grad_Beff`` are the
    workspace's blocks (pointers checked), results and gradients are the allocator route's bit for bit, iteration after
    iteration through the same blocks; a backward whose history a later forward has overwritten raises; wrong shapes
    are refused.  (Blocks this small are not probed: the draw is exercised by ``test_grad_workspace_probes_candidates``.)"""
    sp, p, kw = _problem(12, 64)
    nM = 12 ** 3

    def grads(ws, use_ctx=False):
        rf, gr = p['rf'].clone().requires_grad_(True), p['gr'].clone().requires_grad_(True)
        M0 = sp['M0'].clone().requires_grad_(True)
        beff = beffective.rfgr2beff(rf, gr, sp['loc'], Δf=sp['Δf'], γ=sp['γ'], out=None if ws is None else ws.beff)
        if use_ctx:
            with ws:
                assert workspace.active() is ws
                Mo = sims.blochsim(M0, beff, **kw)
            assert workspace.active() is None
        else:
            Mo = sims.blochsim(M0, beff, workspace=ws, **kw)
        Mo.sum().backward()
        return Mo.detach().clone(), rf.grad.clone(), gr.grad.clone(), M0.grad.clone()

    want = grads(None)
    ws = workspace.GradWorkspace((1, nM, 64, 3), torch.float32, DEV)
    assert ws.report['probed'] is False and tuple(ws.beff.shape) == (1, nM, 64, 3)
    for it in range(3):                                          # the same blocks, iteration after iteration
        got = grads(ws, use_ctx=it == 2)
        assert all(torch.equal(a, b) for a, b in zip(got, want)), it
    assert ws.generation == 3
    # grad_Beff of a leaf Beff IS the workspace's block
    beff = beffective.rfgr2beff(p['rf'], p['gr'], sp['loc'], Δf=sp['Δf'], γ=sp['γ']).requires_grad_(True)
    Mo = sims.blochsim(sp['M0'], beff, workspace=ws, **kw)
    (g,) = torch.autograd.grad(Mo.sum(), beff)
    assert g.data_ptr() == ws._grad.data_ptr()
    ref = torch.autograd.grad(sims.blochsim(sp['M0'], beff, **kw).sum(), beff)[0]
    assert torch.equal(g, ref)
    # one forward / backward pair in flight: the first forward's history is gone after the second forward
    Mo1 = sims.blochsim(sp['M0'], beff, workspace=ws, **kw)
    Mo2 = sims.blochsim(sp['M0'], beff, workspace=ws, **kw)
    with pytest.raises(RuntimeError, match='overwritten by a later'):
        Mo1.sum().backward()
    Mo2.sum().backward()                                         # the latest one is fine
    # under no_grad nothing is drawn
    gen = ws.generation
    with torch.no_grad():
        assert torch.equal(sims.blochsim(sp['M0'], beff, workspace=ws, **kw), Mo2.detach())
    assert ws.generation == gen
    # a workspace built for another shape / dtype refuses
    small = workspace.GradWorkspace((1, 64, 8, 3), torch.float32, DEV, with_beff=False)
    assert small.beff is None
    with pytest.raises(RuntimeError, match='GradWorkspace built for'):
        sims.blochsim(sp['M0'], beff, workspace=small, **kw)
    with pytest.raises(RuntimeError, match='GradWorkspace built for'):
        sims.blochsim(sp['M0'].double(), beff.detach().double().requires_grad_(True), workspace=ws, **kw)


def test_grad_workspace_probes_candidates():
    r"""Blocks above the probing threshold (64 MiB): the history is drawn in parts as ``sims.blochsim`` does by itself,
    candidates are drawn and timed with the library's own K1h / K3 within the caps (count, bytes alive, seconds),
    ``grad_Beff`` gets the fastest candidate for K3, the history stays in its parts unless a single block is clearly
    faster; the others go back to the driver (reserved memory is about three blocks afterwards: history, grad_Beff,
    Beff), and the route through it gives the allocator route's bits."""
    n, nT = 32, 256                                              # Beff = 100.7 MB
    sp, p, kw = _problem(n, nT)
    shape = (1, n ** 3, nT, 3)
    torch.cuda.empty_cache()
    before = torch.cuda.memory_reserved()
    ws = workspace.GradWorkspace(shape, torch.float32, DEV, candidates=5)
    rep = ws.report
    assert rep['probed'] and 2 <= len(rep['K3_ms']) == len(rep['K1h_ms']) - 1 == rep['candidates_drawn'] <= 5
    assert len(set(rep['ptr'])) == len(rep['ptr']) and rep['candidates_cap'] == 5
    h, g = rep['chosen']['hist'], rep['chosen']['grad']
    assert ws._grad.data_ptr() == int(rep['ptr'][g], 16) and rep['K3_ms'][g] == min(rep['K3_ms'])
    if h == 'parts':
        assert len(ws._hist.parts) == rep['hist_parts']
    else:
        assert h != g and ws._hist.parts[0].data_ptr() == int(rep['ptr'][h], 16) and rep['K1h_ms'][h + 1] < 0.96 * rep['K1h_ms'][0]
    assert rep['stopped'] in ('a block of the fast kind found for each kernel', 'candidates used up', 'time used up')
    # (the timed launches only: getting blocks from the driver can take seconds in a process that has just freed 100 GB,
    # as this one has after the headline test -- `seconds['allocate']`, not bounded here)
    assert 0 < rep['seconds']['probe'] < 10 and rep['probe_seconds'] >= rep['seconds']['probe']
    assert rep['peak_bytes'] <= 7 * rep['bytes_per_block']
    grown = torch.cuda.memory_reserved() - before
    assert grown <= 3 * rep['bytes_per_block'] + (64 << 20), (grown, rep['bytes_per_block'])     # the losers were released
    rf, gr = p['rf'].clone().requires_grad_(True), p['gr'].clone().requires_grad_(True)
    sims.blochsim(sp['M0'], beffective.rfgr2beff(rf, gr, sp['loc'], Δf=sp['Δf'], γ=sp['γ'], out=ws.beff),
                  workspace=ws, **kw).sum().backward()
    rf2, gr2 = p['rf'].clone().requires_grad_(True), p['gr'].clone().requires_grad_(True)
    sims.blochsim(sp['M0'], beffective.rfgr2beff(rf2, gr2, sp['loc'], Δf=sp['Δf'], γ=sp['γ']), **kw).sum().backward()
    assert torch.equal(rf.grad, rf2.grad) and torch.equal(gr.grad, gr2.grad)
    # the caps: bytes alive and time
    tight = workspace.GradWorkspace(shape, torch.float32, DEV, candidates=8, probe_bytes=2 * rep['bytes_per_block'],
                                    with_beff=False)
    assert tight.report['candidates_cap'] == 2 and tight.report['candidates_drawn'] <= 2
    hurried = workspace.GradWorkspace(shape, torch.float32, DEV, candidates=8, probe_seconds=0.0, with_beff=False)
    assert hurried.report['candidates_drawn'] == 1 and hurried.report['stopped'] == 'time used up'
    none = workspace.GradWorkspace(shape, torch.float32, DEV, candidates=1, with_beff=False)
    assert none.report['probed'] is False and none._field is None


def test_grad_workspace_context_falls_back_and_stale_blocks_raise():
    r"""(i) inside ``with ws:`` a call the workspace does not fit (another dtype, a longer pulse) uses the
    allocator instead of raising -- only an explicit ``workspace=`` that does not fit raises; a workspace built on one
    device refuses tensors of another; (ii) ``rfgr2beff(..., out=block)`` bumps the block's version counter, so the
    backward of an EARLIER graph that saved the block's previous contents raises instead of silently differentiating
    the wrong field; (iii) fewer spins with more steps can need longer history parts than the workspace holds although
    the total is smaller: refused, not overrun."""
    sp, p, kw = _problem(12, 64)
    nM = 12 ** 3
    ws = workspace.GradWorkspace((1, nM, 64, 3), torch.float32, DEV)
    beff = beffective.rfgr2beff(p['rf'], p['gr'], sp['loc'], Δf=sp['Δf'], γ=sp['γ']).requires_grad_(True)
    with ws:
        assert workspace.active(beff.shape, torch.float32, DEV) is ws
        assert workspace.active(beff.shape, torch.float64, DEV) is None
        assert workspace.active((1, nM, 128, 3), torch.float32, DEV) is None
        gen = ws.generation
        kw64 = {k: v.double() for k, v in kw.items()}
        Mo = sims.blochsim(sp['M0'].double(), beff.detach().double().requires_grad_(True), **kw64)      # the allocator's
        Mo.sum().backward()
        assert ws.generation == gen
        sims.blochsim(sp['M0'], beff, **kw).sum().backward()
        assert ws.generation == gen + 1
    with pytest.raises(RuntimeError, match='GradWorkspace built on'):
        ws.take_hist(16, torch.float32, torch.device('cuda', 1))
    # (iii) 9 tiles x 200 steps < 32 tiles x 64 steps in total, but ceil(9 / 4) tiles x 200 steps per part is more than 8 x 64
    from mrphy_amd import _hist
    old = dict(_hist.policy)
    try:
        _hist.set_policy(parts=4, min_bytes=0)
        ws4 = workspace.GradWorkspace((1, 64 * 32, 64, 3), torch.float32, DEV, with_beff=False)
        assert len(ws4._hist.parts) == 4 and not ws4.fits((1, 64 * 9, 200, 3), torch.float32, DEV)
        assert ws4.fits((1, 64 * 30, 64, 3), torch.float32, DEV)
        b5 = torch.zeros((1, 64 * 9, 200, 3), device=DEV, requires_grad=True)
        with pytest.raises(RuntimeError, match='GradWorkspace built for'):
            sims.blochsim(torch.zeros((1, 64 * 9, 3), device=DEV), b5, workspace=ws4)
    finally:
        _hist.policy.update(old)
    # (ii) a stale saved Beff
    ws = workspace.GradWorkspace((1, nM, 64, 3), torch.float32, DEV)
    rf1, rf2 = p['rf'].clone().requires_grad_(True), (2 * p['rf']).requires_grad_(True)
    b1 = beffective.rfgr2beff(rf1, p['gr'], sp['loc'], Δf=sp['Δf'], γ=sp['γ'], out=ws.beff)
    Mo1 = sims.blochsim(sp['M0'], b1, **kw)                      # saves the block's contents (allocator's history)
    b2 = beffective.rfgr2beff(rf2, p['gr'], sp['loc'], Δf=sp['Δf'], γ=sp['γ'], out=ws.beff)       # ... and rewrites them
    with pytest.raises(RuntimeError, match='modified by an inplace operation'):
        Mo1.sum().backward()
    sims.blochsim(sp['M0'], b2, **kw).sum().backward()           # the latest graph is fine
    want = p['rf'].clone().requires_grad_(True)
    sims.blochsim(sp['M0'], beffective.rfgr2beff(2 * want, p['gr'], sp['loc'], Δf=sp['Δf'], γ=sp['γ']), **kw).sum().backward()
    assert torch.equal(2 * rf2.grad, want.grad)


def test_install_router_sends_device_tensors_to_the_kernels():
    r"""``install()`` into a stand-in ``mrphy`` whose own functions are tripwires: with device tensors every routed
    function runs the HIP path (equal to calling ``mrphy_amd`` directly) and the saved reference callable is never
    reached; with CPU tensors it is the saved callable that runs.  The real reference is routed
    in the build container (``tests/test_abi_and_host.py::test_install_routes_the_reference_object_layer``)."""
    calls = []

    def ref(name):
        def f(*a, **k):
            calls.append(name)
            return name
        f.__module__ = 'mrphy.stand_in'
        return f
    cls = lambda **m: type('C', (), m)  # noqa: E731
    fake = types.SimpleNamespace(
        beffective=types.SimpleNamespace(rfgr2beff=ref('rfgr2beff'), beff2ab=ref('beff2ab')),
        sims=types.SimpleNamespace(blochsim=ref('blochsim'), freeprec=ref('freeprec')),
        slowsims=types.SimpleNamespace(blochsim_1step=ref('blochsim_1step'), blochsim_ab=ref('blochsim_ab')),
        mobjs=types.SimpleNamespace(SpinArray=cls(extract=ref('extract'), embed=ref('embed'), applypulse=ref('applypulse')),
                                    SpinCube=cls(_update_loc_=ref('_update_loc_')), Pulse=cls(interpT=ref('interpT'))))
    sp, p, kw = _problem(6, 32)
    mrphy_amd.install(fake)
    try:
        beff = fake.beffective.rfgr2beff(p['rf'], p['gr'], sp['loc'], Δf=sp['Δf'], γ=sp['γ'])
        assert torch.equal(beff, beffective.rfgr2beff(p['rf'], p['gr'], sp['loc'], Δf=sp['Δf'], γ=sp['γ']))
        Mo = fake.sims.blochsim(sp['M0'], beff, **kw)
        assert torch.equal(Mo, sims.blochsim(sp['M0'], beff, **kw))
        dur = torch.tensor(1e-3, device=DEV)
        assert torch.equal(fake.sims.freeprec(Mo, dur, T1=sp['T1'], T2=sp['T2'], Δf=sp['Δf']),
                           sims.freeprec(Mo, dur, T1=sp['T1'], T2=sp['T2'], Δf=sp['Δf']))
        E = torch.full((1, 6 ** 3), 0.999, device=DEV)
        A, B = fake.beffective.beff2ab(beff, E1=E, E2=E * 0.99, γ=sp['γ'], dt=p['dt'])
        assert torch.equal(fake.slowsims.blochsim_ab(sp['M0'], A, B), slowsims.blochsim_ab(sp['M0'], A, B))
        assert calls == []                                       # no device call reached the "reference"
        # mixed devices: one device tensor is enough to stay on the HIP path (which then refuses the CPU one loudly)
        with pytest.raises((RuntimeError, AssertionError)):
            fake.sims.blochsim(sp['M0'].cpu(), beff, **kw)
        assert calls == []
        # all-CPU calls: the saved reference callables, untouched arguments
        c = lambda x: x.cpu()  # noqa: E731
        assert fake.sims.blochsim(c(sp['M0']), c(beff), T1=c(sp['T1']), T2=c(sp['T2'])) == 'blochsim'
        assert fake.beffective.rfgr2beff(c(p['rf']), c(p['gr']), c(sp['loc'])) == 'rfgr2beff'
        assert fake.sims.freeprec(c(Mo), torch.tensor(1e-3)) == 'freeprec'
        assert calls == ['blochsim', 'rfgr2beff', 'freeprec']
    finally:
        mrphy_amd.uninstall(fake)
    assert fake.sims.blochsim(1) == 'blochsim' and not mrphy_amd._saved


def test_auto_workspace_pool_serves_each_shape():
    r"""``with workspace.auto():`` -- the reference-signature calls get a workspace per ``Beff`` shape, built at first use
    and reused; same bits as without; nothing is built for calls that need no gradient."""
    sp, p, kw = _problem(8, 32)

    def grads():
        rf = p['rf'].clone().requires_grad_(True)
        beff = beffective.rfgr2beff(rf, p['gr'], sp['loc'], Δf=sp['Δf'], γ=sp['γ'])
        sims.blochsim(sp['M0'], beff, **kw).sum().backward()
        return rf.grad
    want = grads()
    pool = workspace.auto(candidates=3)
    with pool:
        with torch.no_grad():
            sims.blochsim(sp['M0'], beffective.rfgr2beff(p['rf'], p['gr'], sp['loc'], Δf=sp['Δf'], γ=sp['γ']), **kw)
        assert pool.pool == {}                                  # no gradient wanted: nothing built
        a = grads()
        assert len(pool.pool) == 1
        (ws,) = pool.pool.values()
        b = grads()
        assert len(pool.pool) == 1 and ws.generation == 2 and ws.beff is None
    assert workspace.active() is None
    assert torch.equal(a, want) and torch.equal(b, want)


def test_grad_workspace_batched_general_shape():
    r"""``GradWorkspace`` for a batched, non-compact problem -- ``Beff`` `(N, *Nd, nT, xyz)` with N = 2, Nd = (5, 7) (70
    spins per batch entry: the last 64-spin tile of the history is ragged) -- through ``blochsim`` and ``blochsim_consts``."""
    g = torch.Generator(device='cpu').manual_seed(21)
    N, Nd, nT = 2, (5, 7), 32
    M0 = torch.rand((N,) + Nd + (3,), generator=g).to(DEV)
    beff0 = (torch.randn((N,) + Nd + (nT, 3), generator=g) * 0.5).to(DEV)
    T1, T2 = (torch.rand((N,) + Nd, generator=g) + 0.5).to(DEV), (torch.rand((1,) + Nd, generator=g) * 0.1 + 0.02).to(DEV)
    ws = workspace.GradWorkspace(beff0.shape, torch.float32, DEV)
    assert tuple(ws.beff.shape) == tuple(beff0.shape)

    def grads(w, fn):
        M = M0.clone().requires_grad_(True)
        b = beff0.clone().requires_grad_(True)
        fn(M, b, w).sum().backward()
        return M.grad, b.grad.clone()
    call = lambda M, b, w: sims.blochsim(M, b, T1=T1, T2=T2, workspace=w)  # noqa: E731
    a, b = grads(None, call), grads(ws, call)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    γ2πdt, E1, E2, E1_1 = sims.relax_constants(T1, T2, mrphy_amd.γH, mrphy_amd.dt0, beff0.ndim, DEV)
    callc = lambda M, b, w: sims.blochsim_consts(M, b, γ2πdt=γ2πdt, E1=E1, E1_1=E1_1, E2=E2, workspace=w)  # noqa: E731
    c, d = grads(None, callc), grads(ws, callc)
    assert torch.equal(c[0], d[0]) and torch.equal(c[1], d[1]) and torch.equal(a[0], c[0])


def test_install_grad_workspace_pool_behind_the_reference_signature():
    r"""``install(mrphy, grad_workspace=True)``: the routed ``mrphy.sims.blochsim`` -- the reference's own signature -- draws the
    history and ``grad_Beff`` of a gradient call from the installed pool (one workspace per ``Beff`` shape); same bits;
    an explicit ``workspace=`` or an enclosing ``with ws:`` takes precedence; ``uninstall`` drops the pool."""
    ref = lambda *a, **k: (_ for _ in ()).throw(AssertionError('reference reached'))  # noqa: E731
    cls = lambda **m: type('C', (), m)  # noqa: E731
    fake = types.SimpleNamespace(
        beffective=types.SimpleNamespace(rfgr2beff=ref, beff2ab=ref), sims=types.SimpleNamespace(blochsim=ref, freeprec=ref),
        slowsims=types.SimpleNamespace(blochsim_1step=ref, blochsim_ab=ref),
        mobjs=types.SimpleNamespace(SpinArray=cls(extract=ref, embed=ref, applypulse=ref), SpinCube=cls(_update_loc_=ref),
                                    Pulse=cls(interpT=ref)))
    sp, p, kw = _problem(8, 32)

    def grads(blochsim):
        rf = p['rf'].clone().requires_grad_(True)
        beff = beffective.rfgr2beff(rf, p['gr'], sp['loc'], Δf=sp['Δf'], γ=sp['γ'])
        blochsim(sp['M0'], beff, **kw).sum().backward()
        return rf.grad
    want = grads(sims.blochsim)
    mrphy_amd.install(fake, grad_workspace=True)
    try:
        pool = mrphy_amd._AUTO_WS
        assert isinstance(pool, workspace.auto) and pool.pool == {}
        assert torch.equal(grads(fake.sims.blochsim), want) and len(pool.pool) == 1
        (ws,) = pool.pool.values()
        assert torch.equal(grads(fake.sims.blochsim), want) and ws.generation == 2 and len(pool.pool) == 1
        mine = workspace.GradWorkspace((1, 8 ** 3, 32, 3), torch.float32, DEV, with_beff=False)
        with mine:                                               # an enclosing workspace takes precedence
            assert torch.equal(grads(fake.sims.blochsim), want)
        assert mine.generation == 1 and ws.generation == 2
        assert workspace.active() is None                        # nothing leaks out of the call
    finally:
        mrphy_amd.uninstall(fake)
    assert mrphy_amd._AUTO_WS is None
