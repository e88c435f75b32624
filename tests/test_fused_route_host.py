r"""The routing decision of ``fused._route`` without a GPU or the library: ``fused._decide_route`` is a pure function of
plain facts, and the rows below are the coverage that the docstrings of ``_route``, ``blochsim_rfgr`` and ``signal_rfgr``
document.  The GPU tests that count calls by name assert the same routes on the device."""
import pytest

from mrphy_amd.fused import _decide_route

SEG, PTX_MAX = 16, 8        # mrphy_blochsim_rfgr_ck_every(), mrphy_blochsim_rfgr_mc_max_coils()

# one transmit coil without a map, fp32, blochsim_rfgr's call, no gradient wanted
ONE = dict(seg=SEG, ptx_max=PTX_MAX, nC=1, one_coil=True, has_b1=False, f64=False, signal=False,
           pulse_grad=False, maps_grad=False, consts_grad=False, rx_grad=False)
PTX4 = dict(ONE, nC=4, one_coil=False, has_b1=True)         # 4-coil parallel transmit with its map
COILS9 = dict(ONE, nC=9, one_coil=False, has_b1=True)
SIGNAL = dict(ONE, signal=True)

FUSED_CKPT = ('fused', True, False, False)        # want_ckpt, maps_fused, γb_grad
FUSED_MAPS = ('fused', True, True, False)
FUSED_PLAIN = ('fused', False, False, False)
SPLIT48 = ('split', 48)
COMPOSED = ('composed', None)

# (what, facts, route at nT = 48, route at nT = 50 or None where the row does not say)
BY_LENGTH = [
    ('pulse gradient, one coil', dict(ONE, pulse_grad=True), FUSED_CKPT, SPLIT48),
    ('pulse gradient, 4 coils with a map', dict(PTX4, pulse_grad=True), FUSED_CKPT, SPLIT48),
    ('map gradient, one coil, not signal', dict(ONE, maps_grad=True), FUSED_MAPS, SPLIT48),
    ("constants' gradient in the signal call, one coil", dict(SIGNAL, consts_grad=True), FUSED_CKPT, None),
    ("constants' gradient, 4-coil pTx", dict(PTX4, consts_grad=True), COMPOSED, COMPOSED),
]

# (what, facts with nT, route)
FIXED = [
    ('pulse gradient, one coil, nT = 8', dict(ONE, pulse_grad=True, nT=8), COMPOSED),
    ('no gradient at all, 4 coils, nT = 48', dict(PTX4, nT=48), FUSED_PLAIN),
    ('no gradient at all, 4 coils, nT = 50', dict(PTX4, nT=50), FUSED_PLAIN),
    ('no gradient at all, 4 coils, nT = 8', dict(PTX4, nT=8), FUSED_PLAIN),
    ('pulse gradient, 9 coils fp32', dict(COILS9, pulse_grad=True, nT=48), COMPOSED),
    ('9 coils fp32, no gradient', dict(COILS9, nT=48), FUSED_PLAIN),
    ('fp64 with 9 coils, no gradient', dict(COILS9, f64=True, nT=48), COMPOSED),
    ('map gradient, one coil, nT = 8', dict(ONE, maps_grad=True, nT=8), COMPOSED),
    ('map gradient under 4-coil pTx', dict(PTX4, maps_grad=True, nT=48), COMPOSED),
    ('map gradient in the signal call', dict(SIGNAL, maps_grad=True, nT=48), COMPOSED),
    ("constants' and map gradients together in the signal call", dict(SIGNAL, consts_grad=True, maps_grad=True, nT=48),
     COMPOSED),
    ('rx gradient', dict(SIGNAL, rx_grad=True, nT=48), COMPOSED),
    ('signal with 4 transmit coils', dict(SIGNAL, nC=4, one_coil=False, has_b1=True, nT=48), COMPOSED),
]


@pytest.mark.parametrize('what, facts, at48, at50', BY_LENGTH, ids=[r[0] for r in BY_LENGTH])
def test_route_by_pulse_length(what, facts, at48, at50):
    assert _decide_route(nT=48, **facts) == at48
    if at50 is not None:
        assert _decide_route(nT=50, **facts) == at50


@pytest.mark.parametrize('what, facts, route', FIXED, ids=[r[0] for r in FIXED])
def test_route(what, facts, route):
    assert _decide_route(**facts) == route


def test_gamma_beff_gradient_travels_with_the_maps():
    r"""A ``γ_beff`` that requires grad where there is a ``Δf`` counts as a map gradient (``_route`` sets both facts),
    and the answer says that the Function gets ``γ_beff`` handed over."""
    assert _decide_route(nT=48, **dict(ONE, maps_grad=True, γb_grad=True)) == ('fused', True, True, True)
