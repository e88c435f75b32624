r"""What the adjoints of ``fused.ab_steadystate`` (Kssb), ``ab_train`` (Ktrb), ``train_signal`` (Ktrsb) and ``ab_sequence``
(Ksqb) branch on and their own test files never vary: WHICH gradients are asked for (every output of the four entry
points is a nullable pointer; Ksqb's workspace and second pass exist only with ``grad_A`` or ``grad_B``; Ktrsb takes two
nullable cotangents), the FORM of the cotangent (a natural-layout weight, ``.sum()``'s stride-0 ones, slices, a buffer
off the 16-byte grid, another dtype) and the FORM of the operands (permuted views, offset buffers, stride-0 expansions,
one broadcast form per operand, CPU tensors of another dtype, fp16 / bf16).

Shapes, problems, yardsticks and runs are the four files' own: ``N = 2, nM = 100, K = 7`` (a ragged 256-block, a ragged
second wave, two grid rows), ``test_ab_sequence.S7`` with its schedule (0, 2, 2, 0, 0, 2, 0), and for the signal
``K = S + 1`` (a second checkpoint segment of length 1) with 3 receive coils.

What is claimed.  A request, a cotangent form or an operand form that changes no number changes no bit: the kernels take
their nullable outputs as run-time null pointers of one code object, every output has lane-private accumulators, and the
host code makes every cotangent and operand contiguous in the data type before the launch -- so those comparisons are
``torch.equal`` against the all-leaves (or the dense, or the contiguous) run of the same numbers.  That run is itself
held to ``test_steadystate._gate`` (fp64 max abs 1e-9, fp32 relative L2 1e-6) against the files' fp64 torch yardsticks on
the CPU, once per family here (``test_one_leaf_at_a_time``), and so is every gradient whose loss the all-leaves run does
not have (a cotangent on one output of the signal) or that is a sum over shared entries in another order (an operand in
a broadcast form).  Every compared gradient is asserted to be non-zero unless the zero is the claim.  The distances
of the gated values go to the ledger as ``requests.<family>.<tag>.<case>.<name>``.
"""
import functools

import pytest

from gpu_common import *  # noqa: F401,F403
import test_ab_sequence as SQ
import test_ab_train as TR
import test_steadystate as SS
import test_train_signal as TS
from test_ab_rfgr import _counted
from test_ab_train import _same_bits
from test_steadystate import _gate

pytestmark = pytest.mark.gpu

TAGS = ['f64', 'f32']
HALF = {'f16': torch.float16, 'bf16': torch.bfloat16}
N, nM, K7, KS, NRX = 2, 100, 7, TS.S + 1, 3
FAMILIES = ('steady', 'train', 'signal', 'sequence')
TRANSIENT = ('train', 'signal', 'sequence')
FWD = dict(steady='mrphy_ab_steadystate_fwd', train=TR.FWD, signal=TS.FWD, sequence=SQ.FWD)
BWD = dict(steady='mrphy_ab_steadystate_bwd', train=TR.BWD, signal=TS.BWD, sequence=SQ.BWD)
WORKSPACE = 'mrphy_ab_sequence_bwd_workspace'
OPERANDS = dict(steady=('A', 'B') + SS.CONSTS, train=('A', 'B') + TR.OPS, signal=('A', 'B') + TR.OPS + ('rx',),
                sequence=('A', 'B') + SQ.OPS)
OUT = dict(steady=('Mss',), train=('Mt',), signal=('sig', 'Mlast'), sequence=('Mt',))
GS, GL = 3, 4                       # mrphy_train_signal_bwd(code, A, B, gs, gMl, ...): the two nullable cotangents


# ---------------------------------------------------------------------------------------------
# the four families behind one signature
# ---------------------------------------------------------------------------------------------
def _problem(fam, tag):
    r"""``(P, want, K)``: the family's own seeded problem on the CPU (for the signal with its receive map as ``P['rx']``),
    the fp64 yardstick of its all-leaves run, and the number of repetitions.  Cached by the files; never modified."""
    if fam == 'steady':
        return SS._kernel_problem(N, nM, tag) + (None,)
    if fam == 'train':
        return TR._kernel_problem(N, nM, K7, tag) + (K7,)
    if fam == 'sequence':
        return SQ._kernel_problem(SQ.S7, tag) + (K7,)
    P, _ = TR._kernel_problem(N, nM, KS, tag)
    return dict(P, rx=TS._rx(N, nM, NRX, tag)), TS._cached_yardstick(N, nM, KS, tag, NRX), KS


def _run(fam, P, K, **kw):
    r"""The family's own ``_run``: outputs and gradients on the device (``leaves=``, ``loss=``, ``over=`` as there)."""
    if fam == 'steady':
        return SS._run(P, **kw)
    if fam == 'train':
        return TR._run(P, K, **kw)
    if fam == 'sequence':
        return SQ._run(P, K, **kw)
    return TS._run(P, K, P['rx'], **kw)


@functools.lru_cache(maxsize=None)
def _base(fam, tag):
    r"""The all-leaves run on contiguous device tensors with the problem's own weights.  Computed once, never modified."""
    P, _, K = _problem(fam, tag)
    return _run(fam, P, K)


def _call(fam, D, K, pulse=None):
    r"""The public function on the tensors ``D`` as they are: a tuple of its outputs, attached to the graph."""
    kw = {('Δf' if k == 'df' else k): D[k] for k in OPERANDS[fam][2:]}
    if fam == 'steady':
        return (fused.ab_steadystate(D['A'], D['B'], **kw),)
    if fam == 'train':
        return (fused.ab_train(D['A'], D['B'], n=K, **kw),)
    if fam == 'sequence':
        return (fused.ab_sequence(D['A'], D['B'], pulse=list(pulse), **kw),)
    return fused.train_signal(D['A'], D['B'], n=K, return_last=True, **kw)


def _gated(fam, tag, case, got, want, keys=None):
    r"""Every ``keys`` of ``got`` at ``test_steadystate._gate`` from ``want``; the figure the gate holds -- fp64: max abs,
    a gradient in units of the yardstick's largest element; fp32: relative L2 -- goes to the ledger next to the gate."""
    keys = list(keys or want)
    for k in keys:
        w = torch.as_tensor(want[k]).detach().double().cpu()
        if tag == 'f64':
            scale = float(w.abs().max()) if 'grad' in k and w.numel() else 1.0
            d = max_abs(got[k], w) / (scale if scale > 0 else 1.0)
        else:
            d = rel_l2(got[k], w)
        record(f'requests.{fam}.{tag}.{case}.{k}', d, 1e-9 if tag == 'f64' else 1e-6)
        print(f'requests.{fam}.{tag}.{case}.{k}: {d:.3e}')
    for k in keys:
        _gate(got[k], want[k], tag, f'{case}: {k}')


def _nonzero(got, what, but=()):
    for k, x in got.items():
        if k not in but:
            assert x is not None and float(x.abs().max()) > 0, (what, k)


def _recorded(monkeypatch, name):
    r"""The argument tuples of every call of the library's entry point ``name`` from here on."""
    lib = mrphy_amd.require_library()
    seen, inner = [], getattr(lib, name)
    monkeypatch.setattr(lib, name, lambda *a: (seen.append(a), inner(*a))[1])
    return seen


# =============================================================================================
# 1. which gradients are asked for
# =============================================================================================
@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('fam', FAMILIES)
def test_one_leaf_at_a_time(fam, tag, monkeypatch):
    r"""The all-leaves run against the family's fp64 yardstick, at the gate.  Then every differentiable operand alone
    requires grad, every other one a plain tensor: the other outputs of the adjoint are null pointers (``gA``, ``gB``,
    ``gC``, ``gMi``, ``gphi`` of Ktrb; those and ``grx`` of Ktrsb, whose phase workspace is asked for with ``phase``
    alone; ``gA``, ``gB``, ``gC`` of Kssb; those, ``grest`` and the workspace of Ksqb).  One backward entry-point call;
    the outputs and the one gradient are the all-leaves run's bit for bit, the other operands' ``.grad`` stay ``None``."""
    P, want, K = _problem(fam, tag)
    base = _base(fam, tag)
    assert set(base) == set(want)
    _gated(fam, tag, 'all_leaves', base, want)
    _nonzero(base, 'all leaves')
    calls = _counted(monkeypatch, (BWD[fam],))
    for X in OPERANDS[fam]:
        calls.clear()
        got = _run(fam, P, K, leaves=(X,))
        assert dict(calls) == {BWD[fam]: 1}, (X, dict(calls))
        for k in OUT[fam]:
            assert torch.equal(got[k], base[k]), (X, k)
        for Y in OPERANDS[fam]:
            g = got['grad_' + Y]
            if Y != X:
                assert g is None, f'{X} alone requires grad, and {Y} got a gradient'
                continue
            assert g is not None and g.shape == P[X].shape and g.dtype == DT[tag] and float(g.abs().max()) > 0, X
            assert torch.equal(g, base['grad_' + X]), f'grad_{X} asked for alone differs from the all-leaves run'


@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('fam', FAMILIES)
def test_everything_but_the_pulse_and_the_pulse_alone(fam, tag, monkeypatch):
    r"""Every optional operand requires grad, ``A`` and ``B`` do not -- for ``ab_sequence`` the run without a workspace:
    the size query is not even made, ``work`` is null, no flush, no second pass -- and the complement, ``A`` and ``B``
    alone: the bits of the all-leaves run, ``None`` for what was not asked for, one backward call each."""
    P, _, K = _problem(fam, tag)
    base = _base(fam, tag)
    calls = _counted(monkeypatch, (BWD[fam],) + ((WORKSPACE,) if fam == 'sequence' else ()))
    optional = tuple(k for k in OPERANDS[fam] if k not in ('A', 'B'))
    for leaves in (optional, ('A', 'B')):
        calls.clear()
        got = _run(fam, P, K, leaves=leaves)
        assert calls[BWD[fam]] == 1, dict(calls)
        if fam == 'sequence':
            assert calls[WORKSPACE] == (1 if 'A' in leaves else 0), (leaves, dict(calls))
        for k in OUT[fam]:
            assert torch.equal(got[k], base[k]), (leaves, k)
        for Y in OPERANDS[fam]:
            g = got['grad_' + Y]
            if Y in leaves:
                assert g is not None and float(g.abs().max()) > 0 and torch.equal(g, base['grad_' + Y]), (leaves, Y)
            else:
                assert g is None, (leaves, Y)


@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('X', ['A', 'B'])
def test_one_half_of_the_bank_of_ab_sequence(tag, X):
    r"""``A`` alone and ``B`` alone: the null halves of ``k_ab_sequence_p2``.  The bits of the all-leaves run; entry 1 of
    the bank, which ``S7``'s schedule never plays, still gets exact zeros; the entries played none."""
    P, _, K = _problem('sequence', tag)
    base = _base('sequence', tag)
    got = _run('sequence', P, K, leaves=(X,))
    g = got['grad_' + X]
    assert got['grad_' + 'AB'.replace(X, '')] is None
    assert g.shape == P[X].shape and torch.equal(g, base['grad_' + X])
    assert float(g[1].abs().max()) == 0.0, f'grad_{X}[1]: the schedule never plays it'
    assert float(g[0].abs().min()) > 0 and float(g[2].abs().min()) > 0


def _peak_rise(fam, D, K, pulse, grad):
    r"""``(outputs, bytes by which the allocator's peak rises over one call)``."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with (torch.enable_grad() if grad else torch.no_grad()):
        out = _call(fam, D, K, pulse)
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - before


@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('fam', FAMILIES)
def test_no_leaf_at_all(fam, tag, monkeypatch):
    r"""No operand requires grad, grad mode on: the outputs do not require grad and are the all-leaves run's bits, one
    forward call and no backward entry point, and the allocator's peak rises by what it rises under ``torch.no_grad()``
    -- for the signal: no checkpoint buffer, which a single leaf brings back."""
    P, _, K = _problem(fam, tag)
    base = _base(fam, tag)
    D = {k: dev(P[k]) for k in OPERANDS[fam]}
    calls = _counted(monkeypatch, (FWD[fam], BWD[fam]))
    out, rise = _peak_rise(fam, D, K, P.get('pulse'), True)
    assert dict(calls) == {FWD[fam]: 1}, dict(calls)
    for k, x in zip(OUT[fam], out):
        assert not x.requires_grad and x.grad_fn is None, k
        assert torch.equal(x, base[k]), k
    _, quiet = _peak_rise(fam, D, K, P.get('pulse'), False)
    print(f'{fam} {tag}: peak rise {rise} B without a leaf, {quiet} B under no_grad')
    assert rise == quiet, (rise, quiet)
    if fam == 'signal':
        _, kept = _peak_rise(fam, dict(D, T1=D['T1'].clone().requires_grad_(True)), K, None, True)
        print(f'{fam} {tag}: peak rise {kept} B with one leaf; the checkpoints: {-(-K // TS.S) * N * nM * 3 * 8} B')
        assert kept > rise, (kept, rise)


# ---------------------------------------------------------------------------------------------
# which output of train_signal carries the cotangent
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('which', ['sig', 'Mlast'])
def test_signal_cotangent_on_one_output(tag, which, monkeypatch):
    r"""A loss on ``sig`` alone -- ``Mlast`` is returned and unused: ``gMl`` null -- and on ``Mlast`` alone -- ``gs`` null:
    every gradient at the gate from the yardstick with the same loss, and the bits of the two-cotangent run whose weights
    on the other output are exact zeros.  With ``Mlast`` alone ``grad_rx`` is exact zeros in the shape of ``rx``."""
    P, _, K = _problem('signal', tag)
    w, v = TS._loss_weights(P, K, P['rx'])
    if which == 'sig':
        v = torch.zeros_like(v)
        loss = lambda sig, Mlast: (sig * dev(w)).sum().backward()  # noqa: E731
    else:
        w = torch.zeros_like(w)
        loss = lambda sig, Mlast: (Mlast * dev(v)).sum().backward()  # noqa: E731
    two = _run('signal', P, K, w=w, v=v)
    seen = _recorded(monkeypatch, BWD['signal'])
    got = _run('signal', P, K, loss=loss)
    assert len(seen) == 1
    assert (seen[0][GS] is None) == (which == 'Mlast') and (seen[0][GL] is None) == (which == 'sig'), seen[0][GS:GL + 1]
    _gated('signal', tag, f'{which}_alone', got, TS._yardstick(P, K, P['rx'], w=w, v=v))
    _same_bits(got, two, f'{which} alone vs exact-zero weights on the other output')
    _nonzero(got, which, but=('grad_rx',) if which == 'Mlast' else ())
    if which == 'Mlast':
        assert got['grad_rx'].shape == P['rx'].shape and float(got['grad_rx'].abs().max()) == 0.0


@pytest.mark.parametrize('tag', TAGS)
def test_signal_cotangent_on_Mlast_alone_without_a_repetition(tag, monkeypatch):
    r"""``K = 0`` and a loss on ``Mlast`` alone: ``Mlast`` is ``Mi``, so ``grad_Mi`` is the cotangent itself; every
    other gradient is exact zeros of its operand's shape."""
    P, _, _ = _problem('signal', tag)
    E = dict(P, phase=P['phase'][:, :0])
    _, v = TS._loss_weights(E, 0, P['rx'])
    seen = _recorded(monkeypatch, BWD['signal'])
    got = _run('signal', E, 0, n=False, loss=lambda sig, Mlast: (Mlast * dev(v)).sum().backward())
    assert all(a[GS] is None for a in seen)
    assert got['sig'].shape == (N, 2, 0, NRX) and torch.equal(got['Mlast'].cpu(), P['Mi'])
    assert float(v.abs().max()) > 0 and torch.equal(got['grad_Mi'].cpu(), v)
    for k in OPERANDS['signal']:
        g = got['grad_' + k]
        assert g is not None and g.shape == E[k].shape and g.dtype == DT[tag], k
        if k != 'Mi':
            assert float(g.abs().sum()) == 0.0, k


@pytest.mark.parametrize('tag', TAGS)
def test_signal_later_coil_blocks_run_without_an_Mlast_cotangent(tag, monkeypatch):
    r"""Nine receive coils, over the capacity: blocks of coils, one simulation each, and ``Mlast`` is the first block's.
    The loss is on ``sig[..., 8]`` (the last block) plus ``Mlast`` (the first): every backward call but one gets a null
    ``gMl``.  Every gradient at the gate from the yardstick; ``grad_rx[..., :8]`` is exact zeros."""
    P, _, K = _problem('signal', tag)
    rx = TS._rx(N, nM, 9, tag)
    cap = int(mrphy_amd.require_library().mrphy_train_signal_max_rx(0 if tag == 'f32' else 1))
    w8, v = TS._sin((N, 2, K), DT[tag]), TS._loss_weights(P, K, rx)[1]
    w = torch.zeros((N, 2, K, 9), dtype=DT[tag])
    w[..., 8] = w8
    seen = _recorded(monkeypatch, BWD['signal'])
    got = _run('signal', dict(P, rx=rx), K,
               loss=lambda sig, Mlast: ((sig[..., 8] * dev(w8)).sum() + (Mlast * dev(v)).sum()).backward())
    assert len(seen) == -(-9 // cap) > 1
    assert sorted(a[GL] is None for a in seen) == [False] + [True] * (len(seen) - 1)
    assert all(a[GS] is not None for a in seen)
    _gated('signal', tag, 'rx9_last_coil_and_Mlast', got, TS._yardstick(P, K, rx, w=w, v=v))
    _nonzero(got, 'nine coils')
    assert got['grad_rx'].shape == rx.shape and float(got['grad_rx'][..., :8].abs().max()) == 0.0
    assert float(got['grad_rx'][..., 8].abs().max()) > 0


# =============================================================================================
# 2. the form of the cotangent
# =============================================================================================
RECORD_FORMS = ['natural', 'stride0', 'last', 'every2', 'head', 'offset', 'wide']
SAMPLE_FORMS = ['view', 'stride0', 'real_row', 'one_coil', 'head', 'offset', 'wide']


def _tag_forms(forms):
    r"""(tag, form) without ('f64', 'wide'): the cotangent of another dtype is an fp64 one handed to the fp32 adjoint."""
    return [(tag, form) for tag in TAGS for form in forms if (tag, form) != ('f64', 'wide')]


@pytest.mark.parametrize('tag,form', _tag_forms(RECORD_FORMS))
@pytest.mark.parametrize('fam', ['train', 'sequence'])
def test_form_of_the_cotangent_of_the_records(fam, tag, form):
    r"""``Mt`` is a ``.movedim(0, -2)`` view of time-major storage and the adjoint reads a contiguous time-major
    cotangent, so every loss but the files' own hands over something else.  'natural': ``(Mt w_nat).sum()`` with a
    contiguous `(N, nM, K, 3)` weight -- what reaches ``backward`` is its time-major VIEW, asserted not contiguous;
    'stride0': ``Mt.sum()``, an expanded one; 'last', 'every2', 'head': losses on ``Mt[..., -1, :]``, ``Mt[..., ::2, :]``,
    ``Mt[..., :3, :]``, zeros elsewhere; 'offset': ``torch.autograd.backward`` with a contiguous time-major cotangent
    that starts one element into its buffer; 'wide' (fp32): an fp64 cotangent of the same values.  Every gradient has
    the bits of the plain time-major run with the same numbers as weights.  After 'head', ``grad_phase[:, k]`` and
    ``ab_sequence``'s ``grad_rest[:, k]`` are exact zeros for ``k >= 3``."""
    P, _, K = _problem(fam, tag)
    w = P['w']                                            # (K, N, nM, 3), the problem's own
    wd, seen = torch.zeros_like(w), []
    nat = lambda x: dev(x).movedim(0, -2)  # noqa: E731   a time-major weight as a view in the layout of Mt
    if form == 'natural':
        wd, wn = w, nat(w).contiguous()

        def loss(Mt):
            Mt.register_hook(lambda g: seen.append(not g.movedim(-2, 0).is_contiguous()))
            (Mt * wn).sum().backward()
    elif form == 'stride0':
        wd = torch.ones_like(w)

        def loss(Mt):
            Mt.register_hook(lambda g: seen.append(0 in g.stride()))
            Mt.sum().backward()
    elif form == 'last':
        wd[-1] = w[-1]
        loss = lambda Mt: (Mt[..., -1, :] * dev(w[-1])).sum().backward()  # noqa: E731
    elif form == 'every2':
        wd[::2] = w[::2]
        loss = lambda Mt: (Mt[..., ::2, :] * nat(w[::2])).sum().backward()  # noqa: E731
    elif form == 'head':
        wd[:3] = w[:3]
        loss = lambda Mt: (Mt[..., :3, :] * nat(w[:3])).sum().backward()  # noqa: E731
    elif form == 'offset':
        wd, g = w, place(cases._after(w))
        assert g.is_contiguous() and g.data_ptr() % 16 != 0
        loss = lambda Mt: torch.autograd.backward([Mt], [g.movedim(0, -2)])  # noqa: E731
    else:
        wd = w
        loss = lambda Mt: torch.autograd.backward([Mt], [nat(w.double())])  # noqa: E731
    got = _run(fam, P, K, loss=loss)
    plain = _base(fam, tag) if wd is w else _run(fam, dict(P, w=wd), K)
    if form in ('natural', 'stride0'):
        assert seen == [True], f'{form}: the cotangent did not arrive in the form under test'
    _same_bits(got, plain, f'{fam} {form}')
    _nonzero(got, form)
    if form == 'head':
        for k in ('grad_phase',) + (('grad_rest',) if fam == 'sequence' else ()):
            assert float(got[k][:, 3:].abs().max()) == 0.0 and float(got[k][:, 2].abs().min()) > 0, k


@pytest.mark.parametrize('tag,form', _tag_forms(SAMPLE_FORMS))
def test_form_of_the_cotangents_of_the_signal(tag, form):
    r"""The same for ``sig`` `(N, xy, K, 3)` and ``Mlast``.  'view': both cotangents are permuted views; 'stride0':
    ``sig.sum() + Mlast.sum()``; 'real_row', 'one_coil', 'head': losses on ``sig[:, 0]``, ``sig[..., 1]`` and
    ``sig[:, :, :3]`` alone (no cotangent for ``Mlast``), the dense run having exact zeros elsewhere; 'offset': both
    contiguous, one element into their buffers; 'wide' (fp32): fp64 cotangents.  The bits of the plain run; ``grad_rx``
    of the coils without a weight is exact zeros, and after 'head' so is ``grad_phase[:, k]`` for ``k >= 3``."""
    P, _, K = _problem('signal', tag)
    w, v = TS._loss_weights(P, K, P['rx'])                # (N, 2, K, 3) and (N, nM, 3), the problem's own
    wd, vd = torch.zeros_like(w), torch.zeros_like(v)
    if form == 'view':
        wd, vd = w, v
        gs, gl = place(w.permute(3, 2, 1, 0).contiguous().permute(3, 2, 1, 0)), place(v.permute(2, 0, 1).contiguous().permute(1, 2, 0))
        assert not gs.is_contiguous() and not gl.is_contiguous()
        loss = lambda sig, Mlast: torch.autograd.backward([sig, Mlast], [gs, gl])  # noqa: E731
    elif form == 'stride0':
        wd, vd = torch.ones_like(w), torch.ones_like(v)
        loss = lambda sig, Mlast: (sig.sum() + Mlast.sum()).backward()  # noqa: E731
    elif form == 'real_row':
        wd[:, 0] = w[:, 0]
        loss = lambda sig, Mlast: (sig[:, 0] * dev(w[:, 0])).sum().backward()  # noqa: E731
    elif form == 'one_coil':
        wd[..., 1] = w[..., 1]
        loss = lambda sig, Mlast: (sig[..., 1] * dev(w[..., 1])).sum().backward()  # noqa: E731
    elif form == 'head':
        wd[:, :, :3] = w[:, :, :3]
        loss = lambda sig, Mlast: (sig[:, :, :3] * dev(w[:, :, :3])).sum().backward()  # noqa: E731
    elif form == 'offset':
        wd, vd = w, v
        gs, gl = place(cases._after(w)), place(cases._after(v))
        assert gs.is_contiguous() and gl.is_contiguous() and gs.data_ptr() % 16 != 0 and gl.data_ptr() % 16 != 0
        loss = lambda sig, Mlast: torch.autograd.backward([sig, Mlast], [gs, gl])  # noqa: E731
    else:
        wd, vd = w, v
        loss = lambda sig, Mlast: torch.autograd.backward([sig, Mlast], [dev(w.double()), dev(v.double())])  # noqa: E731
    got = _run('signal', P, K, loss=loss)
    plain = _base('signal', tag) if wd is w else _run('signal', P, K, w=wd, v=vd)
    _same_bits(got, plain, f'signal {form}')
    _nonzero(got, form)
    if form == 'one_coil':
        assert float(got['grad_rx'][..., [0, 2]].abs().max()) == 0.0 and float(got['grad_rx'][..., 1].abs().max()) > 0
    if form == 'head':
        assert float(got['grad_phase'][:, 3:].abs().max()) == 0.0 and float(got['grad_phase'][:, 2].abs().min()) > 0


# =============================================================================================
# 3. the form of the operands
# =============================================================================================
def _spin_axis(fam, k):
    return 2 if fam == 'sequence' and k in ('A', 'B') else 1


def _spins_in_front(x, axis):
    r"""The same values stored with the spin axis in front and transposed back: not contiguous."""
    return x.movedim(axis, 0).contiguous().movedim(0, axis)


def _every_other(x):
    r"""``x`` `(…, L)` as the view ``wide[..., ::2]`` of a tensor twice as long."""
    wide = torch.zeros(tuple(x.shape[:-1]) + (2 * x.shape[-1],), dtype=x.dtype)
    wide[..., ::2] = x
    return wide[..., ::2]


def _summed(g, x):
    r"""The dense run's gradient ``g`` summed in fp64 over the entries that share an element of the operand ``x``."""
    g = g.double().cpu()
    shp = (tuple(x.shape) + (1,) * (g.ndim - x.ndim)) if x.ndim else (1,) * g.ndim
    return g.sum_to_size(shp).reshape(x.shape)


def _against(fam, tag, case, got, ref, P, over, shared=()):
    r"""The outputs and every gradient of ``got`` are ``ref``'s bit for bit, the gradients of the operands ``shared``
    are ``ref``'s summed in fp64 at the gate; each gradient has the shape, dtype and device of its operand as given
    (``over``, else ``P`` on the device).  Where the two runs' operands differ in dtype, so do their gradients: each is
    one rounding of the same fp64 number, and they are compared in the narrower type."""
    for k in OUT[fam]:
        assert got[k].dtype == ref[k].dtype and torch.equal(got[k], ref[k]), (case, k)
    for k in OPERANDS[fam]:
        g, r, x = got['grad_' + k], ref['grad_' + k], over.get(k, P[k])
        assert g is not None and g.shape == x.shape and g.dtype == x.dtype, (case, k, g.shape, g.dtype)
        assert g.device == (over[k].device if k in over else DEV), (case, k, g.device)
        assert float(g.abs().max()) > 0, (case, k)
        if k in shared:
            _gated(fam, tag, case, {'grad_' + k: g}, {'grad_' + k: _summed(r, x)})
        else:
            narrow = torch.float32 if torch.float32 in (g.dtype, r.dtype) else g.dtype
            assert torch.equal(g.to(narrow).cpu(), r.to(narrow).cpu()), f'{case}: grad_{k}'


FORMS = ['permuted', 'offset', 'expanded', 'mixed_Mi_1nM', 'mixed_Mi_N1', 'host']


@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('fam', TRANSIENT)
def test_form_of_the_operands(fam, tag, form):
    r"""The counterpart of ``test_ab_operands.test_ab_steadystate_views`` for the three transients.

    'permuted': ``A, B`` (the bank), ``Mi``, ``rx`` and the per-spin ``T1, T2, Δf`` stored with the spin axis in front
    and transposed back, ``phase`` and a 1-d ``rest`` as ``wide[..., ::2]``, ``ab_sequence``'s table as the ``.T`` of a
    `(K, N)` tensor: none contiguous on arrival.  'offset': every operand contiguous, one element into its buffer, off
    the 16-byte grid.  'expanded': ``Mi`` `(1, 1, 3)`, ``phase`` `(1, K)`, ``rx`` `(1, ...)` and 0-dim ``T1, T2, Δf``
    expanded to their full shapes, stride 0.  'mixed': ``T1`` 0-dim, ``T2`` `(N, 1)`, ``Δf`` `(1, nM)` in one call --
    each with its own strides --, ``rest`` `(1,)`, and ``Mi`` `(1, nM, 3)` or `(N, 1, 3)`.  'host': ``rest`` (0-dim),
    ``phase, Mi, T1, T2, Δf, rx`` as CPU tensors, for fp32 ``A, B`` in fp64 and the 0-dim ``rest`` in fp32, for fp64
    ``A, B`` the reverse.

    The outputs and every gradient that is not a sum over shared entries are those of the call on contiguous device
    tensors of the data type holding the same numbers (for 'expanded' and 'mixed': written out in full), bit for bit;
    the gradient of an operand given in a broadcast shape is that run's summed in fp64, at the gate.  Each gradient
    has its operand's shape, dtype and device."""
    P, _, K = _problem(fam, tag)
    ops = OPERANDS[fam]
    per_spin = [k for k in ops if k not in ('phase', 'rest')]
    full = lambda x, k: x.expand(P[k].shape).contiguous()  # noqa: E731
    ref, shared = None, ()
    if form == 'permuted':
        given = {k: _spins_in_front(P[k], _spin_axis(fam, k)) for k in per_spin}
        given['phase'] = _every_other(P['phase'])
        given['rest'] = P['rest'].T.contiguous().T if fam == 'sequence' else _every_other(P['rest'])
        over = {k: place(x) for k, x in given.items()}
        assert not any(x.is_contiguous() for x in over.values()), [k for k, x in over.items() if x.is_contiguous()]
    elif form == 'offset':
        given = {k: cases._after(P[k]) for k in ops}
        over = {k: place(x) for k, x in given.items()}
        assert all(x.is_contiguous() and x.data_ptr() % 16 != 0 for x in over.values())
    elif form == 'expanded':
        small = dict(Mi=P['Mi'][:1, :1].clone(), phase=P['phase'][:1].clone(),
                     **{k: P[k][0, 0].clone() for k in ('T1', 'T2', 'df')}, **({'rx': P['rx'][:1].clone()} if fam == 'signal' else {}))
        given = {k: x.expand(P[k].shape) for k, x in small.items()}
        over = {k: place(x) for k, x in given.items()}
        assert all(0 in x.stride() for x in over.values())
        ref = _run(fam, dict(P, **{k: x.contiguous() for k, x in given.items()}), K)
    elif form.startswith('mixed'):
        given = dict(T1=P['T1'][0, 0].clone(), T2=P['T2'][:, :1].clone(), df=P['df'][:1].clone(),
                     rest=(P['rest'][0, 2] if fam == 'sequence' else P['rest'][0]).reshape(1).clone(),
                     Mi=(P['Mi'][:1] if form == 'mixed_Mi_1nM' else P['Mi'][:, :1]).clone())
        over = {k: dev(x) for k, x in given.items()}
        shared = tuple(given)
        dense = {k: full(x, k) for k, x in given.items() if k != 'rest'}
        dense['rest'] = given['rest'].expand(N).contiguous()          # (N,): the constant rest of every family
        ref = _run(fam, dict(P, **dense), K)
    else:
        other = torch.float64 if tag == 'f32' else torch.float32
        names = [k for k in ops if k not in ('A', 'B')]
        given = {k: P[k].to(other) for k in names if k != 'rest'}
        given['rest'] = (P['rest'][0, 2] if fam == 'sequence' else P['rest'][0]).clone()     # 0-dim, in the data type
        assert given['rest'].ndim == 0 and given['rest'].dtype == DT[tag] and given['phase'].dtype == other
        over = {k: x.clone() for k, x in given.items()}
        assert all(x.device.type == 'cpu' for x in over.values())
        # the same numbers in the data type on the device, in the same shapes: nothing is summed differently
        ref = _run(fam, dict(P, **{k: x.to(DT[tag]) for k, x in given.items()}), K)
    if ref is None:
        ref = _base(fam, tag)
    got = _run(fam, P, K, over=over)
    _against(fam, tag, form, got, ref, P, over, shared)


# ---------------------------------------------------------------------------------------------
# fp16 / bf16: half_via_float
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('half', list(HALF))
@pytest.mark.parametrize('fam', FAMILIES)
def test_half_operands_are_computed_in_fp32(fam, half):
    r"""Every floating operand and the loss's weights in fp16 / bf16 -- the fp32 problem's values rounded to the half
    type, the constant ``rest`` on a grid both hold (2^-8 s and 1.5 · 2^-8 s) --: the outputs have the half dtype and are
    the fp32 call's on the widened values, rounded; the gradients arrive in the half dtype and are the fp32 gradients,
    rounded.  That is all ``half_via_float`` promises, and it involves no tolerance."""
    h = HALF[half]
    P32, _, K = _problem(fam, 'f32')
    P32 = dict(P32)
    if fam != 'sequence':
        P32['rest'] = torch.tensor([2.0 ** -8, 1.5 * 2.0 ** -8])
    lower = lambda x: x.to(h) if isinstance(x, torch.Tensor) else x  # noqa: E731
    Ph = {k: lower(x) for k, x in P32.items()}
    Pf = {k: (x.float() if isinstance(x, torch.Tensor) else x) for k, x in Ph.items()}
    if fam != 'sequence':
        assert torch.equal(Pf['rest'], P32['rest'])
    kh, kf = {}, {}
    if fam == 'signal':
        w, v = (x.to(h) for x in TS._loss_weights(P32, K, P32['rx']))
        kh, kf = dict(w=w, v=v), dict(w=w.float(), v=v.float())
    got, ref = _run(fam, Ph, K, **kh), _run(fam, Pf, K, **kf)
    assert set(got) == set(ref)
    for k in got:
        assert got[k].dtype == h and ref[k].dtype == torch.float32, (k, got[k].dtype, ref[k].dtype)
        assert got[k].shape == ref[k].shape and float(got[k].float().abs().max()) > 0, k
        assert torch.equal(got[k], ref[k].to(h)), f'{fam} {half}: {k} is not the fp32 result rounded'
