"""GPU tests (-m gpu) of ConvEngine's point blocking with the REAL kernels.

Every public call of ConvEngine goes through ConvEngine._blocked: a job of more than point_block(n_samples) points runs as consecutive
blocks on ONE cached workspace per block size, and the parts are joined.  BASELINE config 5's 10 000 points run that way (3296 + 3296 +
3296 + 112).  Here RBNN_CONV_WS_GB = 0.001 makes point_block 16, so 40 points run as 16 + 16 + 8: two equal blocks on one workspace and
a ragged tail.

  a  plumbing, bit for bit: rows lo:hi of every blocked call equal the unblocked call of a SECOND engine (own workspaces, budget at its
     default) on x[lo:hi], y[lo:hi] — the same launches on the same batch; every blocked call made twice, the second equal to the first
  b  whole vs blocked on the same engine, where the code makes a point's arithmetic independent of its batch (the exact mode)
  c  the blocked results against fp64 directly, the project's conv bar (1e-5 per point, pooling / sign decisions pinned from the kernels)
Inputs and posteriors as tests/test_hip_sharded_2rank.py builds them.  The two-rank blocked case is in that file.
"""
import types

import pytest
import torch

from conftest import cancellation_condition, rel_err_points
from oracle import bnn_oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("built_library")]
TOL, DEV, ENV = 1e-5, "cuda:0", "RBNN_CONV_WS_GB"
Hc, C, S, N = 32, 10, 3, 40
BLOCKS = [(0, 16), (16, 32), (32, 40)]
CASES = [((1, 28, 28), "exact", "leaky"), ((1, 28, 28), "triple", "leaky"), ((1, 28, 28), "split", "leaky"),
         ((3, 32, 32), "exact", "leaky"), ((3, 32, 32), "triple", "leaky"), ((3, 32, 32), "triple", "tanh")]


def problem(shape, seed=11):
    """(posterior, x, y) of a case: seeds checked on the CPU oracle to stay inside the exclusion cap of test c (see there)."""
    D = shape[0] * shape[1] * shape[2]
    q2 = (shape[1] - 4) // 2 - 5
    post = O.synthetic_posterior("conv", D, Hc, C, S, 0.05, in_ch=shape[0], head=q2 * q2 * Hc)
    x, y = O.synthetic_inputs(N, shape, C, seed=seed)
    return post, x, y


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-{c[1]}-{c[2]}")
def case(request):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from robustbnns_amd.conv import ConvEngine, ConvStackedPosterior
    shape, precision, act = request.param
    post, x, y = problem(shape)
    sp = ConvStackedPosterior(act, shape, C, Hc, post, DEV)
    eng, ref = ConvEngine(sp, precision=precision), ConvEngine(sp, precision=precision)
    assert eng.precision == ref.precision == precision
    g = torch.Generator().manual_seed(3)
    xa = torch.clamp(x + 0.1 * torch.randn(x.shape, generator=g).sign(), 0, 1)
    return types.SimpleNamespace(shape=shape, precision=precision, act=act, post=post, x=x, y=y, xd=x.to(DEV), xa=xa, lab=y.argmax(-1),
                                 eng=eng, ref=ref)


def _cpu(out):
    return tuple(t.detach().cpu().clone() for t in (out if isinstance(out, tuple) else (out,)))


def _blocked(c, monkeypatch, call):
    """call(engine, x, y, lo, hi) on all 40 points (device-resident, as bench.py holds them) at the 16-point budget, TWICE: the second run
    meets whatever the first left in the cached workspaces (Psum, the stashes, dQ2 in Q2's place) and must reproduce it."""
    monkeypatch.setenv(ENV, "0.001")
    assert c.eng.point_block(S) == 16 and c.eng.group_point_block(S) == 16
    first = _cpu(call(c.eng, c.xd, c.y, 0, N))
    second = _cpu(call(c.eng, c.xd, c.y, 0, N))
    for i, (a, b) in enumerate(zip(first, second)):
        assert torch.equal(a, b), f"second blocked call differs from the first in result {i}: {int((a != b).sum())} elements"
    return first


def _per_block(c, monkeypatch, call):
    """The yardstick: the second engine's UNBLOCKED call on each block alone, budget at its default, joined in order."""
    monkeypatch.setenv(ENV, "48")
    assert c.ref.point_block(S) > N
    parts = [_cpu(call(c.ref, c.x[lo:hi], c.y[lo:hi], lo, hi)) for lo, hi in BLOCKS]
    return tuple(torch.cat(col) for col in zip(*parts))


def _same(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape, (what, i, a.shape, b.shape)
        rows = sorted(set((a != b).reshape(len(a), -1).any(1).nonzero().flatten().tolist()))
        assert torch.equal(a, b), f"{what}, result {i}: rows {rows[:12]} differ ({int((a != b).sum())} elements)"


# ------------------------------------------------------------------ a. plumbing, bit for bit
def test_blocked_forward_equals_each_block_alone(case, monkeypatch):
    c = case
    seen = []
    inner = c.eng._forward_kernels
    monkeypatch.setattr(c.eng, "_forward_kernels", lambda Xp, *a: (seen.append(Xp.shape[0]), inner(Xp, *a))[1])
    for what, call in (("forward", lambda e, x, y, lo, hi: e.forward(x, S)), ("forward logits", lambda e, x, y, lo, hi: e.forward(x, S, logits=True)),
                       ("clean_outputs", lambda e, x, y, lo, hi: e.clean_outputs(x, S)),
                       ("clean_outputs logits", lambda e, x, y, lo, hi: e.clean_outputs(x, S, logits=True))):
        seen.clear()
        got = _blocked(c, monkeypatch, call)
        assert seen == [16, 16, 8] * 2, seen                        # the blocks: two of one size on one workspace, and a ragged tail
        assert got[0].shape[0] == N
        _same(got, _per_block(c, monkeypatch, call), what)
    assert len(c.eng._ws_cache) == 2 and set(c.eng._ws_cache) == {(16, S), (8, S)}


def test_blocked_gradients_equal_each_block_alone(case, monkeypatch):
    from robustbnns_amd import _hip
    c = case
    for what, call in (("loss_gradients", lambda e, x, y, lo, hi: e.loss_gradients(x, y, S)),
                       ("loss_gradients norms", lambda e, x, y, lo, hi: e.loss_gradients(x, y, S, norms=True)),
                       ("attack_gradient", lambda e, x, y, lo, hi: e.attack_gradient(x, y, S)),
                       ("attack_gradient mean_logit", lambda e, x, y, lo, hi: e.attack_gradient(x, y, S, mode=_hip.LOSS_MEAN_LOGIT))):
        got = _blocked(c, monkeypatch, call)
        assert len(got) == (3 if "norms" in what else 1) and all(t.shape[0] == N for t in got)
        _same(got, _per_block(c, monkeypatch, call), what)
    g, linf, l2 = _blocked(c, monkeypatch, lambda e, x, y, lo, hi: e.loss_gradients(x, y, S, norms=True))
    assert g.shape == c.x.shape and linf.shape == l2.shape == (N,)
    assert torch.equal(linf, g.reshape(N, -1).abs().max(1)[0])      # the norms are those of the gradient rows they come with


def test_blocked_attacks_equal_each_block_alone(case, monkeypatch):
    from robustbnns_amd import _hip
    c = case
    for what, call in (("fgsm mean_prob", lambda e, x, y, lo, hi: e.fgsm(x, y, S, 0.1, mode=_hip.LOSS_MEAN_PROB)),
                       ("fgsm mean_logit", lambda e, x, y, lo, hi: e.fgsm(x, y, S, 0.1, mode=_hip.LOSS_MEAN_LOGIT)),
                       ("pgd alpha=None", lambda e, x, y, lo, hi: e.pgd(x, y, S, 0.2, iters=3)),
                       ("pgd alpha=2/225", lambda e, x, y, lo, hi: e.pgd(x, y, S, 0.2, alpha=2 / 225, iters=3))):
        got = _blocked(c, monkeypatch, call)
        assert got[0].shape == c.x.shape and not torch.equal(got[0], c.x)
        _same(got, _per_block(c, monkeypatch, call), what)
    ran = []
    call = lambda e, x, y, lo, hi: e.pgd(x, y, S, 0.2, iters=3, before_step=lambda: ran.append(1))
    monkeypatch.setenv(ENV, "0.001")
    got = _cpu(call(c.eng, c.xd, c.y, 0, N))
    assert len(ran) == 3 * (3 - 1)                                  # before every iteration but the first, of EVERY block
    _same(got, _per_block(c, monkeypatch, call), "pgd before_step")
    _same(got, _blocked(c, monkeypatch, lambda e, x, y, lo, hi: e.pgd(x, y, S, 0.2, iters=3)), "pgd before_step vs none")


@pytest.mark.parametrize("with_clean", [False, True])
def test_blocked_evaluate_equals_each_block_alone(case, monkeypatch, with_clean):
    c = case

    def call(e, x, y, lo, hi):
        xa = c.xa[lo:hi].to(x.device)
        clean = e.clean_outputs(x, S) if with_clean else None
        oa, aa, rob, o, a = e.evaluate(x, xa, y, S, clean=clean)
        call.acc.append((oa, aa))
        return rob, o, a

    call.acc = []
    rob, o, a = _blocked(c, monkeypatch, call)
    (oa, aa), again = call.acc[0], call.acc[1]
    assert (oa, aa) == again and rob.shape == (N,) and o.shape == a.shape == (N, C)
    want = _per_block(c, monkeypatch, call)
    _same((rob, o, a), want, "evaluate" + (" clean=" if with_clean else ""))
    # the accuracies: the counts of a host argmax of the returned outputs over ALL points (tests/test_hip_parity.py::test_full_size_properties (f))
    assert oa == 100 * float((o.argmax(-1) == c.lab).sum()) / N
    assert aa == 100 * float((a.argmax(-1) == c.lab).sum()) / N
    per_block = call.acc[2:]
    assert len(per_block) == 3
    assert oa == sum(p[0] * (hi - lo) for p, (lo, hi) in zip(per_block, BLOCKS)) / N
    assert aa == sum(p[1] * (hi - lo) for p, (lo, hi) in zip(per_block, BLOCKS)) / N


# ------------------------------------------------------------------ b. whole vs blocked
@pytest.mark.parametrize("shape", [(1, 28, 28), (3, 32, 32)])
def test_blocked_equals_whole_where_a_point_does_not_depend_on_its_batch(shape, monkeypatch):
    """exact mode only.  The fp32 conv kernels work per (point, sample) item, the head per point column, the sums over samples, the loss
    and the step per point: nothing a point's arithmetic reads comes from another point, so its rows are the same bits whichever batch
    it runs in.  The triple and split modes are NOT held to this: their forward scales the pooled conv1 activations by a power of two
    taken from max |x| over the batch handed to AttackEngine._call_scales (rbnn_input_scales), so a block can legitimately run at
    another scale than the whole; test c holds their blocked results to fp64 instead."""
    from robustbnns_amd import _hip
    from robustbnns_amd.conv import ConvEngine, ConvStackedPosterior
    post, x, y = problem(shape)
    eng = ConvEngine(ConvStackedPosterior("leaky", shape, C, Hc, post, DEV), precision="exact")
    calls = (("forward", lambda: eng.forward(x, S)), ("loss_gradients", lambda: eng.loss_gradients(x, y, S, norms=True)),
             ("attack_gradient", lambda: eng.attack_gradient(x, y, S)), ("fgsm", lambda: eng.fgsm(x, y, S, 0.1)),
             ("fgsm mean_logit", lambda: eng.fgsm(x, y, S, 0.1, mode=_hip.LOSS_MEAN_LOGIT)), ("pgd", lambda: eng.pgd(x, y, S, 0.2, iters=3)),
             ("evaluate", lambda: eng.evaluate(x, x.flip(0), y, S)[2:]))
    for what, call in calls:
        monkeypatch.setenv(ENV, "48")
        whole = _cpu(call())
        monkeypatch.setenv(ENV, "0.001")
        assert eng.point_block(S) == 16
        _same(_cpu(call()), whole, f"{what}: blocked vs whole")


# ------------------------------------------------------------------ c. against fp64
def test_blocked_results_against_fp64(case, monkeypatch):
    """The blocked forward (probabilities, logits) of all 40 points within 1e-5 per point of the fp64 oracle; the blocked loss_gradients
    and attack_gradient within 1e-5 per point of the fp64 oracle that takes the kernels' own pooling / sign decisions (a conv net has
    ~10^4 of them per (point, sample), and one within fp32 rounding of a tie goes either way: tests/test_hip_round2.py).  The decisions
    are read from the second engine's unblocked run of each block — test a holds that run and the blocked one to the same bits.  Against
    the PLAIN fp64 oracle a point may be further than 1e-5 only with a flipped decision, and at most max(3, N // 20) points may;
    cancellation among the samples (conftest.cancellation_condition) must not lift any point's fp32 floor above 1e-5 at these seeds.
    Checked on the CPU before the first GPU run, with torch's fp32 evaluation of the oracle in the kernels' place: no point of either
    geometry, either activation, is over 1e-5 from fp64 or has 2^-23 x its cancellation condition above 1e-5."""
    import test_hip_round2 as R2
    c = case
    p64 = O.cast(c.post, torch.float64)
    probs = _blocked(c, monkeypatch, lambda e, x, y, lo, hi: e.forward(x, S))[0]
    logits = _blocked(c, monkeypatch, lambda e, x, y, lo, hi: e.forward(x, S, logits=True))[0]
    e_p = rel_err_points(probs, O.bnn_forward(c.x.double(), p64, "conv", c.act, S))
    e_l = rel_err_points(logits, O.ensemble_forward(c.x.double(), p64, "conv", c.act, S))
    print(f"[conv blocking {c.shape} {c.precision} {c.act}] forward vs fp64: probabilities {float(e_p.max()):.2e}, logits {float(e_l.max()):.2e}")
    assert float(e_p.max()) < TOL and float(e_l.max()) < TOL
    cond = 2.0 ** -23 * cancellation_condition(c.x, c.lab, c.post, "conv", c.act, S)
    assert float(cond.max()) <= TOL, f"cancellation lifts the fp32 floor of {int((cond > TOL).sum())} points above 1e-5: choose other seeds"
    cap = max(3, N // 20)
    for mode, call, plain in (("per_sample", lambda e, x, y, lo, hi: e.loss_gradients(x, y, S), O.loss_gradients(c.x.double(), c.y, p64, "conv", c.act, S)),
                              ("mean_prob", lambda e, x, y, lo, hi: e.attack_gradient(x, y, S), O.meanprob_gradients(c.x.double(), c.lab, p64, "conv", c.act, S))):
        G = _blocked(c, monkeypatch, call)[0].reshape(c.x.shape)
        monkeypatch.setenv(ENV, "48")
        st1, st2 = [], []
        for lo, hi in BLOCKS:                                       # the kernels' decisions, block by block, from the unblocked run
            Gb = _cpu(call(c.ref, c.x[lo:hi], c.y[lo:hi], lo, hi))[0].reshape(c.x[lo:hi].shape)
            assert torch.equal(Gb, G[lo:hi])
            a, b = R2.conv_stashes(c.ref, hi - lo, S, Hc)
            st1.append(a.clone()); st2.append(b.clone())
        pinned, far, n_diff = R2.conv_pinned_oracle(c.x, c.lab, c.post, c.act, S, torch.cat(st1, 1), torch.cat(st2, 1), mode)
        err, err_plain = R2.per_point_err(G, pinned), R2.per_point_err(G, plain)
        flipped = int(((err_plain >= TOL) & (n_diff > 0)).sum())
        print(f"[conv blocking {c.shape} {c.precision} {c.act} {mode}] pinned: max {float(err.max()):.2e} median {float(err.median()):.2e}; plain: "
              f"max {float(err_plain.max()):.2e}; points off the plain oracle by a flipped decision {flipped}/{N} (cap {cap}), farthest from a tie {far:.1e}")
        assert float(err.max()) < TOL and float(err.median()) < R2.MEDIAN_BAR
        assert far < R2.KINK_CONV
        assert not ((err_plain >= TOL) & (n_diff == 0)).any(), "points differ from the plain fp64 oracle without a flipped decision"
        assert flipped <= cap
