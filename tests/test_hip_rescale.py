"""GPU tests (-m gpu): results must not change under function-preserving rescaling of the weights.

Rescaling a block of units of one sample by a power of two alpha and the next layer's matching weights by 1 / alpha (relu / leaky, max pooling:
tests/test_rescale_guard.py::rescale) computes exactly the same function in fp64, but leaves every other slice of the tensor alpha below the ONE
power-of-two scale that the triple and split images share per tensor (conv1: per sample).  Every case runs under `auto` and is compared with the
fp64 oracle of the UNSCALED posterior: forward (probabilities, logits), loss_gradients, MEAN_PROB and MEAN_LOGIT gradients, FGSM on both, two PGD
steps on the kernel's own iterates and evaluate.  An explicit precision="triple" / "split" must meet the same bar or raise HipError.

  R  fc (a block of hidden units, one whole sample), fc2 (layer-1 units, layer-2 units), conv at 1x28x28 and 3x32x32 (a conv1 channel, a conv2
     channel), alpha in {2^8, 2^16, 2^20, 2^24, 2^30}; SVI guides (fc, conv) rescaled block-wise, checked on the weights actually drawn;
     controls: a lowdim net (D = 16, fp32 FMA) and precision="exact"
  X  where `auto` now falls back: exact at hidden 384 and 640 (fc, fc2); C in {11, 12, 13, 16} for fc / fc2 (exact) and conv (auto = triple,
     and exact); the autograd hook at C = 16 and C = 13 (NaN in G_up's padding classes leaves the result unchanged)
Every case prints one line: resolved precision, alpha, the rescaled slice, the worst error in units of 1e-5 and what each exclusion removed.
Everything goes through the C-ABI (robustbnns_amd._hip); the oracle is the checker only.
"""
import numpy as np
import pytest
import torch

import test_hip_edges as E
import test_hip_round2 as R2
from conftest import cancellation_condition, rel_err_points
from oracle import bnn_oracle as O
from test_rescale_guard import ALPHAS, rescale, rescale_guide

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("built_library")]
TOL, TAU, KINK, DEV = 1e-5, 1e-3, 2e-6, "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from robustbnns_amd import _hip
    _hip.load()


def _line(tag, precision, worst, kink, canc, marg, N, refused=""):
    print(f"[rescale {tag}] precision == {precision}{refused}; worst {worst / TOL:.3f} x 1e-5; excluded: kink {kink} / cancellation {canc} / "
          f"marginal-pixel {marg} of {N} (points / points / pixels)")


def _log2(alpha):
    return f"2^{int(np.log2(alpha))}"


# ------------------------------------------------------------------ the checks against fp64
def _pgd_and_evaluate(eng, arch, act, x, y, post, S, ref_grad):
    """Two PGD steps (MEAN_PROB) on the kernel's own iterates, each one reference step (oracle.pgd_step's fp32 order) from the kernel's x_k with
    the reference gradient ref_grad(x_k) -> (g, ok rows); then evaluate on (x, x_2) against the fp64 forward.  Returns (worst, marginal pixels)."""
    N = x.shape[0]
    eps = 0.1
    alpha = (2 / x.reshape(N, -1).max(1)[0]).reshape((N,) + (1,) * (x.dim() - 1))
    iters = [x] + [eng.pgd(x, y, S, eps, alpha=None, iters=k).cpu() for k in (1, 2)]
    marg = 0
    for k in range(2):
        g, ok = ref_grad(iters[k])
        want = torch.clamp(x + torch.clamp(iters[k] + alpha * g.sign().float() - x, min=-eps, max=eps), min=0, max=1)
        safe, m = E._safe_pixels(g, ok)
        marg = max(marg, m)
        bad = ((iters[k + 1] - want).abs().reshape(N, -1) > 1e-6) & safe
        assert not bad.any(), f"pgd step {k} -> {k + 1}: {int(bad.sum())} non-marginal pixels differ"
    p64 = O.cast(post, torch.float64)
    oa, aa, rob, o, a = eng.evaluate(x, iters[2], y, S)
    o64, a64 = O.bnn_forward(x.double(), p64, arch, act, S), O.bnn_forward(iters[2].double(), p64, arch, act, S)
    worst = max(float(rel_err_points(o.cpu(), o64).max()), float(rel_err_points(a.cpu(), a64).max()))
    assert worst < TOL, f"evaluate: outputs {worst / TOL:.3f} x 1e-5"
    _, _, rob64 = O.attack_evaluation(x.double(), iters[2].double(), y, p64, arch, act, S)
    assert float((rob.cpu().double() - rob64).abs().max()) < TOL
    lab = y.argmax(-1)
    assert oa == 100 * float((o.cpu().argmax(-1) == lab).sum()) / N and aa == 100 * float((a.cpu().argmax(-1) == lab).sum()) / N
    return worst, marg


def _fc_checks(eng, arch, act, x, y, post, S, tag):
    """test_hip_edges' forward / gradient / FGSM / seeds checks against fp64 of `post`, plus two PGD steps and evaluate."""
    worst, kinks, canc, marg = E._fp64_checks(eng, arch, act, x, y, post, S, tag)
    p64 = O.cast(post, torch.float64)
    lab = y.argmax(-1)

    def ref_grad(xk):
        return (O.meanprob_gradients(xk.double(), lab, p64, arch, act, S),
                O.kink_margin(xk.double(), p64, arch, act, S) > KINK)
    w2, m2 = _pgd_and_evaluate(eng, arch, act, x, y, post, S, ref_grad)
    return max(worst, w2), kinks, canc, max(marg, m2)


def _conv_checks(eng, act, x, y, post, S, Hc, tag):
    """conv: forward to 1e-5 against plain fp64; every gradient (PER_SAMPLE, MEAN_PROB, MEAN_LOGIT) against the decision-pinned fp64 oracle (the
    kernels' own pooling / sign decisions, within fp32 noise of a tie), and against plain fp64 wherever no decision differs; FGSM on both
    means and the PGD steps at the safe pixels of the points where the pinned oracle equals the plain one."""
    from robustbnns_amd import _hip
    N = x.shape[0]
    lab = y.argmax(-1)
    labd = lab.int().to(DEV)
    p64 = O.cast(post, torch.float64)
    xd = x.double()
    worst = float(rel_err_points(eng.forward(x, S).cpu(), O.bnn_forward(xd, p64, "conv", act, S)).max())
    worst = max(worst, float(rel_err_points(eng.forward(x, S, logits=True).cpu(), O.ensemble_forward(xd, p64, "conv", act, S)).max()))
    assert worst < TOL, f"{tag}: forward {worst / TOL:.3f} x 1e-5"
    flipped = canc = marg = 0

    def pinned_grad(xk, mode, kind):
        G = eng.gradient(eng.pad_inputs(xk), labd, None, S, mode).cpu().reshape(N, -1).clone()
        st1, st2 = R2.conv_stashes(eng, N, S, Hc)
        pinned, far, n_diff = R2.conv_pinned_oracle(xk, lab, post, act, S, st1, st2, kind)
        assert far < R2.KINK_CONV
        return G, pinned, n_diff

    for mode, kind, bkind in ((_hip.LOSS_PER_SAMPLE, "per_sample", None), (_hip.LOSS_MEAN_PROB, "mean_prob", "bnn"),
                              (_hip.LOSS_MEAN_LOGIT, "mean_logit", "ensemble")):
        G, pinned, n_diff = pinned_grad(x, mode, kind)
        bound = torch.full((N,), TOL, dtype=torch.float64)
        if bkind is not None:
            bound = torch.clamp(2.0 ** -23 * cancellation_condition(x, lab, post, "conv", act, S, bkind), min=TOL)
            canc = max(canc, int((bound > TOL).sum()))
            assert int((bound > TOL).sum()) <= max(1, N // 100)
        err = R2.per_point_err(G, pinned)
        assert not bool((err > bound).any()), f"{tag} {kind}: {float((err / bound).max()):.3f} x the bound (pinned oracle)"
        worst = max(worst, float(err[bound <= TOL].max()))
        plain = (O.loss_gradients(xd, y, p64, "conv", act, S) if kind == "per_sample"
                 else O.meanprob_gradients(xd, lab, p64, "conv", act, S, kind=bkind))
        e_plain = R2.per_point_err(G, plain)
        assert not ((e_plain >= bound) & (n_diff == 0)).any(), f"{tag} {kind}: points differ from plain fp64 without a flipped decision"
        flipped = max(flipped, int((n_diff > 0).sum()))
        if kind == "per_sample":
            e = R2.per_point_err(eng.loss_gradients(x, y, S).cpu(), plain)
            assert not ((e >= TOL) & (n_diff == 0)).any(), f"{tag}: loss_gradients"
            continue
        adv = eng.fgsm(x, y, S, 0.1, mode=mode)
        marg = max(marg, E._check_attack(adv, x, 0.1, plain, (e_plain < TOL) & (n_diff == 0), f"{tag} fgsm {kind}"))

    def ref_grad(xk):
        G, pinned, n_diff = pinned_grad(xk, _hip.LOSS_MEAN_PROB, "mean_prob")
        return pinned.reshape(xk.shape), (n_diff == 0) & (R2.per_point_err(G, pinned) < TOL)
    w2, m2 = _pgd_and_evaluate(eng, "conv", act, x, y, post, S, ref_grad)
    return max(worst, w2), flipped, canc, max(marg, m2)


def _engine(arch, act, shape, H, C, post, precision=None):
    return E._engine(arch, act, shape, H, C, post, precision=precision)


def _all_modes(arch, act, shape, H, C, S, x, y, post, scaled, tag, checks, modes=("triple", "split")):
    """auto on the rescaled posterior, then each explicit mode: meets the same bar or raises HipError.  Returns auto's precision."""
    from robustbnns_amd import _hip
    eng = _engine(arch, act, shape, H, C, scaled)
    res = checks(eng, f"{tag} auto")
    _line(f"{tag} auto", eng.precision, *res, x.shape[0])
    for mode in modes:
        try:
            e = _engine(arch, act, shape, H, C, scaled, precision=mode)
        except _hip.HipError:
            print(f"[rescale {tag} {mode}] refused (HipError)")
            continue
        _line(f"{tag} {mode}", e.precision, *checks(e, f"{tag} {mode}"), x.shape[0])
    return eng.precision


# ------------------------------------------------------------------ R. rescaled posteriors
FC_CASES = [  # arch, act, how, shape, H, C, S, N, std
    ("fc", "relu", "units", (1, 28, 28), 256, 10, 2, 24, 0.05), ("fc", "leaky", "sample", (1, 28, 28), 256, 10, 2, 24, 0.05),
    ("fc2", "leaky", "layer1", (1, 28, 28), 256, 10, 2, 24, 0.05), ("fc2", "relu", "layer2", (1, 28, 28), 256, 10, 2, 24, 0.05),
]


@pytest.mark.parametrize("alpha", ALPHAS, ids=_log2)
@pytest.mark.parametrize("arch,act,how,shape,H,C,S,N,std", FC_CASES)
def test_fc_results_do_not_change_under_rescaling(arch, act, how, shape, H, C, S, N, std, alpha):
    D = int(np.prod(shape))
    post = O.synthetic_posterior(arch, D, H, C, S, std)
    x, y = O.synthetic_inputs(N, shape, C, seed=D + H + N)
    scaled = rescale(post, arch, how, alpha)
    tag = f"R {arch} {act} {how}: {'units 3..18 of ' if how != 'sample' else ''}sample 0, alpha {_log2(alpha)}"
    got = _all_modes(arch, act, shape, H, C, S, x, y, post, scaled, tag,
                     lambda eng, t: _fc_checks(eng, arch, act, x, y, post, S, t))
    assert got == ("triple" if alpha < 2 ** 12 else "exact")


CONV_CASES = [  # act, how, shape, Hc, C, S, N, std
    ("leaky", "conv1", (1, 28, 28), 16, 10, 2, 8, 0.05), ("relu", "conv2", (1, 28, 28), 16, 10, 2, 8, 0.05),
    ("relu", "conv1", (3, 32, 32), 16, 10, 2, 6, 0.05), ("leaky", "conv2", (3, 32, 32), 16, 10, 2, 6, 0.05),
]


@pytest.mark.parametrize("alpha", [2.0 ** 8, 2.0 ** 16, 2.0 ** 24, 2.0 ** 30], ids=_log2)
@pytest.mark.parametrize("act,how,shape,Hc,C,S,N,std", CONV_CASES)
def test_conv_results_do_not_change_under_rescaling(act, how, shape, Hc, C, S, N, std, alpha):
    post = E._conv_post(shape, Hc, C, S, std)
    x, y = O.synthetic_inputs(N, shape, C, seed=Hc + N + 7)
    scaled = rescale(post, "conv", how, alpha, units=5)
    tag = f"R conv {act} {shape} {how}: channel 5 of sample 0, alpha {_log2(alpha)}"
    got = _all_modes("conv", act, shape, Hc, C, S, x, y, post, scaled, tag,
                     lambda eng, t: _conv_checks(eng, act, x, y, post, S, Hc, t))
    assert got == ("triple" if alpha < 2 ** 12 else "exact")


@pytest.mark.parametrize("alpha", [2.0 ** 8, 2.0 ** 24], ids=_log2)
@pytest.mark.parametrize("arch", ["fc", "conv"])
def test_rescaled_svi_guides_on_the_drawn_weights(arch, alpha):
    """A guide whose loc and sigma are rescaled block-wise: the guard decides on the guide's bounds at load (no sync in a redraw); the kernels
    are held to fp64 on the weights that were actually drawn (reading the stack materialises them)."""
    from robustbnns_amd.conv import ConvEngine, ConvStackedPosterior, ConvSviGuide
    from robustbnns_amd.posterior import StackedPosterior, SviGuide
    from robustbnns_amd import AttackEngine
    S, C, act = 2, 10, "leaky"
    if arch == "conv":
        shape, H, N = (1, 28, 28), 16, 8
        base = E._conv_post(shape, H, C, 1, 0.05)
    else:
        shape, H, N = (1, 28, 28), 256, 24
        base = O.synthetic_posterior("fc", 784, H, C, 1, 0.05)
    loc = {k: v[0] for k, v in base.items()}
    scl = {k: torch.full_like(v, -4.0) for k, v in loc.items()}
    loc, scl = rescale_guide(loc, scl, arch, alpha, units=5 if arch == "conv" else slice(3, 19))
    if arch == "conv":
        post = ConvStackedPosterior.for_guide(ConvSviGuide(loc, scl, DEV), act, shape, C, H, S)
        eng = ConvEngine(post)
    else:
        post = StackedPosterior.for_guide(SviGuide(loc, scl, "fc", DEV), act, shape, C, S)
        eng = AttackEngine(post)
    assert eng.precision == ("triple" if alpha < 2 ** 12 else "exact")
    if eng.precision == "triple":
        post.triple_images()
    post.redraw(0x5EED, 3)
    keys = list(base)
    drawn = {k: torch.stack([post.state_dict(i)[k] for i in range(S)]) for k in keys}
    x, y = O.synthetic_inputs(N, shape, C, seed=N + 11)
    tag = f"R svi {arch} {act}: loc and sigma of {'conv2 channel 5' if arch == 'conv' else 'units 3..18'}, alpha {_log2(alpha)}"
    if arch == "conv":
        res = _conv_checks(eng, act, x, y, drawn, S, H, tag)
    else:
        res = _fc_checks(eng, "fc", act, x, y, drawn, S, tag)
    _line(tag, eng.precision, *res, N)


@pytest.mark.parametrize("kind", ["lowdim", "exact"])
def test_rescaling_controls(kind):
    """lowdim (D <= 16: fp32 FMA, no images) and precision="exact" hold the bar as they are, at the largest alpha."""
    arch, act, alpha = "fc", "leaky", ALPHAS[-1]
    if kind == "lowdim":
        shape, H, C, S, N, std = (1, 16, 1), 64, 2, 4, 64, 0.3
    else:
        shape, H, C, S, N, std = (1, 28, 28), 256, 10, 2, 24, 0.05
    D = int(np.prod(shape))
    post = O.synthetic_posterior(arch, D, H, C, S, std)
    x, y = O.synthetic_inputs(N, shape, C, seed=D + 1)
    eng = _engine(arch, act, shape, H, C, rescale(post, arch, "units", alpha), precision=None if kind == "lowdim" else "exact")
    assert eng.precision == kind
    tag = f"R control {kind} units: units 3..18 of sample 0, alpha {_log2(alpha)}"
    _line(tag, eng.precision, *_fc_checks(eng, arch, act, x, y, post, S, tag), N)


# ------------------------------------------------------------------ X. where auto now falls back
@pytest.mark.parametrize("arch,H,precision", [("fc", 384, "exact"), ("fc", 640, "exact"), ("fc2", 384, "exact"), ("fc2", 640, "exact"),
                                              ("fc", 384, None), ("fc2", 640, None)])
def test_exact_runs_every_hidden_size_triple_takes(arch, H, precision):
    """hidden 384 / 640 (k * 128, not a power of two or k * 512): the fp32 kernels' 128-unit tile walks H; exact against fp64, and auto (triple)
    on the same posterior."""
    shape, C, S, N, std = (1, 28, 28), 10, 3, 40, 0.05
    post = O.synthetic_posterior(arch, 784, H, C, S, std)
    x, y = O.synthetic_inputs(N, shape, C, seed=H + 5)
    eng = _engine(arch, "leaky", shape, H, C, post, precision=precision)
    assert eng.precision == (precision or "triple")
    tag = f"X {arch} leaky H={H} {eng.precision}"
    _line(tag, eng.precision, *_fc_checks(eng, arch, "leaky", x, y, post, S, tag), N)


@pytest.mark.parametrize("C", [11, 12, 13, 16])
@pytest.mark.parametrize("arch", ["fc", "fc2"])
def test_fc_more_than_ten_classes(arch, C):
    """11..16 classes: auto resolves to exact (fc_grad_kernel with CQ = 3 at C = 11, 12 and CQ = 4 at 13, 16)."""
    shape, H, S, N, std = (1, 28, 28), 128, 3, 40, 0.05
    post = O.synthetic_posterior(arch, 784, H, C, S, std)
    x, y = O.synthetic_inputs(N, shape, C, seed=C + 3)
    eng = _engine(arch, "leaky", shape, H, C, post)
    assert eng.precision == "exact"
    tag = f"X {arch} leaky H={H} C={C}"
    _line(tag, eng.precision, *_fc_checks(eng, arch, "leaky", x, y, post, S, tag), N)


@pytest.mark.parametrize("precision", [None, "exact"])
@pytest.mark.parametrize("C,shape", [(11, (1, 28, 28)), (12, (3, 32, 32)), (13, (1, 28, 28)), (16, (3, 32, 32))])
def test_conv_more_than_ten_classes(C, shape, precision):
    Hc, S, N = 16, 2, 8
    post = E._conv_post(shape, Hc, C, S, 0.05)
    x, y = O.synthetic_inputs(N, shape, C, seed=C + 9)
    eng = _engine("conv", "leaky", shape, Hc, C, post, precision=precision)
    assert eng.precision == (precision or "triple")
    tag = f"X conv leaky {shape} Hc={Hc} C={C} {eng.precision}"
    _line(tag, eng.precision, *_conv_checks(eng, "leaky", x, y, post, S, Hc, tag), N)


@pytest.mark.parametrize("arch,C,precision", [("fc", 16, None), ("fc", 13, None), ("fc2", 16, None), ("fc2", 13, None),
                                              ("conv", 16, None), ("conv", 13, "exact")])
def test_autograd_hook_with_more_than_ten_classes(arch, C, precision):
    """The hook (UPSTREAM / UPSTREAM_LOGIT) against an fp64 vector-Jacobian product: C = 16 has no padding class, C = 13 has three that carry NaN
    in G_up and must leave the result bit-identical (test_hip_edges C)."""
    shape, S, N, std = (1, 28, 28), 2, 16, 0.05
    H = 32 if arch == "conv" else 128
    post = E._conv_post(shape, H, C, S, std) if arch == "conv" else O.synthetic_posterior(arch, 784, H, C, S, std)
    E.hook_checks(arch, "leaky", shape, H, C, S, N, post, precision or ("triple" if arch == "conv" else "exact"))
