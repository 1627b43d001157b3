"""The fp64 checker of the conv nets on the MI355X (rbnn_conv_fp64.inc, conv_fp64.ConvFp64Engine) against the fp64 oracle.

The bar, per row: gradients max_d |gpu - cpu64| <= 1e-12 * max_d |cpu64|; probabilities 1e-12 absolute; logits 1e-12 * max |z| of the
point.  Where it comes from: the oracle's own fp64 result moves by <= 2.6e-15 (cases 1-5) and <= 2.2e-14 (case 6) when the 32 conv1
channels and the Hc conv2 channels are permuted (the same function summed in another order), an fp32 evaluation sits >= 1.4e-8
(probabilities) / >= 2e-7 (everything else) away — the bar is ~50x above the reference's own worst spread and more than 1e4x below what
ONE fp32 operation anywhere in the path would cost.  Every parity case recomputes that permuted-order spread and asserts it is <= 1e-13.
The smallest pool gap / kink margin over the cases is 1.1e-7: fp64 rounding cannot flip an argmax or an activation's side there.
Every test here fails on a tree without the checker (the module, the class and the three C names do not exist there)."""
import pytest
import torch

from oracle import bnn_oracle as O
from robustbnns_amd import _hip
from robustbnns_amd.conv import ConvEngine, ConvStackedPosterior, conv_geometry
from robustbnns_amd.conv_fp64 import ConvFp64Engine, kink_margin
from robustbnns_amd.engine import LOSS_MEAN_LOGIT, LOSS_MEAN_PROB

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("built_library")]

BAR, SPREAD = 1e-12, 1e-13
#        act      input shape   Hc  C   S  S_total N  std
CASES = {1: ("leaky", (1, 28, 28), 16, 10, 3, 5, 5, 0.05),          # one channel tile; a 5-sample stack (the seeds case)
         2: ("tanh", (1, 28, 28), 48, 7, 2, 2, 3, 0.05),            # Hc ragged against 32 and against the four waves
         3: ("sigm", (1, 28, 28), 32, 2, 2, 2, 3, 0.05),            # C = 2
         4: ("relu", (3, 32, 32), 32, 10, 2, 2, 3, 0.03),           # ragged position tiles: 100 and 196
         5: ("relu", (1, 28, 28), 80, 16, 1, 1, 1, 0.05),           # S = N = 1, C = 16
         6: ("tanh", (1, 28, 28), 16, 10, 2, 2, 3, 0.3),            # saturated, max prob 0.99
         # with 1 .. 6 every (activation, geometry) instantiation of the backward runs: the three that 4 leaves out at 3x32x32
         7: ("leaky", (3, 32, 32), 16, 10, 1, 1, 2, 0.03),
         8: ("tanh", (3, 32, 32), 16, 10, 1, 1, 2, 0.03),
         9: ("sigm", (3, 32, 32), 16, 10, 1, 1, 2, 0.03),
         10: ("relu", (3, 32, 32), 80, 10, 1, 1, 2, 0.03)}          # as 5 at the other geometry: five channel tiles on four waves (a second, ragged
                                                                    # round of the forward), six chunks of the backward
_cache = {}


def _np2(shape):
    return conv_geometry(shape)[1] ** 2


def case(i):
    """(act, shape, C, Hc, fp32 posterior, x, y one-hot) of a case, built once."""
    if i not in _cache:
        act, shape, Hc, C, S, S_total, N, std = CASES[i]
        post = O.synthetic_posterior("conv", shape[0] * shape[1] * shape[2], Hc, C, S_total, std, shape[0], head=_np2(shape) * Hc)
        x, y = O.synthetic_inputs(N, shape, C, seed=10 + i)
        _cache[i] = (act, shape, C, Hc, post, x, y)
    return _cache[i]


def engine(i):
    act, shape, C, Hc, post, x, y = case(i)
    return ConvFp64Engine(ConvStackedPosterior(act, shape, C, Hc, post, "cuda:0"))


def _oracle(xd, y, p64, act, S):
    lab = y.argmax(-1)
    return {"probs": O.bnn_forward(xd, p64, "conv", act, S),
            "logits": O.nn_logits(xd, p64, "conv", act).mean(0),
            "per_sample": O.loss_gradients(xd, y, p64, "conv", act, S),
            "mean_prob": O.meanprob_gradients(xd, lab, p64, "conv", act, S),
            "mean_logit": O._input_grad(xd, lab, p64, "conv", act, "mean_logit")}


def reference(i, seeds=None):
    """The five fp64 oracle results of a case for its used samples, computed once per (case, seeds) and left unchanged."""
    key = ("ref", i, None if seeds is None else tuple(seeds))
    if key not in _cache:
        act, shape, C, Hc, post, x, y = case(i)
        S = CASES[i][4] if seeds is None else len(seeds)
        p64 = O.cast(O.select(post, range(S) if seeds is None else seeds), torch.float64)
        _cache[key] = _oracle(x.double(), y, p64, act, S)
    return _cache[key]


def _permuted(p64, shape, gen):
    """The same function with the 32 conv1 channels and the Hc conv2 channels in another order: model.3.weight's ci axis follows conv1's
    outputs, model.7.weight's [C, Hc, NP2] view follows conv2's."""
    q = {k: v.clone() for k, v in p64.items()}
    S, Hc = q["model.3.bias"].shape
    p1, p2 = torch.randperm(32, generator=gen), torch.randperm(Hc, generator=gen)
    q["model.0.weight"], q["model.0.bias"] = q["model.0.weight"][:, p1], q["model.0.bias"][:, p1]
    q["model.3.weight"] = q["model.3.weight"][:, :, p1][:, p2]
    q["model.3.bias"] = q["model.3.bias"][:, p2]
    Cn = q["model.7.bias"].shape[1]
    q["model.7.weight"] = q["model.7.weight"].reshape(S, Cn, Hc, _np2(shape))[:, :, p2].reshape(S, Cn, -1)
    return q


def row_err(a, b):
    """per row: max_d |a - b|, max_d |b|"""
    a, b = a.double().reshape(a.shape[0], -1).cpu(), b.reshape(b.shape[0], -1)
    return (a - b).abs().amax(1), b.abs().amax(1)


def assert_within(name, got, ref, bar, absolute=False):
    assert got.dtype == torch.float64, (name, got.dtype)
    err, scale = row_err(got, ref)
    rel = err if absolute else err / scale.clamp_min(1e-300)
    print(f"    {name}: worst row {float(rel.max()):.2e} ({float(rel.max() / bar):.3f} x the bar {bar:g})")
    assert float(rel.max()) <= bar, f"{name}: {int((rel > bar).sum())} of {rel.numel()} rows beyond {bar:g}, worst {float(rel.max()):.3e}"


def device_results(eng, x, y, S, seeds=None):
    return {"probs": eng.forward(x, S, seeds),
            "logits": eng.forward(x, S, seeds, logits=True),
            "per_sample": eng.loss_gradients(x, y, S, seeds),
            "mean_prob": eng.attack_gradient(x, y, S, seeds, mode=LOSS_MEAN_PROB).reshape(x.shape),
            "mean_logit": eng.attack_gradient(x, y, S, seeds, mode=LOSS_MEAN_LOGIT).reshape(x.shape)}


ABSOLUTE = {"probs"}


@pytest.mark.parametrize("i,seeds", [(i, None) for i in sorted(CASES)] + [(1, (4, 0, 2))], ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_parity_with_the_fp64_oracle(i, seeds):
    act, shape, C, Hc, post, x, y = case(i)
    S = CASES[i][4] if seeds is None else len(seeds)
    ref = reference(i, seeds)
    # the condition of the bar: the reference's own permuted-order spread on THIS case is a tenth of the bar at most
    p64 = O.cast(O.select(post, range(S) if seeds is None else seeds), torch.float64)
    again = _oracle(x.double(), y, _permuted(p64, shape, torch.Generator().manual_seed(1000 + i)), act, S)
    for name in ref:
        err, scale = row_err(again[name], ref[name])
        spread = float((err if name in ABSOLUTE else err / scale.clamp_min(1e-300)).max())
        print(f"    [reference's own spread] {name}: {spread:.2e}")
        assert spread <= SPREAD, (name, spread)
    got = device_results(engine(i), x, y, S, None if seeds is None else list(seeds))
    torch.cuda.synchronize()
    for name in ref:
        assert_within(f"case {i} {name}", got[name], ref[name], BAR, absolute=name in ABSOLUTE)
    assert got["probs"].shape == (x.shape[0], C) and got["per_sample"].shape == x.shape


def test_norms_are_fp64_norms_of_the_fp64_gradient():
    act, shape, C, Hc, post, x, y = case(1)
    g, linf, l2 = engine(1).loss_gradients(x, y, 3, norms=True)
    ref = reference(1)["per_sample"].reshape(x.shape[0], -1)
    assert g.dtype == linf.dtype == l2.dtype == torch.float64
    assert float(((linf.cpu() - ref.abs().amax(1)).abs() / ref.abs().amax(1)).max()) <= BAR
    assert float(((l2.cpu() - ref.norm(dim=1)).abs() / ref.norm(dim=1)).max()) <= BAR
    assert torch.equal(linf, g.reshape(x.shape[0], -1).abs().amax(1))            # the maximum of the written values, exactly


# ---------------------------------------------------------------------------------------------------------------- exact integers
def _conv_int(h, w, b):
    """Conv2d(5) on int64 tensors."""
    return torch.einsum("ncyxij,ocij->noyx", h.unfold(2, 5, 1).unfold(3, 5, 1), w) + b.view(1, -1, 1, 1)


def _pool_int(h, stride):
    return h.unfold(2, 2, stride).unfold(3, 2, stride).amax((-1, -2))


def _integer_net(shape, Hc, C, S, N, seed):
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g)
    w = {"model.0.weight": ri(-2, 2, S, 32, shape[0], 5, 5), "model.0.bias": ri(-2, 2, S, 32),
         "model.3.weight": ri(-2, 2, S, Hc, 32, 5, 5), "model.3.bias": ri(-2, 2, S, Hc),
         "model.7.weight": ri(-2, 2, S, C, _np2(shape) * Hc), "model.7.bias": ri(-2, 2, S, C)}
    return w, ri(0, 3, N, *shape), g


def _logits_int(w, X, s):
    h = _pool_int(torch.relu(_conv_int(X, w["model.0.weight"][s], w["model.0.bias"][s])), 2)
    h = _pool_int(torch.relu(_conv_int(h, w["model.3.weight"][s], w["model.3.bias"][s])), 1)
    z = h.flatten(1) @ w["model.7.weight"][s].T + w["model.7.bias"][s]
    assert int(z.abs().max()) < 2 ** 53 and z.dtype == torch.int64
    return z


@pytest.mark.parametrize("shape,N", [((1, 28, 28), 2), ((3, 32, 32), 3)], ids=["1x28x28", "3x32x32"])
def test_exact_integers_catch_a_wrong_fragment_map_or_tap_order(shape, N):
    """Integer data: every product and every sum is exact in fp64, so the logits EQUAL the int64 conv / pool / linear result — at any
    tolerance a wrong C/D row map, tap order or routing fails this.  Hc = 48: three channel tiles on four waves.  The backward: integer dZ
    through the C entry point; G equals torch's float64 autograd of the same net (every term an integer; equal positive values in a window
    do occur, so the first-maximum rule is in the comparison)."""
    Hc, C, S = 48, 10, 2
    w, X, g = _integer_net(shape, Hc, C, S, N, seed=5)
    post = ConvStackedPosterior("relu", shape, C, Hc, {k: v.float() for k, v in w.items()}, "cuda:0")
    eng = ConvFp64Engine(post)
    zs = [_logits_int(w, X, s) for s in range(S)]
    for s in range(S):
        got = eng.forward(X.float(), 1, seeds=[s], logits=True).cpu()
        assert got.dtype == torch.float64 and torch.equal(got, zs[s].double()), (s, (got - zs[s].double()).abs().max())
    both = eng.forward(X.float(), 2, logits=True).cpu()                        # the mean of two integers is exact as well
    assert torch.equal(both * 2, (zs[0] + zs[1]).double())
    # backward
    k, Xd = eng.k, X.float().reshape(N, -1).to("cuda:0").contiguous()
    ws = eng.fp64.workspace(N, S)
    k.conv_forward_fp64(post, Xd, None, S, _hip.OUT_LOGITS, ws)
    dZ = torch.zeros(S, N, 16, dtype=torch.float64)
    dZ[:, :, :C] = torch.randint(-3, 4, (S, N, C), generator=g).double()
    ws["dZ"].copy_(dZ.reshape(-1))
    G = torch.empty(N, Xd.shape[1], dtype=torch.float64, device="cuda:0")
    k.conv_input_grad_fp64(post, None, S, N, ws, 1.0, G)
    xr = X.double().requires_grad_(True)
    (O.nn_logits(xr, {k_: v.double() for k_, v in w.items()}, "conv", "relu") * dZ[:, :, :C]).sum().backward()
    assert float(xr.grad.abs().max()) > 0 and torch.equal(xr.grad, xr.grad.round())
    assert torch.equal(G.cpu().reshape(X.shape), xr.grad), float((G.cpu().reshape(X.shape) - xr.grad).abs().max())


# ---------------------------------------------------------------------------------------------------------------- bit identity
def test_bit_identical_runs_rows_and_point_blocks(monkeypatch):
    """Case 1: two runs agree bit for bit; rows 2..4 run alone equal their rows of the N = 5 run; with the workspace budget so low that every
    block is one point the bits stay; canaries behind every workspace buffer stay intact."""
    act, shape, C, Hc, post, x, y = case(1)
    S = 3
    a = device_results(engine(1), x, y, S)
    b = device_results(engine(1), x, y, S)
    for name in a:
        assert torch.equal(a[name], b[name]), name
    part = device_results(engine(1), x[2:5], y[2:5], S)
    for name in a:
        assert torch.equal(part[name], a[name][2:5]), name
    monkeypatch.setenv("RBNN_FP64_WS_GB", "1e-6")
    eng = engine(1)
    assert eng.point_block(S) == 1 and eng.point_blocks(5, S) == [(i, i + 1) for i in range(5)]
    guard, held = 64, []

    def with_canary(n_bytes, dtype=torch.float64):
        n = n_bytes // (8 if dtype == torch.float64 else 1)
        t = torch.full((n + guard,), 123, dtype=dtype, device="cuda:0")
        held.append((t, n))
        return t[:n]
    monkeypatch.setattr(eng.fp64, "buffer", with_canary)
    c = device_results(eng, x, y, S)
    gn = eng.loss_gradients(x, y, S, norms=True)
    torch.cuda.synchronize()
    for name in a:
        assert torch.equal(c[name], a[name]), name
    assert torch.equal(gn[0], a["per_sample"])
    assert len(held) == _hip.CONV_FP64_WS_BUFFERS                              # one cached workspace of one point: every buffer once
    for t, n in held:
        assert bool((t[n:] == 123).all()), "a kernel wrote behind its workspace buffer"


# ---------------------------------------------------------------------------------------------------------------- attacks
def _no_marginal_pixels(g64):
    """The chosen inputs leave no pixel whose gradient is within 1e-9 of the row maximum of zero without being zero (the sign of such a pixel is
    not the oracle's to decide): the cap on excluded pixels is 0."""
    g = g64.reshape(g64.shape[0], -1).abs()
    return int(((g > 0) & (g < 1e-9 * g.amax(1, keepdim=True))).sum()) == 0


@pytest.mark.parametrize("i", [1, 4])
def test_fgsm_takes_the_sign_of_the_fp64_gradient(i):
    act, shape, C, Hc, post, x, y = case(i)
    S = CASES[i][4]
    g64 = reference(i)["mean_prob"]
    assert _no_marginal_pixels(g64)
    adv = engine(i).fgsm(x, y, S, 0.3)
    assert adv.dtype == torch.float32 and adv.shape == x.shape
    assert torch.equal(adv.cpu(), torch.clamp(x + 0.3 * g64.sign().float(), 0, 1))


@pytest.mark.parametrize("i,alpha", [(1, None), (4, 2 / 225)])
def test_pgd_iterates_equal_the_restated_step(i, alpha):
    """Three iterations; every iterate bit-equal to the restated step: the fp64 oracle gradient AT the fp32 iterate, its sign, then the
    reference's three fp32 lines (adversarialAttacks.py:103-105).  alpha None: 2 / max(image) per image (:89)."""
    act, shape, C, Hc, post, x, y = case(i)
    S, eps = CASES[i][4], 0.3
    p64, lab = O.cast(O.select(post, range(S)), torch.float64), y.argmax(-1)
    a = alpha if alpha is not None else (2 / x.reshape(x.shape[0], -1).max(dim=1)[0]).reshape(-1, 1, 1, 1)
    eng = engine(i)
    xi = x.clone()
    for it in range(1, 4):
        g64 = O.meanprob_gradients(xi.double(), lab, p64, "conv", act, S)
        assert _no_marginal_pixels(g64)
        pert = xi + a * g64.sign().float()
        eta = torch.clamp(pert - x, min=-eps, max=eps)
        xi = torch.clamp(x + eta, min=0, max=1)
        got = eng.pgd(x, y, S, eps, alpha=alpha, iters=it)
        assert got.dtype == torch.float32 and torch.equal(got.cpu(), xi), (it, int((got.cpu() != xi).sum()))


# ---------------------------------------------------------------------------------------------------------------- the checker in use
def test_exact_and_triple_sit_within_the_bar_of_the_device_fp64_result():
    """The checker in use as the oracle: the loss_gradients of the fp32-MFMA and of the triple conv kernels lie within the project's 1e-5 bar
    (per row, of the row maximum) of the device fp64 result on the rows whose fp64 margin (conv_fp64.kink_margin: pool gaps and the
    pre-activation at every window's maximum) exceeds the 2e-6 kink rule of test_hip_parity.py; at most 10 % of the rows may be excluded.

    The size follows from those two conditions together (fp64 oracle margins and fp32 torch contractions; profiles/fp64_conv/README.md):
      - The 2e-6 rule is absolute.  It covers an fp32 pre-activation's rounding only while conv2's pre-activations (800-term sums) stay
        around 1: at std 0.05 max |a2| = 0.76 and an fp32 contraction of a2 is off by <= 1.6e-6, at std 0.1 max |a2| = 3 and it is off by
        6e-6 — rows 5e-6 from a kink then flip (measured: 8 kept rows of 64 beyond the bar, up to 14e-5).  So conv2 stays at std 0.05's scale.
      - At that scale a point has 4608 conv1 + 49 Hc conv2 windows per sample and the rule excludes 49 of 64 rows at Hc = 128, S = 4,
        16 to 25 at S = 1, and still 10 to 16 at Hc = 16, S = 1 (conv1's windows alone: ~17 %), whatever the seed.
    Hence one sample, Hc = 32, and the std-0.05 posterior with conv1 scaled by 8 and conv2's weights by 1/8: the SAME function (leaky is
    positively homogeneous, powers of two are exact) whose conv1 pre-activations and pool gaps are 8x further from their kinks in absolute
    terms (max |a1| = 4.7, fp32 error of its 25-term sums <= 9.1e-7).  Seeds 0 .. 15 then exclude 1 to 9 rows of 64; seed 0 excludes 3."""
    shape, Hc, C, S, N = (1, 28, 28), 32, 10, 1, 64
    post = O.synthetic_posterior("conv", 784, Hc, C, S, 0.05, 1, head=49 * Hc)
    post["model.0.weight"], post["model.0.bias"], post["model.3.weight"] = post["model.0.weight"] * 8, post["model.0.bias"] * 8, post["model.3.weight"] / 8
    x, y = O.synthetic_inputs(N, shape, C, seed=0)
    cp = ConvStackedPosterior("leaky", shape, C, Hc, post, "cuda:0")
    g64 = ConvFp64Engine(cp).loss_gradients(x, y, S)
    assert g64.dtype == torch.float64
    keep = (kink_margin(cp, x, S) > 2e-6).cpu()
    print(f"    rows excluded by the 2e-6 kink rule: {int((~keep).sum())} of {N}")
    assert int((~keep).sum()) <= N // 10
    for precision in ("exact", "triple"):
        eng = ConvEngine(cp, precision=precision)
        assert eng.precision == precision
        g = eng.loss_gradients(x, y, S)
        err, scale = row_err(g, g64.cpu())
        rel = err / scale
        print(f"    {precision}: worst kept row {float(rel[keep].max() / 1e-5):.3f} x 1e-5, worst row {float(rel.max() / 1e-5):.3f} x 1e-5 "
              "from the device fp64 result")
        assert g.dtype == torch.float32 and float(rel[keep].max()) <= 1e-5


def test_refusals_on_the_device():
    """What the checker does not cover is refused, not answered in fp32: an input with requires_grad, a CPU posterior, an upstream mode."""
    act, shape, C, Hc, post, x, y = case(1)
    eng = engine(1)
    with pytest.raises(_hip.HipError, match="fp64.*requires_grad"):
        eng.forward(x.clone().requires_grad_(True), 3)
    with pytest.raises(_hip.HipError, match="fp64.*requires_grad"):
        eng.loss_gradients(x.clone().requires_grad_(True), y, 3)
    with pytest.raises(_hip.HipError, match="fp64.*CPU device"):
        ConvFp64Engine(ConvStackedPosterior(act, shape, C, Hc, post, "cpu"))
    for mode in (_hip.LOSS_UPSTREAM, _hip.LOSS_UPSTREAM_LOGIT):
        with pytest.raises(_hip.HipError, match="fp64.*upstream"):
            eng.attack_gradient(x, y, 3, mode=mode)
        with pytest.raises(_hip.HipError, match="fp64.*upstream"):
            eng.fgsm(x, y, 3, 0.3, mode=mode)
