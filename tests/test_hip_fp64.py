"""The fp64 precision mode on the MI355X (rbnn_fp64.inc) against the fp64 oracle.

The bar, per row: gradients max_d |gpu - cpu64| <= 1e-12 * max_d |cpu64|; probabilities 1e-12 absolute; logits 1e-12 * max |z| of the
point.  Where it comes from: the oracle's own fp64 result moves by <= 8.2e-15 of the row maximum when input features and hidden units are
permuted (the same function summed in another order), an fp32 evaluation sits >= 3.1e-7 away — the bar is ~120x above the reference's own
spread and 3e5x below what ONE fp32 operation anywhere in the path would cost.  Every parity case recomputes that permuted-order spread
and asserts it is <= 1e-13, a tenth of the bar, so the reference alone stays well inside it.
Every test here fails on a tree without the mode (precision='fp64' is a ValueError there)."""
import pytest
import torch

from oracle import bnn_oracle as O
from robustbnns_amd import AttackEngine, StackedPosterior, _hip
from robustbnns_amd.engine import LOSS_MEAN_LOGIT, LOSS_MEAN_PROB

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("built_library")]

BAR, SPREAD = 1e-12, 1e-13
#        arch   act      input shape   H    C   S  S_total N   std
CASES = {1: ("fc", "leaky", (1, 28, 28), 128, 10, 5, 5, 33, 0.05),
         2: ("fc", "tanh", (1, 10, 5), 40, 7, 3, 3, 17, 1.0),          # saturated; ragged Hp
         3: ("fc", "sigm", (1, 2, 1), 16, 2, 3, 3, 17, 1.0),
         4: ("fc2", "relu", (1, 28, 28), 128, 10, 3, 3, 17, 0.05),
         5: ("fc2", "sigm", (1, 3, 1), 16, 16, 5, 5, 33, 1.0),
         6: ("fc", "leaky", (3, 32, 32), 512, 10, 3, 3, 17, 0.03),
         7: ("fc2", "tanh", (1, 28, 28), 128, 10, 1, 1, 1, 0.05)}
_cache = {}


def _prod(shape):
    return int(torch.tensor(shape).prod())


def case(i):
    """(arch, act, shape, C, H, fp32 posterior, x, y one-hot) of a case, built once."""
    if i not in _cache:
        arch, act, shape, H, C, S, S_total, N, std = CASES[i]
        post = O.synthetic_posterior(arch, _prod(shape), H, C, S_total, std)
        x, y = O.synthetic_inputs(N, shape, C, seed=10 + i)
        _cache[i] = (arch, act, shape, C, H, post, x, y)
    return _cache[i]


def engine(i, precision="fp64"):
    arch, act, shape, C, H, post, x, y = case(i)
    return AttackEngine(StackedPosterior(arch, act, shape, C, H, post, "cuda:0"), precision=precision)


def reference(i, seeds=None):
    """The five fp64 oracle results of a case — mean probabilities, mean logits, the gradients of the three label losses — for its
    used samples, computed once per (case, seeds) and left unchanged."""
    key = ("ref", i, None if seeds is None else tuple(seeds))
    if key not in _cache:
        arch, act, shape, C, H, post, x, y = case(i)
        S = CASES[i][5] if seeds is None else len(seeds)
        p64 = O.cast(O.select(post, range(S) if seeds is None else seeds), torch.float64)
        _cache[key] = _oracle(x.double(), y, p64, arch, act, S)
    return _cache[key]


def _oracle(xd, y, p64, arch, act, S):
    lab = y.argmax(-1)
    return {"probs": O.bnn_forward(xd, p64, arch, act, S),
            "logits": O.nn_logits(xd, p64, arch, act).mean(0),
            "per_sample": O.loss_gradients(xd, y, p64, arch, act, S),
            "mean_prob": O.meanprob_gradients(xd, lab, p64, arch, act, S),
            "mean_logit": O._input_grad(xd, lab, p64, arch, act, "mean_logit")}


def _permuted(xd, p64, arch, gen):
    """The same function with input features and hidden units in another order: (x', posterior', inverse feature permutation)."""
    keys = ["model.1", "model.3"] + (["model.5"] if arch == "fc2" else [])
    D = p64["model.1.weight"].shape[-1]
    pd = torch.randperm(D, generator=gen)
    q = {k: v.clone() for k, v in p64.items()}
    q["model.1.weight"] = q["model.1.weight"][:, :, pd]
    for lo, hi in zip(keys[:-1], keys[1:]):                     # the hidden units between layer `lo` and layer `hi`
        ph = torch.randperm(q[lo + ".bias"].shape[-1], generator=gen)
        q[lo + ".weight"], q[lo + ".bias"], q[hi + ".weight"] = q[lo + ".weight"][:, ph, :], q[lo + ".bias"][:, ph], q[hi + ".weight"][:, :, ph]
    inv = torch.empty_like(pd)
    inv[pd] = torch.arange(D)
    return xd.reshape(xd.shape[0], -1)[:, pd].reshape(xd.shape), q, inv


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
    D = eng.post.D
    return {"probs": eng.forward(x, S, seeds),
            "logits": eng.forward(x, S, seeds, logits=True),
            "per_sample": eng.loss_gradients(x, y, S, seeds),
            "mean_prob": eng.attack_gradient(x, y, S, seeds, mode=LOSS_MEAN_PROB)[:, :D].reshape(x.shape),
            "mean_logit": eng.attack_gradient(x, y, S, seeds, mode=LOSS_MEAN_LOGIT)[:, :D].reshape(x.shape)}


ABSOLUTE = {"probs"}


@pytest.mark.parametrize("i,seeds", [(i, None) for i in sorted(CASES)] + [(1, (4, 0, 2))], ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_parity_with_the_fp64_oracle(i, seeds):
    arch, act, shape, C, H, post, x, y = case(i)
    S = CASES[i][5] if seeds is None else len(seeds)
    ref = reference(i, seeds)
    # the condition of the bar: the reference's own permuted-order spread on THIS case is a tenth of the bar at most
    p64 = O.cast(O.select(post, range(S) if seeds is None else seeds), torch.float64)
    xq, q, inv = _permuted(x.double(), p64, arch, torch.Generator().manual_seed(1000 + i))
    again = _oracle(xq, y, q, arch, act, S)
    for name in ref:
        a = again[name]
        if name not in ("probs", "logits"):
            a = a.reshape(a.shape[0], -1)[:, inv].reshape(ref[name].shape)
        err, scale = row_err(a, ref[name])
        spread = float((err if name in ABSOLUTE else err / scale.clamp_min(1e-300)).max())
        print(f"    [reference's own spread] {name}: {spread:.2e}")
        assert spread <= SPREAD, (name, spread)
    got = device_results(engine(i), x, y, S, None if seeds is None else list(seeds))
    torch.cuda.synchronize()
    for name in ref:
        assert_within(f"case {i} {name}", got[name], ref[name], BAR, absolute=name in ABSOLUTE)
    assert got["probs"].shape == (x.shape[0], C) and got["per_sample"].shape == x.shape


def test_norms_are_fp64_norms_of_the_fp64_gradient():
    arch, act, shape, C, H, post, x, y = case(1)
    g, linf, l2 = engine(1).loss_gradients(x, y, 5, norms=True)
    ref = reference(1)["per_sample"].reshape(x.shape[0], -1)
    assert g.dtype == linf.dtype == l2.dtype == torch.float64
    assert float(((linf.cpu() - ref.abs().amax(1)).abs() / ref.abs().amax(1)).max()) <= BAR
    assert float(((l2.cpu() - ref.norm(dim=1)).abs() / ref.norm(dim=1)).max()) <= BAR
    assert torch.equal(linf, g.reshape(x.shape[0], -1).abs().amax(1))            # the maximum of the written values, exactly


def test_exact_integers_catch_a_wrong_fragment_map():
    """Integer data: every product and every sum is exact in fp64, so the logits EQUAL the int64 matrix products — at any tolerance a wrong
    C/D row map (the f32 formula on the f64 MFMA) fails this.  D = 21 (ragged D_pad), H = 40 (ragged tiles and K blocks), N = 19 (two tiles)."""
    shape, H, C, S, N = (1, 7, 3), 40, 7, 2, 19
    g = torch.Generator().manual_seed(5)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g)
    W1, b1, W2, b2 = ri(-2, 2, S, H, 21), ri(-2, 2, S, H), ri(-2, 2, S, C, H), ri(-2, 2, S, C)
    X = ri(0, 3, N, *shape)
    post = {"model.1.weight": W1.float(), "model.1.bias": b1.float(), "model.3.weight": W2.float(), "model.3.bias": b2.float()}
    eng = AttackEngine(StackedPosterior("fc", "relu", shape, C, H, post, "cuda:0"), precision="fp64")
    for s in range(S):
        hid = torch.relu(X.reshape(N, 21) @ W1[s].T + b1[s])
        z = hid @ W2[s].T + b2[s]                                              # int64
        got = eng.forward(X.float(), 1, seeds=[s], logits=True).cpu()
        assert got.dtype == torch.float64 and torch.equal(got, z.double()), (s, (got - z.double()).abs().max())
    both = eng.forward(X.float(), 2, logits=True).cpu()                        # the mean of two integers is exact as well
    zs = [torch.relu(X.reshape(N, 21) @ W1[s].T + b1[s]) @ W2[s].T + b2[s] for s in range(S)]
    assert torch.equal(both * 2, (zs[0] + zs[1]).double())


def test_bit_identical_runs_rows_and_point_blocks(monkeypatch):
    """Case 1: two runs agree bit for bit; rows 16..32 run alone equal their rows of the N = 33 run; with the workspace budget so low that
    every block is one 16-point tile the bits stay; canaries behind every fp64 workspace buffer stay intact."""
    arch, act, shape, C, H, post, x, y = case(1)
    S = 5
    a = device_results(engine(1), x, y, S)
    b = device_results(engine(1), x, y, S)
    for name in a:
        assert torch.equal(a[name], b[name]), name
    part = device_results(engine(1), x[16:33], y[16:33], S)
    for name in a:
        assert torch.equal(part[name], a[name][16:33]), name
    monkeypatch.setenv("RBNN_FP64_WS_GB", "1e-6")
    eng = engine(1)
    assert eng.fp64.point_block(S) == 16 and eng.fp64.point_blocks(33, S) == [(0, 16), (16, 32), (32, 33)]
    guard, held = 64, []

    def with_canary(n_bytes, dtype=torch.float64):
        t = torch.full((n_bytes // 8 + guard,), 12345.678, dtype=torch.float64, device="cuda:0")
        held.append((t, n_bytes // 8))
        return t[:n_bytes // 8]
    monkeypatch.setattr(eng.fp64, "buffer", with_canary)
    c = device_results(eng, x, y, S)
    gn = eng.loss_gradients(x, y, S, norms=True)
    torch.cuda.synchronize()
    for name in a:
        assert torch.equal(c[name], a[name]), name
    assert torch.equal(gn[0], a["per_sample"])
    assert len(held) == 2 * 4                                                  # blocks of 16 points and of 1 point: P, dZ, Psum, dact1 each
    for t, n in held:
        assert bool((t[n:] == 12345.678).all()), "a kernel wrote behind its workspace buffer"


def _no_marginal_pixels(g64):
    """The chosen inputs leave no pixel whose gradient is within 1e-9 of the row maximum of zero without being zero (the sign of such a pixel is
    not the oracle's to decide): the cap on excluded pixels is 0."""
    g = g64.reshape(g64.shape[0], -1).abs()
    return int(((g > 0) & (g < 1e-9 * g.amax(1, keepdim=True))).sum()) == 0


@pytest.mark.parametrize("i", [1, 4])
def test_fgsm_takes_the_sign_of_the_fp64_gradient(i):
    arch, act, shape, C, H, post, x, y = case(i)
    S = CASES[i][5]
    g64 = reference(i)["mean_prob"]
    assert _no_marginal_pixels(g64)
    adv = engine(i).fgsm(x, y, S, 0.3)
    assert adv.dtype == torch.float32 and adv.shape == x.shape
    assert torch.equal(adv.cpu(), torch.clamp(x + 0.3 * g64.sign().float(), 0, 1))


@pytest.mark.parametrize("i,alpha", [(1, None), (4, 2 / 225)])
def test_pgd_iterates_equal_the_restated_step(i, alpha):
    """Three iterations; every iterate bit-equal to the restated step: the fp64 oracle gradient AT the fp32 iterate, its sign, then the
    reference's three fp32 lines (adversarialAttacks.py:103-105).  alpha None: 2 / max(image) per image (:89)."""
    arch, act, shape, C, H, post, x, y = case(i)
    S, eps = CASES[i][5], 0.3
    p64, lab = O.cast(O.select(post, range(S)), torch.float64), y.argmax(-1)
    a = alpha if alpha is not None else (2 / x.reshape(x.shape[0], -1).max(dim=1)[0]).reshape(-1, 1, 1, 1)
    eng = engine(i)
    xi = x.clone()
    for it in range(1, 4):
        g64 = O.meanprob_gradients(xi.double(), lab, p64, arch, act, S)
        assert _no_marginal_pixels(g64)
        pert = xi + a * g64.sign().float()
        eta = torch.clamp(pert - x, min=-eps, max=eps)
        xi = torch.clamp(x + eta, min=0, max=1)
        got = eng.pgd(x, y, S, eps, alpha=alpha, iters=it)
        assert got.dtype == torch.float32 and torch.equal(got.cpu(), xi), (it, int((got.cpu() != xi).sum()))


def test_exact_and_triple_sit_within_the_bar_of_the_device_fp64_result():
    """The mode in use as the oracle at a size the CPU restatement is too slow for: fc-512, S = 8, N = 300.  The loss_gradients of the
    fp32-MFMA and of the triple kernels lie within the project's 1e-5 bar (per row, of the row maximum) of the device fp64 result."""
    shape, H, C, S, N = (1, 28, 28), 512, 10, 8, 300
    post = O.synthetic_posterior("fc", 784, H, C, S, 0.05)
    x, y = O.synthetic_inputs(N, shape, C, seed=3)
    sp = StackedPosterior("fc", "leaky", shape, C, H, post, "cuda:0")
    g64 = AttackEngine(sp, precision="fp64").loss_gradients(x, y, S)
    assert g64.dtype == torch.float64
    for precision in ("exact", "triple"):
        g = AttackEngine(sp, precision=precision).loss_gradients(x, y, S)
        err, scale = row_err(g, g64.cpu())
        print(f"    {precision}: worst row {float((err / scale).max() / 1e-5):.3f} x 1e-5 from the device fp64 result")
        assert g.dtype == torch.float32 and float((err / scale).max()) <= 1e-5


def test_refusals_on_the_device():
    """What the mode does not cover is refused on the device as well, not answered in fp32: the autograd hook, a conv posterior."""
    arch, act, shape, C, H, post, x, y = case(1)
    eng = engine(1)
    with pytest.raises(_hip.HipError, match="fp64"):
        eng.forward(x.clone().requires_grad_(True), 5)
    with pytest.raises(_hip.HipError, match="fp64"):
        from robustbnns_amd.conv import ConvEngine, ConvStackedPosterior
        cp = O.synthetic_posterior("conv", 784, 16, 10, 2, 0.05)
        ConvEngine(ConvStackedPosterior("leaky", (1, 28, 28), 10, 16, cp, "cuda:0"), precision="fp64")


def test_the_call_surface_inherits_the_mode_through_the_environment(monkeypatch):
    """RBNN_PRECISION=fp64 reaches BNN.forward, lossGradients.loss_gradient and expected_gradient_norms with no code of their own: float64
    results inside the bar of the oracle (case 1's posterior as a stored HMC posterior), fp32 images from the attack."""
    from robustbnns_amd import lossGradients as LG
    from robustbnns_amd.adversarialAttacks import fgsm_attack
    from robustbnns_amd.model_bnn import BNN
    arch, act, shape, C, H, post, x, y = case(1)
    S, ref = 5, reference(1)
    monkeypatch.setenv("RBNN_PRECISION", "fp64")
    bnn = BNN("mnist", H, act, arch, "hmc", None, None, S, 0, shape, C)
    bnn.set_posterior_samples(post, "cuda:0")
    assert_within("BNN.forward", bnn.forward(x, n_samples=S), ref["probs"], BAR, absolute=True)
    g0 = LG.loss_gradient(bnn, x[0], y[0], n_samples=S)
    assert_within("loss_gradient", g0.unsqueeze(0), ref["per_sample"][:1], BAR)
    norms, grads = LG.expected_gradient_norms(bnn, x, y, [S], "linfty")
    assert norms.dtype.name == "float64" and grads[0].dtype == torch.float64
    want = ref["per_sample"].reshape(x.shape[0], -1).abs().amax(1).numpy()
    assert float(abs(norms[:, 0] - want).max() / want.max()) <= BAR
    adv = fgsm_attack(bnn, x.to("cuda:0"), y.argmax(-1).to("cuda:0"), {"epsilon": 0.3}, n_samples=S)
    assert adv.dtype == torch.float32 and torch.equal(adv.cpu(), torch.clamp(x + 0.3 * ref["mean_prob"].sign().float(), 0, 1))
