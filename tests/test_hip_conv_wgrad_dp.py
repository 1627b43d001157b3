"""The fp64 weight gradients of the conv checker on the MI355X (rbnn_conv_wgrad_dp.inc, ConvFp64Engine.weight_gradients) against fp64
autograd on the CPU.

The bar, per tensor: max |gpu - cpu64| <= 1e-12 * max |cpu64|; per-point CE: 1e-12 * max(1, CE) — the bar of the two existing fp64
checkers (tests/test_hip_fp64.py, tests/test_hip_conv_fp64.py).  1x28x28: conv_restate.grad_case's reference (fp64 autograd of the mean CE);
3x32x32, which no trainer runs: an fp64 nn.Sequential restated here.  Every test fails on a tree without weight_gradients."""
import pytest
import torch
from torch import nn

import conv_restate as CR
from robustbnns_amd import _hip
from robustbnns_amd.conv import ConvStackedPosterior
from robustbnns_amd.conv_fp64 import ConvFp64Engine

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("built_library")]

DEV = "cuda:0"
BAR = 1e-12
# (80, ...): five channel tiles on four waves, a second, ragged round of the forward and six chunks of the backward; (16, "sigm", 2, 10): with it
# every (activation, geometry) instantiation of the backward runs
MNIST_CASES = CR.GRAD_CASES[:7] + [(144, "tanh", 129, 10), (48, "leaky", 500, 3), (80, "relu", 2, 10)]
CIFAR_CASES = [(16, "leaky", 5, 10), (32, "tanh", 3, 7), (48, "relu", 17, 10), (16, "sigm", 2, 10), (80, "leaky", 2, 10)]
_cache = {}


def stacked(params_list):
    return {k: torch.stack([p[k] for p in params_list]) for k in CR.KEYS}


def engine(act, shape, params_list):
    Hc, Cn = int(params_list[0]["model.3.bias"].shape[0]), int(params_list[0]["model.7.bias"].shape[0])
    return ConvFp64Engine(ConvStackedPosterior(act, shape, Cn, Hc, stacked(params_list), DEV))


def assert_tensors_within(name, grads, ce, ref_grad, ref_ce, row=0, scale=1.0, bar=BAR):
    """grads[k][row] against scale * ref_grad[k] for the six tensors, ce[row] against ref_ce; prints every figure before it asserts."""
    assert list(grads) == CR.KEYS
    worst = {}
    for k in CR.KEYS:
        g, r = grads[k], ref_grad[k] * scale
        assert g.dtype == torch.float64 and g.shape[1:] == r.shape, (k, g.dtype, g.shape, r.shape)
        worst[k] = float((g[row].cpu() - r).abs().max() / r.abs().max())
    assert ce.dtype == torch.float64
    e = float(((ce[row].cpu() - ref_ce).abs() / ref_ce.clamp_min(1.0)).max())
    print(f"    {name}: " + ", ".join(f"{k[6:]} {v / bar:.4f}" for k, v in worst.items()) + f", ce {e / bar:.4f}  (x the bar {bar:g})")
    assert max(worst.values()) <= bar, (name, worst)
    assert e <= bar, (name, e)


# ---------------------------------------------------------------------------------------------------------------- 1x28x28
@pytest.mark.parametrize("Hc,act,B,Cn", MNIST_CASES)
def test_mnist_geometry_matches_fp64_autograd(Hc, act, B, Cn):
    c = CR.grad_case(Hc, act, B, Cn)
    ref = c["ref"]
    eng = engine(act, CR.SHAPE, [c["params"]])
    gm, cem = eng.weight_gradients(c["x"], c["lab"], 1, reduction="mean")
    gs, ces = eng.weight_gradients(c["x"], c["lab"], 1)                     # "sum" is the default
    torch.cuda.synchronize()
    assert cem.shape == (1, B) and gm["model.3.weight"].shape == (1, Hc, 32, 5, 5) and gm["model.7.weight"].shape == (1, Cn, 49 * Hc)
    assert_tensors_within(f"Hc={Hc} {act} B={B} C={Cn} mean", gm, cem, ref["grad"], ref["ce"])
    assert_tensors_within(f"Hc={Hc} {act} B={B} C={Cn} sum", gs, ces, ref["grad"], ref["ce"], scale=float(B))
    assert torch.equal(cem, ces)                                            # the per-point CE is unscaled in both


# ---------------------------------------------------------------------------------------------------------------- 3x32x32
_ACT = {"relu": nn.ReLU, "leaky": nn.LeakyReLU, "sigm": nn.Sigmoid, "tanh": nn.Tanh}


def cifar_sequential(act, Hc, Cn, dtype):
    m = nn.Sequential(nn.Conv2d(3, 32, kernel_size=5), _ACT[act](), nn.MaxPool2d(kernel_size=2), nn.Conv2d(32, Hc, kernel_size=5), _ACT[act](),
                      nn.MaxPool2d(kernel_size=2, stride=1), nn.Flatten(), nn.Linear(81 * Hc, Cn))
    return m.to(dtype)


def cifar_case(Hc, act, N, Cn):
    """Parameters of a freshly initialised stack, torch.rand images, labels (every other point: the fp64 prediction), the fp64 autograd of the
    mean CE — built once."""
    key = ("cifar", Hc, act, N, Cn)
    if key not in _cache:
        seed = 1000 * Hc + 10 * N + Cn
        g = torch.Generator().manual_seed(seed)
        with torch.random.fork_rng():
            torch.manual_seed(seed)
            sd = cifar_sequential(act, Hc, Cn, torch.float32).state_dict()
        params = {"model." + k: v.clone() for k, v in sd.items()}
        x = torch.rand(N, 3, 32, 32, generator=g)
        lab = torch.randint(0, Cn, (N,), generator=g)
        m = cifar_sequential(act, Hc, Cn, torch.float64)
        m.load_state_dict({k: v.double() for k, v in sd.items()})
        with torch.no_grad():
            z0 = m(x.double())
        lab = torch.where(torch.arange(N) % 2 == 0, z0.argmax(-1), lab)
        z = m(x.double())
        ce = torch.logsumexp(z, -1) - z.gather(1, lab[:, None])[:, 0]
        ce.mean().backward()
        _cache[key] = {"params": params, "x": x, "lab": lab, "grad": {"model." + k: p.grad for k, p in m.named_parameters()}, "ce": ce.detach()}
    return _cache[key]


@pytest.mark.parametrize("Hc,act,N,Cn", CIFAR_CASES)
def test_cifar_geometry_matches_an_fp64_sequential(Hc, act, N, Cn):
    c = cifar_case(Hc, act, N, Cn)
    eng = engine(act, (3, 32, 32), [c["params"]])
    gm, cem = eng.weight_gradients(c["x"], c["lab"], 1, reduction="mean")
    gs, ces = eng.weight_gradients(c["x"], torch.nn.functional.one_hot(c["lab"], Cn).float(), 1, reduction="sum")        # one-hot labels
    torch.cuda.synchronize()
    assert gm["model.0.weight"].shape == (1, 32, 3, 5, 5) and gm["model.7.weight"].shape == (1, Cn, 81 * Hc)
    assert_tensors_within(f"3x32x32 Hc={Hc} {act} N={N} C={Cn} mean", gm, cem, c["grad"], c["ce"])
    assert_tensors_within(f"3x32x32 Hc={Hc} {act} N={N} C={Cn} sum", gs, ces, c["grad"], c["ce"], scale=float(N))


# ---------------------------------------------------------------------------------------------------------------- several samples
def test_rows_are_the_chosen_samples_own_gradients():
    """A stack of three nets, seeds = [2, 0]: row i is that net's own autograd gradient, and bit for bit the call with that sample alone."""
    c = CR.grad_case(16, "leaky", 8, 10)
    nets = [c["params"]] + [CR.fresh_params("leaky", 16, 10, seed) for seed in (11, 12)]
    eng = engine("leaky", CR.SHAPE, nets)
    g, ce = eng.weight_gradients(c["x"], c["lab"], 2, seeds=[2, 0], reduction="mean")
    assert ce.shape == (2, 8) and all(v.shape[0] == 2 for v in g.values())
    for row, s in enumerate((2, 0)):
        ref = CR.autograd({"params": nets[s], "x": c["x"], "lab": c["lab"]}, "leaky", torch.float64)
        assert_tensors_within(f"stack of 3, row {row} = sample {s}", g, ce, ref["grad"], ref["ce"], row=row)
        g1, ce1 = eng.weight_gradients(c["x"], c["lab"], 1, seeds=[s], reduction="mean")
        for k in CR.KEYS:
            assert torch.equal(g1[k][0], g[k][row]), (k, s)
        assert torch.equal(ce1[0], ce[row])


# ---------------------------------------------------------------------------------------------------------------- bit identity, blocks, bounds
def _blocking_case():
    c = CR.grad_case(48, "leaky", 16, 10)
    return c, c["x"][:11], c["lab"][:11]


def _equal(a, b):
    return all(torch.equal(a[0][k], b[0][k]) for k in CR.KEYS) and torch.equal(a[1], b[1])


def test_bit_identical_between_runs_and_point_block_budgets(monkeypatch):
    """N = 11: the whole batch in one block, 4 + 4 + 3 and 11 blocks of one point give the same bits, a second time on the reused
    workspaces too: every gradient element is one chain over the points, carried through the output buffer from block to block."""
    c, x, lab = _blocking_case()
    monkeypatch.delenv("RBNN_FP64_WS_GB", raising=False)
    eng = engine("leaky", CR.SHAPE, [c["params"]])
    assert eng.wgrad_point_block(1) >= 11
    whole = eng.weight_gradients(x, lab, 1)
    assert _equal(whole, eng.weight_gradients(x, lab, 1))                   # two runs
    assert _equal(whole, engine("leaky", CR.SHAPE, [c["params"]]).weight_gradients(x, lab, 1))
    per_point = sum(eng.k.conv_fp64_workspace_sizes(eng.post, 1, 1).values()) + sum(eng.k.conv_wgrad_dp_workspace_sizes(eng.post, 1, 1).values())
    for budget, nb in ((4.5 * per_point / 2 ** 30, 4), (1e-6, 1)):
        monkeypatch.setenv("RBNN_FP64_WS_GB", repr(budget))
        eb = engine("leaky", CR.SHAPE, [c["params"]])
        assert eb.wgrad_point_block(1) == nb
        sizes = []
        monkeypatch.setattr(eb.k, "conv_weight_grads_dp", lambda p, X, *a, _f=eb.k.conv_weight_grads_dp: (sizes.append(X.shape[0]), _f(p, X, *a))[1])
        first = eb.weight_gradients(x, lab, 1)
        assert sizes == ([4, 4, 3] if nb == 4 else [1] * 11)
        assert _equal(whole, first), nb
        assert _equal(whole, eb.weight_gradients(x, lab, 1)), nb            # on the reused workspaces
        assert _equal(eng.weight_gradients(x, lab, 1, reduction="mean"), eb.weight_gradients(x, lab, 1, reduction="mean")), nb


def test_nothing_is_written_or_read_behind_the_buffers(monkeypatch):
    """Every workspace buffer, the six outputs and the CE carry a NaN canary behind them (4 + 4 + 3 blocks, so the ragged block's buffers too):
    the canaries are intact afterwards and the results are the bits of a run without them."""
    c, x, lab = _blocking_case()
    monkeypatch.delenv("RBNN_FP64_WS_GB", raising=False)
    want = engine("leaky", CR.SHAPE, [c["params"]]).weight_gradients(x, lab, 1)
    eng = engine("leaky", CR.SHAPE, [c["params"]])
    per_point = sum(eng.k.conv_fp64_workspace_sizes(eng.post, 1, 1).values()) + sum(eng.k.conv_wgrad_dp_workspace_sizes(eng.post, 1, 1).values())
    monkeypatch.setenv("RBNN_FP64_WS_GB", repr(4.5 * per_point / 2 ** 30))
    guard, held = 64, []

    def with_canary(n_bytes, dtype=torch.float64):
        n = n_bytes // (8 if dtype == torch.float64 else 1)
        t = torch.full((n + guard,), float("nan") if dtype == torch.float64 else 123, dtype=dtype, device=DEV)
        held.append((t, n))
        return t[:n]
    monkeypatch.setattr(eng.fp64, "buffer", with_canary)
    got = eng.weight_gradients(x, lab, 1)
    torch.cuda.synchronize()
    assert _equal(want, got)
    # two block sizes (4 and 3) x (the forward's buffers + the three new ones), the six outputs, the CE
    assert len(held) == 2 * (_hip.CONV_FP64_WS_BUFFERS + _hip.CONV_WGRAD_DP_WS_BUFFERS) + 6 + 1
    for t, n in held:
        tail = t[n:]
        assert bool((torch.isnan(tail) if t.dtype == torch.float64 else tail == 123).all()), "a kernel wrote behind a buffer"


# ---------------------------------------------------------------------------------------------------------------- the checker in use
@pytest.mark.parametrize("Hc,act,B,Cn", [(48, "leaky", 16, 10), (32, "tanh", 8, 10), (16, "leaky", 65, 2)])
def test_the_fp32_trainer_sits_within_its_bar_of_the_device_fp64_result(Hc, act, B, Cn):
    """ConvNnTrainer.gradients (fp32) against weight_gradients(reduction='mean') on the device: each tensor within 1e-5 max |fp64 dW|, the bar
    tests/test_hip_conv_train.py holds the same gradient to against the CPU restatement; the fp32 per-point CE within 1e-5 max(1, CE).  The
    batches are grad_case's (no point within 2e-6 of a kink or a pooling tie); nothing is excluded here."""
    from robustbnns_amd.conv_train import ConvNnTrainer
    c = CR.grad_case(Hc, act, B, Cn)
    g64, ce64 = engine(act, CR.SHAPE, [c["params"]]).weight_gradients(c["x"], c["lab"], 1, reduction="mean")
    tr = ConvNnTrainer(act, CR.SHAPE, Cn, c["params"], 0.01, DEV, batch_size=B)
    tr.gradients(c["x"].to(DEV), c["lab"].to(DEV))
    torch.cuda.synchronize()
    G = tr.unflat(tr.grad)
    errs = {k: float((G[k].double() - g64[k][0]).abs().max() / (1e-5 * g64[k][0].abs().max())) for k in CR.KEYS}
    e = float(((tr.ws_t["ce"][:B].double() - ce64[0]).abs() / (1e-5 * ce64[0].clamp_min(1.0))).max())
    print(f"    [fp32 trainer against device fp64, Hc={Hc} {act} B={B} C={Cn}] in units of the 1e-5 bar: "
          + ", ".join(f"{k[6:]} {v:.3f}" for k, v in errs.items()) + f", ce {e:.3f}")
    assert max(errs.values()) <= 1.0, errs
    assert e <= 1.0, e


def test_forward_and_loss_gradients_keep_their_bits_around_a_weight_gradient_call():
    """The same engine, the same (N, S): weight_gradients reuses the forward's workspaces and leaves the other methods' results alone."""
    c = CR.grad_case(16, "leaky", 8, 10)
    eng = engine("leaky", CR.SHAPE, [c["params"]])
    y = torch.nn.functional.one_hot(c["lab"], 10).float()
    before = (eng.forward(c["x"], 1), eng.forward(c["x"], 1, logits=True), eng.loss_gradients(c["x"], y, 1))
    g, ce = eng.weight_gradients(c["x"], c["lab"], 1)
    after = (eng.forward(c["x"], 1), eng.forward(c["x"], 1, logits=True), eng.loss_gradients(c["x"], y, 1))
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    assert_tensors_within("after the other methods", g, ce, c["ref"]["grad"], c["ref"]["ce"], scale=8.0)


def test_refusals_on_the_device():
    c = CR.grad_case(16, "leaky", 8, 10)
    eng = engine("leaky", CR.SHAPE, [c["params"]])
    with pytest.raises(_hip.HipError, match="fp64.*requires_grad"):
        eng.weight_gradients(c["x"].clone().requires_grad_(True), c["lab"], 1)
    with pytest.raises(_hip.HipError, match="fp64.*reduction"):
        eng.weight_gradients(c["x"], c["lab"], 1, reduction="none")
    with pytest.raises(_hip.HipError, match="fp64.*labels"):
        eng.weight_gradients(c["x"], c["lab"] + 10, 1)
    with pytest.raises(_hip.HipError, match="fp64.*at least one point"):
        eng.weight_gradients(c["x"][:0], c["lab"][:0], 1)
