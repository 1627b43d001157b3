"""The fp64 weight gradients of the fc / fc2 checker on the MI355X (rbnn_fc_wgrad_dp.inc, AttackEngine.weight_gradients under
precision='fp64') against fp64 autograd on the CPU.

The bar, per tensor: max |gpu - cpu64| <= 1e-12 * max |cpu64|; per-point CE: 1e-12 * max(1, CE) — the measure and bar of
tests/test_hip_conv_wgrad_dp.py.  The reference is oracle.nn_logits under float64 autograd on the fp32 weights widened.  The shapes are the
seven of tests/test_hip_fp64.py, restated.  Every test fails on a tree without weight_gradients and its entry points."""
import pytest
import torch

import svi_restate as R
from oracle import bnn_oracle as O
from robustbnns_amd import AttackEngine, StackedPosterior, _hip

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("built_library")]

DEV = "cuda:0"
BAR = 1e-12
#        arch   act      input shape   H    C   S  N   std
CASES = {1: ("fc", "leaky", (1, 28, 28), 128, 10, 5, 33, 0.05),
         2: ("fc", "tanh", (1, 10, 5), 40, 7, 3, 17, 1.0),             # saturated; H not a multiple of 16, D_pad 64 > D
         3: ("fc", "sigm", (1, 2, 1), 16, 2, 3, 17, 1.0),              # H_pad 32 > H: a padded unit has act(0) = 1/2, its columns must not reach the result
         4: ("fc2", "relu", (1, 28, 28), 128, 10, 3, 17, 0.05),
         5: ("fc2", "sigm", (1, 3, 1), 16, 16, 5, 33, 1.0),
         6: ("fc", "leaky", (3, 32, 32), 512, 10, 3, 17, 0.03),
         7: ("fc2", "tanh", (1, 28, 28), 128, 10, 1, 1, 0.05)}
_cache = {}


def _prod(shape):
    return int(torch.tensor(shape).prod())


def keys_of(arch):
    return R.state_keys(arch)


def case(i):
    """(arch, act, shape, H, C, S, fp32 posterior, x, integer labels) of a case, built once."""
    if i not in _cache:
        arch, act, shape, H, C, S, N, std = CASES[i]
        post = O.synthetic_posterior(arch, _prod(shape), H, C, S, std)
        x, y = O.synthetic_inputs(N, shape, C, seed=10 + i)
        _cache[i] = (arch, act, shape, H, C, S, post, x, y.argmax(-1))
    return _cache[i]


def autograd64(post, x, lab, arch, act):
    """({key: float64 [S, ...] gradient of sum_n CE of every stacked net}, ce float64 [S, N]): the nets are independent, so one backward of
    the sum over samples and points gives every net's own gradient."""
    p64 = {k: v.double().requires_grad_(True) for k, v in post.items()}
    z = O.nn_logits(x.double(), p64, arch, act)
    ce = torch.logsumexp(z, -1) - z.gather(2, lab[None, :, None].expand(z.shape[0], -1, 1))[..., 0]
    ce.sum().backward()
    return {k: v.grad for k, v in p64.items()}, ce.detach()


def reference(i):
    key = ("ref", i)
    if key not in _cache:
        arch, act, shape, H, C, S, post, x, lab = case(i)
        _cache[key] = autograd64(post, x, lab, arch, act)
    return _cache[key]


def engine(arch, act, shape, H, C, post, precision="fp64"):
    return AttackEngine(StackedPosterior(arch, act, shape, C, H, post, DEV), precision=precision)


def engine_of(i, precision="fp64"):
    arch, act, shape, H, C, S, post, x, lab = case(i)
    return engine(arch, act, shape, H, C, post, precision)


def assert_tensors_within(name, arch, grads, ce, ref_grad, ref_ce, scale=1.0, bar=BAR):
    """Every sample row of grads[k] against scale * ref_grad[k], ce against ref_ce; prints every figure before it asserts."""
    assert list(grads) == keys_of(arch), list(grads)
    worst = {}
    for k in grads:
        g, r = grads[k], ref_grad[k].reshape(grads[k].shape) * scale
        assert g.dtype == torch.float64 and g.is_contiguous(), (k, g.dtype)
        worst[k] = max(float((g[s].cpu() - r[s]).abs().max() / r[s].abs().max()) for s in range(g.shape[0]))
    assert ce.dtype == torch.float64 and ce.shape == ref_ce.shape
    e = float(((ce.cpu() - ref_ce).abs() / ref_ce.clamp_min(1.0)).max())
    print(f"    {name}: " + ", ".join(f"{k[6:]} {v / bar:.4f}" for k, v in worst.items()) + f", ce {e / bar:.4f}  (x the bar {bar:g})")
    assert max(worst.values()) <= bar, (name, worst)
    assert e <= bar, (name, e)


def _equal(a, b):
    return list(a[0]) == list(b[0]) and all(torch.equal(a[0][k], b[0][k]) for k in a[0]) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("i", sorted(CASES))
def test_parity_with_fp64_autograd(i):
    arch, act, shape, H, C, S, post, x, lab = case(i)
    ref_grad, ref_ce = reference(i)
    N, D = x.shape[0], _prod(shape)
    eng = engine_of(i)
    gm, cem = eng.weight_gradients(x, lab, S, reduction="mean")
    gs, ces = eng.weight_gradients(x, torch.nn.functional.one_hot(lab, C).float(), S)          # "sum" is the default; one-hot labels
    torch.cuda.synchronize()
    assert cem.shape == (S, N) and gm["model.1.weight"].shape == (S, H, D) and gm[keys_of(arch)[-2]].shape == (S, C, H)
    if arch == "fc2":
        assert gm["model.3.weight"].shape == (S, H, H) and gm["model.3.bias"].shape == (S, H)
    assert_tensors_within(f"case {i} mean", arch, gm, cem, ref_grad, ref_ce, scale=1.0 / N)
    assert_tensors_within(f"case {i} sum", arch, gs, ces, ref_grad, ref_ce)
    assert torch.equal(cem, ces)                                            # the per-point CE is unscaled in both
    rel = {k: float((gs[k] - N * gm[k]).abs().max() / gs[k].abs().max()) for k in gs}
    print(f"    case {i} sum against N x mean: " + ", ".join(f"{k[6:]} {v / BAR:.4f}" for k, v in rel.items()) + f"  (x the bar {BAR:g})")
    assert max(rel.values()) <= BAR, rel


# ---------------------------------------------------------------------------------------------------------------- 2. the contraction, exactly
@pytest.mark.parametrize("arch", ["fc", "fc2"])
def test_the_contractions_are_exact_on_integers(arch):
    """rbnn_fc_weight_grads_dp on small integers, every product and sum exact in fp64: the six outputs are the int64 matrix products, and a
    second call on the same outputs doubles them (the accumulate contract).  A wrong lane map, a transposed tile or a wrong ragged edge
    cannot pass.  Columns the call must not read (X beyond D, dZ beyond C) hold other integers."""
    H, D, Dp, C, N, S = 40, 50, 64, 7, 37, 3
    post = O.synthetic_posterior(arch, D, H, C, S, 0.1)
    sp = StackedPosterior(arch, "leaky", (1, D, 1), C, H, post, DEV)
    assert (sp.Hp, sp.Dp) == (H, Dp)
    g = torch.Generator().manual_seed(7)
    ints = lambda *shape: torch.randint(-8, 9, shape, generator=g)
    X, dZ, dact1, dact2, hid1, hidL = ints(N, Dp), ints(S, N, 16), ints(S, N, H), ints(S, N, H), ints(S, N, H), ints(S, N, H)
    want = {"dW2": torch.einsum("snc,snh->sch", dZ[:, :, :C], hidL), "db2": dZ[:, :, :C].sum(1),
            "dW1": torch.einsum("snh,nd->shd", dact1, X[:, :D]), "db1": dact1.sum(1)}
    if arch == "fc2":
        want.update({"dWm": torch.einsum("snh,snj->shj", dact2, hid1), "dbm": dact2.sum(1)})
    ws = {k: v.double().to(DEV).contiguous() for k, v in (("dZ", dZ), ("dact1", dact1), ("dact2", dact2), ("hid1", hid1), ("hidL", hidL))}
    out = {k: torch.zeros(v.shape, dtype=torch.float64, device=DEV) for k, v in want.items()}
    k = _hip.HipKernels()
    Xd = X.float().to(DEV).contiguous()
    for times in (1, 2):
        k.fc_weight_grads_dp(sp, Xd, S, ws, out)
        torch.cuda.synchronize()
        for name, w in want.items():
            assert torch.equal(out[name].cpu(), (times * w).double()), (arch, name, times)


# ---------------------------------------------------------------------------------------------------------------- 3. several samples
def test_rows_are_the_chosen_samples_own_gradients():
    """seeds = [3, 0, 3] of a stack of five: rows 0 and 2 are bit-equal, every row is that net's own autograd gradient and, bit for bit, the
    call with that sample alone."""
    arch, act, shape, H, C, S, post, x, lab = case(1)
    ref_grad, ref_ce = reference(1)
    eng = engine_of(1)
    g, ce = eng.weight_gradients(x, lab, 3, seeds=[3, 0, 3])
    assert ce.shape == (3, x.shape[0]) and all(v.shape[0] == 3 for v in g.values())
    for k in g:
        assert torch.equal(g[k][0], g[k][2]), k
    assert torch.equal(ce[0], ce[2])
    pick = torch.tensor([3, 0, 3])
    assert_tensors_within("stack of 5, seeds [3, 0, 3]", arch, g, ce, {k: v[pick] for k, v in ref_grad.items()}, ref_ce[pick])
    for row, s in enumerate((3, 0)):
        g1, ce1 = eng.weight_gradients(x, lab, 1, seeds=[s])
        for k in g:
            assert torch.equal(g1[k][0], g[k][row]), (k, s)
        assert torch.equal(ce1[0], ce[row])


# ---------------------------------------------------------------------------------------------------------------- 4., 5. bit identity, blocks, bounds
def _blocking_case():
    """fc2, H = 128, N = 37, S = 3; and the budget under which weight_gradients' point block is 16: 16 + 16 + 5."""
    if "blocking" not in _cache:
        post = O.synthetic_posterior("fc2", 784, 128, 10, 3, 0.05)
        x, y = O.synthetic_inputs(37, (1, 28, 28), 10, seed=41)
        _cache["blocking"] = (post, x, y.argmax(-1))
    return _cache["blocking"]


def _blocking_engine():
    post, x, lab = _blocking_case()
    return engine("fc2", "leaky", (1, 28, 28), 128, 10, post)


def _budget_of_16_points(eng, S):
    per_point = sum(eng.k.f64_workspace_sizes(eng.post, 1, S).values()) + sum(eng.k.fc_wgrad_dp_workspace_sizes(eng.post, 1, S).values())
    return repr(16.5 * per_point / 2 ** 30)


def test_bit_identical_between_runs_and_point_block_budgets(monkeypatch):
    post, x, lab = _blocking_case()
    monkeypatch.delenv("RBNN_FP64_WS_GB", raising=False)
    eng = _blocking_engine()
    assert eng.fp64.point_blocks(37, 3, 2) == [(0, 37)]
    whole = eng.weight_gradients(x, lab, 3)
    assert _equal(whole, eng.weight_gradients(x, lab, 3))                   # two runs
    assert _equal(whole, _blocking_engine().weight_gradients(x, lab, 3))
    whole_mean = eng.weight_gradients(x, lab, 3, reduction="mean")
    eb = _blocking_engine()
    monkeypatch.setenv("RBNN_FP64_WS_GB", _budget_of_16_points(eb, 3))
    assert eb.fp64.point_blocks(37, 3, 2) == [(0, 16), (16, 32), (32, 37)]
    sizes = []
    monkeypatch.setattr(eb.k, "fc_weight_grads_dp", lambda p, X, *a, _f=eb.k.fc_weight_grads_dp: (sizes.append(X.shape[0]), _f(p, X, *a))[1])
    first = eb.weight_gradients(x, lab, 3)
    assert sizes == [16, 16, 5]
    assert _equal(whole, first)
    assert _equal(whole, eb.weight_gradients(x, lab, 3))                    # on the reused workspaces
    assert _equal(whole_mean, eb.weight_gradients(x, lab, 3, reduction="mean"))


def test_nothing_is_written_behind_the_buffers(monkeypatch):
    """Every workspace buffer, the six outputs, the CE and the input gradient's scratch carry a NaN canary behind them (16 + 16 + 5 points, so
    the ragged block's buffers too): the canaries are intact afterwards and the results are the bits of a run without them."""
    post, x, lab = _blocking_case()
    monkeypatch.delenv("RBNN_FP64_WS_GB", raising=False)
    want = _blocking_engine().weight_gradients(x, lab, 3)
    eng = _blocking_engine()
    monkeypatch.setenv("RBNN_FP64_WS_GB", _budget_of_16_points(eng, 3))
    guard, held = 64, []

    def with_canary(n_bytes, dtype=torch.float64):
        assert dtype == torch.float64
        n = n_bytes // 8
        t = torch.full((n + guard,), float("nan"), dtype=dtype, device=DEV)
        held.append((t, n))
        return t[:n]
    monkeypatch.setattr(eng.fp64, "buffer", with_canary)
    got = eng.weight_gradients(x, lab, 3)
    torch.cuda.synchronize()
    assert _equal(want, got)
    # two block sizes (16 and 5) x (the forward's six buffers + the two new ones), the six outputs, the CE, the input gradient's scratch
    assert len(held) == 2 * (_hip.F64_WS_BUFFERS + _hip.FC_WGRAD_DP_WS_BUFFERS) + 6 + 1 + 1
    for t, n in held:
        assert bool(torch.isnan(t[n:]).all()), "a kernel wrote behind a buffer"


# ---------------------------------------------------------------------------------------------------------------- 6. the neighbours
def test_forward_and_loss_gradients_keep_their_bits_around_a_weight_gradient_call():
    """The same engine, the same (N, S): weight_gradients reuses the forward's cached workspaces and leaves the other methods' results alone."""
    arch, act, shape, H, C, S, post, x, lab = case(4)
    eng = engine_of(4)
    y = torch.nn.functional.one_hot(lab, C).float()
    before = (eng.forward(x, S).clone(), eng.forward(x, S, logits=True).clone(), eng.loss_gradients(x, y, S).clone())
    g, ce = eng.weight_gradients(x, lab, S)
    after = (eng.forward(x, S), eng.forward(x, S, logits=True), eng.loss_gradients(x, y, S))
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    assert_tensors_within("after the other methods", arch, g, ce, *reference(4))


# ---------------------------------------------------------------------------------------------------------------- 7. the checker in use
KINK = 2e-6
TRAINER_CASES = [("fc2", "tanh", 128, 33, 5), ("fc", "sigm", 128, 33, 6), ("fc2", "leaky", 128, 33, 7)]
SVI_KEY = 0xC0FFEE


def _trainer_inputs(arch, H, B, seed):
    shape, Cn = (1, 28, 28), 10
    g = torch.Generator().manual_seed(seed)
    shapes = R.shapes_of(arch, 784, H, Cn)
    loc = {k: 0.05 * torch.randn(*s, generator=g) for k, s in shapes.items()}
    x, y = O.synthetic_inputs(B, shape, Cn, seed=seed)
    return shape, Cn, loc, x, y.argmax(-1)


def _fp32_against_fp64(name, G32, ce32, params, x, lab, arch, act, shape, H, Cn, reduction):
    """The fp32 trainer's gradients and per-point CE against weight_gradients at `params` (the fp32 weights the trainer differentiated at),
    in units of the 1e-5 bar; the kink margin of those weights in fp64 (nothing is excluded: the caller asserts it)."""
    shapes = R.shapes_of(arch, 784, H, Cn)
    stacked = {k: params[k].detach().cpu().float().reshape(shapes[k])[None] for k in shapes}
    margin = O.kink_margin(x.double(), {k: v.double() for k, v in stacked.items()}, arch, act, 1)
    g64, ce64 = engine(arch, act, shape, H, Cn, stacked).weight_gradients(x, lab, 1, reduction=reduction)
    torch.cuda.synchronize()
    errs = {k: float((G32[k].double().reshape(g64[k][0].shape) - g64[k][0]).abs().max() / (1e-5 * g64[k][0].abs().max())) for k in g64}
    e = float(((ce32.double() - ce64[0]).abs() / (1e-5 * ce64[0].clamp_min(1.0))).max())
    print(f"    [{name} against device fp64, {arch} 784->{H} {act} B={x.shape[0]}] in units of the 1e-5 bar: "
          + ", ".join(f"{k[6:]} {v:.3f}" for k, v in errs.items()) + f", ce {e:.3f}; smallest kink margin {float(margin.min()):.2e}")
    return errs, e, margin


@pytest.mark.parametrize("arch,act,H,B,seed", TRAINER_CASES)
def test_the_fp32_trainers_sit_within_their_bar_of_the_device_fp64_result(arch, act, H, B, seed):
    """SviTrainer.gradients (raw = -5, at the weights it drew) against reduction='sum' and NnTrainer.gradients against reduction='mean': each
    tensor within 1e-5 max |fp64 gradient| and the fp32 per-point CE within 1e-5 max(1, CE), the bar tests/test_hip_svi_train.py holds them
    to against the CPU restatement.  Nothing is excluded: the leaky case's seed is chosen so that no point of either net is within 2e-6 of a
    kink (smallest margins computed on the CPU: 1.22e-4 at the parameters, 1.27e-4 at the draw), which is asserted here."""
    from robustbnns_amd.nn_train import NnTrainer
    from robustbnns_amd.svi_train import SviTrainer
    shape, Cn, loc, x, lab = _trainer_inputs(arch, H, B, seed)
    sv = SviTrainer(arch, act, shape, Cn, loc, {k: torch.full_like(v, -5.0) for k, v in loc.items()}, 0.01, DEV, SVI_KEY, batch_size=B)
    sv.gradients(x.to(DEV), lab.to(DEV))
    drawn = {k: v.clone() for k, v in sv.unflat(sv.W).items()}
    errs, e, margin = _fp32_against_fp64("SviTrainer", sv.unflat(sv.grad), sv.ws_t["ce"][:B], drawn, x, lab, arch, act, shape, H, Cn, "sum")
    assert float(margin.min()) >= KINK
    assert max(errs.values()) <= 1.0, errs
    assert e <= 1.0, e
    nn = NnTrainer(arch, act, shape, Cn, loc, 0.01, DEV, batch_size=B)
    nn.gradients(x.to(DEV), lab.to(DEV))
    errs, e, margin = _fp32_against_fp64("NnTrainer", nn.unflat(nn.grad), nn.ws_t["ce"][:B], loc, x, lab, arch, act, shape, H, Cn, "mean")
    assert float(margin.min()) >= KINK
    assert max(errs.values()) <= 1.0, errs
    assert e <= 1.0, e


# ---------------------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals_on_the_device():
    import conv_restate as CR
    from robustbnns_amd.conv import ConvStackedPosterior
    conv = ConvStackedPosterior("leaky", CR.SHAPE, 10, 16, {k: v[None] for k, v in CR.fresh_params("leaky", 16, 10, 3).items()}, DEV)
    with pytest.raises(_hip.HipError, match="fp64.*conv"):
        AttackEngine(conv, precision="fp64")
    arch, act, shape, H, C, S, post, x, lab = case(1)
    with pytest.raises(_hip.HipError, match="precision='fp64'"):
        engine_of(1, "exact").weight_gradients(x, lab, S)
    eng = engine_of(1)
    with pytest.raises(_hip.HipError, match="fp64.*reduction"):
        eng.weight_gradients(x, lab, S, reduction="none")
    with pytest.raises(_hip.HipError, match="fp64.*labels"):
        eng.weight_gradients(x, torch.full_like(lab, C), S)
    with pytest.raises(_hip.HipError, match="fp64.*at least one point"):
        eng.weight_gradients(x[:0], lab[:0], S)
    with pytest.raises(_hip.HipError, match="fp64.*requires_grad"):
        eng.weight_gradients(x.clone().requires_grad_(True), lab, S)
