"""GPU tests (-m gpu) of deterministic conv training (model_nn.py:93-106, 175-219; csrc/rbnn_conv_train.hip, robustbnns_amd/conv_train.py): the
weight gradients of all six tensors, per-point CE, step loss and correct count against fp64 autograd at the same parameters, the Adam kernel
against torch.optim.Adam, the statistics kernel alone past one pass of its loop, two runs against each other, what must not be read (NaN behind
every bound) or written (canaries behind every buffer of a trainer sized for exactly B), the slice plan that ran against the restated one
(conv_restate.slice_plan), buffers sized for a large batch used by a small one, NN.train_conv end to end against the fp64 restatement
(tests/conv_restate.py), the files, no device->host sync inside a step, and the guards.  Every check prints one line with its worst figure in
units of its bar.

Mutations these tests are written to catch: no `/ B` in dZ, a missing bias gradient, pool-2 routing that drops one of the overlapping windows,
act' taken at the wrong element for sigm / tanh, dK2 in (tap, ci) instead of (ci, tap) order -> the gradient test.
With conv_restate.REGIME_CASES (slices of several groups / points, ragged last slices, the one-slice plan, more than 32 stages per slice):
k_end not clamped to K in dP1's last slice (the K2w gather runs into model.3.bias and the head's weights, dO2 into the next point's) -> the
gradient test (model.0.*) and, behind a canaried dO2, the bounds tests; kc formed from the slice count instead of the per-slice count (slice
s starts at s kc, so any kc with slices x kc >= K still shares K out: only the one-slice plan of several groups, B = 500, leaves channels
out) -> the gradient test at (48, leaky, 500, 3); the point index of dK1 / dK2 taken relative to the slice (every slice contracts the
first points again), or dK1's staying at its slice's first point (right wherever a slice is one point, B <= 128) -> the gradient test
(model.0.*, model.3.*); a fold that zeroes acc without adding it to tot (the first 512 products of a slice lost; dK1 folds at every B, dP1
and dK2 only in these cases) -> the gradient test; a slice launched and not stored, or a plan other than the restated one -> the plan test; partP sized for the
sizing batch's plan alone -> the large-small test and the host tier's sweep."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

import conv_restate as CR
import nn_restate as NR

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("built_library")]
DEV = "cuda:0"
TRAJ_SPREADS = 4               # tests/test_hip_nn_train.py's spread argument


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu() if t.dtype == torch.float32 else t.detach().cpu().clone()


def _state(tr):
    return {name: _bits(getattr(tr, name)) for name in ("P", "m", "v", "grad", "stats")}


def _trainer(params, act, Cn, batch_size, lr=0.01):
    from robustbnns_amd.conv_train import ConvNnTrainer
    return ConvNnTrainer(act, CR.SHAPE, Cn, params, lr, DEV, batch_size=batch_size)


@pytest.mark.parametrize("Hc,act,B,Cn", CR.GRAD_CASES)
def test_gradients_loss_and_count_match_fp64_autograd(Hc, act, B, Cn):
    """Per tensor: max |dW - fp64| <= 1e-5 max |fp64 dW|.  Per-point CE: absolute error <= 1e-5 max(1, CE).  Step loss: 1e-5 relative to the
    fp64 mean.  Correct count: the fp64 count, give or take the points within nn_restate.MARGIN (at most 2 % of the case:
    tests/test_conv_train_cpu.py).  gradients() first, then step() on the same batch."""
    c = CR.grad_case(Hc, act, B, Cn)
    ref = c["ref"]
    tr = _trainer(c["params"], act, Cn, 4)                                # smaller than most B: the workspaces grow
    x, lab = c["x"].to(DEV), c["lab"].to(DEV)
    tr.gradients(x, lab)
    torch.cuda.synchronize()
    G = tr.unflat(tr.grad)
    assert list(G) == CR.KEYS
    errs = {}
    for k, g64 in ref["grad"].items():
        gmax, err = float(g64.abs().max()), float((G[k].cpu().double() - g64).abs().max())
        errs[k] = err / (1e-5 * gmax)
    print(f"[conv-train grad Hc={Hc} {act} B={B} C={Cn}] gradient error per tensor in units of 1e-5 max|fp64 gradient|: "
          + ", ".join(f"{k[6:]} {v:.3f}" for k, v in errs.items()))
    e = (tr.ws_t["ce"][:B].cpu().double() - ref["ce"]).abs() / (1e-5 * ref["ce"].clamp_min(1.0))
    assert max(errs.values()) <= 1.0, errs
    assert float(e.max()) <= 1.0, float(e.max())
    tr.step(x, lab)
    stats = tr.stats.tolist()
    w_loss = abs(stats[0] - ref["loss"]) / (1e-5 * abs(ref["loss"]))
    assert w_loss <= 1.0, (stats[0], ref["loss"])
    assert stats[1] == stats[0] and stats[0] == float(torch.tensor(stats[0], dtype=torch.float32))       # an fp32 value
    assert ref["c_safe"] <= stats[2] <= ref["c_safe"] + ref["n_marginal"] and stats[2] == int(stats[2]), (stats[2], ref["c_safe"])
    assert tr.t == 1 and not torch.equal(tr.P.cpu(), torch.cat([c["params"][k].reshape(-1) for k in CR.KEYS]))
    print(f"[conv-train grad Hc={Hc} {act} B={B} C={Cn}] worst gradient error {max(errs.values()):.3f} x (1e-5 max|fp64 gradient|); per-point CE "
          f"{float(e.max()):.3f} x bar; step loss {w_loss:.3f} x 1e-5; excluded: {c['n_drop']} of {c['n_pool']} pool points at a kink or a pooling tie, "
          f"{ref['n_marginal']} of {B} points within the argmax margin")


@pytest.mark.parametrize("t", [1, 2, 10, 10 ** 7])
def test_adam_step_kernel_matches_torch_optim_adam(t):
    """tests/test_hip_nn_train.py's bar and scales: 2e-6 x scale.  Elements [100, 400) are dead (grad = m = v = 0): the update is exactly 0."""
    from robustbnns_amd import _hip
    from robustbnns_amd.conv_train import ADAM_EPS, BETAS
    lr = 0.01
    g = torch.Generator().manual_seed(100 + t % 9973)
    tr = _trainer(CR.fresh_params("leaky", 16, 5, 3), "leaky", 5, 4, lr)
    n = tr.n_params
    m0 = 0.2 * torch.randn(n, generator=g)
    vals = {"P": tr.P.cpu(), "grad": 3 * torch.randn(n, generator=g), "m": m0, "v": (m0.abs() + torch.rand(n, generator=g)) ** 2}
    for name in ("grad", "m", "v"):
        vals[name][100:400] = 0.0
    for name, v in vals.items():
        getattr(tr, name).copy_(v)
    _hip.check(tr.k.lib.rbnn_conv_adam_step(C.byref(tr.net), t, lr, BETAS[0], BETAS[1], ADAM_EPS, _hip.stream_of(tr.P)), "rbnn_conv_adam_step")
    torch.cuda.synchronize()
    d = {k: v.double() for k, v in vals.items()}
    w = d["P"].clone().requires_grad_(True)
    opt = torch.optim.Adam([w], lr=lr)
    opt.state[w] = {"step": torch.tensor(float(t - 1)), "exp_avg": d["m"].clone(), "exp_avg_sq": d["v"].clone()}
    w.grad = d["grad"].clone()
    opt.step()
    out = {"P": w.detach(), "m": opt.state[w]["exp_avg"], "v": opt.state[w]["exp_avg_sq"]}
    step_size = lr / (1 - BETAS[0] ** t)
    scale = {"P": d["P"].abs() + step_size * (1 + out["m"].abs() / (out["v"].sqrt() / (1 - BETAS[1] ** t) ** 0.5 + ADAM_EPS)),
             "m": d["grad"].abs() + d["m"].abs(), "v": d["v"] + d["grad"] ** 2}
    worst = 0.0
    for name, sc in scale.items():
        got = getattr(tr, name).cpu().double()
        assert bool(torch.isfinite(got).all()), name
        diff = (got - out[name]).abs()
        if name == "P":
            assert bool((diff[100:400] == 0).all()), "a dead element moved"
        err = float(torch.where(sc > 0, diff / sc.clamp_min(1e-300), torch.where(diff == 0, 0.0, float("inf"))).max())
        assert err <= 2e-6, (name, err)
        worst = max(worst, err / 2e-6)
    print(f"[conv-train adam t={t}] worst error {worst:.3f} x (2e-6 x scale) over P, m, v of {n} parameters; excluded: nothing")


@pytest.mark.parametrize("B", [1, 256, 257, 600])
def test_finalize_sums_every_pass_of_its_loop(B):
    """rbnn_conv_train_finalize alone on hand-filled ce in [0, 5) and flags, twice on one accumulator: B = 257 and 600 take the 256-wide loop
    into a second and a third pass.  stats[2]: the exact count.  stats[0]: an fp32 value within one fp32 ulp of the fp64 mean (a correctly
    rounded mean is within half an ulp; the fp64 sums, this one and the kernel's, err by at most B 2^-53 relative, so only a mean that close
    to an fp32 rounding tie can round to the other neighbour).  stats[1]: the fp64 sum of the two stats[0], exactly."""
    from robustbnns_amd import _hip
    lib, g = _hip.load(), torch.Generator().manual_seed(7000 + B)
    stats = torch.zeros(3, dtype=torch.float64, device=DEV)
    ws, losses, count, worst = _hip.ConvTrainWs(), [], 0, 0.0
    for _ in range(2):
        ce, flags = 5 * torch.rand(B, generator=g), torch.randint(0, 2, (B,), generator=g, dtype=torch.int32)
        ce_d, flags_d = ce.to(DEV), flags.to(DEV)
        ws.ce, ws.correct = _hip.ptr(ce_d), _hip.ptr(flags_d)
        _hip.check(lib.rbnn_conv_train_finalize(C.byref(ws), B, _hip.ptr(stats), _hip.stream_of(stats)), "rbnn_conv_train_finalize")
        got = stats.tolist()                                               # synchronises: ce_d / flags_d outlive the launch
        mean64 = float(ce.double().sum()) / B
        ulp = float(np.spacing(np.float32(max(got[0], mean64))))
        losses.append(got[0])
        count += int(flags.sum())
        print(f"[conv-train finalize B={B}] step loss {got[0]!r}, fp64 mean {mean64!r}: |diff| = {abs(got[0] - mean64) / ulp:.3f} fp32 ulp; "
              f"sum {got[1]!r}; count {got[2]} of {count}")
        assert got[0] == float(np.float32(got[0])) and abs(got[0] - mean64) <= ulp, (got[0], mean64, ulp)
        assert got[1] == sum(losses) and got[2] == count, (got, losses, count)
        worst = max(worst, abs(got[0] - mean64) / ulp)
    print(f"[conv-train finalize B={B}] worst step loss {worst:.3f} fp32 ulp from the fp64 mean (bar 1); excluded: nothing")


def _three_steps(c, act, Cn):
    tr = _trainer(c["params"], act, Cn, 8)
    x, lab = c["x"].to(DEV), c["lab"].to(DEV)
    for sl in (slice(0, 8), slice(8, 16), slice(3, 8)):
        tr.step(x[sl], lab[sl])
    torch.cuda.synchronize()
    return _state(tr)


def test_two_identical_runs_are_bit_identical():
    """Three steps (B = 8, 8, 5): no atomics, every sum in one fixed order."""
    Hc, act, B, Cn = CR.GRAD_CASES[4]
    c = CR.grad_case(Hc, act, B, Cn)
    a, b = _three_steps(c, act, Cn), _three_steps(c, act, Cn)
    for name in a:
        assert torch.equal(a[name], b[name]), f"two identical runs differ in {name}"
    assert float(a["stats"][1]) > 0 and bool(torch.isfinite(a["P"].view(torch.float32)).all())
    print(f"[conv-train repeat Hc={Hc} {act}] P, m, v, grad, stats bit-identical between two runs of 3 steps (B = 8, 8, 5); excluded: nothing")


def _poisoned(Hc, act, B, Cn, poison):
    """One step on B < Bmax points; poison: NaN (0xFF in the stash bytes) in every per-point workspace behind [B, .], in the whole of the
    partial-sum buffers (a step writes what it reads of them), in rows >= B and columns [784, ldx) of the staging matrix, and a class >= C
    in the labels behind B."""
    c = CR.grad_case(Hc, act, B, Cn)
    tr = _trainer(c["params"], act, Cn, 2 * B + 3)
    tr.Dp = 800                                                            # a staging matrix with columns behind the image
    tr.X = torch.zeros(tr.Bmax, tr.Dp, dtype=torch.float32, device=DEV)
    assert B < tr.Bmax
    if poison:
        for k, v in tr.ws_t.items():
            bad = {torch.float32: float("nan"), torch.uint8: 255, torch.int32: Cn}[v.dtype]
            if k in ("part1", "part2", "partP"):
                v[:] = bad
            else:
                v[B * (v.numel() // tr.Bmax):] = bad
        tr.X[B:] = float("nan")
        tr.X[:, 784:] = float("nan")
        tr.labels[B:] = Cn
    tr.step(c["x"].to(DEV), c["lab"].to(DEV))
    torch.cuda.synchronize()
    res = _state(tr)
    res["ce"], res["correct"] = _bits(tr.ws_t["ce"][:B]), _bits(tr.ws_t["correct"][:B])
    for name in ("P", "m", "v", "grad", "ce"):
        assert bool(torch.isfinite(res[name].view(torch.float32)).all()), name
    assert bool(torch.isfinite(tr.stats).all())
    return res


@pytest.mark.parametrize("Hc,act,B,Cn", [CR.GRAD_CASES[1], CR.GRAD_CASES[2], CR.GRAD_CASES[5], CR.REGIME_CASES[0], CR.REGIME_CASES[2]])
def test_nothing_behind_the_bounds_is_read(Hc, act, B, Cn):
    """NaN is data: every index stays inside its allocation, and a NaN that leaked into a sum would stay there.  The two regime cases: slices of
    several groups / points with a ragged last one (dP1's gather of K2w stops at its K; the point behind the batch is never fetched), and dP1's
    one-slice plan."""
    clean, dirty = _poisoned(Hc, act, B, Cn, False), _poisoned(Hc, act, B, Cn, True)
    for name in clean:
        assert torch.equal(clean[name], dirty[name]), f"{name} depends on memory behind the bounds"
    print(f"[conv-train bounds Hc={Hc} {act} B={B} C={Cn}] {len(clean)} results bit-identical and finite with NaN behind [B, .] of every workspace, in rows >= {B} "
          f"and columns [784, 800) of the staged batch; excluded: nothing")


CANARY = {torch.float32: float("nan"), torch.float64: float("nan"), torch.uint8: 255, torch.int32: 0x7FFFFFFF}
PAD = 64                       # elements behind every buffer
FLAT = ("P", "m", "v", "grad")


def _padded(t):
    """A copy of the contiguous tensor t at the front of an allocation with PAD canary elements behind it -> (view, tail)."""
    big = torch.full((t.numel() + PAD,), CANARY[t.dtype], dtype=t.dtype, device=t.device)
    big[:t.numel()].copy_(t.reshape(-1))
    return big[:t.numel()].view(t.shape), big[t.numel():]


def _canaried_step(Hc, act, B, Cn, canaries):
    """One step of a trainer sized for exactly B points; canaries: the flat buffers, the staged batch, its labels, every workspace and stats are
    moved to the front of allocations with PAD canary elements (NaN; 255 in the stash bytes; an impossible class in the labels) behind them.
    -> (results' bit patterns, the tails)."""
    from robustbnns_amd import _hip
    c = CR.grad_case(Hc, act, B, Cn)
    tr = _trainer(c["params"], act, Cn, B)
    assert tr.Bmax == B
    tails = {}
    if canaries:
        for name in FLAT + ("X", "labels", "stats"):
            view, tails[name] = _padded(getattr(tr, name))
            setattr(tr, name, view)
        for k in list(tr.ws_t):
            tr.ws_t[k], tails["ws_" + k] = _padded(tr.ws_t[k])
        _hip.fill(tr.net, tr)
        tr.ws = _hip.fill(_hip.ConvTrainWs, tr.ws_t)
    tr.step(c["x"].to(DEV), c["lab"].to(DEV))
    torch.cuda.synchronize()
    res = _state(tr)
    res["ce"], res["correct"], res["dZ"] = _bits(tr.ws_t["ce"][:B]), _bits(tr.ws_t["correct"][:B]), _bits(tr.ws_t["dZ"][:16 * B])
    for name in FLAT + ("ce",):
        assert bool(torch.isfinite(res[name].view(torch.float32)).all()), name
    assert bool(torch.isfinite(tr.stats).all())
    return res, tails


@pytest.mark.parametrize("Hc,act,B,Cn", [CR.GRAD_CASES[1], CR.GRAD_CASES[6], CR.REGIME_CASES[0], CR.REGIME_CASES[2]])
def test_nothing_behind_the_bounds_is_written(Hc, act, B, Cn):
    """Buffers sized for exactly B points (B = 5, 65, 129 and 500: partP holds one, three, five and one slice).  Written: every canary element
    behind every buffer is still a canary after the step.  Read: the results are bit-identical with and without the canaries."""
    clean, _ = _canaried_step(Hc, act, B, Cn, False)
    dirty, tails = _canaried_step(Hc, act, B, Cn, True)
    for name in clean:
        assert torch.equal(clean[name], dirty[name]), f"{name} depends on memory behind the bounds"
    assert len(tails) == len(FLAT) + 3 + 13, sorted(tails)
    for name, tail in tails.items():
        intact = torch.isnan(tail).all() if tail.dtype.is_floating_point else (tail == CANARY[tail.dtype]).all()
        assert bool(intact) and tail.numel() == PAD, f"the step wrote behind {name}"
    print(f"[conv-train canaries Hc={Hc} {act} B={B} C={Cn}] {len(clean)} results bit-identical and finite with canaries behind {len(tails)} buffers sized for "
          f"exactly {B} points, every canary intact; excluded: nothing")


@pytest.mark.parametrize("Hc,act,B,Cn", [CR.GRAD_CASES[4], CR.GRAD_CASES[6]] + CR.REGIME_CASES)
def test_the_plan_that_ran_is_the_restated_plan(Hc, act, B, Cn):
    """part1, part2 and partP filled with NaN, then gradients(): the floats that are no longer NaN are the first slices x M x N of each buffer,
    with conv_restate.slice_plan's slice count (NaN after them where the buffer is larger than this batch's plan).  A slice launched and not
    written, written twice as wide, or a plan other than the restated one fails here; the gradients are finite."""
    c = CR.grad_case(Hc, act, B, Cn)
    tr = _trainer(c["params"], act, Cn, B)
    for k in ("part1", "part2", "partP"):
        tr.ws_t[k].fill_(float("nan"))
    tr.gradients(c["x"].to(DEV), c["lab"].to(DEV))
    torch.cuda.synchronize()
    plan, want = CR.slice_plan(B, Hc), CR.plan_floats(B, Hc)
    got = {k: int((~torch.isnan(tr.ws_t[k])).sum()) for k in want}
    print(f"[conv-train plan Hc={Hc} {act} B={B} C={Cn}] plan (per, slices) {plan}; floats written / planned / allocated: "
          + ", ".join(f"{k} {got[k]} / {want[k]} / {tr.ws_t[k].numel()}" for k in want))
    for k in want:
        assert got[k] == want[k] <= tr.ws_t[k].numel(), (k, got[k], want[k])
        assert not bool(torch.isnan(tr.ws_t[k][:want[k]]).any()), f"{k}: a hole inside the planned slices"
    assert bool(torch.isfinite(tr.grad).all())


def test_buffers_sized_large_and_used_small_give_the_small_trainers_bits():
    """A trainer grown to B = 129 at Hc = 144 (partP sized for that plan: 5 slices of 129 points), every workspace then filled with NaN (255 in
    the stash bytes), stepped on the first 8 points of the case: dP1 now takes 9 slices of 8 points inside the same partP.  P, m, v, grad,
    stats, the per-point CE and flags are bit-equal to those of a fresh trainer sized for 8."""
    Hc, act, B, Cn = CR.REGIME_CASES[0]
    c = CR.grad_case(Hc, act, B, Cn)
    b = 8
    x, lab = c["x"][:b].to(DEV), c["lab"][:b].to(DEV)
    assert CR.slice_plan(B, Hc)["dP1"] == (2, 5) and CR.slice_plan(b, Hc)["dP1"] == (1, 9)
    res = {}
    for size in (B, b):
        tr = _trainer(c["params"], act, Cn, size)
        assert tr.Bmax == size and CR.plan_floats(b, Hc)["partP"] <= tr.ws_t["partP"].numel()
        if size == B:
            for v in tr.ws_t.values():
                v.fill_({torch.float32: float("nan"), torch.uint8: 255, torch.int32: Cn}[v.dtype])
            tr.X.fill_(float("nan"))
            tr.labels.fill_(Cn)
        tr.step(x, lab)
        torch.cuda.synchronize()
        res[size] = _state(tr)
        res[size]["ce"], res[size]["correct"] = _bits(tr.ws_t["ce"][:b]), _bits(tr.ws_t["correct"][:b])
        assert bool(torch.isfinite(tr.P).all()) and bool(torch.isfinite(tr.grad).all()) and bool(torch.isfinite(tr.stats).all())
    n_diff = 0
    for name in res[b]:
        d = int((res[B][name] != res[b][name]).sum())
        n_diff += d
        assert d == 0, f"{name}: {d} elements differ between the trainer sized for {B} and the one sized for {b}"
    print(f"[conv-train large-small Hc={Hc} {act}] a step on {b} points in buffers sized for {B} (dP1: 9 slices where the sizing batch has 5): {n_diff} "
          f"differing elements over {len(res[b])} results (bar 0); excluded: nothing")


def _nn():
    from robustbnns_amd.model_nn import NN
    m = CR.TRAJ
    return NN(m["dataset"], m["shape"], m["n_classes"], m["hidden"], m["act"], m["arch"], m["lr"], m["epochs"])


def test_train_conv_follows_the_fp64_restatement(capsys, tmp_path, monkeypatch):
    meta = CR.TRAJ
    r64, before, n_tie, spread, _ = CR.traj_reference()
    assert n_tie == 0
    params, x, lab = CR.traj_inputs()
    scale = NR.param_scale(r64.params())
    bar = TRAJ_SPREADS * spread * scale
    tr = _trainer(params, meta["act"], meta["n_classes"], meta["batch"], meta["lr"])
    worst, i = 0.0, 0
    for _ in range(meta["epochs"]):
        for s in range(0, meta["N"], meta["batch"]):
            d = NR.max_diff({k: v.cpu() for k, v in tr.params().items()}, before[i])
            assert d <= bar, (i, d, bar)
            worst, i = max(worst, d), i + 1
            tr.step(x[s:s + meta["batch"]].to(DEV), lab[s:s + meta["batch"]].to(DEV))
    final_hand = {k: v.cpu() for k, v in tr.params().items()}
    d = NR.max_diff(final_hand, r64.params())
    worst = max(worst, d)
    line = (f"[conv-train trajectory] {i} steps: max |P - fp64| = {worst:.2e} = {worst / (spread * scale):.3f} x spread ({spread:.2e} x {scale:.2f}), "
            f"bar {TRAJ_SPREADS}; torch's own fp32 runs: <= 1.000")
    assert d <= bar, line
    # NN.train_conv itself: the same kernels in the same order
    y = torch.eye(meta["n_classes"])[lab]
    loader = DataLoader(TensorDataset(x, y), batch_size=meta["batch"], shuffle=False)
    net = _nn()
    net.load_state_dict(params)
    capsys.readouterr()
    got = net.train_conv(loader, DEV, 3, save=False)
    out = capsys.readouterr().out
    print(line)
    for k, v in net.state_dict().items():
        assert torch.equal(v, final_hand[k]), k
    assert net.device == DEV and " == NN training ==" in out and got.t == i
    # the epoch lines, as tests/test_hip_nn_train.py::_check_lines with the fp64 restatement in the reference's place
    lines = NR.parse_epoch_lines(out)
    per = len(r64.losses) // meta["epochs"]
    assert len(lines) == meta["epochs"]
    for e, (loss, acc) in enumerate(lines):
        loss64 = sum(r64.losses[e * per:(e + 1) * per]) / meta["N"]
        lbar = TRAJ_SPREADS * spread * abs(loss64) + 1e-8
        print(f"   epoch {e + 1}: loss {loss:.8f} fp64 {loss64:.10f}: |diff| = {abs(loss - loss64) / lbar:.3f} x bar; accuracy {acc}")
        assert abs(loss - loss64) <= lbar
        if sum(r64.n_marginal[e * per:(e + 1) * per]) == 0:
            assert f"{acc:.2f}" == f"{100 * sum(r64.correct[e * per:(e + 1) * per]) / meta['N']:.2f}"
    # the trained module drives the attack engine: its cache saw the new parameters
    z = net.forward(x[:8], DEV).cpu().double()
    z64 = CR.logits(x[:8], r64.params(), meta["act"])
    assert float((z - z64).abs().max()) <= 1e-3 * float(z64.abs().max())
    assert float((z64 - CR.logits(x[:8], params, meta["act"])).abs().max()) > 1e-2 * float(z64.abs().max())       # and they moved
    # save=True, then load
    monkeypatch.chdir(tmp_path)
    net2 = _nn()
    net2.load_state_dict(params)
    net2.train_conv(loader, DEV, seed=3)
    again = _nn()
    again.load(DEV)
    for k, v in net2.state_dict().items():
        assert torch.equal(v, again.state_dict()[k]) and torch.equal(v, final_hand[k]), k
    assert torch.equal(again.forward(x[:8], DEV), net2.forward(x[:8], DEV))
    assert os.listdir(tmp_path)


def test_twenty_steps_make_no_device_to_host_sync():
    c = CR.grad_case(*CR.GRAD_CASES[0])
    tr = _trainer(c["params"], "leaky", 10, 8)
    x, lab = c["x"].to(DEV), c["lab"].to(DEV)
    tr.step(x, lab)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for i in range(20):
            tr.step(x[:8 - i % 3], lab[:8 - i % 3])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    loss, correct = tr.epoch_totals()
    assert tr.t == 21 and loss == loss and 0 <= correct <= 21 * 8


def test_guards_raise_with_no_state_changed():
    from robustbnns_amd.conv_train import ConvNnTrainer
    from robustbnns_amd.model_nn import NN
    x, y = torch.rand(8, 1, 28, 28), torch.eye(10)[torch.arange(8)]
    loader = DataLoader(TensorDataset(x, y), batch_size=4)
    conv = NN("mnist", (1, 28, 28), 10, 16, "leaky", "conv", 0.01, 1)
    before = {k: v.clone() for k, v in conv.state_dict().items()}
    with pytest.raises(NotImplementedError, match="no CPU compute path"):
        conv.train_conv(loader, "cpu")
    with pytest.raises(NotImplementedError, match="no CPU compute path"):
        ConvNnTrainer("leaky", (1, 28, 28), 10, conv.state_dict(), 0.01, "cpu")
    with pytest.raises(NotImplementedError, match="1x28x28"):
        ConvNnTrainer("leaky", (3, 32, 32), 10, conv.state_dict(), 0.01, DEV)
    conv.input_shape = (3, 32, 32)
    with pytest.raises(NotImplementedError, match="1x28x28"):
        conv.train_conv(loader, DEV)
    conv.input_shape = (1, 28, 28)
    with pytest.raises(NotImplementedError, match="conv"):
        conv.train(loader, DEV)                                            # NN.train keeps refusing conv
    fc = NN("mnist", (1, 28, 28), 10, 16, "leaky", "fc", 0.01, 1)
    with pytest.raises(ValueError, match="train"):
        fc.train_conv(loader, DEV)
    assert all(torch.equal(v, before[k]) for k, v in conv.state_dict().items()) and not hasattr(conv, "device") and not hasattr(fc, "device")
