"""GPU tests (-m gpu) of deterministic training (model_nn.py:175-219, model_ensemble.py:69-83; csrc/rbnn_nn_train.hip,
robustbnns_amd/nn_train.py): every member's weight gradients, per-point CE, step loss and correct count against fp64 autograd at the same
parameters, the Adam kernel against torch.optim.Adam, the statistics kernel alone past one pass of its loop, lockstep against the members alone, gathered rows against a staged copy, what must not
be read (NaN behind every bound), NN.train / Ensemble_NN.train end to end on the reference's recorded runs against the fp64 restatement
(tests/nn_restate.py), the files, no device->host sync inside a step, and the guards.  Every check prints one line with its worst figure
in units of its bar.

Mutations these tests are written to catch (the test meant to turn red): no `/ B` in dZ -> the weight gradients; a member reading its
neighbour's rows -> the weight gradients (M > 1); no bias-gradient column -> the weight gradients; t + 1 in the bias correction -> the Adam
test (t = 1, 2, 10); the last maximum in the flag -> test_correct_flag_takes_the_first_maximum."""
import ctypes as C

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

import nn_restate as NR
from oracle import bnn_oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("built_library")]
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu() if t.dtype == torch.float32 else t.detach().cpu().clone()


def _state(tr):
    return {name: _bits(getattr(tr, name)) for name in ("P", "m", "v", "grad", "stats")}


@pytest.mark.parametrize("arch,act,shape,H,Cn,B,M", NR.GRAD_CASES)
def test_every_members_gradients_loss_and_count_match_fp64_autograd(arch, act, shape, H, Cn, B, M):
    """Per tensor and member: max |dW - fp64| <= 1e-5 max |fp64 dW| (C = 1: exactly zero).  Per-point CE: absolute error <= 1e-5 max(1, CE) on
    each branch of the head kernel.  Step loss: 1e-5 relative to the fp64 mean.  Correct count: the fp64 count, give or take the points within
    nn_restate.MARGIN (at most 2 % of the case: tests/test_nn_train_cpu.py)."""
    from robustbnns_amd.nn_train import NnTrainer
    c = NR.grad_case(arch, act, shape, H, Cn, B, M)
    tr = NnTrainer(arch, act, shape, Cn, c["params"], 0.01, DEV, batch_size=64)          # smaller than some B: the workspaces grow
    tr.set_data(c["x"], c["lab"])
    rows = c["rows"].to(DEV)
    tr.gradients(rows=rows)
    torch.cuda.synchronize()
    ce_gpu = tr.ws_t["ce"][:M * B].view(M, B).cpu().double()
    w_g = w_ce = w_loss = 0.0
    refs = [NR.member_fp64(c, m, arch, act) for m in range(M)]
    for m, ref in enumerate(refs):
        G = tr.unflat(tr.grad, m)
        for k, g64 in ref["grad"].items():
            gmax, err = float(g64.abs().max()), float((G[k].cpu().double() - g64).abs().max())
            assert err <= 1e-5 * gmax, (m, k, err, gmax)
            w_g = max(w_g, err / (1e-5 * gmax) if gmax else 0.0)
        e = (ce_gpu[m] - ref["ce"]).abs() / (1e-5 * ref["ce"].clamp_min(1.0))
        assert float(e.max()) <= 1.0, (m, float(e.max()))
        w_ce = max(w_ce, float(e.max()))
    tr.step(rows=rows)
    stats = tr.stats.tolist()
    n_marg = 0
    for m, ref in enumerate(refs):
        assert abs(stats[m][0] - ref["loss"]) <= 1e-5 * abs(ref["loss"]), (m, stats[m][0], ref["loss"])
        w_loss = max(w_loss, abs(stats[m][0] - ref["loss"]) / (1e-5 * abs(ref["loss"])) if ref["loss"] else 0.0)
        assert stats[m][1] == stats[m][0] and stats[m][0] == float(torch.tensor(stats[m][0], dtype=torch.float32))       # an fp32 value
        assert ref["c_safe"] <= stats[m][2] <= ref["c_safe"] + ref["n_marginal"] and stats[m][2] == int(stats[m][2]), (m, stats[m][2], ref["c_safe"])
        n_marg += ref["n_marginal"]
    print(f"[nn-train grad {arch} {c['D']}->{H}->{Cn} {act} B={B} M={M}] worst gradient error {w_g:.3f} x (1e-5 max|fp64 gradient|); per-point CE {w_ce:.3f} x bar; "
          f"step loss {w_loss:.3f} x 1e-5; excluded: kink {c['n_kink']} of {c['n_pool']} pool points, {n_marg} of {M * B} points within the argmax margin")


def test_correct_flag_takes_the_first_maximum():
    """Exact ties: W2 = 0 makes every logit the bias, and equal biases tie in fp32 and fp64 alike; torch.argmax takes the first."""
    from robustbnns_amd.nn_train import NnTrainer
    D, H, Cn, B = 10, 32, 5, 40
    p = {k: 0.3 * torch.randn(*s, generator=torch.Generator().manual_seed(1)) for k, s in O.param_shapes("fc", D, H, Cn)}
    p["model.3.weight"].zero_()
    p["model.3.bias"].copy_(torch.tensor([0.5, 2.0, -1.0, 2.0, 2.0]))
    x, y = O.synthetic_inputs(B, (1, D, 1), Cn, seed=3)
    lab = y.argmax(-1)
    assert int((lab == 1).sum()) and int((lab == 3).sum()) and int((lab == 4).sum())
    tr = NnTrainer("fc", "tanh", (1, D, 1), Cn, [p], 0.01, DEV, batch_size=B)
    tr.step(x.to(DEV), lab.to(DEV))
    flags = tr.ws_t["correct"][:B].cpu()
    assert torch.equal(flags, (lab == 1).to(torch.int32)) and float(tr.stats[0, 2]) == float((lab == 1).sum())


@pytest.mark.parametrize("t", [1, 2, 10, 1000, 100000, 10 ** 7])
def test_adam_step_kernel_matches_torch_optim_adam(t):
    """tests/test_hip_svi_train.py's bar: every output is a chain of at most ~10 fp32 operations on operands bounded by the scale named below:
    2e-6 x scale.  Elements [100, 400) of every member are dead (grad = m = v = 0): eps alone in the denominator, the update is exactly 0 and
    a scale of 0 admits no error at all."""
    from robustbnns_amd import _hip
    from robustbnns_amd.nn_train import ADAM_EPS, BETAS, NnTrainer
    arch, D, H, Cn, lr, M = "fc2", 20, 64, 5, 0.01, 3
    g = torch.Generator().manual_seed(100 + t % 9973)
    params = [{k: 0.3 * torch.randn(*s, generator=g) for k, s in O.param_shapes(arch, D, H, Cn)} for _ in range(M)]
    tr = NnTrainer(arch, "leaky", (1, D, 1), Cn, params, lr, DEV, batch_size=8)
    n = tr.n_params
    m0 = 0.2 * torch.randn(M, n, generator=g)
    vals = {"P": tr.P.cpu(), "grad": 3 * torch.randn(M, n, generator=g), "m": m0, "v": (m0.abs() + torch.rand(M, n, generator=g)) ** 2}
    for name in ("grad", "m", "v"):
        vals[name][:, 100:400] = 0.0
    for name, v in vals.items():
        getattr(tr, name).copy_(v)
    _hip.check(tr.k.lib.rbnn_nn_adam_step(C.byref(tr.net), t, lr, BETAS[0], BETAS[1], ADAM_EPS, _hip.stream_of(tr.P)), "rbnn_nn_adam_step")
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
            assert bool((diff[:, 100:400] == 0).all()), "a dead element moved"
        err = float(torch.where(sc > 0, diff / sc.clamp_min(1e-300), torch.where(diff == 0, 0.0, float("inf"))).max())
        assert err <= 2e-6, (name, err)
        worst = max(worst, err / 2e-6)
    print(f"[nn-train adam t={t}] worst error {worst:.3f} x (2e-6 x scale) over P, m, v of {M} members; excluded: nothing")


def _finalize_twice(ces, flags, B):
    """rbnn_nn_train_finalize alone, once per (ce, flags) pair of [M, B] tensors, on one accumulator -> stats.tolist() after every call."""
    from robustbnns_amd import _hip
    lib, M = _hip.load(), int(ces[0].shape[0])
    net, ws = _hip.NnTrainNet(), _hip.NnTrainWs()
    net.arch, net.activation, net.in_features, net.hidden, net.n_classes, net.n_members = 1, 1, 17, 32, 3, M
    stats = torch.zeros(M, 3, dtype=torch.float64, device=DEV)
    out = []
    for ce, fl in zip(ces, flags):
        ce_d, fl_d = ce.contiguous().to(DEV), fl.contiguous().to(DEV)
        ws.ce, ws.correct = _hip.ptr(ce_d), _hip.ptr(fl_d)
        _hip.check(lib.rbnn_nn_train_finalize(C.byref(net), C.byref(ws), B, _hip.ptr(stats), _hip.stream_of(stats)), "rbnn_nn_train_finalize")
        out.append(stats.tolist())                                         # synchronises: ce_d / fl_d outlive the launch
    return out


@pytest.mark.parametrize("B", [1, 256, 257, 600])
def test_finalize_sums_every_pass_of_its_loop_per_member(B):
    """M = 3 members with different hand-filled ce in [0, 5) and flags, two calls on one accumulator: B = 257 and 600 take the 256-wide loop
    into a second and a third pass.  Per member, stats[2]: the exact count.  stats[0]: an fp32 value within one fp32 ulp of the fp64 mean (a
    correctly rounded mean is within half an ulp; the fp64 sums, this one and the kernel's, err by at most B 2^-53 relative, so only a mean
    that close to an fp32 rounding tie can round to the other neighbour).  stats[1]: the fp64 sum of the two stats[0], exactly.  Member 1's
    row is what member 1 gets alone (M = 1), bit for bit: members 0 and 2 do not reach it."""
    M, g = 3, torch.Generator().manual_seed(9000 + B)
    ces = [5 * torch.rand(M, B, generator=g) for _ in range(2)]
    flags = [torch.randint(0, 2, (M, B), generator=g, dtype=torch.int32) for _ in range(2)]
    assert not torch.equal(ces[0][0], ces[0][1]) and not torch.equal(ces[0][2], ces[0][1])
    runs = _finalize_twice(ces, flags, B)
    alone = _finalize_twice([c[1:2] for c in ces], [f[1:2] for f in flags], B)
    worst = 0.0
    for m in range(M):
        losses, count = [], 0
        for i, got in enumerate(runs):
            mean64 = float(ces[i][m].double().sum()) / B
            ulp = float(np.spacing(np.float32(max(got[m][0], mean64))))
            losses.append(got[m][0])
            count += int(flags[i][m].sum())
            print(f"[nn-train finalize B={B} member {m}] step loss {got[m][0]!r}, fp64 mean {mean64!r}: |diff| = {abs(got[m][0] - mean64) / ulp:.3f} "
                  f"fp32 ulp; sum {got[m][1]!r}; count {got[m][2]} of {count}")
            assert got[m][0] == float(np.float32(got[m][0])) and abs(got[m][0] - mean64) <= ulp, (m, got[m][0], mean64, ulp)
            assert got[m][1] == sum(losses) and got[m][2] == count, (m, got[m], losses, count)
            worst = max(worst, abs(got[m][0] - mean64) / ulp)
    assert [r[1] for r in runs] == [r[0] for r in alone], (runs, alone)
    print(f"[nn-train finalize B={B}] worst step loss {worst:.3f} fp32 ulp from the fp64 mean (bar 1) over {M} members; member 1 in lockstep == alone; "
          f"excluded: nothing")


class _SviGradients:
    """SviTrainer's draw + training forward + weight gradients for a hidden size its constructor refuses: it sets up the accuracy forward, whose
    draw takes 16 or a multiple of 32 hidden units, and gradients() never runs that forward.  The same three entry points, in SviTrainer's order,
    on buffers laid out as its own (its attribute names)."""

    def __init__(self, arch, act, shape, Cn, loc, raw, key, B):
        from robustbnns_amd import _hip
        from robustbnns_amd.svi_train import state_keys
        self.hip, self.key, self.keys = _hip, key, state_keys(arch)
        self.shapes = {k: tuple(loc[k].shape) for k in self.keys}
        D, H = shape[0] * shape[1] * shape[2], self.shapes[self.keys[1]][0]
        z = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=DEV)
        flat = lambda d: torch.cat([d[k].reshape(-1).float() for k in self.keys]).to(DEV)
        self.loc, self.sigma = flat(loc), torch.nn.functional.softplus(flat(raw))
        self.n_params = self.loc.numel()
        self.W, self.grad = z(self.n_params), z(self.n_params)
        self.net = _hip.SviTrainNet()
        self.net.arch, self.net.activation = _hip.ARCHS[arch], _hip.ACTIVATIONS[act]
        self.net.in_features, self.net.hidden, self.net.n_classes = D, H, Cn
        for name in ("loc", "sigma", "W", "grad"):
            setattr(self.net, name, getattr(self, name).data_ptr())
        self.ws_t = {k + i: z(B, H) for i in (("1", "2") if arch == "fc2" else ("1",)) for k in ("hid", "dact", "dA")}
        self.ws_t["dZ"], self.ws_t["ce"] = z(B, _hip.CPAD), z(B)
        self.ws = _hip.SviTrainWs()
        for k in _hip.SVI_TRAIN_WS_KEYS:
            setattr(self.ws, k, _hip.ptr(self.ws_t.get(k)))
        self.D, self.Dp = D, 16 * ((D + 15) // 16)
        self.X, self.labels = z(B, self.Dp), torch.zeros(B, dtype=torch.int32, device=DEV)

    def unflat(self, buf):
        out, off = {}, 0
        for k in self.keys:
            n = 1
            for v in self.shapes[k]:
                n *= v
            out[k], off = buf[off:off + n].view(self.shapes[k]), off + n
        return out

    def gradients(self, x, labels):
        hip, B = self.hip, int(x.shape[0])
        self.X[:B, :self.D].copy_(x.reshape(B, -1))
        self.labels[:B].copy_(labels.reshape(B))
        lib, st, net = hip.HipKernels().lib, hip.stream_of(self.X), C.byref(self.net)
        hip.check(lib.rbnn_svi_train_draw(net, C.c_uint64(self.key), C.c_uint32(0), st), "rbnn_svi_train_draw")
        hip.check(lib.rbnn_svi_train_forward(net, hip.ptr(self.X), self.Dp, B, hip.ptr(self.labels), C.byref(self.ws), st), "rbnn_svi_train_forward")
        hip.check(lib.rbnn_svi_weight_grads(net, hip.ptr(self.X), self.Dp, B, C.byref(self.ws), st), "rbnn_svi_weight_grads")


@pytest.mark.parametrize("arch,act,D,H,Cn,B", [("fc", "tanh", 17, 96, 3, 32), ("fc2", "leaky", 10, 80, 10, 128), ("fc2", "sigm", 2, 16, 2, 64)])
def test_svi_and_nn_trainers_run_one_forward_and_backward(arch, act, D, H, Cn, B):
    """The SVI trainer (a summed CE) and an M = 1 NnTrainer (its mean) launch the same GEMM and head kernels: at the weights the SVI side drew,
    on the same staged batch, hid / act' / CE are equal bit for bit, and with B a power of two dZ and the weight gradients differ by the exact
    factor B.  The cases are the smallest with a ragged tile in each of M, N and K and with both forward epilogues.  Precondition (asserted, loc
    of std 0.1 and raw scale -3 keep the logits O(1)): no nonzero dZ, dA or gradient below 2^-100, so that 1 / B scales nothing into a denormal.
    Hidden 80 is a size SviTrainer's constructor refuses (its accuracy forward's draw: 16 or a multiple of 32): that case drives the same entry
    points through _SviGradients; the line printed says which side ran."""
    from robustbnns_amd.nn_train import NnTrainer
    from robustbnns_amd.svi_train import SviTrainer
    assert B & (B - 1) == 0
    shape, g = (1, D, 1), torch.Generator().manual_seed(D + H)
    shapes = O.param_shapes(arch, D, H, Cn)
    loc = {k: 0.1 * torch.randn(*s, generator=g) for k, s in shapes}
    raw = {k: torch.full(s, -3.0) for k, s in shapes}
    x, y = O.synthetic_inputs(B, shape, Cn, seed=D)
    x, lab = (4 * x - 2).to(DEV), y.argmax(-1).to(DEV)
    try:
        sv = SviTrainer(arch, act, shape, Cn, loc, raw, 0.01, DEV, 0x5EED, batch_size=B)
    except NotImplementedError:
        sv = _SviGradients(arch, act, shape, Cn, loc, raw, 0x5EED, B)
    sv.gradients(x, lab)
    nn = NnTrainer(arch, act, shape, Cn, [sv.unflat(sv.W)], 0.01, DEV, batch_size=B)
    nn.gradients(x, lab)
    torch.cuda.synchronize()
    assert torch.equal(nn.P[0], sv.W) and torch.equal(nn.X, sv.X) and torch.equal(nn.labels, sv.labels)
    layers = ("1", "2") if arch == "fc2" else ("1",)
    for k in ["dZ", "grad"] + ["dA" + i for i in layers]:
        nz = (sv.grad if k == "grad" else sv.ws_t[k]).abs()
        nz = nz[nz != 0]
        assert nz.numel() and float(nz.min()) >= 2.0 ** -100, (k, nz.numel())
    for k in ["ce"] + [n + i for i in layers for n in ("hid", "dact")]:
        assert torch.equal(nn.ws_t[k].view_as(sv.ws_t[k]), sv.ws_t[k]), k
    assert torch.equal(nn.ws_t["dZ"].view_as(sv.ws_t["dZ"]) * B, sv.ws_t["dZ"]), "dZ"
    assert torch.equal(nn.grad[0] * B, sv.grad), "grad"
    print(f"[nn-train = svi-train {arch} {D}->{H}->{Cn} {act} B={B}, SVI side: {type(sv).__name__}] ce, hid, act' equal; dZ and {sv.n_params} weight gradients "
          f"equal after the exact factor B; excluded: nothing")


def _lockstep_case():
    arch, act, shape, H, Cn, B, M = "fc2", "leaky", (1, 28, 28), 128, 10, 100, 7
    return (arch, act, shape, H, Cn, B, M), NR.grad_case(arch, act, shape, H, Cn, B, M)


def _run(params, c, case, rows_per_step, staged=False):
    from robustbnns_amd.nn_train import NnTrainer
    arch, act, shape, H, Cn, B, M = case
    tr = NnTrainer(arch, act, shape, Cn, params, 0.01, DEV, batch_size=B)
    tr.set_data(c["x"], c["lab"])
    xd, ld = c["x"].to(DEV), c["lab"].to(DEV)
    for rows in rows_per_step:
        if staged:
            tr.step(xd[rows[0].long()], ld[rows[0].long()])
        else:
            tr.step(rows=rows.contiguous())
    torch.cuda.synchronize()
    return _state(tr)


def test_lockstep_members_are_bit_identical_to_members_trained_alone_and_runs_repeat():
    case, c = _lockstep_case()
    M, B = case[-1], case[-2]
    g = torch.Generator().manual_seed(9)
    steps = [torch.stack([torch.randperm(len(c["lab"]), generator=g)[:b] for _ in range(M)]).to(torch.int32).to(DEV) for b in (B, B, 37)]
    together = _run(c["params"], c, case, steps)
    again = _run(c["params"], c, case, steps)
    for name in together:
        assert torch.equal(together[name], again[name]), f"two identical runs differ in {name}"
    for m in range(M):
        alone = _run(c["params"][m:m + 1], c, case, [r[m:m + 1] for r in steps])
        for name in together:
            assert torch.equal(together[name][m:m + 1], alone[name]), f"member {m} of the lockstep run differs from the member alone in {name}"
    assert float(together["stats"][:, 1].min()) > 0
    print(f"[nn-train lockstep fc2 784->128->10 M={M}] P, m, v, grad, stats of every member bit-identical to M = 1 runs after 3 steps (B = {B}, {B}, 37) "
          f"and between two runs; excluded: nothing")


def test_gathered_rows_equal_a_staged_copy_of_the_same_rows():
    case, c = _lockstep_case()
    M, B = case[-1], case[-2]
    g = torch.Generator().manual_seed(10)
    one = [torch.randperm(len(c["lab"]), generator=g)[:b].to(torch.int32).to(DEV) for b in (B, 37)]
    shared = [r[None].repeat(M, 1) for r in one]                      # every member on the same rows: what a staged batch means
    gathered, staged = _run(c["params"], c, case, shared), _run(c["params"], c, case, shared, staged=True)
    for name in gathered:
        assert torch.equal(gathered[name], staged[name]), name
    g1, s1 = _run(c["params"][:1], c, case, [r[None] for r in one]), _run(c["params"][:1], c, case, [r[None] for r in one], staged=True)
    for name in g1:
        assert torch.equal(g1[name], s1[name]), name
    print(f"[nn-train gather] rows through the index array = a staged copy of them, bit for bit (M = {M} and M = 1, B = {B} then 37); excluded: nothing")


def _poisoned(arch, D, Cn, B, M, poison, use_rows):
    """One step on B < Bmax points; poison: NaN in everything the entry points have no business reading (the workspaces behind [M, B, .], rows >=
    B and columns [D, Dp) of the staging matrix, pool rows no member names) and a class >= C in the labels nobody names."""
    from robustbnns_amd.nn_train import NnTrainer
    shape, H = (1, D, 1), 32
    g = torch.Generator().manual_seed(D + B)
    params = [{k: 0.5 * torch.randn(*s, generator=g) for k, s in O.param_shapes(arch, D, H, Cn)} for _ in range(M)]
    x, y = O.synthetic_inputs(3 * B, shape, Cn, seed=D)
    x, lab = 4 * x - 2, y.argmax(-1)
    tr = NnTrainer(arch, "leaky", shape, Cn, params, 0.01, DEV, batch_size=64)
    assert B < tr.Bmax and tr.Dp > D
    rows = torch.stack([torch.randperm(3 * B, generator=g)[:B] for _ in range(M)])
    tr.set_data(x, lab)
    nan = float("nan")
    if poison:
        for k, v in tr.ws_t.items():
            per = v.numel() // (M * tr.Bmax)
            v[M * B * per:] = Cn if k == "correct" else nan
        tr.X[B:] = nan
        tr.X[:B, D:] = nan
        tr.labels[B:] = Cn
        unused = torch.ones(3 * B, dtype=torch.bool)
        unused[rows.reshape(-1)] = False
        if use_rows:
            tr.data[unused.to(DEV)] = nan
            tr.data_labels[unused.to(DEV)] = Cn
        else:
            tr.data[:] = nan
            tr.data_labels[:] = Cn
    if use_rows:
        tr.step(rows=rows.to(torch.int32).to(DEV))
    else:
        tr.step(x[rows[0]].to(DEV), lab[rows[0]].to(DEV))
    torch.cuda.synchronize()
    res = _state(tr)
    res["ce"], res["correct"] = _bits(tr.ws_t["ce"][:M * B]), _bits(tr.ws_t["correct"][:M * B])
    for name in ("P", "m", "v", "grad", "ce"):
        assert bool(torch.isfinite(res[name].view(torch.float32)).all()), name
    assert bool(torch.isfinite(tr.stats).all())
    return res


@pytest.mark.parametrize("use_rows", [False, True])
@pytest.mark.parametrize("arch,D,Cn,B,M", [("fc", 2, 2, 37, 3), ("fc", 10, 3, 5, 1), ("fc", 17, 10, 61, 2), ("fc2", 2, 2, 3, 3), ("fc2", 10, 10, 37, 2),
                                           ("fc2", 17, 3, 1, 3)])
def test_nothing_behind_the_bounds_is_read(arch, D, Cn, B, M, use_rows):
    """NaN is data: every index stays inside its allocation, and a NaN that leaked into a sum would stay there."""
    clean, dirty = _poisoned(arch, D, Cn, B, M, False, use_rows), _poisoned(arch, D, Cn, B, M, True, use_rows)
    for name in clean:
        assert torch.equal(clean[name], dirty[name]), f"{name} depends on memory behind the bounds"
    print(f"[nn-train bounds {arch} D={D} C={Cn} B={B} M={M} rows={use_rows}] {len(clean)} results bit-identical with NaN behind [M, B, .], in rows >= {B} and "
          f"columns [{D}, Dp) of the staged batch and in every pool row no member names; excluded: nothing")


# The trajectory bar.  The fixture's `spread` is the distance of the REFERENCE's fp32 run from the fp64 restatement of the same run, relative to
# the largest parameter.  Two correct fp32 implementations with different summation orders can each sit one spread from fp64 (2), and the MFMA
# GEMM accumulates in another order than torch's CPU GEMM at every layer of every step, forward and backward (x 2): 4 spreads.
TRAJ_SPREADS = 4


def _nn_of(meta):
    from robustbnns_amd.model_nn import NN
    return NN(meta["dataset"], tuple(meta["shape"]), meta["n_classes"], meta["hidden"], meta["act"], meta["arch"], meta["lr"], meta["epochs"])


def _check_lines(out_lines, meta, runs64, offset, what):
    """Accuracy equal to the reference's line where no point of the epoch is within the margin.  Loss: to the digits the spread allows, not to
    all 8 — within TRAJ_SPREADS x the larger of the reference's own distance from the fp64 restatement's epoch loss and spread x the loss (a
    relative parameter perturbation of one spread moves the logits, and with them a loss of order 1 per point, by that relative amount), plus
    the 8th digit both lines are rounded to."""
    per = len(runs64.losses) // meta["epochs"]
    for e in range(meta["epochs"]):
        loss_ref, acc_ref = meta["lines"][offset + e]
        loss, acc = out_lines[offset + e]
        loss64 = sum(runs64.losses[e * per:(e + 1) * per]) / meta["N"]
        bar = TRAJ_SPREADS * max(abs(loss_ref - loss64), meta["spread"] * abs(loss_ref)) + 1e-8
        print(f"   {what} epoch {e + 1}: loss {loss:.8f} reference {loss_ref:.8f} fp64 {loss64:.10f}: |diff| = {abs(loss - loss_ref) / bar:.3f} x bar; accuracy {acc} / {acc_ref}")
        assert abs(loss - loss_ref) <= bar
        if sum(runs64.n_marginal[e * per:(e + 1) * per]) == 0:
            assert acc == acc_ref


@pytest.mark.parametrize("name", NR.NN_CASES)
def test_nn_train_follows_the_fp64_restatement_of_the_references_run(name, capsys):
    from robustbnns_amd.nn_train import NnTrainer
    meta, arr = NR.load(name)
    arch = meta["arch"]
    r64, before = NR.run_nn_case(name, torch.float64)
    scale = NR.param_scale(r64.params())
    bar = TRAJ_SPREADS * meta["spread"] * scale
    # per step, with a hand-driven trainer on the same batches
    x, lab = arr["x"], arr["y"].argmax(-1)
    tr = NnTrainer(arch, meta["act"], tuple(meta["shape"]), meta["n_classes"], [NR.state_of(arr, "init:", arch)], meta["lr"], DEV, batch_size=meta["batch"])
    worst, i = 0.0, 0
    for _ in range(meta["epochs"]):
        for s in range(0, meta["N"], meta["batch"]):
            d = NR.max_diff({k: v.cpu() for k, v in tr.params()[0].items()}, before[i])
            assert d <= bar, (i, d, bar)
            worst, i = max(worst, d), i + 1
            tr.step(x[s:s + meta["batch"]].to(DEV), lab[s:s + meta["batch"]].to(DEV))
    final_hand = {k: v.cpu() for k, v in tr.params()[0].items()}
    d = NR.max_diff(final_hand, r64.params())
    worst = max(worst, d)
    assert d <= bar
    # NN.train itself: the same kernels in the same order
    net = _nn_of(meta)
    net.load_state_dict(NR.state_of(arr, "init:", arch))
    loader = DataLoader(TensorDataset(x, arr["y"]), batch_size=meta["batch"], shuffle=False)
    capsys.readouterr()
    net.train(loader, DEV, seed=meta["seed"], save=False)
    out = capsys.readouterr().out
    for k, v in net.state_dict().items():
        assert torch.equal(v, final_hand[k]), k
    assert net.device == DEV and " == NN training ==" in out
    print(f"[nn-train trajectory {name}] {i} steps: max |P - fp64| = {worst:.2e} = {worst / (meta['spread'] * scale):.3f} x spread ({meta['spread']:.2e} x {scale:.2f}), "
          f"bar {TRAJ_SPREADS}; the reference's own fp32 run: 1.000")
    _check_lines(NR.parse_epoch_lines(out), meta, r64, 0, name)
    if meta["dataset"] == "half_moons":               # the trained module drives the attack engine: its cache key saw the new parameters
        assert float((net.forward(x[:8], DEV).cpu().double() - NR.logits(x[:8].double(), r64.params(), arch, meta["act"])).abs().max()) < 1e-2


def _train_ens(meta, arr):
    from robustbnns_amd.model_ensemble import Ensemble_NN
    torch.manual_seed(meta["seed0"])
    ens = Ensemble_NN(meta["dataset"], meta["hidden"], meta["act"], meta["arch"], meta["epochs"], meta["lr"], tuple(meta["shape"]), meta["n_classes"], meta["M"])
    ens.train(arr["x"], arr["y"], DEV)
    return ens


@pytest.mark.parametrize("name", NR.ENS_CASES)
def test_ensemble_train_follows_the_fp64_restatement_of_the_references_run(name, capsys):
    meta, arr = NR.load(name)
    r64 = NR.run_ens_case(name, torch.float64)
    capsys.readouterr()
    ens = _train_ens(meta, arr)
    out = capsys.readouterr().out
    lines = NR.parse_epoch_lines(out)
    assert list(ens.ensemble_models) == [str(s) for s in range(meta["M"])] and len(lines) == meta["M"] * meta["epochs"]
    worst = 0.0
    for m in range(meta["M"]):
        scale = NR.param_scale(r64[m].params())
        d = NR.max_diff(dict(ens.ensemble_models[str(m)].state_dict()), r64[m].params())
        assert d <= TRAJ_SPREADS * meta["spread"] * scale, (m, d)
        worst = max(worst, d / (meta["spread"] * scale))
        _check_lines(lines, meta, r64[m], m * meta["epochs"], f"{name} member {m}")
    print(f"[nn-train trajectory {name}] M = {meta['M']}, {meta['epochs']} epochs of N = {meta['N']} in batches of 100: max |P - fp64| = {worst:.3f} x spread "
          f"({meta['spread']:.2e}), bar {TRAJ_SPREADS}")


def test_trained_ensemble_and_net_round_trip_through_their_files(tmp_path, monkeypatch):
    import os
    from robustbnns_amd.model_ensemble import Ensemble_NN
    from robustbnns_amd.savedir import TESTS
    meta, arr = NR.load(NR.ENS_CASES[0])
    x = arr["x"][:64]
    stores = []
    for run in ("a", "b"):
        os.makedirs(tmp_path / run)
        monkeypatch.chdir(tmp_path / run)
        ens = _train_ens(meta, arr)
        member = ens.ensemble_models["0"].name
        files = sorted(os.listdir(os.path.join(TESTS, ens.name, "weights")))
        assert files == [f"{member}_weights_{s}.pt" for s in range(meta["M"])]
        stores.append([torch.load(os.path.join(TESTS, ens.name, "weights", f), weights_only=False) for f in files])
    for a, b in zip(*stores):
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    fresh = Ensemble_NN(meta["dataset"], meta["hidden"], meta["act"], meta["arch"], meta["epochs"], meta["lr"], tuple(meta["shape"]), meta["n_classes"], meta["M"])
    fresh.load(DEV)
    assert torch.equal(fresh.forward(x, n_samples=meta["M"]), ens.forward(x, n_samples=meta["M"]))
    assert torch.equal(fresh.forward(x, n_samples=2), ens.forward(x, n_samples=2))
    # NN.train with save=True, then load
    nmeta, narr = NR.load(NR.NN_CASES[0])
    nets = []
    for _ in range(2):
        net = _nn_of(nmeta)
        net.load_state_dict(NR.state_of(narr, "init:", nmeta["arch"]))
        net.train(DataLoader(TensorDataset(narr["x"], narr["y"]), batch_size=nmeta["batch"]), DEV)
        nets.append(net)
    again = _nn_of(nmeta)
    again.load(DEV)
    for k, v in nets[1].state_dict().items():
        assert torch.equal(v, again.state_dict()[k]) and torch.equal(v, nets[0].state_dict()[k]), k
    assert torch.equal(again.forward(narr["x"][:16], DEV), nets[1].forward(narr["x"][:16], DEV))


def test_fifty_lockstep_steps_make_no_device_to_host_sync():
    from robustbnns_amd.nn_train import NnTrainer
    M, B, N = 5, 100, 2000
    g = torch.Generator().manual_seed(2)
    params = [{k: 0.05 * torch.randn(*s, generator=g) for k, s in O.param_shapes("fc2", 784, 256, 10)} for _ in range(M)]
    tr = NnTrainer("fc2", "leaky", (1, 28, 28), 10, params, 0.01, DEV, batch_size=B)
    tr.set_data(torch.rand(N, 1, 28, 28, generator=g), torch.randint(0, 10, (N,), generator=g))
    sched = torch.stack([torch.randperm(N, generator=g) for _ in range(3 * M)]).view(M, 3 * N).to(torch.int32).to(DEV)
    xs, ls = torch.rand(B, 1, 28, 28, device=DEV), torch.randint(0, 10, (B,), device=DEV)
    tr.step(rows=sched[:, :B].contiguous())
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for i in range(1, 51):
            tr.step(rows=sched[:, i * B:(i + 1) * B].contiguous())
        tr.step(xs, ls)                                   # the staged path as well
    finally:
        torch.cuda.set_sync_debug_mode(0)
    totals = tr.epoch_totals()
    assert tr.t == 52 and len(totals) == M and all(loss == loss and 0 <= correct <= 52 * B for loss, correct in totals)


def test_guards_raise_not_implemented_with_no_state_changed():
    from robustbnns_amd.model_ensemble import Ensemble_NN
    from robustbnns_amd.model_nn import NN
    from robustbnns_amd.nn_train import NnTrainer
    x, y = O.synthetic_inputs(16, (1, 28, 28), 10, seed=1)
    loader = DataLoader(TensorDataset(x, y), batch_size=8)
    conv = NN("mnist", (1, 28, 28), 10, 16, "leaky", "conv", 0.01, 1)
    before = {k: v.clone() for k, v in conv.state_dict().items()}
    with pytest.raises(NotImplementedError, match="conv"):
        conv.train(loader, DEV)
    assert all(torch.equal(v, before[k]) for k, v in conv.state_dict().items()) and not hasattr(conv, "device")
    ens = Ensemble_NN("mnist", 16, "leaky", "conv", 1, 0.01, (1, 28, 28), 10, 2)
    with pytest.raises(NotImplementedError, match="conv"):
        ens.train(x, y, DEV)
    with pytest.raises(NotImplementedError, match="no CPU compute path"):
        Ensemble_NN("mnist", 16, "leaky", "fc", 1, 0.01, (1, 28, 28), 10, 2).train(x, y, "cpu")
    assert ens.ensemble_models == {}
    fc = NN("mnist", (1, 28, 28), 10, 16, "leaky", "fc", 0.01, 1)
    with pytest.raises(NotImplementedError, match="no CPU compute path"):
        fc.train(loader, "cpu")
    # a trainer refuses rows it cannot use before anything is launched: no half-applied step
    tr = NnTrainer("fc", "leaky", (1, 28, 28), 10, [fc.state_dict()], 0.01, DEV, batch_size=8)
    keep = _state(tr)
    with pytest.raises(ValueError):
        tr.step(rows=torch.zeros(1, 8, dtype=torch.int32, device=DEV))              # no resident data
    tr.set_data(x, y.argmax(-1))
    for bad in (torch.zeros(2, 8, dtype=torch.int32, device=DEV), torch.zeros(1, 8, dtype=torch.int64, device=DEV), torch.zeros(1, 8, dtype=torch.int32)):
        with pytest.raises(ValueError):
            tr.step(rows=bad)
    now = _state(tr)
    assert tr.t == 0 and all(torch.equal(keep[k], now[k]) for k in keep)
    assert fc.train(False) is fc and fc.training is False
