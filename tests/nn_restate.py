"""CPU restatement of deterministic training (what robustbnns_amd.nn_train.NnTrainer computes; model_nn.py:175-219) in any float dtype:
plain torch autograd on the mean cross-entropy + torch.optim.Adam, from a recorded init over recorded batches.  In fp32 it lands on the
reference's recorded parameters (tests/test_nn_train_cpu.py); in fp64 it is the yardstick of the GPU tests.  Also the helpers the
nn_train fixtures (tests/golden/nn_train_*.npz, written by tests/golden/make_golden_nn_train.py) are read with."""
import ast
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import bnn_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NN_CASES = ["nn_train_nn_moons_fc2_h32", "nn_train_nn_small_fc_h16"]
ENS_CASES = ["nn_train_ens_moons_fc_h32", "nn_train_ens_small_fc2_h16"]
# A point whose two largest fp64 LOGITS are this close (relative to the point's largest |logit|) may be scored either way: the GPU's logits are
# within the forward bar 1e-5 max|z| of fp64 each, so two of them can swap order only if their fp64 gap is below 2e-5 max|z|.
MARGIN = 2e-5


def layer_keys(arch):
    return {"fc": ("model.1", "model.3"), "fc2": ("model.1", "model.3", "model.5")}[arch]


def state_keys(arch):
    return [k + s for k in layer_keys(arch) for s in (".weight", ".bias")]


def logits(x, W, arch, act):
    h = x.reshape(x.shape[0], -1)
    ks = layer_keys(arch)
    for i, k in enumerate(ks):
        h = h @ W[k + ".weight"].T + W[k + ".bias"]
        if i + 1 < len(ks):
            h = O._act(h, act)
    return h


def hidden_preacts(x, W, arch, act):
    """Every hidden pre-activation of the batch, concatenated per point [B, sum H] (the kink margin of relu / leaky)."""
    h, out = x.reshape(x.shape[0], -1), []
    for k in layer_keys(arch)[:-1]:
        a = h @ W[k + ".weight"].T + W[k + ".bias"]
        out.append(a)
        h = O._act(a, act)
    return torch.cat(out, 1)


def first_argmax(z):
    best = torch.zeros(z.shape[0], dtype=torch.long)
    top = z[:, 0].clone()
    for c in range(1, z.shape[1]):
        better = z[:, c] > top
        best[better] = c
        top = torch.where(better, z[:, c], top)
    return best


def marginal(z):
    """Points whose two largest logits are within MARGIN x max|z| of each other (none for a single class)."""
    if z.shape[1] < 2:
        return torch.zeros(z.shape[0], dtype=torch.bool)
    t = z.topk(2, dim=-1)[0]
    return (t[:, 0] - t[:, 1]) < MARGIN * z.abs().max(-1)[0]


class Restatement:
    """One member: step(x, labels) = optimizer.zero_grad(); loss = CrossEntropyLoss()(net(x), labels); loss.backward(); optimizer.step()."""

    def __init__(self, params, arch, act, lr, dtype=torch.float64):
        self.arch, self.act, self.dtype = arch, act, dtype
        self.W = {k: params[k].detach().cpu().to(dtype).clone().requires_grad_(True) for k in state_keys(arch)}
        self.opt = torch.optim.Adam(list(self.W.values()), lr=lr)
        self.losses, self.correct, self.n_marginal = [], [], []

    def step(self, x, labels):
        self.opt.zero_grad()
        z = logits(x.to(self.dtype), self.W, self.arch, self.act)
        loss = F.cross_entropy(z, labels)
        loss.backward()
        self.opt.step()
        zd = z.detach()
        mg = marginal(zd)
        self.losses.append(float(loss.detach()))
        self.correct.append(int(((first_argmax(zd) == labels) & ~mg).sum()))
        self.n_marginal.append(int(mg.sum()))

    def params(self):
        return {k: v.detach().clone() for k, v in self.W.items()}


def load(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    meta = ast.literal_eval(str(d["meta"]))
    return meta, {k: torch.from_numpy(np.asarray(d[k])) for k in d.files if k != "meta"}


def state_of(arr, prefix, arch):
    return {k: arr[prefix + k] for k in state_keys(arch)}


def run_nn_case(name, dtype):
    """The NN.train fixture's run restated: returns (Restatement, list of the parameters BEFORE every step)."""
    meta, arr = load(name)
    x, lab = arr["x"], arr["y"].argmax(-1)
    r = Restatement(state_of(arr, "init:", meta["arch"]), meta["arch"], meta["act"], meta["lr"], dtype)
    before = []
    for _ in range(meta["epochs"]):
        for i in range(0, meta["N"], meta["batch"]):
            before.append(r.params())
            r.step(x[i:i + meta["batch"]], lab[i:i + meta["batch"]])
    return r, before


def run_ens_case(name, dtype):
    """The Ensemble_NN.train fixture's run restated member by member over the recorded rows: a list of Restatements."""
    meta, arr = load(name)
    x, lab = arr["x"], arr["y"].argmax(-1)
    out = []
    for m in range(meta["M"]):
        r = Restatement(state_of(arr, f"init{m}:", meta["arch"]), meta["arch"], meta["act"], meta["lr"], dtype)
        for e in range(meta["epochs"]):
            rows = arr["rows"][m, e]
            for i in range(0, meta["N"], 100):
                r.step(x[rows[i:i + 100]], lab[rows[i:i + 100]])
        out.append(r)
    return out


def param_scale(p):
    return max(float(v.abs().max()) for v in p.values())


def max_diff(a, b):
    return max(float((a[k].double() - b[k].double()).abs().max()) for k in a)


def parse_epoch_lines(text):
    """[(loss, accuracy)] of the reference's epoch lines in captured output."""
    import re
    return [(float(a), float(b)) for a, b in re.findall(r"\[Epoch \d+\]\t loss: ([0-9.eE+-]+) \t accuracy: ([0-9.]+)", text)]


# ------------------------------------------------------------------ the kernel-level cases shared by the host and the GPU tier
KINK = 2e-6          # tests/test_hip_svi_train.py's: points with a hidden pre-activation this close to 0 are left out (act' jumps there)
# (arch, act, shape, H, C, B, M): fc / fc2, the four activations, a partial 64-tile beside a full one (H = 96, 160), H = 1024, D % 16 != 0
# (10, 17), D = 3072, 1 and 16 classes, B = 1, 3, 65, 100, 300, M = 1, 3, 7
GRAD_CASES = [("fc", "leaky", (1, 28, 28), 128, 10, 100, 3), ("fc2", "leaky", (1, 28, 28), 128, 10, 100, 7), ("fc", "relu", (1, 28, 28), 512, 10, 100, 1),
              ("fc2", "tanh", (1, 28, 28), 256, 10, 65, 3), ("fc2", "sigm", (1, 2, 1), 32, 2, 100, 7), ("fc", "sigm", (1, 28, 28), 96, 10, 65, 3),
              ("fc2", "relu", (1, 28, 28), 160, 10, 300, 3), ("fc", "leaky", (1, 28, 28), 1024, 10, 100, 3), ("fc2", "tanh", (1, 28, 28), 1024, 10, 65, 1),
              ("fc", "leaky", (1, 5, 2), 96, 2, 65, 7), ("fc", "tanh", (1, 17, 1), 160, 10, 3, 3), ("fc2", "leaky", (1, 17, 1), 96, 10, 65, 3),
              ("fc", "relu", (3, 32, 32), 128, 10, 65, 1), ("fc2", "sigm", (3, 32, 32), 96, 10, 100, 3), ("fc", "leaky", (1, 28, 28), 32, 1, 65, 3),
              ("fc", "tanh", (1, 28, 28), 64, 16, 65, 7), ("fc2", "leaky", (1, 28, 28), 128, 16, 300, 1), ("fc2", "sigm", (1, 28, 28), 64, 10, 1, 3),
              ("fc", "leaky", (1, 28, 28), 128, 10, 1, 7), ("fc2", "relu", (1, 17, 1), 32, 10, 3, 7)]


def grad_case(arch, act, shape, H, Cn, B, M):
    """The inputs of one GRAD_CASES case, from the oracle alone (no GPU): M members' parameters, a resident pool of points none of which is
    within KINK of an activation kink for any member, labels (every other point: member 0's fp64 prediction, so that both branches of the
    head kernel's CE are met and the correct count is far from 0), and each member's own B rows of the pool."""
    D = shape[0] * shape[1] * shape[2]
    g = torch.Generator().manual_seed(1000 * H + 10 * B + M)
    std = 0.05 if D > 16 else 0.5
    params = [{k: std * torch.randn(*s, generator=g) for k, s in O.param_shapes(arch, D, H, Cn)} for _ in range(M)]
    n_pool = 2 * B + 8
    x, y = O.synthetic_inputs(n_pool, shape, Cn, seed=B + M)
    if D <= 16:
        x = 4 * x - 2
    lab = y.argmax(-1)
    p64 = [{k: v.double() for k, v in p.items()} for p in params]
    ok = torch.ones(n_pool, dtype=torch.bool)
    if act in ("relu", "leaky"):
        for p in p64:
            ok &= hidden_preacts(x.double(), p, arch, act).abs().min(1)[0] > KINK
    n_kink = int((~ok).sum())
    x, lab = x[ok], lab[ok]
    z0 = logits(x.double(), p64[0], arch, act)
    lab = torch.where(torch.arange(len(lab)) % 2 == 0, first_argmax(z0), lab)
    rows = torch.stack([torch.randperm(len(lab), generator=g)[:B] for _ in range(M)]).to(torch.int32)
    return {"D": D, "params": params, "p64": p64, "x": x, "lab": lab, "rows": rows, "n_kink": n_kink, "n_pool": n_pool}


def member_fp64(c, m, arch, act):
    """fp64 autograd at member m's parameters on its rows: (mean CE, {key: gradient}, per-point CE, on the log1pf branch, correct among the
    non-marginal points, marginal points)."""
    r = c["rows"][m].long()
    x, lab = c["x"][r].double(), c["lab"][r]
    W = {k: v.clone().requires_grad_(True) for k, v in c["p64"][m].items()}
    z = logits(x, W, arch, act)
    ce = torch.logsumexp(z, -1) - z.gather(1, lab[:, None])[:, 0]
    loss = ce.mean()
    loss.backward()
    zd = z.detach()
    mg = marginal(zd)
    return {"loss": float(loss.detach()), "grad": {k: v.grad for k, v in W.items()}, "ce": ce.detach(),
            "log1p": zd.gather(1, lab[:, None])[:, 0] == zd.max(-1)[0],
            "c_safe": int(((first_argmax(zd) == lab) & ~mg).sum()), "n_marginal": int(mg.sum())}
