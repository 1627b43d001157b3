"""CPU restatement of deterministic conv training (what robustbnns_amd.conv_train.ConvNnTrainer computes; model_nn.py:93-106, 175-219) in any
float dtype: an nn.Sequential of the same six layers, plain torch autograd on the mean cross-entropy + torch.optim.Adam.  In fp64 it is the
yardstick of tests/test_hip_conv_train.py; tests/test_conv_train_cpu.py holds it against itself in fp32.  Also the inputs of both tiers: the
gradient cases (with what they leave out, decided by the fp64 evaluation alone) and the trajectory case."""
import torch
import torch.nn.functional as F
from torch import nn

import nn_restate as NR

KEYS = [k + s for k in ("model.0", "model.3", "model.7") for s in (".weight", ".bias")]
SHAPE = (1, 28, 28)
_ACT = {"relu": nn.ReLU, "leaky": nn.LeakyReLU, "sigm": nn.Sigmoid, "tanh": nn.Tanh}
# relu / leaky have a kink and both max-pools have ties: a point whose fp64 forward has a conv pre-activation within KINK of 0 (relu / leaky),
# or a pooling window whose two largest pre-activations are within TIE of each other, is legitimately discontinuous — fp32 may route the
# gradient elsewhere.  Such points are never in a batch.
KINK = 2e-6
TIE = 2e-6
# (Hc, act, B, C): a one-tile and a three-tile Hc, the four activations, B = 1, an odd B, a B past a 64-point boundary, fewer than 16 classes
GRAD_CASES = [(16, "leaky", 8, 10), (16, "relu", 5, 3), (32, "tanh", 8, 10), (16, "sigm", 3, 10), (48, "leaky", 16, 10), (64, "leaky", 1, 10),
              (16, "leaky", 65, 2)]
# ... and the cases named by the regime of the weight gradients' slice plan (slice_plan below) that they reach, which the seven above do not
# (one point per slice of dK1, at most 5 of dK2, one 16-channel group per slice of dP1: no fold, no ragged slice):
#   (144, tanh, 129, 10)  dP1: 291 tiles (the last one ragged), 5 slices of 2 groups, the last of 1 group; dK2: 15 slices of 9 points, the last
#                         of 3, 36 stages (one fold), M = 144 leaves a ragged 64-row tile; dK1: 65 slices of 2 points, the last of 1, 72 stages
#   (80, relu, 300, 10)   dP1: 3 slices of 2 groups, the last of 1; dK2: 16 slices of 19 points, the last of 15; dK1: 100 slices of 3 points
#   (48, leaky, 500, 3)   dP1: ONE slice of 3 groups, 75 stages (two folds); dK2: 16 slices of 32 points, the last of 20, 128 stages (a fold on
#                         the last stage); dK1: 125 slices of 4 points
#   (16, sigm, 129, 2)    the fourth activation past B = 128, the fewest classes; dP1: one group; dK2 and dK1 as the first
REGIME_CASES = [(144, "tanh", 129, 10), (80, "relu", 300, 10), (48, "leaky", 500, 3), (16, "sigm", 129, 2)]
GRAD_CASES += REGIME_CASES

# ------------------------------------------------------------------ the slice plan of the three conv GEMMs of the weight gradients
# Restated from the comments of csrc/rbnn_conv_train.hip.  Every contraction is split across blocks and K is staged STAGE_K at a time; inside
# a slice the running accumulator is folded into a second one every FOLD_STAGES stages.
#   dK2: K = (point, 64 positions), split over the batch: never more than min(B, MAX_SPLITS2) slices
#   dK1: K = (point, 576 positions), split over the batch: never more than min(B, MAX_SPLITS1) slices
#   dP1: K = (conv2 channel, 25 taps), M = (point, 144 pooled positions) in tiles of TILE_M rows, split over groups of GROUP conv2 channels
#        (GROUP_K = 400 products): as many slices as bring the grid to DP1_BLOCKS blocks, at most one per group and at least one
MAX_SPLITS2, MAX_SPLITS1, DP1_BLOCKS = 16, 128, 2048
TILE_M, GROUP, GROUP_K, STAGE_K, FOLD_STAGES = 64, 16, 400, 16, 32
PP1, C1, N2, N1 = 144, 32, 801, 26                # pooled conv1 positions, conv1 channels, columns of a dK2 / dK1 partial (the taps | the bias)
POINT_K = {"dK2": 64, "dK1": 576}                 # products one point adds to the contraction


def _cdiv(a, b):
    return -(-a // b)


def slice_plan(B, Hc):
    """{"dP1": (per, n), "dK2": (per, n), "dK1": (per, n)}: n slices of `per` units each (the last one: what remains) — a unit is one point
    for dK2 and dK1 and one group of 16 conv2 channels for dP1."""
    plan = {}
    for name, cap in (("dK2", MAX_SPLITS2), ("dK1", MAX_SPLITS1)):
        per = _cdiv(B, cap)
        plan[name] = (per, _cdiv(B, per))
    tiles, groups = _cdiv(B * PP1, TILE_M), Hc // GROUP
    want = min(max(DP1_BLOCKS // tiles, 1), groups)
    per = _cdiv(groups, want)
    plan["dP1"] = (per, _cdiv(groups, per))
    return plan


def plan_units(B, Hc):
    """The units each GEMM's slices share out: B points for dK2 and dK1, Hc / 16 groups for dP1."""
    return {"dP1": Hc // GROUP, "dK2": B, "dK1": B}


def plan_stages(B, Hc):
    """Stages of a full slice per GEMM (the fold fires after every FOLD_STAGES of them)."""
    p = slice_plan(B, Hc)
    return {"dP1": p["dP1"][0] * GROUP_K // STAGE_K, "dK2": p["dK2"][0] * POINT_K["dK2"] // STAGE_K, "dK1": p["dK1"][0] * POINT_K["dK1"] // STAGE_K}


def plan_floats(B, Hc):
    """Floats of partP, part2 and part1 that a step on B points writes: slices x M x N of each GEMM."""
    p = slice_plan(B, Hc)
    return {"partP": p["dP1"][1] * B * PP1 * C1, "part2": p["dK2"][1] * Hc * N2, "part1": p["dK1"][1] * C1 * N1}


def sequential(act, Hc, Cn, dtype=torch.float64):
    """The reference's conv stack (model_nn.py:98-106) for 1x28x28 inputs."""
    m = nn.Sequential(nn.Conv2d(1, 32, kernel_size=5), _ACT[act](), nn.MaxPool2d(kernel_size=2), nn.Conv2d(32, Hc, kernel_size=5), _ACT[act](),
                      nn.MaxPool2d(kernel_size=2, stride=1), nn.Flatten(), nn.Linear(49 * Hc, Cn))
    return m.to(dtype)


def fresh_params(act, Hc, Cn, seed):
    """The parameters of a freshly initialised stack, keyed like NN.state_dict(); the global generator is left as it was."""
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        sd = sequential(act, Hc, Cn, torch.float32).state_dict()
    return {"model." + k: v.clone() for k, v in sd.items()}


def module_of(params, act, dtype):
    Hc, Cn = int(params["model.3.bias"].shape[0]), int(params["model.7.bias"].shape[0])
    m = sequential(act, Hc, Cn, dtype)
    m.load_state_dict({k[len("model."):]: v.detach().to(dtype) for k, v in params.items()})
    return m


def logits(x, params, act):
    """fp64 logits of x [B, 1, 28, 28] at `params` (no autograd)."""
    with torch.no_grad():
        return module_of(params, act, torch.float64)(x.double())


def _window_gap(a, stride):
    """Per point: the smallest gap between the two largest values of any 2 x 2 pooling window of a [B, C, H, W]."""
    w = a.unfold(2, 2, stride).unfold(3, 2, stride).reshape(a.shape[0], -1, 4)
    t = w.topk(2, dim=-1)[0]
    return (t[..., 0] - t[..., 1]).min(1)[0]


def discontinuous(x, params, act):
    """bool [B]: the points of x whose fp64 forward at `params` sits within KINK of an activation kink (relu / leaky) or within TIE of a
    pooling tie (either pool)."""
    with torch.no_grad():
        m = module_of(params, act, torch.float64)
        a1 = m[0](x.double())
        a2 = m[3](m[2](m[1](a1)))
        bad = (_window_gap(a1, 2) < TIE) | (_window_gap(a2, 1) < TIE)
        if act in ("relu", "leaky"):
            bad |= (a1.abs().reshape(len(x), -1).min(1)[0] < KINK) | (a2.abs().reshape(len(x), -1).min(1)[0] < KINK)
    return bad


_CASES = {}


def grad_case(Hc, act, B, Cn):
    """The inputs of one GRAD_CASES case (computed once, shared, never modified): a freshly initialised stack's parameters, the first B of a pool
    of 3 B + 8 torch.rand images that are not discontinuous, labels (every other point: the fp64 prediction, so that both branches of the
    head's CE are met and the correct count is far from 0), and the fp64 reference."""
    key = (Hc, act, B, Cn)
    if key in _CASES:
        return _CASES[key]
    seed = 1000 * Hc + 10 * B + Cn + 3              # (+ 3: with it every case's pool keeps the cap of tests/test_conv_train_cpu.py, at most a third dropped)
    g = torch.Generator().manual_seed(seed)
    params = fresh_params(act, Hc, Cn, seed)
    n_pool = 3 * B + 8
    x = torch.rand(n_pool, *SHAPE, generator=g)
    lab = torch.randint(0, Cn, (n_pool,), generator=g)
    bad = discontinuous(x, params, act)
    n_drop = int(bad.sum())
    x, lab = x[~bad][:B], lab[~bad][:B]
    z0 = logits(x, params, act)
    lab = torch.where(torch.arange(len(lab)) % 2 == 0, NR.first_argmax(z0), lab)
    c = {"params": params, "x": x, "lab": lab, "n_drop": n_drop, "n_pool": n_pool}
    c["ref"] = autograd(c, act, torch.float64)
    _CASES[key] = c
    return c


def autograd(c, act, dtype):
    """Autograd at the case's parameters in `dtype`: mean CE, {key: gradient}, per-point CE, and in fp64 terms the correct count among the
    non-marginal points and the marginal points (nn_restate.MARGIN)."""
    m = module_of(c["params"], act, dtype)
    z = m(c["x"].to(dtype))
    ce = torch.logsumexp(z, -1) - z.gather(1, c["lab"][:, None])[:, 0]
    loss = ce.mean()
    loss.backward()
    zd = z.detach().double()
    mg = NR.marginal(zd)
    return {"loss": float(loss.detach()), "grad": {"model." + k: p.grad.double() for k, p in m.named_parameters()}, "ce": ce.detach().double(),
            "log1p": zd.gather(1, c["lab"][:, None])[:, 0] == zd.max(-1)[0],
            "c_safe": int(((NR.first_argmax(zd) == c["lab"]) & ~mg).sum()), "n_marginal": int(mg.sum())}


class Restatement:
    """step(x, labels) = optimizer.zero_grad(); loss = CrossEntropyLoss()(net(x), labels); loss.backward(); optimizer.step()."""

    def __init__(self, params, act, lr, dtype=torch.float64):
        self.act, self.dtype = act, dtype
        self.m = module_of(params, act, dtype)
        self.opt = torch.optim.Adam(self.m.parameters(), lr=lr)
        self.losses, self.correct, self.n_marginal = [], [], []

    def step(self, x, labels):
        self.opt.zero_grad()
        z = self.m(x.to(self.dtype))
        loss = F.cross_entropy(z, labels)
        loss.backward()
        self.opt.step()
        zd = z.detach().double()
        mg = NR.marginal(zd)
        self.losses.append(float(loss.detach()))
        self.correct.append(int(((NR.first_argmax(zd) == labels) & ~mg).sum()))
        self.n_marginal.append(int(mg.sum()))

    def params(self):
        return {"model." + k: v.detach().clone() for k, v in self.m.state_dict().items()}


# ------------------------------------------------------------------ the trajectory case
# tanh (no kink), Hc 16, 20 points in batches of 8 (8, 8, 4), 2 epochs, lr 0.01.  TRAJ_SEED is chosen on the CPU so that no batch point of any
# step of the fp64 run has a pooling window within TIE of a tie (tests/test_conv_train_cpu.py asserts it): a run that passes a tie spreads
# 10 - 100 times wider and measures nothing.  (Seeds 1 and 62 meet that condition too and were passed over: there tanh saturates in one conv2
# channel, two pre-activations 2.8e-5 apart pool as VALUES 2.3e-8 apart, fp32 picks the other one and the runs spread 7.7e-5 and 3.8e-4.
# The host test asserts the small spread beside the condition.)
TRAJ = {"dataset": "mnist", "shape": SHAPE, "n_classes": 10, "hidden": 16, "act": "tanh", "arch": "conv", "lr": 0.01, "epochs": 2, "N": 20, "batch": 8}
TRAJ_SEED = 77
TRAJ_ORDERS = 4                # the batch as given and three within-batch permutations of its points


def traj_inputs(seed=None):
    seed = TRAJ_SEED if seed is None else seed
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(TRAJ["N"], *SHAPE, generator=g)
    lab = torch.randint(0, TRAJ["n_classes"], (TRAJ["N"],), generator=g)
    return fresh_params(TRAJ["act"], TRAJ["hidden"], TRAJ["n_classes"], seed), x, lab


def traj_run(dtype, order=0, seed=None, check_ties=False):
    """The trajectory case restated: (Restatement, the parameters BEFORE every step, the number of batch points met within TIE of a pooling
    tie — counted only with check_ties).  order > 0 permutes the points inside every batch (another summation order, the same sums)."""
    params, x, lab = traj_inputs(seed)
    r = Restatement(params, TRAJ["act"], TRAJ["lr"], dtype)
    g = torch.Generator().manual_seed(100 + order)
    before, n_tie = [], 0
    for _ in range(TRAJ["epochs"]):
        for i in range(0, TRAJ["N"], TRAJ["batch"]):
            xb, lb = x[i:i + TRAJ["batch"]], lab[i:i + TRAJ["batch"]]
            if order:
                p = torch.randperm(len(lb), generator=g)
                xb, lb = xb[p], lb[p]
            before.append(r.params())
            if check_ties:
                n_tie += int(discontinuous(xb, before[-1], TRAJ["act"]).sum())
            r.step(xb, lb)
    return r, before, n_tie


_TRAJ = {}


def traj_reference():
    """(fp64 Restatement, parameters before every step, batch points within TIE of a tie, spread): spread = the largest distance of torch's
    fp32 restatement from the fp64 one over every step and the TRAJ_ORDERS summation orders, relative to the largest parameter."""
    if not _TRAJ:
        r64, before, n_tie = traj_run(torch.float64, check_ties=True)
        scale = NR.param_scale(r64.params())
        spreads = []
        for order in range(TRAJ_ORDERS):
            r32, b32, _ = traj_run(torch.float32, order)
            spreads.append(max([NR.max_diff(a, b) for a, b in zip(b32, before)] + [NR.max_diff(r32.params(), r64.params())]) / scale)
        _TRAJ["v"] = (r64, before, n_tie, max(spreads), spreads)
    return _TRAJ["v"]
