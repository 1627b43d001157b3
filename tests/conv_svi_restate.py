"""CPU restatement of SVI training of one conv guide (what robustbnns_amd.conv_svi_train.ConvSviTrainer computes; model_bnn.py:105-136,
:303-365 on the conv stack of model_nn.py:93-106) in any float dtype: W = loc + softplus(raw) eps with the oracle's restatement of the draw's
generator at sample 0 (each tensor ONE row of n_elem columns: counter (e / 4, tensor id, 0, draw id)), the summed cross-entropy of
conv_restate.sequential at W by autograd, the analytic KL and g_loc / g_raw of svi_restate.step_gradients, svi_restate.adam_update, and the
10-sample accuracy forward under key ^ ACC_KEY.  Also the inputs of both test tiers: the gradient cases (their points taken from a pool by
conv_restate.discontinuous at the drawn fp64 W) and the trajectory case."""
import numpy as np
import torch
import torch.nn.functional as F
from torch.func import functional_call

import conv_restate as CR
import svi_restate as SR
from oracle import bnn_oracle as O

KEYS = CR.KEYS
TENSOR_IDS = {k: i for i, k in enumerate(KEYS)}                      # robustbnns_amd.conv.ConvSviGuide.TENSOR_IDS
ACC_SAMPLES, ACC_KEY = SR.ACC_SAMPLES, SR.ACC_KEY
MASK = 0xFFFFFFFFFFFFFFFF


def shapes_of(Hc, Cn):
    return {"model.0.weight": (32, 1, 5, 5), "model.0.bias": (32,), "model.3.weight": (Hc, 32, 5, 5), "model.3.bias": (Hc,),
            "model.7.weight": (Cn, 49 * Hc), "model.7.bias": (Cn,)}


def guide(Hc, Cn, seed, std=0.05):
    """(loc, raw) of a small-scale guide (the _guide(..., std=0.05) convention of the fc tests: the conv forward is not saturated)."""
    g = torch.Generator().manual_seed(seed)
    shapes = shapes_of(Hc, Cn)
    loc = {k: std * torch.randn(*s, generator=g) for k, s in shapes.items()}
    raw = {k: -3.0 + 0.5 * torch.randn(*s, generator=g) for k, s in shapes.items()}
    return loc, raw


def draw_eps(shapes, key, draw_id, n_samples=1, sample_keys=None):
    """state_dict key -> float64 eps [n_samples, *shape] of rbnn_svi_draw_flat for (key, draw_id) — or per-sample keys, sample 0 in the counter."""
    out = {}
    for k, shp in shapes.items():
        n = int(np.prod(shp))
        e = np.stack([O.philox_normals(sample_keys[s] if sample_keys is not None else key, draw_id, TENSOR_IDS[k], s, 1, n,
                                       sample_is_key=sample_keys is not None)[0] for s in range(n_samples)])
        out[k] = torch.from_numpy(e).reshape((n_samples,) + tuple(shp))
    return out


def logits_at(W, x, act, dtype):
    """Logits of x [B, 1, 28, 28] at the weights W (key -> tensor, autograd flows into them) on conv_restate.sequential."""
    Hc, Cn = int(W["model.3.bias"].shape[0]), int(W["model.7.bias"].shape[0])
    m = CR.sequential(act, Hc, Cn, dtype)
    return functional_call(m, {k[len("model."):]: v for k, v in W.items()}, (x.reshape(-1, *CR.SHAPE).to(dtype),))


def ce_points(z, y):
    return torch.logsumexp(z, -1) - z.gather(1, y[:, None])[:, 0]


def ce_grads(x, y, W, act):
    """(per-point CE, {key: d sum_b CE / dW}) at ONE weight sample W by autograd, in W's dtype."""
    Wg = {k: v.detach().clone().requires_grad_(True) for k, v in W.items()}
    ce = ce_points(logits_at(Wg, x, act, next(iter(W.values())).dtype), y.long())
    grads = torch.autograd.grad(ce.sum(), [Wg[k] for k in KEYS])
    return ce.detach(), dict(zip(KEYS, grads))


def step_gradients(loc, raw, eps, x, y, act):
    """(loss, g_loc, g_raw, dCE/dW, W) of the ELBO at the draw w = loc + softplus(raw) eps: svi_restate.step_gradients' formulas."""
    sig = {k: F.softplus(raw[k]) for k in loc}
    W = {k: loc[k] + sig[k] * eps[k] for k in loc}
    ce, dW = ce_grads(x, y, W, act)
    g_loc = {k: dW[k] + loc[k] for k in loc}
    g_raw = {k: (dW[k] * eps[k] + sig[k] - 1 / sig[k]) * torch.sigmoid(raw[k]) for k in loc}
    return ce.sum() + SR.kl(loc, raw), g_loc, g_raw, dW, W


def elbo_autograd(loc, raw, eps, x, y, act):
    """(loss, d loss / d loc, d loss / d raw) by full torch autograd of the ELBO through the reparameterised draw."""
    L = {k: v.detach().clone().requires_grad_(True) for k, v in loc.items()}
    R = {k: v.detach().clone().requires_grad_(True) for k, v in raw.items()}
    W = {k: L[k] + F.softplus(R[k]) * eps[k] for k in L}
    loss = ce_points(logits_at(W, x, act, L[KEYS[0]].dtype), y.long()).sum() + SR.kl(L, R)
    loss.backward()
    return float(loss.detach()), {k: L[k].grad for k in L}, {k: R[k].grad for k in R}


class Restatement:
    """ConvSviTrainer.step on the CPU: same init, same (key, draw id = step) eps, in `dtype`."""

    def __init__(self, loc, raw, act, lr, key, dtype=torch.float64):
        self.act, self.lr, self.key, self.dtype = act, lr, int(key) & MASK, dtype
        self.loc = {k: loc[k].detach().cpu().to(dtype).clone() for k in KEYS}
        self.raw = {k: raw[k].detach().cpu().to(dtype).clone() for k in KEYS}
        z = lambda: {k: torch.zeros_like(v) for k, v in self.loc.items()}
        self.m_loc, self.v_loc, self.m_raw, self.v_raw = z(), z(), z(), z()
        self.t, self.losses = 0, []

    def eps(self, t):
        return {k: v[0].to(self.dtype) for k, v in draw_eps({k: tuple(v.shape) for k, v in self.loc.items()}, self.key, t).items()}

    def drawn(self, t):
        """The weights of step t's draw at the current parameters."""
        e = self.eps(t)
        return {k: self.loc[k] + F.softplus(self.raw[k]) * e[k] for k in KEYS}

    def step(self, x, y):
        loss, gl, gr, _, _ = step_gradients(self.loc, self.raw, self.eps(self.t), x, y, self.act)
        self.t += 1
        for k in KEYS:
            SR.adam_update(self.loc[k], gl[k], self.m_loc[k], self.v_loc[k], self.t, self.lr)
            SR.adam_update(self.raw[k], gr[k], self.m_raw[k], self.v_raw[k], self.t, self.lr)
        self.losses.append(float(loss))
        return float(loss)


def accuracy_forward(loc, raw, act, x, key, t, n_samples=ACC_SAMPLES):
    """The per-step training accuracy of ConvSviTrainer.step(accuracy=True) in fp64 at the guide (loc, raw) AFTER the update of step t:
    n_samples weight sets with eps of the draw (key ^ ACC_KEY, draw id t, sample s), Psum = sum over the samples of softmax(logits).
    -> (Psum [B, C], first-maximum prediction [B], gap between the two largest MEAN probabilities [B])."""
    shapes = {k: tuple(loc[k].shape) for k in KEYS}
    eps = draw_eps(shapes, (int(key) ^ ACC_KEY) & MASK, t, n_samples)
    psum = 0.0
    with torch.no_grad():
        for s in range(n_samples):
            W = {k: loc[k].detach().cpu().double() + F.softplus(raw[k].detach().cpu().double()) * eps[k][s] for k in KEYS}
            psum = psum + torch.softmax(logits_at(W, x.detach().cpu(), act, torch.float64), -1)
    return psum, SR.first_argmax(psum), SR.top2_gap(psum / n_samples)


# ------------------------------------------------------------------ the gradient cases
# (Hc, act, B, C): a one-tile and a three-tile Hc, B = 1, an odd B and a B past a 64-point boundary, 3 and 10 classes, the four activations;
# and conv_restate.REGIME_CASES[0], whose slice plan (conv_restate.slice_plan) has several units per slice, ragged last slices and a fold in
# each of the three GEMMs of the weight gradients, through the SVI entry points
GRAD_CASES = [(16, "leaky", 5, 10), (16, "relu", 65, 3), (48, "tanh", 1, 10), (48, "sigm", 65, 3), (48, "leaky", 5, 10), CR.REGIME_CASES[0]]
GRAD_KEY, GRAD_DRAW = 0x0123456789ABCDEF, 5
_CASES = {}


def pool_points(W64, act, B, Cn, seed):
    """The first B of a pool of 3 B + 8 torch.rand images that are not conv_restate.discontinuous at the drawn fp64 weights W64, with labels
    (every other point: the fp64 prediction at W64).  -> (x, lab, n_drop, n_pool)"""
    g = torch.Generator().manual_seed(seed)
    n_pool = 3 * B + 8
    x = torch.rand(n_pool, *CR.SHAPE, generator=g)
    lab = torch.randint(0, Cn, (n_pool,), generator=g)
    bad = CR.discontinuous(x, W64, act)
    x, lab = x[~bad][:B], lab[~bad][:B]
    with torch.no_grad():
        z0 = logits_at(W64, x, act, torch.float64)
    lab = torch.where(torch.arange(len(lab)) % 2 == 0, SR.first_argmax(z0), lab)
    return x, lab, int(bad.sum()), n_pool


def grad_case(Hc, act, B, Cn):
    """One GRAD_CASES case (computed once, shared, never modified): the guide, the drawn fp64 weights of (GRAD_KEY, GRAD_DRAW), the points."""
    key = (Hc, act, B, Cn)
    if key not in _CASES:
        seed = 1000 * Hc + 10 * B + Cn
        loc, raw = guide(Hc, Cn, seed)
        eps = {k: v[0] for k, v in draw_eps(shapes_of(Hc, Cn), GRAD_KEY, GRAD_DRAW).items()}
        W64 = {k: loc[k].double() + F.softplus(raw[k].double()) * eps[k] for k in KEYS}
        x, lab, n_drop, n_pool = pool_points(W64, act, B, Cn, seed + 1)
        _CASES[key] = {"loc": loc, "raw": raw, "eps": eps, "W64": W64, "x": x, "lab": lab, "n_drop": n_drop, "n_pool": n_pool}
    return _CASES[key]


# ------------------------------------------------------------------ the trajectory case
# tanh (no kink), Hc 16, 20 steps of B = 8, lr 0.01.  A pooling tie within conv_restate.TIE is met by about one point-evaluation in five at
# these scales, so no seed gives 160 of them without one: as everywhere here, the batch of step i is taken from a pool of its own (3 B + 8
# images) by conv_restate.discontinuous at the fp64 run's drawn weights of that step, and every other run (fp32 on the CPU, the GPU) is given
# the batches the fp64 run chose.  TRAJ_SEED is one for which every step's pool keeps the cap (at most a third dropped), asserted on the CPU.
TRAJ = {"hidden": 16, "act": "tanh", "n_classes": 10, "lr": 0.01, "steps": 20, "batch": 8, "key": 0x5EED0C0FFEE}
TRAJ_SEED = 0
# max |theta_fp32 - theta_fp64| of loc and of raw over the 20 steps of this restatement itself (same init, same eps, same batches), measured on
# the CPU by tests/test_conv_svi_train_cpu.py::test_trajectory_case_meets_no_discontinuity_and_its_spread_is_the_recorded_one
TRAJ_SPREAD = {"loc": 1.24e-5, "raw": 8.32e-6}
_TRAJ = {}


def traj_reference(seed=None):
    """The fp64 run, which also chooses the batches: {"r64": Restatement after the 20 steps, "loc", "raw": the initial guide, "batches":
    [(x, lab)], "drops": [(dropped, pool size)] per step, "n_bad": batch points within the discontinuity margins (0 by construction, counted
    again on the chosen batches), "after": [(loc, raw) after every step]}."""
    seed = TRAJ_SEED if seed is None else seed
    if seed not in _TRAJ:
        loc, raw = guide(TRAJ["hidden"], TRAJ["n_classes"], seed + 500)
        r = Restatement(loc, raw, TRAJ["act"], TRAJ["lr"], TRAJ["key"], torch.float64)
        out = {"r64": r, "loc": loc, "raw": raw, "batches": [], "drops": [], "after": [], "n_bad": 0}
        for i in range(TRAJ["steps"]):
            W = r.drawn(i)
            xb, lb, n_drop, n_pool = pool_points(W, TRAJ["act"], TRAJ["batch"], TRAJ["n_classes"], 7919 * seed + i)
            out["n_bad"] += int(CR.discontinuous(xb, W, TRAJ["act"]).sum())
            r.step(xb, lb)
            out["batches"].append((xb, lb))
            out["drops"].append((n_drop, n_pool))
            out["after"].append(({k: v.clone() for k, v in r.loc.items()}, {k: v.clone() for k, v in r.raw.items()}))
        _TRAJ[seed] = out
    return _TRAJ[seed]


def traj_spread(seed=None):
    """{"loc", "raw"}: max |fp32 - fp64| of the restatement over every step, the fp32 run on the fp64 run's batches."""
    ref = traj_reference(seed)
    r = Restatement(ref["loc"], ref["raw"], TRAJ["act"], TRAJ["lr"], TRAJ["key"], torch.float32)
    worst = {"loc": 0.0, "raw": 0.0}
    for (xb, lb), (l64, r64) in zip(ref["batches"], ref["after"]):
        r.step(xb, lb)
        worst["loc"] = max(worst["loc"], max(float((r.loc[k].double() - l64[k]).abs().max()) for k in KEYS))
        worst["raw"] = max(worst["raw"], max(float((r.raw[k].double() - r64[k]).abs().max()) for k in KEYS))
    return worst
