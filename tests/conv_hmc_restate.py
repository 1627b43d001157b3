"""CPU restatement of HMC over the weights of a conv net of the 1x28x28 geometry (what robustbnns_amd.conv_hmc.ConvHmcSampler computes;
model_bnn.py:260-301 on the conv stack of model_nn.py:93-106) in any float dtype: hmc_restate.Restatement — the chain algorithm, its
constants, the acceptance uniform — with the conv potential and the conv momentum put under it:

  potential   U(q) = sum_b CE(z_b(q), y_b) + 1/2 sum q^2 with the summed CE and dCE/dW of conv_svi_restate.ce_grads (autograd on
              conv_restate.sequential); the gradient is returned WITHOUT the prior's q, as the device caches dCE/dW;
  momentum    conv_svi_restate.draw_eps (each tensor ONE row of n_elem columns: counter (e / 4, tensor id, 0, draw id)) over sqrt(m_inv).

Pooling ties.  Both max-pools make grad U jump where two entries of a window tie (and relu / leaky where a conv pre-activation crosses 0);
conv_svi_restate meets a point within conv_restate.TIE of one at about one point-evaluation in five.  A trajectory compared with fp64
therefore runs on a CHOSEN batch (`choose_batch`): from a pool of 6 B + 16 torch.rand images the points conv_restate.discontinuous flags at
q0 are dropped, the fp64 trajectory runs on the first B survivors, the points flagged at any of its L + 1 positions are dropped and the batch
refilled, until no point is flagged.  The conditions (tests/test_conv_hmc_cpu.py asserts them): the loop ends within MAX_ROUNDS rounds, at most
two thirds of the pool is dropped, B clean points remain.  Every other run (fp32 on the CPU, the GPU) gets the batch the fp64 run chose.

Bounds.  hmc_restate.BOUND's rule: FACTOR = 4 x the deviation of THIS restatement run in torch fp32 on the CPU from itself in fp64, on the
tests' own cases below (`PYTHONPATH=.:tests python tests/conv_hmc_restate.py` prints the figures; the factor covers another summation order
on the MFMA).  leapfrog_q / leapfrog_r: max |difference| over max |fp64 value| of the vector; U, K: relative; dH: absolute in units of
hmc_restate.energy_scale (|U'| + K' + K).  tests/test_conv_hmc_cpu.py reproduces them.
"""
import numpy as np
import torch

import conv_restate as CR
import conv_svi_restate as V
import hmc_restate as HR

KEYS = CR.KEYS
FACTOR = HR.FACTOR
MAX_ROUNDS = 16
# worst fp32-CPU-vs-fp64 deviation over LEAP_CASES (leapfrog_q, leapfrog_r) and TRANSITION_CASES (U, K, dH).  The leapfrog figures do not move
# with torch's thread count; U, K and dH are fp32 sums over 21 514 elements whose order follows it (1, 2, 4, 16 and 32 threads gave U 4.88e-08
# ... 5.13e-08, K 5.07e-08 ... 8.10e-08, dH 1.35e-08 ... 3.14e-08): the worst of those runs is recorded.
MEASURED_FP32 = {"leapfrog_q": 9.43e-08, "leapfrog_r": 1.69e-07, "U": 5.14e-08, "K": 8.10e-08, "dH": 3.14e-08}
BOUND = {k: FACTOR * v for k, v in MEASURED_FP32.items()}


class Restatement(HR.Restatement):
    """ConvHmcSampler on the CPU in `dtype`: same initial position, same (key, draw id) momenta and uniforms.  x: [B, 1, 28, 28] or [B, 784]."""

    def __init__(self, act, q0, x, y, step_size, num_steps, key, dtype=torch.float64, adapt_step_size=True, adapt_mass_matrix=True):
        import math
        self.arch, self.act, self.dtype, self.key = "conv", act, dtype, int(key) & 0xFFFFFFFFFFFFFFFF
        self.keys = list(KEYS)
        self.shapes = {k: tuple(q0[k].shape) for k in self.keys}
        self.x, self.y = x.reshape(x.shape[0], *CR.SHAPE).to(dtype), y.long()
        self.q = self.flat(q0)
        self.m_inv = torch.ones_like(self.q)
        self.eps, self.traj = float(step_size), float(step_size) * num_steps
        self.adapt_step_size, self.adapt_mass_matrix = adapt_step_size, adapt_mass_matrix
        self.da = {"t": 0.0, "gbar": 0.0, "xbar": 0.0, "mu": math.log(10 * self.eps)}
        self.w_mean, self.w_m2 = torch.zeros_like(self.q), torch.zeros_like(self.q)
        self.U, self.g = self.potential(self.q)
        self.searches = 0
        self.log, self.search_log, self.adapt_log, self.search_scales = [], [], [], []

    def potential(self, q):
        """(U, dCE/dW) at q: U a Python float, the gradient WITHOUT the prior's q."""
        ce, g = V.ce_grads(self.x, self.y, self.unflat(q), self.act)
        return float(ce.sum()) + float(0.5 * (q * q).sum()), self.flat(g)

    def momentum(self, key, draw_id):
        e = V.draw_eps(self.shapes, int(key) & 0xFFFFFFFFFFFFFFFF, draw_id)
        return self.flat({k: v[0] for k, v in e.items()}) / torch.sqrt(self.m_inv)


def potential_at(q_flat, shapes, x, y, act):
    """fp64 U at a flat position (any float dtype), on the batch (x, y)."""
    rs = Restatement.__new__(Restatement)
    rs.keys, rs.shapes, rs.act, rs.dtype = list(KEYS), shapes, act, torch.float64
    rs.x, rs.y = x.reshape(x.shape[0], *CR.SHAPE).double(), y.long()
    return rs.potential(q_flat.detach().cpu().double())[0]


def predict(stack, x, act):
    """Mean softmax over the stack's samples in fp64 (hmc_restate.predict for the conv stack).  stack: dict key -> [S, ...]."""
    S = int(next(iter(stack.values())).shape[0])
    with torch.no_grad():
        return sum(torch.softmax(V.logits_at({k: stack[k][s].detach().cpu().double() for k in KEYS}, x.detach().cpu(), act, torch.float64), -1)
                   for s in range(S)) / S


# ---------------------------------------------------------------------------------------------------------------------------------------
# The cases of tests/test_hip_conv_hmc.py (shared with the derivation of its bounds)
# ---------------------------------------------------------------------------------------------------------------------------------------
# (Hc, activation, B, C, L, step size): a one-tile and a three-tile Hc; B = 1, an odd B, a B past a 64-point boundary; C = 3 (the bias tensor a
# partial quad at the end of the buffer); the four activations; two step sizes
LEAP_CASES = [(16, "tanh", 8, 10, 3, 1e-3), (16, "leaky", 5, 3, 2, 1e-3), (48, "sigm", 65, 10, 2, 1e-3), (16, "relu", 1, 10, 2, 1e-3),
              (16, "tanh", 8, 10, 3, 1e-2)]
LEAP_KEY, Q0_SEED, POOL_SEED = 0xABCDEF, 77, 5
# what choose_batch met on LEAP_CASES, in their order: (rounds, points dropped, pool size), measured on the CPU and asserted there
SELECTION = [(2, 16, 64), (7, 27, 46), (9, 211, 406), (0, 6, 22), (4, 24, 64)]
# (name, Hc, activation, B, C, L, step size, key): one accepted transition and one rejected one (a step size past the stability limit)
TRANSITION_CASES = [("accept", 16, "tanh", 8, 10, 3, 1e-3, 21), ("reject", 16, "tanh", 8, 10, 3, 5e-2, 21)]
# the short full run: Hc, activation, B, C, step size, num_steps, warmup (all three window kinds), samples
RUN = {"Hc": 16, "act": "tanh", "B": 8, "C": 10, "eps": 1e-3, "steps": 4, "warmup": 24, "samples": 6, "key": 77}
_CHOSEN = {}


def start_position(Hc, Cn):
    return V.guide(Hc, Cn, Q0_SEED)[0]


def choose_batch(Hc, act, B, Cn, L, eps, key=LEAP_KEY, draw_id=0):
    """The tie-free batch of one trajectory (computed once, shared, never modified): {"q0", "x", "lab", "rounds", "dropped", "pool", "r0",
    "end": the fp64 trajectory's (q, r, dCE/dW, U)}.  The trajectory starts at start_position with the momentum of (key, draw_id), unit m_inv."""
    case = (Hc, act, B, Cn, L, eps, key, draw_id)
    if case in _CHOSEN:
        return _CHOSEN[case]
    g = torch.Generator().manual_seed(POOL_SEED)
    n_pool = 6 * B + 16
    x = torch.rand(n_pool, *CR.SHAPE, generator=g)
    lab = torch.randint(0, Cn, (n_pool,), generator=g)
    q0 = start_position(Hc, Cn)
    q64 = {k: v.double() for k, v in q0.items()}
    alive = ~CR.discontinuous(x, q64, act)
    rounds, out = 0, None
    while int(alive.sum()) >= B and rounds <= MAX_ROUNDS:
        idx = torch.nonzero(alive)[:B, 0]
        rs = Restatement(act, q0, x[idx], lab[idx], eps, L, key)
        r0 = rs.momentum(key, draw_id)
        q, r, gq, bad = rs.q, r0, rs.g, torch.zeros(B, dtype=torch.bool)
        for _ in range(L):
            q, r, gq, U = rs.leapfrog(q, r, gq, 1)
            bad |= CR.discontinuous(x[idx], rs.unflat(q), act)
        if not bool(bad.any()):
            out = {"q0": q0, "x": x[idx], "lab": lab[idx], "r0": r0, "end": (q, r, gq, U)}
            break
        alive[idx[bad]] = False
        rounds += 1
    res = {"rounds": rounds, "dropped": int((~alive).sum()), "pool": n_pool, "clean": out is not None}
    res.update(out or {})
    _CHOSEN[case] = res
    return res


def leap_deviation(case):
    """(leapfrog_q, leapfrog_r) of the fp32 CPU trajectory from the fp64 one on the chosen batch."""
    Hc, act, B, Cn, L, eps = case
    c = choose_batch(*case)
    rs = Restatement(act, c["q0"], c["x"], c["lab"], eps, L, LEAP_KEY, dtype=torch.float32)
    q32, r32, _, _ = rs.leapfrog(rs.q, rs.momentum(LEAP_KEY, 0), rs.g, L)
    return HR.relmax(q32, c["end"][0]), HR.relmax(r32, c["end"][1])


def transition_case(name, Hc, act, B, Cn, L, eps, key):
    """The chosen batch of a TRANSITION_CASES case (transition 0: the momentum of (key, 0)) and the fp64 restatement's record of it."""
    c = choose_batch(Hc, act, B, Cn, L, eps, key, 0)
    assert c["clean"]
    rs = Restatement(act, c["q0"], c["x"], c["lab"], eps, L, key, adapt_step_size=False)
    U0 = rs.U
    return c, U0, rs.transition(0)


def transition_deviation(case):
    """(U, K, dH) deviations of the fp32 CPU transition from the fp64 one, as hmc_restate._transition_dev forms them."""
    c, _, b = transition_case(*case)
    name, Hc, act, B, Cn, L, eps, key = case
    a = Restatement(act, c["q0"], c["x"], c["lab"], eps, L, key, dtype=torch.float32, adapt_step_size=False).transition(0)
    assert b["accepted"] == (name == "accept") and a["accepted"] == b["accepted"], (name, a["dH"], b["dH"])
    dU = abs(a["U_new"] - b["U_new"]) / abs(b["U_new"])
    dK = max(abs(a["K_new"] - b["K_new"]) / b["K_new"], abs(a["K_old"] - b["K_old"]) / b["K_old"])
    return dU, dK, abs(a["dH"] - b["dH"]) / HR.energy_scale(b)


def measure():
    """MEASURED_FP32, measured again."""
    w = {k: 0.0 for k in MEASURED_FP32}
    for case in LEAP_CASES:
        dq, dr = leap_deviation(case)
        c = choose_batch(*case)
        print(f"  leapfrog {case}: rounds {c['rounds']} dropped {c['dropped']} / {c['pool']}  q {dq:.2e}  r {dr:.2e}", flush=True)
        w["leapfrog_q"], w["leapfrog_r"] = max(w["leapfrog_q"], dq), max(w["leapfrog_r"], dr)
    for case in TRANSITION_CASES:
        dU, dK, dH = transition_deviation(case)
        c, _, rec = transition_case(*case)
        print(f"  transition {case}: rounds {c['rounds']} dropped {c['dropped']} / {c['pool']}  accepted {rec['accepted']} dH {rec['dH']:.3e} "
              f"u {rec['u']:.3f}  U {dU:.2e} K {dK:.2e} dH/scale {dH:.2e} (scale {HR.energy_scale(rec):.0f})", flush=True)
        w["U"], w["K"], w["dH"] = max(w["U"], dU), max(w["K"], dK), max(w["dH"], dH)
    return w


def run_inputs():
    """(q0, x, lab) of the short full run: the small-scale start position and the first B images of the pool (ties not excluded)."""
    g = torch.Generator().manual_seed(POOL_SEED + 1)
    x = torch.rand(RUN["B"], *CR.SHAPE, generator=g)
    return start_position(RUN["Hc"], RUN["C"]), x, torch.randint(0, RUN["C"], (RUN["B"],), generator=g)


# BNN.train_hmc_conv end to end: Hc 16, 10 classes, n_samples 3, warmup 4, 16 random points in batches of 8.  The chain starts at pyro's
# Uniform(-2, 2) (BNN._hmc_prologue), where U is about 1.5e4; with this step_size / num_steps the fp64 restatement's search ends after four
# tries and its trajectories have 1 to 3 steps, so the test stays short.
#
# The data seed.  A chain four warmup transitions away from Uniform(-2, 2) has logits near 90, where ANY fp32 forward is about 1e-5 off
# fp64 in a probability: torch's own fp32 forward on the CPU, at the fp64 replay's stack (e2e_replay), is 0.46e-5 ... 1.36e-5 off over the
# data seeds 0 ... 29, so at most seeds the 1e-5 forward bar measures the number format and not the kernels.  The seed is the FIRST one
# (from 0) at which torch's fp32 forward stays within HALF the bar — a rule on the reference's own error, decided on the CPU without the
# code under test; tests/test_conv_hmc_cpu.py asserts it.  Seeds 0 ... 3: 1.06e-05, 4.58e-06, 1.25e-05, 1.13e-05.
E2E = {"Hc": 16, "act": "tanh", "C": 10, "n_samples": 3, "warmup": 4, "n": 16, "batch": 8, "step_size": 5e-3, "num_steps": 4, "seed": 1}


def e2e_data(seed=None):
    g = torch.Generator().manual_seed(E2E["seed"] if seed is None else seed)
    x = torch.rand(E2E["n"], *CR.SHAPE, generator=g)
    lab = torch.randint(0, E2E["C"], (E2E["n"],), generator=g)
    return x, torch.nn.functional.one_hot(lab, E2E["C"]).float()


def e2e_replay(seed=None):
    """BNN.train_hmc_conv on the CPU in fp64 (hmc_restate.replay_train_hmc's sequence of draws from the CPU generator: the loader's iterator,
    the initial position, the key, the resampling indices; the chain on the LAST batch) -> (restatement, resampled stack as a dict key ->
    [n_samples, ...], the data x)."""
    import random
    from torch.utils.data import DataLoader
    x, y = e2e_data(seed)
    random.seed(0)
    torch.manual_seed(0)
    np.random.seed(0)
    for xb, yb in DataLoader(list(zip(x, y)), batch_size=E2E["batch"], shuffle=False):
        pass
    q0 = HR.initial_position(V.shapes_of(E2E["Hc"], E2E["C"]))
    key = int(torch.randint(-(2 ** 63), 2 ** 63 - 1, (1,), dtype=torch.int64).item()) & 0xFFFFFFFFFFFFFFFF
    batch_samples = int(E2E["n_samples"] / max(1, int(len(x) / E2E["batch"]))) + 1
    rs = Restatement(E2E["act"], q0, xb, yb.argmax(-1), E2E["step_size"], E2E["num_steps"], key)
    S = rs.run(batch_samples, E2E["warmup"])[torch.randint(0, batch_samples, (E2E["n_samples"],))]
    return rs, {k: torch.stack([rs.unflat(row)[k] for row in S]) for k in KEYS}, x


def torch_fp32_forward_deviation(stack, x, act):
    """max |p_fp32 - p_fp64| of torch's own forward on the CPU (mean softmax over the stack's samples) at the fp64 stack rounded to fp32."""
    S = int(next(iter(stack.values())).shape[0])
    with torch.no_grad():
        p32 = sum(torch.softmax(V.logits_at({k: stack[k][s].float() for k in KEYS}, x, act, torch.float32), -1) for s in range(S)) / S
    return float((p32.double() - predict(stack, x, act)).abs().max())


if __name__ == "__main__":
    torch.set_num_threads(8)
    print({k: float(f"{v:.2e}") for k, v in measure().items()})
    print("SELECTION =", [(choose_batch(*c)["rounds"], choose_batch(*c)["dropped"], choose_batch(*c)["pool"]) for c in LEAP_CASES])
