"""CPU restatement of HMC over the weights of an fc / fc2 net (what robustbnns_amd.hmc.HmcSampler computes; model_bnn.py:260-301), in any
float dtype: the algorithm of pyro 1.3.0's HMC(model, step_size, num_steps) under MCMC(num_samples, warmup_steps, num_chains=1) with its
defaults.  pyro-ppl is not installed, so every constant of pyro's below is [recalled], not checked; seed-for-seed parity with pyro's RNG
stream is unpinned.  The fp64 run of this file is the definition the kernels are held to.

Position q: the flat parameter vector in SviTrainer's layout (state_dict order, unpadded, row-major).
U(q) = sum_b CE(z_b(q), y_b) + 1/2 sum q^2 (N(0, 1) priors + the summed Categorical likelihood of BNN.model, constants dropped),
grad U = dCE/dW + q (svi_restate.ce_grads).  Diagonal inverse mass m_inv (ones at first), r = eps_n / sqrt(m_inv), K = 1/2 sum m_inv r^2.

One transition: fresh momentum; L velocity-Verlet steps (r -= eps/2 grad U; q += eps m_inv r; grad U again; r -= eps/2 grad U);
dH = (U' + K') - (U + K), NaN -> +inf; accept_prob = min(1, exp(-dH)); accept iff u < accept_prob; a rejection keeps position, cached
gradient and cached U.  L = max(1, int(trajectory_length / eps)), trajectory_length = step_size * num_steps of the constructor.

Warmup [recalled]: dual averaging on log eps (target 0.8, t0 = 10, kappa = 0.75, gamma = 0.05, prox centre mu = log(10 eps)); windows
(`windows`): < 20 one window, else start buffer 75, end buffer 50, first middle window 25 (all three scaled to 15 % / 10 % / the rest if
they do not fit), middle windows doubling, the last one absorbing the remainder; Welford mean / M2 of the post-decision position in middle
windows, m_inv = (n / (n + 5)) M2 / (n - 1) + 1e-3 * 5 / (n + 5) at their end; once before the first transition and at every window end
BUT THE LAST the reasonable-step-size search (one leapfrog step from fresh momentum; direction = +1 if -dH > log 0.8 else -1; eps *= 2^direction
with new momentum each try until the direction flips), then dual averaging restarts with mu = log(10 eps).  The last window ends on the
dual-averaged exp(xbar), which is the sampling phase's step size: a search there would replace what warmup adapted by a power-of-two probe
result (on the one-class net of tests/hmc_exact_cases.py it left chains sampling at step sizes past the leapfrog stability limit).

Randomness (the kernel header of csrc/rbnn_hmc.hip states the same):
  momentum of transition i    O.svi_draw_philox's eps on zero loc / zero raw scale for (key, draw id i, sample 0);
  step-size-search momenta    the same generator under key ^ SEARCH_KEY, draw id = the number of search tries so far;
  acceptance uniform u_i      component 0 of O.philox4x32_10 with counter (i, 0, 0, 0) under key ^ UNIF_KEY, times 2^-32.
"""
import math

import numpy as np
import torch

import svi_restate as R
from oracle import bnn_oracle as O

UNIF_KEY, SEARCH_KEY = 0xE7037ED1A0B428DB, 0xA0761D6478BD642F       # robustbnns_amd._hip.HMC_UNIF_KEY / HMC_SEARCH_KEY
TARGET, T0, KAPPA, GAMMA = 0.8, 10.0, 0.75, 0.05                    # pyro.ops.dual_averaging.DualAveraging defaults + HMC's target [recalled]
START_BUFFER, END_BUFFER, INIT_WINDOW = 75, 50, 25                  # pyro.infer.mcmc.adaptation.WarmupAdapter [recalled]
INIT_RADIUS = 2.0                                                   # pyro's init_to_uniform [recalled]
MAX_SEARCH = 64                                                     # tries of one step-size search before it is a failure (never met)

# ---------------------------------------------------------------------------------------------------------------------------------------
# Bounds of tests/test_hip_hmc.py.  Each is 4 x the deviation of THIS restatement run in torch fp32 on the CPU from itself in fp64, on the
# test's own cases below (`PYTHONPATH=. python tests/hmc_restate.py` prints the measured figures; the factor 4 covers another summation order
# over up to 5000 batch terms on the MFMA).  leapfrog_q / leapfrog_r / m_inv / samples: max |difference| over max |fp64 value| of the vector;
# U, K, eps: relative; dH: absolute, in units of the sums it is a difference of (energy_scale = |U'| + K' + K), from the single-transition
# cases — along a chain the positions drift apart and dH with them, which the eps / m_inv / samples figures of the full runs carry.
# `PYTHONPATH=. python tests/hmc_restate.py keys` looks for the keys of RUN_CASES: the first key whose fp64 margins hold AND whose fp32 run takes
# the same decisions (the figures below are that run's deviations).  The fc2-32 run needed 1716 candidates: about one key in a thousand has
# 44 decisions that all clear 100 x the dH bound (energy scale ~2000: a margin of 0.04 to 0.1 on every |u - accept_prob|), and of the first
# three of those two had an fp32 run that decides otherwise (117) or drifts 1.7e-02 in eps (498); the run was not shortened.
# ---------------------------------------------------------------------------------------------------------------------------------------
# leapfrog_q was measured before the relu / leaky cases lost their near-kink points (leap_case); on the batches as they now are it is 3.64e-07
# (leapfrog_r unchanged).  The smaller, earlier figure is kept: the bound did not get wider with the selection.
MEASURED_FP32 = {                 # worst fp32-CPU-vs-fp64 deviation over the cases below
    "leapfrog_q": 2.68e-07, "leapfrog_r": 3.8e-07, "U": 5.81e-08, "K": 7.74e-08, "dH": 4.98e-08, "eps": 1.61e-04, "m_inv": 1.16e-04, "samples": 8.61e-05,
    # tests/test_hip_hmc_exact.py: the fp32 round trip of REVERSE_CASE from its start; Welford's recurrence in fp32 over hmc_exact_cases.welford_rows
    "reverse_q": 1.79e-07, "welford_mean": 4.03e-07, "welford_m_inv": 3.79e-03,
}
# The statistical conditions of tests/test_hip_hmc_exact.py and this file's own fp64 figures on the tests' exact inputs (CPU):
#   stationarity (16 chains x 200 samples, hand-set m_inv, eps 0.25, L 6): |mean q^2 - 1| <= 0.03, |mean q| <= 0.03; here 0.9972 and -0.0047
#     (with the momentum mutated to eps_n sqrt(m_inv): mean q^2 2.4674);
#   adaptation (hmc_exact_cases.ADAPT, 16 chains): every chain's mean accept_prob over the sampling phase in [0.7, 0.98], |mean q^2 - 1| <= 0.05;
#     here 0.8668 ... 0.9270 (mean 0.899), step sizes 0.398 ... 0.560, mean q^2 0.9834; its first 4 chains (the CPU tier): 0.8894 ... 0.9270,
#     mean q^2 0.9624.  With the search also run after the last window: 9.6e-09 ... 0.968 (mean 0.356), step sizes 0.28 ... 1.88.
FACTOR = 4.0
BOUND = {k: FACTOR * v for k, v in MEASURED_FP32.items()}


def windows(warmup):
    """[(start, end, kind)] with end exclusive and kind in {"start", "middle", "end"}: the adaptation windows tiling [0, warmup)."""
    if warmup <= 0:
        return []
    if warmup < 20:
        return [(0, warmup, "start")]
    start, end, init = START_BUFFER, END_BUFFER, INIT_WINDOW
    if start + end + init > warmup:
        start, end = int(0.15 * warmup), int(0.1 * warmup)
        init = warmup - start - end
    out = [(0, start, "start")] if start > 0 else []
    end_start = warmup - end
    cur, size = start, init
    while cur < end_start:
        if 3 * size <= end_start - cur:
            nxt = 2 * size
        else:
            size = end_start - cur                       # the last middle window absorbs the remainder
            nxt = size
        out.append((cur, cur + size, "middle"))
        cur, size = cur + size, nxt
    if end > 0:
        out.append((end_start, warmup, "end"))
    return out


def dual_averaging_update(state, accept_prob):
    """state = dict(t, gbar, xbar, mu); returns (x, xbar) after one update with g = TARGET - accept_prob."""
    t = state["t"] + 1.0
    g = TARGET - accept_prob
    gbar = (1.0 - 1.0 / (t + T0)) * state["gbar"] + g / (t + T0)
    x = state["mu"] - (math.sqrt(t) / GAMMA) * gbar
    eta = t ** (-KAPPA)
    xbar = (1.0 - eta) * state["xbar"] + eta * x
    state.update(t=t, gbar=gbar, xbar=xbar)
    return x, xbar


def initial_position(shapes):
    """pyro's init_to_uniform(radius=2): every element Uniform(-2, 2) from torch's CPU generator, key by key in state_dict order."""
    return {k: (torch.rand(s) * 2 - 1) * INIT_RADIUS for k, s in shapes.items()}


def uniform(key, i):
    k = (int(key) ^ UNIF_KEY) & 0xFFFFFFFFFFFFFFFF
    x0 = O.philox4x32_10(np.uint32(i & 0xFFFFFFFF), np.uint32(0), np.uint32(0), np.uint32(0), np.uint32(k & 0xFFFFFFFF), np.uint32(k >> 32))[0]
    return float(x0) * 2.0 ** -32


class Restatement:
    """HmcSampler on the CPU in `dtype`: same initial position, same (key, draw id) momenta and uniforms.  The adaptation scalars (eps, the
    dual-averaging state, U, K, dH) are Python floats in every dtype, as the device's state block is fp64."""

    def __init__(self, arch, act, q0, x, y, step_size, num_steps, key, dtype=torch.float64, adapt_step_size=True, adapt_mass_matrix=True):
        self.arch, self.act, self.dtype, self.key = arch, act, dtype, int(key) & 0xFFFFFFFFFFFFFFFF
        self.keys = R.state_keys(arch)
        self.shapes = {k: tuple(q0[k].shape) for k in self.keys}
        self.x, self.y = x.reshape(x.shape[0], -1).to(dtype), y.long()
        self.q = self.flat(q0)
        self.m_inv = torch.ones_like(self.q)
        self.eps, self.traj = float(step_size), float(step_size) * num_steps
        self.adapt_step_size, self.adapt_mass_matrix = adapt_step_size, adapt_mass_matrix
        self.da = {"t": 0.0, "gbar": 0.0, "xbar": 0.0, "mu": math.log(10 * self.eps)}
        self.w_mean, self.w_m2 = torch.zeros_like(self.q), torch.zeros_like(self.q)
        self.U, self.g = self.potential(self.q)
        self.searches = 0
        self.log, self.search_log, self.adapt_log, self.search_scales = [], [], [], []

    # -- layout
    def flat(self, d):
        return torch.cat([d[k].detach().reshape(-1).to(self.dtype) for k in self.keys])

    def unflat(self, v):
        out, off = {}, 0
        for k in self.keys:
            n = int(np.prod(self.shapes[k]))
            out[k] = v[off:off + n].view(self.shapes[k])
            off += n
        return out

    # -- the pieces
    def potential(self, q):
        """(U, dCE/dW) at q: U a Python float, the gradient WITHOUT the prior's q (the device caches dCE/dW too)."""
        ce, g = R.ce_grads(self.x, self.y, self.unflat(q), self.arch, self.act)
        return float(ce) + float(0.5 * (q * q).sum()), self.flat(g)

    def kinetic(self, r):
        return float(0.5 * (self.m_inv * r * r).sum())

    def momentum(self, key, draw_id):
        e = R.draw_eps(self.shapes, self.arch, key, draw_id)
        return self.flat({k: v[0] for k, v in e.items()}) / torch.sqrt(self.m_inv)

    def length(self, eps=None):
        return max(1, int(self.traj / (self.eps if eps is None else eps)))

    def leapfrog(self, q, r, g, n, eps=None):
        """n velocity-Verlet steps from (q, r) with dCE/dW = g at q -> (q, r, dCE/dW, U) at the end."""
        eps = self.eps if eps is None else eps
        U = None
        for _ in range(n):
            r = r - 0.5 * eps * (g + q)
            q = q + eps * self.m_inv * r
            U, g = self.potential(q)
            r = r - 0.5 * eps * (g + q)
        return q, r, g, U

    def _probe(self, eps):
        """dH of one leapfrog step at eps from fresh momentum of the search stream."""
        r = self.momentum(self.key ^ SEARCH_KEY, self.searches)
        self.searches += 1
        K0 = self.kinetic(r)
        _, r1, _, U1 = self.leapfrog(self.q, r, self.g, 1, eps)
        K1 = self.kinetic(r1)
        dH = (U1 + K1) - (self.U + K0)
        self.search_scales.append(abs(U1) + K1 + K0)
        return math.inf if dH != dH else dH

    def find_reasonable_step_size(self):
        log08, tries = math.log(0.8), []
        dH = self._probe(self.eps)
        tries.append((self.eps, dH))
        direction = 1 if -dH > log08 else -1
        new = direction
        while new == direction:
            assert len(tries) <= MAX_SEARCH, "the step-size search did not end"
            self.eps = self.eps * 2.0 ** direction
            dH = self._probe(self.eps)
            tries.append((self.eps, dH))
            new = 1 if -dH > log08 else -1
        self.search_log.append(tries)
        self.da = {"t": 0.0, "gbar": 0.0, "xbar": 0.0, "mu": math.log(10 * self.eps)}

    def search_margin(self):
        """min over every search try of | -dH - log 0.8 | (what a direction decision rests on)."""
        return min((abs(-dH - math.log(0.8)) for tries in self.search_log for _, dH in tries), default=math.inf)

    def transition(self, i, adapt=False, window_end=False, welford_n=0):
        eps, frac = self.eps, self.traj / self.eps - math.floor(self.traj / self.eps)
        L = self.length()
        r0 = self.momentum(self.key, i)
        K0 = self.kinetic(r0)
        q1, r1, g1, U1 = self.leapfrog(self.q, r0, self.g, L)
        K1 = self.kinetic(r1)
        dH = (U1 + K1) - (self.U + K0)
        dH = math.inf if dH != dH else dH
        ap = min(1.0, math.exp(-dH)) if dH > -700 else 1.0
        u = uniform(self.key, i)
        acc = u < ap
        if acc:
            self.q, self.g, self.U = q1, g1, U1
        if adapt:
            xx, xbar = dual_averaging_update(self.da, ap)
            self.eps = math.exp(xbar if window_end else xx)
        if welford_n > 0:
            self.welford(self.q, welford_n)
        rec = {"eps": eps, "L": L, "dH": dH, "accept_prob": ap, "accepted": acc, "u": u, "U_new": U1, "K_new": K1, "K_old": K0,
               "margin": abs(u - ap), "L_fraction": frac, "q_end": q1, "r_end": r1}
        self.log.append(rec)
        return rec

    def welford(self, q, n):
        """Row n (1-based) of a window enters the running mean / M2."""
        d = q - self.w_mean
        self.w_mean = self.w_mean + d / n
        self.w_m2 = self.w_m2 + d * (q - self.w_mean)

    def window_end(self, n):
        self.m_inv = (n / ((n + 5.0) * (n - 1.0))) * self.w_m2 + 1e-3 * 5.0 / (n + 5.0)
        self.w_mean, self.w_m2 = torch.zeros_like(self.q), torch.zeros_like(self.q)

    def run(self, num_samples, warmup):
        """The chain: warmup transitions with adaptation, then num_samples transitions at fixed eps, L.  Returns the stack [S, n_params];
        self.adapt_log[i] = (eps, m_inv.clone()) after warmup transition i."""
        sched = windows(warmup)
        if warmup > 0 and self.adapt_step_size:
            self.find_reasonable_step_size()
        for (a, b, kind) in sched:
            mid = kind == "middle" and self.adapt_mass_matrix
            for i in range(a, b):
                self.transition(i, adapt=self.adapt_step_size, window_end=(i == b - 1), welford_n=(i - a + 1) if mid else 0)
                if i == b - 1:
                    if mid:
                        self.window_end(b - a)
                    if self.adapt_step_size and b < warmup:          # after the last window the averaged exp(xbar) is the sampling step size
                        self.find_reasonable_step_size()
                self.adapt_log.append((self.eps, self.m_inv.clone()))
        out = []
        for i in range(num_samples):
            self.transition(warmup + i)
            out.append(self.q.clone())
        return torch.stack(out) if out else torch.zeros(0, self.q.numel(), dtype=self.dtype)

    def margins(self):
        """(min |u - accept_prob|, min distance of trajectory_length / eps from an integer, min search margin) over the whole run."""
        m = min(r["margin"] for r in self.log)

        def rel(rec):                  # L = max(1, int(ratio)) changes at the integers >= 2 only; a relative change d of eps moves ratio by ratio d
            ratio = self.traj / rec["eps"]
            return (2.0 - ratio if ratio < 1.5 else min(rec["L_fraction"], 1 - rec["L_fraction"])) / ratio
        f = min(rel(r) for r in self.log)
        return m, f, self.search_margin()


def predict(stack, shapes_keys, x, arch, act):
    """Mean softmax over the stack's samples in fp64: BNN.forward of the chain.  stack: dict key -> [S, ...]."""
    return O.bnn_forward(x.double(), {k: v.double() for k, v in stack.items()}, arch, act, int(next(iter(stack.values())).shape[0]))


def relmax(a, b):
    """max |a - b| over max |b| (b: the fp64 value)."""
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))


# ---------------------------------------------------------------------------------------------------------------------------------------
# The cases of tests/test_hip_hmc.py (shared with the derivation of its bounds below)
# ---------------------------------------------------------------------------------------------------------------------------------------
# (arch, activation, D, H, C, B, L, unit m_inv): both nets, the four activations, ragged D / H / B, L = 1 and 10
LEAP_CASES = [("fc", "leaky", 2, 16, 2, 3, 1, True), ("fc2", "tanh", 10, 32, 3, 37, 10, False), ("fc", "sigm", 17, 96, 10, 1024, 10, True),
              ("fc2", "relu", 784, 512, 10, 5000, 1, False), ("fc", "relu", 784, 32, 10, 37, 10, False), ("fc2", "leaky", 2, 96, 2, 1024, 10, True),
              ("fc2", "sigm", 17, 16, 10, 3, 1, False), ("fc", "tanh", 10, 512, 10, 5000, 10, True)]
LEAP_KEY = 0x0123456789ABCDEF


KINK = 2e-6          # as tests/test_hip_svi_train.py: a hidden pre-activation this close to 0 may fall on either side in fp32, and act' jumps there


def kink_margin(q, x, arch, act):
    """Per point: the smallest |hidden pre-activation| at the weights q (key -> tensor) in fp64; inf for the smooth activations."""
    if act not in ("relu", "leaky"):
        return torch.full((x.shape[0],), float("inf"), dtype=torch.float64)
    ks = R.layer_keys(arch)
    h, m = x.double(), torch.full((x.shape[0],), float("inf"), dtype=torch.float64)
    for k in ks[:-1]:
        a = h @ q[k + ".weight"].double().T + q[k + ".bias"].double()
        m = torch.minimum(m, a.abs().amin(1))
        h = O._act(a, act)
    return m


def leap_case(arch, act, D, H, Cn, B, L, unit, filter_kinks=True):
    """Inputs of one LEAP_CASES case: position (uniform, half-width 0.1 at D > 16, else 0.5), batch, labels, m_inv, step size.
    relu / leaky: the gradient of U is DISCONTINUOUS in q where a hidden pre-activation of a point crosses 0, so a point within KINK of such a
    crossing at any position of the fp64 trajectory where the gradient is taken (q_0 ... q_L) belongs to either side in fp32 — one unit of one
    point on the other side moves a weight gradient by that point's whole contribution.  Such points are taken out of the batch, as the
    gradient tests of SVI training do ("dropped" counts them).  Those tests look at ONE position and allow 1 % of the batch; a trajectory has
    L + 1 positions, each with its own near-crossings, so the allowance here is 5 % of the batch (the most: 40 of 1024 points, 3.9 %, over the
    11 positions of the fc2-leaky 2 -> 96 case, 192 hidden units a point; 25 of 5000 over the 2 positions of the fc2-relu 784 -> 512 case).  Removing a point moves the trajectory, so
    the selection is repeated until the trajectory of the remaining batch has no such point."""
    g = torch.Generator().manual_seed(1000 * H + B)
    shapes = R.shapes_of(arch, D, H, Cn)
    q0 = {k: (0.1 if D > 16 else 0.5) * (torch.rand(*s, generator=g) * 2 - 1) for k, s in shapes.items()}
    x = torch.rand(B, D, generator=g) if D > 16 else 4 * torch.rand(B, D, generator=g) - 2
    lab = torch.randint(0, Cn, (B,), generator=g)
    n = sum(int(np.prod(s)) for s in shapes.values())
    m_inv = torch.ones(n) if unit else 0.5 + torch.rand(n, generator=g)
    eps = min(0.01, 2.0 / B)
    dropped = 0
    while filter_kinks and act in ("relu", "leaky"):
        rs = Restatement(arch, act, q0, x, lab, eps, L, LEAP_KEY)
        rs.m_inv = m_inv.double()
        q, r, gq = rs.q, rs.momentum(LEAP_KEY, 0), rs.g
        margin = kink_margin(rs.unflat(q), x, arch, act)
        for _ in range(L):
            q, r, gq, _ = rs.leapfrog(q, r, gq, 1)
            margin = torch.minimum(margin, kink_margin(rs.unflat(q), x, arch, act))
        ok = margin > KINK
        if bool(ok.all()):
            break
        dropped += int((~ok).sum())
        x, lab = x[ok], lab[ok]
    return {"shapes": shapes, "q0": q0, "x": x, "lab": lab, "m_inv": m_inv, "eps": eps, "dropped": dropped}


# (name, arch, activation, H, n points, step size, L, key): one accepted transition and one rejected one (large step size) on half-moons
TRANSITION_CASES = [("accept", "fc2", "tanh", 32, 200, 0.002, 5, 21), ("reject", "fc2", "tanh", 32, 200, 0.07, 5, 21),
                    ("accept", "fc", "leaky", 64, 200, 0.002, 5, 22), ("reject", "fc", "leaky", 64, 200, 0.07, 5, 22)]


def transition_case(arch, act, H, n, seed=4):
    x, y = R.two_moons(n, 0.1, seed)
    g = torch.Generator().manual_seed(H + n)
    q0 = {k: 0.5 * (torch.rand(*s, generator=g) * 2 - 1) for k, s in R.shapes_of(arch, 2, H, 2).items()}
    return q0, x, y.argmax(-1)


# (arch, activation, H, n points, step size, num_steps, warmup, samples, key, init seed): the full runs on half-moons; the keys are chosen by
# `python tests/hmc_restate.py keys` so that the fp64 run's decision margins hold at EVERY transition (test_hip_hmc.py checks them again)
RUN_CASES = [("fc2", "leaky", 32, 128, 0.01, 4, 24, 20, 1716, 0), ("fc", "tanh", 64, 128, 0.01, 4, 24, 20, 3, 1)]


def run_case(arch, act, H, n, seed):
    x, y = R.two_moons(n, 0.1, 7)
    torch.manual_seed(seed)
    return initial_position(R.shapes_of(arch, 2, H, 2)), x, y.argmax(-1)


def replay_train_hmc(x, y, batch_size, arch, act, H, n_samples, warmup, step_size, num_steps, dtype=torch.float64):
    """BNN.train_hmc on the CPU: the same sequence of draws from the CPU generator after the seeding (a DataLoader's iterator draws its base
    seed when it is made, shuffled or not; then the initial position, the key, and after the chain the resampling indices), the chain on the
    LAST batch.  Returns (restatement, resampled stack [n_samples, n_params], key, indices)."""
    import random
    from torch.utils.data import DataLoader
    random.seed(0)
    torch.manual_seed(0)
    np.random.seed(0)
    loader = DataLoader(list(zip(x, y)), batch_size=batch_size, shuffle=False)
    for xb, yb in loader:
        pass
    q0 = initial_position(R.shapes_of(arch, int(np.prod(x.shape[1:])), H, int(y.shape[-1])))
    key = int(torch.randint(-(2 ** 63), 2 ** 63 - 1, (1,), dtype=torch.int64).item()) & 0xFFFFFFFFFFFFFFFF
    batch_samples = int(n_samples / max(1, int(len(x) / batch_size))) + 1
    rs = Restatement(arch, act, q0, xb, yb.argmax(-1), step_size, num_steps, key, dtype=dtype)
    S = rs.run(batch_samples, warmup)
    idx = torch.randint(0, batch_samples, (n_samples,))
    return rs, S[idx], key, idx


# BNN.train_hmc end to end (test_hip_hmc.py): MoonsBNN(hidden, "leaky", "fc2", "hmc", ..., n_samples, warmup, n_inputs) on two_moons(n_inputs,
# 0.1, data seed), held-out two_moons(200, 0.1, data seed + 1000).  train_hmc seeds itself, so its key is fixed; the DATA SEED is the free
# parameter: `PYTHONPATH=. python tests/hmc_restate.py e2e` looks for one at which the fp64 replay's margins hold at every transition.
E2E = {"hidden": 16, "n_samples": 20, "warmup": 20, "n_inputs": 128, "data_seed": 0}
FORWARD_BAR = 1e-5           # the forward kernels' bar on a probability (tests/conftest.py)


def e2e_case(data_seed):
    x, y = R.two_moons(E2E["n_inputs"], 0.1, data_seed)
    xt, yt = R.two_moons(200, 0.1, data_seed + 1000)
    return x, y, xt, yt


def e2e_replay(data_seed, dtype=torch.float64):
    x, y, xt, yt = e2e_case(data_seed)
    rs, S, key, idx = replay_train_hmc(x, y, 1024, "fc2", "leaky", E2E["hidden"], E2E["n_samples"], E2E["warmup"], 0.001, 10, dtype)
    p = predict(_unflat_stack(rs, S), None, xt, "fc2", "leaky")
    return rs, S, p, key


def _unflat_stack(rs, S):
    out, off = {}, 0
    for k in rs.keys:
        n = int(np.prod(rs.shapes[k]))
        out[k] = S[:, off:off + n].reshape((S.shape[0],) + rs.shapes[k])
        off += n
    return out


def e2e_prediction_bar(p32, p64):
    """How far a mean probability of the GPU chain may lie from the fp64 replay's: 4 x the fp32 replay's own deviation (the samples differ
    within their bound and the probabilities with them) + the forward kernels' bar.  A point is compared if its top-2 gap exceeds twice that."""
    return FACTOR * float((p32.double() - p64).abs().max()) + FORWARD_BAR


def energy_scale(rec):
    """The size of the sums dH is a difference of: |U'| + K' + K."""
    return abs(rec["U_new"]) + rec["K_new"] + rec["K_old"]


def _leap_dev():
    worst = {"leapfrog_q": 0.0, "leapfrog_r": 0.0}
    for case in LEAP_CASES:
        c = leap_case(*case)
        out = {}
        for dt in (torch.float64, torch.float32):
            rs = Restatement(case[0], case[1], c["q0"], c["x"], c["lab"], c["eps"], case[6], LEAP_KEY, dtype=dt)
            rs.m_inv = c["m_inv"].to(dt)
            out[dt] = rs.leapfrog(rs.q, rs.momentum(LEAP_KEY, 0), rs.g, case[6])
        dq, dr = relmax(out[torch.float32][0], out[torch.float64][0]), relmax(out[torch.float32][1], out[torch.float64][1])
        print(f"  leapfrog {case}: q {dq:.2e}  r {dr:.2e}  points within the kink margin taken out: {c['dropped']}")
        worst["leapfrog_q"], worst["leapfrog_r"] = max(worst["leapfrog_q"], dq), max(worst["leapfrog_r"], dr)
    return worst


REVERSE_CASE = LEAP_CASES[1]             # fc2 / tanh, D 10, H 32, C 3, B 37, L 10, non-unit m_inv: smooth, so no kink filter


def reverse_round_trip(rs, r0, L):
    """L steps from (rs.q, r0), the momentum negated, L more: -> the position the round trip ends at (rs.q in exact arithmetic)."""
    q1, r1, g1, _ = rs.leapfrog(rs.q, r0, rs.g, L)
    return rs.leapfrog(q1, -r1, g1, L)[0]


def _reverse_dev():
    case = REVERSE_CASE
    c = leap_case(*case)
    rs = Restatement(case[0], case[1], c["q0"], c["x"], c["lab"], c["eps"], case[6], LEAP_KEY, dtype=torch.float32)
    rs.m_inv = c["m_inv"].float()
    d = relmax(reverse_round_trip(rs, rs.momentum(LEAP_KEY, 0), case[6]), rs.q)
    print(f"  time reversal {case}: fp32 round trip {d:.2e} of max |q| from its start")
    return {"reverse_q": d}


def _welford_dev():
    """The Welford recurrence of `Restatement.welford` in fp32 over tests/hmc_exact_cases.welford_rows against the fp64 two-pass figures."""
    import hmc_exact_cases as HX
    rows = HX.welford_rows()
    mean64, m264, minv64 = (torch.from_numpy(v) for v in HX.welford_reference(rows))
    rs = Restatement.__new__(Restatement)
    rs.w_mean, rs.w_m2 = torch.zeros(rows.shape[1]), torch.zeros(rows.shape[1])
    for t, row in enumerate(rows, start=1):
        rs.welford(row, t)
    dm = relmax(rs.w_mean, mean64)
    rs.q = rows[0]
    rs.window_end(rows.shape[0])
    dv = relmax(rs.m_inv, minv64)
    naive = rows.square().sum(0) - rows.shape[0] * rows.mean(0).square()          # the fp32 sum of squares, for the record
    print(f"  welford over {tuple(rows.shape)} rows at 1000 +- 0.01: fp32 recurrence mean {dm:.2e}  m_inv {dv:.2e}"
          f"  (an fp32 sum of squares gives M2 off by {relmax(naive, m264):.1e} of its max)")
    return {"welford_mean": dm, "welford_m_inv": dv}


def _transition_dev():
    worst = {"U": 0.0, "K": 0.0, "dH": 0.0}
    for (name, arch, act, H, n, eps, L, key) in TRANSITION_CASES:
        q0, x, lab = transition_case(arch, act, H, n)
        rec = {}
        for dt in (torch.float64, torch.float32):
            rs = Restatement(arch, act, q0, x, lab, eps, L, key, dtype=dt, adapt_step_size=False)
            rec[dt] = rs.transition(0)
        a, b = rec[torch.float32], rec[torch.float64]
        dU, dK = abs(a["U_new"] - b["U_new"]) / abs(b["U_new"]), max(abs(a["K_new"] - b["K_new"]) / b["K_new"], abs(a["K_old"] - b["K_old"]) / b["K_old"])
        ddH = abs(a["dH"] - b["dH"]) / energy_scale(b)
        print(f"  transition {name} {arch}: accepted {b['accepted']} dH {b['dH']:.3e} U {dU:.2e} K {dK:.2e} dH/scale {ddH:.2e} (scale {energy_scale(b):.0f})")
        assert b["accepted"] == (name == "accept") and a["accepted"] == b["accepted"]
        worst = {"U": max(worst["U"], dU), "K": max(worst["K"], dK), "dH": max(worst["dH"], ddH)}
    return worst


def _run(case, key, dtype):
    arch, act, H, n, eps, steps, warmup, samples, _, seed = case
    q0, x, lab = run_case(arch, act, H, n, seed)
    rs = Restatement(arch, act, q0, x, lab, eps, steps, key, dtype=dtype)
    return rs, rs.run(samples, warmup)


def run_margins_ok(rs, bound, in_dH=False):
    """The fp64 run's margins against the bounds: every |u - accept_prob| and every search try's |-dH - log 0.8| above 100 x the dH bound (in
    units of the transition's energy scale), every L-deciding distance above the eps bound.  in_dH: the decision margin taken where the
    error lives, |dH - (-log u)| (the decision flips where dH crosses -log u; |log a - log u| >= |a - u| on (0, 1], so this holds wherever
    the |u - accept_prob| form does, and also at a diverged trajectory whose dH of 1e5 and more rejects whatever its last digits are)."""
    def decision(r):
        if in_dH:
            return abs(r["dH"] + math.log(max(r["u"], 1e-300))) if math.isfinite(r["dH"]) else math.inf
        return r["margin"]
    m = min(decision(r) / (100 * bound["dH"] * energy_scale(r)) if math.isfinite(energy_scale(r)) else math.inf for r in rs.log)
    tries = [dH for t in rs.search_log for _, dH in t]
    s = min((abs(-dH - math.log(0.8)) / (100 * bound["dH"] * sc) for dH, sc in zip(tries, rs.search_scales) if math.isfinite(dH)), default=math.inf)
    f = rs.margins()[1] / bound["eps"] if bound["eps"] > 0 else math.inf
    return m, s, f


if __name__ == "__main__":
    import sys
    torch.set_num_threads(8)
    if sys.argv[1:] == ["e2e"]:
        for seed in range(0, 400):
            r64, _, p64, key = e2e_replay(seed)
            r32, _, p32, _ = e2e_replay(seed, torch.float32)
            same = [a["accepted"] == b["accepted"] and a["L"] == b["L"] for a, b in zip(r32.log, r64.log)]
            bar = e2e_prediction_bar(p32, p64)
            share = float((R.top2_gap(p64) <= 2 * bar).float().mean())
            m = run_margins_ok(r64, BOUND, in_dH=True)
            print(f"  data seed {seed} key {key:#x}: margins {m[0]:.2f} {m[1]:.2f} {m[2]:.2f}  fp32 same decisions {all(same)}  bar {bar:.1e}  excluded {share:.3f}", flush=True)
            if min(m) > 1 and all(same) and share <= 0.01:
                break
    elif sys.argv[1:] == ["keys"]:
        for case in RUN_CASES:
            for key in range(1, 4000):
                rs, _ = _run(case, key, torch.float64)
                m, s, f = run_margins_ok(rs, BOUND)
                print(f"  {case[0]} key {key}: margins in units of their bar: decision {m:.2f} search {s:.2f} L {f:.2f}", flush=True)
                if min(m, s, f) > 1:
                    r32, _ = _run(case, key, torch.float32)
                    de = max(abs(a[0] - b[0]) / b[0] for a, b in zip(r32.adapt_log, rs.adapt_log))
                    same = all(a["accepted"] == b["accepted"] and a["L"] == b["L"] for a, b in zip(r32.log, rs.log))
                    print(f"      its fp32 run: same decisions {same}, eps within {de:.2e}", flush=True)
                    if same and de <= BOUND["eps"]:
                        break
    else:
        w = _leap_dev()
        w.update(_transition_dev())
        w.update(_reverse_dev())
        w.update(_welford_dev())
        for case in RUN_CASES:
            key = case[8] if case[8] is not None else 1
            (r64, s64), (r32, s32) = _run(case, key, torch.float64), _run(case, key, torch.float32)
            same = [a["accepted"] == b["accepted"] and a["L"] == b["L"] for a, b in zip(r32.log, r64.log)]
            de = max(abs(a[0] - b[0]) / b[0] for a, b in zip(r32.adapt_log, r64.adapt_log))
            dm, ds = relmax(r32.m_inv, r64.m_inv), relmax(s32, s64)
            ddh = max(abs(a["dH"] - b["dH"]) / energy_scale(b) for a, b in zip(r32.log, r64.log) if math.isfinite(b["dH"]))
            print(f"  run {case[:3]} key {key}: same decisions {all(same)} eps {de:.2e} m_inv {dm:.2e} samples {ds:.2e} dH/scale {ddh:.2e}"
                  f"  L {sorted(set(r['L'] for r in r64.log))} acceptance {sum(r['accepted'] for r in r64.log)}/{len(r64.log)}")
            for k, v in (("eps", de), ("m_inv", dm), ("samples", ds)):
                w[k] = max(w.get(k, 0.0), v)
        print({k: float(f"{v:.2e}") for k, v in w.items()})
