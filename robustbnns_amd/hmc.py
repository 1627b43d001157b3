"""HMC posteriors of fc / fc2 nets on the GPU — the `_train_hmc` half of the reference (model_bnn.py:260-301): the algorithm of pyro 1.3.0's
HMC(model, step_size, num_steps) under MCMC(num_samples, warmup_steps, num_chains=1), restated in tests/hmc_restate.py (pyro's constants
there are [recalled]; seed-for-seed parity with pyro's RNG stream is unpinned, as for the SVI draw).

Position q = the flat parameter buffer of svi_train.SviTrainer (state_dict order, unpadded, row-major);
U(q) = sum_b CE(z_b(q), y_b) + 1/2 sum q^2, grad U = dCE/dW + q.  dCE/dW is rbnn_svi_train_forward + rbnn_svi_weight_grads
(csrc/rbnn_train.hip); the momentum draw, the fused leapfrog updates, the one-block decision with dual averaging, the commit with Welford and the sample
stack, and the window end are csrc/rbnn_hmc.hip.  Launches of one leapfrog step: fc 2 + 1 + 1, fc2 4 + 1 + 1 (forward, weight gradients,
one fused update); of one transition with L steps: 1 (momentum) + 1 (opening update) + L x (step) + 1 (decision) + 1 (commit).

Host synchronisation: warmup reads the device's state block once per transition (L follows the adapted step size, and the step-size search
loops on a device value); sampling (step size and L fixed) makes NO device->host synchronisation — the logs and the sample stack are read
once at the end of run().
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _hip
from .flat_params import flatten, train_workspace, unflat, ws_struct
from .posterior import LAYER_KEYS
from .svi_train import state_keys

INIT_RADIUS = 2.0                   # pyro's init_to_uniform [recalled]
START_BUFFER, END_BUFFER, INIT_WINDOW = 75, 50, 25      # pyro's WarmupAdapter [recalled]
MAX_SEARCH = 64                     # tries of one step-size search before it is an error
LOG_COLUMNS = ("eps", "dH", "accept_prob", "accepted", "u", "U_new", "K_new", "K_old")


def initial_position(shapes):
    """pyro's init_to_uniform(radius=2): every element Uniform(-2, 2) from torch's CPU generator, key by key in state_dict order.
    shapes: list of (key, shape)."""
    return {k: (torch.rand(shp) * 2 - 1) * INIT_RADIUS for k, shp in shapes}


def windows(warmup):
    """[(start, end, kind)], end exclusive, kind in {"start", "middle", "end"}: pyro's adaptation windows [recalled] tiling [0, warmup).
    < 20: one window; else buffers of 75 / 50 and a first middle window of 25 (15 % / 10 % / the rest if they do not fit), middle windows
    doubling, the last one absorbing the remainder."""
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
            size = end_start - cur
            nxt = size
        out.append((cur, cur + size, "middle"))
        cur, size = cur + size, nxt
    if end > 0:
        out.append((end_start, warmup, "end"))
    return out


class HmcSampler:
    """Device-resident state of one HMC chain over an fc / fc2 net: the trajectory's position / dCE/dW (an rbnn_svi_train_net's W / grad), the
    chain's cached position and gradient, momentum, the diagonal inverse mass, Welford's mean / M2, the fp64 state block, the per-transition
    log and the sample stack.  `launches` counts kernel launches by the entry points' documented launch counts."""

    def __init__(self, arch, activation, input_shape, n_classes, q0, step_size, num_steps, device, key, adapt_step_size=True,
                 adapt_mass_matrix=True, batch_size=128):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise NotImplementedError(f"HMC runs on the MI355X kernels only (device {device!r}): there is no CPU compute path")
        if arch not in LAYER_KEYS:
            raise NotImplementedError(f"HMC covers fc and fc2, not {arch!r} (conv needs conv weight gradients)")
        self.k = _hip.HipKernels()
        self.arch, self.activation, self.device = arch, activation, dev
        self.input_shape = tuple(int(v) for v in input_shape)
        self.keys = state_keys(arch)
        self.shapes = {k: tuple(q0[k].shape) for k in self.keys}
        self.D = int(np.prod(self.input_shape))
        self.H, self.C = int(self.shapes[self.keys[1]][0]), int(n_classes)
        net = _hip.SviTrainNet()
        net.arch, net.activation = _hip.ARCHS[arch], _hip.ACTIVATIONS[activation]
        net.in_features, net.hidden, net.n_classes = self.D, self.H, self.C
        nq, ne = C.c_int64(0), C.c_int64(0)
        n = int(self.k.lib.rbnn_hmc_sizes(C.byref(net), C.byref(nq), C.byref(ne)))
        _hip.check(min(n, 0), "rbnn_hmc_sizes")
        self.n_params = n
        z = lambda m=n: torch.zeros(m, dtype=torch.float32, device=dev)
        self.W, self.grad = z(), z()
        net.W, net.grad = self.W.data_ptr(), self.grad.data_ptr()
        self.net = net
        self.q_cur = flatten(q0, self.keys).to(dev)
        assert self.q_cur.numel() == n, (self.q_cur.numel(), n)
        self.g_cur, self.r, self.w_mean, self.w_m2 = z(), z(), z(), z()
        self.m_inv = torch.ones(n, dtype=torch.float32, device=dev)
        self.k0_part, self.k1_part, self.p_part = z(int(nq.value)), z(int(ne.value)), z(int(ne.value))
        self.state = torch.zeros(_hip.HMC_STATE, dtype=torch.float64, device=dev)
        self.log_t = self.samples_t = None
        self.step_size, self.num_steps = float(step_size), int(num_steps)
        self.trajectory_length = self.step_size * self.num_steps
        self.adapt_step_size, self.adapt_mass_matrix = bool(adapt_step_size), bool(adapt_mass_matrix)
        self.key = int(key) & 0xFFFFFFFFFFFFFFFF
        self.eps_host = self.step_size
        self.searches = 0
        self.search_log = []
        self.launches = 0
        self.fwd_launches = 2 if arch == "fc" else 4
        self.Bmax = self.B = 0
        self._ensure(int(batch_size))
        self._set_state(eps=self.step_size, mu=math.log(10 * self.step_size))
        self._bind()
        # the logs of the last run(): one entry per transition, warmup included
        self.eps_log = self.L_log = self.dH_log = self.accept_prob_log = self.accepted_log = None

    # -- buffers --------------------------------------------------------------------------------------------------------------------
    def _bind(self):
        ch = _hip.HmcChain()
        for name in ("q_cur", "g_cur", "r", "m_inv", "w_mean", "w_m2", "k0_part", "k1_part", "p_part", "state"):
            setattr(ch, name, getattr(self, name).data_ptr())
        ch.log = None if self.log_t is None else self.log_t.data_ptr()
        ch.samples = None if self.samples_t is None else self.samples_t.data_ptr()
        ch.log_rows = 0 if self.log_t is None else int(self.log_t.shape[0])
        ch.sample_rows = 0 if self.samples_t is None else int(self.samples_t.shape[0])
        self.chain = ch

    def _ensure(self, B):
        if B <= self.Bmax:
            return
        self.ws_t = train_workspace(self.arch, B, self.H, self.device)
        self.ws = ws_struct(_hip.SviTrainWs, _hip.SVI_TRAIN_WS_KEYS, self.ws_t)
        self.X = torch.zeros(B, self.D, dtype=torch.float32, device=self.device)
        self.labels = torch.zeros(B, dtype=torch.int32, device=self.device)
        self.Bmax = B

    def unflat(self, buf):
        """state_dict key -> view of `buf` ([n_params] or [S, n_params]) in that tensor's shape."""
        return unflat(buf, self.keys, self.shapes)

    def _set_state(self, **kv):
        """Host -> device writes of state-block entries (warmup / set-up only)."""
        for name, v in kv.items():
            self.state[_hip.HMC_ST[name]] = float(v)

    def read_state(self):
        """The state block as a dict (a device->host synchronisation)."""
        s = self.state.tolist()
        return {name: s[i] for name, i in _hip.HMC_ST.items()}

    # -- launches -------------------------------------------------------------------------------------------------------------------
    def _st(self):
        return _hip.stream_of(self.W)

    def _gradient(self):
        """dCE/dW and the per-point CE at self.W: the training forward (fc 2 launches, fc2 4) + the weight gradients (1)."""
        lib, net = self.k.lib, C.byref(self.net)
        _hip.check(lib.rbnn_svi_train_forward(net, _hip.ptr(self.X), self.D, self.B, _hip.ptr(self.labels), C.byref(self.ws), self._st()),
                   "rbnn_svi_train_forward")
        _hip.check(lib.rbnn_svi_weight_grads(net, _hip.ptr(self.X), self.D, self.B, C.byref(self.ws), self._st()), "rbnn_svi_weight_grads")
        self.launches += self.fwd_launches + 1

    def _update(self, phase):
        _hip.check(self.k.lib.rbnn_hmc_leapfrog_update(C.byref(self.net), C.byref(self.chain), phase, self._st()), "rbnn_hmc_leapfrog_update")
        self.launches += 1

    def _momentum(self, key, draw_id):
        _hip.check(self.k.lib.rbnn_hmc_momentum(C.byref(self.net), C.byref(self.chain), C.c_uint64(key & 0xFFFFFFFFFFFFFFFF),
                                                C.c_uint32(draw_id & 0xFFFFFFFF), self._st()), "rbnn_hmc_momentum")
        self.launches += 1

    def _decide(self, mode, transition=0, adapt=False, window_end=False):
        _hip.check(self.k.lib.rbnn_hmc_decide(C.byref(self.net), C.byref(self.chain), _hip.ptr(self.ws_t["ce"]), self.B, C.c_uint64(self.key),
                                              int(transition), mode, int(adapt), int(window_end), self._st()), "rbnn_hmc_decide")
        self.launches += 1

    def _commit(self, force=False, welford_n=0, sample_row=-1):
        _hip.check(self.k.lib.rbnn_hmc_commit(C.byref(self.net), C.byref(self.chain), int(force), int(welford_n), int(sample_row), self._st()),
                   "rbnn_hmc_commit")
        self.launches += 1

    # -- the chain ------------------------------------------------------------------------------------------------------------------
    def stage(self, x, labels):
        """The batch the potential is taken over (x [B, ...], labels int [B]) and the potential / gradient at the current position."""
        B = int(x.shape[0])
        self._ensure(B)
        self.B = B
        self.X[:B].copy_(x.reshape(B, -1))
        self.labels[:B].copy_(labels.reshape(B))
        self.refresh()

    def refresh(self):
        """U and dCE/dW of the chain's current position (after stage(), or after q_cur was written from outside)."""
        self.W.copy_(self.q_cur)
        self._gradient()
        self._update(_hip.HMC_ENERGY)
        self._decide(_hip.HMC_DECIDE_INIT)
        self._commit(force=True)

    def leapfrog(self, n, fused=True):
        """n leapfrog steps from (q_cur, r) at the state block's step size; the end point is left in self.W / self.r / self.grad and its K' and
        1/2 sum q'^2 in the partial sums.  fused=False: the plain half kick / drift / gradient / half kick sequence the fused updates restate."""
        if fused:
            self._update(_hip.HMC_OPEN)
            for s in range(n):
                self._gradient()
                self._update(_hip.HMC_MID if s + 1 < n else _hip.HMC_CLOSE)
            return
        self.W.copy_(self.q_cur)
        self.grad.copy_(self.g_cur)
        for s in range(n):
            self._update(_hip.HMC_KICK)
            self._update(_hip.HMC_DRIFT)
            self._gradient()
            self._update(_hip.HMC_KICK)
        self._update(_hip.HMC_ENERGY)

    def length(self, eps=None):
        return max(1, int(self.trajectory_length / (self.eps_host if eps is None else eps)))

    def transition(self, i, L=None, adapt=False, window_end=False, welford_n=0, sample_row=-1):
        """Transition i with L leapfrog steps (default: from the host's copy of the step size).  No device->host synchronisation."""
        L = self.length() if L is None else L
        self._momentum(self.key, i)
        self.leapfrog(L)
        self._decide(_hip.HMC_DECIDE_TRANSITION, i, adapt, window_end)
        self._commit(False, welford_n, sample_row)
        return L

    def _probe(self, eps):
        self._set_state(eps=eps)
        self._momentum(self.key ^ _hip.HMC_SEARCH_KEY, self.searches)
        self.searches += 1
        self.leapfrog(1)
        self._decide(_hip.HMC_DECIDE_PROBE)
        return self.read_state()["dH"]

    def find_reasonable_step_size(self):
        """pyro's search [recalled] from the current step size: one leapfrog step from fresh momentum, direction = +1 if -dH > log 0.8 else -1,
        eps *= 2^direction with new momentum each try until the direction flips; then dual averaging restarts with mu = log(10 eps)."""
        log08, tries = math.log(0.8), []
        eps = self.eps_host
        dH = self._probe(eps)
        tries.append((eps, dH))
        direction = 1 if -dH > log08 else -1
        new = direction
        while new == direction:
            if len(tries) > MAX_SEARCH:
                raise RuntimeError(f"the HMC step-size search did not end after {MAX_SEARCH} tries (last eps {eps:g}, dH {dH:g})")
            eps = eps * 2.0 ** direction
            dH = self._probe(eps)
            tries.append((eps, dH))
            new = 1 if -dH > log08 else -1
        self.search_log.append(tries)
        self.eps_host = eps
        self._set_state(eps=eps, t=0.0, gbar=0.0, xbar=0.0, mu=math.log(10 * eps))

    def run(self, x, labels, num_samples, warmup):
        """One chain on the batch: `warmup` adapting transitions, then num_samples at fixed step size and L.  Returns the sample stack as a dict
        state_dict key -> [num_samples, ...] (device tensors); the logs (eps_log, L_log, dH_log, accept_prob_log, accepted_log: one entry per
        transition, warmup included) and the final m_inv stay on the sampler."""
        num_samples, warmup = int(num_samples), int(warmup)
        total = warmup + num_samples
        self.log_t = torch.zeros(max(1, total), _hip.HMC_LOG, dtype=torch.float64, device=self.device)
        self.samples_t = torch.zeros(max(1, num_samples), self.n_params, dtype=torch.float32, device=self.device)
        self._bind()
        self.stage(x, labels)
        Ls = []
        if warmup > 0 and self.adapt_step_size:
            self.find_reasonable_step_size()
        for (a, b, kind) in windows(warmup):
            mid = kind == "middle" and self.adapt_mass_matrix
            for i in range(a, b):
                last = i == b - 1
                Ls.append(self.transition(i, None, self.adapt_step_size, last, (i - a + 1) if mid else 0))
                if last and mid:
                    _hip.check(self.k.lib.rbnn_hmc_window_end(C.byref(self.net), C.byref(self.chain), b - a, self._st()), "rbnn_hmc_window_end")
                    self.launches += 1
                if self.adapt_step_size:
                    self.eps_host = self.read_state()["eps"]            # warmup's one read per transition: L follows the adapted step size
                    if last:
                        self.find_reasonable_step_size()
        self.sample(warmup, num_samples, Ls)
        log = self.log_t[:total].cpu()                                  # the one read of the sampling phase
        self.eps_log, self.dH_log, self.accept_prob_log = log[:, 0].tolist(), log[:, 1].tolist(), log[:, 2].tolist()
        self.accepted_log, self.L_log, self.log = [bool(v) for v in log[:, 3].tolist()], Ls, log
        return self.unflat(self.samples_t[:num_samples])

    def sample(self, first, num_samples, Ls=None):
        """num_samples transitions first, first + 1, ... at the fixed step size and L, row i of the sample stack = the position after transition
        first + i.  No device->host synchronisation."""
        L = self.length()
        for i in range(num_samples):
            self.transition(first + i, L, False, False, 0, i)
            if Ls is not None:
                Ls.append(L)
