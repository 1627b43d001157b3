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

LockstepHmc runs K chains of one net shape with every launch covering all of them (the chain is grid dimension y: rbnn_hmc_lockstep_*), each
chain bit-identical to HmcSampler running it alone; split_r_hat is the convergence figure that goes with several chains.

The chain algorithm (transition, step-size search, warmup windows, sampling, logs) is written once, in _Chains, over K chains with per-chain
host lists; _OneChain (K = 1, the single-chain entry points, scalar / flat public values) and _LockstepChains (K chains behind every launch:
the per-chain device values, the state block's accessors, the element-wise launches) supply the launches, and their subclasses the gradient,
the staging of the batch and the shape of what they return.  HmcSampler is _OneChain on rbnn_hmc_* with the fc / fc2 gradient,
conv_hmc.ConvHmcSampler _OneChain on rbnn_conv_hmc_* with the conv gradient; LockstepHmc is _LockstepChains on rbnn_hmc_lockstep_*,
conv_hmc.ConvLockstepHmc _LockstepChains on rbnn_conv_hmc_chains_* (BNN.train_hmc_conv runs both conv classes).  HmcSampler and LockstepHmc
refuse a conv net.
"""
import ctypes as C
import math

import torch

from . import _hip
from .flat_params import FlatNets, flatten, keys_tensor, require_gpu_fc, set_data, train_workspace

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


def _view(name, k=None):
    """A per-chain host list of _Chains as a public attribute: the list itself (LockstepHmc), or chain k's entry (HmcSampler)."""
    if k is None:
        return property(lambda self: getattr(self, name), lambda self, v: setattr(self, name, list(v)))
    return property(lambda self: getattr(self, name)[k], lambda self, v: getattr(self, name).__setitem__(k, v))


class _Chains(FlatNets):
    """The buffers and the algorithm of K HMC chains over nets of one shape; the per-chain host values are lists of K: _eps (the host's copy
    of the step sizes), _traj (step size x num_steps), _searches (the probes' draw counters), _search_log.  A subclass supplies the launches
    (_gradient, _update, leapfrog, _draw, _decide, _commit, _window_end; each adds its documented launch count to `launches`), the state
    block's accessors (_set_state, read_state), set_active / _set_steps, _bind / _ensure and stage().  PARAM_KEYS / _hmc_sizes are what a net
    other than fc / fc2 replaces (conv_hmc.ConvHmcSampler): its state_dict keys and the sizes query of its own entry points."""
    PARAM_KEYS = None                                                    # None: the state_dict keys of fc / fc2

    def __init__(self, arch, activation, input_shape, n_classes, q0s, step_size, num_steps, device, keys, adapt_step_size, adapt_mass_matrix,
                 members):
        super().__init__(arch, activation, input_shape, n_classes, q0s[0], device, members, keys=self.PARAM_KEYS)
        K = self.K = len(q0s)
        dev, z = self.device, self.zeros
        n, self.n_qpart, self.n_epart = self._hmc_sizes()
        self.n_params = n
        self.W, self.grad = z(n), z(n)
        self.q_cur = torch.stack([flatten(q0, self.keys) for q0 in q0s]).reshape(*self.lead, n).to(dev)
        self.g_cur, self.r, self.w_mean, self.w_m2 = z(n), z(n), z(n), z(n)
        self.m_inv = torch.ones(*self.lead, n, dtype=torch.float32, device=dev)
        self.k0_part, self.k1_part, self.p_part = z(self.n_qpart), z(self.n_epart), z(self.n_epart)
        self.state = torch.zeros(*self.lead, _hip.HMC_STATE, dtype=torch.float64, device=dev)
        self.log_t = self.samples_t = None
        self.chain_keys = [int(k) & 0xFFFFFFFFFFFFFFFF for k in keys]
        sizes = [float(v) for v in step_size] if isinstance(step_size, (list, tuple)) else [float(step_size)] * K
        if len(sizes) != K:
            raise ValueError(f"{len(sizes)} step sizes for {K} chains")
        self.step_size, self.num_steps = (sizes if self.lead else sizes[0]), int(num_steps)
        self._traj, self._eps = [e * self.num_steps for e in sizes], list(sizes)
        self._searches, self._search_log = [0] * K, [[] for _ in range(K)]
        self.adapt_step_size, self.adapt_mass_matrix = bool(adapt_step_size), bool(adapt_mass_matrix)
        self.launches = self.B = 0
        # the logs of the last run(): one entry per transition, warmup included
        self.eps_log = self.L_log = self.dH_log = self.accept_prob_log = self.accepted_log = None

    def _hmc_sizes(self):
        """(n_params, the lengths of k0_part and of k1_part / p_part) of the nets' shape."""
        nq, ne = C.c_int64(0), C.c_int64(0)
        n = self.sizes("rbnn_hmc_sizes", self.descriptor(_hip.SviTrainNet), nq, ne)
        return n, int(nq.value), int(ne.value)

    def _start(self, batch_size):
        """The end of a subclass's constructor: the workspaces, the state block's step size and dual-averaging centre, the C structs."""
        self._ensure(int(batch_size))
        self._set_state(eps=self._eps, mu=[math.log(10 * e) for e in self._eps])
        self._bind()

    def _chain_struct(self, cls, rows_dim, **more):
        """An HmcChain or HmcLockstep: the chain buffers (attributes of the same names), log / samples ([..., rows, .] with rows at dimension
        rows_dim) and their row counts; more: the pointers that only HmcLockstep has."""
        ch = _hip.fill(cls, {**vars(self), "log": self.log_t, "samples": self.samples_t, **more})
        ch.log_rows = 0 if self.log_t is None else int(self.log_t.shape[rows_dim])
        ch.sample_rows = 0 if self.samples_t is None else int(self.samples_t.shape[rows_dim])
        return ch

    def _st(self):
        return _hip.stream_of(self.W)

    def _read(self, name):
        """One entry of every chain's state block (a device->host synchronisation)."""
        s = self.read_state()
        return [c[name] for c in s] if self.lead else [s[name]]

    # -- the chains -----------------------------------------------------------------------------------------------------------------
    def refresh(self):
        """U and dCE/dW of the chains' current positions (after stage(), or after q_cur was written from outside)."""
        self.W.copy_(self.q_cur)
        self._gradient()
        self._update(_hip.HMC_ENERGY)
        self._decide(_hip.HMC_DECIDE_INIT)
        self._commit(force=True)

    def _length(self, k, eps=None):
        return max(1, int(self._traj[k] / (self._eps[k] if eps is None else eps)))

    def lengths(self):
        return [self._length(k) for k in range(self.K)]

    def transition(self, i, L=None, adapt=False, window_end=False, welford_n=0, sample_row=-1):
        """Transition i of every active chain, chain k with L[k] leapfrog steps (an int: every chain; default: from the host's copies of the
        step sizes).  No device->host synchronisation.  -> the lengths (HmcSampler: its one)"""
        self._draw(i)
        L = self.leapfrog(self.lengths() if L is None else L)
        self._decide(_hip.HMC_DECIDE_TRANSITION, i, adapt, window_end)
        self._commit(False, welford_n, sample_row)
        return L

    def _probe(self, eps, live):
        """One try of the search for the chains in `live`: -> the K values of dH (a frozen chain's is its last one)."""
        self.set_active(live)
        self._set_state(eps=eps)                                         # a frozen chain's entry is the value its block already holds
        self._draw(None)
        for k in range(self.K):
            self._searches[k] += int(live[k])
        self.leapfrog(1)
        self._decide(_hip.HMC_DECIDE_PROBE)
        return self._read("dH")

    def find_reasonable_step_size(self):
        """pyro's search [recalled] from the current step sizes (run() calls it before the first transition and after every warmup window but
        the last, whose dual-averaged exp(xbar) is the sampling phase's step size): one leapfrog step from fresh momentum, direction = +1 if
        -dH > log 0.8 else -1, eps *= 2^direction with new momentum each try until the direction flips; then dual averaging restarts with
        mu = log(10 eps).  All chains probe together, each with its own try counter; a chain whose direction has flipped is frozen
        (active = 0) while the others go on."""
        log08, K = math.log(0.8), self.K
        eps, tries, live = list(self._eps), [[] for _ in range(K)], [True] * K
        dH = self._probe(eps, live)
        direction = [1 if -dH[k] > log08 else -1 for k in range(K)]
        for k in range(K):
            tries[k].append((eps[k], dH[k]))
        while any(live):
            for k in range(K):
                if live[k]:
                    if len(tries[k]) > MAX_SEARCH:
                        raise RuntimeError(f"the HMC step-size search{f' of chain {k}' if self.lead else ''} did not end after {MAX_SEARCH} "
                                           f"tries (last eps {eps[k]:g}, dH {dH[k]:g})")
                    eps[k] = eps[k] * 2.0 ** direction[k]
            dH = self._probe(eps, live)
            for k in range(K):
                if live[k]:
                    tries[k].append((eps[k], dH[k]))
                    live[k] = (1 if -dH[k] > log08 else -1) == direction[k]
        self.set_active(None)
        for k in range(K):
            self._search_log[k].append(tries[k])
        self._eps = eps
        self._set_state(eps=eps, t=0.0, gbar=0.0, xbar=0.0, mu=[math.log(10 * e) for e in eps])

    def _run(self, num_samples, warmup, *batch):
        """`warmup` adapting transitions, then num_samples at fixed step sizes and lengths, of all chains on stage(*batch); then the logs
        (eps_log, L_log, dH_log, accept_prob_log, accepted_log: per chain one entry per transition, warmup included) are read."""
        num_samples, warmup = int(num_samples), int(warmup)
        total, K = warmup + num_samples, self.K
        self.log_t = torch.zeros(*self.lead, max(1, total), _hip.HMC_LOG, dtype=torch.float64, device=self.device)
        self.samples_t = torch.zeros(*self.lead, max(1, num_samples), self.n_params, dtype=torch.float32, device=self.device)
        self._bind()
        self.stage(*batch)
        Ls = [[] for _ in range(K)]

        def note(L):
            for k in range(K):
                Ls[k].append(L[k])

        if warmup > 0 and self.adapt_step_size:
            self.find_reasonable_step_size()
        for (a, b, kind) in windows(warmup):
            mid = kind == "middle" and self.adapt_mass_matrix
            for i in range(a, b):
                last = i == b - 1
                L = self.lengths()
                note(L)
                self.transition(i, L, self.adapt_step_size, last, (i - a + 1) if mid else 0)
                if last and mid:
                    self._window_end(b - a)
                if self.adapt_step_size:
                    self._eps = self._read("eps")                       # warmup's one read per transition: L follows the adapted step sizes
                    if last and b < warmup:                             # the last window's exp(xbar) is the sampling step size: no search
                        self.find_reasonable_step_size()
        self._set_steps(self.lengths())                                   # host -> device, before the sampling phase
        self.sample(warmup, num_samples, note)
        log = self.log = self.log_t[..., :total, :].cpu()                 # the one read of the sampling phase
        self.eps_log, self.dH_log, self.accept_prob_log = log[..., 0].tolist(), log[..., 1].tolist(), log[..., 2].tolist()
        self.accepted_log, self.L_log = (log[..., 3] != 0).tolist(), Ls

    def sample(self, first, num_samples, note=None):
        """num_samples transitions first, first + 1, ... at the fixed step sizes and lengths; row i of every chain's stack = its position after
        transition first + i.  No device->host synchronisation (the lengths are on the device since the end of warmup)."""
        L = self.lengths()
        for i in range(num_samples):
            self.transition(first + i, L, False, False, 0, i)
            if note is not None:
                note(L)


class _OneChain(_Chains):
    """K = 1: one chain through the single-chain entry points ENTRY + "momentum" / "leapfrog_update" / "decide" / "commit" / "window_end" on
    one rbnn_hmc_chain, with scalar / flat public values.  A subclass builds self.net (W = the trajectory's position, grad = dCE/dW) in its
    constructor and supplies _ensure (the workspaces ws_t with "ce", the staged X [Bmax, D] and labels) and _gradient."""
    ENTRY = "rbnn_hmc_"
    eps_host, searches, search_log, trajectory_length = (_view(n, 0) for n in ("_eps", "_searches", "_search_log", "_traj"))

    def _one_chain(self, net, batch_size):
        """The end of the constructor: the chain's key, the net's trajectory pointers, the workspaces, the state block."""
        self.key = self.chain_keys[0]
        self.net = net
        net.W, net.grad = self.W.data_ptr(), self.grad.data_ptr()
        self.Bmax = 0
        self._start(batch_size)

    def _call(self, name, *args):
        _hip.check(getattr(self.k.lib, self.ENTRY + name)(C.byref(self.net), C.byref(self.chain), *args, self._st()), self.ENTRY + name)
        self.launches += 1

    # -- buffers --------------------------------------------------------------------------------------------------------------------
    def _bind(self):
        self.chain = self._chain_struct(_hip.HmcChain, 0)

    def _set_state(self, **kv):
        """Host -> device writes of state-block entries (warmup / set-up only)."""
        for name, v in kv.items():
            self.state[_hip.HMC_ST[name]] = float(v[0] if isinstance(v, list) else v)

    def read_state(self):
        """The state block as a dict (a device->host synchronisation)."""
        s = self.state.tolist()
        return {name: s[i] for name, i in _hip.HMC_ST.items()}

    def set_active(self, mask=None):
        pass                                                              # one chain: always active,

    def _set_steps(self, L):
        pass                                                              # and the host closes its last step (HMC_CLOSE in leapfrog)

    # -- launches -------------------------------------------------------------------------------------------------------------------
    def _update(self, phase):
        self._call("leapfrog_update", phase)

    def _momentum(self, key, draw_id):
        self._call("momentum", C.c_uint64(key & 0xFFFFFFFFFFFFFFFF), C.c_uint32(draw_id & 0xFFFFFFFF))

    def _draw(self, i):
        """The momentum of transition i, or (None) of the search's next probe: a stream of its own, numbered by the try counter."""
        if i is None:
            self._momentum(self.key ^ _hip.HMC_SEARCH_KEY, self._searches[0])
        else:
            self._momentum(self.key, i)

    def _decide(self, mode, transition=0, adapt=False, window_end=False):
        self._call("decide", _hip.ptr(self.ws_t["ce"]), self.B, C.c_uint64(self.key), int(transition), mode, int(adapt), int(window_end))

    def _commit(self, force=False, welford_n=0, sample_row=-1):
        self._call("commit", int(force), int(welford_n), int(sample_row))

    def _window_end(self, n):
        self._call("window_end", n)

    # -- the chain ------------------------------------------------------------------------------------------------------------------
    def stage(self, x, labels):
        """The batch the potential is taken over (x [B, ...], labels int [B]) and the potential / gradient at the current position."""
        B = int(x.shape[0])
        self._ensure(B)
        self.B = B
        self.X[:B].copy_(x.reshape(B, -1))
        self.labels[:B].copy_(labels.reshape(B))
        self.refresh()

    def leapfrog(self, n, fused=True):
        """n leapfrog steps (or [n], as the driver passes lengths) from (q_cur, r) at the state block's step size; the end point is left in
        self.W / self.r / self.grad and its K' and 1/2 sum q'^2 in the partial sums.  fused=False: the plain half kick / drift / gradient /
        half kick sequence the fused updates restate.  -> n"""
        n = n[0] if isinstance(n, list) else n
        if fused:
            self._update(_hip.HMC_OPEN)
            for s in range(n):
                self._gradient()
                self._update(_hip.HMC_MID if s + 1 < n else _hip.HMC_CLOSE)
            return n
        self.W.copy_(self.q_cur)
        self.grad.copy_(self.g_cur)
        for s in range(n):
            self._update(_hip.HMC_KICK)
            self._update(_hip.HMC_DRIFT)
            self._gradient()
            self._update(_hip.HMC_KICK)
        self._update(_hip.HMC_ENERGY)
        return n

    def length(self, eps=None):
        return self._length(0, eps)

    def run(self, x, labels, num_samples, warmup):
        """One chain on the batch: `warmup` adapting transitions, then num_samples at fixed step size and L.  Returns the sample stack as a dict
        state_dict key -> [num_samples, ...] (device tensors); the logs (eps_log, L_log, dH_log, accept_prob_log, accepted_log: one entry per
        transition, warmup included) and the final m_inv stay on the sampler."""
        self._run(num_samples, warmup, x, labels)
        self.L_log = self.L_log[0]
        return self.unflat(self.samples_t[:int(num_samples)])


class HmcSampler(_OneChain):
    """Device-resident state of one HMC chain over an fc / fc2 net: the trajectory's position / dCE/dW (an rbnn_svi_train_net's W / grad), the
    chain's cached position and gradient, momentum, the diagonal inverse mass, Welford's mean / M2, the fp64 state block, the per-transition
    log and the sample stack.  `launches` counts kernel launches by the entry points' documented launch counts."""

    def __init__(self, arch, activation, input_shape, n_classes, q0, step_size, num_steps, device, key, adapt_step_size=True,
                 adapt_mass_matrix=True, batch_size=128):
        require_gpu_fc("HMC", arch, device)
        super().__init__(arch, activation, input_shape, n_classes, [q0], float(step_size), num_steps, device, [key], adapt_step_size,
                         adapt_mass_matrix, None)
        self._one_chain(self.descriptor(_hip.SviTrainNet), batch_size)

    def _ensure(self, B):
        if B <= self.Bmax:
            return
        self.ws_t = train_workspace(self.arch, B, self.H, self.device)
        self.ws = _hip.fill(_hip.SviTrainWs, self.ws_t)
        self.staging(B)

    def _gradient(self):
        """dCE/dW and the per-point CE at self.W: the training forward (fc 2 launches, fc2 4) + the weight gradients (1)."""
        lib, net = self.k.lib, C.byref(self.net)
        _hip.check(lib.rbnn_svi_train_forward(net, _hip.ptr(self.X), self.D, self.B, _hip.ptr(self.labels), C.byref(self.ws), self._st()),
                   "rbnn_svi_train_forward")
        _hip.check(lib.rbnn_svi_weight_grads(net, _hip.ptr(self.X), self.D, self.B, C.byref(self.ws), self._st()), "rbnn_svi_weight_grads")
        self.launches += self.fwd_launches + 1


class _LockstepChains(_Chains):
    """What the classes that run K chains behind every launch share (LockstepHmc; conv_hmc.ConvLockstepHmc): one rbnn_hmc_lockstep chain block
    with the per-chain keys, lengths, draw ids and activity on the device, the state block's accessors, and the momentum / update / commit /
    window-end launches through the entry points ENTRY + their names.  A subclass checks its own arguments (refuse_bad_chains among them),
    calls _Chains' constructor with members = K and then _lockstep(batch_size), and supplies _bind (self.net, then _bind_chain), _ensure,
    _gradient, _decide, stage() and run()."""
    ENTRY = "rbnn_hmc_lockstep_"
    eps_host, searches, search_log, trajectory_length = (_view(n) for n in ("_eps", "_searches", "_search_log", "_traj"))
    set_data = set_data
    length = _Chains._length

    @staticmethod
    def refuse_bad_chains(who, q0s, keys):
        """The refusals of a chain count, before the library is loaded."""
        if len(q0s) < 1 or len(keys) != len(q0s):
            raise ValueError(f"{who} needs one key per chain and at least one chain: {len(q0s)} start positions, {len(keys)} keys")
        if len(q0s) > 65535:
            raise ValueError(f"at most 65535 chains run in lockstep (the chain is a grid dimension), not {len(q0s)}")

    def _lockstep(self, batch_size):
        """The end of a subclass's constructor: the per-chain device values, then _Chains._start."""
        K, dev = self.K, self.device
        self.keys_t = keys_tensor(self.chain_keys, dev)
        self.steps_t = torch.ones(K, dtype=torch.int32, device=dev)
        self.draw_ids_t = torch.zeros(K, dtype=torch.int32, device=dev)
        self.active_t = torch.ones(K, dtype=torch.int32, device=dev)
        self.active = None                                               # None: every chain; else the host's copy of active_t
        self._steps_host = [1] * K
        self.X = self.labels = self.rows_t = None
        self._start(batch_size)

    def _bind_chain(self, **more):
        """self.chain: the rbnn_hmc_lockstep of the chain buffers (more: buffers that are not attributes of their field's name)."""
        ch = self._chain_struct(_hip.HmcLockstep, 1, keys=self.keys_t, steps=self.steps_t, active=None if self.active is None else self.active_t,
                                **more)
        ch.chain_stride, ch.qpart_stride, ch.epart_stride = self.n_params, self.n_qpart, self.n_epart
        self.chain = ch

    def _call(self, name, *args):
        _hip.check(getattr(self.k.lib, self.ENTRY + name)(C.byref(self.net), C.byref(self.chain), *args, self._st()), self.ENTRY + name)
        self.launches += 1

    def _set_state(self, **kv):
        """Host -> device writes of state-block entries (warmup / set-up only): one value for every chain, or one per chain."""
        for name, v in kv.items():
            if isinstance(v, (list, tuple)):
                self.state[:, _hip.HMC_ST[name]] = torch.tensor([float(e) for e in v], dtype=torch.float64)
            else:
                self.state[:, _hip.HMC_ST[name]] = float(v)

    def read_state(self):
        """One dict per chain (a device->host synchronisation)."""
        return [{name: row[i] for name, i in _hip.HMC_ST.items()} for row in self.state.tolist()]

    def set_active(self, mask=None):
        """mask: K truth values (host -> device), or None for all chains.  A chain that is not active is neither read nor written by the
        momentum, update, decision, commit and window-end launches that follow."""
        if mask is None or all(mask):
            self.active = None
        else:
            self.active = [bool(m) for m in mask]
            self.active_t.copy_(torch.tensor([int(m) for m in self.active], dtype=torch.int32))
        self.chain.active = None if self.active is None else self.active_t.data_ptr()

    def _set_steps(self, Ls):
        if list(Ls) != self._steps_host:                                  # host -> device, only when a length changed
            self.steps_t.copy_(torch.tensor([int(v) for v in Ls], dtype=torch.int32))
            self._steps_host = list(Ls)

    # -- launches -------------------------------------------------------------------------------------------------------------------
    def _update(self, phase, step=-1):
        self._call("update", phase, step)

    def _momentum(self, key_xor, draw_id, per_chain=False):
        self._call("momentum", C.c_uint64(key_xor), C.c_uint32(draw_id & 0xFFFFFFFF), _hip.ptr(self.draw_ids_t) if per_chain else None)

    def _draw(self, i):
        """The momenta of transition i, or (None) of the search's next probe: every chain's try counter goes to the device first."""
        if i is None:
            self.draw_ids_t.copy_(torch.tensor(self._searches, dtype=torch.int32))
            self._momentum(_hip.HMC_SEARCH_KEY, 0, per_chain=True)
        else:
            self._momentum(0, i)

    def _commit(self, force=False, welford_n=0, sample_row=-1):
        self._call("commit", int(force), int(welford_n), int(sample_row))

    def _window_end(self, n):
        self._call("window_end", n)

    def leapfrog(self, Ls):
        """Chain k takes Ls[k] leapfrog steps (an int: every chain) from (q_cur, r) at its own step size: max(Ls) gradient + update launches,
        the update of step s closing the chains whose length is s + 1 (steps_t).  -> the K lengths"""
        Ls = [int(Ls)] * self.K if isinstance(Ls, int) else [int(v) for v in Ls]
        self._set_steps(Ls)
        self._update(_hip.HMC_OPEN)
        for s in range(max(Ls)):
            self._gradient()
            self._update(_hip.HMC_MID, s)
        return Ls


class LockstepHmc(_LockstepChains):
    """K independent chains over nets of ONE shape in lockstep: every launch covers all chains, so a transition costs the launches of a single
    chain whatever K is.  Each chain has its own key, start position, step size, mass matrix, state block, log and sample stack, and may have
    its own batch (rows / counts into resident data); warmup, the number of samples, num_steps and the adapt flags are shared.  Chain k is
    bit-identical to HmcSampler(…, q0s[k], …, keys[k]) alone on its batch: sample stack, log, m_inv, q_cur, g_cur, state, L_log, search tries.

    Adapted step sizes differ, so the chains' trajectory lengths L_k do: the host issues max_k L_k leapfrog steps and the update launch of
    step s closes the chains with L_k == s + 1 and skips those behind it (their forward / gradient launches still run, on a position that
    no longer moves).  The step-size search probes all chains together and freezes a chain whose direction has flipped (`active`).
    `launches` counts kernel launches as HmcSampler does."""

    def __init__(self, arch, activation, input_shape, n_classes, q0s, step_size, num_steps, device, keys, adapt_step_size=True,
                 adapt_mass_matrix=True, batch_size=128):
        require_gpu_fc("HMC", arch, device)
        q0s, keys = list(q0s), list(keys)
        self.refuse_bad_chains("LockstepHmc", q0s, keys)
        super().__init__(arch, activation, input_shape, n_classes, q0s, step_size, num_steps, device, keys, adapt_step_size, adapt_mass_matrix,
                         len(q0s))
        self.cap = 0
        self.counts_t = None
        self._lockstep(batch_size)

    # -- buffers --------------------------------------------------------------------------------------------------------------------
    def _bind(self):
        net = self.descriptor(_hip.NnTrainNet, self.K)
        net.P, net.grad, net.member_stride = self.W.data_ptr(), self.grad.data_ptr(), self.n_params
        self.net = net
        self._bind_chain()

    def _ensure(self, B):
        """Workspaces for K x B points (packed [K, B, .] for the call's B)."""
        if self.K * B <= self.cap:
            return
        self.ws_t = train_workspace(self.arch, self.K * B, self.H, self.device)
        self.ws_t["correct"] = torch.zeros(self.K * B, dtype=torch.int32, device=self.device)
        self.ws = _hip.fill(_hip.NnTrainWs, self.ws_t)
        self.cap = self.K * B

    # -- launches -------------------------------------------------------------------------------------------------------------------
    def _gradient(self):
        _hip.check(self.k.lib.rbnn_hmc_lockstep_gradient(C.byref(self.net), _hip.ptr(self.X), self.D, int(self.X.shape[0]), _hip.ptr(self.labels),
                                                         _hip.ptr(self.rows_t), _hip.ptr(self.counts_t), self.B, C.byref(self.ws), self._st()),
                   "rbnn_hmc_lockstep_gradient")
        self.launches += self.fwd_launches + 1

    def _decide(self, mode, transition=0, adapt=False, window_end=False):
        self._call("decide", _hip.ptr(self.ws_t["ce"]), _hip.ptr(self.counts_t), self.B, int(transition), mode, int(adapt), int(window_end))

    # -- data -----------------------------------------------------------------------------------------------------------------------
    def stage(self, rows=None, counts=None):
        """The chains' batches — rows [K, B] int32 into the resident data with counts [K] (None: B) of them valid per chain, or rows None: the
        whole resident data for every chain — and the potential / gradient at the current positions."""
        if self.X is None:
            raise ValueError("set_data(x, labels) first")
        if rows is None:
            self.rows_t, self.B = None, int(self.X.shape[0])
        else:
            rows = torch.as_tensor(rows)
            if rows.dim() != 2 or rows.shape[0] != self.K:
                raise ValueError(f"rows must be [{self.K}, B], not {tuple(rows.shape)}")
            self.rows_t, self.B = rows.to(self.device, torch.int32).contiguous(), int(rows.shape[1])
        if counts is None:
            self.counts_t = None
        else:
            counts = [int(c) for c in (counts.tolist() if torch.is_tensor(counts) else counts)]
            if len(counts) != self.K or min(counts) < 1 or max(counts) > self.B:
                raise ValueError(f"counts must be {self.K} values in [1, {self.B}], not {counts}")
            self.counts_t = torch.tensor(counts, dtype=torch.int32).to(self.device)
        self._ensure(self.B)
        self.refresh()

    def run(self, x=None, labels=None, num_samples=0, warmup=0, rows=None, counts=None):
        """`warmup` adapting transitions, then num_samples at fixed step sizes and lengths, of all chains.  run(x, labels, …): every chain on
        that batch; run(rows=[K, B], counts=[K] or None, …): chain k on rows[k, :counts[k]] of the resident data (set_data).  Returns one
        stack dict per chain (state_dict key -> [num_samples, ...], device tensors); eps_log / L_log / dH_log / accept_prob_log / accepted_log /
        search_log are lists with one entry per chain, m_inv is [K, n_params]."""
        if x is not None:
            if rows is not None:
                raise ValueError("run() takes a batch (x, labels) or rows into the resident data, not both")
            self.set_data(x, labels)
        self._run(num_samples, warmup, rows, counts)
        return [self.unflat(self.samples_t[k, :int(num_samples)]) for k in range(self.K)]


def split_r_hat(values):
    """Split-R-hat (Gelman et al., BDA3 section 11.4) of `values` [K, n]: each chain is halved (the middle draw of an odd n is dropped), giving
    m = 2K sequences of length h = n // 2; with W the mean of their variances and B = h var(their means),
    R-hat = sqrt(((h - 1) / h W + B / h) / W).  Host only, fp64.  Constant sequences (W = 0): 1.0 if their means agree too, else inf.
    The usual `values`: each chain's logged U_new over the sampling phase."""
    v = torch.as_tensor(values, dtype=torch.float64)
    if v.dim() != 2 or v.shape[1] < 4:
        raise ValueError(f"split_r_hat needs [K, n] with n >= 4, not {tuple(v.shape)}")
    h = v.shape[1] // 2
    halves = torch.cat([v[:, :h], v[:, v.shape[1] - h:]], 0)
    W = float(halves.var(dim=1, unbiased=True).mean())
    Bh = float(halves.mean(dim=1).var(unbiased=True))                   # B / h
    if W == 0.0:
        return 1.0 if Bh == 0.0 else math.inf
    return math.sqrt(((h - 1) / h * W + Bh) / W)
