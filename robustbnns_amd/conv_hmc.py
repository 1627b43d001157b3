"""HMC posteriors of conv nets of the 1x28x28 geometry on the GPU — `_train_hmc` (model_bnn.py:260-301, which is architecture-blind) for the
reference's `conv` architecture (model_nn.py:93-106), reached through BNN.train_hmc_conv.

ConvHmcSampler is hmc.HmcSampler's chain (hmc._Chains' algorithm: transition, step-size search, warmup windows, sampling, logs; its module
docstring and tests/hmc_restate.py have the formulas) with the conv kernels under it:

  * position     q = the flat parameter buffer of conv_train.ConvNnTrainer (state_dict order model.0 / model.3 / model.7, unpadded);
                 U(q) = sum_b CE(z_b(q), y_b) + 1/2 sum q^2, grad U = dCE/dW + q;
  * gradient     dCE/dW and the per-point CE at the trajectory's position: rbnn_conv_svi_train_forward (3 + 1 launches) and
                 rbnn_conv_svi_weight_grads (7 launches) of csrc/rbnn_conv_train.hip, the summed cross-entropy;
  * the rest     momentum, the fused leapfrog updates, the decision, the commit and the window end are the single chain's kernels of
                 csrc/rbnn_hmc.hip on the conv layout (rbnn_conv_hmc_*): element e of tensor i draws component e % 4 of the Philox block with
                 counter (e / 4, i, 0, draw id), the conv SVI draw's counter layout.

A leapfrog step is 4 + 7 + 1 = 12 launches, a transition with L steps 1 + 1 + 12 L + 1 + 1; one stream, no atomics; warmup reads the state
block once per transition, sampling makes no device->host synchronisation.  Two runs with one key are bit-identical.

ConvLockstepHmc runs K such chains of one net shape with every launch covering all of them (BNN.train_hmc_conv(num_chains=K)): it is
hmc.LockstepHmc's host side (hmc._LockstepChains) on the rbnn_conv_hmc_chains_* entry points.  The chains are the members of the conv
ensemble's forward and weight gradients (4 + 7 launches whatever K is), so the positions, gradients and every per-parameter chain buffer are
TENSOR-MAJOR — six blocks [K, size of tensor] — and the four element-wise lockstep kernels of csrc/rbnn_hmc.hip, the ones hmc.LockstepHmc
launches, run the single chain's bodies on that layout through their tensor-major view; the partial sums, state blocks, logs and sample
stacks stay chain-major.  Chain k is bit-identical to ConvHmcSampler running it
alone; hmc.split_r_hat is the convergence figure that goes with several chains.  conv_hmc_chains_group says how many chains' workspaces fit
the conv workspace budget.

What stays refused: the 3x32x32 geometry, CPU devices.
"""
import ctypes as C

import torch

from . import _hip
from .conv_train import CONV_KEYS, check_conv_trainable, conv_group, conv_net, conv_workspace, flat_of as chain_flat, tensor_major
from .hmc import _LockstepChains, _OneChain


class ConvHmcSampler(_OneChain):
    """Device-resident state of one HMC chain over a conv net of the 1x28x28 geometry: HmcSampler's buffers and public surface (stage, refresh,
    leapfrog(n, fused), transition, find_reasonable_step_size, run, the logs, m_inv, read_state), the trajectory's position / dCE/dW being an
    rbnn_conv_svi_train_net's W / grad and the workspaces an rbnn_conv_train_ws for up to Bmax points (grown, never shrunk).  `launches`
    counts kernel launches by the entry points' documented launch counts."""
    ENTRY = "rbnn_conv_hmc_"
    PARAM_KEYS = CONV_KEYS

    def __init__(self, activation, input_shape, n_classes, q0, step_size, num_steps, device, key, adapt_step_size=True, adapt_mass_matrix=True,
                 batch_size=128):
        check_conv_trainable(input_shape, device)
        super().__init__("conv", activation, input_shape, n_classes, [q0], float(step_size), num_steps, device, [key], adapt_step_size,
                         adapt_mass_matrix, None)
        self._one_chain(conv_net(_hip.ConvSviTrainNet, activation, self.H, self.C), batch_size)

    def _hmc_sizes(self):
        nq, ne = C.c_int64(0), C.c_int64(0)
        n = self.sizes("rbnn_conv_hmc_sizes", conv_net(_hip.ConvSviTrainNet, self.activation, self.H, self.C), nq, ne)
        return n, int(nq.value), int(ne.value)

    def _ensure(self, B):
        if B <= self.Bmax:
            return
        sz = _hip.ConvTrainBytes()
        _hip.check(self.k.lib.rbnn_conv_svi_train_sizes(C.byref(self.net), B, None, C.byref(sz)), "rbnn_conv_svi_train_sizes")
        self.ws_t, self.ws = conv_workspace(sz, _hip.CONV_TRAIN_WS_KEYS, _hip.ConvTrainWs, self.device)
        self.staging(B)

    def _gradient(self):
        """dCE/dW and the per-point CE at self.W: the conv training forward (3 + 1 launches) + the conv weight gradients (7)."""
        lib, net = self.k.lib, C.byref(self.net)
        _hip.check(lib.rbnn_conv_svi_train_forward(net, _hip.ptr(self.X), self.D, _hip.ptr(self.labels), self.B, C.byref(self.ws), self._st()),
                   "rbnn_conv_svi_train_forward")
        _hip.check(lib.rbnn_conv_svi_weight_grads(net, _hip.ptr(self.X), self.D, self.B, C.byref(self.ws), self._st()),
                   "rbnn_conv_svi_weight_grads")
        self.launches += 4 + 7


# ---------------------------------------------------------------------------------------------------------------------------------------
# K chains behind every launch
# ---------------------------------------------------------------------------------------------------------------------------------------
# The per-parameter buffers of K chains, [K * n_params] in conv_train's tensor-major layout: tensor_major(flat [K, n_params], blocks) makes one,
# chain_flat(buf, k, blocks, K) (conv_train.flat_of) gives chain k's values back as a flat [n_params] tensor in state_dict order.
TENSOR_MAJOR = ("W", "grad", "q_cur", "g_cur", "r", "m_inv", "w_mean", "w_m2")


class ConvLockstepHmc(_LockstepChains):
    """K independent chains over conv nets of ONE shape (activation, hidden size, classes; the 1x28x28 geometry) with every launch covering
    all of them, the conv counterpart of hmc.LockstepHmc: a transition costs the launches of a single chain (1 + 1 + 12 L + 1 + 1, L the
    longest trajectory) whatever K is.  Each chain has its own key, start position, step size (one value or K), mass matrix, state block, log
    and sample stack, and may have its own rows of the resident data (set_data; stage(rows [K, B])); all chains of a batch share its point
    count B (there are no counts), warmup, the number of samples, num_steps and the adapt flags.  Chain k is bit-identical to
    ConvHmcSampler(…, q0s[k], …, keys[k]) alone on data[rows[k]]: sample stack, log, m_inv, q_cur, g_cur, state, L_log, search tries.

    The per-parameter buffers (TENSOR_MAJOR) are [K * n_params], six blocks [K, size of tensor] in state_dict order — an implementation
    detail: chain_flat(buf, k) gives chain k's values as a flat [n_params] tensor in state_dict order, m_inv reads as [K, n_params]
    chain-major, and the sample stacks are [K, rows, n_params] with every row flat, as the single chain's.  stage() gathers the chains'
    batches once (1 launch); the gradient of a leapfrog step works on the staged copy.  `launches` counts kernel launches by the entry
    points' documented launch counts."""
    ENTRY = "rbnn_conv_hmc_chains_"
    PARAM_KEYS = CONV_KEYS

    def __init__(self, activation, input_shape, n_classes, q0s, step_size, num_steps, device, keys, adapt_step_size=True, adapt_mass_matrix=True,
                 batch_size=128):
        check_conv_trainable(input_shape, device)
        q0s, keys = list(q0s), list(keys)
        self.refuse_bad_chains("ConvLockstepHmc", q0s, keys)
        super().__init__("conv", activation, input_shape, n_classes, q0s, step_size, num_steps, device, keys, adapt_step_size, adapt_mass_matrix,
                         len(q0s))
        self.q_cur = tensor_major(self.q_cur, self.blocks)              # the K flat start positions, converted once
        for name in ("W", "grad", "g_cur", "r", "w_mean", "w_m2"):      # zeros: one flat buffer each
            setattr(self, name, getattr(self, name).reshape(-1))
        self.Bmax = 0
        self._lockstep(batch_size)

    @property
    def m_inv(self):
        """The diagonal inverse masses, [K, n_params] chain-major (a copy)."""
        return torch.stack([chain_flat(self._m_inv, k, self.blocks, self.K) for k in range(self.K)])

    @m_inv.setter
    def m_inv(self, v):
        v = tensor_major(v.reshape(self.K, -1), self.blocks)
        if "_m_inv" in vars(self):
            self._m_inv.copy_(v)                                        # in place: the chain block keeps pointing at it
        else:
            self._m_inv = v.to(self.device)

    def chain_flat(self, buf, k):
        """Chain k's values of one of the tensor-major buffers ("m_inv": self._m_inv) as a flat [n_params] tensor in state_dict order."""
        return chain_flat(buf, k, self.blocks, self.K)

    def _net(self):
        """A fresh descriptor of the K chains' nets, every pointer NULL (the sizes queries run before self.net is bound)."""
        return conv_net(_hip.ConvHmcChainsNet, self.activation, self.H, self.C, n_chains=self.K)

    def _hmc_sizes(self):
        nq, ne = C.c_int64(0), C.c_int64(0)
        net = self._net()
        n = int(self.k.lib.rbnn_conv_hmc_chains_sizes(C.byref(net), 0, C.byref(nq), C.byref(ne), None))     # no workspace sizes: no point count
        _hip.check(min(n, 0), "rbnn_conv_hmc_chains_sizes")
        return n, int(nq.value), int(ne.value)

    # -- buffers --------------------------------------------------------------------------------------------------------------------
    def _bind(self):
        net = self._net()
        net.W, net.grad = self.W.data_ptr(), self.grad.data_ptr()
        self.net = net
        self._bind_chain(m_inv=self._m_inv)

    def _ensure(self, B):
        """Workspaces for batches of up to B points per chain (grown, never shrunk; a call packs them [K, its own B, .])."""
        if B <= self.Bmax:
            return
        sz = _hip.ConvEnsBytes()
        _hip.check(min(int(self.k.lib.rbnn_conv_hmc_chains_sizes(C.byref(self._net()), B, None, None, C.byref(sz))), 0), "rbnn_conv_hmc_chains_sizes")
        self.ws_t, self.ws = conv_workspace(sz, _hip.CONV_ENS_WS_KEYS, _hip.ConvEnsWs, self.device)
        self.Bmax = B

    # -- launches -------------------------------------------------------------------------------------------------------------------
    def _gradient(self):
        """dCE/dW and the per-point CE of every chain at self.W on the staged batches: the members' forward (3 + 1 launches) + their weight
        gradients (7)."""
        _hip.check(self.k.lib.rbnn_conv_hmc_chains_gradient(C.byref(self.net), self.B, C.byref(self.ws), self._st()), "rbnn_conv_hmc_chains_gradient")
        self.launches += 4 + 7

    def _decide(self, mode, transition=0, adapt=False, window_end=False):
        self._call("decide", _hip.ptr(self.ws_t["ce"]), self.B, int(transition), mode, int(adapt), int(window_end))

    # -- data -----------------------------------------------------------------------------------------------------------------------
    def stage(self, rows=None):
        """The chains' batches — rows [K, B] int32 into the resident data, or None: the whole resident data for every chain — gathered into
        the workspace (1 launch), and the potential / gradient at the current positions."""
        if self.X is None:
            raise ValueError("set_data(x, labels) first")
        n_rows = int(self.X.shape[0])
        if rows is None:
            rows = torch.arange(n_rows, dtype=torch.int32).repeat(self.K, 1)
        else:
            rows = torch.as_tensor(rows)
            if rows.dim() != 2 or int(rows.shape[0]) != self.K or int(rows.shape[1]) < 1:
                raise ValueError(f"rows must be [{self.K}, B] with B >= 1, not {tuple(rows.shape)}")
        self.rows_t, self.B = rows.to(self.device, torch.int32).contiguous(), int(rows.shape[1])
        self._ensure(self.B)
        _hip.check(self.k.lib.rbnn_conv_hmc_chains_stage(C.byref(self.net), _hip.ptr(self.X), int(self.X.stride(0)), n_rows, _hip.ptr(self.labels),
                                                         _hip.ptr(self.rows_t), self.B, C.byref(self.ws), self._st()), "rbnn_conv_hmc_chains_stage")
        self.launches += 1
        self.refresh()

    def run(self, x=None, labels=None, num_samples=0, warmup=0, rows=None):
        """`warmup` adapting transitions, then num_samples at fixed step sizes and lengths, of all chains.  run(x, labels, …): every chain on
        that batch; run(rows=[K, B], …): chain k on rows[k] of the resident data (set_data).  Returns one stack dict per chain (state_dict
        key -> [num_samples, ...], device tensors); eps_log / L_log / dH_log / accept_prob_log / accepted_log / search_log are lists with one
        entry per chain, m_inv is [K, n_params]."""
        if x is not None:
            if rows is not None:
                raise ValueError("run() takes a batch (x, labels) or rows into the resident data, not both")
            self.set_data(x, labels)
        self._run(num_samples, warmup, rows)
        return [self.unflat(self.samples_t[k, :int(num_samples)]) for k in range(self.K)]


def conv_hmc_chains_group(activation, hidden, n_classes, n_chains, batch_size, budget_gb=None):
    """The largest number of chains (<= n_chains, >= 1) whose packed workspaces for batch_size points and eight per-parameter buffers fit the
    conv workspace budget (conv_train.conv_group), by rbnn_conv_hmc_chains_sizes for one chain.  Never more than a launch takes: 65535
    chains, 2^22 packed points.  (The logs and the sample stacks are not counted: [warmup + samples, 8] doubles and [samples, n_params]
    floats per chain.)"""
    out = _hip.ConvEnsBytes()
    net = conv_net(_hip.ConvHmcChainsNet, activation, hidden, n_classes, n_chains=1)
    _hip.check(min(int(_hip.load().rbnn_conv_hmc_chains_sizes(C.byref(net), int(batch_size), None, None, C.byref(out))), 0), "rbnn_conv_hmc_chains_sizes")
    per_chain = sum(getattr(out, k) for k in _hip.CONV_ENS_WS_KEYS) + len(TENSOR_MAJOR) * 4 * out.n_params
    return conv_group(per_chain, n_chains, budget_gb, 65535, (1 << 22) // int(batch_size))
