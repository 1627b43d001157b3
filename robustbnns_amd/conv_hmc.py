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

What stays refused: conv chains in lockstep (BNN.train_hmc_conv has no num_chains), the 3x32x32 geometry, CPU devices.
"""
import ctypes as C

import torch

from . import _hip
from .conv_train import _WS_DTYPES, CONV_KEYS, check_conv_trainable
from .hmc import _OneChain


def _conv_net(activation, hidden, n_classes):
    net = _hip.ConvSviTrainNet()
    net.activation, net.in_channels, net.in_width = _hip.ACTIVATIONS[activation], 1, 28
    net.hidden, net.n_classes = int(hidden), int(n_classes)
    return net


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
        self._one_chain(_conv_net(activation, self.H, self.C), batch_size)

    def _hmc_sizes(self):
        nq, ne = C.c_int64(0), C.c_int64(0)
        n = self.sizes("rbnn_conv_hmc_sizes", _conv_net(self.activation, self.H, self.C), nq, ne)
        return n, int(nq.value), int(ne.value)

    def _ensure(self, B):
        if B <= self.Bmax:
            return
        sz = _hip.ConvTrainBytes()
        _hip.check(self.k.lib.rbnn_conv_svi_train_sizes(C.byref(self.net), B, None, C.byref(sz)), "rbnn_conv_svi_train_sizes")
        self.ws_t = {}
        for k in _hip.CONV_TRAIN_WS_KEYS:
            dt = _WS_DTYPES.get(k, torch.float32)
            self.ws_t[k] = torch.zeros(getattr(sz, k) // torch.empty(0, dtype=dt).element_size(), dtype=dt, device=self.device)
        self.ws = _hip.fill(_hip.ConvTrainWs, self.ws_t)
        self.X = torch.zeros(B, self.D, dtype=torch.float32, device=self.device)
        self.labels = torch.zeros(B, dtype=torch.int32, device=self.device)
        self.Bmax = B

    def _gradient(self):
        """dCE/dW and the per-point CE at self.W: the conv training forward (3 + 1 launches) + the conv weight gradients (7)."""
        lib, net = self.k.lib, C.byref(self.net)
        _hip.check(lib.rbnn_conv_svi_train_forward(net, _hip.ptr(self.X), self.D, _hip.ptr(self.labels), self.B, C.byref(self.ws), self._st()),
                   "rbnn_conv_svi_train_forward")
        _hip.check(lib.rbnn_conv_svi_weight_grads(net, _hip.ptr(self.X), self.D, self.B, C.byref(self.ws), self._st()),
                   "rbnn_conv_svi_weight_grads")
        self.launches += 4 + 7
