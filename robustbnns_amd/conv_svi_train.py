"""SVI training of ONE conv guide of the 1x28x28 geometry on the GPU — `_train_svi`'s algorithm (model_bnn.py:105-136, :303-365) for the
reference's `conv` architecture (model_nn.py:93-106), reached through BNN.train_conv.

One `ConvSviTrainer.step(x, labels)` is one `svi.step` of SVI(model, guide, pyro.optim.Adam({"lr": lr}), TraceMeanField_ELBO()), the step
svi_train.SviTrainer makes for fc / fc2 (its docstring has the formulas), around the conv kernels:

  * draw      W = loc + sigma * eps for the six tensors, rbnn_svi_draw_flat's generator at sample 0 (1 launch);
  * forward   the exact fp32-MFMA conv forward on W and the head with the SUMMED cross-entropy (3 + 1 launches);
  * gradients dCE/dW of all six tensors, the kernels of the deterministic conv trainer (7 launches);
  * Adam + KL rbnn_svi_step.hpp's kernel over the six tensors: eps regenerated, loc / raw / sigma / moments, the KL partial sums (1 launch);
  * accuracy  the reference's forward(x_batch, n_samples=10): 10 weight sets drawn from the LIVE loc / sigma into a resident
              conv.ConvStackedPosterior under key ^ ACC_KEY and draw id = step, rbnn_conv_forward on the exact path (no image is built),
              rbnn_reduce_samples (1 + 3 + 1 launches);
  * finalize  rbnn_svi_train_finalize: the step's loss, its running sum, the correct predictions (1 launch).

14 launches a step without the accuracy forward, 19 with it (csrc/rbnn_conv_train.hip), plus the two torch copies that stage the batch; one
stream, no atomics, no device->host synchronisation: two runs are bit-identical.  ConvSviTrainer stands on flat_params.FlatNets with conv's key
list and offers SviTrainer's surface (gradients, step, begin_epoch, epoch_totals, params); the epoch loop is BNN's, shared with BNN.train.

What stays refused: conv SVI guides in lockstep, the 3x32x32 geometry, CPU devices.  HMC posteriors of conv nets are sampled by
conv_hmc.ConvHmcSampler (BNN.train_hmc_conv), on the forward and weight gradients this step runs; conv chains in lockstep stay refused too.
"""
import ctypes as C

import torch
import torch.nn.functional as F

from . import _hip
from .conv import ConvStackedPosterior, ConvSviGuide
from .conv_train import _WS_DTYPES, CONV_KEYS, check_conv_trainable
from .flat_params import FlatNets, flatten
from .svi_train import ACC_KEY, ACC_SAMPLES, ADAM_EPS, BETAS


class _LiveConvGuide:
    """What ConvStackedPosterior.redraw reads of a conv.ConvSviGuide (loc, sigma, the tensor ids), over views of the trainer's flat loc / sigma
    buffers: no copy, no sync, and every accuracy draw sees the current parameters.  No triple / split image is built from it, so
    ConvSviGuide's bounds are not needed."""
    TENSOR_IDS = ConvSviGuide.TENSOR_IDS

    def __init__(self, loc, sigma, device):
        self.loc, self.sigma, self.device = loc, sigma, torch.device(device)


class ConvSviTrainer(FlatNets):
    """Device-resident SVI state of one conv guide: flat loc / raw / sigma / Adam moments, the one-sample weight buffer and its gradient
    [n_params] in state_dict order, the workspaces for up to Bmax points, the resident S = 10 stack of the accuracy forward and a device-side
    accumulator stats [3] = [step loss, sum of step losses, correct predictions]."""

    def __init__(self, activation, input_shape, n_classes, loc, raw, lr, device, key, batch_size=128):
        check_conv_trainable(input_shape, device)
        super().__init__("conv", activation, input_shape, n_classes, loc, device, keys=CONV_KEYS)
        dev, z = self.device, self.zeros
        self.Dp = self.D
        net = _hip.ConvSviTrainNet()
        net.activation, net.in_channels, net.in_width = _hip.ACTIVATIONS[activation], 1, 28
        net.hidden, net.n_classes = self.H, self.C
        self.net = net
        sz, self.n_partials = self._sizes(1)
        n = self.n_params = int(sz.n_params)
        self.loc, self.raw = flatten(loc, self.keys).to(dev), flatten(raw, self.keys).to(dev)
        assert self.loc.numel() == n, (self.loc.numel(), n)
        self.sigma = F.softplus(self.raw)
        self.m_loc, self.v_loc, self.m_raw, self.v_raw, self.W, self.grad = z(n), z(n), z(n), z(n), z(n), z(n)
        _hip.fill(net, self)
        self.kl_part = z(self.n_partials)
        self.stats = torch.zeros(3, dtype=torch.float64, device=dev)
        self.lr, self.key, self.t = float(lr), int(key) & 0xFFFFFFFFFFFFFFFF, 0
        self.guide = _LiveConvGuide(self.unflat(self.loc), self.unflat(self.sigma), dev)
        self.acc_post = ConvStackedPosterior.for_guide(self.guide, activation, self.input_shape, self.C, self.H, ACC_SAMPLES)
        self.Bmax = 0
        self._ensure(int(batch_size))

    def _sizes(self, B):
        """(rbnn_conv_train_bytes for B points, n_partials)."""
        out, n_part = _hip.ConvTrainBytes(), C.c_int64(0)
        _hip.check(self.k.lib.rbnn_conv_svi_train_sizes(C.byref(self.net), B, C.byref(n_part), C.byref(out)), "rbnn_conv_svi_train_sizes")
        return out, int(n_part.value)

    def _ensure(self, B):
        """Workspaces for batches of up to B points (grown, never shrunk: a short last batch reuses them)."""
        if B <= self.Bmax:
            return
        dev, sz = self.device, self._sizes(B)[0]
        self.ws_t = {}
        for k in _hip.CONV_TRAIN_WS_KEYS:
            dt = _WS_DTYPES.get(k, torch.float32)
            self.ws_t[k] = torch.zeros(getattr(sz, k) // torch.empty(0, dtype=dt).element_size(), dtype=dt, device=dev)
        self.ws = _hip.fill(_hip.ConvTrainWs, self.ws_t)
        self.X = torch.zeros(B, self.Dp, dtype=torch.float32, device=dev)
        self.labels = torch.zeros(B, dtype=torch.int32, device=dev)
        self.Psum = torch.zeros(B, _hip.CPAD, dtype=torch.float32, device=dev)
        sizes = self.k.conv_workspace_sizes(self.acc_post, B, ACC_SAMPLES)
        self.acc_ws = {k: torch.zeros(sizes[k] // (1 if k in ("st1", "st2") else 4), dtype=torch.uint8 if k in ("st1", "st2") else torch.float32,
                                      device=dev) for k in ("P", "P1", "st1", "Q2", "st2")}           # the forward's buffers: no dZ, no input gradients
        self.Bmax = B

    def _stage(self, x, labels):
        B = int(x.shape[0])
        self._ensure(B)
        self.X[:B].copy_(x.reshape(B, -1))
        self.labels[:B].copy_(labels.reshape(B))
        return B

    def gradients(self, x, labels):
        """Draw + training forward + weight gradients of the NEXT step (no update): self.W holds the drawn weights, self.grad dCE/dW,
        ws_t["ce"] the per-point CE of the B points."""
        B = self._stage(x, labels)
        lib, st, net, ws = self.k.lib, _hip.stream_of(self.X), C.byref(self.net), C.byref(self.ws)
        _hip.check(lib.rbnn_conv_svi_train_draw(net, C.c_uint64(self.key), C.c_uint32(self.t & 0xFFFFFFFF), st), "rbnn_conv_svi_train_draw")
        _hip.check(lib.rbnn_conv_svi_train_forward(net, _hip.ptr(self.X), self.Dp, _hip.ptr(self.labels), B, ws, st), "rbnn_conv_svi_train_forward")
        _hip.check(lib.rbnn_conv_svi_weight_grads(net, _hip.ptr(self.X), self.Dp, B, ws, st), "rbnn_conv_svi_weight_grads")
        return B

    def step(self, x, labels, accuracy=True):
        """One SVI step on the device batch (x [B, 1, 28, 28] or [B, 784], labels int [B]); accuracy: the 10-sample forward of the updated
        guide is scored too.  No device->host synchronisation."""
        B = self.gradients(x, labels)
        lib, st = self.k.lib, _hip.stream_of(self.X)
        _hip.check(lib.rbnn_conv_svi_adam_step(C.byref(self.net), C.c_uint64(self.key), C.c_uint32(self.t & 0xFFFFFFFF), self.t + 1, self.lr,
                                               BETAS[0], BETAS[1], ADAM_EPS, _hip.ptr(self.kl_part), st), "rbnn_conv_svi_adam_step")
        psum = None
        if accuracy:
            self.acc_post.redraw(self.key ^ ACC_KEY, self.t)
            self.k.conv_forward(self.acc_post, self.X[:B], None, ACC_SAMPLES, _hip.OUT_PROBS, self.acc_ws)
            self.k.reduce_samples(self.acc_ws["P"], ACC_SAMPLES, B, self.C, 1.0, self.Psum)
            psum = self.Psum
        _hip.check(lib.rbnn_svi_train_finalize(_hip.ptr(self.kl_part), self.n_partials, _hip.ptr(self.ws_t["ce"]), B, _hip.ptr(psum), _hip.CPAD,
                                               _hip.ptr(self.labels), self.C, _hip.ptr(self.stats), st), "rbnn_svi_train_finalize")
        self.t += 1

    def begin_epoch(self):
        self.stats[1:].zero_()

    def epoch_totals(self):
        """(sum of the step losses, correct predictions) since begin_epoch(): the one device->host sync of an epoch."""
        s = self.stats.tolist()
        return s[1], s[2]

    def params(self):
        """(loc, raw scale) as dicts state_dict key -> fresh device tensor."""
        return ({k: v.clone() for k, v in self.unflat(self.loc).items()}, {k: v.clone() for k, v in self.unflat(self.raw).items()})
