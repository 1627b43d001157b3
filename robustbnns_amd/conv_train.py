"""Deterministic training of ONE conv net of the 1x28x28 geometry on the GPU — NN.train's algorithm (model_nn.py:175-219) for the reference's
`conv` architecture (model_nn.py:93-106), reached through NN.train_conv.

One `ConvNnTrainer.step` is one `optimizer.step()` of torch.optim.Adam (single-tensor formula, betas (0.9, 0.999), eps 1e-8, no weight decay)
on nn.CrossEntropyLoss() (the MEAN of the batch's cross-entropies): the exact fp32-MFMA conv forward the attack path runs, the head, the
weight gradients of all six tensors, Adam and the step's statistics (csrc/rbnn_conv_train.hip: 13 launches on one stream, no atomics, no
device->host synchronisation).  ConvNnTrainer stands on what NnTrainer stands on (flat_params.FlatNets with conv's key list, nn_train.AdamNets:
the Adam buffers, stats, the staged batch) as a single net: the buffers are flat [n_params] in state_dict order, stats is [3].  The epoch loop is
nn_train.train_on_loader, the one NN.train runs.

What stays refused: every entry point of the fc trainers (NN.train, Ensemble_NN.train, NnTrainer, BNN.train, BNN.train_hmc, the lockstep
forms) on a conv net, the 3x32x32 geometry, conv HMC / ensembles.  SVI posteriors of conv nets are trained by conv_svi_train.ConvSviTrainer
(BNN.train_conv), on this module's forward and weight gradients.
"""
import ctypes as C

import torch

from . import _hip
from .flat_params import flatten, require_gpu_fc
from .nn_train import ENSEMBLE_BATCH, AdamNets, train_on_loader
from .svi_train import ADAM_EPS, BETAS

CONV_KEYS = [k + sfx for k in ("model.0", "model.3", "model.7") for sfx in (".weight", ".bias")]
GEOMETRY = (1, 28, 28)
_WS_DTYPES = {"st1": torch.uint8, "st2": torch.uint8, "correct": torch.int32}


def check_conv_trainable(input_shape, device):
    """The two refusals, before the library is loaded or a generator touched: a device that is not the GPU, a geometry other than 1x28x28."""
    require_gpu_fc("conv training", device=device)
    if tuple(int(v) for v in input_shape) != GEOMETRY:
        raise NotImplementedError(f"conv training covers the 1x28x28 geometry, not {tuple(input_shape)!r}")


class ConvNnTrainer(AdamNets):
    """Device-resident training state of one conv net: flat parameters, Adam moments and gradients [n_params], the workspaces for up to Bmax
    points and a device-side accumulator stats [3] = [step loss, sum of step losses, correct predictions]."""

    def __init__(self, activation, input_shape, n_classes, params, lr, device, batch_size=ENSEMBLE_BATCH):
        check_conv_trainable(input_shape, device)
        super().__init__("conv", activation, input_shape, n_classes, params, device, keys=CONV_KEYS)
        self.Dp = self.D
        net = _hip.ConvTrainNet()
        net.activation, net.in_channels, net.in_width = _hip.ACTIVATIONS[activation], 1, 28
        net.hidden, net.n_classes = self.H, self.C
        self.net = net
        self.adam_state(net, self._sizes(1).n_params, flatten(params, self.keys), lr)
        self._ensure(int(batch_size))

    def _sizes(self, B):
        out = _hip.ConvTrainBytes()
        _hip.check(self.k.lib.rbnn_conv_train_sizes(C.byref(self.net), B, C.byref(out)), "rbnn_conv_train_sizes")
        return out

    def _ensure(self, B):
        """Workspaces for batches of up to B points (grown, never shrunk; a call packs them [its own B, .])."""
        if B <= self.Bmax:
            return
        sz = self._sizes(B)
        self.ws_t = {}
        for k in _hip.CONV_TRAIN_WS_KEYS:
            dt = _WS_DTYPES.get(k, torch.float32)
            self.ws_t[k] = torch.zeros(getattr(sz, k) // torch.empty(0, dtype=dt).element_size(), dtype=dt, device=self.device)
        self.ws = _hip.fill(_hip.ConvTrainWs, self.ws_t)
        self.staging(B)

    def gradients(self, x, labels):
        """Training forward + weight gradients of the NEXT step (no update): self.grad holds dL/dP, ws_t["ce"] the per-point CE and
        ws_t["correct"] the per-point flags of the B points."""
        B = self.stage(x, labels)
        lib, st, net, ws = self.k.lib, _hip.stream_of(self.X), C.byref(self.net), C.byref(self.ws)
        _hip.check(lib.rbnn_conv_train_forward(net, _hip.ptr(self.X), self.Dp, _hip.ptr(self.labels), B, ws, st), "rbnn_conv_train_forward")
        _hip.check(lib.rbnn_conv_weight_grads(net, _hip.ptr(self.X), self.Dp, B, ws, st), "rbnn_conv_weight_grads")
        return B

    def step(self, x, labels):
        """One Adam step on the staged batch (x [B, 1, 28, 28] or [B, 784], labels int [B]).  No device->host synchronisation."""
        B = self.gradients(x, labels)
        lib, st = self.k.lib, _hip.stream_of(self.P)
        _hip.check(lib.rbnn_conv_adam_step(C.byref(self.net), self.t + 1, self.lr, BETAS[0], BETAS[1], ADAM_EPS, st), "rbnn_conv_adam_step")
        _hip.check(lib.rbnn_conv_train_finalize(C.byref(self.ws), B, _hip.ptr(self.stats), st), "rbnn_conv_train_finalize")
        self.t += 1

    def epoch_totals(self):
        """(sum of the step losses, correct predictions) since begin_epoch(): the one device->host sync of an epoch."""
        s = self.stats.tolist()
        return s[1], s[2]

    def params(self):
        """A state_dict-shaped dict of fresh device tensors."""
        return {k: v.clone() for k, v in self.unflat(self.P).items()}


def train_conv_nn(net, train_loader, device, seed=0, save=True):
    """model_nn.py:175-219 for a conv NN, from its CURRENT parameters: one step per batch of the loader; the trained parameters are written
    back into the module."""
    if net.architecture != "conv":
        raise ValueError(f"train_conv trains the conv architecture; a {net.architecture!r} net trains through train")
    check_conv_trainable(net.input_shape, device)
    return train_on_loader(net, train_loader, device, seed, save, lambda B: ConvNnTrainer(
        net.activation, net.input_shape, net.output_size, net.state_dict(), net.lr, device, batch_size=B), lambda v: v)
