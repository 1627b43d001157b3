"""Deterministic training of ONE conv net of the 1x28x28 geometry on the GPU — NN.train's algorithm (model_nn.py:175-219) for the reference's
`conv` architecture (model_nn.py:93-106), reached through NN.train_conv.

One `ConvNnTrainer.step` is one `optimizer.step()` of torch.optim.Adam (single-tensor formula, betas (0.9, 0.999), eps 1e-8, no weight decay)
on nn.CrossEntropyLoss() (the MEAN of the batch's cross-entropies): the exact fp32-MFMA conv forward the attack path runs, the head, the
weight gradients of all six tensors, Adam and the step's statistics (csrc/rbnn_conv_train.hip: 13 launches on one stream, no atomics, no
device->host synchronisation).  The attribute and method names are NnTrainer's with M = 1; the buffers are flat [n_params] in state_dict order.

What stays refused: every entry point of the fc trainers (NN.train, Ensemble_NN.train, NnTrainer, BNN.train, BNN.train_hmc, the lockstep
forms) on a conv net, the 3x32x32 geometry, conv SVI / HMC / ensembles.
"""
import ctypes as C

import torch

from . import _hip
from .flat_params import flatten, unflat, ws_struct
from .nn_train import ENSEMBLE_BATCH, epoch_line, seed_all
from .svi_train import ADAM_EPS, BETAS

CONV_KEYS = [k + sfx for k in ("model.0", "model.3", "model.7") for sfx in (".weight", ".bias")]
GEOMETRY = (1, 28, 28)
_WS_DTYPES = {"st1": torch.uint8, "st2": torch.uint8, "correct": torch.int32}


def check_conv_trainable(input_shape, device):
    """The two refusals, before the library is loaded or a generator touched: a device that is not the GPU, a geometry other than 1x28x28."""
    if torch.device(device).type != "cuda":
        raise NotImplementedError(f"conv training runs on the MI355X kernels only (device {device!r}): there is no CPU compute path")
    if tuple(int(v) for v in input_shape) != GEOMETRY:
        raise NotImplementedError(f"conv training covers the 1x28x28 geometry, not {tuple(input_shape)!r}")


class ConvNnTrainer:
    """Device-resident training state of one conv net: flat parameters, Adam moments and gradients [n_params], the workspaces for up to Bmax
    points and a device-side accumulator stats [3] = [step loss, sum of step losses, correct predictions]."""

    def __init__(self, activation, input_shape, n_classes, params, lr, device, batch_size=ENSEMBLE_BATCH):
        check_conv_trainable(input_shape, device)
        self.k = _hip.HipKernels()
        self.activation, self.device = activation, torch.device(device)
        self.input_shape, self.C = GEOMETRY, int(n_classes)
        self.keys = self.state_keys = list(CONV_KEYS)
        self.shapes = {k: tuple(params[k].shape) for k in self.keys}
        self.H, self.D, self.Dp = int(self.shapes["model.3.bias"][0]), 784, 784
        net = _hip.ConvTrainNet()
        net.activation, net.in_channels, net.in_width = _hip.ACTIVATIONS[activation], 1, 28
        net.hidden, net.n_classes = self.H, self.C
        self.net = net
        self.n_params = n = self._sizes(1).n_params
        self.P = flatten(params, self.keys).to(self.device)
        assert tuple(self.P.shape) == (n,), (tuple(self.P.shape), n)
        zeros = lambda: torch.zeros(n, dtype=torch.float32, device=self.device)
        self.m, self.v, self.grad = zeros(), zeros(), zeros()
        for name in ("P", "m", "v", "grad"):
            setattr(net, name, getattr(self, name).data_ptr())
        self.stats = torch.zeros(3, dtype=torch.float64, device=self.device)
        self.lr, self.t = float(lr), 0
        self.Bmax = 0
        self.X = self.labels = None
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
        self.ws = ws_struct(_hip.ConvTrainWs, _hip.CONV_TRAIN_WS_KEYS, self.ws_t)
        self.X = torch.zeros(B, self.Dp, dtype=torch.float32, device=self.device)         # the staged batch
        self.labels = torch.zeros(B, dtype=torch.int32, device=self.device)
        self.Bmax = B

    def unflat(self, buf):
        """state_dict key -> view of `buf` (one of the flat buffers) in that tensor's shape."""
        return unflat(buf, self.keys, self.shapes)

    def _stage(self, x, labels):
        B = int(x.shape[0])
        self._ensure(B)
        self.X[:B, :self.D].copy_(x.reshape(B, -1))
        self.labels[:B].copy_(labels.reshape(B))
        return B

    def gradients(self, x, labels):
        """Training forward + weight gradients of the NEXT step (no update): self.grad holds dL/dP, ws_t["ce"] the per-point CE and
        ws_t["correct"] the per-point flags of the B points."""
        B = self._stage(x, labels)
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

    def begin_epoch(self):
        self.stats[1:].zero_()

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
    print("\n == NN training ==")
    net.device = device
    seed_all(seed)
    tr = ConvNnTrainer(net.activation, net.input_shape, net.output_size, net.state_dict(), net.lr, device,
                       batch_size=getattr(train_loader, "batch_size", None) or ENSEMBLE_BATCH)
    n = len(train_loader.dataset)
    for epoch in range(net.epochs):
        tr.begin_epoch()
        for x_batch, y_batch in train_loader:
            tr.step(x_batch.to(device), y_batch.to(device).argmax(-1))
        total_loss, correct = tr.epoch_totals()
        print(epoch_line(epoch, total_loss, correct, n), end="\t")
    net.load_state_dict({k: v.cpu() for k, v in tr.params().items()})
    net._engine = None
    if save:
        net.save()
    return tr
