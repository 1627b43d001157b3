"""SVI training of fc / fc2 guides on the GPU — the `_train_svi` half of the reference (model_bnn.py:105-136, :303-365).

One `SviTrainer.step(x, labels)` is one `svi.step` of SVI(model, guide, pyro.optim.Adam({"lr": lr}), TraceMeanField_ELBO()):

  * ONE weight sample w = loc + softplus(raw) * eps (pyro.random_module samples once per guide call, outside the data plate);
  * loss = sum_b CE(z_b, y_b) (Categorical(logits=log_softmax(z)) observed over the plate: a sum, not a mean)
           + sum over every parameter element of KL(N(loc, sigma) || N(0, 1)) (TraceMeanField's analytic KL against the N(0, 1) priors);
  * g_loc = dCE/dw + loc,  g_raw = (dCE/dw * eps + sigma - 1/sigma) * sigmoid(raw);
  * one torch.optim.Adam step (single-tensor formula, betas (0.9, 0.999), eps 1e-8, no weight decay) on every loc and raw scale.

Then the reference's per-step training accuracy, `self.forward(x_batch, n_samples=10)` (model_bnn.py:327-329): 10 weight samples drawn from
the trainer's LIVE loc / sigma buffers by rbnn_svi_draw into a resident stack and run through the exact-path forward kernels.

Kernels: csrc/rbnn_train.hip (draw, training forward, weight gradients, Adam + KL, finalize).  Launches per step: fc 6, fc2 8, plus the
two torch copies that stage the batch and the accuracy forward (rbnn_svi_draw, rbnn_fc_forward — fc2: two kernels —, rbnn_reduce_samples).
A step makes NO device->host synchronisation: the loss and the correct predictions accumulate on the device and are read once per epoch.  eps is a pure function of (key, draw id = global step, tensor, element), so the update
regenerates it instead of storing it.  Seed-for-seed parity with pyro's own RNG stream is unpinned, as for the draw (model_bnn.py docstring).
"""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

from . import _hip
from .flat_params import flatten, train_workspace, unflat, ws_struct
from .posterior import LAYER_KEYS, StackedPosterior, SviGuide, round_up

BETAS = (0.9, 0.999)                    # torch.optim.Adam defaults, what pyro.optim.Adam({"lr": lr}) wraps
ADAM_EPS = 1e-8
ACC_SAMPLES = 10                        # model_bnn.py:327
ACC_KEY = 0x9E3779B97F4A7C15            # xor-ed into the training key: the accuracy forward's draws are a stream of their own


def state_keys(arch):
    return [k + sfx for k in LAYER_KEYS[arch] for sfx in (".weight", ".bias")]


def initial_params(shapes):
    """The guide's pyro.param initialisers on first use (model_bnn.py:124-126): for every state_dict key in order, `<key>_loc` = randn,
    then `<key>_scale` = randn, from torch's CPU generator.  shapes: list of (key, shape)."""
    loc, raw = {}, {}
    for k, shp in shapes:
        loc[k] = torch.randn(shp)
        raw[k] = torch.randn(shp)
    return loc, raw


def draw_key():
    """64 bits from torch's CPU generator: the Philox key of one train() call's draws (host arithmetic only)."""
    return int(torch.randint(-(2 ** 63), 2 ** 63 - 1, (1,), dtype=torch.int64).item()) & 0xFFFFFFFFFFFFFFFF


class _LiveGuide:
    """What rbnn_svi_draw reads of a posterior.SviGuide (its descriptor), over views of the trainer's flat loc / sigma buffers: no copy, no
    sync, and every accuracy draw sees the current parameters.  No triple / split images are built from it, so SviGuide's bounds are not needed."""
    descriptor = SviGuide.descriptor

    def __init__(self, arch, loc, sigma, device):
        self.arch, self.device = arch, torch.device(device)
        self.loc, self.sigma = loc, sigma
        self.hidden = int(loc["b1"].numel())
        self._desc = None


class SviTrainer:
    """Device-resident SVI state of one fc / fc2 guide: flat loc / raw / sigma / Adam moments, the one-sample weight buffer, the workspaces,
    the resident S = 10 stack of the accuracy forward and a device-side accumulator [step loss, sum of losses, correct predictions]."""

    def __init__(self, arch, activation, input_shape, n_classes, loc, raw, lr, device, key, batch_size=128):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise NotImplementedError(f"SVI training runs on the MI355X kernels only (device {device!r}): there is no CPU compute path")
        if arch not in LAYER_KEYS:
            raise NotImplementedError(f"SVI training covers fc and fc2, not {arch!r} (conv needs conv weight gradients)")
        self.k = _hip.HipKernels()
        self.arch, self.activation, self.device = arch, activation, dev
        self.input_shape = tuple(int(v) for v in input_shape)
        self.keys = state_keys(arch)
        self.shapes = {k: tuple(loc[k].shape) for k in self.keys}
        self.D = int(np.prod(self.input_shape))
        self.Dp = round_up(self.D, 16)
        self.H, self.C = int(self.shapes[self.keys[1]][0]), int(n_classes)
        net = _hip.SviTrainNet()
        net.arch, net.activation = _hip.ARCHS[arch], _hip.ACTIVATIONS[activation]
        net.in_features, net.hidden, net.n_classes = self.D, self.H, self.C
        n_part = C.c_int64(0)
        n = int(self.k.lib.rbnn_svi_train_sizes(C.byref(net), C.byref(n_part)))
        _hip.check(min(n, 0), "rbnn_svi_train_sizes")
        self.n_params, self.n_partials = n, int(n_part.value)
        self.loc, self.raw = flatten(loc, self.keys).to(dev), flatten(raw, self.keys).to(dev)
        assert self.loc.numel() == n, (self.loc.numel(), n)
        self.sigma = F.softplus(self.raw)
        z = lambda: torch.zeros(n, dtype=torch.float32, device=dev)
        self.m_loc, self.v_loc, self.m_raw, self.v_raw, self.W, self.grad = z(), z(), z(), z(), z(), z()
        for name in ("loc", "raw", "sigma", "m_loc", "v_loc", "m_raw", "v_raw", "W", "grad"):
            setattr(net, name, getattr(self, name).data_ptr())
        self.net = net
        self.kl_part = torch.zeros(self.n_partials, dtype=torch.float32, device=dev)
        self.stats = torch.zeros(3, dtype=torch.float64, device=dev)
        self.lr, self.key, self.t = float(lr), int(key) & 0xFFFFFFFFFFFFFFFF, 0
        roles = ("W1", "b1", "W2", "b2") if arch == "fc" else ("W1", "b1", "Wm", "bm", "W2", "b2")
        role_of = dict(zip(self.keys, roles))
        self.guide = _LiveGuide(arch, {role_of[k]: v for k, v in self.unflat(self.loc).items()},
                                {role_of[k]: v for k, v in self.unflat(self.sigma).items()}, dev)
        self.guide.loc["W1"] = self.guide.loc["W1"].reshape(self.H, self.D)
        self.guide.sigma["W1"] = self.guide.sigma["W1"].reshape(self.H, self.D)
        self.acc_post = StackedPosterior.for_guide(self.guide, activation, self.input_shape, self.C, ACC_SAMPLES)
        if not self.k.svi_draw_supported(self.acc_post, False):
            raise NotImplementedError(f"{arch} hidden {self.H}, {self.C} classes: outside what rbnn_svi_draw covers (the accuracy forward's draw)")
        # rbnn_fc_forward (the accuracy forward) takes a padded hidden size of 32, 64 or k * 128 only; the training kernels take any.  A trainer
        # of another size (96, 160, ...) computes gradients and steps without the accuracy; step(accuracy=True) refuses it up front (BNN's hidden sizes, powers of two >= 16, are all covered)
        Hp = self.acc_post.Hp
        self.accuracy_supported = Hp in (32, 64) or Hp % 128 == 0
        self.Bmax = 0
        self._ensure(int(batch_size))

    def unflat(self, buf):
        """state_dict key -> view of `buf` (one of the flat buffers) in that tensor's shape."""
        return unflat(buf, self.keys, self.shapes)

    def _ensure(self, B):
        """Workspaces for batches of up to B points (grown, never shrunk: a short last batch reuses them)."""
        if B <= self.Bmax:
            return
        dev = self.device
        e = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
        self.ws_t = train_workspace(self.arch, B, self.H, dev)
        self.ws = ws_struct(_hip.SviTrainWs, _hip.SVI_TRAIN_WS_KEYS, self.ws_t)
        self.X = e(B, self.Dp)                                  # rows of Dp floats, zero columns [D, Dp): what rbnn_fc_forward reads
        self.labels = torch.zeros(B, dtype=torch.int32, device=dev)
        self.Psum = e(B, _hip.CPAD)
        sizes = self.k.workspace_sizes(self.acc_post, B, ACC_SAMPLES)
        self.acc_ws = {k: torch.empty(max(1, sizes[k] // 4), dtype=torch.float32, device=dev) for k in _hip.WS_KEYS
                       if sizes[k] and k not in ("dZ", "slabs")}
        self.Bmax = B

    def _stage(self, x, labels):
        B = int(x.shape[0])
        self._ensure(B)
        self.X[:B, :self.D].copy_(x.reshape(B, -1))
        self.labels[:B].copy_(labels.reshape(B))
        return B

    def gradients(self, x, labels):
        """Draw + training forward + weight gradients of the NEXT step (no update): self.W holds the drawn weights, self.grad dCE/dW,
        ws_t["ce"] the per-point CE."""
        B = self._stage(x, labels)
        lib, st, net = self.k.lib, _hip.stream_of(self.X), C.byref(self.net)
        _hip.check(lib.rbnn_svi_train_draw(net, C.c_uint64(self.key), C.c_uint32(self.t & 0xFFFFFFFF), st), "rbnn_svi_train_draw")
        _hip.check(lib.rbnn_svi_train_forward(net, _hip.ptr(self.X), self.Dp, B, _hip.ptr(self.labels), C.byref(self.ws), st),
                   "rbnn_svi_train_forward")
        _hip.check(lib.rbnn_svi_weight_grads(net, _hip.ptr(self.X), self.Dp, B, C.byref(self.ws), st), "rbnn_svi_weight_grads")
        return B

    def step(self, x, labels, accuracy=True):
        """One SVI step on the device batch (x [B, ...], labels int [B]); accuracy: the 10-sample forward of the updated guide is scored too.
        No device->host synchronisation."""
        if accuracy and not self.accuracy_supported:          # before anything is launched: no half-applied step
            raise NotImplementedError(f"hidden {self.H}: outside what rbnn_fc_forward covers (32, 64 or a multiple of 128): no accuracy forward")
        B = self.gradients(x, labels)
        lib, st = self.k.lib, _hip.stream_of(self.X)
        _hip.check(lib.rbnn_svi_adam_step(C.byref(self.net), C.c_uint64(self.key), C.c_uint32(self.t & 0xFFFFFFFF), self.t + 1, self.lr,
                                          BETAS[0], BETAS[1], ADAM_EPS, _hip.ptr(self.kl_part), st), "rbnn_svi_adam_step")
        psum = None
        if accuracy:
            self.acc_post.redraw(self.key ^ ACC_KEY, self.t)
            self.k.fc_forward(self.acc_post, self.X[:B], None, ACC_SAMPLES, _hip.OUT_PROBS, self.acc_ws)
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
