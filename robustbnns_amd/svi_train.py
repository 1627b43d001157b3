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

import torch
import torch.nn.functional as F

from . import _hip
from .flat_params import FlatNets, flatten, keys_tensor, require_gpu_fc, set_data, state_keys, train_workspace
from .posterior import StackedPosterior, SviGuide, padded_hidden, round_up

BETAS = (0.9, 0.999)                    # torch.optim.Adam defaults, what pyro.optim.Adam({"lr": lr}) wraps
ADAM_EPS = 1e-8
ACC_SAMPLES = _hip.SVI_LOCKSTEP_ACC_SAMPLES  # model_bnn.py:327
ACC_KEY = 0x9E3779B97F4A7C15            # xor-ed into the training key: the accuracy forward's draws are a stream of their own


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


def accuracy_draw_covered(kernels, arch, in_features, hidden, n_classes):
    """rbnn_svi_draw_supported for the accuracy stack of a guide of this shape, padded as StackedPosterior pads it (the predicate reads the
    descriptor's sizes only): what SviTrainer and LockstepSvi both refuse by."""
    d = _hip.Posterior()
    d.arch, d.in_features, d.in_stride = _hip.ARCHS[arch], int(in_features), round_up(int(in_features), 16)
    d.hidden, d.n_classes = padded_hidden(int(hidden)), int(n_classes)
    return bool(kernels.lib.rbnn_svi_draw_supported(C.byref(d), 0))


class _LiveGuide:
    """What rbnn_svi_draw reads of a posterior.SviGuide (its descriptor), over views of the trainer's flat loc / sigma buffers: no copy, no
    sync, and every accuracy draw sees the current parameters.  No triple / split images are built from it, so SviGuide's bounds are not needed."""
    descriptor = SviGuide.descriptor

    def __init__(self, arch, loc, sigma, device):
        self.arch, self.device = arch, torch.device(device)
        self.loc, self.sigma = loc, sigma
        self.hidden = int(loc["b1"].numel())
        self._desc = None


class SingleGuide(FlatNets):
    """The host surface SviTrainer and conv_svi_train.ConvSviTrainer share: one SVI step around a class's own gradients(), the epoch counters
    and the parameters.  A class names its Adam + KL entry point (ADAM_ENTRY: both take the same arguments) and runs its accuracy forward
    (accuracy_forward(B): the ACC_SAMPLES nets of acc_post on self.X[:B] into acc_ws["P"])."""

    def step(self, x, labels, accuracy=True):
        """One SVI step on the device batch (x [B, ...], labels int [B]); accuracy: the 10-sample forward of the updated guide is scored too.
        No device->host synchronisation."""
        B = self.gradients(x, labels)
        lib, st = self.k.lib, _hip.stream_of(self.X)
        _hip.check(getattr(lib, self.ADAM_ENTRY)(C.byref(self.net), C.c_uint64(self.key), C.c_uint32(self.t & 0xFFFFFFFF), self.t + 1, self.lr,
                                                 BETAS[0], BETAS[1], ADAM_EPS, _hip.ptr(self.kl_part), st), self.ADAM_ENTRY)
        psum = None
        if accuracy:
            self.acc_post.redraw(self.key ^ ACC_KEY, self.t)
            self.accuracy_forward(B)
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


class SviTrainer(SingleGuide):
    """Device-resident SVI state of one fc / fc2 guide: flat loc / raw / sigma / Adam moments, the one-sample weight buffer, the workspaces,
    the resident S = 10 stack of the accuracy forward and a device-side accumulator [step loss, sum of losses, correct predictions]."""
    ADAM_ENTRY = "rbnn_svi_adam_step"

    def __init__(self, arch, activation, input_shape, n_classes, loc, raw, lr, device, key, batch_size=128):
        require_gpu_fc("SVI training", arch, device)
        super().__init__(arch, activation, input_shape, n_classes, loc, device)
        dev, z = self.device, self.zeros
        self.Dp = round_up(self.D, 16)
        net, n_part = self.descriptor(_hip.SviTrainNet), C.c_int64(0)
        n = self.sizes("rbnn_svi_train_sizes", net, n_part)
        self.n_params, self.n_partials = n, int(n_part.value)
        self.loc, self.raw = flatten(loc, self.keys).to(dev), flatten(raw, self.keys).to(dev)
        assert self.loc.numel() == n, (self.loc.numel(), n)
        self.sigma = F.softplus(self.raw)
        self.m_loc, self.v_loc, self.m_raw, self.v_raw, self.W, self.grad = z(n), z(n), z(n), z(n), z(n), z(n)
        self.net = _hip.fill(net, self)
        self.kl_part = z(self.n_partials)
        self.stats = torch.zeros(3, dtype=torch.float64, device=dev)
        self.lr, self.key, self.t = float(lr), int(key) & 0xFFFFFFFFFFFFFFFF, 0
        roles = ("W1", "b1", "W2", "b2") if arch == "fc" else ("W1", "b1", "Wm", "bm", "W2", "b2")
        role_of = dict(zip(self.keys, roles))
        self.guide = _LiveGuide(arch, {role_of[k]: v for k, v in self.unflat(self.loc).items()},
                                {role_of[k]: v for k, v in self.unflat(self.sigma).items()}, dev)
        self.guide.loc["W1"] = self.guide.loc["W1"].reshape(self.H, self.D)
        self.guide.sigma["W1"] = self.guide.sigma["W1"].reshape(self.H, self.D)
        self.acc_post = StackedPosterior.for_guide(self.guide, activation, self.input_shape, self.C, ACC_SAMPLES)
        if not accuracy_draw_covered(self.k, arch, self.D, self.H, self.C):
            raise NotImplementedError(f"{arch} hidden {self.H}, {self.C} classes: outside what rbnn_svi_draw covers (the accuracy forward's draw)")
        # rbnn_fc_forward (the accuracy forward) takes a padded hidden size of 32, 64 or k * 128 only; the training kernels take any.  A trainer
        # of another size (96, 160, ...) computes gradients and steps without the accuracy; step(accuracy=True) refuses it up front (BNN's hidden sizes, powers of two >= 16, are all covered)
        Hp = self.acc_post.Hp
        self.accuracy_supported = Hp in (32, 64) or Hp % 128 == 0
        self.Bmax = 0
        self._ensure(int(batch_size))

    def _ensure(self, B):
        """Workspaces for batches of up to B points (grown, never shrunk: a short last batch reuses them)."""
        if B <= self.Bmax:
            return
        dev = self.device
        self.ws_t = train_workspace(self.arch, B, self.H, dev)
        self.ws = _hip.fill(_hip.SviTrainWs, self.ws_t)
        self.Psum = torch.zeros(B, _hip.CPAD, dtype=torch.float32, device=dev)
        sizes = self.k.workspace_sizes(self.acc_post, B, ACC_SAMPLES)
        self.acc_ws = {k: torch.empty(max(1, sizes[k] // 4), dtype=torch.float32, device=dev) for k in _hip.WS_KEYS
                       if sizes[k] and k not in ("dZ", "slabs")}
        self.staging(B)                                         # X: rows of Dp floats, zero columns [D, Dp): what rbnn_fc_forward reads

    def gradients(self, x, labels):
        """Draw + training forward + weight gradients of the NEXT step (no update): self.W holds the drawn weights, self.grad dCE/dW,
        ws_t["ce"] the per-point CE."""
        B = self.stage(x, labels)
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
        super().step(x, labels, accuracy)

    def accuracy_forward(self, B):
        self.k.fc_forward(self.acc_post, self.X[:B], None, ACC_SAMPLES, _hip.OUT_PROBS, self.acc_ws)


class LockstepGuides(FlatNets):
    """The host surface LockstepSvi and conv_svi_train.ConvLockstepSvi share: the refusals of a list of guides, the per-guide key and
    learning-rate tensors, the resident data, the device log of the epoch sums and the run over a schedule.  schedule, load_schedule,
    scheduled_step and step differ for real (counts against `active`, a fixed B against each step's own) and are each class's own."""
    set_data = set_data

    @staticmethod
    def refuse_bad_guides(who, shape_words, state_keys, locs, raws, lrs, keys, batch_size):
        """The refusals of K guides, before the library is loaded; shape_words: what lockstep guides share, in words.  -> the K learning rates."""
        K = len(locs)
        if K < 1:
            raise ValueError(f"{who} needs at least one guide")
        if len(raws) != K or len(keys) != K:
            raise ValueError(f"{K} guides need one raw-scale dict and one key per guide, not {len(raws)} and {len(keys)}")
        lrs = [float(v) for v in lrs] if isinstance(lrs, (list, tuple)) else [float(lrs)] * K
        if len(lrs) != K:
            raise ValueError(f"{len(lrs)} learning rates for {K} guides")
        if K * ACC_SAMPLES > 65535:
            raise ValueError(f"{K} guides x {ACC_SAMPLES} accuracy samples exceed the 65535 nets of one launch")
        if int(batch_size) < 1:
            raise ValueError(f"batch_size must be at least 1, not {batch_size}")
        shapes = {k: tuple(locs[0][k].shape) for k in state_keys}
        for i in range(K):
            for d in (locs[i], raws[i]):
                if {k: tuple(d[k].shape) for k in shapes} != shapes:
                    raise ValueError(f"guide {i} has another net shape than guide 0: lockstep guides share one {shape_words}")
        return lrs

    def guide_values(self, lrs, keys):
        """The guides' Philox keys and learning rates on the host (keys_list, lrs) and on the device (keys_t, lr_t)."""
        self.keys_list = [int(k) & 0xFFFFFFFFFFFFFFFF for k in keys]
        self.keys_t = keys_tensor(self.keys_list, self.device)
        self.lrs = lrs
        self.lr_t = torch.tensor(lrs, dtype=torch.float64).to(self.device)

    def begin_log(self, n_epochs):
        """A zeroed device log [K, n_epochs, 2] for the epoch sums (loss, correct predictions)."""
        self.epoch_log = torch.zeros(self.K, max(1, int(n_epochs)), 2, dtype=torch.float64, device=self.device)

    def run(self, schedule, accuracy=True):
        """Every step of a schedule(), the epoch sums into the device log (epoch_totals() reads it)."""
        for t in range(self.load_schedule(schedule)):
            self.scheduled_step(t, accuracy)

    def epoch_totals(self):
        """Per guide the list of (sum of the step losses, correct predictions) of its epochs: the one device->host read of a run."""
        return [[(row[0], row[1]) for row in guide] for guide in self.epoch_log.tolist()]


class LockstepSvi(LockstepGuides):
    """K SVI guides of ONE net shape (arch, activation, input shape, hidden size, classes) trained in lockstep: every launch of a step covers
    all K guides (csrc/rbnn_svi_lockstep.hip; the guide is grid dimension y).  Guide k has its own parameters, key, learning rate and batches —
    rows[k, :counts[k]] of the resident data (set_data) — and is bit-identical to an SviTrainer stepped alone on the same batches, except for the
    accuracy forward, whose logits come from the training GEMM's tile plan (Psum within the 1e-5 forward bar of SviTrainer's, the drawn weights
    bit-equal).  A guide with counts[k] == 0 has finished: no kernel reads or writes it.

    Launches per step, whatever K: draw 1, training forward 2 (fc) / 4 (fc2), weight gradients 1, Adam + KL 1, finalize 1 = 6 / 8, plus the
    accuracy forward's 3 / 4 (draw of the K x 10 weight sets, the hidden layers, softmax + sum over the samples); run() adds two torch
    launches that write the step's rows from the schedule (an add and a minimum).  No device->host synchronisation: the schedule (counts, first
    rows, epoch ends) is uploaded once before the first step, the epoch sums are written to a device log and read once after the last."""

    def __init__(self, arch, activation, input_shape, n_classes, locs, raws, lrs, device, keys, batch_size=64):
        require_gpu_fc("SVI training", arch, device)
        K = len(locs)
        lrs = self.refuse_bad_guides("LockstepSvi", "(arch, hidden, classes, input)", state_keys(arch), locs, raws, lrs, keys, batch_size)
        super().__init__(arch, activation, input_shape, n_classes, locs[0], device, members=K)
        self.K, n_part = K, C.c_int64(0)
        n = self.sizes("rbnn_svi_train_sizes", self.descriptor(_hip.SviTrainNet), n_part)
        self.n_params, self.n_partials = n, int(n_part.value)
        # what SviTrainer refuses, refused the same way: the sizes its accuracy stack (rbnn_svi_draw) and accuracy forward (rbnn_fc_forward) cover
        Hp = padded_hidden(self.H)
        if not accuracy_draw_covered(self.k, arch, self.D, self.H, self.C):
            raise NotImplementedError(f"{arch} hidden {self.H}, {self.C} classes: outside what rbnn_svi_draw covers (the accuracy forward's draw)")
        self.accuracy_supported = Hp in (32, 64) or Hp % 128 == 0
        self.loc = torch.stack([flatten(d, self.state_keys) for d in locs]).to(self.device)
        self.device = dev = self.loc.device                  # "cuda" names the current card: step() compares against where the buffers are
        self.raw = torch.stack([flatten(d, self.state_keys) for d in raws]).to(dev)
        assert tuple(self.loc.shape) == (K, n), (tuple(self.loc.shape), K, n)
        self.sigma = F.softplus(self.raw)
        z = self.zeros
        self.m_loc, self.v_loc, self.m_raw, self.v_raw, self.W, self.grad = z(n), z(n), z(n), z(n), z(n), z(n)
        self.kl_part = z(self.n_partials)
        self.stats = torch.zeros(K, 3, dtype=torch.float64, device=dev)
        self.guide_values(lrs, keys)
        self.keys = self.keys_list
        self.t = 0
        net = self.descriptor(_hip.NnTrainNet, K)
        net.P, net.grad, net.member_stride = self.W.data_ptr(), self.grad.data_ptr(), n
        self.net = net
        self.guides = _hip.fill(_hip.SviLockstep, {**vars(self), "keys": self.keys_t})
        self.guides.part_stride = self.n_partials
        self.X = self.labels = None
        self.epoch_log = None
        self.B = int(batch_size)
        S = ACC_SAMPLES
        self.ws_t = train_workspace(arch, K * self.B, self.H, dev)
        self.ws_t["correct"] = torch.zeros(K * self.B, dtype=torch.int32, device=dev)
        self.ws = _hip.fill(_hip.NnTrainWs, self.ws_t)
        e = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
        self.acc_t = {"W": e(K * S, n), "hid1": e(K * S * self.B, self.H), "dact": e(K * S * self.B, self.H), "Psum": e(K, self.B, _hip.CPAD)}
        if arch == "fc2":
            self.acc_t["hid2"] = e(K * S * self.B, self.H)
        self.acc = _hip.fill(_hip.SviLockstepAcc, self.acc_t)
        self.Psum = self.acc_t["Psum"]
        self.rows_t = torch.zeros(K, self.B, dtype=torch.int32, device=dev)
        self._arange = torch.arange(self.B, dtype=torch.int32, device=dev).unsqueeze(0)
        self.launches = 0

    def step(self, rows, counts, accuracy=True, epoch_slot=None):
        """One SVI step of every guide with counts[k] > 0 on rows[k, :counts[k]] of the resident data.  rows: int32 device tensor [K, batch_size]
        whose entries behind counts[k] are valid rows too; counts, epoch_slot: int32 device tensors [K] (epoch_slot[k] >= 0: guide k's epoch ends
        with this step, its sums go to row epoch_slot[k] of self.epoch_log).  All active guides are at the same step number self.t.  No
        device->host synchronisation."""
        if accuracy and not self.accuracy_supported:          # before anything is launched: no half-applied step
            raise NotImplementedError(f"hidden {self.H}: outside what rbnn_fc_forward covers (32, 64 or a multiple of 128): no accuracy forward")
        if self.X is None:
            raise ValueError("set_data(x, labels) first")
        if tuple(rows.shape) != (self.K, self.B) or rows.dtype != torch.int32 or not rows.is_contiguous() or rows.device != self.device:
            raise ValueError(f"rows must be a contiguous int32 [{self.K}, {self.B}] tensor on {self.device}")
        if tuple(counts.shape) != (self.K,) or counts.dtype != torch.int32 or counts.device != self.device:
            raise ValueError(f"counts must be an int32 [{self.K}] tensor on {self.device}")
        if epoch_slot is not None and self.epoch_log is None:
            raise ValueError("epoch_slot needs self.epoch_log (begin_log(n_epochs))")
        lib, st = self.k.lib, _hip.stream_of(self.W)
        net, g, n_rows = C.byref(self.net), C.byref(self.guides), int(self.X.shape[0])
        draw_id = C.c_uint32(self.t & 0xFFFFFFFF)
        _hip.check(lib.rbnn_svi_multi_draw(net, g, _hip.ptr(counts), draw_id, st), "rbnn_svi_multi_draw")
        _hip.check(lib.rbnn_svi_multi_gradient(net, _hip.ptr(self.X), self.D, n_rows, _hip.ptr(self.labels), _hip.ptr(rows), _hip.ptr(counts), self.B,
                                               C.byref(self.ws), st), "rbnn_svi_multi_gradient")
        _hip.check(lib.rbnn_svi_multi_adam_step(net, g, _hip.ptr(counts), draw_id, self.t + 1, _hip.ptr(self.lr_t), BETAS[0], BETAS[1], ADAM_EPS, st),
                   "rbnn_svi_multi_adam_step")
        self.launches += self.fwd_launches + 3
        psum = None
        if accuracy:
            _hip.check(lib.rbnn_svi_multi_accuracy(net, g, _hip.ptr(self.X), self.D, n_rows, _hip.ptr(rows), _hip.ptr(counts), self.B,
                                                   C.c_uint64(ACC_KEY), draw_id, C.byref(self.acc), st), "rbnn_svi_multi_accuracy")
            self.launches += self.fwd_launches // 2 + 2
            psum = self.Psum
        _hip.check(lib.rbnn_svi_multi_finalize(net, g, _hip.ptr(self.ws_t["ce"]), _hip.ptr(psum), _hip.ptr(self.labels), n_rows, _hip.ptr(rows),
                                               _hip.ptr(counts), self.B, _hip.ptr(epoch_slot), _hip.ptr(self.epoch_log),
                                               0 if self.epoch_log is None else int(self.epoch_log.shape[1]), st), "rbnn_svi_multi_finalize")
        self.launches += 1
        self.t += 1

    @staticmethod
    def schedule(n_points, epochs, batch_size, first_rows=None):
        """The unshuffled epochs of K members as host tensors [T, K] (T = the longest member's number of steps): member k walks rows
        first_rows[k] .. first_rows[k] + n_points[k] in batches of batch_size (a short last batch), epochs[k] times, then stops.
        -> {"start", "last", "count", "slot"}: first row, last valid row, number of points (0: finished) and the epoch that ends (-1: none)."""
        K = len(n_points)
        first_rows = [0] * K if first_rows is None else [int(v) for v in first_rows]
        per = [(int(n) + batch_size - 1) // batch_size for n in n_points]
        T = max(p * int(e) for p, e in zip(per, epochs))
        out = {name: torch.zeros(T, K, dtype=torch.int32) for name in ("start", "last", "count")}
        out["slot"] = torch.full((T, K), -1, dtype=torch.int32)
        for k in range(K):
            n, f = int(n_points[k]), first_rows[k]
            for t in range(per[k] * int(epochs[k])):
                i = t % per[k]
                c = min(batch_size, n - i * batch_size)
                out["start"][t, k], out["count"][t, k], out["last"][t, k] = f + i * batch_size, c, f + i * batch_size + c - 1
                if i == per[k] - 1:
                    out["slot"][t, k] = t // per[k]
        return out

    def load_schedule(self, schedule):
        """Uploads a schedule() (the one host->device copy of a run) and starts a fresh device log for its epochs.  -> its number of steps."""
        self.sched = {k: v.to(self.device) for k, v in schedule.items()}
        self.begin_log(int(schedule["slot"].max()) + 1)
        return int(schedule["count"].shape[0])

    def scheduled_step(self, t, accuracy=True):
        """Step t of the loaded schedule: rows[k, b] = min(start[k] + b, last[k]) (two torch launches), then step().  No synchronisation."""
        s = self.sched
        torch.add(s["start"][t].unsqueeze(1), self._arange, out=self.rows_t)
        torch.minimum(self.rows_t, s["last"][t].unsqueeze(1), out=self.rows_t)
        self.launches += 2
        self.step(self.rows_t, s["count"][t], accuracy, s["slot"][t])

    def params(self, k):
        """(loc, raw scale) of guide k as dicts state_dict key -> fresh device tensor."""
        return ({n: v.clone() for n, v in self.unflat(self.loc[k]).items()}, {n: v.clone() for n, v in self.unflat(self.raw[k]).items()})
