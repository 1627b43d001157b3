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
list, through svi_train.SingleGuide (step, begin_epoch, epoch_totals, params: shared with SviTrainer); the epoch loop is BNN's, shared with BNN.train.

Several guides of ONE conv net shape train in LOCKSTEP: `ConvLockstepSvi.step(rows)` is that step for K guides, each with its own
parameters, Philox key, learning rate and rows of a resident data set, in one set of launches whose count does not depend on K (the
rbnn_conv_svi_guides_* entry points: 15 launches a step without the accuracy forward, 20 with it).  Its flat buffers are tensor-major (six
blocks [K, size of tensor], conv_train.ConvEnsembleTrainer's layout); guide k is bit-identical to a ConvSviTrainer stepped alone on
data[rows[k]] — parameters, moments, the drawn weights, gradients, per-point CE, the accuracy stack, Psum and the counters.  All guides of a
step share its point count; a guide that has finished its epochs is switched off by the step's `active` array (the kernels that write a
guide's state return at once for it: nothing is moved, so no remaining guide's addresses or bits change, and the schedule that says who is
active is known on the host before the first step).  model_bnn.train_conv_svi_lockstep is BNN.train_conv for several nets on it; guides train
in groups when their workspaces exceed the RBNN_CONV_WS_GB budget (conv_svi_lockstep_group).

What stays refused: the 3x32x32 geometry, CPU devices.  HMC posteriors of conv nets are sampled by conv_hmc.ConvHmcSampler
(BNN.train_hmc_conv), on the forward and weight gradients this step runs; several chains at once by conv_hmc.ConvLockstepHmc.
"""
import ctypes as C

import torch
import torch.nn.functional as F

from . import _hip
from .conv import ConvStackedPosterior, ConvSviGuide
from .conv_train import CONV_KEYS, check_conv_trainable, conv_group, conv_net, conv_workspace, tensor_major, views
from .flat_params import flatten
from .svi_train import ACC_KEY, ACC_SAMPLES, ADAM_EPS, BETAS, LockstepGuides, LockstepSvi, SingleGuide


class _LiveConvGuide:
    """What ConvStackedPosterior.redraw reads of a conv.ConvSviGuide (loc, sigma, the tensor ids), over views of the trainer's flat loc / sigma
    buffers: no copy, no sync, and every accuracy draw sees the current parameters.  No triple / split image is built from it, so
    ConvSviGuide's bounds are not needed."""
    TENSOR_IDS = ConvSviGuide.TENSOR_IDS

    def __init__(self, loc, sigma, device):
        self.loc, self.sigma, self.device = loc, sigma, torch.device(device)


class ConvSviTrainer(SingleGuide):
    """Device-resident SVI state of one conv guide: flat loc / raw / sigma / Adam moments, the one-sample weight buffer and its gradient
    [n_params] in state_dict order, the workspaces for up to Bmax points, the resident S = 10 stack of the accuracy forward and a device-side
    accumulator stats [3] = [step loss, sum of step losses, correct predictions].  step(x, labels, accuracy=True) is SingleGuide's, on x
    [B, 1, 28, 28] or [B, 784]."""
    ADAM_ENTRY = "rbnn_conv_svi_adam_step"

    def __init__(self, activation, input_shape, n_classes, loc, raw, lr, device, key, batch_size=128):
        check_conv_trainable(input_shape, device)
        super().__init__("conv", activation, input_shape, n_classes, loc, device, keys=CONV_KEYS)
        dev, z = self.device, self.zeros
        self.net = net = conv_net(_hip.ConvSviTrainNet, activation, self.H, self.C)
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
        dev = self.device
        self.ws_t, self.ws = conv_workspace(self._sizes(B)[0], _hip.CONV_TRAIN_WS_KEYS, _hip.ConvTrainWs, dev)
        self.Psum = torch.zeros(B, _hip.CPAD, dtype=torch.float32, device=dev)
        sizes = self.k.conv_workspace_sizes(self.acc_post, B, ACC_SAMPLES)
        self.acc_ws = {k: torch.zeros(sizes[k] // (1 if k in ("st1", "st2") else 4), dtype=torch.uint8 if k in ("st1", "st2") else torch.float32,
                                      device=dev) for k in ("P", "P1", "st1", "Q2", "st2")}           # the forward's buffers: no dZ, no input gradients
        self.staging(B)

    def gradients(self, x, labels):
        """Draw + training forward + weight gradients of the NEXT step (no update): self.W holds the drawn weights, self.grad dCE/dW,
        ws_t["ce"] the per-point CE of the B points."""
        B = self.stage(x, labels)
        lib, st, net, ws = self.k.lib, _hip.stream_of(self.X), C.byref(self.net), C.byref(self.ws)
        _hip.check(lib.rbnn_conv_svi_train_draw(net, C.c_uint64(self.key), C.c_uint32(self.t & 0xFFFFFFFF), st), "rbnn_conv_svi_train_draw")
        _hip.check(lib.rbnn_conv_svi_train_forward(net, _hip.ptr(self.X), self.Dp, _hip.ptr(self.labels), B, ws, st), "rbnn_conv_svi_train_forward")
        _hip.check(lib.rbnn_conv_svi_weight_grads(net, _hip.ptr(self.X), self.Dp, B, ws, st), "rbnn_conv_svi_weight_grads")
        return B

    def accuracy_forward(self, B):
        self.k.conv_forward(self.acc_post, self.X[:B], None, ACC_SAMPLES, _hip.OUT_PROBS, self.acc_ws)


FLAT_BUFFERS = ("loc", "raw", "sigma", "m_loc", "v_loc", "m_raw", "v_raw", "W", "grad")


class ConvLockstepSvi(LockstepGuides):
    """K SVI guides of ONE conv net shape (activation, hidden size, classes; the 1x28x28 geometry) trained in lockstep: every launch of a step
    covers all K guides (csrc/rbnn_conv_train.hip, the rbnn_conv_svi_guides_* entry points).  The nine flat buffers are [K * n_params],
    TENSOR-MAJOR (six blocks [K, size of tensor] in state_dict order: unflat(buf, k) gives guide k's views), the workspaces packed [K, B, .] for
    the call's B, stats [K, 3].  Guide k has its own parameters, key, learning rate and batch — rows[k] of the resident data (set_data) — and is
    bit-identical to a ConvSviTrainer stepped alone on data[rows[k]].  All guides of a step share its point count B = rows.shape[1].

    Finished guides: `active` (int32 [K] on the device) switches a guide off for a step — the draw, the Adam + KL update, the accuracy draw
    and sum and finalize return at once for it, so its loc, raw, sigma, moments, W, stats, log rows and accuracy weight sets are never
    written again (its rows are still staged and run through the forward: the workspaces, Psum among them, are packed by the call's B and
    hold nothing that outlives a step).  An array was chosen over compacting the
    tensor-major blocks to the remaining guides: compaction would move every remaining guide's state at a step the others do not see, for a
    saving the schedules of a grid (equal or nearly equal epoch counts) hardly have, while the array moves nothing.

    Launches per step, whatever K: draw 1, staging + forward + head 5, weight gradients 7, Adam + KL 1, finalize 1 = 15, plus the accuracy
    forward's 5 (the draw of the K x 10 weight sets, the three forward kernels, the sum over the samples); scheduled_step() adds two torch
    launches that write the step's rows from the schedule.  No device->host synchronisation: the schedule is uploaded once before the first
    step, the epoch sums go to a device log that epoch_totals() reads once after the last."""

    def __init__(self, activation, input_shape, n_classes, locs, raws, lrs, device, keys, batch_size=128):
        check_conv_trainable(input_shape, device)
        K = len(locs)
        lrs = self.refuse_bad_guides("ConvLockstepSvi", "(hidden, classes, input)", CONV_KEYS, locs, raws, lrs, keys, batch_size)
        super().__init__("conv", activation, input_shape, n_classes, locs[0], device, keys=CONV_KEYS)
        self.K = K
        self.net = conv_net(_hip.ConvSviLockstepNet, activation, self.H, self.C, n_guides=K)
        sz = self._sizes(1)
        n = self.n_params = int(sz.n_params)
        self.n_partials = int(sz.n_partials)
        assert sum(self.blocks) == n, (self.blocks, n)
        major = lambda ds: tensor_major(torch.stack([flatten(d, self.keys) for d in ds]), self.blocks)     # [K, n] guide-major -> six blocks [K, size]
        self.loc = major(locs).to(self.device)
        self.device = dev = self.loc.device                  # "cuda" names the current card: step() compares against where the buffers are
        self.raw = major(raws).to(dev)
        self.sigma = F.softplus(self.raw)
        z = self.zeros
        self.m_loc, self.v_loc, self.m_raw, self.v_raw, self.W, self.grad = (z(K * n) for _ in range(6))
        self.kl_part = z(K * self.n_partials)
        self.stats = torch.zeros(K, 3, dtype=torch.float64, device=dev)
        self.guide_values(lrs, keys)
        _hip.fill(self.net, {**vars(self), "keys": self.keys_t})
        self.net.part_stride = self.n_partials
        self.all_active = torch.ones(K, dtype=torch.int32, device=dev)
        self.acc_W = z(K * ACC_SAMPLES * n)                  # the accuracy stack does not depend on B: allocated once
        self.X = self.labels = self.epoch_log = None
        self.t = self.launches = self.Bmax = 0
        self._rows = {}
        self._ensure(int(batch_size))

    def _sizes(self, B):
        out = _hip.ConvSviLockstepBytes()
        _hip.check(self.k.lib.rbnn_conv_svi_guides_sizes(C.byref(self.net), B, C.byref(out)), "rbnn_conv_svi_guides_sizes")
        return out

    def _ensure(self, B):
        """Workspaces for batches of up to B points per guide (grown, never shrunk; a call packs them [K, its own B, .])."""
        if B <= self.Bmax:
            return
        self.ws_t, self.ws = conv_workspace(self._sizes(B), _hip.CONV_SVI_LOCKSTEP_WS_KEYS, _hip.ConvSviLockstepWs, self.device,
                                            given={"acc_W": self.acc_W})
        self.Psum = self.ws_t["Psum"]
        self._arange = torch.arange(B, dtype=torch.int32, device=self.device).unsqueeze(0)
        self.Bmax = B

    def unflat(self, buf, k=0):
        """state_dict key -> view of guide k's tensor inside its block of `buf` (one of the flat buffers), in that tensor's shape:
        ConvEnsembleTrainer.unflat."""
        return views(buf, k, self.K, self)

    def acc_sample(self, k, s):
        """state_dict key -> view of weight set s of guide k in the accuracy forward's stack (tensor-major over the K * 10 sets)."""
        return views(self.acc_W, k * ACC_SAMPLES + s, self.K * ACC_SAMPLES, self)

    def _checked(self, rows, active, epoch_slot=None):
        """(B, active) of a call, its arguments checked and the workspaces grown to B; nothing is launched before this."""
        if self.X is None:
            raise ValueError("set_data(x, labels) first")
        if (not torch.is_tensor(rows) or rows.dim() != 2 or int(rows.shape[0]) != self.K or int(rows.shape[1]) < 1 or rows.dtype != torch.int32
                or not rows.is_contiguous() or rows.device != self.device):
            raise ValueError(f"rows must be a contiguous int32 [{self.K}, B] tensor on {self.device}")
        active = self.all_active if active is None else active
        for name, v in (("active", active), ("epoch_slot", epoch_slot)):
            if v is not None and (tuple(v.shape) != (self.K,) or v.dtype != torch.int32 or v.device != self.device):
                raise ValueError(f"{name} must be an int32 [{self.K}] tensor on {self.device}")
        if epoch_slot is not None and self.epoch_log is None:
            raise ValueError("epoch_slot needs self.epoch_log (begin_log(n_epochs))")
        B = int(rows.shape[1])
        self._ensure(B)
        return B, active

    def _gradients(self, rows, B, active):
        lib, st, net = self.k.lib, _hip.stream_of(self.W), C.byref(self.net)
        _hip.check(lib.rbnn_conv_svi_guides_draw(net, _hip.ptr(active), C.c_uint32(self.t & 0xFFFFFFFF), st), "rbnn_conv_svi_guides_draw")
        _hip.check(lib.rbnn_conv_svi_guides_gradient(net, _hip.ptr(self.X), int(self.X.stride(0)), int(self.X.shape[0]), _hip.ptr(self.labels),
                                                    _hip.ptr(rows), B, C.byref(self.ws), st), "rbnn_conv_svi_guides_gradient")
        self.launches += 13

    def gradients(self, rows, active=None):
        """Draw + staging + training forward + weight gradients of the NEXT step (no update): self.W holds the drawn weights and self.grad
        dCE/dW of every guide (tensor-major), ws_t["ce"] the per-point CE packed [K, B]."""
        B, active = self._checked(rows, active)
        self._gradients(rows, B, active)
        return B

    def step(self, rows, accuracy=True, epoch_slot=None, active=None):
        """One SVI step of every active guide on rows[k] of the resident data.  rows: contiguous int32 device tensor [K, B]; a finished
        guide's rows are staged and run through the forward like the others, so they should be valid rows too (scheduled_step() gives such a
        guide row 0: its start and last are 0 in the schedule; whatever is passed, the staging kernel clamps every index into [0, n_rows),
        so a bad index reads a wrong row and never outside the data); active: int32 device tensor [K], 0 = the guide has finished (None: all are active);
        epoch_slot: int32 device tensor [K] (epoch_slot[k] >= 0: guide k's epoch ends with this step, its sums go to row epoch_slot[k] of
        self.epoch_log).  All active guides are at the same step number self.t.  No device->host synchronisation; every refusal comes before
        anything is launched."""
        B, active = self._checked(rows, active, epoch_slot)
        self._gradients(rows, B, active)
        lib, st = self.k.lib, _hip.stream_of(self.W)
        net, ws, act = C.byref(self.net), C.byref(self.ws), _hip.ptr(active)
        draw_id = C.c_uint32(self.t & 0xFFFFFFFF)
        _hip.check(lib.rbnn_conv_svi_guides_adam_step(net, act, draw_id, self.t + 1, _hip.ptr(self.lr_t), BETAS[0], BETAS[1], ADAM_EPS, st),
                   "rbnn_conv_svi_guides_adam_step")
        self.launches += 1
        if accuracy:
            _hip.check(lib.rbnn_conv_svi_guides_accuracy(net, act, B, C.c_uint64(ACC_KEY), draw_id, ws, st), "rbnn_conv_svi_guides_accuracy")
            self.launches += 5
        _hip.check(lib.rbnn_conv_svi_guides_finalize(net, act, ws, int(bool(accuracy)), B, _hip.ptr(epoch_slot), _hip.ptr(self.epoch_log),
                                                    0 if self.epoch_log is None else int(self.epoch_log.shape[1]), st), "rbnn_conv_svi_guides_finalize")
        self.launches += 1
        self.t += 1

    @staticmethod
    def schedule(n_points, epochs, batch_size, first_rows=None):
        """LockstepSvi.schedule for guides that share their point count (n_points: one number, or K equal ones): the unshuffled epochs as host
        tensors [T, K] — "start", "last", "count", "slot" — and "active" = (count > 0).  Guide k stops after epochs[k] epochs."""
        K = len(epochs)
        pts = [int(n_points)] * K if not isinstance(n_points, (list, tuple)) else [int(n) for n in n_points]
        if len(pts) != K or len(set(pts)) != 1:
            raise ValueError(f"conv guides in lockstep share one point count per step: n_points {pts} for {K} guides")
        out = LockstepSvi.schedule(pts, epochs, batch_size, first_rows)
        out["active"] = (out["count"] > 0).to(torch.int32)
        return out

    def load_schedule(self, schedule):
        """Uploads a schedule() (the one host->device copy of a run; each step's point count stays on the host) and starts a fresh device log
        for its epochs.  -> its number of steps."""
        self.sched_B = [int(v) for v in schedule["count"].max(dim=1).values.tolist()]
        self.sched = {k: v.to(self.device) for k, v in schedule.items() if k != "count"}
        self.begin_log(int(schedule["slot"].max()) + 1)
        self._ensure(max(self.sched_B))
        return len(self.sched_B)

    def scheduled_step(self, t, accuracy=True):
        """Step t of the loaded schedule: rows[k, b] = min(start[k] + b, last[k]) (two torch launches), then step().  No synchronisation."""
        s, B = self.sched, self.sched_B[t]
        if B not in self._rows:
            self._rows[B] = torch.zeros(self.K, B, dtype=torch.int32, device=self.device)
        rows = self._rows[B]
        torch.add(s["start"][t].unsqueeze(1), self._arange[:, :B], out=rows)
        torch.minimum(rows, s["last"][t].unsqueeze(1), out=rows)
        self.launches += 2
        self.step(rows, accuracy, s["slot"][t], s["active"][t])

    def params(self, k):
        """(loc, raw scale) of guide k as dicts state_dict key -> fresh device tensor."""
        return ({n: v.clone() for n, v in self.unflat(self.loc, k).items()}, {n: v.clone() for n, v in self.unflat(self.raw, k).items()})


def conv_svi_lockstep_group(activation, hidden, n_classes, n_guides, batch_size, budget_gb=None):
    """The largest number of guides (<= n_guides, >= 1) whose packed workspaces for batch_size points and nine flat buffers fit the conv
    workspace budget (conv_train.conv_group), by rbnn_conv_svi_guides_sizes for one guide, and never more than a launch takes
    (65535 // 10).  The accuracy forward's 10 x batch_size activations per guide are its large term."""
    out = _hip.ConvSviLockstepBytes()
    _hip.check(_hip.load().rbnn_conv_svi_guides_sizes(C.byref(conv_net(_hip.ConvSviLockstepNet, activation, hidden, n_classes, n_guides=1)),
                                                      int(batch_size), C.byref(out)), "rbnn_conv_svi_guides_sizes")
    per_guide = sum(getattr(out, k) for k in _hip.CONV_SVI_LOCKSTEP_WS_KEYS) + len(FLAT_BUFFERS) * 4 * out.n_params
    return conv_group(per_guide, n_guides, budget_gb, 65535 // ACC_SAMPLES)
