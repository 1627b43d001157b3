"""Deterministic training of ONE conv net of the 1x28x28 geometry on the GPU — NN.train's algorithm (model_nn.py:175-219) for the reference's
`conv` architecture (model_nn.py:93-106), reached through NN.train_conv.

One `ConvNnTrainer.step` is one `optimizer.step()` of torch.optim.Adam (single-tensor formula, betas (0.9, 0.999), eps 1e-8, no weight decay)
on nn.CrossEntropyLoss() (the MEAN of the batch's cross-entropies): the exact fp32-MFMA conv forward the attack path runs, the head, the
weight gradients of all six tensors, Adam and the step's statistics (csrc/rbnn_conv_train.hip: 13 launches on one stream, no atomics, no
device->host synchronisation).  ConvNnTrainer stands on what NnTrainer stands on (flat_params.FlatNets with conv's key list, nn_train.AdamNets:
the Adam buffers, stats, the staged batch) as a single net: the buffers are flat [n_params] in state_dict order, stats is [3].  The epoch loop is
nn_train.train_on_loader, the one NN.train runs.

A deep ensemble of conv nets (model_ensemble.py:69-83, reached through Ensemble_NN.train_conv) trains in LOCKSTEP: `ConvEnsembleTrainer.step` is
that step for M members of one shape, each on its own rows of a resident data set, with the member as a grid dimension of every launch (the
rbnn_conv_ens_* entry points: 14 launches whatever M is).  Its flat buffers are tensor-major (six blocks [M, size of tensor]); member m is
bit-identical to that net trained alone by ConvNnTrainer.  The host loop is nn_train.train_members, the one Ensemble_NN.train runs; members
train in groups when their workspaces exceed the RBNN_CONV_WS_GB budget (conv_ensemble_group).

What the six conv classes (these two, conv_svi_train's ConvSviTrainer / ConvLockstepSvi, conv_hmc's ConvHmcSampler / ConvLockstepHmc) share
beyond flat_params.FlatNets stands here once: the net descriptor of the geometry (conv_net), the workspace allocator and its dtype table
(conv_workspace), the tensor-major layout of the lockstep forms' flat buffers (tensor_major, views, flat_of) and the group budget
(conv_group on conv.conv_ws_budget).  gradients() / step() / _gradient() stay written out in each class: they are the per-step path.

What stays refused: every entry point of the fc trainers (NN.train, Ensemble_NN.train, NnTrainer, BNN.train, BNN.train_hmc, the lockstep
forms) on a conv net, the 3x32x32 geometry.  SVI posteriors of conv nets are trained by
conv_svi_train.ConvSviTrainer (BNN.train_conv; several guides in lockstep: conv_svi_train.ConvLockstepSvi, on the member kernels of the
ensemble) and HMC posteriors sampled by conv_hmc.ConvHmcSampler (BNN.train_hmc_conv; several chains at once: conv_hmc.ConvLockstepHmc, on
the member kernels too), on this module's forward and weight gradients.
"""
import ctypes as C

import torch

from . import _hip
from .conv import conv_ws_budget
from .flat_params import flatten, require_gpu_fc
from .nn_train import ENSEMBLE_BATCH, AdamNets, train_members, train_on_loader
from .svi_train import ADAM_EPS, BETAS

CONV_KEYS = [k + sfx for k in ("model.0", "model.3", "model.7") for sfx in (".weight", ".bias")]
GEOMETRY = (1, 28, 28)
_WS_DTYPES = {"st1": torch.uint8, "st2": torch.uint8, "acc_st1": torch.uint8, "acc_st2": torch.uint8, "correct": torch.int32, "labels": torch.int32}


def check_conv_trainable(input_shape, device):
    """The two refusals, before the library is loaded or a generator touched: a device that is not the GPU, a geometry other than 1x28x28."""
    require_gpu_fc("conv training", device=device)
    if tuple(int(v) for v in input_shape) != GEOMETRY:
        raise NotImplementedError(f"conv training covers the 1x28x28 geometry, not {tuple(input_shape)!r}")


def conv_net(cls, activation, hidden, n_classes, **count):
    """A net descriptor `cls` of _hip for a conv net of GEOMETRY with every pointer NULL; count: n_members / n_guides / n_chains = how many
    nets the descriptor of a lockstep form covers."""
    net = cls()
    net.activation, net.in_channels, net.in_width = _hip.ACTIVATIONS[activation], GEOMETRY[0], GEOMETRY[1]
    net.hidden, net.n_classes = int(hidden), int(n_classes)
    for name, v in count.items():
        setattr(net, name, int(v))
    return net


def conv_workspace(sizes, keys, struct_cls, device, given=None):
    """(ws_t, ws): the zeroed workspace buffers named `keys`, of the byte counts a `*_sizes` entry point wrote into `sizes` (fp32 unless
    _WS_DTYPES says otherwise), and the `struct_cls` of _hip that points at them.  given: key -> buffer that exists already."""
    ws_t = dict(given or {})
    for k in keys:
        if k not in ws_t:
            dt = _WS_DTYPES.get(k, torch.float32)
            ws_t[k] = torch.zeros(getattr(sizes, k) // torch.empty(0, dtype=dt).element_size(), dtype=dt, device=device)
    return ws_t, _hip.fill(struct_cls, ws_t)


# The TENSOR-MAJOR layout of the lockstep forms' flat buffers, a device contract (the rbnn_conv_ens_* kernels address it): for n nets of one
# shape, six blocks [n, size of tensor] in state_dict order, so net i's tensor t starts at n * (the single net's offset of t) + i * size.
def tensor_major(flat, blocks):
    """[n, n_params] net-major (each row flat in state_dict order) -> [n * n_params] tensor-major."""
    return torch.cat([t.reshape(-1) for t in flat.split(list(blocks), dim=1)])


def _slices(buf, i, n, blocks):
    """Net i's slice of every block of a tensor-major buffer of n nets: views, in state_dict order."""
    out, off = [], 0
    for size in blocks:
        out.append(buf[off + i * size:off + (i + 1) * size])
        off += n * size
    return out


def views(buf, i, n, nets):
    """state_dict key -> view of net i's tensor inside its block of `buf`, tensor-major over n nets, in that tensor's shape; nets: the
    FlatNets whose state_keys / shapes / blocks describe one net."""
    return {k: t.reshape(nets.shapes[k]) for k, t in zip(nets.state_keys, _slices(buf, i, n, nets.blocks))}


def flat_of(buf, i, blocks, n):
    """Net i's values of a tensor-major buffer of n nets as a flat [n_params] tensor in state_dict order (a copy)."""
    return torch.cat(_slices(buf, i, n, blocks))


def conv_group(per_net_bytes, n, budget_gb, *caps):
    """The largest number of nets (<= n and the caps, >= 1) of per_net_bytes each that fit the conv workspace budget (conv.conv_ws_budget:
    budget_gb, or RBNN_CONV_WS_GB, default 48 GB of the 288 GB).  The lockstep sizes are linear in the count, so one net's figure decides."""
    return max(1, min(int(n), int(conv_ws_budget(budget_gb) // per_net_bytes), *caps))


class ConvNnTrainer(AdamNets):
    """Device-resident training state of one conv net: flat parameters, Adam moments and gradients [n_params], the workspaces for up to Bmax
    points and a device-side accumulator stats [3] = [step loss, sum of step losses, correct predictions]."""

    def __init__(self, activation, input_shape, n_classes, params, lr, device, batch_size=ENSEMBLE_BATCH):
        check_conv_trainable(input_shape, device)
        super().__init__("conv", activation, input_shape, n_classes, params, device, keys=CONV_KEYS)
        self.net = conv_net(_hip.ConvTrainNet, activation, self.H, self.C)
        self.adam_state(self.net, self._sizes(1).n_params, flatten(params, self.keys), lr)
        self._ensure(int(batch_size))

    def _sizes(self, B):
        out = _hip.ConvTrainBytes()
        _hip.check(self.k.lib.rbnn_conv_train_sizes(C.byref(self.net), B, C.byref(out)), "rbnn_conv_train_sizes")
        return out

    def _ensure(self, B):
        """Workspaces for batches of up to B points (grown, never shrunk; a call packs them [its own B, .])."""
        if B <= self.Bmax:
            return
        self.ws_t, self.ws = conv_workspace(self._sizes(B), _hip.CONV_TRAIN_WS_KEYS, _hip.ConvTrainWs, self.device)
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


class ConvEnsembleTrainer(AdamNets):
    """Device-resident training state of M conv nets of one shape in lockstep: parameters, Adam moments and gradients flat [M * n_params],
    TENSOR-MAJOR (six blocks [M, size of tensor] in state_dict order: unflat(buf, member) gives a member's views), the workspaces packed
    [M, B, .] and stats [M, 3] = [step loss, sum of step losses, correct predictions] per member.  The batch of member m is rows[m] of the
    resident data (set_data); member m computes what a ConvNnTrainer of that net computes on those rows, bit for bit."""

    def __init__(self, activation, input_shape, n_classes, params_list, lr, device, batch_size=ENSEMBLE_BATCH):
        check_conv_trainable(input_shape, device)
        if isinstance(params_list, dict):
            params_list = [params_list]
        super().__init__("conv", activation, input_shape, n_classes, params_list[0], device, keys=CONV_KEYS)
        self.M = len(params_list)
        self.net = conv_net(_hip.ConvEnsNet, activation, self.H, self.C, n_members=self.M)
        n = self._sizes(1).n_params
        self.adam_state(self.net, self.M * n, tensor_major(torch.stack([flatten(p, self.keys) for p in params_list]), self.blocks), lr)
        self.n_params = n
        self.stats = torch.zeros(self.M, 3, dtype=torch.float64, device=self.device)
        self.data = self.data_labels = None
        self._ensure(int(batch_size))

    def _sizes(self, B):
        out = _hip.ConvEnsBytes()
        _hip.check(self.k.lib.rbnn_conv_ens_sizes(C.byref(self.net), B, C.byref(out)), "rbnn_conv_ens_sizes")
        return out

    def _ensure(self, B):
        """Workspaces for batches of up to B points per member (grown, never shrunk; a call packs them [M, its own B, .])."""
        if B <= self.Bmax:
            return
        self.ws_t, self.ws = conv_workspace(self._sizes(B), _hip.CONV_ENS_WS_KEYS, _hip.ConvEnsWs, self.device)
        self.Bmax = B

    def unflat(self, buf, member=0):
        """state_dict key -> view of member `member`'s tensor inside its block of `buf` (one of the flat buffers), in that tensor's shape."""
        return views(buf, member, self.M, self)

    def set_data(self, x, labels):
        """The resident data set the row indices of step(rows=...) refer to: x [N, ...] and integer labels [N], copied to the device once."""
        N = int(x.shape[0])
        self.data = x.reshape(N, -1).to(self.device, torch.float32).contiguous()
        self.data_labels = labels.reshape(N).to(self.device, torch.int32).contiguous()
        assert int(self.data.shape[1]) == self.D, (tuple(self.data.shape), self.D)

    def _batch(self, rows):
        """B of a call, its rows checked (NnTrainer._batch's refusals) and the workspaces grown to it; nothing is launched before this."""
        if self.data is None:
            raise ValueError("step(rows=...) needs set_data(x, labels) first")
        if (not torch.is_tensor(rows) or rows.dim() != 2 or int(rows.shape[0]) != self.M or rows.dtype != torch.int32 or rows.device.type != "cuda"
                or not rows.is_contiguous()):
            raise ValueError(f"rows must be a contiguous int32 [{self.M}, B] tensor on {self.device}")
        B = int(rows.shape[1])
        self._ensure(B)
        return B

    def gradients(self, rows):
        """Staging, training forward and weight gradients of the NEXT step (no update): self.grad holds dL/dP of every member, ws_t["ce"] the
        per-point CE and ws_t["correct"] the per-point flags, packed [M, B]."""
        B = self._batch(rows)
        lib, st, net, ws = self.k.lib, _hip.stream_of(self.data), C.byref(self.net), C.byref(self.ws)
        _hip.check(lib.rbnn_conv_ens_stage(net, _hip.ptr(self.data), int(self.data.stride(0)), int(self.data.shape[0]), _hip.ptr(self.data_labels),
                                           _hip.ptr(rows), B, ws, st), "rbnn_conv_ens_stage")
        _hip.check(lib.rbnn_conv_ens_forward(net, B, ws, st), "rbnn_conv_ens_forward")
        _hip.check(lib.rbnn_conv_ens_weight_grads(net, B, ws, st), "rbnn_conv_ens_weight_grads")
        return B

    def step(self, rows):
        """One Adam step of every member on rows [M, B] of the resident data.  No device->host synchronisation."""
        B = self.gradients(rows)
        lib, st, net = self.k.lib, _hip.stream_of(self.P), C.byref(self.net)
        _hip.check(lib.rbnn_conv_ens_adam_step(net, self.t + 1, self.lr, BETAS[0], BETAS[1], ADAM_EPS, st), "rbnn_conv_ens_adam_step")
        _hip.check(lib.rbnn_conv_ens_finalize(net, C.byref(self.ws), B, _hip.ptr(self.stats), st), "rbnn_conv_ens_finalize")
        self.t += 1

    def epoch_totals(self):
        """Per member (sum of the step losses, correct predictions) since begin_epoch(): the one device->host sync of an epoch."""
        return [(s[1], s[2]) for s in self.stats.tolist()]

    def params(self):
        """One state_dict-shaped dict of fresh device tensors per member."""
        return [{k: v.clone() for k, v in self.unflat(self.P, m).items()} for m in range(self.M)]


def conv_ensemble_group(activation, hidden, n_classes, n_members, batch_size, budget_gb=None):
    """The largest number of members (<= n_members, >= 1) whose packed workspaces for batch_size points and four flat buffers fit the conv
    workspace budget (conv_group), by rbnn_conv_ens_sizes for one member."""
    out = _hip.ConvEnsBytes()
    _hip.check(_hip.load().rbnn_conv_ens_sizes(C.byref(conv_net(_hip.ConvEnsNet, activation, hidden, n_classes, n_members=1)), int(batch_size),
                                               C.byref(out)), "rbnn_conv_ens_sizes")
    return conv_group(sum(getattr(out, k) for k in _hip.CONV_ENS_WS_KEYS) + 4 * 4 * out.n_params, n_members, budget_gb)


def train_conv_ensemble(ens, x_train, y_train, device, group=None):
    """Ensemble_NN.train_conv: model_ensemble.py:69-83 for a conv ensemble of the 1x28x28 geometry, the host side of nn_train.train_ensemble
    (train_members) around ConvEnsembleTrainer.  group: members trained at a time — None: all of them when their workspaces fit the
    RBNN_CONV_WS_GB budget, else the largest group that does; the groups follow one another and no member's bits depend on the grouping."""
    if ens.architecture != "conv":
        raise ValueError(f"train_conv trains the conv architecture; a {ens.architecture!r} ensemble trains through train")
    check_conv_trainable(ens.input_shape, device)
    if group is None:
        group = conv_ensemble_group(ens.activation, ens.hidden_size, ens.output_size, max(len(ens.random_seeds), 1), min(ENSEMBLE_BATCH, max(int(len(x_train)), 1)))
    return train_members(ens, x_train, y_train, device, lambda params, B: ConvEnsembleTrainer(
        ens.activation, ens.input_shape, ens.output_size, params, ens.lr, device, batch_size=B), group=group)


def train_conv_nn(net, train_loader, device, seed=0, save=True):
    """model_nn.py:175-219 for a conv NN, from its CURRENT parameters: one step per batch of the loader; the trained parameters are written
    back into the module."""
    if net.architecture != "conv":
        raise ValueError(f"train_conv trains the conv architecture; a {net.architecture!r} net trains through train")
    check_conv_trainable(net.input_shape, device)
    return train_on_loader(net, train_loader, device, seed, save, lambda B: ConvNnTrainer(
        net.activation, net.input_shape, net.output_size, net.state_dict(), net.lr, device, batch_size=B), lambda v: v)
