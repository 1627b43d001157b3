"""Deterministic training of fc / fc2 nets on the GPU — NN.train (model_nn.py:175-219) and Ensemble_NN.train (model_ensemble.py:69-83).

One `NnTrainer.step` is one `optimizer.step()` of torch.optim.Adam (single-tensor formula, betas (0.9, 0.999), eps 1e-8, no weight decay) on
nn.CrossEntropyLoss() (the MEAN of the batch's cross-entropies) for M independent members of the same shape in LOCKSTEP: every launch covers
all members (csrc/rbnn_nn_train.hip; fc 5 launches per step, fc2 7, whatever M is).  The reference trains the members of a deep ensemble one
after the other; they share nothing but their shapes, so member m of a lockstep run is bit-identical to that member trained alone.

The batch of member m is rows[m] of a data matrix that stays on the device (`set_data`): each member follows its own permutation of the
epoch, nothing is copied per member.  `step(x, labels)` stages one batch for every member instead (NN.train's loader).

The training accuracy is scored on the training forward's own logits (model_nn.py:207: `outputs.argmax(-1)` of the same forward), and the
step loss is the fp32 mean the reference adds up (`loss.item()`); both accumulate on the device per member and are read once per epoch:
a step makes NO device->host synchronisation.
"""
import ctypes as C
import random

import numpy as np
import torch

from . import _hip
from .flat_params import FlatNets, flatten, require_gpu_fc, train_workspace
from .posterior import round_up
from .svi_train import ADAM_EPS, BETAS

ENSEMBLE_BATCH = 100                    # model_ensemble.py:73


class AdamNets(FlatNets):
    """What NnTrainer, ConvNnTrainer and ConvEnsembleTrainer (conv_train.py) share beyond FlatNets: the Adam buffers and their pointers in the
    net descriptor, the statistics, lr / t and begin_epoch.  gradients() and step() are written out in each class (they are the per-step path)."""

    def adam_state(self, net, n, P, lr):
        """P (CPU, [n] or [M, n]) onto the device beside zeroed m / v / grad, their addresses into `net`; stats [3] or [M, 3]; nothing staged."""
        self.net, self.n_params, self.P = net, n, P.to(self.device)
        assert tuple(self.P.shape) == self.lead + (n,), (tuple(self.P.shape), self.lead, n)
        self.m, self.v, self.grad = self.zeros(n), self.zeros(n), self.zeros(n)
        _hip.fill(net, self)
        self.stats = torch.zeros(*self.lead, 3, dtype=torch.float64, device=self.device)
        self.lr, self.t = float(lr), 0
        self.Bmax = 0
        self.X = self.labels = None

    def begin_epoch(self):
        self.stats[..., 1:].zero_()


class NnTrainer(AdamNets):
    """Device-resident training state of M fc / fc2 nets of one shape: flat parameters, Adam moments and gradients [M, n_params], the
    workspaces [M, B, .] and a device-side accumulator stats [M, 3] = [step loss, sum of step losses, correct predictions]."""

    def __init__(self, arch, activation, input_shape, n_classes, params, lr, device, batch_size=ENSEMBLE_BATCH):
        check_trainable(arch, device)
        if isinstance(params, dict):
            params = [params]
        super().__init__(arch, activation, input_shape, n_classes, params[0], device, members=len(params))
        self.M = len(params)
        self.Dp = round_up(self.D, 16)
        net = self.descriptor(_hip.NnTrainNet, self.M)
        net.member_stride = n = self.sizes("rbnn_nn_train_sizes", net)
        self.adam_state(net, n, torch.stack([flatten(d, self.keys) for d in params]), lr)
        self.data = self.data_labels = None
        self._ensure(int(batch_size))

    def unflat(self, buf, member=0):
        """state_dict key -> view of member `member` of `buf` (one of the flat buffers) in that tensor's shape."""
        return super().unflat(buf[member])

    def _ensure(self, B):
        """Workspaces for batches of up to B points per member (grown, never shrunk; a call packs them [M, its own B, .])."""
        if B <= self.Bmax:
            return
        dev, M = self.device, self.M
        self.ws_t = {k: v.reshape(-1) for k, v in train_workspace(self.arch, M * B, self.H, dev).items()}
        self.ws_t["correct"] = torch.zeros(M * B, dtype=torch.int32, device=dev)
        self.ws = _hip.fill(_hip.NnTrainWs, self.ws_t)
        self.staging(B)

    def set_data(self, x, labels):
        """The resident data set the row indices of step(rows=...) refer to: x [N, ...] and integer labels [N], copied to the device once."""
        N = int(x.shape[0])
        self.data = x.reshape(N, -1).to(self.device, torch.float32).contiguous()
        self.data_labels = labels.reshape(N).to(self.device, torch.int32).contiguous()
        assert int(self.data.shape[1]) == self.D, (tuple(self.data.shape), self.D)

    def _batch(self, x, labels, rows):
        """(X, ldx, n_rows, labels, rows pointer, B) of a call: a staged batch, or row indices [M, B] into the resident data."""
        if rows is not None:
            if self.data is None:
                raise ValueError("step(rows=...) needs set_data(x, labels) first")
            if rows.dim() != 2 or int(rows.shape[0]) != self.M or rows.dtype != torch.int32 or rows.device.type != "cuda" or not rows.is_contiguous():
                raise ValueError(f"rows must be a contiguous int32 [{self.M}, B] tensor on {self.device}")
            B = int(rows.shape[1])
            self._ensure(B)
            return self.data, int(self.data.stride(0)), int(self.data.shape[0]), self.data_labels, rows, B
        B = self.stage(x, labels)
        return self.X, self.Dp, self.Bmax, self.labels, None, B

    def gradients(self, x=None, labels=None, rows=None):
        """Training forward + weight gradients of the NEXT step (no update): self.grad holds dL/dP of every member, ws_t["ce"] the per-point CE
        and ws_t["correct"] the per-point flags, packed [M, B]."""
        X, ldx, n_rows, lab, rows, B = self._batch(x, labels, rows)
        lib, st, net = self.k.lib, _hip.stream_of(X), C.byref(self.net)
        _hip.check(lib.rbnn_nn_train_forward(net, _hip.ptr(X), ldx, n_rows, _hip.ptr(lab), _hip.ptr(rows), B, C.byref(self.ws), st),
                   "rbnn_nn_train_forward")
        _hip.check(lib.rbnn_nn_weight_grads(net, _hip.ptr(X), ldx, n_rows, _hip.ptr(rows), B, C.byref(self.ws), st), "rbnn_nn_weight_grads")
        return B

    def step(self, x=None, labels=None, rows=None):
        """One Adam step of every member: on the staged batch (x [B, ...], labels int [B]; the same batch for every member) or on rows [M, B]
        of the resident data.  No device->host synchronisation."""
        B = self.gradients(x, labels, rows)
        lib, st, net = self.k.lib, _hip.stream_of(self.P), C.byref(self.net)
        _hip.check(lib.rbnn_nn_adam_step(net, self.t + 1, self.lr, BETAS[0], BETAS[1], ADAM_EPS, st), "rbnn_nn_adam_step")
        _hip.check(lib.rbnn_nn_train_finalize(net, C.byref(self.ws), B, _hip.ptr(self.stats), st), "rbnn_nn_train_finalize")
        self.t += 1

    def epoch_totals(self):
        """Per member (sum of the step losses, correct predictions) since begin_epoch(): the one device->host sync of an epoch."""
        return [(s[1], s[2]) for s in self.stats.tolist()]

    def params(self):
        """One state_dict-shaped dict of fresh device tensors per member."""
        return [{k: v.clone() for k, v in self.unflat(self.P, m).items()} for m in range(self.M)]


def check_trainable(arch, device):
    """The guards of NnTrainer, also for callers that have host work to do before they construct one."""
    require_gpu_fc("deterministic training", arch, device)


def seed_all(seed):
    """model_nn.py:182-186"""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def epoch_line(epoch, total_loss, correct, n):
    """model_nn.py:211-214"""
    return f"\n[Epoch {epoch + 1}]\t loss: {total_loss / n:.8f} \t accuracy: {100 * correct / n:.2f}"


def train_on_loader(net, train_loader, device, seed, save, trainer, one):
    """NN.train (model_nn.py:175-219) behind its guards, from the net's CURRENT parameters (the reference initialises at construction and
    reseeds only here): one step per batch of the loader; the trained parameters are written back into the module.  trainer(batch_size) makes
    the trainer; one(v) is the net's entry of what its epoch_totals() and params() return."""
    print("\n == NN training ==")
    net.device = device
    seed_all(seed)
    tr = trainer(getattr(train_loader, "batch_size", None) or ENSEMBLE_BATCH)
    n = len(train_loader.dataset)
    for epoch in range(net.epochs):
        tr.begin_epoch()
        for x_batch, y_batch in train_loader:
            tr.step(x_batch.to(device), y_batch.to(device).argmax(-1))
        total_loss, correct = one(tr.epoch_totals())
        print(epoch_line(epoch, total_loss, correct, n), end="\t")
    net.load_state_dict({k: v.cpu() for k, v in one(tr.params()).items()})
    net._engine = None
    if save:
        net.save()
    return tr


def train_nn(net, train_loader, device, seed=0, save=True):
    """NN.train of an fc / fc2 net: M = 1 steps on the loader's batches."""
    check_trainable(net.architecture, device)
    return train_on_loader(net, train_loader, device, seed, save, lambda B: NnTrainer(
        net.architecture, net.activation, net.input_shape, net.output_size, [net.state_dict()], net.lr, device, batch_size=B), lambda v: v[0])


def ensemble_schedule(ens, n_points):
    """The host side of Ensemble_NN.train's sequential loop (model_ensemble.py:69-83), on the CPU: for every seed in order, the member NN is
    constructed (its init draws from the generator state the previous member's training left behind), the generators are seeded with the
    seed (model_nn.py:182-186), and the member's `epochs` permutations are drawn the way DataLoader(..., batch_size=100, shuffle=True) draws
    them — by iterating such a loader over the indices.  Training itself draws nothing from the CPU generator, so these are the initial
    weights and the batches of the reference's run.  Returns (members, int64 schedule [M, epochs, n_points])."""
    from torch.utils.data import DataLoader
    from .model_nn import NN
    members, schedule = [], []
    for seed in ens.random_seeds:
        loader = DataLoader(dataset=list(range(n_points)), batch_size=ENSEMBLE_BATCH, shuffle=True)
        net = NN(dataset_name=ens.dataset_name, input_shape=ens.input_shape, output_size=ens.output_size, hidden_size=ens.hidden_size,
                 activation=ens.activation, architecture=ens.architecture, epochs=ens.epochs, lr=ens.lr)
        seed_all(seed)
        schedule.append(torch.stack([torch.cat([b.reshape(-1).to(torch.int64) for b in loader]) for _ in range(ens.epochs)]))
        members.append(net)
    if not members:
        return members, torch.zeros(0, ens.epochs, n_points, dtype=torch.int64)
    return members, torch.stack(schedule)


def train_members(ens, x_train, y_train, device, trainer, group=None):
    """model_ensemble.py:69-83 behind its guards, for Ensemble_NN.train (fc / fc2) and Ensemble_NN.train_conv: every member's run of the
    reference's sequential loop, in lockstep.  trainer(params_list, batch_size) makes the lockstep trainer of those members (set_data,
    step(rows=...), begin_epoch, epoch_totals, params).  group: how many members train at a time (None: all of them); the groups follow one
    another, and since ensemble_schedule has fixed every member's weights and batches on the CPU, grouping changes no member's bits.
    Returns the (last) trainer."""
    n = int(len(x_train))
    members, schedule = ensemble_schedule(ens, n)
    x = torch.as_tensor(x_train)
    lab = torch.as_tensor(y_train).argmax(-1)
    group = len(members) if not group else max(1, min(int(group), len(members)))
    tr, lines, params = None, [], []
    for g0 in range(0, len(members), max(group, 1)):
        part = members[g0:g0 + group]
        tr = trainer([m.state_dict() for m in part], min(ENSEMBLE_BATCH, n))
        tr.set_data(x, lab)
        sched = schedule[g0:g0 + group].to(torch.int32).to(tr.device)
        part_lines = [[] for _ in part]
        for epoch in range(ens.epochs):
            tr.begin_epoch()
            for i in range(0, n, ENSEMBLE_BATCH):
                tr.step(rows=sched[:, epoch, i:i + ENSEMBLE_BATCH].contiguous())
            for m, (total_loss, correct) in enumerate(tr.epoch_totals()):
                part_lines[m].append(epoch_line(epoch, total_loss, correct, n))
        lines += part_lines
        params += tr.params()
    ens.device = device
    ens.ensemble_models = {}
    ens._ens_engine = None
    for seed, net, p, ls in zip(ens.random_seeds, members, params, lines):
        print("\n == NN training ==")                       # the members' epoch lines, member by member as the reference prints them
        for line in ls:
            print(line, end="\t")
        net.load_state_dict({k: v.cpu() for k, v in p.items()})
        net.device, net._engine = device, None
        ens.ensemble_models[str(seed)] = net
    ens.save()
    return tr


def train_ensemble(ens, x_train, y_train, device):
    """Ensemble_NN.train: every member's run of the reference's sequential loop, in lockstep (all members in every launch)."""
    check_trainable(ens.architecture, device)
    return train_members(ens, x_train, y_train, device, lambda params, B: NnTrainer(
        ens.architecture, ens.activation, ens.input_shape, ens.output_size, params, ens.lr, device, batch_size=B))
