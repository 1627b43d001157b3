"""What SviTrainer, LockstepSvi, NnTrainer, HmcSampler, LockstepHmc and the six conv classes (ConvNnTrainer, ConvEnsembleTrainer, ConvSviTrainer,
ConvLockstepSvi, ConvHmcSampler, ConvLockstepHmc) share: the refusals (require_gpu_fc), the constructor state of a trainer of nets of one shape
(FlatNets: shapes, the tensors' sizes `blocks`, the net descriptors, zeroed buffers, the parameter views, the staged batch; set_data: the resident
data of the lockstep classes), the flat parameter buffers (state_dict order, unpadded, row-major) and the workspaces.  What only the conv classes
share is in conv_train.py (the 1x28x28 descriptor, the workspace allocator, the tensor-major layout, the group budget); what only the lockstep
guides share is svi_train.LockstepGuides."""
import ctypes as C

import numpy as np
import torch

from . import _hip
from .posterior import LAYER_KEYS


def require_gpu_fc(what, arch=None, device=None):
    """The two refusals of everything that trains or samples on the GPU, with `what` as their subject: a device that is not the GPU, an
    architecture other than fc / fc2.  An argument left None is not checked (conv training leaves arch out)."""
    if device is not None and torch.device(device).type != "cuda":
        raise NotImplementedError(f"{what} runs on the MI355X kernels only (device {device!r}): there is no CPU compute path")
    if arch is not None and arch not in LAYER_KEYS:
        raise NotImplementedError(f"{what} covers fc and fc2, not {arch!r} (a conv net trains through NN.train_conv / BNN.train_conv, a conv "
                                  "ensemble through Ensemble_NN.train_conv, conv HMC chains are sampled by BNN.train_hmc_conv (num_chains of "
                                  "them at once) and several conv SVI guides at once train through train_conv_svi_lockstep)")


def state_keys(arch):
    return [k + sfx for k in LAYER_KEYS[arch] for sfx in (".weight", ".bias")]


def state_shapes(module):
    """[(state_dict key, shape)] of a torch module, in state_dict order."""
    return [(k, tuple(v.shape)) for k, v in module.state_dict().items()]


def keys_tensor(keys, device):
    """uint64 Philox keys in an int64 tensor (the same bits) on `device`."""
    return torch.tensor([k - (1 << 64) if k >= (1 << 63) else k for k in keys], dtype=torch.int64).to(device)


def flatten(params, keys):
    """dict key -> tensor => one fp32 CPU vector, the tensors of `keys` in order."""
    return torch.cat([params[k].detach().reshape(-1).to("cpu", torch.float32) for k in keys])


def unflat(buf, keys, shapes):
    """key -> view of `buf` ([n_params], or [..., n_params]: the leading dimensions are kept) in that tensor's shape."""
    out, off = {}, 0
    lead = tuple(buf.shape[:-1])
    for k in keys:
        m = int(np.prod(shapes[k]))
        out[k] = buf[..., off:off + m].reshape(lead + tuple(shapes[k]))
        off += m
    return out


def train_workspace(arch, n, H, device):
    """The zeroed buffers of the training forward / backward for n points: hid / dact / dA [n, H] per hidden layer, dZ [n, CPAD], ce [n]."""
    e = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=device)
    ws = {k + i: e(n, H) for i in (("1", "2") if arch == "fc2" else ("1",)) for k in ("hid", "dact", "dA")}
    return {**ws, "dZ": e(n, _hip.CPAD), "ce": e(n)}


class FlatNets:
    """The constructor state of a trainer or sampler of nets of one shape, a single net (members None: buffers [n]) or `members` of them in
    lockstep (buffers [members, n]): the kernels' handle, arch / activation / device / input_shape, the state_dict keys (`state_keys`, and
    `keys` until a class puts something else there; those of fc / fc2 unless `keys` names them, as conv does) and `shapes` (taken from
    `like`, a dict key -> tensor) with their element counts `blocks`, D / H / C, Dp (the row stride of a staged batch: D until a class pads
    it) and fwd_launches."""

    def __init__(self, arch, activation, input_shape, n_classes, like, device, members=None, keys=None):
        self.k = _hip.HipKernels()
        self.arch, self.activation, self.device = arch, activation, torch.device(device)
        self.input_shape = tuple(int(v) for v in input_shape)
        self.state_keys = self.keys = state_keys(arch) if keys is None else list(keys)
        self.shapes = {k: tuple(like[k].shape) for k in self.state_keys}
        self.blocks = [int(np.prod(self.shapes[k])) for k in self.state_keys]
        self.D = self.Dp = int(np.prod(self.input_shape))
        self.H, self.C = int(self.shapes[self.state_keys[-3]][0]), int(n_classes)      # the bias in front of the output layer: fc model.1, fc2 / conv model.3
        self.lead = () if members is None else (int(members),)
        self.fwd_launches = 2 if arch == "fc" else 4

    def descriptor(self, cls, n_members=None):
        """An _hip.SviTrainNet or _hip.NnTrainNet (n_members given) with the net's shape filled in and every pointer NULL."""
        net = cls()
        net.arch, net.activation = _hip.ARCHS[self.arch], _hip.ACTIVATIONS[self.activation]
        net.in_features, net.hidden, net.n_classes = self.D, self.H, self.C
        if n_members is not None:
            net.n_members = n_members
        return net

    def sizes(self, entry, net, *outs):
        """n_params from the `*_sizes` entry point named `entry` for the descriptor `net`; outs: the entry point's c_int64 out-parameters."""
        n = int(getattr(self.k.lib, entry)(C.byref(net), *[C.byref(o) for o in outs]))
        _hip.check(min(n, 0), entry)
        return n

    def zeros(self, n):
        """A zeroed fp32 buffer [n], or [members, n]."""
        return torch.zeros(*self.lead, n, dtype=torch.float32, device=self.device)

    def unflat(self, buf):
        """state_dict key -> view of `buf` ([n_params] or [..., n_params]) in that tensor's shape."""
        return unflat(buf, self.state_keys, self.shapes)

    def staging(self, B):
        """The buffers of a staged batch of up to B points (X [B, Dp], labels [B]); the end of a class's _ensure(B)."""
        self.X = torch.zeros(B, self.Dp, dtype=torch.float32, device=self.device)
        self.labels = torch.zeros(B, dtype=torch.int32, device=self.device)
        self.Bmax = B

    def stage(self, x, labels):
        """x [B, ...] and integer labels [B] into X / labels (the workspaces grown to B points first) -> B."""
        B = int(x.shape[0])
        self._ensure(B)
        self.X[:B, :self.D].copy_(x.reshape(B, -1))
        self.labels[:B].copy_(labels.reshape(B))
        return B


def set_data(self, x, labels):
    """The resident data the members' batches are gathered from: x [n_rows, ...], labels int [n_rows].  (A method of the lockstep classes.)"""
    n = int(x.shape[0])
    self.X = x.reshape(n, -1).to(self.device, torch.float32).contiguous()
    self.labels = labels.reshape(n).to(self.device, torch.int32).contiguous()
    if self.X.shape[1] != self.D:
        raise ValueError(f"the data have {self.X.shape[1]} features, the nets {self.D}")
