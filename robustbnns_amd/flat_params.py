"""What SviTrainer, NnTrainer and HmcSampler share: the flat parameter buffers (state_dict order, unpadded, row-major) and the workspaces."""
import numpy as np
import torch

from . import _hip


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


def ws_struct(cls, keys, tensors):
    """The C struct of a workspace dict (a missing key: NULL)."""
    ws = cls()
    for k in keys:
        setattr(ws, k, _hip.ptr(tensors.get(k)))
    return ws
