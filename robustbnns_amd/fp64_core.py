"""What the fp64 checkers share on the host: AttackEngine's precision='fp64' (fc / fc2, rbnn_fp64.inc, rbnn_fc_wgrad_dp.inc) and
conv_fp64.ConvFp64Engine (rbnn_conv_fp64.inc, rbnn_conv_wgrad_dp.inc), each with its weight gradients.  The workspace budget, the point blocks
cut from it, the cached workspaces, the sequence forward -> sum over samples -> loss -> input gradient per block and what both
weight_gradients refuse are written here once; a user gives the pair of kernel wrappers, its workspace-size queries, the block unit and the
gradient's width.

Every result element is one accumulation chain that does not know its block, so blocking changes no bits."""
import os

import torch

from . import _hip
from ._hip import LOSS_MEAN_LOGIT, LOSS_MEAN_PROB, LOSS_PER_SAMPLE, OUT_LOGITS, OUT_PROBS

_U8 = ("arg1", "arg2")                      # the conv forward's argmax images: bytes, every other buffer is float64


def ws_budget():
    """Bytes the fp64 workspaces of one point block may take: RBNN_FP64_WS_GB (default 4)."""
    return float(os.environ.get("RBNN_FP64_WS_GB", "4")) * 2 ** 30


def wgrad_arguments(who, x, y, n_classes, reduction):
    """What both checkers' weight_gradients refuse before anything is launched (`who` names the checker in the message): a reduction other
    than 'sum' / 'mean', no point, labels outside [0, n_classes).  -> (x as a tensor, integer labels [N], N)"""
    if reduction not in ("sum", "mean"):
        raise _hip.HipError(f"{who}'s weight gradients take reduction 'sum' or 'mean', not {reduction!r}")
    x, yl = torch.as_tensor(x), torch.as_tensor(y)
    N = int(x.shape[0])
    if N < 1:
        raise _hip.HipError(f"{who}'s weight gradients need at least one point")
    if yl.dim() >= 2:
        yl = yl.argmax(-1)
    if yl.numel() != N:
        raise ValueError(f"{yl.numel()} labels for {N} points")
    if int(yl.min()) < 0 or int(yl.max()) >= n_classes:
        raise _hip.HipError(f"{who}'s weight gradients take labels in [0, {n_classes}): got {int(yl.min())} .. {int(yl.max())}")
    return x, yl, N


class Fp64Core:
    def __init__(self, kernels, posterior, device, sizes, forward, input_grad, unit, width, refusal):
        """sizes: the workspace-size queries (net, N, S) -> {name: bytes}; the first is the forward's and gradient's, a further one a user's
        extra buffers (the conv weight gradients').  forward (net, X, sidx, S, out_kind, ws) and input_grad (net, sidx, S, N, ws, scale, G,
        linf, l2): the kernel wrappers.  unit: blocks are multiples of this many points (the fc kernels' 16-point tile; conv: 1).  width:
        columns of the gradient.  refusal: the user's message for a loss that is not one of the three label losses."""
        self.k, self.post, self.device, self.sizes = kernels, posterior, device, list(sizes)
        self._forward, self._input_grad, self.unit, self.width, self.refusal = forward, input_grad, unit, width, refusal
        self._ws_cache = [{} for _ in self.sizes]

    # ------------------------------------------------------------------ workspaces and point blocks
    def buffer(self, n_bytes, dtype=torch.float64):
        """Every fp64 workspace and every buffer a kernel adds to is allocated here (n_bytes of `dtype`: float64, or uint8)."""
        return torch.empty(n_bytes // torch.empty((), dtype=dtype).element_size(), dtype=dtype, device=self.device)

    def point_block(self, S, n_sizes=1):
        """Points per block: the workspaces of the first n_sizes queries stay within the budget.  A multiple of the unit, at least one."""
        per_point = sum(sum(f(self.post, 1, S).values()) for f in self.sizes[:n_sizes])
        return max(self.unit, int(ws_budget() // per_point) // self.unit * self.unit)

    def point_blocks(self, N, S, n_sizes=1):
        nb = self.point_block(S, n_sizes)
        return [(lo, min(N, lo + nb)) for lo in range(0, N, nb)]

    def workspace(self, N, S, which=0):
        """The buffers of query `which` for a block of N points: the full block and a ragged tail block stay cached."""
        cache = self._ws_cache[which]
        ws = cache.pop((N, S), None)
        if ws is None:
            ws = {k: self.buffer(v, torch.uint8 if k in _U8 else torch.float64) for k, v in self.sizes[which](self.post, N, S).items() if v}
            while len(cache) > 1:
                cache.pop(next(iter(cache)))
        cache[(N, S)] = ws
        return ws

    # ------------------------------------------------------------------ forward, gradient, attack step
    def check_mode(self, mode):
        if mode not in (LOSS_MEAN_PROB, LOSS_PER_SAMPLE, LOSS_MEAN_LOGIT):
            raise _hip.HipError(self.refusal)

    def forward(self, X, sidx, S, out_kind, out=None):
        """Mean over the samples of the probabilities (or logits): float64 [N, 16], columns >= C zero."""
        N = X.shape[0]
        if out is None:
            out = torch.zeros(N, _hip.CPAD, dtype=torch.float64, device=self.device)
        for lo, hi in self.point_blocks(N, S):
            ws = self.workspace(hi - lo, S)
            self._forward(self.post, X[lo:hi], sidx, S, out_kind, ws)
            self.k.reduce_samples_f64(ws["P"], S, hi - lo, self.post.C, 1.0 / S, out[lo:hi])
        return out

    def sample_blocks(self, X, sidx, S):
        """The probabilities forward per point block -> (lo, hi, P float64 [S, hi - lo, 16]): every sample's own output, before the mean (a
        view of the cached workspace, valid until the next launch)."""
        for lo, hi in self.point_blocks(X.shape[0], S):
            ws = self.workspace(hi - lo, S)
            self._forward(self.post, X[lo:hi], sidx, S, OUT_PROBS, ws)
            yield lo, hi, ws["P"][:S * (hi - lo) * _hip.CPAD].view(S, hi - lo, _hip.CPAD)

    def gradient(self, X, labels, sidx, S, mode, norms=None):
        """The summed expected input gradient, float64 [N, width] (a fresh tensor): forward + sum over samples + loss + backward per point
        block.  The 1/S of every loss is inside dZ, as in the fp64 oracle.  norms = (linf [N], l2 [N]) float64 buffers: filled too."""
        self.check_mode(mode)
        N, p = X.shape[0], self.post
        G = torch.empty(N, self.width, dtype=torch.float64, device=self.device)
        for lo, hi in self.point_blocks(N, S):
            n, ws = hi - lo, self.workspace(hi - lo, S)
            self._forward(p, X[lo:hi], sidx, S, OUT_LOGITS if mode == LOSS_MEAN_LOGIT else OUT_PROBS, ws)
            Psum = None
            if mode != LOSS_PER_SAMPLE:
                Psum = ws["Psum"].view(n, _hip.CPAD)
                self.k.reduce_samples_f64(ws["P"], S, n, p.C, 1.0, Psum)
            self.k.loss_dlogits_f64(mode, ws["P"], Psum, labels[lo:hi], S, 1.0 / S, n, p.C, ws["dZ"])
            self._input_grad(p, sidx, S, n, ws, 1.0, G[lo:hi], None if norms is None else norms[0][lo:hi],
                             None if norms is None else norms[1][lo:hi])
        return G

    def step(self, X, X0, labels, sidx, S, mode, alpha, alpha_scalar, eps, project):
        """One FGSM / PGD step on the fp32 images X: only the SIGN of the fp64 gradient is read."""
        G = self.gradient(X, labels, sidx, S, mode)
        return self.k.attack_step_f64(X, X0, G, alpha, alpha_scalar, eps, project, self.post.D)
