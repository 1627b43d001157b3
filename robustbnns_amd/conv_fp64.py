"""The fp64 checker of the conv nets on the GPU (csrc/rbnn_conv_fp64.inc): forward, the three label-loss gradients with their norms,
FGSM / PGD from the fp64 gradient's sign; and, for the conv trainers, the per-sample WEIGHT gradients of the cross-entropy on the logits
(csrc/rbnn_conv_wgrad_dp.inc: weight_gradients).

The conv half of AttackEngine's precision='fp64' — which keeps refusing conv posteriors: this is an entry point of its own, as
conv training is (train_conv).  The posterior stays the fp32 ConvStackedPosterior (K1w .. Fb as they stand: a stored stack or a
redrawable SVI stack alike) and is widened on load; every operation from the first product on is fp64, conv2 and conv2^T on the f64
MFMA.  One kernel block is one (sample, point), every result element has one fixed accumulation order and nothing is atomic, so runs
are bit-identical and a point's result depends neither on N nor on the point block it ran in.

One GPU, the HIP kernels, the label losses: everything else is refused with HipError before anything is launched.  Point blocks are
cut so that the fp64 workspaces stay under RBNN_FP64_WS_GB (default 4); the unit is one point."""
import torch

from . import _hip
from ._hip import LOSS_MEAN_PROB, LOSS_PER_SAMPLE, OUT_LOGITS, OUT_PROBS
from .engine import AttackEngine, to_labels
from .fp64_core import Fp64Core, wgrad_arguments


def kink_margin(post, x, n_samples, block=512):
    """Per point, over the first n_samples samples: how far the conv net is from a discontinuity of its gradient — the smallest, over every
    pooling window of both layers, of the gap between the window's two largest pre-activations and of |the largest| (oracle.kink_margin's
    conv rule; relu / leaky, else +inf).  float64 [N] on the posterior's device.  A DIAGNOSTIC of the checker's users (which rows a
    comparison of fp32 results may keep), not a kernel: fp64 torch contractions on the device over the fp32 weights, `block` points at a time."""
    dev = post.device
    out = torch.full((x.shape[0],), float("inf"), dtype=torch.float64, device=dev)
    if post.activation not in ("relu", "leaky"):
        return out
    slope = 0.0 if post.activation == "relu" else 0.01
    conv = lambda h, w, b: torch.einsum("ncyxij,ocij->noyx", h.unfold(2, 5, 1).unfold(3, 5, 1), w) + b.view(1, -1, 1, 1)
    for lo in range(0, x.shape[0], block):
        xd = x[lo:lo + block].to(dev, torch.float64).reshape(-1, post.Cin, post.W, post.W)
        for s in range(n_samples):
            a = conv(xd, post.K1w[s].double().view(32, post.Cin, 5, 5), post.K1b[s].double())
            for layer, stride in ((1, 2), (2, 1)):
                win = a.unfold(2, 2, stride).unfold(3, 2, stride).reshape(a.shape[0], a.shape[1], -1, 4)
                top2 = win.topk(2, dim=-1)[0]
                m = torch.minimum(top2[..., 0] - top2[..., 1], top2[..., 0].abs()).reshape(a.shape[0], -1).amin(1)
                out[lo:lo + block] = torch.minimum(out[lo:lo + block], m)
                if layer == 1:
                    top = top2[..., 0].reshape(a.shape[0], 32, post.P1W, post.P1W)
                    a = conv(torch.where(top > 0, top, top * slope), post.K2w[s].double().view(post.H, 32, 5, 5), post.K2b[s].double())
    return out


class ConvFp64Engine:
    def __init__(self, posterior, kernels=None, group=None):
        self.post = posterior
        if getattr(posterior, "arch", None) != "conv":
            raise _hip.HipError("ConvFp64Engine is the fp64 checker of conv posteriors; fc / fc2: AttackEngine(..., precision='fp64')")
        if group is not None:
            import torch.distributed as dist
            if dist.get_world_size(group) > 1:
                raise _hip.HipError("the fp64 conv checker runs on one GPU: fp64 under a process group of more than one rank is not built")
        self.k = kernels if kernels is not None else _hip.HipKernels()
        if not isinstance(self.k, _hip.HipKernels) or self.device.type != "cuda":
            raise _hip.HipError("the fp64 conv checker needs the HIP kernels and a posterior on the GPU: there is no fp64 path on a CPU device "
                                "or through substitute kernels")
        # blocks of whole points; the second size query is weight_gradients' (dO2, dO1, ce)
        self.fp64 = Fp64Core(self.k, posterior, self.device, [self.k.conv_fp64_workspace_sizes, self.k.conv_wgrad_dp_workspace_sizes],
                             self.k.conv_forward_fp64, self.k.conv_input_grad_fp64, 1, posterior.D,
                             "the fp64 conv checker differentiates the three label losses; the autograd hook's upstream modes are not built in fp64")

    @property
    def device(self):
        return self.post.device

    # ------------------------------------------------------------------ point blocks (fp64_core: RBNN_FP64_WS_GB, default 4; the unit is one point)
    def point_block(self, S):
        """Points per block: the fp64 workspaces of a block (rbnn_conv_fp64_workspace_query: P, dZ, Psum, P1, Q2, the two argmax byte
        images, the per-sample gradients) stay within the budget."""
        return self.fp64.point_block(S)

    def point_blocks(self, N, S):
        return self.fp64.point_blocks(N, S)

    def wgrad_point_block(self, S):
        """Points per block of weight_gradients: the forward's workspaces and dO2, dO1, ce together stay within the budget."""
        return self.fp64.point_block(S, 2)

    # ------------------------------------------------------------------ inputs
    def _inputs(self, x, clone=False):
        """[N, Cin, W, W] -> contiguous fp32 [N, D] on the device, 16-byte aligned."""
        if torch.is_tensor(x) and x.requires_grad:
            raise _hip.HipError("the fp64 conv checker takes no input with requires_grad: the autograd hook is not built in fp64, and an fp32 "
                                "backward under this name would be a lie")
        x = torch.as_tensor(x)
        xf = x.detach().reshape(x.shape[0], -1).to(self.device, torch.float32).contiguous()
        if xf.shape[1] != self.post.D:
            raise ValueError(f"inputs flatten to {xf.shape[1]} features, posterior expects {self.post.D}")
        return xf.clone() if (clone or xf.data_ptr() % 16) else xf

    def _samples(self, n_samples, seeds):
        """model_bnn.py:200-202,246-252: the first n_samples stored samples, or `seeds` as indices -> (int32 index buffer or None, count)."""
        return AttackEngine.sample_index(self, n_samples, seeds)

    # ------------------------------------------------------------------ forward and gradient
    def forward(self, x, n_samples, seeds=None, logits=False):
        """Mean over the samples of the probabilities (or logits): float64 [N, C]."""
        X = self._inputs(x)
        sidx, S = self._samples(n_samples, seeds)
        return self.fp64.forward(X, sidx, S, OUT_LOGITS if logits else OUT_PROBS)[:, :self.post.C].clone()

    # ------------------------------------------------------------------ per-sample outputs and predictive uncertainty (csrc/rbnn_predictive.inc)
    def _sample_blocks(self, x, sidx, S):
        return self.fp64.sample_blocks(self._inputs(x), sidx, S)

    def sample_outputs(self, x, n_samples, seeds=None):
        """[S, N, C] float64: the probabilities of every sample; forward() is their mean.  A copy."""
        from .uncertainty import engine_sample_outputs
        return engine_sample_outputs(self, x, n_samples, seeds)

    def uncertainty(self, x, n_samples, y=None, seeds=None, n_samples_list=None):
        """AttackEngine.uncertainty from the fp64 P of this checker: the same kernel, its double-precision instantiation."""
        from .uncertainty import engine_uncertainty
        return engine_uncertainty(self, x, n_samples, y, seeds, n_samples_list)

    def loss_gradients(self, x, y, n_samples, seeds=None, norms=False):
        """lossGradients.loss_gradient for every row of x (lossGradients.py:20-40): float64 in x's shape; norms=True: also the per-point
        Linf and L2 norms of those gradients (float64 [N] each)."""
        X = self._inputs(x)
        sidx, S = self._samples(n_samples, seeds)
        nb = None
        if norms:
            nb = (torch.empty(X.shape[0], dtype=torch.float64, device=self.device), torch.empty(X.shape[0], dtype=torch.float64, device=self.device))
        G = self.fp64.gradient(X, to_labels(y, self.device), sidx, S, LOSS_PER_SAMPLE, nb).reshape(x.shape)
        return (G, nb[0], nb[1]) if norms else G

    def attack_gradient(self, x, y, n_samples, seeds=None, mode=LOSS_MEAN_PROB):
        """The gradient whose SIGN fgsm / pgd take (adversarialAttacks.py:74-79): float64 [N, D]."""
        self.fp64.check_mode(mode)
        X = self._inputs(x)
        sidx, S = self._samples(n_samples, seeds)
        return self.fp64.gradient(X, to_labels(y, self.device), sidx, S, mode)

    # ------------------------------------------------------------------ weight gradients (csrc/rbnn_conv_wgrad_dp.inc)
    def weight_gradients(self, x, y, n_samples, seeds=None, reduction="sum"):
        """The weight gradients of the trainers' loss in fp64, per sample: ({state_dict key: float64 [S, *state_dict shape]}, ce float64
        [S, N]).  Row s is d/dW_s of sum_n CE(W_s; x_n, y_n) ('sum': the data term of the SVI / HMC step) or of the mean over the N points
        ('mean': ConvNnTrainer's loss, the 1/N inside dZ as in its head); CE = logsumexp(z) - z_y on the LOGITS (nn.CrossEntropyLoss), and
        `ce` is the per-point CE, unscaled in both.  The points run in blocks under RBNN_FP64_WS_GB and every gradient element is one
        accumulation chain over the points in ascending order, carried from block to block: the result is bit-identical between runs and
        between point-block budgets."""
        p = self.post
        x, yl, N = wgrad_arguments("the fp64 conv checker", x, y, p.C, reduction)
        X = self._inputs(x)
        labels = to_labels(yl, self.device)
        sidx, S = self._samples(n_samples, seeds)
        shapes = {"dK1w": (32, p.Cin, 5, 5), "dK1b": (32,), "dK2w": (p.H, 32, 5, 5), "dK2b": (p.H,), "dFw": (p.C, p.NP2 * p.H), "dFb": (p.C,)}
        out = {}
        for k, shp in shapes.items():               # the kernels add to these: zero before the first block
            n = S * int(torch.Size(shp).numel())
            out[k] = self.fp64.buffer(-(-n // 2) * 16)[:n].view((S,) + shp).zero_()
        ce = self.fp64.buffer(-(-S * N // 2) * 16)[:S * N].view(S, N)
        for lo, hi in self.fp64.point_blocks(N, S, 2):
            n, own = hi - lo, self.fp64.workspace(hi - lo, S, 1)
            ws = {**self.fp64.workspace(n, S), **own}
            self.k.conv_forward_fp64(p, X[lo:hi], sidx, S, OUT_LOGITS, ws)
            self.k.conv_head_ce_dp(ws["P"], labels[lo:hi], S, n, p.C, 1.0 / N if reduction == "mean" else 1.0, ws["dZ"], ws["ce"])
            self.k.conv_weight_grads_dp(p, X[lo:hi], sidx, S, ws, out)
            ce[:, lo:hi] = ws["ce"].view(S, n)
        keys = ("model.0.weight", "model.0.bias", "model.3.weight", "model.3.bias", "model.7.weight", "model.7.bias")
        return dict(zip(keys, (out[k] for k in _hip.CONV_WGRAD_DP_OUT_KEYS))), ce

    # ------------------------------------------------------------------ attacks: fp32 images from the sign of the fp64 gradient
    def fgsm(self, x, y, n_samples, epsilon=0.3, seeds=None, mode=LOSS_MEAN_PROB):
        """adversarialAttacks.fgsm_attack on every row of x (adversarialAttacks.py:69-83): fp32 images."""
        self.fp64.check_mode(mode)
        X = self._inputs(x, clone=True)
        sidx, S = self._samples(n_samples, seeds)
        self.fp64.step(X, None, to_labels(y, self.device), sidx, S, mode, None, float(epsilon), 0.0, False)
        return X.reshape(x.shape)

    def pgd(self, x, y, n_samples, epsilon, alpha=None, iters=40, seeds=None, mode=LOSS_MEAN_PROB):
        """adversarialAttacks.pgd_attack on every row of x (adversarialAttacks.py:86-108): fp32 images.
        alpha=None: 2/max(image) per image (:89); a float: the same step for all (2/225, :91)."""
        self.fp64.check_mode(mode)
        X0 = self._inputs(x, clone=True)
        sidx, S = self._samples(n_samples, seeds)
        labels = to_labels(y, self.device)
        X = X0.clone()
        alpha_t = None
        if alpha is None:
            alpha_t = torch.empty(X.shape[0], dtype=torch.float32, device=self.device)
            self.k.pgd_alpha(X0, self.post.D, alpha_t)
        for _ in range(iters):
            self.fp64.step(X, X0, labels, sidx, S, mode, alpha_t, 0.0 if alpha is None else float(alpha), float(epsilon), True)
        return X.reshape(x.shape)
