"""CPU restatement of SVI training of an fc / fc2 guide (what robustbnns_amd.svi_train.SviTrainer computes; model_bnn.py:105-136, :303-365)
in any float dtype: w = loc + softplus(raw) eps, L = sum_b CE(z_b, y_b) + sum KL(N(loc, sigma) || N(0, 1)), its analytic gradients and
torch.optim.Adam's single-tensor update.  eps is the oracle's restatement of the draw's generator (O.svi_draw_philox) at sample 0."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import bnn_oracle as O

BETAS, ADAM_EPS = (0.9, 0.999), 1e-8
ACC_SAMPLES = 10                        # model_bnn.py:327: the per-step training accuracy is forward(x_batch, n_samples=10)
ACC_KEY = 0x9E3779B97F4A7C15            # xor-ed into the training key: the accuracy forward's draws (robustbnns_amd.svi_train.ACC_KEY)


def layer_keys(arch):
    return {"fc": ("model.1", "model.3"), "fc2": ("model.1", "model.3", "model.5")}[arch]


def state_keys(arch):
    return [k + s for k in layer_keys(arch) for s in (".weight", ".bias")]


def roles(arch):
    """state_dict key -> the draw's tensor name (O.SVI_TENSOR_IDS)."""
    names = ("W1", "b1", "W2", "b2") if arch == "fc" else ("W1", "b1", "Wm", "bm", "W2", "b2")
    return dict(zip(state_keys(arch), names))


def shapes_of(arch, D, H, C):
    return dict(O.param_shapes(arch, D, H, C))


def draw_eps(shapes, arch, key, draw_id, n_samples=1, sample_keys=None):
    """state_dict key -> float64 eps [n_samples, *shape] of rbnn_svi_draw / rbnn_svi_train_draw for (key, draw_id)."""
    r = roles(arch)
    zero = {r[k]: torch.zeros(s) for k, s in shapes.items()}
    _, E = O.svi_draw_philox(zero, zero, key, draw_id, n_samples, sample_keys)
    return {k: E[r[k]] for k in shapes}


def ce_grads(x, y, W, arch, act):
    """sum_b CE(z_b, y_b) and its gradient with respect to every tensor of ONE weight sample W (key -> tensor).  x [B, D], y int64 [B]."""
    ks = layer_keys(arch)
    h, pre, hs = x, [], [x]
    for i, k in enumerate(ks):
        a = h @ W[k + ".weight"].T + W[k + ".bias"]
        if i + 1 < len(ks):
            pre.append(a)
            h = O._act(a, act)
            hs.append(h)
    z = a
    ce = (torch.logsumexp(z, -1) - z.gather(1, y[:, None])[:, 0]).sum()
    d = torch.softmax(z, -1) - F.one_hot(y, z.shape[1]).to(z.dtype)
    g = {}
    for i in reversed(range(len(ks))):
        k = ks[i]
        g[k + ".weight"] = d.T @ hs[i]
        g[k + ".bias"] = d.sum(0)
        if i > 0:
            d = (d @ W[k + ".weight"]) * O._act_grad(pre[i - 1], act)
    return ce, g


def kl(loc, raw):
    tot = 0.0
    for k in loc:
        s = F.softplus(raw[k])
        tot = tot + ((-torch.log(s) + 0.5 * (s * s + loc[k] * loc[k])) - 0.5).sum()
    return tot


def step_gradients(loc, raw, eps, x, y, arch, act):
    """(loss, g_loc, g_raw, dCE/dW, W) of the ELBO at the draw w = loc + softplus(raw) eps."""
    sig = {k: F.softplus(raw[k]) for k in loc}
    W = {k: loc[k] + sig[k] * eps[k] for k in loc}
    ce, dW = ce_grads(x, y, W, arch, act)
    g_loc = {k: dW[k] + loc[k] for k in loc}
    g_raw = {k: (dW[k] * eps[k] + sig[k] - 1 / sig[k]) * torch.sigmoid(raw[k]) for k in loc}
    return ce + kl(loc, raw), g_loc, g_raw, dW, W


def adam_update(p, g, m, v, t, lr):
    """torch.optim.Adam's single-tensor step (defaults but lr), in place; t = the step number of this update (>= 1)."""
    m.lerp_(g, 1 - BETAS[0])
    v.mul_(BETAS[1]).addcmul_(g, g, value=1 - BETAS[1])
    bc1, bc2 = 1 - BETAS[0] ** t, 1 - BETAS[1] ** t
    denom = (v.sqrt() / bc2 ** 0.5).add_(ADAM_EPS)
    p.addcdiv_(m, denom, value=-lr / bc1)


class Restatement:
    """SviTrainer.step on the CPU: same init, same (key, draw id = step) eps, in `dtype`."""

    def __init__(self, loc, raw, arch, act, lr, key, dtype=torch.float64, record=False):
        self.losses = [] if record else None              # record=True: the loss of every step, in order (epoch sums are formed from it)
        self.arch, self.act, self.lr, self.key, self.dtype = arch, act, lr, key, dtype
        self.loc = {k: loc[k].detach().cpu().to(dtype).clone() for k in state_keys(arch)}
        self.raw = {k: raw[k].detach().cpu().to(dtype).clone() for k in state_keys(arch)}
        z = lambda: {k: torch.zeros_like(v) for k, v in self.loc.items()}
        self.m_loc, self.v_loc, self.m_raw, self.v_raw = z(), z(), z(), z()
        self.t = 0
        self._eps = {}

    def eps(self, t):
        if t not in self._eps:
            self._eps[t] = draw_eps({k: tuple(v.shape) for k, v in self.loc.items()}, self.arch, self.key, t)
        return {k: v[0].to(self.dtype) for k, v in self._eps[t].items()}

    def step(self, x, y):
        loss, gl, gr, _, _ = step_gradients(self.loc, self.raw, self.eps(self.t), x.reshape(x.shape[0], -1).to(self.dtype), y.long(),
                                            self.arch, self.act)
        self.t += 1
        for k in self.loc:
            adam_update(self.loc[k], gl[k], self.m_loc[k], self.v_loc[k], self.t, self.lr)
            adam_update(self.raw[k], gr[k], self.m_raw[k], self.v_raw[k], self.t, self.lr)
        if self.losses is not None:
            self.losses.append(float(loss))
        return float(loss)


def first_argmax(p):
    """Index of the FIRST maximum of every row (finalize_kernel's rule: a later class wins only if strictly larger)."""
    best = torch.zeros(p.shape[0], dtype=torch.long)
    top = p[:, 0].clone()
    for c in range(1, p.shape[1]):
        better = p[:, c] > top
        best[better] = c
        top = torch.where(better, p[:, c], top)
    return best


def top2_gap(p):
    """Per row: the gap between the two largest entries (inf for a single class)."""
    if p.shape[1] < 2:
        return torch.full((p.shape[0],), float("inf"), dtype=p.dtype)
    t = p.topk(2, dim=-1)[0]
    return t[:, 0] - t[:, 1]


def accuracy_forward(loc, raw, arch, act, x, key, t, n_samples=ACC_SAMPLES):
    """The per-step training accuracy of SviTrainer.step(accuracy=True) in fp64, at the guide (loc, raw) as it stands AFTER the update of
    step t (t = 0 for the first step): n_samples weights loc + softplus(raw) eps with eps of the draw (key ^ ACC_KEY, draw id t, sample s),
    Psum = sum over the samples of softmax(logits) (rbnn_reduce_samples at scale 1.0), the first-maximum argmax of Psum and, per point, the gap
    between the two largest MEAN probabilities.  Returns (Psum [B, C], prediction [B], gap [B])."""
    shapes = {k: tuple(v.shape) for k, v in loc.items()}
    eps = draw_eps(shapes, arch, (int(key) ^ ACC_KEY) & 0xFFFFFFFFFFFFFFFF, t, n_samples)
    post = {k: loc[k].detach().cpu().double()[None] + F.softplus(raw[k].detach().cpu().double())[None] * eps[k] for k in shapes}
    psum = torch.softmax(O.nn_logits(x.detach().cpu().double(), post, arch, act), -1).sum(0)
    return psum, first_argmax(psum), top2_gap(psum / n_samples)


def predict(loc, raw, x, arch, act, seeds):
    """BNN.forward(x, n_samples=len(seeds), seeds=seeds) of the guide (loc, raw) in fp64: the seeded in-place draw (sample key = seed)."""
    shapes = {k: tuple(v.shape) for k, v in loc.items()}
    eps = draw_eps(shapes, arch, 0, 0, len(seeds), sample_keys=list(seeds))
    post = {k: loc[k].double()[None] + F.softplus(raw[k].double())[None] * eps[k] for k in loc}
    return O.bnn_forward(x.double(), post, arch, act, len(seeds))


def two_moons(n, noise, seed):
    """Two interleaving half circles (the half-moons data set), numpy-generated: x [n, 1, 2, 1] float32, one-hot y [n, 2]."""
    rng = np.random.RandomState(seed)
    n1 = n // 2
    t1, t2 = np.pi * rng.rand(n1), np.pi * rng.rand(n - n1)
    x = np.concatenate([np.stack([np.cos(t1), np.sin(t1)], 1), np.stack([1 - np.cos(t2), 0.5 - np.sin(t2)], 1)]) + noise * rng.randn(n, 2)
    lab = np.r_[np.zeros(n1, dtype=np.int64), np.ones(n - n1, dtype=np.int64)]
    perm = rng.permutation(n)
    x, lab = x[perm], lab[perm]
    y = np.zeros((n, 2), dtype=np.float32)
    y[np.arange(n), lab] = 1.0
    return torch.from_numpy(x.astype(np.float32)).reshape(n, 1, 2, 1), torch.from_numpy(y)
