"""The torch-autograd baselines of the tools/*_timing.py programs, each stated once: the fc2 and conv shape tables, the synthetic inputs and
initial weights, the forward, the potential's gradient, the HMC transition, the SVI step and the deterministic Adam member step.  Plain eager
torch on whatever device its arguments live on; nothing here reads a value back to the host."""
import torch
import torch.nn.functional as F

KEYS = {"fc2": [k + s for k in ("model.1", "model.3", "model.5") for s in (".weight", ".bias")],
        "conv": [k + s for k in ("model.0", "model.3", "model.7") for s in (".weight", ".bias")]}
ACC_SAMPLES = 10


def fc2_shapes(D, H, C):
    return list(zip(KEYS["fc2"], [(H, D), (H,), (H, H), (H,), (C, H), (C,)]))


def conv_shapes(Hc, Cn):
    return list(zip(KEYS["conv"], [(32, 1, 5, 5), (32,), (Hc, 32, 5, 5), (Hc,), (Cn, 49 * Hc), (Cn,)]))


def images(n, Cn, dev, shape=(1, 28, 28), g=None):
    """n synthetic points in [0, 1) and their labels, from the generator g of `dev` (one seeded with 0 where none is given)."""
    g = g or torch.Generator(device=dev).manual_seed(0)
    return torch.rand(n, *shape, device=dev, generator=g), torch.randint(0, Cn, (n,), device=dev, generator=g)


def normal_weights(shapes, scale, g, shift=0.0):
    return {k: shift + scale * torch.randn(*s, generator=g) for k, s in shapes}


def logits(arch, W, x):
    """The forward of the fc2 / conv net of model_nn.py with leaky activations, from the weights W by state-dict key."""
    k = KEYS[arch]
    if arch == "fc2":
        h = F.leaky_relu(x.flatten(1) @ W[k[0]].T + W[k[1]])
        h = F.leaky_relu(h @ W[k[2]].T + W[k[3]])
    else:
        h = F.max_pool2d(F.leaky_relu(F.conv2d(x, W[k[0]], W[k[1]])), 2)
        h = F.max_pool2d(F.leaky_relu(F.conv2d(h, W[k[2]], W[k[3]])), 2, stride=1).flatten(1)
    return h @ W[k[4]].T + W[k[5]]


def potential_grad(arch, x, y, prior=True):
    """-> grad(p) -> (U, dU/dp) of U = sum CE (+ 1/2 sum p^2) at the weights p by torch autograd."""
    def grad(p):
        p = {k: v.detach().requires_grad_(True) for k, v in p.items()}
        u = F.cross_entropy(logits(arch, p, x), y, reduction="sum")
        if prior:
            u = u + 0.5 * sum((v * v).sum() for v in p.values())
        return u.detach(), dict(zip(p, torch.autograd.grad(u, list(p.values()))))
    return grad


def hmc_transition(grad, cur, gen, L, eps):
    """One HMC transition with unit mass: L leapfrog steps of size eps, so L gradient evaluations (the potential and gradient of the current
    position are carried in `cur` = (q, U, grad, ...), as the chains cache them; (q, None) starts one), eager ops, no host read
    -> (q, U, grad, dH)."""
    q, u0, g = cur[:3] if cur[1] is not None else (cur[0],) + grad(cur[0])
    g0 = g
    r = {k: torch.randn(v.shape, device=v.device, generator=gen) for k, v in q.items()}
    k0 = 0.5 * sum((v * v).sum() for v in r.values())
    p = q
    for _ in range(L):
        r = {k: r[k] - 0.5 * eps * g[k] for k in r}
        p = {k: p[k] + eps * r[k] for k in p}
        u1, g = grad(p)
        r = {k: r[k] - 0.5 * eps * g[k] for k in r}
    dH = (u1 + 0.5 * sum((v * v).sum() for v in r.values())) - (u0 + k0)
    acc = torch.rand((), device=dH.device, generator=gen) < torch.exp(-dH).clamp(max=1.0)
    return {k: torch.where(acc, p[k], q[k]) for k in q}, torch.where(acc, u1, u0), {k: torch.where(acc, g[k], g0[k]) for k in q}, dH


def svi_parameters(loc, raw, lr, dev):
    """(loc, raw, Adam over both) of a mean-field guide as leaves on dev."""
    loc, raw = ({k: v.to(dev).clone().requires_grad_(True) for k, v in d.items()} for d in (loc, raw))
    return loc, raw, torch.optim.Adam(list(loc.values()) + list(raw.values()), lr=lr)


def svi_step(forward, loc, raw, opt, x, y, accuracy=False):
    """One SVI step of a mean-field normal guide under the N(0, I) prior: w = loc + softplus(raw) eps, sum CE of forward(w, x) + KL, backward,
    Adam; accuracy: the hits of the mean softmax over ACC_SAMPLES more weight sets, under no_grad."""
    opt.zero_grad(set_to_none=True)
    W, kl = {}, 0.0
    for k in loc:
        sig = F.softplus(raw[k])
        W[k] = loc[k] + sig * torch.randn_like(sig)
        kl = kl + ((-torch.log(sig) + 0.5 * (sig * sig + loc[k] * loc[k])) - 0.5).sum()
    (F.cross_entropy(forward(W, x), y, reduction="sum") + kl).backward()
    opt.step()
    if accuracy:
        with torch.no_grad():
            p = 0.0
            for _ in range(ACC_SAMPLES):
                p = p + torch.softmax(forward({k: loc[k] + F.softplus(raw[k]) * torch.randn_like(raw[k]) for k in loc}, x), -1)
            return (p.argmax(-1) == y).sum()


def adam_member_step(forward, W, opt, x, y):
    """One deterministic training step of one member: mean CE of forward(W, x), backward, Adam."""
    opt.zero_grad(set_to_none=True)
    F.cross_entropy(forward(W, x), y).backward()
    opt.step()
