"""Per-transition time of HMC on the GPU (robustbnns_amd.hmc.HmcSampler, csrc/rbnn_hmc.hip) against a torch-autograd HMC transition on the
same GPU, at the shapes of the reference's half-moons grid (fc2, hidden 32 / 128 / 512, B = 1024, D = 2) and of saved model_1 (fc2-512,
B = 5000, D = 784).  Both run L = 10 leapfrog steps at a fixed step size with unit mass (the sampling phase: no adaptation, no host reads).
Each figure: median and min..max over REPS blocks of N transitions, timed with device events after a warm-up block.  One JSON line per shape.

    python tools/hmc_timing.py [--reps 7] [--n 20]

--chains K: instead, K chains in lockstep (hmc.LockstepHmc: every launch covers all K) against K consecutive HmcSampler transitions in the
same process, on half-moons fc2-32 and fc2-512 at B = 1024: chain-transitions per second of both and their ratio, one JSON line per shape.

    python tools/hmc_timing.py --chains 8
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as G                                    # noqa: E402
from timing import blocks                                # noqa: E402

SHAPES = [("fc2", 2, 32, 2, 1024), ("fc2", 2, 128, 2, 1024), ("fc2", 2, 512, 2, 1024), ("fc2", 784, 512, 10, 5000)]
L, EPS = 10, 1e-4


def shapes_of(D, H, C):
    return {"model.1.weight": (H, D), "model.1.bias": (H,), "model.3.weight": (H, H), "model.3.bias": (H,), "model.5.weight": (C, H),
            "model.5.bias": (C,)}


def autograd_transition(cur, x, lab, gen):
    """One HMC transition with unit mass in torch autograd: the same arithmetic as the kernels' chain (L gradient evaluations: the potential
    and gradient of the current position are carried in `cur` = (q, U, grad) as the chain caches them), eager ops, no host read."""
    def U(p):
        h = torch.nn.functional.leaky_relu(x @ p["model.1.weight"].T + p["model.1.bias"])
        h = torch.nn.functional.leaky_relu(h @ p["model.3.weight"].T + p["model.3.bias"])
        z = h @ p["model.5.weight"].T + p["model.5.bias"]
        return torch.nn.functional.cross_entropy(z, lab, reduction="sum") + 0.5 * sum((v * v).sum() for v in p.values())

    def grad(p):
        p = {k: v.detach().requires_grad_(True) for k, v in p.items()}
        u = U(p)
        return u.detach(), dict(zip(p, torch.autograd.grad(u, list(p.values()))))

    q, u0, g = cur if cur[1] is not None else (cur[0],) + grad(cur[0])
    g0 = g
    r = {k: torch.randn(v.shape, device=v.device, generator=gen) for k, v in q.items()}
    k0 = 0.5 * sum((v * v).sum() for v in r.values())
    p = q
    for _ in range(L):
        r = {k: r[k] - 0.5 * EPS * g[k] for k in r}
        p = {k: p[k] + EPS * r[k] for k in p}
        u1, g = grad(p)
        r = {k: r[k] - 0.5 * EPS * g[k] for k in r}
    dH = (u1 + 0.5 * sum((v * v).sum() for v in r.values())) - (u0 + k0)
    acc = torch.rand((), device=dH.device, generator=gen) < torch.exp(-dH).clamp(max=1.0)
    return ({k: torch.where(acc, p[k], q[k]) for k in q}, torch.where(acc, u1, u0), {k: torch.where(acc, g[k], g0[k]) for k in q})


def timed(fn, reps, n):
    def block():
        for _ in range(n):
            fn()
    out = [ms / n for ms in blocks(block, reps, warmup=fn)]
    return {"median_ms": statistics.median(out), "min_ms": out[0], "max_ms": out[-1]}


CHAIN_SHAPES = [("fc2", 2, 32, 2, 1024), ("fc2", 2, 512, 2, 1024)]


def chains_main(a):
    """K chains in lockstep against K single chains one after the other: the same L, step size, batch and start positions on both sides."""
    from robustbnns_amd.hmc import HmcSampler, LockstepHmc
    dev, K = "cuda:0", a.chains
    for arch, D, H, C, B in CHAIN_SHAPES:
        g = torch.Generator().manual_seed(0)
        q0s = [{k: 0.1 * torch.randn(*s, generator=g) for k, s in shapes_of(D, H, C).items()} for _ in range(K)]
        x, lab = torch.rand(B, D, generator=g).to(dev), torch.randint(0, C, (B,), generator=g).to(dev)
        singles = [HmcSampler(arch, "leaky", (1, D, 1), C, q0s[k], EPS, L, dev, 1 + k, adapt_step_size=False, batch_size=B) for k in range(K)]
        for s in singles:
            s.stage(x, lab)
        ls = LockstepHmc(arch, "leaky", (1, D, 1), C, q0s, EPS, L, dev, list(range(1, 1 + K)), adapt_step_size=False, batch_size=B)
        ls.set_data(x, lab)
        ls.stage()
        state = {"i": 0, "j": 0}

        def serial_step():
            for s in singles:
                s.transition(state["i"], L)
            state["i"] += 1

        def lockstep_step():
            ls.transition(state["j"], L)
            state["j"] += 1

        serial, lock = timed(serial_step, a.reps, a.n), timed(lockstep_step, a.reps, a.n)
        same = all(torch.equal(ls.q_cur[k], singles[k].q_cur) for k in range(K))       # both sides ran the same number of transitions
        tps = lambda t: 1e3 * K / t["median_ms"]
        print(json.dumps({"shape": f"{arch} {D}->{H}->{H}->{C} B={B} L={L}", "chains": K, "serial": serial, "lockstep": lock,
                          "serial_chain_transitions_per_s": tps(serial), "lockstep_chain_transitions_per_s": tps(lock),
                          "ratio": serial["median_ms"] / lock["median_ms"], "chains_bit_identical": same}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--chains", type=int, default=0, help="K > 0: K chains in lockstep against K consecutive single chains")
    a = ap.parse_args()
    G.build()
    if a.chains > 0:
        return chains_main(a)
    from robustbnns_amd.hmc import HmcSampler
    dev = "cuda:0"
    for arch, D, H, C, B in SHAPES:
        g = torch.Generator().manual_seed(0)
        q0 = {k: 0.1 * torch.randn(*s, generator=g) for k, s in shapes_of(D, H, C).items()}
        x, lab = torch.rand(B, D, generator=g).to(dev), torch.randint(0, C, (B,), generator=g).to(dev)
        s = HmcSampler(arch, "leaky", (1, D, 1), C, q0, EPS, L, dev, 1, adapt_step_size=False, batch_size=B)
        s.stage(x, lab)
        state = {"i": 0}

        def hip_step():
            s.transition(state["i"], L)
            state["i"] += 1

        hip = timed(hip_step, a.reps, a.n)
        gen = torch.Generator(device=dev).manual_seed(0)
        cur = {"s": ({k: v.to(dev) for k, v in q0.items()}, None, None)}

        def torch_step():
            cur["s"] = autograd_transition(cur["s"], x, lab, gen)

        ref = timed(torch_step, a.reps, a.n)
        print(json.dumps({"shape": f"{arch} {D}->{H}->{H}->{C} B={B} L={L}", "n_params": s.n_params, "hip": hip, "torch_autograd": ref,
                          "speedup_median": ref["median_ms"] / hip["median_ms"]}), flush=True)


if __name__ == "__main__":
    main()
