"""Time HMC over conv nets (robustbnns_amd.conv_hmc.ConvHmcSampler) on synthetic MNIST-shaped data at the reference's HMC batch, B = 5000
(model_bnn.py:403), for conv-512 and conv-1024: chain-transitions per second and ms per leapfrog step at L = 10, fixed step size, unit mass
(the sampling phase: no adaptation, no host reads), next to a plain torch-autograd HMC transition on the same GPU in the same process (the
six layers by torch.nn.functional, sum CE + 1/2 sum q^2, torch.autograd.grad, eager element-wise updates; hmc_timing.py's transition).
conv_svi_train_timing.py's protocol: device events; after one warm-up block, 7 blocks of --n transitions each: the figure is the median
block, its noise the spread (max - min) / median.

    python tools/conv_hmc_timing.py [--nets 512,1024] [--n 2] [--batch 5000] [--torch 1] [--chains 1,8]

--chains 1,8: instead, K chains behind every launch (robustbnns_amd.conv_hmc.ConvLockstepHmc) against K ConvHmcSamplers stepped one after the
other in the same process, the same protocol, in chain-transitions per second (K transitions a launch set).  K is cut to what
conv_hmc_chains_group allows for the batch (the RBNN_CONV_WS_GB budget); the line says which K was measured.

Every net (with --chains: every net and K) is measured in a child process of its own, started through steps.Runner (one time limit each;
after a fault, an abort or a time limit nothing more is started); the child's JSON line is printed and kept in its log under
<OUT>/conv_hmc_timing/.  --child: the measuring program itself (what to put behind `rocprofv3 --kernel-trace --stats --`, with --n 1 --torch 0)."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import steps as S                                  # noqa: E402
from timing import blocks as _blocks               # noqa: E402

KEYS = [k + s for k in ("model.0", "model.3", "model.7") for s in (".weight", ".bias")]
L, EPS = 10, 1e-5


def shapes_of(Hc, Cn):
    return [("model.0.weight", (32, 1, 5, 5)), ("model.0.bias", (32,)), ("model.3.weight", (Hc, 32, 5, 5)), ("model.3.bias", (Hc,)),
            ("model.7.weight", (Cn, 49 * Hc)), ("model.7.bias", (Cn,))]


def torch_grad(p, x, y):
    """(U, dU/dq) of U = sum CE + 1/2 sum q^2 at p by torch autograd."""
    p = {k: v.detach().requires_grad_(True) for k, v in p.items()}
    h = F.max_pool2d(F.leaky_relu(F.conv2d(x, p[KEYS[0]], p[KEYS[1]])), 2)
    h = F.max_pool2d(F.leaky_relu(F.conv2d(h, p[KEYS[2]], p[KEYS[3]])), 2, stride=1)
    z = h.flatten(1) @ p[KEYS[4]].T + p[KEYS[5]]
    u = F.cross_entropy(z, y, reduction="sum") + 0.5 * sum((v * v).sum() for v in p.values())
    return u.detach(), dict(zip(p, torch.autograd.grad(u, list(p.values()))))


def torch_transition(cur, x, y, gen):
    """One HMC transition with unit mass in torch autograd: L gradient evaluations (the potential and gradient of the current position are
    carried in `cur` = (q, U, grad), as the chain caches them), eager ops, no host read."""
    q, u0, g = cur if cur[1] is not None else (cur[0],) + torch_grad(cur[0], x, y)
    g0 = g
    r = {k: torch.randn(v.shape, device=v.device, generator=gen) for k, v in q.items()}
    k0 = 0.5 * sum((v * v).sum() for v in r.values())
    p = q
    for _ in range(L):
        r = {k: r[k] - 0.5 * EPS * g[k] for k in r}
        p = {k: p[k] + EPS * r[k] for k in p}
        u1, g = torch_grad(p, x, y)
        r = {k: r[k] - 0.5 * EPS * g[k] for k in r}
    dH = (u1 + 0.5 * sum((v * v).sum() for v in r.values())) - (u0 + k0)
    acc = torch.rand((), device=dH.device, generator=gen) < torch.exp(-dH).clamp(max=1.0)
    return ({k: torch.where(acc, p[k], q[k]) for k in q}, torch.where(acc, u1, u0), {k: torch.where(acc, g[k], g0[k]) for k in q})


def figures(ms, n):
    per = ms[len(ms) // 2] / n
    return {"ms_per_transition": per, "ms_per_leapfrog_step": per / L, "chain_transitions_per_s": 1e3 / per, "spread": (ms[-1] - ms[0]) / ms[len(ms) // 2]}


def child(a):
    from robustbnns_amd.conv_hmc import ConvHmcSampler
    dev, B, Cn, n = "cuda:0", a.batch, 10, a.n
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(B, 1, 28, 28, device=dev, generator=g)
    y = torch.randint(0, Cn, (B,), device=dev, generator=g)
    for Hc in (int(v) for v in a.nets.split(",")):
        g = torch.Generator().manual_seed(0)
        q0 = {k: 0.05 * torch.randn(*s, generator=g) for k, s in shapes_of(Hc, Cn)}
        s = ConvHmcSampler("leaky", (1, 28, 28), Cn, q0, EPS, L, dev, 0x1234, adapt_step_size=False, batch_size=B)
        s.stage(x, y)
        state = {"i": 0}

        def block():
            for _ in range(n):
                s.transition(state["i"], L)
                state["i"] += 1
        n0 = s.launches
        ms = _blocks(block)
        res = {"net": f"conv-{Hc}", "batch": B, "L": L, "n_params": s.n_params, "transitions_per_block": n, "blocks": 7,
               "launches_per_transition": (s.launches - n0) // (8 * n), "this": figures(ms, n)}
        del s
        torch.cuda.empty_cache()
        if a.torch:
            gen = torch.Generator(device=dev).manual_seed(0)
            cur = {"s": ({k: v.to(dev) for k, v in q0.items()}, None, None)}

            def torch_block():
                for _ in range(n):
                    cur["s"] = torch_transition(cur["s"], x, y, gen)
            res["torch_autograd"] = figures(_blocks(torch_block), n)
            res["torch_over_this"] = res["torch_autograd"]["ms_per_transition"] / res["this"]["ms_per_transition"]
            del cur
            torch.cuda.empty_cache()
        print(json.dumps(res), flush=True)


def chains_child(a):
    """One (net, K): K ConvHmcSamplers stepped one after the other, then (their memory freed) one ConvLockstepHmc of the same K chains."""
    from robustbnns_amd.conv_hmc import ConvHmcSampler, ConvLockstepHmc, conv_hmc_chains_group
    dev, B, Cn, n, asked = "cuda:0", a.batch, 10, a.n, int(a.chains)
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(B, 1, 28, 28, device=dev, generator=g)
    y = torch.randint(0, Cn, (B,), device=dev, generator=g)
    for Hc in (int(v) for v in a.nets.split(",")):
        K = conv_hmc_chains_group("leaky", Hc, Cn, asked, B)
        g = torch.Generator().manual_seed(0)
        q0s = [{k: 0.05 * torch.randn(*s, generator=g) for k, s in shapes_of(Hc, Cn)} for _ in range(K)]
        keys = [0x1234 + k for k in range(K)]
        state = {"i": 0}
        singles = [ConvHmcSampler("leaky", (1, 28, 28), Cn, q0s[k], EPS, L, dev, keys[k], adapt_step_size=False, batch_size=B) for k in range(K)]
        for s in singles:
            s.stage(x, y)

        def one_after_the_other():
            for _ in range(n):
                for s in singles:
                    s.transition(state["i"], L)
                state["i"] += 1
        apart = figures(_blocks(one_after_the_other), n * K)
        n_params = singles[0].n_params
        del singles
        torch.cuda.empty_cache()
        ls = ConvLockstepHmc("leaky", (1, 28, 28), Cn, q0s, EPS, L, dev, keys, adapt_step_size=False, batch_size=B)
        ls.set_data(x, y)
        ls.stage()
        state["i"] = 0

        def together():
            for _ in range(n):
                ls.transition(state["i"], L)
                state["i"] += 1
        n0 = ls.launches
        ms = _blocks(together)
        res = {"net": f"conv-{Hc}", "batch": B, "L": L, "n_params": n_params, "chains_asked": asked, "chains": K, "transitions_per_block": n,
               "blocks": 7, "launches_per_transition": (ls.launches - n0) // (8 * n), "lockstep": figures(ms, n * K), "one_after_the_other": apart}
        res["lockstep_over_apart"] = res["lockstep"]["chain_transitions_per_s"] / apart["chain_transitions_per_s"]
        del ls
        torch.cuda.empty_cache()
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", default="512,1024")
    ap.add_argument("--n", type=int, default=2, help="transitions per timed block")
    ap.add_argument("--batch", type=int, default=5000)
    ap.add_argument("--torch", type=int, default=1, help="0: skip the torch-autograd side")
    ap.add_argument("--child", action="store_true", help="measure in this process (what the runner starts, one net at a time)")
    ap.add_argument("--chains", default="", help="e.g. 1,8: time K chains behind every launch against K single chains one after the other")
    a = ap.parse_args()
    if a.child:
        return chains_child(a) if a.chains else child(a)
    runner = S.Runner("conv_hmc_timing")
    for Hc in a.nets.split(","):
        for K in (a.chains.split(",") if a.chains else ()):
            text = runner.gpu("timing", f"conv{Hc}_k{K}", [S.PY, os.path.abspath(__file__), "--child", "--nets", Hc, "--n", str(a.n), "--batch",
                                                         str(a.batch), "--chains", K])
            print(json.dumps(S.last_json(text)), flush=True)
        if a.chains:
            continue
        text = runner.gpu("timing", f"conv{Hc}", [S.PY, os.path.abspath(__file__), "--child", "--nets", Hc, "--n", str(a.n), "--batch", str(a.batch),
                                                  "--torch", str(a.torch)])
        print(json.dumps(S.last_json(text)), flush=True)


if __name__ == "__main__":
    main()
