"""Time HMC over conv nets (robustbnns_amd.conv_hmc.ConvHmcSampler) on synthetic MNIST-shaped data at the reference's HMC batch, B = 5000
(model_bnn.py:403), for conv-512 and conv-1024: chain-transitions per second and ms per leapfrog step at L = 10, fixed step size, unit mass
(the sampling phase: no adaptation, no host reads), next to a plain torch-autograd HMC transition on the same GPU in the same process
(torch_baselines: the six layers by torch.nn.functional, sum CE + 1/2 sum q^2, torch.autograd.grad, eager element-wise updates).
timing.py's protocol: device events; after one warm-up block, --blocks blocks of --n transitions each: the figure is the median block, its
noise the spread (max - min) / median.

    python tools/conv_hmc_timing.py [--nets 512,1024] [--n 2] [--batch 5000] [--torch 1] [--chains 1,8]

--chains 1,8: instead, K chains behind every launch (robustbnns_amd.conv_hmc.ConvLockstepHmc) against K ConvHmcSamplers stepped one after the
other in the same process, the same protocol, in chain-transitions per second (K transitions a launch set).  K is cut to what
conv_hmc_chains_group allows for the batch (the RBNN_CONV_WS_GB budget); the line says which K was measured.

Every net (with --chains: every net and K) is measured in a child process of its own through timing.cases; the child's JSON line is printed
and kept in its log under <OUT>/conv_hmc_timing/.  --child: the measuring program itself (what to put behind
`rocprofv3 --kernel-trace --stats --`, with --n 1 --torch 0)."""
import argparse

import torch

import timing as T
import torch_baselines as TB

L, EPS = 10, 1e-5
DEV, CN = "cuda:0", 10


def figures(ms, n):
    s = T.summary(ms, n)
    return {"ms_per_transition": s["median"], "ms_per_leapfrog_step": s["median"] / L, "chain_transitions_per_s": 1e3 / s["median"],
            "spread": s["spread"]}


def measure(Hc, B, n, with_torch, blocks=T.BLOCKS):
    from robustbnns_amd.conv_hmc import ConvHmcSampler
    x, y = TB.images(B, CN, DEV)
    q0 = TB.normal_weights(TB.conv_shapes(Hc, CN), 0.05, torch.Generator().manual_seed(0))
    s = ConvHmcSampler("leaky", (1, 28, 28), CN, q0, EPS, L, DEV, 0x1234, adapt_step_size=False, batch_size=B)
    s.stage(x, y)
    state = {"i": 0}

    def block():
        for _ in range(n):
            s.transition(state["i"], L)
            state["i"] += 1
    n0 = s.launches
    ms = T.blocks(block, blocks)
    res = {"net": f"conv-{Hc}", "batch": B, "L": L, "n_params": s.n_params, "transitions_per_block": n, "blocks": len(ms),
           "launches_per_transition": (s.launches - n0) // ((1 + len(ms)) * n), "this": figures(ms, n)}
    del s
    torch.cuda.empty_cache()
    if with_torch:
        gen, grad = torch.Generator(device=DEV).manual_seed(0), TB.potential_grad("conv", x, y)
        cur = {"s": ({k: v.to(DEV) for k, v in q0.items()}, None)}

        def torch_block():
            for _ in range(n):
                cur["s"] = TB.hmc_transition(grad, cur["s"], gen, L, EPS)
        res["torch_autograd"] = figures(T.blocks(torch_block, blocks), n)
        res["torch_over_this"] = res["torch_autograd"]["ms_per_transition"] / res["this"]["ms_per_transition"]
    return res


def measure_chains(Hc, asked, B, n, blocks=T.BLOCKS):
    """One (net, K): K ConvHmcSamplers stepped one after the other, then (their memory freed) one ConvLockstepHmc of the same K chains."""
    from robustbnns_amd.conv_hmc import ConvHmcSampler, ConvLockstepHmc, conv_hmc_chains_group
    x, y = TB.images(B, CN, DEV)
    K = conv_hmc_chains_group("leaky", Hc, CN, asked, B)
    g = torch.Generator().manual_seed(0)
    q0s = [TB.normal_weights(TB.conv_shapes(Hc, CN), 0.05, g) for _ in range(K)]
    keys = [0x1234 + k for k in range(K)]
    state = {"i": 0}
    singles = [ConvHmcSampler("leaky", (1, 28, 28), CN, q0s[k], EPS, L, DEV, keys[k], adapt_step_size=False, batch_size=B) for k in range(K)]
    for s in singles:
        s.stage(x, y)

    def one_after_the_other():
        for _ in range(n):
            for s in singles:
                s.transition(state["i"], L)
            state["i"] += 1
    apart = figures(T.blocks(one_after_the_other, blocks), n * K)
    n_params = singles[0].n_params
    del singles
    torch.cuda.empty_cache()
    ls = ConvLockstepHmc("leaky", (1, 28, 28), CN, q0s, EPS, L, DEV, keys, adapt_step_size=False, batch_size=B)
    ls.set_data(x, y)
    ls.stage()
    state["i"] = 0

    def together():
        for _ in range(n):
            ls.transition(state["i"], L)
            state["i"] += 1
    n0 = ls.launches
    ms = T.blocks(together, blocks)
    res = {"net": f"conv-{Hc}", "batch": B, "L": L, "n_params": n_params, "chains_asked": asked, "chains": K, "transitions_per_block": n,
           "blocks": len(ms), "launches_per_transition": (ls.launches - n0) // ((1 + len(ms)) * n), "lockstep": figures(ms, n * K),
           "one_after_the_other": apart}
    res["lockstep_over_apart"] = res["lockstep"]["chain_transitions_per_s"] / apart["chain_transitions_per_s"]
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", default="512,1024")
    ap.add_argument("--n", type=int, default=2, help="transitions per timed block")
    ap.add_argument("--batch", type=int, default=5000)
    ap.add_argument("--blocks", type=int, default=T.BLOCKS, help="timed blocks")
    ap.add_argument("--torch", type=int, default=1, help="0: skip the torch-autograd side")
    ap.add_argument("--child", action="store_true", help="measure one net (and one K) in this process (what the runner starts)")
    ap.add_argument("--chains", default="", help="e.g. 1,8: time K chains behind every launch against K single chains one after the other")
    a = ap.parse_args(argv)
    if a.child:
        return T.child(lambda: measure_chains(int(a.nets), int(a.chains), a.batch, a.n, a.blocks) if a.chains
                       else measure(int(a.nets), a.batch, a.n, a.torch, a.blocks))
    common = T.opts(a, "n", "batch", "blocks")
    T.cases("conv_hmc_timing", __file__, [(f"conv{Hc}_k{K}", ["--nets", Hc, "--chains", K] + common) if K else
                                          (f"conv{Hc}", ["--nets", Hc, "--torch", a.torch] + common)
                                          for Hc in a.nets.split(",") for K in (a.chains.split(",") if a.chains else [""])])


if __name__ == "__main__":
    main()
