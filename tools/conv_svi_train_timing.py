"""Time SVI training of conv guides (robustbnns_amd.conv_svi_train.ConvSviTrainer) on synthetic MNIST-shaped data at batch 128 for conv-512
(model_0) and conv-1024 (model_2 / 4 / 8), with and without the accuracy forward, next to a plain torch-autograd restatement of the same step
on the same GPU (torch_baselines.svi_step over the six layers by torch.nn.functional; its accuracy forward: 10 more weight sets and forwards
under no_grad).  timing.py's protocol: device events; after one warm-up block, --blocks blocks of --steps steps each: the figure is the median
block in ms per step, its noise the spread (max - min) / median.

    python tools/conv_svi_train_timing.py [--nets 512,1024] [--steps 40] [--torch 1]

Every net is measured in a child process of its own through timing.cases; the child's JSON line is printed and kept in its log under
<OUT>/conv_svi_timing/.  --child: the measuring program itself (what to put behind `rocprofv3 --kernel-trace --stats --`, with --steps 5
--torch 0).

    python tools/conv_svi_train_timing.py --members 1,8,32 [--nets 512,1024] [--steps 40]

times the lockstep step of K conv guides (ConvLockstepSvi, B = 128) at each K against that many ConvSviTrainers stepped one after the other on
the same rows in the same process, in guide-steps per second, with and without the accuracy forward; every (net, K, accuracy) is measured
in a child of its own, its log under <OUT>/conv_svi_lockstep_timing/.  --child --members K --accuracy 0|1 --torch 0: the lockstep side alone
(for a kernel trace)."""
import argparse

import torch

import timing as T
import torch_baselines as TB

DEV, CN = "cuda:0", 10


def figure(ms, steps, K=None):
    s = T.summary(ms, steps)
    return {"ms_per_step": s["median"], "spread": s["spread"], **({"guide_steps_per_s": 1e3 * K / s["median"]} if K else {})}


def guide(Hc, g):
    return TB.normal_weights(TB.conv_shapes(Hc, CN), 0.05, g), TB.normal_weights(TB.conv_shapes(Hc, CN), 0.5, g, shift=-3.0)


def measure(Hc, steps, with_torch, B=128, blocks=T.BLOCKS):
    from robustbnns_amd.conv_svi_train import ConvSviTrainer
    X, Y = TB.images(steps * B, CN, DEV)
    batch = lambda i: (X[i * B:(i + 1) * B], Y[i * B:(i + 1) * B])
    loc, raw = guide(Hc, torch.Generator().manual_seed(0))
    tr = ConvSviTrainer("leaky", (1, 28, 28), CN, loc, raw, 0.01, DEV, 0x1234, batch_size=B)
    res = {"net": f"conv-{Hc}", "batch": B, "steps_per_block": steps, "blocks": blocks}
    for acc in (True, False):
        def block():
            for i in range(steps):
                tr.step(*batch(i), accuracy=acc)
        res["with_accuracy" if acc else "no_accuracy"] = figure(T.blocks(block, blocks), steps)
    del tr
    torch.cuda.empty_cache()
    if with_torch:
        tl, traw, opt = TB.svi_parameters(loc, raw, 0.01, DEV)
        forward = lambda W, x: TB.logits("conv", W, x)
        for acc in (True, False):
            def torch_block():
                for i in range(steps):
                    TB.svi_step(forward, tl, traw, opt, *batch(i), acc)
            key = "with_accuracy" if acc else "no_accuracy"
            res["torch_autograd_" + key] = figure(T.blocks(torch_block, blocks), steps)
            res["torch_over_this_" + key] = res["torch_autograd_" + key]["ms_per_step"] / res[key]["ms_per_step"]
    return res


def measure_members(Hc, K, acc, steps, with_torch, B=128, N=4096, blocks=T.BLOCKS):
    """One net, one K, with or without the accuracy forward: ConvLockstepSvi's step at B = 128 on rows of 4096 resident points, against K
    ConvSviTrainers stepped one after the other on the same rows in this process (the single guide's code: the baseline).  The figure is
    guide-steps per second from the median block."""
    from robustbnns_amd.conv_svi_train import ConvLockstepSvi, ConvSviTrainer
    g = torch.Generator().manual_seed(0)
    X, Y = torch.rand(N, 1, 28, 28, generator=g), torch.randint(0, CN, (N,), generator=g)
    rows = torch.randint(0, N, (steps, K, B), generator=g, dtype=torch.int32).to(DEV)
    locs = [TB.normal_weights(TB.conv_shapes(Hc, CN), 0.05, g) for _ in range(K)]
    raws = [TB.normal_weights(TB.conv_shapes(Hc, CN), 0.5, g, shift=-3.0) for _ in range(K)]
    res = {"net": f"conv-{Hc}", "guides": K, "batch": B, "accuracy": acc, "steps_per_block": steps, "blocks": blocks}
    tr = ConvLockstepSvi("leaky", (1, 28, 28), CN, locs, raws, 0.01, DEV, [0x1234 + k for k in range(K)], batch_size=B)
    tr.set_data(X, Y)

    def block():
        for i in range(steps):
            tr.step(rows[i], accuracy=acc)
    res["lockstep"] = figure(T.blocks(block, blocks), steps, K)
    res["launches_per_step"] = tr.launches // tr.t
    del tr
    torch.cuda.empty_cache()
    if not with_torch:                                 # (--torch 0 skips the other side here too: the lockstep step alone, for a kernel trace)
        return res
    Xd, Yd = X.to(DEV), Y.to(DEV)
    singles = [ConvSviTrainer("leaky", (1, 28, 28), CN, locs[k], raws[k], 0.01, DEV, 0x1234 + k, batch_size=B) for k in range(K)]
    idx = rows.long()

    def single_block():
        for i in range(steps):
            for k, one in enumerate(singles):
                one.step(Xd[idx[i, k]], Yd[idx[i, k]], accuracy=acc)
    res["one_after_the_other"] = figure(T.blocks(single_block, blocks), steps, K)
    res["lockstep_over_sequential"] = res["one_after_the_other"]["ms_per_step"] / res["lockstep"]["ms_per_step"]
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", default="512,1024")
    ap.add_argument("--steps", type=int, default=40, help="steps per timed block")
    ap.add_argument("--blocks", type=int, default=T.BLOCKS, help="timed blocks")
    ap.add_argument("--torch", type=int, default=1, help="0: skip the torch-autograd side")
    ap.add_argument("--child", action="store_true", help="measure one net in this process (what the runner starts)")
    ap.add_argument("--members", default="", help="e.g. 1,8,32: time ConvLockstepSvi at these guide counts instead")
    ap.add_argument("--accuracy", type=int, default=1, help="with --members --child: 0 = without the accuracy forward")
    a = ap.parse_args(argv)
    if a.child:
        return T.child(lambda: measure_members(int(a.nets), int(a.members), bool(a.accuracy), a.steps, a.torch, blocks=a.blocks) if a.members
                       else measure(int(a.nets), a.steps, a.torch, blocks=a.blocks))
    common = T.opts(a, "steps", "blocks", "torch")
    if a.members:
        return T.cases("conv_svi_lockstep_timing", __file__, [(f"conv{Hc}_k{K}_acc{acc}", ["--nets", Hc, "--members", K, "--accuracy", acc] + common)
                                                              for Hc in a.nets.split(",") for K in a.members.split(",") for acc in ("1", "0")])
    T.cases("conv_svi_timing", __file__, [(f"conv{Hc}", ["--nets", Hc] + common) for Hc in a.nets.split(",")])


if __name__ == "__main__":
    main()
