"""Time deterministic training (robustbnns_amd.nn_train.NnTrainer) on synthetic MNIST-shaped data (60 000 x 784) for the reference's fc2-512
(model_5, lr 0.01) and fc2-1024 (model_7, lr 0.02): lockstep steps of M = 1, 10, 100 members at batch 100 (Ensemble_NN.train), next to the
same trainer at M = 1 called once per member (what training the members one after the other costs in this build) and to a plain
torch-autograd member step on the same GPU, and NN.train's own M = 1 step at batch 64.  timing.py's protocol: device events; after --warmup
steps, --blocks blocks of --steps steps each: a figure is the median block in ms per step, its noise the spread (max - min) / median beside it.
One JSON line per net.

    python tools/nn_train_timing.py [--steps N] [--nets 512,1024] [--members 1,10,100]

Every net is measured in a child process of its own through timing.cases (its log under <OUT>/nn_train_timing/).  --child --nets H: the
measuring program itself (what to put behind `rocprofv3 --kernel-trace --stats --`, with --steps 20 --torch-steps 0 --members 100 --blocks 1)."""
import argparse

import torch

import timing as T
import torch_baselines as TB

DEV = "cuda:0"


def figure(ms, steps, key, spread_key):
    s = T.summary(ms, steps)
    return {key: s["median"], spread_key: s["spread"]}


def timed(fn, steps, warm, blocks):
    def block():
        for i in range(steps):
            fn(i)
    return T.blocks(block, blocks, warmup=warm)


def measure(H, members, steps, warmup, torch_steps, shape=(1, 28, 28), C=10, N=60000, B=100, blocks=T.BLOCKS):
    from robustbnns_amd.model_nn import saved_NNs
    from robustbnns_amd.nn_train import NnTrainer
    D = shape[0] * shape[1] * shape[2]
    g = torch.Generator(device=DEV).manual_seed(0)
    X, Y = TB.images(N, C, DEV, shape, g)
    lr = {512: saved_NNs["model_5"]["lr"], 1024: saved_NNs["model_7"]["lr"]}.get(H, 0.01)
    torch.manual_seed(0)
    member = lambda: {k: (torch.rand(s) * 2 - 1) / (s[-1] ** 0.5) for k, s in TB.fc2_shapes(D, H, C)}
    res = {"net": f"fc2-{H}", "lr": lr, "batch": B, "steps": steps, "blocks": blocks}
    one = NnTrainer("fc2", "leaky", shape, C, [member()], lr, DEV, batch_size=B)
    one.set_data(X, Y)
    for M in members:
        tr = NnTrainer("fc2", "leaky", shape, C, [member() for _ in range(M)], lr, DEV, batch_size=B)
        tr.set_data(X, Y)
        sched = torch.stack([torch.randperm(N, device=DEV, generator=g) for _ in range(M)]).to(torch.int32)
        rows = [sched[:, (i * B) % (N - B):(i * B) % (N - B) + B].contiguous() for i in range(steps)]

        def warm():
            for i in range(warmup):
                tr.step(rows=rows[i % steps])
                one.step(rows=rows[i % steps][:1])

        def sequential(i):
            for m in range(M):
                one.step(rows=rows[i][m:m + 1])
        lock = figure(timed(lambda i: tr.step(rows=rows[i]), steps, warm, blocks), steps, "lockstep_ms_per_step", "lockstep_spread")
        seq = figure(timed(sequential, max(1, steps // max(1, M // 10)), warm, blocks), max(1, steps // max(1, M // 10)),
                     "sequential_ms_per_step", "sequential_spread")
        ms, sq = lock["lockstep_ms_per_step"], seq["sequential_ms_per_step"]
        res[f"M={M}"] = {**lock, "lockstep_ms_per_member_step": ms / M, **seq, "sequential_ms_per_member_step": sq / M, "gain": sq / ms}
        del tr
    x64, y64 = X[:64], Y[:64]

    def warm64():
        for i in range(warmup):
            one.step(x64, y64)
    res.update(figure(timed(lambda i: one.step(x64, y64), steps, warm64, blocks), steps, "nn_train_batch64_ms_per_step", "nn_train_batch64_spread"))
    if torch_steps:
        W = {k: v.to(DEV).requires_grad_(True) for k, v in member().items()}
        opt = torch.optim.Adam(list(W.values()), lr=lr)
        xb, yb = X[:B], Y[:B]
        forward = lambda W, x: TB.logits("fc2", W, x)
        step = lambda i: TB.adam_member_step(forward, W, opt, xb, yb)
        res.update(figure(timed(step, torch_steps, lambda: [step(i) for i in range(warmup)], blocks), torch_steps,
                          "torch_autograd_ms_per_member_step", "torch_autograd_spread"))
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=T.BLOCKS, help="timed blocks")
    ap.add_argument("--torch-steps", type=int, default=200)
    ap.add_argument("--nets", default="512,1024")
    ap.add_argument("--members", default="1,10,100")
    ap.add_argument("--child", action="store_true", help="measure ONE net in this process (what the runner starts)")
    a = ap.parse_args(argv)
    if a.child:
        return T.child(lambda: measure(int(a.nets), [int(v) for v in a.members.split(",")], a.steps, a.warmup, a.torch_steps, blocks=a.blocks))
    T.cases("nn_train_timing", __file__, [(f"fc2_{H}", ["--nets", H] + T.opts(a, "members", "steps", "warmup", "blocks", "torch_steps"))
                                          for H in a.nets.split(",")], "nn_train_timing")


if __name__ == "__main__":
    main()
