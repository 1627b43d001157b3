"""Time SVI training (robustbnns_amd.svi_train.SviTrainer) on synthetic MNIST-shaped data (60 000 x 784, batch 128) for the reference's
fc2-512 (model_5, lr 0.01) and fc2-1024 (model_7, lr 0.02), next to a plain torch-autograd restatement of the same step on the same GPU
(torch_baselines.svi_step: w = loc + softplus(raw) eps, sum CE + KL, backward, torch.optim.Adam).  timing.py's protocol: device events; after
--warmup steps, --blocks blocks of one epoch's steps each: a figure is the median block in ms per step, its noise the spread
(max - min) / median beside it.  Prints one JSON line per net.

    python tools/svi_train_timing.py [--steps-per-epoch N] [--nets 512,1024]
    python tools/svi_train_timing.py --members 1,8,32 [--nets 32,512] [--steps 40]

--members K: K guides of one net shape in lockstep (svi_train.LockstepSvi, every launch covers all K) against K consecutive SviTrainer runs of
the same steps in the same process: fc2-32 on half-moons-shaped data (batch 64) and fc2-512 on MNIST-shaped data (batch 128), with and without
the accuracy forward.  After one warm-up block, --blocks blocks of --steps steps each are timed; a figure is the median block in member-steps
per second, its noise the spread over the blocks.  One JSON line per (net, K).

Every net (with --members: every (net, K)) is measured in a child process of its own through timing.cases (its log under
<OUT>/svi_train_timing/).  --child --nets H: the measuring program itself (what to put behind `rocprofv3 --kernel-trace --stats --`, with
--steps-per-epoch 20 --torch-steps 0 --blocks 1; count launches per step from the trace)."""
import argparse

import torch

import timing as T
import torch_baselines as TB

DEV = "cuda:0"


def measure_members(H, K, steps, blocks=T.BLOCKS):
    from robustbnns_amd.svi_train import LockstepSvi, SviTrainer, initial_params
    moons = H < 128
    shape, D, C, B, lr = ((1, 2, 1), 2, 2, 64, 0.05) if moons else ((1, 28, 28), 784, 10, 128, 0.01)
    N = steps * B
    X, Y = TB.images(N, C, DEV, shape)
    X = X * (4 if moons else 1) - (2 if moons else 0)
    torch.manual_seed(0)
    inits = [initial_params(TB.fc2_shapes(D, H, C)) for _ in range(K)]
    ls = LockstepSvi("fc2", "leaky", shape, C, [i[0] for i in inits], [i[1] for i in inits], [lr] * K, DEV, list(range(1, K + 1)), batch_size=B)
    ls.set_data(X, Y)
    ls.load_schedule(LockstepSvi.schedule([N] * K, [1] * K, B))
    trainers = [SviTrainer("fc2", "leaky", shape, C, inits[k][0], inits[k][1], lr, DEV, k + 1, batch_size=B) for k in range(K)]
    res = {"net": f"fc2-{H}", "batch": B, "members": K, "steps_per_block": steps, "blocks": blocks}
    for acc in (True, False):
        def lock_block():
            for t in range(steps):
                ls.scheduled_step(t, acc)

        def serial_block():
            for tr in trainers:
                for t in range(steps):
                    tr.step(X[t * B:(t + 1) * B], Y[t * B:(t + 1) * B], accuracy=acc)
        lock, serial = T.summary(T.blocks(lock_block, blocks)), T.summary(T.blocks(serial_block, blocks))
        rate = lambda s: K * steps / (s["median"] / 1e3)
        res["with_accuracy" if acc else "no_accuracy"] = {
            "lockstep_member_steps_per_s": rate(lock), "lockstep_spread": lock["spread"],
            "serial_member_steps_per_s": rate(serial), "serial_spread": serial["spread"], "lockstep_over_serial": serial["median"] / lock["median"]}
    return res


def measure(H, steps, warmup, torch_steps, shape=(1, 28, 28), C=10, N=60000, B=128, blocks=T.BLOCKS):
    """steps: of a timed block (0: one epoch, ceil(N / B))."""
    from robustbnns_amd.model_bnn import saved_BNNs
    from robustbnns_amd.svi_train import SviTrainer, initial_params
    X, Y = TB.images(N, C, DEV, shape)
    epoch = (N + B - 1) // B
    steps = steps or epoch
    lr = {512: saved_BNNs["model_5"][1]["lr"], 1024: saved_BNNs["model_7"][1]["lr"]}.get(H, 0.01)
    torch.manual_seed(0)
    loc, raw = initial_params(TB.fc2_shapes(shape[0] * shape[1] * shape[2], H, C))
    tr = SviTrainer("fc2", "leaky", shape, C, loc, raw, lr, DEV, 0x1234, batch_size=B)
    batch = lambda i: (X[(i * B) % N:(i * B) % N + B], Y[(i * B) % N:(i * B) % N + B])

    def figure(step, n):
        def block():
            for i in range(n):
                step(i)
        s = T.summary(T.blocks(block, blocks, warmup=lambda: [step(i) for i in range(warmup)]), n)
        return {"ms_per_step": s["median"], "ms_per_epoch_469": s["median"] * epoch, "spread": s["spread"]}
    res = {"net": f"fc2-{H}", "lr": lr, "batch": B, "steps": steps, "blocks": blocks}
    for acc in (True, False):
        res["with_accuracy" if acc else "no_accuracy"] = figure(lambda i: tr.step(*batch(i), accuracy=acc), steps)
    if torch_steps:
        tl, traw, opt = TB.svi_parameters(loc, raw, lr, DEV)
        forward = lambda W, x: TB.logits("fc2", W, x)
        res["torch_autograd_no_accuracy"] = figure(lambda i: TB.svi_step(forward, tl, traw, opt, *batch(i)), torch_steps)
        res["speedup_no_accuracy"] = res["torch_autograd_no_accuracy"]["ms_per_step"] / res["no_accuracy"]["ms_per_step"]
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", default="", help="e.g. 1,8,32: time K guides in lockstep against K consecutive trainers (see the module docstring)")
    ap.add_argument("--steps", type=int, default=40, help="--members: steps per timed block")
    ap.add_argument("--steps-per-epoch", type=int, default=0, help="0: the whole epoch (60000 / 128 = 469 steps)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=T.BLOCKS, help="timed blocks")
    ap.add_argument("--torch-steps", type=int, default=200)
    ap.add_argument("--nets", default="512,1024", help="with --members, the default is 32,512")
    ap.add_argument("--child", action="store_true", help="measure ONE net (and ONE K) in this process (what the runner starts)")
    a = ap.parse_args(argv)
    if a.child:
        return T.child(lambda: measure_members(int(a.nets), int(a.members), a.steps, a.blocks) if a.members
                       else measure(int(a.nets), a.steps_per_epoch, a.warmup, a.torch_steps, blocks=a.blocks))
    nets = ("32,512" if a.members and a.nets == "512,1024" else a.nets).split(",")
    if a.members:
        return T.cases("svi_train_timing", __file__, [(f"fc2_{H}_k{K}", ["--nets", H, "--members", K] + T.opts(a, "steps", "blocks"))
                                                      for H in nets for K in a.members.split(",")], "svi_train_timing")
    T.cases("svi_train_timing", __file__, [(f"fc2_{H}", ["--nets", H] + T.opts(a, "steps_per_epoch", "warmup", "blocks", "torch_steps"))
                                           for H in nets], "svi_train_timing")


if __name__ == "__main__":
    main()
