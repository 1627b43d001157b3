"""Time SVI training (robustbnns_amd.svi_train.SviTrainer) on synthetic MNIST-shaped data (60 000 x 784, batch 128) for the reference's
fc2-512 (model_5, lr 0.01) and fc2-1024 (model_7, lr 0.02), next to a plain torch-autograd restatement of the same step on the same GPU
(w = loc + softplus(raw) eps, sum CE + KL, backward, torch.optim.Adam).  Device events, after a warm-up.  Prints one JSON line per net.

    python tools/svi_train_timing.py [--steps-per-epoch N] [--nets 512,1024]
    python tools/svi_train_timing.py --members 1,8,32 [--nets 32,512] [--steps 40]

--members K: K guides of one net shape in lockstep (svi_train.LockstepSvi, every launch covers all K) against K consecutive SviTrainer runs of
the same steps in the same process: fc2-32 on half-moons-shaped data (batch 64) and fc2-512 on MNIST-shaped data (batch 128), with and without
the accuracy forward.  After one warm-up block, 7 blocks of --steps steps each are timed with device events; a figure is the median block in
member-steps per second, its noise the spread (max - min) / median over the 7 blocks.  One JSON line per (net, K).

Under `rocprofv3 --kernel-trace --stats` use a short run (--steps-per-epoch 20 --torch-steps 0) and count launches per step from the trace."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from timing import block_ms, blocks as _blocks     # noqa: E402


def torch_step(params, opt, x, y):
    opt.zero_grad(set_to_none=True)
    keys = list(params)
    W = {}
    kl = 0.0
    for i in range(0, len(keys), 2):
        loc, raw = params[keys[i]], params[keys[i + 1]]
        sig = F.softplus(raw)
        W[keys[i]] = loc + sig * torch.randn_like(loc)
        kl = kl + ((-torch.log(sig) + 0.5 * (sig * sig + loc * loc)) - 0.5).sum()
    h = x
    names = [k for k in keys[::2]]
    for j in range(0, len(names), 2):
        h = h @ W[names[j]].T + W[names[j + 1]]
        if j + 2 < len(names):
            h = F.leaky_relu(h)
    loss = F.cross_entropy(h, y, reduction="sum") + kl
    loss.backward()
    opt.step()


def members_main(a):
    from robustbnns_amd.svi_train import LockstepSvi, SviTrainer, initial_params
    dev, steps = "cuda:0", a.steps
    for H in (int(v) for v in a.nets.split(",")):
        moons = H < 128
        shape, D, C, B, lr = ((1, 2, 1), 2, 2, 64, 0.05) if moons else ((1, 28, 28), 784, 10, 128, 0.01)
        N = steps * B
        g = torch.Generator(device=dev).manual_seed(0)
        X = torch.rand(N, *shape, device=dev, generator=g) * (4 if moons else 1) - (2 if moons else 0)
        Y = torch.randint(0, C, (N,), device=dev, generator=g)
        shapes = [("model.1.weight", (H, D)), ("model.1.bias", (H,)), ("model.3.weight", (H, H)), ("model.3.bias", (H,)),
                  ("model.5.weight", (C, H)), ("model.5.bias", (C,))]
        for K in (int(v) for v in a.members.split(",")):
            torch.manual_seed(0)
            inits = [initial_params(shapes) for _ in range(K)]
            ls = LockstepSvi("fc2", "leaky", shape, C, [i[0] for i in inits], [i[1] for i in inits], [lr] * K, dev, list(range(1, K + 1)), batch_size=B)
            ls.set_data(X, Y)
            ls.load_schedule(LockstepSvi.schedule([N] * K, [1] * K, B))
            trainers = [SviTrainer("fc2", "leaky", shape, C, inits[k][0], inits[k][1], lr, dev, k + 1, batch_size=B) for k in range(K)]
            res = {"net": f"fc2-{H}", "batch": B, "members": K, "steps_per_block": steps, "blocks": 7}
            for acc in (True, False):
                def lock_block():
                    for t in range(steps):
                        ls.scheduled_step(t, acc)

                def serial_block():
                    for tr in trainers:
                        for t in range(steps):
                            tr.step(X[t * B:(t + 1) * B], Y[t * B:(t + 1) * B], accuracy=acc)
                lock, serial = _blocks(lock_block), _blocks(serial_block)
                rate = lambda ms: K * steps / (ms / 1e3)
                res["with_accuracy" if acc else "no_accuracy"] = {
                    "lockstep_member_steps_per_s": rate(lock[3]), "lockstep_spread": (lock[-1] - lock[0]) / lock[3],
                    "serial_member_steps_per_s": rate(serial[3]), "serial_spread": (serial[-1] - serial[0]) / serial[3],
                    "lockstep_over_serial": serial[3] / lock[3]}
            print(json.dumps(res), flush=True)
            del ls, trainers
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", default="", help="e.g. 1,8,32: time K guides in lockstep against K consecutive trainers (see the module docstring)")
    ap.add_argument("--steps", type=int, default=40, help="--members: steps per timed block")
    ap.add_argument("--steps-per-epoch", type=int, default=0, help="0: the whole epoch (60000 / 128 = 469 steps)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--torch-steps", type=int, default=200)
    ap.add_argument("--nets", default="512,1024")
    a = ap.parse_args()
    if a.members:
        if a.nets == "512,1024":
            a.nets = "32,512"
        return members_main(a)
    from robustbnns_amd.model_bnn import saved_BNNs
    from robustbnns_amd.svi_train import SviTrainer, initial_params
    dev = "cuda:0"
    N, B, D, C = 60000, 128, 784, 10
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.rand(N, 1, 28, 28, device=dev, generator=g)
    Y = torch.randint(0, C, (N,), device=dev, generator=g)
    steps = a.steps_per_epoch or (N + B - 1) // B
    lrs = {512: saved_BNNs["model_5"][1]["lr"], 1024: saved_BNNs["model_7"][1]["lr"]}
    for H in (int(v) for v in a.nets.split(",")):
        lr = lrs[H]
        shapes = [("model.1.weight", (H, D)), ("model.1.bias", (H,)), ("model.3.weight", (H, H)), ("model.3.bias", (H,)),
                  ("model.5.weight", (C, H)), ("model.5.bias", (C,))]
        torch.manual_seed(0)
        loc, raw = initial_params(shapes)
        tr = SviTrainer("fc2", "leaky", (1, 28, 28), C, loc, raw, lr, dev, 0x1234, batch_size=B)
        batch = lambda i: (X[(i * B) % N:(i * B) % N + B], Y[(i * B) % N:(i * B) % N + B])
        for i in range(a.warmup):
            tr.step(*batch(i))
        torch.cuda.synchronize()
        res = {"net": f"fc2-{H}", "lr": lr, "batch": B, "steps": steps}
        for acc in (True, False):
            def hip_block():
                for i in range(steps):
                    tr.step(*batch(i), accuracy=acc)
            ms = block_ms(hip_block)
            key = "with_accuracy" if acc else "no_accuracy"
            res[key] = {"ms_per_step": ms / steps, "ms_per_epoch_469": ms / steps * ((N + B - 1) // B)}
        if a.torch_steps:
            params = {}
            for k, s in shapes:
                params[k + "_loc"] = loc[k].to(dev).clone().requires_grad_(True)
                params[k + "_scale"] = raw[k].to(dev).clone().requires_grad_(True)
            opt = torch.optim.Adam(list(params.values()), lr=lr)
            for i in range(a.warmup):
                torch_step(params, opt, X[i * B:(i + 1) * B].reshape(B, -1), Y[i * B:(i + 1) * B])
            torch.cuda.synchronize()

            def torch_block():
                for i in range(a.torch_steps):
                    xb, yb = batch(i)
                    torch_step(params, opt, xb.reshape(B, -1), yb)
            ms = block_ms(torch_block) / a.torch_steps
            res["torch_autograd_no_accuracy"] = {"ms_per_step": ms, "ms_per_epoch_469": ms * ((N + B - 1) // B)}
            res["speedup_no_accuracy"] = ms / res["no_accuracy"]["ms_per_step"]
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
