"""Time deterministic training (robustbnns_amd.nn_train.NnTrainer) on synthetic MNIST-shaped data (60 000 x 784) for the reference's fc2-512
(model_5, lr 0.01) and fc2-1024 (model_7, lr 0.02): lockstep steps of M = 1, 10, 100 members at batch 100 (Ensemble_NN.train), next to the
same trainer at M = 1 called once per member (what training the members one after the other costs in this build) and to a plain
torch-autograd member step on the same GPU, and NN.train's own M = 1 step at batch 64.  Device events, after a warm-up.  One JSON line per net.

    python tools/nn_train_timing.py [--steps N] [--nets 512,1024] [--members 1,10,100]

Under `rocprofv3 --kernel-trace --stats` use a short run (--steps 20 --torch-steps 0 --members 100 --nets 512)."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from timing import block_ms                         # noqa: E402


def timed(fn, steps):
    def block():
        for i in range(steps):
            fn(i)
    return block_ms(block) / steps


def torch_step(W, opt, x, y):
    opt.zero_grad(set_to_none=True)
    h = F.leaky_relu(x @ W[0].T + W[1])
    h = F.leaky_relu(h @ W[2].T + W[3])
    F.cross_entropy(h @ W[4].T + W[5], y).backward()
    opt.step()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--torch-steps", type=int, default=200)
    ap.add_argument("--nets", default="512,1024")
    ap.add_argument("--members", default="1,10,100")
    a = ap.parse_args()
    from robustbnns_amd.model_nn import saved_NNs
    from robustbnns_amd.nn_train import NnTrainer
    dev = "cuda:0"
    N, B, D, C = 60000, 100, 784, 10
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.rand(N, 1, 28, 28, device=dev, generator=g)
    Y = torch.randint(0, C, (N,), device=dev, generator=g)
    lrs = {512: saved_NNs["model_5"]["lr"], 1024: saved_NNs["model_7"]["lr"]}
    for H in (int(v) for v in a.nets.split(",")):
        lr = lrs.get(H, 0.01)
        shapes = [("model.1.weight", (H, D)), ("model.1.bias", (H,)), ("model.3.weight", (H, H)), ("model.3.bias", (H,)),
                  ("model.5.weight", (C, H)), ("model.5.bias", (C,))]
        torch.manual_seed(0)
        member = lambda: {k: (torch.rand(s) * 2 - 1) / (s[-1] ** 0.5) for k, s in shapes}
        res = {"net": f"fc2-{H}", "lr": lr, "batch": B, "steps": a.steps}
        one = NnTrainer("fc2", "leaky", (1, 28, 28), C, [member()], lr, dev, batch_size=B)
        one.set_data(X, Y)
        for M in (int(v) for v in a.members.split(",")):
            tr = NnTrainer("fc2", "leaky", (1, 28, 28), C, [member() for _ in range(M)], lr, dev, batch_size=B)
            tr.set_data(X, Y)
            sched = torch.stack([torch.randperm(N, device=dev, generator=g) for _ in range(M)]).to(torch.int32)
            rows = [sched[:, (i * B) % (N - B):(i * B) % (N - B) + B].contiguous() for i in range(a.steps)]
            for i in range(a.warmup):
                tr.step(rows=rows[i % a.steps])
                one.step(rows=rows[i % a.steps][:1])
            torch.cuda.synchronize()
            ms = timed(lambda i: tr.step(rows=rows[i]), a.steps)

            def sequential(i):
                for m in range(M):
                    one.step(rows=rows[i][m:m + 1])
            seq = timed(sequential, max(1, a.steps // max(1, M // 10)))
            res[f"M={M}"] = {"lockstep_ms_per_step": ms, "lockstep_ms_per_member_step": ms / M, "sequential_ms_per_step": seq,
                             "sequential_ms_per_member_step": seq / M, "gain": seq / ms}
            del tr
        x64, y64 = X[:64], Y[:64]
        for i in range(a.warmup):
            one.step(x64, y64)
        torch.cuda.synchronize()
        res["nn_train_batch64_ms_per_step"] = timed(lambda i: one.step(x64, y64), a.steps)
        if a.torch_steps:
            W = [v.to(dev).requires_grad_(True) for v in member().values()]
            opt = torch.optim.Adam(W, lr=lr)
            xb, yb = X[:B].reshape(B, -1), Y[:B]
            for i in range(a.warmup):
                torch_step(W, opt, xb, yb)
            torch.cuda.synchronize()
            res["torch_autograd_ms_per_member_step"] = timed(lambda i: torch_step(W, opt, xb, yb), a.torch_steps)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
