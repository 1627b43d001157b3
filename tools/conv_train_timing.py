"""Time deterministic conv training (robustbnns_amd.conv_train.ConvNnTrainer) on synthetic MNIST-shaped data at batch 128 for conv-512
(model_0) and conv-1024 (model_9), next to a torch-autograd step of the same net on the same GPU (an nn.Sequential of the six layers,
nn.CrossEntropyLoss, torch.optim.Adam).  Device events; after one warm-up block, 7 blocks of --steps steps each: the figure is the median
block in ms per step, its noise the spread (max - min) / median.  The same blocks are then timed per entry point (forward + head, weight
gradients, Adam, finalize).  Prints one JSON line per net.

    python tools/conv_train_timing.py [--nets 512,1024] [--steps 40] [--torch 1]

Under `rocprofv3 --kernel-trace --stats` use a short run (--steps 5 --torch 0): the per-launch breakdown is the trace's."""
import argparse
import ctypes as C
import json
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from timing import blocks as _blocks               # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", default="512,1024")
    ap.add_argument("--steps", type=int, default=40, help="steps per timed block")
    ap.add_argument("--torch", type=int, default=1, help="0: skip the torch-autograd side")
    a = ap.parse_args()
    from robustbnns_amd import _hip
    from robustbnns_amd.conv_train import ADAM_EPS, BETAS, ConvNnTrainer
    dev, B, Cn, steps = "cuda:0", 128, 10, a.steps
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.rand(steps * B, 1, 28, 28, device=dev, generator=g)
    Y = torch.randint(0, Cn, (steps * B,), device=dev, generator=g)
    batch = lambda i: (X[i * B:(i + 1) * B], Y[i * B:(i + 1) * B])
    for Hc in (int(v) for v in a.nets.split(",")):
        torch.manual_seed(0)
        seq = nn.Sequential(nn.Conv2d(1, 32, 5), nn.LeakyReLU(), nn.MaxPool2d(2), nn.Conv2d(32, Hc, 5), nn.LeakyReLU(), nn.MaxPool2d(2, stride=1),
                            nn.Flatten(), nn.Linear(49 * Hc, Cn))
        tr = ConvNnTrainer("leaky", (1, 28, 28), Cn, {"model." + k: v for k, v in seq.state_dict().items()}, 0.01, dev, batch_size=B)

        def block():
            for i in range(steps):
                tr.step(*batch(i))
        ms = _blocks(block)
        res = {"net": f"conv-{Hc}", "batch": B, "steps_per_block": steps, "blocks": 7, "ms_per_step": ms[3] / steps, "spread": (ms[-1] - ms[0]) / ms[3]}
        # per entry point: the same calls, one entry point per timed block, on the state the steps above left
        lib, st, net, ws = tr.k.lib, _hip.stream_of(tr.P), C.byref(tr.net), C.byref(tr.ws)
        x, lab = _hip.ptr(tr.X), _hip.ptr(tr.labels)
        parts = {"forward_and_head": lambda: lib.rbnn_conv_train_forward(net, x, tr.Dp, lab, B, ws, st),
                 "weight_grads": lambda: lib.rbnn_conv_weight_grads(net, x, tr.Dp, B, ws, st),
                 "adam": lambda: lib.rbnn_conv_adam_step(net, tr.t + 1, tr.lr, BETAS[0], BETAS[1], ADAM_EPS, st),
                 "finalize": lambda: lib.rbnn_conv_train_finalize(ws, B, _hip.ptr(tr.stats), st)}
        res["ms_per_entry_point"] = {}
        for name, call in parts.items():
            def part_block():
                for _ in range(steps):
                    _hip.check(call(), name)
            pm = _blocks(part_block)
            res["ms_per_entry_point"][name] = pm[3] / steps
        if a.torch:
            seq = seq.to(dev)
            opt = torch.optim.Adam(seq.parameters(), lr=0.01)
            loss_fn = nn.CrossEntropyLoss()

            def torch_block():
                for i in range(steps):
                    xb, yb = batch(i)
                    opt.zero_grad(set_to_none=True)
                    loss_fn(seq(xb), yb).backward()
                    opt.step()
            tm = _blocks(torch_block)
            res["torch_autograd"] = {"ms_per_step": tm[3] / steps, "spread": (tm[-1] - tm[0]) / tm[3]}
            res["torch_over_this"] = tm[3] / ms[3]
        print(json.dumps(res), flush=True)
        del tr
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
