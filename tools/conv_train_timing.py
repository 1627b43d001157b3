"""Time deterministic conv training (robustbnns_amd.conv_train.ConvNnTrainer) on synthetic MNIST-shaped data at batch 128 for conv-512
(model_0) and conv-1024 (model_9), next to a torch-autograd step of the same net on the same GPU (an nn.Sequential of the six layers,
nn.CrossEntropyLoss, torch.optim.Adam).  Device events; after one warm-up block, 7 blocks of --steps steps each: the figure is the median
block in ms per step, its noise the spread (max - min) / median.  The same blocks are then timed per entry point (forward + head, weight
gradients, Adam, finalize).  Prints one JSON line per net.

    python tools/conv_train_timing.py [--nets 512,1024] [--steps 40] [--torch 1]

Under `rocprofv3 --kernel-trace --stats` use a short run (--steps 5 --torch 0): the per-launch breakdown is the trace's.

    python tools/conv_train_timing.py --members 1,8,32 [--nets 512,1024] [--steps 40]

times the lockstep step of a conv ensemble (ConvEnsembleTrainer, B = 100) at each member count against that many ConvNnTrainers stepped one
after the other in the same process, in member-steps per second; every (net, M) is measured in a child process of its own, started through
steps.Runner (one time limit each; after a fault, an abort or a time limit nothing more is started), and its JSON line is printed and kept in
its log under <OUT>/conv_ensemble_timing/.  --child: the measuring program itself (what to put behind `rocprofv3 --kernel-trace --stats --`,
with --steps 5 --torch 0: the lockstep side alone)."""
import argparse
import ctypes as C
import json
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import steps as S                                  # noqa: E402
from timing import blocks as _blocks               # noqa: E402


def members_child(a):
    """One net, one member count M: ConvEnsembleTrainer's lockstep step at B = 100 (model_ensemble.py:73) on rows of 4000 resident points,
    against M ConvNnTrainers stepped one after the other on the same rows in this process (the single net's code: the baseline).  The figure
    is member-steps per second from the median block."""
    from robustbnns_amd.conv_train import ConvEnsembleTrainer, ConvNnTrainer
    dev, B, Cn, steps, N = "cuda:0", 100, 10, a.steps, 4000
    Hc, M = int(a.nets), int(a.members)
    g = torch.Generator().manual_seed(0)
    X, Y = torch.rand(N, 1, 28, 28, generator=g), torch.randint(0, Cn, (N,), generator=g)
    rows = torch.randint(0, N, (steps, M, B), generator=g, dtype=torch.int32).to(dev)
    params = []
    for k in range(M):
        torch.manual_seed(k)
        seq = nn.Sequential(nn.Conv2d(1, 32, 5), nn.LeakyReLU(), nn.MaxPool2d(2), nn.Conv2d(32, Hc, 5), nn.LeakyReLU(), nn.MaxPool2d(2, stride=1),
                            nn.Flatten(), nn.Linear(49 * Hc, Cn))
        params.append({"model." + k2: v for k2, v in seq.state_dict().items()})
    res = {"net": f"conv-{Hc}", "members": M, "batch": B, "steps_per_block": steps, "blocks": 7}
    tr = ConvEnsembleTrainer("leaky", (1, 28, 28), Cn, params, 0.01, dev, batch_size=B)
    tr.set_data(X, Y)

    def block():
        for i in range(steps):
            tr.step(rows=rows[i])
    ms = _blocks(block)
    res["lockstep"] = {"ms_per_step": ms[3] / steps, "spread": (ms[-1] - ms[0]) / ms[3], "member_steps_per_s": 1e3 * M * steps / ms[3]}
    del tr
    torch.cuda.empty_cache()
    if not a.torch:                                    # (--torch 0 skips the other side here too: the lockstep step alone, for a kernel trace)
        return print(json.dumps(res), flush=True)
    Xd, Yd = X.to(dev), Y.to(dev)
    singles = [ConvNnTrainer("leaky", (1, 28, 28), Cn, p, 0.01, dev, batch_size=B) for p in params]
    idx = rows.long()

    def single_block():
        for i in range(steps):
            for k, one in enumerate(singles):
                one.step(Xd[idx[i, k]], Yd[idx[i, k]])
    sm = _blocks(single_block)
    res["one_after_the_other"] = {"ms_per_step": sm[3] / steps, "spread": (sm[-1] - sm[0]) / sm[3], "member_steps_per_s": 1e3 * M * steps / sm[3]}
    res["lockstep_over_sequential"] = sm[3] / ms[3]
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", default="512,1024")
    ap.add_argument("--steps", type=int, default=40, help="steps per timed block")
    ap.add_argument("--torch", type=int, default=1, help="0: skip the torch-autograd side")
    ap.add_argument("--members", default="", help="e.g. 1,8,32: time ConvEnsembleTrainer at these member counts instead, B = 100")
    ap.add_argument("--child", action="store_true", help="with --members: measure ONE net and ONE member count in this process (what the runner starts)")
    a = ap.parse_args()
    if a.members and a.child:
        return members_child(a)
    if a.members:
        # every (net, M) in a child process of its own through the checked runner: one time limit each, nothing more started after a failure
        runner = S.Runner("conv_ensemble_timing")
        for Hc in a.nets.split(","):
            for M in a.members.split(","):
                text = runner.gpu("timing", f"conv{Hc}_m{M}", [S.PY, os.path.abspath(__file__), "--child", "--nets", Hc, "--members", M, "--steps", str(a.steps),
                                                               "--torch", str(a.torch)])
                print(json.dumps(S.last_json(text)), flush=True)
        return
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
