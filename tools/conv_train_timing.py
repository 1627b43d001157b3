"""Time deterministic conv training (robustbnns_amd.conv_train.ConvNnTrainer) on synthetic MNIST-shaped data at batch 128 for conv-512
(model_0) and conv-1024 (model_9), next to a torch-autograd step of the same net on the same GPU (an nn.Sequential of the six layers,
nn.CrossEntropyLoss, torch.optim.Adam).  timing.py's protocol: device events; after one warm-up block, --blocks blocks of --steps steps each:
the figure is the median block in ms per step, its noise the spread (max - min) / median.  The same blocks are then timed per entry point
(forward + head, weight gradients, Adam, finalize).  Prints one JSON line per net.

    python tools/conv_train_timing.py [--nets 512,1024] [--steps 40] [--torch 1]

    python tools/conv_train_timing.py --members 1,8,32 [--nets 512,1024] [--steps 40]

times the lockstep step of a conv ensemble (ConvEnsembleTrainer, B = 100) at each member count against that many ConvNnTrainers stepped one
after the other in the same process, in member-steps per second.  Every net (with --members: every (net, M)) is measured in a child process
of its own through timing.cases, and its JSON line is printed and kept in its log under <OUT>/conv_train_timing/ or
<OUT>/conv_ensemble_timing/.  --child: the measuring program itself (what to put behind `rocprofv3 --kernel-trace --stats --`, with --steps 5
--torch 0: the per-launch breakdown is the trace's; with --members, the lockstep side alone)."""
import argparse
import ctypes as C

import torch
from torch import nn

import timing as T
import torch_baselines as TB

DEV, CN = "cuda:0", 10


def figure(ms, steps, M=None):
    s = T.summary(ms, steps)
    return {"ms_per_step": s["median"], "spread": s["spread"], **({"member_steps_per_s": 1e3 * M / s["median"]} if M else {})}


def sequential(Hc, seed):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Conv2d(1, 32, 5), nn.LeakyReLU(), nn.MaxPool2d(2), nn.Conv2d(32, Hc, 5), nn.LeakyReLU(), nn.MaxPool2d(2, stride=1),
                         nn.Flatten(), nn.Linear(49 * Hc, CN))


def state(seq):
    return {"model." + k: v for k, v in seq.state_dict().items()}


def measure_members(Hc, M, steps, with_torch, B=100, N=4000, blocks=T.BLOCKS):
    """One net, one member count M: ConvEnsembleTrainer's lockstep step at B = 100 (model_ensemble.py:73) on rows of 4000 resident points,
    against M ConvNnTrainers stepped one after the other on the same rows in this process (the single net's code: the baseline).  The figure
    is member-steps per second from the median block."""
    from robustbnns_amd.conv_train import ConvEnsembleTrainer, ConvNnTrainer
    g = torch.Generator().manual_seed(0)
    X, Y = torch.rand(N, 1, 28, 28, generator=g), torch.randint(0, CN, (N,), generator=g)
    rows = torch.randint(0, N, (steps, M, B), generator=g, dtype=torch.int32).to(DEV)
    params = [state(sequential(Hc, k)) for k in range(M)]
    res = {"net": f"conv-{Hc}", "members": M, "batch": B, "steps_per_block": steps, "blocks": blocks}
    tr = ConvEnsembleTrainer("leaky", (1, 28, 28), CN, params, 0.01, DEV, batch_size=B)
    tr.set_data(X, Y)

    def block():
        for i in range(steps):
            tr.step(rows=rows[i])
    res["lockstep"] = figure(T.blocks(block, blocks), steps, M)
    del tr
    torch.cuda.empty_cache()
    if not with_torch:                                 # (--torch 0 skips the other side here too: the lockstep step alone, for a kernel trace)
        return res
    Xd, Yd = X.to(DEV), Y.to(DEV)
    singles = [ConvNnTrainer("leaky", (1, 28, 28), CN, p, 0.01, DEV, batch_size=B) for p in params]
    idx = rows.long()

    def single_block():
        for i in range(steps):
            for k, one in enumerate(singles):
                one.step(Xd[idx[i, k]], Yd[idx[i, k]])
    res["one_after_the_other"] = figure(T.blocks(single_block, blocks), steps, M)
    res["lockstep_over_sequential"] = res["one_after_the_other"]["ms_per_step"] / res["lockstep"]["ms_per_step"]
    return res


def measure(Hc, steps, with_torch, B=128, blocks=T.BLOCKS):
    from robustbnns_amd import _hip
    from robustbnns_amd.conv_train import ADAM_EPS, BETAS, ConvNnTrainer
    X, Y = TB.images(steps * B, CN, DEV)
    batch = lambda i: (X[i * B:(i + 1) * B], Y[i * B:(i + 1) * B])
    seq = sequential(Hc, 0)
    tr = ConvNnTrainer("leaky", (1, 28, 28), CN, state(seq), 0.01, DEV, batch_size=B)

    def block():
        for i in range(steps):
            tr.step(*batch(i))
    this = figure(T.blocks(block, blocks), steps)
    res = {"net": f"conv-{Hc}", "batch": B, "steps_per_block": steps, "blocks": blocks, **this}
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
        res["ms_per_entry_point"][name] = T.summary(T.blocks(part_block, blocks), steps)["median"]
    if with_torch:
        seq = seq.to(DEV)
        opt = torch.optim.Adam(seq.parameters(), lr=0.01)
        loss_fn = nn.CrossEntropyLoss()

        def torch_block():
            for i in range(steps):
                xb, yb = batch(i)
                opt.zero_grad(set_to_none=True)
                loss_fn(seq(xb), yb).backward()
                opt.step()
        res["torch_autograd"] = figure(T.blocks(torch_block, blocks), steps)
        res["torch_over_this"] = res["torch_autograd"]["ms_per_step"] / this["ms_per_step"]
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", default="512,1024")
    ap.add_argument("--steps", type=int, default=40, help="steps per timed block")
    ap.add_argument("--blocks", type=int, default=T.BLOCKS, help="timed blocks")
    ap.add_argument("--torch", type=int, default=1, help="0: skip the torch-autograd side")
    ap.add_argument("--members", default="", help="e.g. 1,8,32: time ConvEnsembleTrainer at these member counts instead, B = 100")
    ap.add_argument("--child", action="store_true", help="measure ONE net (and ONE member count) in this process (what the runner starts)")
    a = ap.parse_args(argv)
    if a.child:
        return T.child(lambda: measure_members(int(a.nets), int(a.members), a.steps, a.torch, blocks=a.blocks) if a.members
                       else measure(int(a.nets), a.steps, a.torch, blocks=a.blocks))
    common = T.opts(a, "steps", "blocks", "torch")
    if a.members:
        return T.cases("conv_ensemble_timing", __file__, [(f"conv{Hc}_m{M}", ["--nets", Hc, "--members", M] + common)
                                                          for Hc in a.nets.split(",") for M in a.members.split(",")])
    T.cases("conv_train_timing", __file__, [(f"conv{Hc}", ["--nets", Hc] + common) for Hc in a.nets.split(",")])


if __name__ == "__main__":
    main()
