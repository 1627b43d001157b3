"""Time SVI training of conv guides (robustbnns_amd.conv_svi_train.ConvSviTrainer) on synthetic MNIST-shaped data at batch 128 for conv-512
(model_0) and conv-1024 (model_2 / 4 / 8), with and without the accuracy forward, next to a plain torch-autograd restatement of the same step
on the same GPU (w = loc + softplus(raw) eps, the six layers by torch.nn.functional, sum CE + KL, backward, torch.optim.Adam; its accuracy
forward: 10 more weight sets and forwards under no_grad).  svi_train_timing.py's protocol: device events; after one warm-up block, 7 blocks of
--steps steps each: the figure is the median block in ms per step, its noise the spread (max - min) / median.

    python tools/conv_svi_train_timing.py [--nets 512,1024] [--steps 40] [--torch 1]

Every net is measured in a child process of its own, started through steps.Runner (one time limit each; after a fault, an abort or a time
limit nothing more is started); the child's JSON line is printed and kept in its log under <OUT>/conv_svi_timing/.  --child: the measuring
program itself (what to put behind `rocprofv3 --kernel-trace --stats --`, with --steps 5 --torch 0).

    python tools/conv_svi_train_timing.py --members 1,8,32 [--nets 512,1024] [--steps 40]

times the lockstep step of K conv guides (ConvLockstepSvi, B = 128) at each K against that many ConvSviTrainers stepped one after the other on
the same rows in the same process, in guide-steps per second, with and without the accuracy forward; every (net, K, accuracy) is measured
in a child of its own through the same runner, its log under <OUT>/conv_svi_lockstep_timing/.  --child --members K --accuracy 0|1 --torch 0:
the lockstep side alone (for a kernel trace)."""
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
ACC_SAMPLES = 10


def shapes_of(Hc, Cn):
    return [("model.0.weight", (32, 1, 5, 5)), ("model.0.bias", (32,)), ("model.3.weight", (Hc, 32, 5, 5)), ("model.3.bias", (Hc,)),
            ("model.7.weight", (Cn, 49 * Hc)), ("model.7.bias", (Cn,))]


def torch_logits(W, x):
    h = F.max_pool2d(F.leaky_relu(F.conv2d(x, W[KEYS[0]], W[KEYS[1]])), 2)
    h = F.max_pool2d(F.leaky_relu(F.conv2d(h, W[KEYS[2]], W[KEYS[3]])), 2, stride=1)
    return h.flatten(1) @ W[KEYS[4]].T + W[KEYS[5]]


def torch_step(loc, raw, opt, x, y, accuracy):
    opt.zero_grad(set_to_none=True)
    W, kl = {}, 0.0
    for k in KEYS:
        sig = F.softplus(raw[k])
        W[k] = loc[k] + sig * torch.randn_like(sig)
        kl = kl + ((-torch.log(sig) + 0.5 * (sig * sig + loc[k] * loc[k])) - 0.5).sum()
    loss = F.cross_entropy(torch_logits(W, x), y, reduction="sum") + kl
    loss.backward()
    opt.step()
    if accuracy:
        with torch.no_grad():
            p = 0.0
            for _ in range(ACC_SAMPLES):
                p = p + torch.softmax(torch_logits({k: loc[k] + F.softplus(raw[k]) * torch.randn_like(raw[k]) for k in KEYS}, x), -1)
            return (p.argmax(-1) == y).sum()


def child(a):
    from robustbnns_amd.conv_svi_train import ConvSviTrainer
    dev, B, Cn, steps = "cuda:0", 128, 10, a.steps
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.rand(steps * B, 1, 28, 28, device=dev, generator=g)
    Y = torch.randint(0, Cn, (steps * B,), device=dev, generator=g)
    batch = lambda i: (X[i * B:(i + 1) * B], Y[i * B:(i + 1) * B])
    for Hc in (int(v) for v in a.nets.split(",")):
        g = torch.Generator().manual_seed(0)
        loc = {k: 0.05 * torch.randn(*s, generator=g) for k, s in shapes_of(Hc, Cn)}
        raw = {k: -3.0 + 0.5 * torch.randn(*s, generator=g) for k, s in shapes_of(Hc, Cn)}
        tr = ConvSviTrainer("leaky", (1, 28, 28), Cn, loc, raw, 0.01, dev, 0x1234, batch_size=B)
        res = {"net": f"conv-{Hc}", "batch": B, "steps_per_block": steps, "blocks": 7}
        for acc in (True, False):
            def block():
                for i in range(steps):
                    tr.step(*batch(i), accuracy=acc)
            ms = _blocks(block)
            res["with_accuracy" if acc else "no_accuracy"] = {"ms_per_step": ms[3] / steps, "spread": (ms[-1] - ms[0]) / ms[3]}
        del tr
        torch.cuda.empty_cache()
        if a.torch:
            tl = {k: v.to(dev).clone().requires_grad_(True) for k, v in loc.items()}
            traw = {k: v.to(dev).clone().requires_grad_(True) for k, v in raw.items()}
            opt = torch.optim.Adam(list(tl.values()) + list(traw.values()), lr=0.01)
            for acc in (True, False):
                def torch_block():
                    for i in range(steps):
                        torch_step(tl, traw, opt, *batch(i), acc)
                tm = _blocks(torch_block)
                key = "with_accuracy" if acc else "no_accuracy"
                res["torch_autograd_" + key] = {"ms_per_step": tm[3] / steps, "spread": (tm[-1] - tm[0]) / tm[3]}
                res["torch_over_this_" + key] = tm[3] / steps / res[key]["ms_per_step"]
            del tl, traw, opt
            torch.cuda.empty_cache()
        print(json.dumps(res), flush=True)


def members_child(a):
    """One net, one K, with or without the accuracy forward: ConvLockstepSvi's step at B = 128 on rows of 4096 resident points, against K
    ConvSviTrainers stepped one after the other on the same rows in this process (the single guide's code: the baseline).  The figure is
    guide-steps per second from the median block."""
    from robustbnns_amd.conv_svi_train import ConvLockstepSvi, ConvSviTrainer
    dev, B, Cn, steps, N = "cuda:0", 128, 10, a.steps, 4096
    Hc, K, acc = int(a.nets), int(a.members), bool(a.accuracy)
    g = torch.Generator().manual_seed(0)
    X, Y = torch.rand(N, 1, 28, 28, generator=g), torch.randint(0, Cn, (N,), generator=g)
    rows = torch.randint(0, N, (steps, K, B), generator=g, dtype=torch.int32).to(dev)
    locs = [{k: 0.05 * torch.randn(*s, generator=g) for k, s in shapes_of(Hc, Cn)} for _ in range(K)]
    raws = [{k: -3.0 + 0.5 * torch.randn(*s, generator=g) for k, s in shapes_of(Hc, Cn)} for _ in range(K)]
    res = {"net": f"conv-{Hc}", "guides": K, "batch": B, "accuracy": acc, "steps_per_block": steps, "blocks": 7}
    tr = ConvLockstepSvi("leaky", (1, 28, 28), Cn, locs, raws, 0.01, dev, [0x1234 + k for k in range(K)], batch_size=B)
    tr.set_data(X, Y)

    def block():
        for i in range(steps):
            tr.step(rows[i], accuracy=acc)
    ms = _blocks(block)
    res["lockstep"] = {"ms_per_step": ms[3] / steps, "spread": (ms[-1] - ms[0]) / ms[3], "guide_steps_per_s": 1e3 * K * steps / ms[3]}
    res["launches_per_step"] = tr.launches // tr.t
    del tr
    torch.cuda.empty_cache()
    if not a.torch:                                    # (--torch 0 skips the other side here too: the lockstep step alone, for a kernel trace)
        return print(json.dumps(res), flush=True)
    Xd, Yd = X.to(dev), Y.to(dev)
    singles = [ConvSviTrainer("leaky", (1, 28, 28), Cn, locs[k], raws[k], 0.01, dev, 0x1234 + k, batch_size=B) for k in range(K)]
    idx = rows.long()

    def single_block():
        for i in range(steps):
            for k, one in enumerate(singles):
                one.step(Xd[idx[i, k]], Yd[idx[i, k]], accuracy=acc)
    sm = _blocks(single_block)
    res["one_after_the_other"] = {"ms_per_step": sm[3] / steps, "spread": (sm[-1] - sm[0]) / sm[3], "guide_steps_per_s": 1e3 * K * steps / sm[3]}
    res["lockstep_over_sequential"] = sm[3] / ms[3]
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", default="512,1024")
    ap.add_argument("--steps", type=int, default=40, help="steps per timed block")
    ap.add_argument("--torch", type=int, default=1, help="0: skip the torch-autograd side")
    ap.add_argument("--child", action="store_true", help="measure in this process (what the runner starts, one net at a time)")
    ap.add_argument("--members", default="", help="e.g. 1,8,32: time ConvLockstepSvi at these guide counts instead")
    ap.add_argument("--accuracy", type=int, default=1, help="with --members --child: 0 = without the accuracy forward")
    a = ap.parse_args()
    if a.members and a.child:
        return members_child(a)
    if a.members:
        # every (net, K, accuracy) in a child process of its own through the checked runner: one time limit each, nothing more started after a failure
        runner = S.Runner("conv_svi_lockstep_timing")
        for Hc in a.nets.split(","):
            for K in a.members.split(","):
                for acc in ("1", "0"):
                    text = runner.gpu("timing", f"conv{Hc}_k{K}_acc{acc}", [S.PY, os.path.abspath(__file__), "--child", "--nets", Hc, "--members", K,
                                                                            "--accuracy", acc, "--steps", str(a.steps), "--torch", str(a.torch)])
                    print(json.dumps(S.last_json(text)), flush=True)
        return
    if a.child:
        return child(a)
    runner = S.Runner("conv_svi_timing")
    for Hc in a.nets.split(","):
        text = runner.gpu("timing", f"conv{Hc}", [S.PY, os.path.abspath(__file__), "--child", "--nets", Hc, "--steps", str(a.steps), "--torch", str(a.torch)])
        print(json.dumps(S.last_json(text)), flush=True)


if __name__ == "__main__":
    main()
