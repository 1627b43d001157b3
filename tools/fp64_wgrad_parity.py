#!/usr/bin/env python3
"""The fp32 weight gradients against the DEVICE fp64 ones at the sizes the project trains at, and what an fp64 pass costs.

    python tools/fp64_wgrad_parity.py [--cases 128x512,100x1024,5000x512,5000x1024] [--acts leaky,tanh] [--reps 5]
    python tools/fp64_wgrad_parity.py --nets fc [--cases fc2x512x128,fc2x1024x128,fc2x512x1024,fcx512x100] [--acts leaky,tanh] [--reps 5]

--nets conv (the default):

1x28x28, one net, C = 10, a freshly initialised stack (torch's default initialisation, seeded), torch.rand images, random labels.  Per
(B, Hc, activation) and per tensor, max |fp32 - fp64| / max |fp64| in units of 1e-5 against ConvFp64Engine.weight_gradients:
  - the mean-CE gradient of ConvNnTrainer.gradients (the deterministic trainer's step) against reduction='mean';
  - the summed-CE gradient of ConvSviTrainer.gradients (rbnn_conv_svi_weight_grads: the SVI step's and the HMC leapfrog's data gradient) at the
    weights it drew, against reduction='sum' at those weights, with the relative error of the fp32 summed CE (the data term of HMC's potential:
    the fp32 per-point values summed in fp64, as the sampler sums them) and the worst per-point CE error in units of 1e-5 max(1, CE);
  - the median time of one weight_gradients pass and of one fp32 gradients() pass of the SVI trainer (draw + forward + weight gradients), each
    over --reps passes, the device synchronised around every pass.
Nothing is excluded: at these sizes no point is free of a near pooling tie (profiles/fp64_conv/README.md), so a tensor whose figure is far
beyond 1 has met a flipped pooling maximum or activation side in fp32, which the figures of the other tensors show.
Every case is measured in a child process of its own, started through steps.Runner (kind bench_full: one time limit each; after a fault, an
abort or a time limit nothing more is started); the child's JSON line is kept in its log under <OUT>/fp64_wgrad_parity/.  --child: the
measuring process.

--nets fc: fc / fc2 nets on 1x28x28, one net, C = 10, torch's default initialisation (seeded), torch.rand images, random labels; a case is
ARCHxHIDDENxB.  SviTrainer.gradients (sigma = softplus(-5): the kernels of the SVI step and of HMC's potential gradient) at the weights it
drew against AttackEngine(precision='fp64').weight_gradients(reduction='sum') at those weights, NnTrainer.gradients against
reduction='mean'; the same figures and times, and per net the number of points whose oracle.kink_margin (fp64, on the CPU) is below
2e-6.  Nothing is excluded.  Its logs go to <OUT>/fp64_fc_wgrad_parity/."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import steps as S                                  # noqa: E402
from fp64_parity import timed                      # noqa: E402

BAR = 1e-5
SHAPE, CLASSES = (1, 28, 28), 10
KEYS = [k + s for k in ("model.0", "model.3", "model.7") for s in (".weight", ".bias")]


def fresh_params(act, Hc, seed):
    import torch
    from torch import nn
    a = {"relu": nn.ReLU, "leaky": nn.LeakyReLU, "sigm": nn.Sigmoid, "tanh": nn.Tanh}[act]
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        m = nn.Sequential(nn.Conv2d(1, 32, 5), a(), nn.MaxPool2d(2), nn.Conv2d(32, Hc, 5), a(), nn.MaxPool2d(2, 1), nn.Flatten(), nn.Linear(49 * Hc, CLASSES))
    return {"model." + k: v.detach().clone() for k, v in m.state_dict().items()}


def tensor_errs(G32, g64):
    """{key: max |fp32 - fp64| / max |fp64| in units of BAR} of one net's gradients (g64: row 0 of the engine's stack)."""
    return {k: float((G32[k].double().reshape(-1) - g64[k][0].reshape(-1)).abs().max() / g64[k][0].abs().max() / BAR) for k in KEYS}


def child(B, Hc, act, reps):
    import torch
    from robustbnns_amd.conv import ConvStackedPosterior
    from robustbnns_amd.conv_fp64 import ConvFp64Engine
    from robustbnns_amd.conv_svi_train import ConvSviTrainer
    from robustbnns_amd.conv_train import ConvNnTrainer
    dev = "cuda:0"
    params = fresh_params(act, Hc, 1000 * Hc + B)
    g = torch.Generator().manual_seed(B + Hc)
    x, lab = torch.rand(B, *SHAPE, generator=g).to(dev), torch.randint(0, CLASSES, (B,), generator=g).to(dev)
    engine = lambda p: ConvFp64Engine(ConvStackedPosterior(act, SHAPE, CLASSES, Hc, {k: p[k][None] for k in KEYS}, dev))
    rec = {"B": B, "Hc": Hc, "act": act, "bar": BAR, "device": torch.cuda.get_device_name(0)}
    # the deterministic trainer: mean CE
    tr = ConvNnTrainer(act, SHAPE, CLASSES, params, 1e-3, dev, batch_size=B)
    tr.gradients(x, lab)
    e64 = engine(params)
    rec["point_block"] = e64.wgrad_point_block(1)
    g64, ce64 = e64.weight_gradients(x, lab, 1, reduction="mean")
    rec["mean"] = tensor_errs(tr.unflat(tr.grad), g64)
    rec["mean_ce_worst_point"] = float(((tr.ws_t["ce"][:B].double() - ce64[0]).abs() / ce64[0].clamp_min(1.0)).max() / BAR)
    del tr, e64, g64
    # the SVI / HMC step's data gradient: summed CE at the drawn weights
    sv = ConvSviTrainer(act, SHAPE, CLASSES, params, {k: torch.full_like(v, -5.0) for k, v in params.items()}, 1e-3, dev, 0xC0FFEE, batch_size=B)
    sv.gradients(x, lab)
    drawn = {k: v.clone() for k, v in sv.unflat(sv.W).items()}
    e64 = engine(drawn)
    g64, ce64 = e64.weight_gradients(x, lab, 1)
    ce32 = sv.ws_t["ce"][:B].double()
    rec["sum"] = tensor_errs(sv.unflat(sv.grad), g64)
    rec["sum_ce_rel_err"] = float((ce32.sum() - ce64[0].sum()).abs() / ce64[0].sum())
    rec["sum_ce_worst_point"] = float(((ce32 - ce64[0]).abs() / ce64[0].clamp_min(1.0)).max() / BAR)
    rec["sum_ce_fp64"] = float(ce64[0].sum())
    del g64
    rec["fp64_pass_ms_median"], rec["fp64_pass_ms"] = timed(lambda: e64.weight_gradients(x, lab, 1), reps)
    rec["fp32_pass_ms_median"], rec["fp32_pass_ms"] = timed(lambda: sv.gradients(x, lab), reps)
    print(json.dumps(rec))


FC_DEFAULT = "fc2x512x128,fc2x1024x128,fc2x512x1024,fcx512x100"
KINK = 2e-6


def fc_keys(arch):
    return [k + s for k in (("model.1", "model.3") if arch == "fc" else ("model.1", "model.3", "model.5")) for s in (".weight", ".bias")]


def fc_fresh_params(arch, act, H, seed):
    import torch
    from torch import nn
    a = {"relu": nn.ReLU, "leaky": nn.LeakyReLU, "sigm": nn.Sigmoid, "tanh": nn.Tanh}[act]
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        mid = [nn.Linear(H, H), a()] if arch == "fc2" else []
        m = nn.Sequential(nn.Flatten(), nn.Linear(784, H), a(), *mid, nn.Linear(H, CLASSES))
    return {"model." + k: v.detach().clone() for k, v in m.state_dict().items()}


def fc_child(arch, H, B, act, reps):
    import torch
    from oracle import bnn_oracle as O
    from robustbnns_amd import AttackEngine, StackedPosterior
    from robustbnns_amd.nn_train import NnTrainer
    from robustbnns_amd.svi_train import SviTrainer
    dev, keys = "cuda:0", fc_keys(arch)
    params = fc_fresh_params(arch, act, H, 1000 * H + B)
    g = torch.Generator().manual_seed(B + H)
    x, lab = torch.rand(B, *SHAPE, generator=g), torch.randint(0, CLASSES, (B,), generator=g)
    xd, labd = x.to(dev), lab.to(dev)
    engine = lambda p: AttackEngine(StackedPosterior(arch, act, SHAPE, CLASSES, H, {k: p[k].detach().cpu()[None] for k in keys}, dev), precision="fp64")
    near_kink = lambda p: int((O.kink_margin(x.double(), {k: p[k].detach().cpu().double()[None] for k in keys}, arch, act, 1) < KINK).sum())
    errs = lambda G32, g64: {k: float((G32[k].double().reshape(-1) - g64[k][0].reshape(-1)).abs().max() / g64[k][0].abs().max() / BAR) for k in keys}
    rec = {"arch": arch, "H": H, "B": B, "act": act, "bar": BAR, "device": torch.cuda.get_device_name(0)}
    # the deterministic trainer: mean CE
    tr = NnTrainer(arch, act, SHAPE, CLASSES, params, 1e-3, dev, batch_size=B)
    tr.gradients(xd, labd)
    e64 = engine(params)
    rec["point_block"] = e64.fp64.point_block(1, 2)
    g64, ce64 = e64.weight_gradients(x, lab, 1, reduction="mean")
    rec["mean"] = errs(tr.unflat(tr.grad), g64)
    rec["mean_ce_worst_point"] = float(((tr.ws_t["ce"][:B].double() - ce64[0]).abs() / ce64[0].clamp_min(1.0)).max() / BAR)
    rec["mean_points_near_kink"] = near_kink(params)
    del tr, e64, g64
    # the SVI / HMC step's data gradient: summed CE at the drawn weights
    sv = SviTrainer(arch, act, SHAPE, CLASSES, params, {k: torch.full_like(v, -5.0) for k, v in params.items()}, 1e-3, dev, 0xC0FFEE, batch_size=B)
    sv.gradients(xd, labd)
    drawn = {k: v.clone() for k, v in sv.unflat(sv.W).items()}
    e64 = engine(drawn)
    g64, ce64 = e64.weight_gradients(x, lab, 1)
    ce32 = sv.ws_t["ce"][:B].double()
    rec["sum"] = errs(sv.unflat(sv.grad), g64)
    rec["sum_ce_rel_err"] = float((ce32.sum() - ce64[0].sum()).abs() / ce64[0].sum())
    rec["sum_ce_worst_point"] = float(((ce32 - ce64[0]).abs() / ce64[0].clamp_min(1.0)).max() / BAR)
    rec["sum_ce_fp64"] = float(ce64[0].sum())
    rec["sum_points_near_kink"] = near_kink(drawn)
    del g64
    rec["fp64_pass_ms_median"], rec["fp64_pass_ms"] = timed(lambda: e64.weight_gradients(x, lab, 1), reps)
    rec["fp32_pass_ms_median"], rec["fp32_pass_ms"] = timed(lambda: sv.gradients(xd, labd), reps)
    print(json.dumps(rec))


def fc_line(rec):
    f = lambda d: ", ".join("%s %.3f" % (k[6:], v) for k, v in d.items())
    return ("%s 784 -> %d, B = %d, %s on %s (fp64 point block %d)\n"
            "    mean-CE gradient (NnTrainer), x 1e-5 max|fp64|: %s; per-point CE worst %.3f x 1e-5 max(1, CE); points within %g of a kink: %d\n"
            "    summed-CE gradient (SVI / HMC step), x 1e-5 max|fp64|: %s; summed CE %.6g rel. err. %.2e, per-point CE worst %.3f x 1e-5 max(1, CE); "
            "points within %g of a kink: %d\n"
            "    one weight_gradients pass %.2f ms, one fp32 gradients() pass %.3f ms (medians of %d)"
            % (rec["arch"], rec["H"], rec["B"], rec["act"], rec["device"], rec["point_block"], f(rec["mean"]), rec["mean_ce_worst_point"], KINK,
               rec["mean_points_near_kink"], f(rec["sum"]), rec["sum_ce_fp64"], rec["sum_ce_rel_err"], rec["sum_ce_worst_point"], KINK,
               rec["sum_points_near_kink"], rec["fp64_pass_ms_median"], rec["fp32_pass_ms_median"], len(rec["fp64_pass_ms"])))


def fc_main(a):
    cases = [(c.split("x")[0], int(c.split("x")[1]), int(c.split("x")[2]), act) for c in (a.cases or FC_DEFAULT).split(",") for act in a.acts.split(",")]
    if a.child:
        return fc_child(*cases[0], a.reps)
    runner = S.Runner("fp64_fc_wgrad_parity")
    with open(os.path.join(runner.out, "summary.txt"), "w") as f:
        for arch, H, B, act in cases:
            text = runner.gpu("bench_full", "%s_H%d_B%d_%s" % (arch, H, B, act),
                              [S.PY, os.path.abspath(__file__), "--nets", "fc", "--child", "--cases", "%sx%dx%d" % (arch, H, B), "--acts", act,
                               "--reps", str(a.reps)])
            rec = S.last_json(text)
            print(fc_line(rec), flush=True)
            f.write(fc_line(rec) + "\n" + json.dumps(rec) + "\n")
            f.flush()


def line(rec):
    f = lambda d: ", ".join("%s %.3f" % (k[6:], v) for k, v in d.items())
    return ("B = %d, Hc = %d, %s on %s (fp64 point block %d)\n"
            "    mean-CE gradient (ConvNnTrainer), x 1e-5 max|fp64|: %s; per-point CE worst %.3f x 1e-5 max(1, CE)\n"
            "    summed-CE gradient (SVI / HMC step), x 1e-5 max|fp64|: %s; summed CE %.6g rel. err. %.2e, per-point CE worst %.3f x 1e-5 max(1, CE)\n"
            "    one weight_gradients pass %.1f ms, one fp32 gradients() pass %.2f ms (medians of %d)"
            % (rec["B"], rec["Hc"], rec["act"], rec["device"], rec["point_block"], f(rec["mean"]), rec["mean_ce_worst_point"], f(rec["sum"]),
               rec["sum_ce_fp64"], rec["sum_ce_rel_err"], rec["sum_ce_worst_point"], rec["fp64_pass_ms_median"], rec["fp32_pass_ms_median"],
               len(rec["fp64_pass_ms"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", default="conv", choices=("conv", "fc"))
    ap.add_argument("--cases", default=None, help="comma-separated; conv: BxHc (default 128x512,100x1024,5000x512,5000x1024), fc: ARCHxHIDDENxB (default %s)" % FC_DEFAULT)
    ap.add_argument("--acts", default="leaky,tanh")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", action="store_true", help="measure in this process (what the runner starts, one case at a time)")
    a = ap.parse_args()
    if a.nets == "fc":
        return fc_main(a)
    cases = [(int(c.split("x")[0]), int(c.split("x")[1]), act) for c in (a.cases or "128x512,100x1024,5000x512,5000x1024").split(",") for act in a.acts.split(",")]
    if a.child:
        return child(*cases[0], a.reps)
    runner = S.Runner("fp64_wgrad_parity")
    with open(os.path.join(runner.out, "summary.txt"), "w") as f:
        for B, Hc, act in cases:
            text = runner.gpu("bench_full", "B%d_Hc%d_%s" % (B, Hc, act),
                              [S.PY, os.path.abspath(__file__), "--child", "--cases", "%dx%d" % (B, Hc), "--acts", act, "--reps", str(a.reps)])
            rec = S.last_json(text)
            print(line(rec), flush=True)
            f.write(line(rec) + "\n" + json.dumps(rec) + "\n")
            f.flush()


if __name__ == "__main__":
    main()
