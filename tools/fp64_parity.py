#!/usr/bin/env python3
"""The fp32 precision modes against the DEVICE fp64 result at workload size, and what an fp64 pass costs.

    python tools/fp64_parity.py [--nets c2,fc2] [--reps 7]
    python tools/fp64_parity.py --nets conv [--points N]          # bench.py's conv-512 (S = 16, N = 2048) against conv_fp64.ConvFp64Engine

At BASELINE C2's size (fc-512, S = 100, N = 10 000) and at fc2-512, S = 100 (bench.py's workloads of those names, same inputs and posterior), for
each of `auto`, `exact` and `split`:
  - the worst row error of loss_gradients and of the FGSM gradient (attack_gradient) against precision='fp64' on the same device, per row
    max_d |g - g64| / max_d |g64|, in units of the project's 1e-5 bar — over ALL rows, and over the rows the project's parity rule keeps:
    those whose smallest hidden |pre-activation| over the used samples exceeds KINK = 2e-6 (oracle.kink_margin's rule, tests/test_hip_parity.py:
    act' of relu / leaky jumps at 0, so an fp32 pre-activation that lands on the other side of 0 than the fp64 one moves that row by one
    hidden unit's whole contribution; at this size, 5e8 pre-activations, about a tenth of the rows have one that close).  The margin is a
    diagnostic of this tool: fp64 torch matmuls on the device over the fp32 weights;
  - the number of adversarial pixels (fgsm, eps = 0.3) that differ from the fp64 mode's, i.e. whose gradient sign differs (all rows / kept rows);
A conv net (--nets conv; any conv workload of bench.py is taken, only `conv` was measured: ConvEngine's modes against ConvFp64Engine) keeps the rows whose conv margin exceeds KINK: the smallest, over
the pooling windows of both layers, of the gap between a window's two largest pre-activations and of |the largest| (oracle.kink_margin's conv
rule; conv_fp64.kink_margin, fp64 torch contractions on the device).
and the time of a loss_gradients pass in fp64 next to `exact`, each the median of --reps passes (device synchronised around every pass).
Every net is measured in a child process of its own, started through steps.Runner (kind bench_full: one time limit each; after a fault, an
abort or a time limit nothing more is started); the child's JSON line is printed and kept in its log under <OUT>/fp64_parity/.  --child: the
measuring process (what the runner starts, one net at a time)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import steps as S                                  # noqa: E402

BAR = 1e-5
KINK = 2e-6
MODES = ("auto", "exact", "split")


def row_err(g, g64):
    """per row: max_d |g - g64| / max_d |g64|"""
    a, b = g.double().reshape(g.shape[0], -1), g64.reshape(g64.shape[0], -1)
    return (a - b).abs().amax(1) / b.abs().amax(1).clamp_min(1e-300)


def kink_margin(sp, x, n):
    """per point: the smallest |hidden pre-activation| over the first n samples and every hidden layer, in fp64 (torch on the device)."""
    import torch
    xd = x.reshape(x.shape[0], -1).to(sp.device, torch.float64)
    slope = 0.0 if sp.activation == "relu" else 0.01
    margin = torch.full((x.shape[0],), float("inf"), dtype=torch.float64, device=sp.device)
    if sp.activation not in ("relu", "leaky"):
        return margin
    for s in range(n):
        a = xd @ sp.W1[s, :, :sp.D].double().T + sp.b1[s].double()
        margin = torch.minimum(margin, a.abs().amin(1))
        if sp.arch == "fc2":
            a = torch.where(a > 0, a, a * slope) @ sp.Wm[s].double().T + sp.bm[s].double()
            margin = torch.minimum(margin, a.abs().amin(1))
    return margin


def timed(fn, reps):
    import torch
    out = []
    fn()                                            # the first pass allocates the workspaces
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(out), out


def child(name, reps, points=0):
    import torch
    import bench
    from robustbnns_amd import AttackEngine, StackedPosterior, _hip
    w = bench.WORKLOADS[name]
    if points:
        w = dict(w, N=points)
    x, y, post = bench.make_problem(w, 0, "cuda:0")
    n, D = w["S"], x[0].numel()
    if w["arch"] == "conv":
        from robustbnns_amd import conv_fp64
        from robustbnns_amd.conv import ConvEngine, ConvStackedPosterior
        sp = ConvStackedPosterior(w["act"], w["shape"], w["C"], w["H"], post, "cuda:0")
        e64, engine = conv_fp64.ConvFp64Engine(sp), (lambda mode: ConvEngine(sp, precision=mode))
        margin, block = (lambda: conv_fp64.kink_margin(sp, x, n)), e64.point_block(n)
    else:
        sp = StackedPosterior(w["arch"], w["act"], w["shape"], w["C"], w["H"], post, "cuda:0")
        e64, engine = AttackEngine(sp, precision="fp64"), (lambda mode: AttackEngine(sp, precision=mode))
        margin, block = (lambda: kink_margin(sp, x, n)), e64.fp64.point_block(n)
    g64 = e64.loss_gradients(x, y, n)
    a64 = e64.attack_gradient(x, y, n)[:, :D]
    adv64 = e64.fgsm(x, y, n, 0.3)
    keep = margin() > KINK
    rec = {"net": name, "arch": w["arch"], "H": w["H"], "S": n, "N": w["N"], "act": w["act"], "bar": BAR, "fp64_point_block": block,
           "kink": KINK, "rows_kept": int(keep.sum()), "modes": {}}
    keep_px = keep.reshape((-1,) + (1,) * (x.dim() - 1))
    for mode in MODES:
        try:
            e = engine(mode)
        except _hip.HipError as exc:                # a mode that does not cover the posterior says so; nothing was launched
            rec["modes"][mode] = {"refused": str(exc)}
            continue
        g = e.loss_gradients(x, y, n)
        a = e.attack_gradient(x, y, n)[:, :D]
        adv = e.fgsm(x, y, n, 0.3)
        eg, ea = row_err(g, g64) / BAR, row_err(a, a64) / BAR
        worst = lambda e: float(e.max()) if e.numel() else float("nan")      # (a conv net at workload size may keep no row at all)
        rec["modes"][mode] = {"resolved": e.precision, "loss_gradients_worst_row_over_bar": float(eg.max()),
                              "loss_gradients_worst_kept_row_over_bar": worst(eg[keep]), "loss_gradients_kept_rows_beyond_bar": int((eg[keep] > 1).sum()),
                              "loss_gradients_rows_beyond_bar": int((eg > 1).sum()), "loss_gradients_median_row_over_bar": float(eg.median()),
                              "fgsm_gradient_median_row_over_bar": float(ea.median()),
                              "fgsm_gradient_worst_row_over_bar": float(ea.max()), "fgsm_gradient_worst_kept_row_over_bar": worst(ea[keep]),
                              "fgsm_gradient_kept_rows_beyond_bar": int((ea[keep] > 1).sum()), "fgsm_gradient_rows_beyond_bar": int((ea > 1).sum()),
                              "adversarial_pixels_that_differ": int((adv != adv64).sum()),
                              "adversarial_pixels_that_differ_in_kept_rows": int(((adv != adv64) & keep_px).sum()), "pixels": adv.numel()}
        del e, g, a, adv
    exact = engine("exact")
    rec["fp64_pass_ms_median"], rec["fp64_pass_ms"] = timed(lambda: e64.loss_gradients(x, y, n), reps)
    rec["exact_pass_ms_median"], rec["exact_pass_ms"] = timed(lambda: exact.loss_gradients(x, y, n), reps)
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec))


def line(rec):
    out = ["%s (%s-%d, S = %d, N = %d, %s) on %s: fp64 pass %.1f ms, exact pass %.2f ms (medians of %d; fp64 point block %d); "
           "%d of %d rows kept (kink margin > %g)"
           % (rec["net"], rec["arch"], rec["H"], rec["S"], rec["N"], rec["act"], rec["device"], rec["fp64_pass_ms_median"], rec["exact_pass_ms_median"],
              len(rec["fp64_pass_ms"]), rec["fp64_point_block"], rec["rows_kept"], rec["N"], rec["kink"])]
    for mode, m in rec["modes"].items():
        if "refused" in m:
            out.append("    %-5s refused: %s" % (mode, m["refused"]))
            continue
        out.append("    %-5s (-> %-6s) worst row, kept rows: loss_gradients %.3f x 1e-5 (%d beyond), FGSM gradient %.3f x 1e-5 (%d beyond); all rows: "
                   "%.1f x 1e-5 (%d beyond, median %.3f), %.1f x 1e-5 (%d beyond, median %.3f); adversarial pixels that differ: %d in kept rows, %d in all, of %d"
                   % (mode, m["resolved"], m["loss_gradients_worst_kept_row_over_bar"], m["loss_gradients_kept_rows_beyond_bar"],
                      m["fgsm_gradient_worst_kept_row_over_bar"], m["fgsm_gradient_kept_rows_beyond_bar"], m["loss_gradients_worst_row_over_bar"],
                      m["loss_gradients_rows_beyond_bar"], m.get("loss_gradients_median_row_over_bar", float("nan")), m["fgsm_gradient_worst_row_over_bar"],
                      m["fgsm_gradient_rows_beyond_bar"], m.get("fgsm_gradient_median_row_over_bar", float("nan")),
                      m["adversarial_pixels_that_differ_in_kept_rows"], m["adversarial_pixels_that_differ"], m["pixels"]))
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", default="c2,fc2")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--points", type=int, default=0, help="override the workload's point count (conv-512, S = 16: an fp64 pass is 240 ms per 2048 points)")
    ap.add_argument("--child", action="store_true", help="measure in this process (what the runner starts, one net at a time)")
    a = ap.parse_args()
    if a.child:
        return child(a.nets, a.reps, a.points)
    runner = S.Runner("fp64_parity")
    with open(os.path.join(runner.out, "summary.txt"), "w") as f:
        for name in a.nets.split(","):
            text = runner.gpu("bench_full", name, [S.PY, os.path.abspath(__file__), "--child", "--nets", name, "--reps", str(a.reps), "--points", str(a.points)])
            rec = S.last_json(text)
            print(line(rec), flush=True)
            f.write(line(rec) + "\n" + json.dumps(rec) + "\n")
            f.flush()


if __name__ == "__main__":
    main()
