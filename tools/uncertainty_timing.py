"""Time and cross-precision parity of the predictive uncertainty (robustbnns_amd.uncertainty, csrc/rbnn_predictive.inc).

    python tools/uncertainty_timing.py [--reps 7] [--cases fc512,conv512,parity_fc,parity_conv]

fc512: BASELINE config 2's size — fc, hidden 512, S = 100 stored samples, N = 10 000 points, 10 classes; conv512: conv, Hc = 512, 1x28x28,
S = 16, N = 2048.  Each figure: median and min..max of wall-clock times around whole calls, the device synchronised before and after.
    engine.uncertainty(x, S, y)       beside engine.forward(x, S) of the same call (what the parent gives: the mean alone)
    rbnn_predictive_stats alone       on the P of that forward, beside a device copy of the same P (the floor of one read and one write)
    a float64 torch restatement       of the same definitions on the same GPU from the same P
parity_fc / parity_conv: the largest difference of every figure between each fp32 mode (exact, triple, split) and the fp64 checker on the
same posterior and inputs, at fc-512, S = 100, N = 1000 and conv-64, S = 8, N = 256 (reported, not asserted: a different prediction at a
near-tie moves confidence, agreement and variance by what the two classes differ in).
Every case is measured in a child process of its own through timing.cases; one JSON line per case.  --child: the measuring program itself."""
import argparse

import torch

import timing as T

DEV = "cuda:0"
FLOATS = ("entropy", "expected_entropy", "mutual_information", "confidence", "agreement", "variance", "nll", "brier")


def engines(kind, hidden, n_samples, precisions):
    """{precision: engine} on one synthetic posterior (tests' recipe: N(0, 0.05^2) weights per stored sample), and its fp64 checker."""
    from oracle import bnn_oracle as O
    from robustbnns_amd import AttackEngine, StackedPosterior
    if kind == "fc":
        sp = StackedPosterior("fc", "leaky", (1, 28, 28), 10, hidden, O.synthetic_posterior("fc", 784, hidden, 10, n_samples, 0.05), DEV)
        return {p: AttackEngine(sp, precision=p) for p in precisions}, AttackEngine(sp, precision="fp64")
    from robustbnns_amd.conv import ConvEngine, ConvStackedPosterior
    from robustbnns_amd.conv_fp64 import ConvFp64Engine
    sp = ConvStackedPosterior("leaky", (1, 28, 28), 10, hidden, O.synthetic_posterior("conv", 784, hidden, 10, n_samples, 0.05), DEV)
    return {p: ConvEngine(sp, precision=p) for p in precisions}, ConvFp64Engine(sp)


def torch_restatement(P, Cn, y):
    """The definitions of include/robustbnns_hip.h in torch float64 on P's device -> the ten figures."""
    p = P[:, :, :Cn].double()
    Sn = p.shape[0]
    pbar = p.mean(0)
    plogp = lambda q: torch.where(q > 0, q * torch.log(torch.where(q > 0, q, torch.ones_like(q))), torch.zeros_like(q))
    H, E = -plogp(pbar).sum(-1), -plogp(p).sum(-1).mean(0)
    pred = pbar.argmax(-1)
    rows = torch.arange(p.shape[1], device=p.device)
    own = p[:, rows, pred]
    return {"entropy": H, "expected_entropy": E, "mutual_information": H - E, "confidence": pbar[rows, pred],
            "agreement": (p.argmax(-1) == pred).double().sum(0) / Sn, "variance": own.var(0, unbiased=False), "nll": -torch.log(pbar[rows, y]),
            "brier": ((pbar - torch.nn.functional.one_hot(y, Cn)) ** 2).sum(-1), "prediction": pred.int(), "correct": (pred == y).int()}


def time_case(kind, hidden, n_samples, N, reps):
    from oracle import bnn_oracle as O
    from robustbnns_amd import _hip
    eng = engines(kind, hidden, n_samples, [None])[0][None]
    x, y = O.synthetic_inputs(N, (1, 28, 28), 10, seed=1)
    x, y = x.to(DEV), y.argmax(-1).to(DEV)
    res = {"arch": kind, "hidden": hidden, "S": n_samples, "N": N, "C": 10, "precision": eng.precision}
    res["forward"] = T.stats(T.wall(lambda: eng.forward(x, n_samples), reps))
    res["uncertainty"] = T.stats(T.wall(lambda: eng.uncertainty(x, n_samples, y=y), reps))
    res["uncertainty_8_prefixes"] = T.stats(T.wall(lambda: eng.uncertainty(x, n_samples, y=y, n_samples_list=[1, 2, 3, 5, 8, 10, 12, n_samples]), reps))
    P = eng.sample_outputs(x, n_samples)
    P16 = torch.zeros(n_samples, N, _hip.CPAD, device=DEV)
    P16[:, :, :10] = P                                            # the layout the forward leaves: rows padded to 16
    res["P_bytes"] = P16.numel() * 4
    out = {f: torch.empty(1, N, dtype=torch.int32 if f in ("prediction", "correct") else torch.float64, device=DEV)
           for f in _hip.HipKernels.PREDICTIVE_OUTPUTS}
    k, labels = _hip.HipKernels(), y.int()
    res["stats_kernel"] = T.stats(T.wall(lambda: k.predictive_stats(P16, 10, labels, [n_samples], out), reps))
    dst = torch.empty_like(P16)
    res["device_copy"] = T.stats(T.wall(lambda: dst.copy_(P16), reps))
    res["torch_float64"] = T.stats(T.wall(lambda: torch_restatement(P16, 10, y), reps))
    t = torch_restatement(P16, 10, y)
    res["max_diff_vs_torch"] = {f: float((out[f][0] - t[f]).abs().max()) for f in FLOATS}
    res["prediction_mismatches_vs_torch"] = int((out["prediction"][0] != t["prediction"]).sum())
    return res


def parity_case(kind, hidden, n_samples, N):
    from oracle import bnn_oracle as O
    engs, chk = engines(kind, hidden, n_samples, ["exact", "triple", "split"])
    x, y = O.synthetic_inputs(N, (1, 28, 28), 10, seed=2)
    ref = chk.uncertainty(x, n_samples, y=y)
    res = {"arch": kind, "hidden": hidden, "S": n_samples, "N": N, "C": 10, "modes": {}}
    for p, eng in engs.items():
        u = eng.uncertainty(x, n_samples, y=y)
        agree = u.prediction == ref.prediction
        res["modes"][p] = {"max_abs_diff": {f: float((getattr(u, f) - getattr(ref, f)).abs().max()) for f in FLOATS},
                           "max_abs_diff_same_prediction": {f: float((getattr(u, f) - getattr(ref, f))[agree].abs().max()) for f in FLOATS},
                           "prediction_mismatches": int((~agree).sum()), "correct_mismatches": int((u.correct != ref.correct).sum())}
    return res


CASES = {"fc512": lambda reps: time_case("fc", 512, 100, 10000, reps), "conv512": lambda reps: time_case("conv", 512, 16, 2048, reps),
         "parity_fc": lambda reps: parity_case("fc", 512, 100, 1000), "parity_conv": lambda reps: parity_case("conv", 64, 8, 256)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=T.BLOCKS)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--child", action="store_true", help="measure ONE case in this process (what the runner starts)")
    a = ap.parse_args(argv)
    if a.child:
        return T.child(lambda: {**CASES[a.cases](a.reps), "case": a.cases})
    T.cases("uncertainty_timing", __file__, [(case, ["--cases", case] + T.opts(a, "reps")) for case in a.cases.split(",")])


if __name__ == "__main__":
    main()
