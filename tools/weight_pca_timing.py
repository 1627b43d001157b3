"""Time of the weight-space PCA (robustbnns_amd.weight_pca, csrc/rbnn_wpca.inc) at the size of the reference's test_multimodal.py — P = 669 706
weights (fc2-512 on 1x28x28), 50 posterior rows per net, 150 rows under same_pca, 1000 rows of the N(0, I) prior — against the reference's
method on the same host: sklearn.decomposition.PCA on the materialised rows (numpy's SVD restatement where sklearn is not installed).

    python tools/weight_pca_timing.py [--reps 7] [--host-reps 3] [--cases posterior50,same150,prior1000]

Each figure: median and min..max of wall-clock times around whole calls, the device synchronised before and after (a fit includes the copy of
the Gram matrix to the host and torch.linalg.eigh there; the host method's figures leave out the copy of the rows to the host, which the
reference pays too).  The posterior rows are synthetic: one point far from the origin plus a small spread, as the samples of one HMC chain lie.
Every case is measured in a child process of its own, started through steps.Runner (one time limit each; a fault, an abort or a time limit
ends the tool); one JSON line per case.  --child: the measuring program itself."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as G                                    # noqa: E402
import steps as S                                  # noqa: E402

P = 784 * 512 + 512 + 512 * 512 + 512 + 512 * 10 + 10            # 669 706
KEY = 0x57504341
DEV = "cuda:0"


def wall(fn, reps):
    """ms of `reps` calls after one warm-up call, sorted."""
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return sorted(out)


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": ms[0], "max_ms": ms[-1], "runs": len(ms)}


def posterior_rows(n, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(1, P, device=DEV, generator=g) + 0.01 * torch.randn(n, P, device=DEV, generator=g)).contiguous()


def host_pca():
    """-> (name, fit(X) -> model, transform(model, Y)) of the reference's method."""
    try:
        from sklearn import decomposition
        return ("sklearn.decomposition.PCA", lambda X: decomposition.PCA(n_components=2).fit(X), lambda m, Y: m.transform(Y))
    except ImportError:
        def fit(X):
            mean = X.mean(0)
            return mean, np.linalg.svd(X - mean, full_matrices=False)[2][:2]
        return "numpy.linalg.svd", fit, lambda m, Y: (Y - m[0]) @ m[1].T


def child(a):
    from robustbnns_amd.weight_pca import MatrixRows, PriorRows, WeightPCA
    G.build()
    name, host_fit, host_transform = host_pca()
    res = {"case": a.cases, "P": P, "host_method": name}

    def host(fn):
        t = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            fn()
            t.append(1e3 * (time.perf_counter() - t0))
        return stats(sorted(t))
    if a.cases == "prior1000":
        prior = PriorRows(KEY, 1000, P, DEV)
        res["fit_with_draw"] = stats(wall(lambda: WeightPCA(2, device=DEV).fit(prior), a.reps))
        Xh = prior.materialize().cpu().numpy()
        res["host_fit"] = host(lambda: host_fit(Xh))
    else:
        n = 50 if a.cases == "posterior50" else 150
        X, Y = posterior_rows(n, 1), posterior_rows(50, 2)
        pca = WeightPCA(2, device=DEV)
        res["rows"] = n
        res["fit"] = stats(wall(lambda: pca.fit(MatrixRows(X)), a.reps))
        res["transform_50_rows"] = stats(wall(lambda: pca.transform(MatrixRows(Y)), a.reps))
        res["components"] = stats(wall(lambda: pca.components(), a.reps))
        if n == 150:                                               # same_pca: the prior's 1000 rows against the one fit, drawn on the way
            prior = PriorRows(KEY, 1000, P, DEV)
            res["transform_prior_1000_rows_with_draw"] = stats(wall(lambda: pca.transform(prior), a.reps))
        Xh, Yh = X.cpu().numpy(), Y.cpu().numpy()
        model = host_fit(Xh)
        res["host_fit"] = host(lambda: host_fit(Xh))
        res["host_transform_50_rows"] = host(lambda: host_transform(model, Yh))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--cases", default="posterior50,same150,prior1000")
    ap.add_argument("--child", action="store_true", help="measure in this process (what the runner starts, one case at a time)")
    a = ap.parse_args()
    if a.child:
        return child(a)
    runner = S.Runner("weight_pca_timing")
    for case in a.cases.split(","):
        text = runner.gpu("timing", case, [S.PY, os.path.abspath(__file__), "--child", "--cases", case, "--reps", str(a.reps), "--host-reps",
                                           str(a.host_reps)])
        print(json.dumps(S.last_json(text)), flush=True)


if __name__ == "__main__":
    main()
