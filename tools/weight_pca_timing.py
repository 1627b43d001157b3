"""Time of the weight-space PCA (robustbnns_amd.weight_pca, csrc/rbnn_wpca.inc) at the size of the reference's test_multimodal.py — P = 669 706
weights (fc2-512 on 1x28x28), 50 posterior rows per net, 150 rows under same_pca, 1000 rows of the N(0, I) prior — against the reference's
method on the same host: sklearn.decomposition.PCA on the materialised rows (numpy's SVD restatement where sklearn is not installed).

    python tools/weight_pca_timing.py [--reps 7] [--host-reps 3] [--cases posterior50,same150,prior1000]

Each figure: median and min..max of wall-clock times around whole calls, the device synchronised before and after (a fit includes the copy of
the Gram matrix to the host and torch.linalg.eigh there; the host method's figures leave out the copy of the rows to the host, which the
reference pays too).  The posterior rows are synthetic: one point far from the origin plus a small spread, as the samples of one HMC chain lie.
Every case is measured in a child process of its own through timing.cases; one JSON line per case.  --child: the measuring program itself."""
import argparse

import numpy as np
import torch

import timing as T

P = 784 * 512 + 512 + 512 * 512 + 512 + 512 * 10 + 10            # 669 706
KEY = 0x57504341
DEV = "cuda:0"


def posterior_rows(n, seed, P=P):
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


CASES = {"posterior50": 50, "same150": 150, "prior1000": None}      # rows of the fit; None: the prior's rows, drawn on the way


def measure(case, reps, host_reps, rows=None, P=P, prior_rows=1000):
    """rows: of the fit (the case's own where None)."""
    from robustbnns_amd.weight_pca import MatrixRows, PriorRows, WeightPCA
    name, host_fit, host_transform = host_pca()
    res = {"case": case, "P": P, "host_method": name}
    host = lambda fn: T.stats(T.wall(fn, host_reps, warmup=False, sync=lambda: None))     # host work alone: no device to wait for
    if case == "prior1000":
        prior = PriorRows(KEY, prior_rows, P, DEV)
        res["fit_with_draw"] = T.stats(T.wall(lambda: WeightPCA(2, device=DEV).fit(prior), reps))
        Xh = prior.materialize().cpu().numpy()
        res["host_fit"] = host(lambda: host_fit(Xh))
        return res
    n = rows or CASES[case]
    X, Y = posterior_rows(n, 1, P), posterior_rows(50, 2, P)
    pca = WeightPCA(2, device=DEV)
    res["rows"] = n
    res["fit"] = T.stats(T.wall(lambda: pca.fit(MatrixRows(X)), reps))
    res["transform_50_rows"] = T.stats(T.wall(lambda: pca.transform(MatrixRows(Y)), reps))
    res["components"] = T.stats(T.wall(lambda: pca.components(), reps))
    if case == "same150":                                          # same_pca: the prior's 1000 rows against the one fit, drawn on the way
        prior = PriorRows(KEY, prior_rows, P, DEV)
        res["transform_prior_1000_rows_with_draw"] = T.stats(T.wall(lambda: pca.transform(prior), reps))
    Xh, Yh = X.cpu().numpy(), Y.cpu().numpy()
    model = host_fit(Xh)
    res["host_fit"] = host(lambda: host_fit(Xh))
    res["host_transform_50_rows"] = host(lambda: host_transform(model, Yh))
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=T.BLOCKS)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--child", action="store_true", help="measure ONE case in this process (what the runner starts)")
    a = ap.parse_args(argv)
    if a.child:
        return T.child(lambda: measure(a.cases, a.reps, a.host_reps))
    T.cases("weight_pca_timing", __file__, [(case, ["--cases", case] + T.opts(a, "reps", "host_reps")) for case in a.cases.split(",")])


if __name__ == "__main__":
    main()
