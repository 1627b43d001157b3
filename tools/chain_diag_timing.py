"""Time of the per-weight chain diagnostics (robustbnns_amd.chain_diagnostics, csrc/rbnn_chain_diag.inc) at the size of the reference's
fc2-512 net — P = 669 706 weights — for the pooled stacks of 8 chains of 50 and of 250 draws.

    python tools/chain_diag_timing.py [--reps 7] [--torch-reps 3] [--cases 8x50,8x250]

Each figure: median and min..max of wall-clock times around whole calls, the device synchronised before and after.  Beside diagnose():
a device copy of the same bytes (the floor of one read of the input) and a torch float64 restatement of the same definitions on the same
GPU, swept in column slabs so that its temporaries stay bounded.  The draws are synthetic: one point far from the origin plus an AR(1)-like
walk per chain, as the samples of HMC chains lie.  Every case is measured in a child process of its own through timing.cases; one JSON line
per case.  --child: the measuring program itself."""
import argparse

import torch

import timing as T

P = 784 * 512 + 512 + 512 * 512 + 512 + 512 * 10 + 10            # 669 706
DEV = "cuda:0"
TORCH_SLAB = 32768


def chain_rows(K, draws, seed, P=P):
    g = torch.Generator(device=DEV).manual_seed(seed)
    X = torch.empty(K * draws, P, device=DEV)
    centre = torch.randn(1, P, device=DEV, generator=g)
    for c in range(K):
        walk = 0.01 * torch.randn(draws, P, device=DEV, generator=g)
        for t in range(1, draws):
            walk[t] += 0.7 * walk[t - 1]
        X[c * draws:(c + 1) * draws] = centre + walk + 0.003 * torch.randn(1, P, device=DEV, generator=g)
    return X


def _r_hat(x):
    """x [M, n, w] float64 -> [w]"""
    M, n = x.shape[0], x.shape[1]
    m = x.mean(1)
    W = ((x - m[:, None]) ** 2).sum(1).div(n).mean(0) * n / (n - 1)
    V = W * (n - 1) / n + (m.var(0, unbiased=True) if M > 1 else 0)
    return torch.where(W == 0, torch.where(V == 0, 1.0, float("inf")).to(W.dtype), (V / W).sqrt())


def torch_restatement(X, K):
    """The definitions of include/robustbnns_hip.h in torch float64, vectorised over a slab of columns -> (split_r_hat, tau, n_eff) [P]."""
    draws, P = X.shape[0] // K, X.shape[1]
    h = draws // 2
    out = [torch.empty(P, dtype=torch.float64, device=X.device) for _ in range(3)]
    for e0 in range(0, P, TORCH_SLAB):
        x = X[:, e0:e0 + TORCH_SLAB].double().view(K, draws, -1)
        m = x.mean(1)
        d = x - m[:, None]
        gam = torch.stack([(d[:, :draws - k] * d[:, k:]).sum(1).div(draws - k).mean(0) for k in range(2 * h)])
        W = gam[0] * draws / (draws - 1)
        V = W * (draws - 1) / draws + (m.var(0, unbiased=True) if K > 1 else 0)
        rho = 1 - (W - gam) / V
        rho[0] = 1
        Rho = rho[0::2] + rho[1::2]
        tau = -1 + 2 * torch.cummin(Rho.clamp_min(0), 0).values.sum(0)
        tau = torch.where(W == 0, float("nan"), tau)
        sl = slice(e0, e0 + x.shape[2])
        out[0][sl] = _r_hat(torch.cat([x[:, :h], x[:, draws - h:]], 0))
        out[1][sl] = tau
        out[2][sl] = K * draws / tau
    return out


def measure(K, draws, reps, torch_reps, P=P):
    from robustbnns_amd.chain_diagnostics import diagnose
    X = chain_rows(K, draws, 1, P)
    res = {"case": f"{K}x{draws}", "P": P, "chains": K, "draws": draws, "input_bytes": X.numel() * 4}
    res["diagnose"] = T.stats(T.wall(lambda: diagnose(X, K), reps))
    dst = torch.empty_like(X)
    res["device_copy"] = T.stats(T.wall(lambda: dst.copy_(X), reps))
    del dst
    res["torch_float64"] = T.stats(T.wall(lambda: torch_restatement(X, K), torch_reps))
    d, t = diagnose(X, K), torch_restatement(X, K)
    res["max_rel_diff_tau_vs_torch"] = float(((d.tau - t[1]).abs() / t[1].abs().clamp_min(1e-300)).max())
    res["n_eff_median"] = float(d.n_eff.median())
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=T.BLOCKS)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--cases", default="8x50,8x250")
    ap.add_argument("--child", action="store_true", help="measure ONE case in this process (what the runner starts)")
    a = ap.parse_args(argv)
    if a.child:
        return T.child(lambda: measure(*(int(v) for v in a.cases.split("x")), a.reps, a.torch_reps))
    T.cases("chain_diag_timing", __file__, [(case, ["--cases", case] + T.opts(a, "reps", "torch_reps")) for case in a.cases.split(",")])


if __name__ == "__main__":
    main()
