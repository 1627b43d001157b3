"""The comparator and the inputs of the chain-diagnostics tests (tests/test_hip_chain_diag.py, tests/test_chain_diag_cpu.py): the definitions of
include/robustbnns_hip.h — pyro's ops.stats formulas — restated in numpy.longdouble, so that the restatement's own rounding (2^-64 per
operation) is negligible beside the kernel's 2^-53; the planted inputs; the bar; and an exact restatement in fractions.Fraction for integer
draws.  Nothing here imports the package.

One column is one problem: x[c, t], C chains of N draws, fp32 widened.
    m_c = mean_t x[c,t];  d = x - m_c;  S[c,k] = sum_{t < N-k} d[c,t] d[c,t+k];  gamma[c,k] = S[c,k] / (N - k)
    W = mean_c gamma[c,0] N / (N - 1);  V = W (N - 1) / N + var_c(m_c) (unbiased, C > 1);  r_hat = sqrt(V / W)
    split_r_hat: the same on the 2C sequences x[c, :h], x[c, N-h:], h = N // 2
    rho_0 = 1, rho_k = 1 - (W - mean_c gamma[c,k]) / V;  Rho_p = rho_2p + rho_2p+1, p < N // 2
    Rho'_p = min_{q <= p} max(Rho_q, 0);  tau = -1 + 2 sum_p Rho'_p;  n_eff = C N / tau;  n_pairs = first p with Rho_p <= 0, else N // 2
    W == 0: r_hat = 1 if V == 0 else inf, tau = n_eff = NaN, n_pairs = 0"""
from fractions import Fraction

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
CASES = [(1, 8, 37, 0), (2, 9, 37, 0), (4, 64, 300, 0), (4, 64, 300, 1000), (3, 33, 130, 1000), (8, 250, 64, 0), (2, 512, 20, 0)]
RHO_MARGIN = 1e-6            # a column is compared only where every |Rho_p| up to the stopping pair is at least this
TAU_FLOOR = 0.1              # n_eff is compared only where tau is at least this


def planted(C, N, P, offset):
    """fp32 [C, N, P]: one AR(1) series per chain and column, the columns' correlations spread over (-0.6, 0.95) — the stopping pair runs
    from 1 to N // 2 — and their scales over two decades, every chain shifted by 0.3 of its column's scale, all `offset` from the origin."""
    rng = np.random.default_rng(20261021 + 1000 * C + N)
    phi = rng.uniform(-0.6, 0.95, P)
    scale = 10 ** rng.uniform(-2, 0, P)
    e = rng.standard_normal((C, N, P))
    x = np.empty_like(e)
    x[:, 0] = e[:, 0]
    for t in range(1, N):
        x[:, t] = phi * x[:, t - 1] + np.sqrt(1 - phi ** 2) * e[:, t]
    return np.float32(offset + scale * x + 0.3 * scale * rng.standard_normal((C, 1, P)))


def as_rows(x):
    """[C, N, P] -> the chain-major matrix [C * N, P] the kernel takes."""
    return np.ascontiguousarray(x.reshape(x.shape[0] * x.shape[1], x.shape[2]))


def _gamma(x):
    """x [M, n, P] longdouble -> (means [M, P], gamma [M, n, P])."""
    M, n, P = x.shape
    m = x.sum(1) / n
    d = x - m[:, None, :]
    g = np.empty((M, n, P), dtype=LD)
    for k in range(n):
        g[:, k] = (d[:, :n - k] * d[:, k:]).sum(1) / (n - k)
    return m, g


def _wv(m, g0, n):
    M = m.shape[0]
    W = g0.mean(0) * n / (n - 1)
    V = W * (n - 1) / n
    if M > 1:
        V = V + ((m - m.mean(0)) ** 2).sum(0) / (M - 1)
    return W, V


def _ratio(V, W):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.sqrt(V / W)
    return np.where(W == 0, np.where(V == 0, LD(1), LD(np.inf)), r)


def r_hat_of(x):
    """r_hat of the sequences x [M, n, P] as they are (longdouble)."""
    x = np.asarray(x, dtype=LD)
    m = x.sum(1) / x.shape[1]
    d = x - m[:, None, :]
    W, V = _wv(m, (d * d).sum(1) / x.shape[1], x.shape[1])
    return _ratio(V, W)


def split_halves(x):
    """[C, N, P] -> [2C, N // 2, P]: the first h and the last h draws of each chain."""
    h = x.shape[1] // 2
    return np.concatenate([x[:, :h], x[:, x.shape[1] - h:]], 0)


class Restated:
    """Every result for the fp32 draws x32 [C, N, P], as float64 arrays [P] (n_pairs int64), with what the comparison needs: Rho [N // 2, P],
    A = max |x|, s = sqrt(min_c gamma[c,0]), the bar B = 4 N^1.5 u (1 + A / s) and `decided`, the columns whose stopping pair no rounding
    of the size of the bar can move."""

    def __init__(self, x32):
        x = np.asarray(x32, dtype=np.float32).astype(LD)
        C, N, P = x.shape
        h = N // 2
        self.C, self.N, self.P = C, N, P
        m, g = _gamma(x)
        W, V = _wv(m, g[:, 0], N)
        flat = x.reshape(C * N, P)
        mean = flat.sum(0) / (C * N)
        std = np.sqrt(((flat - mean) ** 2).sum(0) / (C * N - 1))
        const = W == 0
        with np.errstate(divide="ignore", invalid="ignore"):
            rho = 1 - (W - g.mean(0)) / V                       # [N, P]
            rho[0] = 1
            Rho = rho[0:2 * h:2] + rho[1:2 * h:2]               # [h, P]
            stop = Rho <= 0
            n_pairs = np.where(stop.any(0), stop.argmax(0), h)
            mono = np.minimum.accumulate(np.maximum(Rho, 0), 0)
            tau = -1 + 2 * mono.sum(0)
            tau = np.where(const, LD(np.nan), tau)
            n_eff = C * N / tau
        n_pairs = np.where(const, 0, n_pairs)
        self.mean, self.std = mean.astype(np.float64), std.astype(np.float64)
        self.r_hat = _ratio(V, W).astype(np.float64)
        self.split_r_hat = r_hat_of(split_halves(x)).astype(np.float64)
        self.tau, self.n_eff, self.n_pairs = tau.astype(np.float64), n_eff.astype(np.float64), n_pairs.astype(np.int64)
        self.Rho = Rho.astype(np.float64)
        self.A = np.abs(x).max((0, 1)).astype(np.float64)
        self.s = np.sqrt(g[:, 0].min(0)).astype(np.float64)
        with np.errstate(divide="ignore"):
            self.B = 4.0 * N ** 1.5 * U * (1.0 + self.A / self.s)
        upto = np.arange(h)[:, None] <= np.minimum(self.n_pairs, h - 1)[None, :]          # the pairs up to and including the stopping pair
        with np.errstate(invalid="ignore"):
            self.decided = ~const & ~((np.abs(self.Rho) < RHO_MARGIN) & upto).any(0)


    def ratios(self, what, got, capped):
        """got: the seven float64 / integer arrays [P] by name.  Prints how many columns each condition removed and the worst error of each
        quantity in units of its bar, asserts the caps on the removed columns (at most 5 % for tau and n_pairs; for n_eff too when
        `capped`) and every bar -> {name: worst error / bar}.
        The bars: mean N u A absolute; std, r_hat, split_r_hat 2 B relative; tau 4 N B absolute; n_pairs equal; n_eff relative within what
        4 N B on tau implies, |d n_eff| / n_eff <= 4 N B / (tau - 4 N B), where tau >= TAU_FLOOR."""
        N, P, B = self.N, self.P, self.B
        dec = self.decided
        with np.errstate(invalid="ignore"):
            pos = dec & (self.tau >= TAU_FLOOR)
        print(f"[chain_diag parity] {what} C={self.C} N={N} P={P}: {int((~dec).sum())} of {P} columns removed for tau / n_pairs "
              f"(|Rho_p| < {RHO_MARGIN:g} up to the stopping pair), {int((dec & ~pos).sum())} more for n_eff (tau < {TAU_FLOOR}); "
              f"n_pairs {int(self.n_pairs.min())} .. {int(self.n_pairs.max())}, largest B {B.max():.2e}")
        assert (~dec).sum() <= 0.05 * P, f"{what}: the margin removes {(~dec).sum()} of {P} columns"
        if capped:
            assert (~pos).sum() <= 0.05 * P, f"{what}: tau < {TAU_FLOOR} removes {(~pos).sum()} of {P} columns"
        g = {k: np.asarray(v) for k, v in got.items()}
        out = {"mean": float((np.abs(g["mean"] - self.mean) / (N * U * self.A)).max())}
        for k in ("std", "r_hat", "split_r_hat"):
            ref = getattr(self, k)
            out[k] = float((np.abs(g[k] - ref) / np.abs(ref) / (2 * B)).max())
        out["tau"] = float((np.abs(g["tau"] - self.tau)[dec] / (4 * N * B[dec])).max())
        out["n_pairs"] = float((g["n_pairs"][dec] != self.n_pairs[dec]).sum())
        if pos.any():
            bar = 4 * N * B[pos] / (self.tau[pos] - 4 * N * B[pos])
            assert (bar > 0).all()
            out["n_eff"] = float((np.abs(g["n_eff"] - self.n_eff)[pos] / np.abs(self.n_eff[pos]) / bar).max())
        print(f"[chain_diag parity] {what}: worst error / bar: " + ", ".join(f"{k} {v:.2e}" for k, v in out.items() if k != "n_pairs")
              + f"; n_pairs mismatches {int(out['n_pairs'])}")
        for k, v in out.items():
            assert (v == 0) if k == "n_pairs" else (v <= 1.0), f"{what}: {k} is {v:.3g} x its bar from the restatement"
        return out


def exact_tau(col):
    """One column of integer draws [C][N] -> (n_pairs, tau as a Fraction): the same definitions without a rounding.  W != 0 is required."""
    C, N = len(col), len(col[0])
    h = N // 2
    x = [[Fraction(int(v)) for v in chain] for chain in col]
    m = [sum(ch) / N for ch in x]
    d = [[v - m[c] for v in x[c]] for c in range(C)]
    gam = [sum(sum(d[c][t] * d[c][t + k] for t in range(N - k)) / (N - k) for c in range(C)) / C for k in range(N)]
    W = gam[0] * N / (N - 1)
    V = W * (N - 1) / N
    if C > 1:
        mm = sum(m) / C
        V += sum((v - mm) ** 2 for v in m) / (C - 1)
    assert W != 0
    rho = [Fraction(1)] + [1 - (W - gam[k]) / V for k in range(1, N)]
    total, low, n_pairs = Fraction(0), None, h
    for p in range(h):
        Rho = rho[2 * p] + rho[2 * p + 1]
        if Rho <= 0:
            n_pairs = p
            break
        low = Rho if low is None else min(low, Rho)
        total += low
    return n_pairs, -1 + 2 * total
