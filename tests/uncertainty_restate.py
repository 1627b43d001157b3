"""The definitions of the predictive uncertainty (include/robustbnns_hip.h, csrc/rbnn_predictive.inc) restated in numpy.longdouble, the
planted inputs of the GPU tests and the derived bars.  Not a test file: tests/test_uncertainty_cpu.py and tests/test_hip_uncertainty.py import it.

For one point, p_s[c] the probabilities of sample s < S over the classes c < C (columns >= C of the padded rows are never read), natural
logarithms, 0 ln 0 = 0:
    pbar[c]            = (sum_s p_s[c]) / S
    entropy            = -sum_c pbar[c] ln pbar[c]
    expected_entropy   = (1 / S) sum_s (-sum_c p_s[c] ln p_s[c])
    mutual_information = entropy - expected_entropy                     (nothing clamped)
    prediction         = the first maximum of pbar (torch's argmax rule)
    confidence         = pbar[prediction]
    agreement          = double(number of s whose own first maximum == prediction) / double(S)
    variance           = the population variance over s of p_s[prediction]
    nll = -ln pbar[y] (+inf at 0),  brier = sum_c (pbar[c] - [c == y])^2,  correct = (prediction == y)
Calibration: b = min(n_bins - 1, max(0, (int)ceil(confidence * n_bins) - 1)) in float64, intervals (lo, hi]; per bin the count, the sum of
confidence and the number correct; ece = sum_b (n_b / N) |acc_b - conf_b|, mce the largest such gap over the non-empty bins.

Bars, from u = 2^-53 and B = C (2 S + 8) u: every quantity is a sum of at most C (S + 1) terms of magnitude <= 1, |p ln p| <= 1 / e, and
an error dp <= S u p in pbar moves p ln p by at most S u.  entropy, expected_entropy, variance, brier: B absolute; mutual_information 2 B;
confidence (S + 2) u; nll (S + 4) u max(1, nll), inf equal to inf; agreement equal bits; prediction, correct equal."""
import math
from types import SimpleNamespace

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
FLOAT_FIELDS = ("entropy", "expected_entropy", "mutual_information", "confidence", "agreement", "variance", "nll", "brier")
INT_FIELDS = ("prediction", "correct")
FIELDS = FLOAT_FIELDS + INT_FIELDS
SHAPES = [(1, 1, 2), (3, 5, 10), (7, 67, 10), (100, 130, 10), (512, 33, 16), (64, 4099, 3)]      # (S, N, C) of the kernel-level tests
LDP = 16


def plogp(p):
    return np.where(p > 0, p * np.log(np.where(p > 0, p, 1)), 0)


def restate(P, C, S, labels=None):
    """The figures of the first S samples of P [>= S, N, >= C] in longdouble -> SimpleNamespace of [N] arrays (agreement float64: the same
    expression as the kernel's; prediction, correct int32) plus pbar [N, C], gap (between the two largest pbar) and sample_gap (the smallest
    NONZERO gap between the two largest p_s over the samples; inf when every sample's top two tie exactly)."""
    p = np.asarray(P)[:S, :, :C].astype(LD)
    N = p.shape[1]
    total = np.zeros((N, C), LD)
    mean, m2 = np.zeros((N, C), LD), np.zeros((N, C), LD)
    for s in range(S):
        total += p[s]
        d = p[s] - mean
        mean += d / LD(s + 1)
        m2 += d * (p[s] - mean)
    pbar = total / LD(S)
    rows = np.arange(N)
    pred = pbar.argmax(1)                                   # numpy's argmax is the first maximum, as torch's
    r = SimpleNamespace(pbar=pbar)
    r.entropy = -plogp(pbar).sum(1)
    r.expected_entropy = -plogp(p).sum((0, 2)) / LD(S)
    r.mutual_information = r.entropy - r.expected_entropy
    r.prediction = pred.astype(np.int32)
    r.confidence = pbar[rows, pred]
    votes = (p.argmax(2) == pred[None, :]).sum(0)
    r.agreement = votes.astype(np.float64) / np.float64(S)
    r.variance = m2[rows, pred] / LD(S)
    top = np.sort(pbar, 1)
    r.gap = top[:, -1] - top[:, -2]
    stop = np.sort(p, 2)
    sg = stop[:, :, -1] - stop[:, :, -2]
    r.sample_gap = np.where(sg > 0, sg, np.inf).min(0)
    if labels is not None:
        y = np.asarray(labels).astype(np.int64)
        named = (y >= 0) & (y < C)
        py = np.where(named, pbar[rows, np.where(named, y, 0)], 0)
        with np.errstate(divide="ignore"):
            r.nll = -np.log(py)
        r.brier = ((pbar - (np.arange(C)[None, :] == y[:, None])) ** 2).sum(1)
        r.correct = (pred == y).astype(np.int32)
    return r


def bars(S, C, nll=None):
    B = C * (2 * S + 8) * U
    b = {"entropy": B, "expected_entropy": B, "variance": B, "brier": B, "mutual_information": 2 * B, "confidence": (S + 2) * U}
    if nll is not None:
        b["nll"] = (S + 4) * U * np.maximum(1.0, np.where(np.isfinite(nll), nll, 1.0).astype(np.float64))
    return b


def check(got, ref, S, C, what=""):
    """got: name -> host array of the device's figures (a missing / None name is skipped) against restate()'s `ref` at the bars above.
    Asserts the precondition first: every point's two largest pbar, and every sample's two largest p_s unless they tie EXACTLY (a sample's
    probabilities are compared as they stand, unrounded: an exact tie is decided by the first-maximum rule on both sides), lie further apart
    than the confidence bar.  -> name -> the worst error in units of its bar."""
    cbar = (S + 2) * U
    assert (ref.gap > cbar).all() or C == 1, (what, "a point's two largest pbar are closer than the confidence bar", float(ref.gap.min()))
    assert (ref.sample_gap > cbar).all(), (what, "a sample's two largest probabilities are closer than the confidence bar")
    b = bars(S, C, getattr(ref, "nll", None))
    worst = {}
    for f in FIELDS:
        g = got.get(f)
        if g is None:
            continue
        want = getattr(ref, f)
        if f in INT_FIELDS:
            assert g.dtype == np.int32 and (g == want).all(), (what, f)
        elif f == "agreement":
            assert g.dtype == np.float64 and (g.view(np.int64) == want.view(np.int64)).all(), (what, f)
        else:
            assert g.dtype == np.float64, (what, f)
            inf = np.isinf(want.astype(np.float64))
            assert (np.isinf(g) == inf).all() and (g[inf] > 0).all(), (what, f, "inf where the restatement has none, or the reverse")
            err = np.abs(g.astype(LD)[~inf] - want[~inf])
            ratio = err / (b[f][~inf] if np.ndim(b[f]) else b[f])
            worst[f] = float(ratio.max()) if ratio.size else 0.0
            assert worst[f] <= 1.0, (what, f, worst[f])
    return worst


def planted(S, N, C, seed=0, dtype=np.float32):
    """(P [S, N, LDP] of `dtype` with NaN in the columns >= C, labels int32 [N]).  Softmax rows of logits scaled by 1, 3, 10 or 30 per point
    (at 30 many probabilities are exactly 0 in float32); where S >= 3, points n % 7 == 3 have every third sample one-hot and points
    n % 7 == 5 every second sample uniform; points n % 5 == 1 have one class at probability 0 in every sample and that class as their
    label (pbar[y] == 0)."""
    rng = np.random.default_rng(1000 * S + 10 * N + C + seed)
    scale = np.array([1.0, 3.0, 10.0, 30.0])[np.arange(N) % 4]
    z = rng.standard_normal((S, N, C)) * scale[None, :, None]
    z -= z.max(-1, keepdims=True)
    e = np.exp(z)
    p = (e / e.sum(-1, keepdims=True)).astype(np.float32).astype(np.float64) if dtype == np.float32 else e / e.sum(-1, keepdims=True)
    y = rng.integers(0, C, N)
    if S >= 3:
        for n in range(N):
            if n % 7 == 3:
                for s in range(0, S, 3):
                    p[s, n] = 0.0
                    p[s, n, (n + s) % C] = 1.0
            if n % 7 == 5:
                p[1::2, n] = np.float32(1.0 / C) if dtype == np.float32 else 1.0 / C
    for n in range(1, N, 5):
        c0 = (n + 1) % C
        p[:, n, c0] = 0.0
        rest = p[:, n].sum(-1)
        p[rest == 0, n, (c0 + 1) % C] = 1.0                                     # (a one-hot row that sat on c0 moves on)
        p[:, n] /= p[:, n].sum(-1, keepdims=True)                              # rows stay probabilities: the largest is at least 1 / C
        y[n] = c0
    P = np.full((S, N, LDP), np.nan, dtype)
    P[:, :, :C] = p.astype(dtype)
    return P, y.astype(np.int32)


def dyadic(S=8, N=24, C=4, seed=3):
    """Probabilities k / 8: every sum is exact.  Points 0 .. 5 have planted exact ties of pbar (and of single samples) between classes
    that are not the first; the rest are random multiples of 1/8.  -> (P float32 [S, N, LDP], labels)."""
    rng = np.random.default_rng(seed)
    p = np.zeros((S, N, C))
    for n in range(N):
        for s in range(S):
            k = rng.multinomial(8, np.ones(C) / C)
            p[s, n] = k / 8.0
    p[:, 0] = [0.25, 0.25, 0.25, 0.25][:C]                                   # every class ties, in every sample and in the mean
    p[:, 1] = [0.0, 0.5, 0.5, 0.0][:C]                                       # classes 1 and 2 tie everywhere: the first of them wins
    p[0::2, 2], p[1::2, 2] = [0.0, 0.0, 1.0, 0.0][:C], [0.0, 0.0, 0.0, 1.0][:C]     # the samples disagree, the mean ties 2 with 3
    p[0::2, 3], p[1::2, 3] = [0.5, 0.0, 0.5, 0.0][:C], [0.0, 0.5, 0.0, 0.5][:C]     # ties inside every sample, a four-way tie in the mean
    p[:, 4] = [0.125, 0.375, 0.125, 0.375][:C]
    p[:, 5] = [0.0, 0.0, 0.0, 1.0][:C]
    P = np.full((S, N, LDP), np.nan, np.float32)
    P[:, :, :C] = p
    return P, rng.integers(0, C, N).astype(np.int32)


# ---------------------------------------------------------------------- calibration
def bin_of(confidence, n_bins):
    return min(n_bins - 1, max(0, int(math.ceil(float(np.float64(confidence) * np.float64(n_bins)))) - 1))


def calibrate(confidence, correct, nll, brier, n_bins):
    """-> SimpleNamespace: count, good (int64 [n_bins]), sconf (longdouble [n_bins]), sum_nll, sum_brier (longdouble), n_correct, ece, mce,
    accuracy."""
    N = len(confidence)
    count, good, sconf = np.zeros(n_bins, np.int64), np.zeros(n_bins, np.int64), np.zeros(n_bins, LD)
    for cf, ok in zip(confidence, correct):
        b = bin_of(cf, n_bins)
        count[b] += 1
        good[b] += int(ok)
        sconf[b] += LD(cf)
    some = count > 0
    gap = np.abs(good[some] / count[some].astype(LD) - sconf[some] / count[some].astype(LD))
    return SimpleNamespace(count=count, good=good, sconf=sconf, sum_nll=np.asarray(nll).astype(LD).sum(), sum_brier=np.asarray(brier).astype(LD).sum(),
                           n_correct=int(np.asarray(correct).sum()), accuracy=float(np.asarray(correct).sum()) / N,
                           ece=float((count[some] / LD(N) * gap).sum()), mce=float(gap.max()) if gap.size else 0.0)


def auroc_pairs(negative, positive):
    """P(positive > negative) + P(tie) / 2 by counting every pair."""
    neg, pos = np.asarray(negative, np.float64), np.asarray(positive, np.float64)
    wins = (pos[:, None] > neg[None, :]).sum() + 0.5 * (pos[:, None] == neg[None, :]).sum()
    return float(wins) / (len(neg) * len(pos))
