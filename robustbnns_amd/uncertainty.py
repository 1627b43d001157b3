"""Posterior-predictive uncertainty and calibration on the GPU (csrc/rbnn_predictive.inc): what the per-sample probabilities of a forward
say beyond their mean.  Every forward of this package ends in the mean over the samples; the questions a user of a Bayesian-robustness code
base asks next — how uncertain is the net on the adversarial points, is that disagreement between posterior samples (epistemic) or not
(aleatoric), is the predictive calibrated, does the uncertainty detect the attack — need the samples themselves.

Per point, from p_s[c] (sample s, class c), pbar = mean_s p_s, natural logarithms, 0 ln 0 = 0, double precision from the first sum on
(include/robustbnns_hip.h states the definitions in full):
    entropy = -sum_c pbar ln pbar,  expected_entropy = mean_s (-sum_c p_s ln p_s),  mutual_information = their difference (unclamped),
    prediction = first argmax of pbar,  confidence = pbar[prediction],  agreement = share of samples whose own argmax is the prediction,
    variance = population variance over s of p_s[prediction] (Welford);  with labels: nll = -ln pbar[y], brier, correct.
`AttackEngine.uncertainty` / `sample_outputs` (and ConvEngine's, ConvFp64Engine's) run it on the P their forward kernels wrote;
`predictive_uncertainty` does so for a BNN, an Ensemble_NN or an NN, `calibration` bins a result by confidence (ECE, MCE, the bin table),
`attack_uncertainty` is attack_evaluation's companion: the figures of the clean and the adversarial set side by side and how well each
score tells them apart (AUROC).  Uncertainty under a process group, an uncertainty-driven attack loss and plotting are out of scope."""
import collections
import random

import numpy
import torch

from . import _hip

FIELDS = ("entropy", "expected_entropy", "mutual_information", "confidence", "agreement", "variance", "nll", "brier", "prediction", "correct")
INT_FIELDS = ("prediction", "correct")
LABEL_FIELDS = ("nll", "brier", "correct")
MAX_PREFIXES = _hip.PREDICTIVE_MAX_PREFIXES
MAX_BINS = _hip.PREDICTIVE_MAX_BINS
# the score of each AUROC: higher = more suspect
AUROC_SCORES = {"auroc_entropy": lambda u: u.entropy, "auroc_mutual_information": lambda u: u.mutual_information,
                "auroc_confidence": lambda u: 1.0 - u.confidence}

PredictiveUncertainty = collections.namedtuple("PredictiveUncertainty", FIELDS)


# ---------------------------------------------------------------------- what is refused before the library is loaded
def check_prefixes(n_samples, n_samples_list):
    """-> the prefix lengths of a call: [n_samples], or n_samples_list — 1 .. MAX_PREFIXES strictly ascending lengths in 1 .. n_samples."""
    S = int(n_samples)
    if S < 1:
        raise ValueError(f"uncertainty() needs n_samples >= 1, not {n_samples}")
    if n_samples_list is None:
        return [S]
    pre = [int(v) for v in n_samples_list]
    if not pre:
        raise ValueError("n_samples_list is empty: leave it None for the one figure of n_samples, or name the prefix lengths")
    if len(pre) > MAX_PREFIXES:
        raise ValueError(f"n_samples_list holds {len(pre)} lengths, one call takes {MAX_PREFIXES}: split the list over several calls")
    if any(b <= a for a, b in zip(pre, pre[1:])):
        raise ValueError(f"n_samples_list {pre} is not strictly ascending: sort it and drop the repeats")
    if pre[0] < 1 or pre[-1] > S:
        raise ValueError(f"n_samples_list {pre} leaves 1 .. n_samples = {S}: raise n_samples to its largest entry")
    return pre


def check_bins(n_bins):
    if not 1 <= int(n_bins) <= MAX_BINS:
        raise ValueError(f"calibration() takes 1 <= n_bins <= {MAX_BINS}, not {n_bins}: merge bins of a finer table on the host")
    return int(n_bins)


def check_engine(eng, what):
    """The two refusals of an engine: more than one rank, and anything but the HIP kernels on the GPU."""
    if getattr(eng, "world", 1) > 1:
        raise NotImplementedError(f"{what} is not built under a process group (world size {eng.world}): every rank holds a part of the "
                                  "samples only; build a single-GPU engine on the whole posterior (make_engine(posterior) without a group)")
    if torch.device(eng.device).type != "cuda" or not isinstance(eng.k, _hip.HipKernels):
        raise NotImplementedError(f"{what} runs on the MI355X kernels only (device {str(eng.device)!r}): there is no CPU compute path; "
                                  "load the net on 'cuda'")


def check_labels(y, N):
    """one-hot [N, C] or integer [N] labels -> integer labels [N] (on y's device); None stays None."""
    if y is None:
        return None
    y = torch.as_tensor(y)
    if y.dim() >= 2:
        y = y.argmax(-1)
    if y.numel() != N:
        raise ValueError(f"y holds {y.numel()} labels for {N} points: pass one label per row of x, or leave y out")
    return y.reshape(-1)


# ---------------------------------------------------------------------- engine level
def engine_sample_outputs(eng, x, n_samples, seeds=None):
    """[S, N, C]: the per-sample probabilities the engine's forward kernels wrote for x, a copy (float32; float64 from the fp64 checkers)."""
    from .engine import AttackEngine
    check_engine(eng, "sample_outputs()")
    sidx, S = AttackEngine.sample_index(eng, n_samples, seeds)
    out, Cn = None, eng.post.C
    for lo, hi, P in eng._sample_blocks(x, sidx, S):
        if out is None:
            out = torch.empty(S, x.shape[0], Cn, dtype=P.dtype, device=P.device)
        out[:, lo:hi] = P[:, :, :Cn]
    return out


def engine_uncertainty(eng, x, n_samples, y=None, seeds=None, n_samples_list=None):
    """PredictiveUncertainty of the rows of x on the GPU: float64 (prediction, correct: int32) [N], or [J, N] with n_samples_list (row j: the
    first n_samples_list[j] samples of the call, bit for bit the figures of a call with that n_samples); nll, brier, correct None without y."""
    from .engine import AttackEngine, to_labels
    prefixes = check_prefixes(n_samples, n_samples_list)
    N = int(x.shape[0])
    y = check_labels(y, N)
    if N < 1:
        raise ValueError("uncertainty() needs at least one point")
    check_engine(eng, "uncertainty()")
    sidx, S = AttackEngine.sample_index(eng, n_samples, seeds)
    labels = None if y is None else to_labels(y, eng.device)
    J = len(prefixes)
    out = {f: torch.empty(J, N, dtype=torch.int32 if f in INT_FIELDS else torch.float64, device=eng.device)
           for f in FIELDS if labels is not None or f not in LABEL_FIELDS}
    for lo, hi, P in eng._sample_blocks(x, sidx, S):
        eng.k.predictive_stats(P, eng.post.C, None if labels is None else labels[lo:hi], prefixes, out, lo)
    pick = (lambda t: t) if n_samples_list is not None else (lambda t: t[0])
    return PredictiveUncertainty(*(pick(out[f]) if f in out else None for f in FIELDS))


def concat(parts):
    """The records of consecutive point blocks as one."""
    return PredictiveUncertainty(*(None if p0 is None else torch.cat(col, -1) for p0, col in ((c[0], c) for c in zip(*parts))))


# ---------------------------------------------------------------------- nets
def _engine_of(net, n_samples, seeds, n_samples_list, avg_posterior):
    """(engine, S, seeds) from the hot path of a BNN / Ensemble_NN / NN, after every refusal that needs no library."""
    from . import adversarialAttacks as A
    from .model_bnn import BNN
    if avg_posterior:
        raise ValueError("avg_posterior=True is one net of mean weights, not a distribution: it has no predictive uncertainty; "
                         "leave avg_posterior False and choose n_samples")
    device = getattr(net, "device", None)
    if device is not None and torch.device(device).type != "cuda":
        raise NotImplementedError(f"predictive uncertainty runs on the MI355X kernels only (device {str(device)!r}): there is no CPU compute "
                                  "path; load the net on 'cuda'")
    if n_samples is None:
        if n_samples_list is not None and len(n_samples_list):
            n_samples = max(int(v) for v in n_samples_list)
        elif isinstance(net, BNN):
            n_samples = 10                                  # BNN.forward's default
    if n_samples is not None:
        check_prefixes(n_samples, n_samples_list)
    if isinstance(net, BNN) and seeds:
        eng, S, sd, _ = net.hot_path(n_samples, False, seeds)
    else:
        eng, S, sd, _ = A._hot_path(net, n_samples, False)
    return eng, S, sd


def predictive_uncertainty(net, x, n_samples=None, y=None, seeds=None, n_samples_list=None, avg_posterior=False):
    """The predictive uncertainty of `net` on the rows of x -> PredictiveUncertainty (GPU tensors).  net: a BNN (hmc: the stored samples,
    svi: fresh draws, or `seeds`; every architecture), an Ensemble_NN (the members are the samples, each with its own softmax) or an NN
    (one sample: entropy == expected_entropy, no epistemic part).  n_samples None: the largest of n_samples_list, else 10 for a BNN
    (BNN.forward's default), every member of an ensemble, 1 for an NN.
    An ensemble's `prediction` is the argmax of the mean PROBABILITY over the members; Ensemble_NN.forward averages the members' LOGITS and
    its argmax can differ where the members disagree."""
    eng, S, sd = _engine_of(net, n_samples, seeds, n_samples_list, avg_posterior)
    return eng.uncertainty(x.to(eng.device), S, y=y, seeds=sd, n_samples_list=n_samples_list)


# ---------------------------------------------------------------------- calibration
def bin_of(confidence, n_bins):
    """The bin of a confidence, the kernel's expression restated: intervals (lo, hi], confidence 0 in the first."""
    import math
    return min(n_bins - 1, max(0, int(math.ceil(confidence * n_bins)) - 1))


def calibration(unc, n_bins=15):
    """Reliability of a PredictiveUncertainty with labels ([N] fields: pick a row of a prefix result first) -> dict: accuracy, nll and brier
    (means), ece = sum_b (n_b / N) |acc_b - conf_b|, mce = max_b |acc_b - conf_b| over the non-empty bins, n_bins, `bins`, a DataFrame
    lo, hi, count, confidence, accuracy per bin (NaN where a bin is empty), and `sums`, the kernel's sums as they came.  The sums come from rbnn_predictive_calibration (fixed order, no
    atomics); the handful of divisions run in float64 on the host."""
    import ctypes as C
    nb = check_bins(n_bins)
    if unc.correct is None:
        raise ValueError("calibration() needs the figures that labels give (nll, brier, correct): call uncertainty(..., y=labels)")
    if unc.confidence.dim() != 1:
        raise ValueError(f"calibration() takes the [N] figures of one n_samples, not {tuple(unc.confidence.shape)}: pick a row of the "
                         "n_samples_list result, e.g. PredictiveUncertainty(*(f[j] for f in unc))")
    conf, N = unc.confidence.contiguous(), int(unc.confidence.shape[0])
    dev = conf.device
    if dev.type != "cuda":
        raise NotImplementedError(f"calibration() runs on the MI355X kernels only (device {str(dev)!r}): there is no CPU compute path")
    lib = _hip.load()
    need = C.c_size_t(0)
    _hip.check(lib.rbnn_predictive_calibration_query(N, nb, C.byref(need)), "rbnn_predictive_calibration_query")
    ws = torch.empty(need.value // 8, dtype=torch.int64, device=dev)
    count, good = torch.empty(nb, dtype=torch.int64, device=dev), torch.empty(nb, dtype=torch.int64, device=dev)
    sconf, totals = torch.empty(nb, dtype=torch.float64, device=dev), torch.empty(2, dtype=torch.float64, device=dev)
    n_correct = torch.empty(1, dtype=torch.int64, device=dev)
    _hip.check(lib.rbnn_predictive_calibration(_hip.ptr(conf), _hip.ptr(unc.correct.contiguous()), _hip.ptr(unc.nll.contiguous()),
                                               _hip.ptr(unc.brier.contiguous()), N, nb, _hip.ptr(count), _hip.ptr(sconf), _hip.ptr(good),
                                               _hip.ptr(totals), _hip.ptr(n_correct), _hip.ptr(ws), need.value, _hip.stream_of(conf)),
               "rbnn_predictive_calibration")
    return calibration_from_sums(count.cpu().numpy(), sconf.cpu().numpy(), good.cpu().numpy(), totals.cpu().numpy(), int(n_correct.item()), N)


def calibration_from_sums(count, sconf, good, totals, n_correct, N):
    """The host half of calibration(): float64 divisions of the kernel's sums."""
    import pandas
    nb = len(count)
    some = count > 0
    cnt = numpy.where(some, count, 1).astype(numpy.float64)
    conf_b = numpy.where(some, sconf / cnt, numpy.nan)
    acc_b = numpy.where(some, good.astype(numpy.float64) / cnt, numpy.nan)
    gap = numpy.abs(acc_b - conf_b)[some]
    ece = float(((count[some].astype(numpy.float64) / float(N)) * gap).sum())
    edges = numpy.arange(nb + 1, dtype=numpy.float64) / nb
    bins = pandas.DataFrame({"lo": edges[:-1], "hi": edges[1:], "count": count, "confidence": conf_b, "accuracy": acc_b})
    return {"accuracy": n_correct / float(N), "nll": float(totals[0]) / N, "brier": float(totals[1]) / N, "ece": ece,
            "mce": float(gap.max()) if gap.size else 0.0, "n_bins": nb, "bins": bins,
            "sums": {"count": count, "confidence": sconf, "correct": good, "nll": float(totals[0]), "brier": float(totals[1]), "n_correct": n_correct}}


# ---------------------------------------------------------------------- attacks
def auroc(score_negative, score_positive):
    """The Mann-Whitney statistic P(positive > negative) + P(tie) / 2 of two score vectors, ties sharing average ranks: float64 torch on the
    scores' device -> a Python float."""
    neg, pos = score_negative.reshape(-1).double(), score_positive.reshape(-1).double()
    n0, n1 = neg.numel(), pos.numel()
    if not n0 or not n1:
        raise ValueError("auroc() needs at least one score of each class")
    _, inv, counts = torch.unique(torch.cat([neg, pos]), return_inverse=True, return_counts=True)
    counts = counts.double()
    rank = (counts.cumsum(0) - (counts - 1.0) / 2.0)[inv]                         # 1-based average rank of every score
    return float((rank[n0:].sum() - n1 * (n1 + 1) / 2.0) / (float(n0) * float(n1)))


def attack_uncertainty(net, x_test, x_attack, y_test, device, n_samples=None):
    """attack_evaluation's companion (the same seeding, ONE engine and the same samples for both sets) -> (DataFrame, summary).
    DataFrame: one row per point and set — kind ('clean' / 'adversarial'), idx, and the ten figures.  summary: 'mean' (the means of every
    figure per kind), 'calibration' (calibration() per kind) and auroc_entropy, auroc_mutual_information, auroc_confidence: how well
    entropy, mutual information and 1 - confidence separate the adversarial points (the positive class) from the clean ones."""
    import pandas
    from .model_bnn import set_rng_seed
    random.seed(0)
    set_rng_seed(0)                                        # adversarialAttacks.py:160-161, as attack_evaluation
    eng, S, sd = _engine_of(net, n_samples, None, None, False)
    if len(x_test) != len(x_attack):
        raise ValueError("\nInput arrays should have the same length.")
    unc = {"clean": eng.uncertainty(x_test.to(device), S, y=y_test, seeds=sd), "adversarial": eng.uncertainty(x_attack.to(device), S, y=y_test, seeds=sd)}
    frames = []
    for kind, u in unc.items():
        cols = {"kind": kind, "idx": numpy.arange(len(x_test))}
        cols.update({f: getattr(u, f).cpu().numpy() for f in FIELDS})
        frames.append(pandas.DataFrame(cols))
    summary = {"mean": {kind: {f: float(getattr(u, f).double().mean()) for f in FIELDS} for kind, u in unc.items()},
               "calibration": {kind: calibration(u) for kind, u in unc.items()}, "n_samples": S}
    for name, score in AUROC_SCORES.items():
        summary[name] = auroc(score(unc["clean"]), score(unc["adversarial"]))
    return pandas.concat(frames, ignore_index=True), summary
