"""Per-weight convergence diagnostics of HMC chains on the GPU (csrc/rbnn_chain_diag.inc): the half of pyro's MCMC that the samplers of
hmc.py / conv_hmc.py dropped with it.  The reference runs its chains through pyro's MCMC, whose mcmc.diagnostics() / mcmc.summary() give a
split R-hat and an effective sample size per element of every sample site; hmc_history["r_hat_U"] is one split R-hat of one scalar and
multimodal.chains_pca a two-dimensional picture — neither says which weights have mixed, nor how many independent draws the stack is worth.

`diagnose` takes the pooled chain-major draws as one fp32 matrix [n_chains * n_draws, P] on the GPU and returns, per column, the pooled mean
and std, r_hat, split_r_hat, Geyer's tau with n_eff = n_chains * n_draws / tau, and n_pairs, the number of lag pairs the sum took
(pyro's ops.stats formulas; include/robustbnns_hip.h states them in full).  One lane per column, double precision, the chain mean
subtracted before any product.  `weight_diagnostics` is mcmc.diagnostics() for the stack of a train_hmc(num_chains=K) /
train_hmc_conv(num_chains=K) run, `diagnostics_summary` one line per parameter tensor, `print_summary` that table beside r_hat_U.
Single-chain runs keep only resampled draws, which are not a time series; plotting and storing the figures in hmc_history are out of scope."""
import collections

import numpy
import torch

from . import _hip
from .flat_params import require_gpu_fc

MIN_DRAWS = 4
MAX_DRAWS = _hip.CHAIN_DIAG_MAX_DRAWS          # rbnn_chain_diag's cap: the LDS of a CU at the narrowest tile
SLAB = 64                                      # slab borders are multiples of the widest tile (and keep a 16-byte base 16-byte aligned)
FIELDS = ("mean", "std", "r_hat", "split_r_hat", "tau", "n_eff", "n_pairs")
SUMMARY_COLUMNS = ["site", "size", "n_eff_min", "n_eff_median", "r_hat_max", "r_hat_above_1_1"]

ChainDiagnostics = collections.namedtuple("ChainDiagnostics", FIELDS)


def slab_plan(P, n_rows, ws_bytes=None):
    """[(e0, w)]: the column slabs of one diagnose() call, one launch each.  ws_bytes bounds the input bytes a launch sweeps (n_rows * w * 4);
    every slab but the last has the same whole number of SLAB-column groups, at least one; None: one slab.  A column's bits do not depend on
    the plan."""
    if ws_bytes is None:
        return [(0, P)]
    w = max(1, int(ws_bytes) // (4 * n_rows * SLAB)) * SLAB
    return [(e0, min(w, P - e0)) for e0 in range(0, P, w)]


def _check_rows(rows, n_chains):
    """Every refusal of diagnose(), before the library is loaded -> (n_draws, P, row stride)."""
    if not isinstance(rows, torch.Tensor) or rows.dim() != 2:
        raise ValueError("diagnose() takes a 2-D tensor [n_chains * n_draws, P]")
    if rows.dtype != torch.float32:
        raise ValueError(f"diagnose() takes float32 rows, not {rows.dtype}")
    n, P, K = int(rows.shape[0]), int(rows.shape[1]), int(n_chains)
    if K < 1:
        raise ValueError(f"diagnose() needs n_chains >= 1, not {n_chains}")
    if P < 1:
        raise ValueError(f"diagnose() needs at least one column, not {tuple(rows.shape)}")
    if n % K:
        raise ValueError(f"the rows hold {n} draws, not a multiple of their {K} chains")
    draws = n // K
    if not MIN_DRAWS <= draws <= MAX_DRAWS:
        raise ValueError(f"diagnose() takes {MIN_DRAWS} <= draws per chain <= {MAX_DRAWS} (the kernel's lag accumulators sit in LDS), not {draws}")
    if P > 1 and rows.stride(1) != 1:
        raise ValueError(f"diagnose() takes rows with stride(1) == 1, not {rows.stride(1)}")
    if rows.stride(0) < P:
        raise ValueError(f"diagnose() takes a row stride >= P = {P}, not {rows.stride(0)}")
    require_gpu_fc("Chain diagnostics", device=rows.device)
    return draws, P, int(rows.stride(0))


def diagnose(rows, n_chains, ws_bytes=None):
    """rows: fp32 [n_chains * n_draws, P] on the GPU, chain-major (row c * n_draws + t is draw t of chain c), stride(1) == 1, any row stride
    >= P -> ChainDiagnostics(mean, std, r_hat, split_r_hat, tau, n_eff: float64 [P]; n_pairs: int32 [P]) on the GPU."""
    if ws_bytes is not None and int(ws_bytes) < 1:
        raise ValueError(f"diagnose() needs a positive byte budget, not {ws_bytes}")
    draws, P, ld = _check_rows(rows, n_chains)
    lib = _hip.load()
    out = [torch.empty(P, dtype=torch.int32 if f == "n_pairs" else torch.float64, device=rows.device) for f in FIELDS]
    st = _hip.stream_of(rows)
    for e0, w in slab_plan(P, int(rows.shape[0]), ws_bytes):
        _hip.check(lib.rbnn_chain_diag(rows.data_ptr() + 4 * e0, ld, int(n_chains), draws, w,
                                       *(o.data_ptr() + o.element_size() * e0 for o in out), st), "rbnn_chain_diag")
    return ChainDiagnostics(*out)


def _stack_rows(net, who):
    """-> (fp32 [K * draws, P], K, the parameter keys and shapes) of the pooled chains of a lockstep run."""
    from .multimodal import _flatten
    hist = getattr(net, "hmc_history", None) or {}
    if "stack" not in hist:
        raise ValueError(f"{who}() needs the pooled chains of a train_hmc(num_chains=K) or train_hmc_conv(num_chains=K) run with K > 1: "
                         "this net's hmc_history has no \"stack\" (a one-chain run keeps only resampled draws, which are not a time series)")
    stack, K = hist["stack"], len(hist["chains"])
    keys = [k for k, _ in net.basenet.named_parameters()]
    return _flatten(stack, keys), K, [(k, tuple(stack[k].shape[1:])) for k in keys]


def weight_diagnostics(net):
    """pyro's mcmc.diagnostics() for net.hmc_history["stack"]: an OrderedDict state_dict key -> {"n_eff", "r_hat", "tau"} (float64) and
    "n_pairs" (int32), each of that parameter's shape, on the GPU.  r_hat is the split form, as in pyro.  fc, fc2 and conv stacks."""
    W, K, shapes = _stack_rows(net, "weight_diagnostics")
    d = diagnose(W, K)
    out, off = collections.OrderedDict(), 0
    for k, shape in shapes:
        n = int(numpy.prod(shape, dtype=numpy.int64))
        cut = lambda t: t[off:off + n].reshape(shape)
        out[k] = {"n_eff": cut(d.n_eff), "r_hat": cut(d.split_r_hat), "tau": cut(d.tau), "n_pairs": cut(d.n_pairs)}
        off += n
    return out


def summary_line(site, n_eff, r_hat):
    """One line of diagnostics_summary from float64 host arrays.  A constant weight has no n_eff (NaN): the minimum and the median (numpy's:
    the mean of the two middle values of an even count) skip it; r_hat_above_1_1 is the share of elements above 1.1."""
    n_eff, r_hat = numpy.asarray(n_eff, dtype=numpy.float64).ravel(), numpy.asarray(r_hat, dtype=numpy.float64).ravel()
    some = bool((~numpy.isnan(n_eff)).any())
    return {"site": site, "size": int(r_hat.size),
            "n_eff_min": float(numpy.nanmin(n_eff)) if some else float("nan"),
            "n_eff_median": float(numpy.nanmedian(n_eff)) if some else float("nan"),
            "r_hat_max": float(r_hat.max()), "r_hat_above_1_1": float((r_hat > 1.1).mean())}


def diagnostics_summary(net):
    """pyro's mcmc.summary() in one line per parameter tensor and an "all" line -> DataFrame site, size, n_eff_min, n_eff_median, r_hat_max,
    r_hat_above_1_1."""
    import pandas
    diag = weight_diagnostics(net)
    host = [(k, v["n_eff"].cpu().numpy().ravel(), v["r_hat"].cpu().numpy().ravel()) for k, v in diag.items()]
    lines = [summary_line(*h) for h in host]
    lines.append(summary_line("all", numpy.concatenate([h[1] for h in host]), numpy.concatenate([h[2] for h in host])))
    return pandas.DataFrame(lines, columns=SUMMARY_COLUMNS)


def print_summary(net):
    """The summary beside the run's one scalar figure, hmc_history["r_hat_U"] -> the DataFrame."""
    df = diagnostics_summary(net)
    print(df.to_string(index=False))
    print(f"r_hat_U (split R-hat of the chains' potential): {net.hmc_history.get('r_hat_U', float('nan')):.4f}")
    return df
