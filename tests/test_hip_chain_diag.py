"""Per-weight chain diagnostics on the GPU (csrc/rbnn_chain_diag.inc, chain_diagnostics.py) against the numpy.longdouble restatement of
tests/chain_diag_restate.py, then exactness on integer draws, the bit contracts (torch.equal throughout), the layouts and the drivers.
Every test fails on a tree without the feature, where the module does not exist.

The bar is derived, not measured.  u = 2^-53; per column A = max |x| and s = sqrt(min_c gamma[c,0]); B = 4 N^1.5 u (1 + A / s).
  * The chain mean is a sum of N terms of size <= A in ascending t and one division: |m' - m_c| <= N u A (what `mean` is held to, absolute:
    the pooled mean is the mean of the chains' means).
  * Every d of a chain is therefore shifted by the same eps, |eps| <= N u A, and rounded once (u |d|).  The computed
    S'[c,k] = sum (d_t - eps)(d_t+k - eps) differs from S[c,k] by eps (sum d_t + sum d_t+k) + (N - k) eps^2, at most
    2 (N - k) N u A max|d| with max|d| <= sqrt(S[c,0]) = sqrt(N gamma[c,0]): in gamma[c,k] that is 2 N^1.5 u A sqrt(gamma[c,0]), i.e.
    2 N^1.5 u (A / s) relative to gamma[c,0].
  * The N - k fma's of a lag sum add at most (N - k) u sum |d_t d_t+k| <= (N - k) u S[c,0] (Cauchy-Schwarz): N u gamma[c,0] in gamma[c,k];
    the single roundings of d (2 u each way) and of the division are of that size too: together below N^1.5 u gamma[c,0] for N >= 4.
  * So every gamma[c,k] is within (B / 2) gamma[c,0] of its value, and the chain averages within (B / 2) mean_c gamma[c,0].  W is such an
    average; V adds the spread of the means, whose error 2 sqrt(spread) N u A is below (B / 2) V because sqrt(spread) <= sqrt(V) and
    sqrt(V) >= s sqrt((N - 1) / N).  std^2 is the same two sums.  Ratios and square roots of quantities within B / 2: std, r_hat and
    split_r_hat (the same argument at h = N // 2 < N) within 2 B relative — a factor 2 to spare.
  * rho_k = 1 - (W - mean_c gamma[c,k]) / V moves by at most B, a pair sum Rho_p by 2 B, and tau = -1 + 2 sum of at most N / 2 terms, each a
    running minimum of pair sums, by 2 N B: held to 4 N B absolute.  n_eff = C N / tau within 4 N B / (tau - 4 N B) relative.
  * The stopping pair is decided by the sign of a pair sum: a column is compared for tau, n_eff and n_pairs only where every |Rho_p| up to
    and including the stopping pair is at least 1e-6 in the restatement, far above 2 B (at most 7e-8 in these cases); n_eff only where
    tau >= 0.1 (short chains give tau <= 0 by the formula: 9 of 37, 4 of 37 and 4 of 130 columns at N = 8, 9, 33 and none at N >= 64, where
    the test caps the share at 5 % as it does for the margin, which removes no column of this recipe).
The offset-1000 cases are what an fp32 centring or an E[x^2] - m^2 formula fails: A / s reaches 1e5 there and the bar scales with it, while
those forms lose A^2 u / s^2.

Measured on one MI355X (profiles/chain_diag/parity.txt): the worst error of every quantity over the seven cases, in units of its bar."""
import collections
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import chain_diag_restate as R
from robustbnns_amd import _hip

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("built_library")]
DEV = "cuda:0"
_cache = {}


def D():
    from robustbnns_amd import chain_diagnostics
    return chain_diagnostics


def case(C_, N, P, offset):
    """(fp32 matrix [C N, P] on the host, its restatement): computed once per case and left unchanged."""
    key = (C_, N, P, offset)
    if key not in _cache:
        x = R.planted(C_, N, P, offset)
        _cache[key] = (R.as_rows(x), R.Restated(x))
    return _cache[key]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(d):
    return {k: v.cpu().numpy() for k, v in d._asdict().items()}


def same(a, b):
    """Two ChainDiagnostics (or tensors) bit for bit; NaN equals NaN."""
    if isinstance(a, torch.Tensor):
        return a.dtype == b.dtype and a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan()) if a.is_floating_point() else (a == b)).all())
    return all(same(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("C_,N,P,offset", R.CASES)
def test_every_quantity_is_within_its_derived_bar(C_, N, P, offset):
    X, ref = case(C_, N, P, offset)
    d = D().diagnose(dev(X), C_)
    for k, v in d._asdict().items():
        assert v.shape == (P,) and v.device.type == "cuda" and v.dtype == (torch.int32 if k == "n_pairs" else torch.float64), k
    ref.ratios(f"offset {offset}", host(d), capped=N >= 64)


# ------------------------------------------------------------------ exactness
def test_integer_draws_give_the_exact_stopping_pair_and_tau():
    """Draws in -8 .. 8, N = 16: the means, every d and every lag sum are exact in fp64; what is rounded is one division per gamma and the
    O(N) operations behind them — n_pairs equals the Fraction restatement and tau lies within 64 N u of it."""
    Cn, N, P = 2, 16, 70
    rng = np.random.default_rng(16)
    x = rng.integers(-8, 9, (Cn, N, P)).astype(np.float32)
    d = host(D().diagnose(dev(R.as_rows(x)), Cn))
    worst = 0.0
    for e in range(P):
        n_pairs, tau = R.exact_tau(x[:, :, e].tolist())
        assert d["n_pairs"][e] == n_pairs, e
        worst = max(worst, abs(float(d["tau"][e]) - float(tau)))
        assert abs(Fraction(float(d["tau"][e])) - tau) <= 64 * N * R.U, e
    print(f"[chain_diag exact] worst |tau - exact| = {worst:.2e} (allowed {64 * N * R.U:.2e})")


def test_constant_columns_follow_the_convention():
    """W == 0: r_hat and split_r_hat 1 when the levels agree and inf when they differ, tau and n_eff NaN, n_pairs 0; the columns beside them
    are untouched by it."""
    Cn, N, P = 3, 10, 5
    rng = np.random.default_rng(3)
    x = rng.standard_normal((Cn, N, P)).astype(np.float32)
    x[:, :, 1] = 2.5                                             # constant
    x[:, :, 3] = np.array([1.0, 1.0, 4.0])[:, None]              # constant per chain, different levels
    d = host(D().diagnose(dev(R.as_rows(x)), Cn))
    ref = R.Restated(x)
    for e, r in ((1, 1.0), (3, np.inf)):
        assert d["r_hat"][e] == r and d["split_r_hat"][e] == r and np.isnan(d["tau"][e]) and np.isnan(d["n_eff"][e]) and d["n_pairs"][e] == 0
        assert ref.r_hat[e] == r and ref.split_r_hat[e] == r and np.isnan(ref.tau[e]) and ref.n_pairs[e] == 0
    assert d["mean"][1] == 2.5 and d["std"][1] == 0.0 and d["mean"][3] == 2.0 and abs(d["std"][3] - ref.std[3]) <= 1e-15
    live = [0, 2, 4]
    assert np.isfinite(d["tau"][live]).all() and (d["n_pairs"][live] == ref.n_pairs[live]).all()
    assert np.abs(d["r_hat"][live] - ref.r_hat[live]).max() <= 1e-13


# ------------------------------------------------------------------ structure
def raw(X, ld, Cn, N, P, outs):
    _hip.check(_hip.load().rbnn_chain_diag(X, ld, Cn, N, P, *outs, _hip.stream_of(torch.empty(0, device=DEV))), "rbnn_chain_diag")


@pytest.mark.parametrize("C_,N,P,offset", [(2, 9, 37, 0), (4, 64, 300, 1000), (8, 250, 64, 0)])       # the three tile widths
def test_bits_depend_on_the_column_alone(C_, N, P, offset):
    Xh, _ = case(C_, N, P, offset)
    X = dev(Xh)
    full = D().diagnose(X, C_)
    assert same(D().diagnose(X, C_), full)                                      # two runs
    # two byte budgets: one 64-column group per launch, and two
    for groups in (1, 2):
        budget = groups * 64 * C_ * N * 4
        assert len(D().slab_plan(P, C_ * N, budget)) == -(-P // (64 * groups))
        assert same(D().diagnose(X, C_, ws_bytes=budget), full)
    # columns [j0, j1) alone: contiguous, then with another row stride and a base one float off the 16-byte grid (the scalar-load path)
    for j0, j1 in ((0, 1), (5, 23), (P - 17, P), (16, min(P, 90))):
        w = j1 - j0
        alone = D().diagnose(X[:, j0:j1].contiguous(), C_)
        assert same(alone, [v[j0:j1] for v in full]), (j0, j1)
        buf = torch.full((C_ * N * (w + 3) + 1,), float("nan"), dtype=torch.float32, device=DEV)
        view = buf[1:].view(C_ * N, w + 3)[:, :w]
        view.copy_(X[:, j0:j1])
        assert view.data_ptr() % 16 == 4 and view.stride(0) == w + 3
        assert same(D().diagnose(view, C_), alone), (j0, j1)
        # a view into the full matrix: the row stride P, the base wherever column j0 lies
        assert same(D().diagnose(X[:, j0:j1], C_), alone), (j0, j1)


def test_canaries_stay_and_null_outputs_are_left_out():
    C_, N, P, offset = 4, 64, 300, 0
    Xh, _ = case(C_, N, P, offset)
    X = dev(Xh)
    full = D().diagnose(X, C_)
    pad = 9

    def buffers():
        return [torch.full((P + pad,), -77, dtype=torch.int32, device=DEV) if f == "n_pairs"
                else torch.full((P + pad,), float("nan"), dtype=torch.float64, device=DEV) for f in D().FIELDS]
    outs = buffers()
    raw(X.data_ptr(), P, C_, N, P, [o.data_ptr() for o in outs])
    for f, o, want in zip(D().FIELDS, outs, full):
        assert same(o[:P], want), f
        assert bool((o[P:] == -77).all()) if f == "n_pairs" else bool(o[P:].isnan().all()), f
    # every output alone, and all but one: what is null is not written, what is not has the same bits
    for i, f in enumerate(D().FIELDS):
        for keep in ([i], [j for j in range(7) if j != i]):
            outs = buffers()
            raw(X.data_ptr(), P, C_, N, P, [outs[j].data_ptr() if j in keep else None for j in range(7)])
            for j in range(7):
                if j in keep:
                    assert same(outs[j][:P], full[j]), (f, j)
                else:
                    assert bool((outs[j] == -77).all()) if j == 6 else bool(outs[j].isnan().all()), (f, j)


# ------------------------------------------------------------------ drivers
class Basenet:
    """What the drivers read of a net's basenet: named_parameters() in the state_dict's order."""

    def __init__(self, shapes):
        self.shapes = shapes

    def named_parameters(self):
        return [(k, torch.empty(s)) for k, s in self.shapes]


def hand_built(arch, H, K=3, draws=6):
    from oracle import bnn_oracle as O
    shapes = O.param_shapes(arch, 784, H, 10)
    g = torch.Generator().manual_seed(len(arch) + H)
    level = {k: torch.randn(s, generator=g) for k, s in shapes}
    stack = {k: torch.cat([level[k].unsqueeze(0) + 1.0 * c + 0.05 * torch.randn((draws,) + tuple(s), generator=g).cumsum(0)
                           for c in range(K)]).to(DEV) for k, s in shapes}
    return SimpleNamespace(hmc_history={"stack": stack, "chains": [{}] * K, "r_hat_U": 1.23}, basenet=Basenet(shapes)), shapes, K


@pytest.mark.parametrize("arch,H", [("fc2", 16), ("conv", 16), ("fc", 8)])
def test_weight_diagnostics_and_summary_follow_the_state_dict(arch, H, capsys):
    net, shapes, K = hand_built(arch, H)
    diag = D().weight_diagnostics(net)
    assert isinstance(diag, collections.OrderedDict) and list(diag) == [k for k, _ in shapes]
    flat = torch.cat([net.hmc_history["stack"][k].reshape(K * 6, -1) for k, _ in shapes], 1).contiguous()
    d = D().diagnose(flat, K)
    off = 0
    for k, s in shapes:
        n = int(np.prod(s))
        assert set(diag[k]) == {"n_eff", "r_hat", "tau", "n_pairs"}
        for name, src in (("n_eff", d.n_eff), ("r_hat", d.split_r_hat), ("tau", d.tau), ("n_pairs", d.n_pairs)):
            assert tuple(diag[k][name].shape) == tuple(s) and diag[k][name].dtype == src.dtype, (k, name)
            assert same(diag[k][name].reshape(-1), src[off:off + n]), (k, name)
        off += n
    assert off == flat.shape[1]
    df = D().diagnostics_summary(net)
    assert list(df.columns) == D().SUMMARY_COLUMNS and df["site"].tolist() == [k for k, _ in shapes] + ["all"]
    assert df["size"].tolist() == [int(np.prod(s)) for _, s in shapes] + [flat.shape[1]]
    n_eff, r_hat = d.n_eff.cpu().numpy(), d.split_r_hat.cpu().numpy()
    last = df.iloc[-1]
    assert last["n_eff_min"] == np.nanmin(n_eff) and last["n_eff_median"] == np.nanmedian(n_eff)
    assert last["r_hat_max"] == r_hat.max() and last["r_hat_above_1_1"] == (r_hat > 1.1).mean()
    k0, s0 = shapes[1]
    first = df.iloc[1]
    n0 = int(np.prod(shapes[0][1]))
    assert first["site"] == k0 and first["n_eff_min"] == np.nanmin(n_eff[n0:n0 + int(np.prod(s0))])
    # the chains were planted 1.0 apart with a spread far below it: nothing has mixed, and the summary says so
    assert last["r_hat_above_1_1"] > 0.9
    capsys.readouterr()
    assert D().print_summary(net).equals(df)
    text = capsys.readouterr().out
    assert "r_hat_U" in text and "1.2300" in text and "n_eff_median" in text
