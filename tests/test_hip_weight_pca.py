"""Weight-space PCA on the GPU (csrc/rbnn_wpca.inc, weight_pca.py, multimodal.py) against the float64 restatement of
tests/weight_pca_restate.py, which also derives the bar: scores within 8 B, unit-norm components within 8 B / sqrt(lambda1),
B = 2 (P + n) 2^-53 R sqrt(lambda1), R <= 8 asserted on the restatement's own spectrum before anything is compared.  Then the bit
contracts (torch.equal throughout), the layouts, the prior's generator and the drivers.  The shapes are the smallest at which each
mechanism can go wrong; every test fails on a tree without the feature, where the modules do not exist.

Measured on one MI355X (profiles/wpca/parity.txt): the worst error of any case is recorded there in units of B."""
import ctypes as C

import numpy as np
import pytest
import torch

import weight_pca_restate as R
from robustbnns_amd import _hip

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("built_library")]
DEV = "cuda:0"
CH = _hip.WPCA_CHUNK
KEY = 0x5EED0FC0FFEE1234
CASES = [(3, 7), (17, 7), (17, 4099), (50, 4099), (150, 1031), (1000, 64), (17, 3 * CH + 5)]
_cache = {}


def W():
    from robustbnns_amd import weight_pca
    return weight_pca


def case(n, P, offset=0.0):
    """(fp32 rows on the host, their restatement): computed once per shape and left unchanged."""
    if (n, P, offset) not in _cache:
        X = R.planted(n, P, offset)
        _cache[(n, P, offset)] = (X, R.Restated(X))
    return _cache[(n, P, offset)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def fit(X, **kw):
    return W().WeightPCA(2, device=DEV, **kw).fit(W().MatrixRows(X if isinstance(X, torch.Tensor) else dev(X)))


# ------------------------------------------------------------------ 1, 2: parity
@pytest.mark.parametrize("n,P", CASES)
def test_fit_transform_transform_and_components_match_the_restatement(n, P):
    X, ref = case(n, P)
    Y = R.fresh_rows(X, 5)
    pca = W().WeightPCA(2, device=DEV)
    scores = pca.fit_transform(W().MatrixRows(dev(X)))
    assert scores.dtype == torch.float64 and tuple(scores.shape) == (n, 2) and torch.equal(scores, pca.scores_)
    V = pca.components()
    assert V.dtype == torch.float64 and tuple(V.shape) == (2, P)
    T = pca.transform(W().MatrixRows(dev(Y)))
    assert tuple(T.shape) == (5, 2)
    ref.ratios("parity", scores=scores.numpy(), transform=(T.numpy(), Y), components=V.cpu().numpy())
    assert np.abs(pca.singular_values_.numpy() - ref.singular_values).max() <= R.MARGIN * ref.B
    assert np.abs(pca.explained_variance_.numpy() - ref.singular_values ** 2 / (n - 1)).max() <= R.MARGIN * ref.B * np.sqrt(ref.lam[0]) / (n - 1) * 2
    assert np.abs(pca.mean_.cpu().numpy() - ref.mean).max() <= 4 * n * 2.0 ** -53 * max(1.0, np.abs(X).max())
    # the fitted rows transform to their scores
    back = pca.transform(W().MatrixRows(dev(X)))
    ref.ratios("parity, the fitted rows transformed", transform=(back.numpy(), X))


def test_the_mean_is_subtracted_before_the_product():
    """Rows 1000 away from the origin with a spread of order 1: the same bar.  A Gram matrix of the raw rows corrected afterwards carries
    n 1000^2 P 2^-53 ~ 2e-5 of rounding into entries of order 10 and misses the bar by orders of magnitude."""
    X, ref = case(50, 4099, 1000.0)
    pca = fit(X)
    Y = R.fresh_rows(X, 5)
    out = ref.ratios("offset 1000", scores=pca.scores_.numpy(), transform=(pca.transform(W().MatrixRows(dev(Y))).numpy(), Y),
                     components=pca.components().cpu().numpy())
    # the restated after-the-fact form, for the record: it is what the bar excludes
    X64 = X.astype(np.float64)
    s = X64 @ ref.mean
    G_bad = X64 @ X64.T - s[:, None] - s[None, :] + ref.mean @ ref.mean
    G_good = (X64 - ref.mean) @ (X64 - ref.mean).T
    print(f"[wpca parity] offset 1000: |G corrected afterwards - G centred first| = {np.abs(G_bad - G_good).max():.2e}, "
          f"|gram_ - G centred first| = {np.abs(pca.gram_.cpu().numpy() - G_good).max():.2e}")
    assert np.abs(pca.gram_.cpu().numpy() - G_good).max() <= 4099 * 2.0 ** -53 * np.diag(G_good).max() * 2
    assert out["scores"] <= R.MARGIN


def test_sixteen_components_are_the_kernels_limit_and_match_their_formula():
    """k = 16, the axes kernel's register budget: scores of the two planted directions against the restatement, and every axis against
    V = (u / sqrt(lambda))^T (X - mean) evaluated in float64 on the host from the fitted u, lambda and mean — the two evaluations differ by
    their summation orders only: at most 2 n 2^-53 sum_i |A[k, i]| |x[i, e] - mean[e]| per element."""
    n, P, k = 20, 37, 16
    X, ref = case(n, P)
    pca = W().WeightPCA(k, device=DEV).fit(W().MatrixRows(dev(X)))
    ref.ratios("k = 16", scores=pca.scores_[:, :2].numpy(), components=pca.components()[:2].cpu().numpy())
    A = (pca.u_ / pca.singular_values_).t().numpy()
    Xc = X.astype(np.float64) - pca.mean_.cpu().numpy()
    V = pca.components().cpu().numpy()
    assert V.shape == (k, P) and (np.abs(V - A @ Xc) <= 2 * n * 2.0 ** -53 * (np.abs(A) @ np.abs(Xc))).all()
    lam = pca.singular_values_.numpy() ** 2
    assert (np.diff(lam) <= 0).all() and np.abs(pca.explained_variance_.numpy() - lam / (n - 1)).max() <= 1e-15 * lam[0]


# ------------------------------------------------------------------ 3: bit contracts
def low_level_cross(Y, X, mu, ws_bytes=None):
    """rbnn_wpca_cross_gram on whole matrices with a workspace of ws_bytes (default: one round) -> float64 [m, n] on the GPU."""
    lib = _hip.load()
    m, n, P = Y.shape[0], X.shape[0], X.shape[1]
    lo, hi = C.c_size_t(0), C.c_size_t(0)
    _hip.check(lib.rbnn_wpca_workspace_query(m, n, P, C.byref(lo), C.byref(hi)), "query")
    ws_bytes = hi.value if ws_bytes is None else max(lo.value, ws_bytes)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=DEV)
    out = torch.zeros(m, n, dtype=torch.float64, device=DEV)
    _hip.check(lib.rbnn_wpca_cross_gram(Y.data_ptr(), Y.stride(0), m, X.data_ptr(), X.stride(0), n, mu.data_ptr(), P, out.data_ptr(), n,
                                        ws.data_ptr(), ws_bytes, _hip.stream_of(X)), "rbnn_wpca_cross_gram")
    return out


def test_bit_contracts_runs_symmetry_rounds_and_row_subsets():
    n, P = 50, 3 * CH + 5
    X = dev(R.planted(n, P))
    a = fit(X)
    b = fit(X)
    assert torch.equal(a.gram_, b.gram_) and torch.equal(a.scores_, b.scores_) and torch.equal(a.mean_, b.mean_)
    assert torch.equal(a.components(), b.components())
    assert torch.equal(a.gram_, a.gram_.t())
    # a budget of one chunk per slab: four slabs, four rounds
    plan = W().slab_plan(P, 1, W().tiles(n, n), 0)
    assert len(plan) == 4
    c = fit(X, ws_bytes=1)
    assert torch.equal(a.gram_, c.gram_) and torch.equal(a.scores_, c.scores_) and torch.equal(a.mean_, c.mean_)
    assert torch.equal(a.components(), c.components())
    Y = dev(R.fresh_rows(X.cpu().numpy(), 5))
    assert torch.equal(a.transform(W().MatrixRows(Y)), c.transform(W().MatrixRows(Y)))
    # the rounds inside one call: a workspace of one chunk, of two, of all four
    full = low_level_cross(X, X, a.mean_)
    assert torch.equal(full, a.gram_)
    for chunks in (1, 2):
        assert torch.equal(low_level_cross(X, X, a.mean_, ws_bytes=chunks * W().tiles(n, n) * 2048), full)
    # C[i, j] is a function of row i, row j, the mean and P: any rows against any rows, across tile borders, sizes no multiples of 16
    ia = torch.tensor([0, 15, 16, 17, 31, 32, 49, 3, 40], device=DEV)             # 9 rows
    ib = torch.tensor(list(range(14, 35)) + [49, 0], device=DEV)                   # 23 rows
    sub = low_level_cross(X[ia].contiguous(), X[ib].contiguous(), a.mean_)
    assert torch.equal(sub, a.gram_[ia][:, ib])
    one = low_level_cross(X[7:8], X[48:49], a.mean_)                               # m = n = 1
    assert torch.equal(one, a.gram_[7:8, 48:49])
    # through the public interface too: cross_gram of a subset of the fitted rows
    assert torch.equal(a.cross_gram(W().MatrixRows(X[ia].contiguous())), a.gram_[ia])


# ------------------------------------------------------------------ 4: layout
def test_row_stride_and_base_offset_change_no_bit_and_no_canary():
    n, P, m = 17, CH + 7, 5
    Xh = R.planted(n, P)
    Yh = R.fresh_rows(Xh, m)
    ref = fit(Xh)
    ref_T, ref_V = ref.transform(W().MatrixRows(dev(Yh))), ref.components()

    def strided(A):
        """A in a buffer with row stride P + 3, starting one float behind the (aligned) base: NaN everywhere else."""
        buf = torch.full((A.shape[0] * (P + 3) + 1,), float("nan"), dtype=torch.float32, device=DEV)
        view = buf[1:].view(A.shape[0], P + 3)[:, :P]
        view.copy_(dev(A))
        assert view.data_ptr() % 16 == 4 and view.stride(0) == P + 3
        return buf, view

    bx, vx = strided(Xh)
    by, vy = strided(Yh)
    pca = fit(vx)
    assert torch.equal(pca.gram_, ref.gram_) and torch.equal(pca.mean_, ref.mean_) and torch.equal(pca.scores_, ref.scores_)
    assert torch.equal(pca.transform(W().MatrixRows(vy)), ref_T)
    assert torch.equal(pca.components(), ref_V)
    # the gaps still hold their NaNs (and the NaNs reached no result)
    for buf, A in ((bx, Xh), (by, Yh)):
        gaps = torch.ones_like(buf, dtype=torch.bool)
        gaps[1:].view(A.shape[0], P + 3)[:, :P] = False
        assert bool(torch.isnan(buf[gaps]).all()) and int(gaps.sum()) == 3 * A.shape[0] + 1
    assert bool(torch.isfinite(pca.gram_).all()) and bool(torch.isfinite(pca.components()).all())
    # canaries behind the output buffers of the raw calls: C [m, ldc > n], mu, V [k, ldv > P], generated rows [n, ld > w]
    lib, st = _hip.load(), _hip.stream_of(vx)
    nan64 = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=DEV)
    X = dev(Xh)
    mu = nan64(P + 8)
    _hip.check(lib.rbnn_wpca_col_mean(X.data_ptr(), P, n, P, mu.data_ptr(), st), "col_mean")
    assert torch.equal(mu[:P], ref.mean_) and bool(torch.isnan(mu[P:]).all())
    Cm = nan64(m + 1, n + 3)
    Cm[:m, :n] = 0
    ws = torch.empty(2 * W().tiles(m, n) * 256, dtype=torch.float64, device=DEV)
    Y = dev(Yh)
    _hip.check(lib.rbnn_wpca_cross_gram(Y.data_ptr(), P, m, X.data_ptr(), P, n, ref.mean_.data_ptr(), P, Cm.data_ptr(), n + 3, ws.data_ptr(),
                                        ws.numel() * 8, st), "cross_gram")
    assert torch.equal(Cm[:m, :n], ref.cross_gram(W().MatrixRows(Y)))
    assert bool(torch.isnan(Cm[:m, n:]).all()) and bool(torch.isnan(Cm[m:]).all())
    V = nan64(3, P + 5)
    A = (ref.u_ / ref.singular_values_).t().contiguous().to(DEV)
    _hip.check(lib.rbnn_wpca_components(A.data_ptr(), 2, X.data_ptr(), P, n, ref.mean_.data_ptr(), P, V.data_ptr(), P + 5, st), "components")
    assert torch.equal(V[:2, :P], ref_V) and bool(torch.isnan(V[:2, P:]).all()) and bool(torch.isnan(V[2]).all())
    rows = torch.full((4, 14), float("nan"), dtype=torch.float32, device=DEV)
    _hip.check(lib.rbnn_wpca_normal_rows(C.c_uint64(KEY), 2, 3, 8, 10, rows.data_ptr(), 14, st), "normal_rows")
    assert bool(torch.isfinite(rows[:3, :10]).all()) and bool(torch.isnan(rows[:3, 10:]).all()) and bool(torch.isnan(rows[3]).all())
    assert torch.equal(rows[:3, :10], W().PriorRows(KEY, 5, 18, DEV).materialize()[2:5, 8:18])


# ------------------------------------------------------------------ 5: the generator
def test_prior_rows_match_the_oracle_and_depend_on_key_row_and_column_only():
    from oracle import bnn_oracle as O
    n, P = 8, 1031
    prior = W().PriorRows(KEY, n, P, DEV)
    rows = prior.materialize()
    for r in range(n):
        eps = torch.from_numpy(O.philox_normals(KEY, 0, 0x57504341, r, 1, P)[0])
        err = ((rows[r].cpu().double() - eps).abs() / (1 + eps.abs())).max()
        assert float(err) <= 2e-5, (r, float(err))                      # the bar tests/test_hip_svi.py holds the SVI draw to
    assert torch.equal(prior.materialize(rows=[5, 7]), rows[[5, 7]])
    assert torch.equal(W().PriorRows(KEY, 3, P, DEV).materialize(), rows[:3])          # not on n
    assert torch.equal(prior.materialize(P=517), rows[:, :517])                        # not on the width
    assert torch.equal(W().PriorRows(KEY, n, 517, DEV).materialize(), rows[:, :517])
    buf = torch.empty(n, 64, dtype=torch.float32, device=DEV)                          # a slab in the middle
    prior.draw(0, n, 512, 61, buf)
    assert torch.equal(buf[:, :61], rows[:, 512:573])
    assert not torch.equal(W().PriorRows(KEY + 1, n, P, DEV).materialize(), rows)


def test_prior_rows_have_the_moments_of_a_standard_normal():
    """Deterministic for its key: |mean| <= 6 / sqrt(nP), |var - 1| <= 6 sqrt(2 / (nP)), every row correlation <= 6 / sqrt(P)."""
    n, P = 64, 65536
    Z = W().PriorRows(KEY, n, P, DEV).materialize().double()
    mean, var = float(Z.mean()), float(Z.var())
    corr = torch.corrcoef(Z)
    off = float((corr - torch.eye(n, dtype=torch.float64, device=Z.device)).abs().max())
    print(f"[wpca prior] mean {mean:.3e} (bound {6 / (n * P) ** 0.5:.3e}), var - 1 {var - 1:.3e} (bound {6 * (2 / (n * P)) ** 0.5:.3e}), "
          f"largest row correlation {off:.3e} (bound {6 / P ** 0.5:.3e})")
    assert abs(mean) <= 6 / (n * P) ** 0.5 and abs(var - 1) <= 6 * (2 / (n * P)) ** 0.5 and off <= 6 / P ** 0.5


# ------------------------------------------------------------------ 6: the two row sources
@pytest.mark.parametrize("budget", ["one slab", "default"])
def test_prior_rows_fit_like_their_materialised_matrix(budget):
    n, P = 40, 4099
    prior = W().PriorRows(KEY, n, P, DEV)
    kw = {}
    if budget == "one slab":                                            # one chunk per slab: three slabs
        kw = {"ws_bytes": 1}
        assert len(W().slab_plan(P, 1, W().tiles(n, n), n)) == 3
    a = W().WeightPCA(2, device=DEV, **kw).fit(prior)
    b = W().WeightPCA(2, device=DEV).fit(W().MatrixRows(prior.materialize()))
    assert torch.equal(a.gram_, b.gram_) and torch.equal(a.scores_, b.scores_) and torch.equal(a.mean_, b.mean_)
    assert torch.equal(a.components(), b.components())
    Y = W().PriorRows(KEY ^ 0xABCDEF, 7, P, DEV)
    assert torch.equal(a.transform(Y), b.transform(W().MatrixRows(Y.materialize())))


# ------------------------------------------------------------------ 7: the drivers
def planted_stacks(arch, D, H, Cn, S, scales):
    """One planted [S, P] matrix per scale, cut into the tensors of the architecture in parameters() order -> ([stacked dict], [matrix]).
    Every set has the planted spectrum on its own (R does not see a scale); the scales 1 : 0.4 : 0.15 keep the concatenation's
    eigenvalues 9, 4 (set 0), 4 * 0.16 (set 1), ... apart, so the one fit of same_pca is as well conditioned."""
    from oracle import bnn_oracle as O
    shapes = O.param_shapes(arch, D, H, Cn)
    P = sum(int(np.prod(s)) for _, s in shapes)
    stacks, mats = [], []
    for seed, scale in enumerate(scales):
        X = R.planted(S, P, seed=seed + 1) * np.float32(scale)
        off, st = 0, {}
        for k, s in shapes:
            m = int(np.prod(s))
            st[k] = torch.from_numpy(X[:, off:off + m].reshape((S,) + tuple(s)).copy())
            off += m
        stacks.append(st)
        mats.append(X)
    return stacks, mats


def make_bnn(arch, H, stack, shape=(1, 28, 28), Cn=10):
    from robustbnns_amd.model_bnn import BNN
    S = next(iter(stack.values())).shape[0]
    bnn = BNN("mnist", H, "leaky", arch, "hmc", None, None, S, 0, shape, Cn)
    bnn.set_posterior_samples(stack, DEV)
    return bnn


@pytest.fixture(scope="module")
def three_nets():
    S, H = 6, 32
    stacks, mats = planted_stacks("fc2", 784, H, 10, S, scales=(1.0, 0.4, 0.15))
    nets = {n_inputs: make_bnn("fc2", H, st) for n_inputs, st in zip((1000, 10000, 60000), stacks)}
    return nets, mats, S


@pytest.mark.parametrize("same_pca", [False, True])
def test_build_pca_df_is_the_reference_frame(three_nets, same_pca):
    from robustbnns_amd import multimodal
    nets, mats, S = three_nets
    P, n_prior = mats[0].shape[1], 24
    df = multimodal.build_pca_df(nets, S, same_pca=same_pca, key=KEY, n_prior=n_prior)
    assert list(df.columns) == ["n_samples", "n_training_points", "x", "y"] and len(df) == n_prior + 3 * S
    assert df["n_training_points"].tolist() == [0] * n_prior + [1000] * S + [10000] * S + [60000] * S
    assert df["n_samples"].tolist() == [n_prior] * n_prior + [S] * (3 * S)
    xy = df[["x", "y"]].to_numpy()
    prior = W().PriorRows(KEY, n_prior, P, DEV).materialize().cpu().numpy()
    if same_pca:
        ref = R.Restated(np.concatenate(mats))
        ref.ratios("build_pca_df same_pca, prior", transform=(xy[:n_prior], prior))
        for i, X in enumerate(mats):
            ref.ratios(f"build_pca_df same_pca, net {i}", transform=(xy[n_prior + i * S:n_prior + (i + 1) * S], X))
    else:
        # the prior fitted on itself is no planted input: its spectrum is flat, R is what it is, and B carries it
        R.Restated(prior).ratios("build_pca_df separate, prior", scores=xy[:n_prior], planted=False)
        for i, X in enumerate(mats):
            R.Restated(X).ratios(f"build_pca_df separate, net {i}", scores=xy[n_prior + i * S:n_prior + (i + 1) * S])


@pytest.mark.parametrize("arch,H,shape", [("fc", 32, (1, 28, 28)), ("fc2", 32, (1, 28, 28)), ("conv", 16, (1, 28, 28))])
def test_posterior_weights_are_the_flattened_parameters(arch, H, shape):
    from oracle import bnn_oracle as O
    from robustbnns_amd import multimodal
    S = 3
    bnn = make_bnn(arch, H, O.synthetic_posterior(arch, 784, H, 10, S, 0.05), shape)
    Wt = multimodal.posterior_weights(bnn)
    assert Wt.dtype == torch.float32 and Wt.device.type == "cuda" and Wt.is_contiguous()
    pp = bnn.posterior_predictive
    want = torch.stack([torch.cat([p.detach().flatten() for p in pp[i].parameters()]) for i in range(S)])
    assert tuple(Wt.shape) == tuple(want.shape) and torch.equal(Wt.cpu(), want.cpu())


def test_chains_pca_separates_two_planted_chains():
    from oracle import bnn_oracle as O
    from robustbnns_amd import multimodal
    H, draws = 32, 5
    shapes = O.param_shapes("fc2", 784, H, 10)
    g = torch.Generator().manual_seed(3)
    centre = {k: torch.randn(s, generator=g) for k, s in shapes}
    stack = {k: torch.cat([sgn * centre[k].unsqueeze(0) + 0.01 * torch.randn((draws,) + tuple(s), generator=g) for sgn in (1.0, -1.0)]).to(DEV)
             for k, s in shapes}
    bnn = make_bnn("fc2", H, {k: v[:4].cpu() for k, v in stack.items()})
    bnn.hmc_history = {"stack": stack, "chains": [{}, {}], "r_hat_U": 9.9}
    df = multimodal.chains_pca(bnn)
    assert list(df.columns) == ["chain", "draw", "x", "y"] and len(df) == 2 * draws
    assert df["chain"].tolist() == [0] * draws + [1] * draws and df["draw"].tolist() == list(range(draws)) * 2
    x = df["x"].to_numpy()
    assert (np.sign(x[:draws]) == np.sign(x[0])).all() and (np.sign(x[draws:]) == -np.sign(x[0])).all() and abs(x).min() > 1.0
    bnn.hmc_history = {"eps": []}
    with pytest.raises(ValueError, match='no "stack"'):
        multimodal.chains_pca(bnn)
