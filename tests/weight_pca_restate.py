"""The comparator and the inputs of the weight-space PCA tests (tests/test_hip_weight_pca.py): PCA restated in float64 with numpy's SVD,
planted inputs whose spectrum is known, and the bar the two are held to.

The bar is derived, not chosen.  The fp64 contraction of the Gram matrix G over P columns perturbs G[i, j] by at most P 2^-53 |y_i| |x_j|;
Davis-Kahan gives the eigenvectors an error of at most |dG| / gap; so with R = trace(G) / min(lambda1 - lambda2, lambda2 - lambda3) the
scores agree within B = 2 (P + n) 2^-53 R sqrt(lambda1) and the unit-norm components within B / sqrt(lambda1).  The tests allow 8 B: the
margin covers eigh's and the SVD's own n 2^-53 terms.  R is taken from the restatement's spectrum and asserted <= 8 before anything is
compared: a case whose directions its own rounding decides proves nothing."""
import numpy as np

R_MAX = 8.0
MARGIN = 8.0


def flip(U, Vt):
    """sklearn's u-based svd_flip at the time of the reference: the entry of largest magnitude of every column of U is positive."""
    idx = np.abs(U).argmax(0)
    s = np.sign(U[idx, np.arange(U.shape[1])])
    s[s == 0] = 1.0
    return U * s, Vt * s[:, None]


class Restated:
    """PCA of the fp32 rows X32 [n, P], widened to float64: mean, scores = U S, components = V^T, lam = S^2 (all of them), R and the bar B."""

    def __init__(self, X32, k=2):
        X = np.asarray(X32, dtype=np.float32).astype(np.float64)
        self.n, self.P, self.k = X.shape[0], X.shape[1], k
        self.mean = X.mean(0)
        U, S, Vt = np.linalg.svd(X - self.mean, full_matrices=False)
        U, Vt = flip(U, Vt)
        self.scores, self.components, self.singular_values = U[:, :k] * S[:k], Vt[:k], S[:k]
        lam = np.concatenate([S ** 2, np.zeros(3)])
        self.lam = lam
        self.R = float(lam.sum() / min(lam[0] - lam[1], lam[1] - lam[2]))
        self.B = 2.0 * (self.P + self.n) * 2.0 ** -53 * self.R * float(np.sqrt(lam[0]))

    def transform(self, Y32):
        return (np.asarray(Y32, dtype=np.float32).astype(np.float64) - self.mean) @ self.components.T

    def assert_conditioned(self):
        assert self.R <= R_MAX, f"the restatement's own spectrum gives R = {self.R:.2f} > {R_MAX}: the case decides nothing"

    def ratios(self, what, scores=None, transform=None, components=None, planted=True):
        """Each given result against its restatement (transform = (values, Y32)): prints the measured error in units of B (components: of
        B / sqrt(lambda1)) and asserts it within the margin.  A transformed row y is (y - mean) . v: an axis error of B / sqrt(lambda1)
        moves it by |y - mean| B / sqrt(lambda1), so a row further from the mean than sqrt(lambda1) — a prior draw against a posterior's
        axes — is held to B scaled by that factor, every other row to B itself.  planted=False: rows that are not the planted inputs (the
        prior fitted on itself): the same bar from their own R, whatever it is.  -> {name: ratio}"""
        if planted:
            self.assert_conditioned()
        out = {}
        if scores is not None:
            out["scores"] = float(np.abs(np.asarray(scores) - self.scores).max() / self.B)
        if transform is not None:
            Y = np.asarray(transform[1], dtype=np.float32).astype(np.float64)
            far = np.maximum(1.0, np.linalg.norm(Y - self.mean, axis=1) / np.sqrt(self.lam[0]))
            out["transform"] = float((np.abs(np.asarray(transform[0]) - self.transform(transform[1])).max(1) / (self.B * far)).max())
        if components is not None:
            out["components"] = float(np.abs(np.asarray(components) - self.components).max() / (self.B / np.sqrt(self.lam[0])))
        print(f"[wpca parity] {what} n={self.n} P={self.P}: R = {self.R:.2f}, B = {self.B:.3e}, error / B: "
              + ", ".join(f"{k} {v:.2e}" for k, v in out.items()))
        for k, v in out.items():
            assert v <= MARGIN, f"{what}: {k} is {v:.2f} x B from the restatement (allowed {MARGIN})"
        return out


def _orthonormal(rng, rows, cols, centred=False):
    """[rows, cols] with orthonormal columns (and zero column sums)."""
    A = rng.standard_normal((rows, cols))
    if centred:
        A -= A.mean(0)
    Q, _ = np.linalg.qr(A)
    return Q


def planted(n, P, offset=0.0, seed=0):
    """fp32 [n, P]: X = offset[None, :] + sqrt(n) (3 a1 b1^T + 2 a2 b2^T) + noise, a orthonormal and centred, b orthonormal, the noise
    N(0, 1 / P) per entry: lambda1 ~ 9 n, lambda2 ~ 4 n, the noise adds ~ n to the trace, R ~ 14 / 4."""
    rng = np.random.default_rng(1000 * seed + 7 * n + P)
    a, b = _orthonormal(rng, n, 2, centred=True), _orthonormal(rng, P, min(2, P))
    X = np.sqrt(n) * (3.0 * np.outer(a[:, 0], b[:, 0]) + 2.0 * np.outer(a[:, 1], b[:, 1]))
    X += rng.standard_normal((n, P)) / np.sqrt(P)
    return (X + offset * np.ones(P)[None, :]).astype(np.float32)


def fresh_rows(X32, m=5, seed=1):
    """m fp32 rows to transform: midpoints of pairs of rows of X plus noise of the planted size — no further from the mean than X's own."""
    rng = np.random.default_rng(seed)
    X = np.asarray(X32, dtype=np.float64)
    i, j = rng.integers(0, X.shape[0], m), rng.integers(0, X.shape[0], m)
    return (0.5 * (X[i] + X[j]) + rng.standard_normal((m, X.shape[1])) / np.sqrt(X.shape[1])).astype(np.float32)
