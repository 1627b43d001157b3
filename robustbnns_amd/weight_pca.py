"""PCA of weight vectors on the GPU (csrc/rbnn_wpca.inc): the projection half of the reference's test_multimodal.py, which flattens every
posterior sample into one vector of P weights and projects the samples — and 1000 draws of the N(0, I) prior — onto two principal
components with sklearn.decomposition.PCA on the host.

With n rows and P columns, n << P, PCA is the n x n Gram matrix G = Xc Xc^T of the centred rows and its eigenproblem: G = U diag(lambda) U^T,
scores = U sqrt(lambda), principal axes = Xc^T U / sqrt(lambda).  The contraction over P runs in double precision on the fp64 matrix pipe, the
mean subtracted before the product; the n x n eigenproblem runs on the host (torch.linalg.eigh, float64).  Rows come from a row source:
MatrixRows (a resident fp32 matrix) or PriorRows (the prior's rows, a pure function of a Philox key, generated slab by slab and never stored).
The driver sweeps P in column slabs cut from a byte budget (slab_plan); slab borders are chunk borders, so the budget changes no bit."""
import ctypes as C

import torch

from . import _hip
from .flat_params import require_gpu_fc

CHUNK = _hip.WPCA_CHUNK                      # columns of one partial sum: slab borders are multiples of it
MAX_COMPONENTS = _hip.WPCA_MAX_COMPONENTS    # rbnn_wpca_components' limit
DEFAULT_WS_BYTES = 256 << 20
_ROWS_PER_DRAW = 65535                       # rbnn_wpca_normal_rows: rows per launch


def tiles(m, n):
    return ((m + 15) // 16) * ((n + 15) // 16)


def chunk_bytes(n_tiles, generated_rows):
    """Bytes one chunk of columns takes in a sweep: the partial sums of every output tile (256 doubles each) and CHUNK fp32 columns of every
    generated row."""
    return n_tiles * 256 * 8 + generated_rows * CHUNK * 4


def slab_plan(P, ws_bytes, n_tiles=0, generated_rows=0):
    """[(e0, w)]: the column slabs of a sweep over P columns.  Every slab but the last is the same whole number of chunks — as many as the
    budget holds, at least one —, the last takes what is left; a sweep that needs no buffer per column is one slab."""
    per = chunk_bytes(n_tiles, generated_rows)
    n_chunks = (P + CHUNK - 1) // CHUNK
    per_slab = n_chunks if per == 0 else max(1, min(n_chunks, int(ws_bytes) // per))
    w = per_slab * CHUNK
    return [(e0, min(w, P - e0)) for e0 in range(0, P, w)]


class MatrixRows:
    """The rows of a resident fp32 matrix [n, P] with unit column stride and any row stride >= P."""

    generated_rows = 0

    def __init__(self, t):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise ValueError("MatrixRows takes a 2-D tensor [n, P]")
        if t.dtype != torch.float32:
            raise ValueError(f"MatrixRows takes float32 rows, not {t.dtype}")
        self.n, self.P = int(t.shape[0]), int(t.shape[1])
        if self.n < 1 or self.P < 1:
            raise ValueError(f"MatrixRows needs at least one row and one column, not {tuple(t.shape)}")
        if self.P > 1 and t.stride(1) != 1:
            raise ValueError(f"MatrixRows takes rows with stride(1) == 1, not {t.stride(1)}")
        if self.n > 1 and t.stride(0) < self.P:
            raise ValueError(f"MatrixRows takes a row stride >= P = {self.P}, not {t.stride(0)}")
        require_gpu_fc("Weight-space PCA", device=t.device)
        self.t, self.device = t, t.device
        self.ld = int(t.stride(0)) if self.n > 1 else self.P

    def buffer(self, w):
        return None

    def slab(self, e0, w, buf):
        """-> (address of row 0, column e0; row stride in elements)"""
        return self.t.data_ptr() + 4 * e0, self.ld


class PriorRows:
    """n rows of the N(0, I) prior over P weights: element (r, e) is component e % 4 of the standard normals of Philox counter
    (e // 4, WPCA_TENSOR, r, 0) under the 64-bit key — a function of (key, r, e) alone."""

    def __init__(self, key, n, P, device="cuda"):
        self.key, self.n, self.P = int(key) & 0xFFFFFFFFFFFFFFFF, int(n), int(P)
        if self.n < 1 or self.P < 1:
            raise ValueError(f"PriorRows needs at least one row and one column, not n = {n}, P = {P}")
        require_gpu_fc("Weight-space PCA", device=device)
        self.device = torch.device(device)
        self.generated_rows = self.n

    def buffer(self, w):
        return torch.empty(self.n, (w + 3) // 4 * 4, dtype=torch.float32, device=self.device)

    def draw(self, r0, n, e0, w, out):
        """Rows r0 .. r0 + n, columns e0 .. e0 + w (e0 % 4 == 0) into out [n, >= w]."""
        lib = _hip.load()
        for a in range(0, n, _ROWS_PER_DRAW):
            b = min(n, a + _ROWS_PER_DRAW)
            _hip.check(lib.rbnn_wpca_normal_rows(C.c_uint64(self.key), r0 + a, b - a, e0, w, out.data_ptr() + 4 * a * out.stride(0),
                                                 out.stride(0), _hip.stream_of(out)), "rbnn_wpca_normal_rows")

    def slab(self, e0, w, buf):
        self.draw(0, self.n, e0, w, buf)
        return buf.data_ptr(), int(buf.stride(0))

    def materialize(self, rows=None, P=None):
        """The rows (all, or those of the index list `rows`) of the first P columns (default: all) as an fp32 tensor: for tests and small cases."""
        P = self.P if P is None else int(P)
        if rows is None:
            out = torch.empty(self.n, P, dtype=torch.float32, device=self.device)
            self.draw(0, self.n, 0, P, out)
            return out
        rows = [int(r) for r in rows]
        out = torch.empty(len(rows), P, dtype=torch.float32, device=self.device)
        for i, r in enumerate(rows):
            self.draw(r, 1, 0, P, out[i:i + 1])
        return out


def as_rows(rows):
    return rows if isinstance(rows, (MatrixRows, PriorRows)) else MatrixRows(rows)


def flip_signs(u):
    """sklearn's u-based svd_flip at the time of the reference: the entry of largest magnitude of every column of u is positive."""
    idx = u.abs().argmax(0)
    s = torch.sign(u[idx, torch.arange(u.shape[1])])
    return u * torch.where(s == 0, torch.ones_like(s), s)


class WeightPCA:
    """fit(rows) / transform(rows) / fit_transform(rows) / components() in the manner of sklearn.decomposition.PCA.  After fit():
    scores_ [n, k] (= fit_transform), singular_values_, explained_variance_ (float64, on the host), mean_
    (float64 [P]) and gram_ (float64 [n, n]) on the GPU."""

    def __init__(self, n_components=2, device="cuda", ws_bytes=DEFAULT_WS_BYTES):
        require_gpu_fc("Weight-space PCA", device=device)
        if not 1 <= int(n_components) <= MAX_COMPONENTS:
            raise ValueError(f"WeightPCA takes 1 <= n_components <= {MAX_COMPONENTS} (the axes kernel's accumulators), not {n_components}")
        if int(ws_bytes) < 1:
            raise ValueError(f"WeightPCA needs a positive workspace budget, not {ws_bytes}")
        self.n_components, self.device, self.ws_bytes = int(n_components), torch.device(device), int(ws_bytes)
        self.rows_ = None

    # ------------------------------------------------------------------ the sweep
    def _sweep(self, Y, X, mean, out, fit):
        """out [m, n] += the cross-Gram of Y's rows (None: X's own) against X's rows, slab by slab; fit: the slab's means are written first."""
        lib = _hip.load()
        m, n, P = (X.n if Y is None else Y.n), X.n, X.P
        n_tiles = tiles(m, n)
        plan = slab_plan(P, self.ws_bytes, n_tiles, X.generated_rows + (0 if Y is None else Y.generated_rows))
        w0 = plan[0][1]
        ws = torch.empty(n_tiles * 256 * ((w0 + CHUNK - 1) // CHUNK), dtype=torch.float64, device=self.device)
        bx, by = X.buffer(w0), (None if Y is None else Y.buffer(w0))
        st = _hip.stream_of(out)
        for e0, w in plan:
            px, ldx = X.slab(e0, w, bx)
            mu = mean.data_ptr() + 8 * e0
            if fit:
                _hip.check(lib.rbnn_wpca_col_mean(px, ldx, n, w, mu, st), "rbnn_wpca_col_mean")
            py, ldy = (px, ldx) if Y is None else Y.slab(e0, w, by)
            _hip.check(lib.rbnn_wpca_cross_gram(py, ldy, m, px, ldx, n, mu, w, out.data_ptr(), out.stride(0), ws.data_ptr(),
                                                ws.numel() * 8, st), "rbnn_wpca_cross_gram")
        return out

    # ------------------------------------------------------------------ sklearn's interface
    def fit(self, rows):
        rows = as_rows(rows)
        n, P, k = rows.n, rows.P, self.n_components
        if n < 3:
            raise ValueError(f"WeightPCA needs at least 3 rows, not {n}")
        if k > min(n - 1, P):
            raise ValueError(f"n_components = {k} exceeds min(n - 1, P) = {min(n - 1, P)}")
        mean = torch.empty(P, dtype=torch.float64, device=self.device)
        G = self._sweep(None, rows, mean, torch.zeros(n, n, dtype=torch.float64, device=self.device), fit=True)
        lam, U = torch.linalg.eigh(G.cpu())
        lam, U = lam.flip(0)[:k], flip_signs(U.flip(1)[:, :k])
        if not bool(lam[-1] > 0):
            raise ValueError(f"the rows span fewer than {k} directions around their mean: eigenvalue {k} of the Gram matrix is {float(lam[-1]):.3e}")
        self.rows_, self.mean_, self.gram_, self.u_ = rows, mean, G, U
        self.singular_values_ = lam.sqrt()
        self.scores_ = U * self.singular_values_
        self.explained_variance_ = lam / (n - 1)
        return self

    def fit_transform(self, rows):
        return self.fit(rows).scores_

    def _fitted(self):
        if self.rows_ is None:
            raise ValueError("this WeightPCA is not fitted yet: call fit() first")

    def cross_gram(self, rows):
        """float64 [m, n] on the GPU: the centred rows against the fitted rows, centred with the fitted mean (the fitted source is re-swept)."""
        self._fitted()
        rows = as_rows(rows)
        if rows.P != self.rows_.P:
            raise ValueError(f"the rows have P = {rows.P} columns, the fit had {self.rows_.P}")
        return self._sweep(rows, self.rows_, self.mean_, torch.zeros(rows.n, self.rows_.n, dtype=torch.float64, device=self.device), fit=False)

    def transform(self, rows):
        """float64 [m, k] on the host: (Y - mean) V^T = cross-Gram times u / sqrt(lambda)."""
        return self.cross_gram(rows).cpu() @ (self.u_ / self.singular_values_)

    def components(self):
        """The principal axes, float64 [k, P] on the GPU (unit rows): V = (u / sqrt(lambda))^T (X - mean), computed on demand."""
        self._fitted()
        lib = _hip.load()
        X, k, P = self.rows_, self.n_components, self.rows_.P
        A = (self.u_ / self.singular_values_).t().contiguous().to(self.device)
        V = torch.empty(k, P, dtype=torch.float64, device=self.device)
        plan = slab_plan(P, self.ws_bytes, 0, X.generated_rows)
        bx = X.buffer(plan[0][1])
        st = _hip.stream_of(V)
        for e0, w in plan:
            px, ldx = X.slab(e0, w, bx)
            _hip.check(lib.rbnn_wpca_components(A.data_ptr(), k, px, ldx, X.n, self.mean_.data_ptr() + 8 * e0, w, V.data_ptr() + 8 * e0, P, st),
                       "rbnn_wpca_components")
        return V
