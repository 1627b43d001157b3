// rbnn_wpca.inc — weight-space PCA of posterior samples on the double-precision matrix pipe (included by rbnn_nn_train.hip, the smallest unit:
// nothing here touches a trainer).  n rows (posterior samples, or draws of the N(0, I) prior) of P weights, n << P: PCA is the n x n Gram
// matrix of the centred rows, contracted over P, and an n x n eigenproblem the host solves.  The kernels:
//   wpca_normal_rows_kernel     out[r][e] = the standard normal of Philox counter (e / 4, WPCA_TENSOR, r, 0), component e % 4: the prior's rows,
//                               a pure function of (key, r, e) — generated slab by slab, the n x P matrix never exists
//   wpca_col_mean_kernel        mu[e] = (sum_r x[r][e]) / n, fp64, r ascending
//   wpca_cross_gram_kernel      partial[chunk][i][j] = sum_{e in chunk} (y[i][e] - mu[e]) (x[j][e] - mu[e]) on v_mfma_f64_16x16x4_f64
//   wpca_chunk_sum_kernel       C[i][j] += partial[0][i][j] + partial[1][i][j] + ... in chunk order
//   wpca_components_kernel      V[k][e] = sum_i A[k][i] (x[i][e] - mu[e]), fp64, i ascending, k <= 16
//
// The Gram contraction: one wave (a block is one wave) = one 16 x 16 output tile x one chunk of RBNN_WPCA_CHUNK columns.  P is the long
// dimension and the output tiny (50 x 50 rows: 16 tiles), so the parallelism comes from the chunks.  The wave starts from zero and walks its
// chunk in blocks of 16 columns; step r of a block takes k = lg <-> column 16 g + 4 lg + r (rbnn_fp64_common.hpp's map: one 16-byte load of four
// consecutive fp32 values feeds four steps), columns past P contribute zeros.  The mean is subtracted in fp64 BEFORE the product — never
// sum y x minus a correction, which cancels for samples far from the origin.  A round is as many chunks as the caller's workspace holds; the
// second kernel adds a round's partials to the output in chunk order, one thread per element, so that the accumulator is carried from round
// to round (and from column slab to column slab, whose borders the caller keeps on chunk borders) through the output buffer, as the
// contraction of rbnn_fc_wgrad_dp.inc carries its own from point block to point block.  Nothing is atomic.  C[i][j] is
// (((0 + p_0) + p_1) + ...) over ALL chunks of the P columns whatever the rounds: its bits are a function of row i of Y, row j of X, mu and P
// alone — not of m, n, the other rows (rows past the last repeat the last one and are never stored), the workspace or the slabs.  The MFMA's
// product is symmetric in its operands, so a Gram matrix of X against X equals its transpose bit for bit.
//
// Loads: rows have their own strides and the base pointers need 4-byte alignment only.  The 16-byte loads are chosen per call (both bases
// 16-byte aligned, both strides multiples of 4) and fall back to four scalar loads otherwise; the last, ragged group of four columns is always
// read scalar, so nothing past column P of a row is touched.  Both paths widen the same fp32 values: same bits.

#include "rbnn_fp64_common.hpp"
#include <algorithm>

#define WPCA_CHUNK RBNN_WPCA_CHUNK
static_assert(WPCA_CHUNK % 16 == 0, "a chunk is whole 16-column blocks");

namespace {

constexpr int WPCA_ELT_THREADS = 256;

// ---------------------------------------------------------------------------------------------------
// The prior's rows: thread = (row, quad of columns).  grid.x over the quads of the slab, grid.y = row.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WPCA_ELT_THREADS) wpca_normal_rows_kernel(uint32_t k0, uint32_t k1, int r0, long long e0, long long w,
                                                                             float* __restrict__ out, long long ld) {
    const long long q = (long long)blockIdx.x * WPCA_ELT_THREADS + threadIdx.x;              // quad within the slab
    if (4 * q >= w) return;
    const int r = r0 + (int)blockIdx.y;
    const Rng rng = {k0, k1, (uint32_t)r, 0u};
    float nrm[4];
    rng.quad(RBNN_WPCA_TENSOR, (uint32_t)(e0 / 4 + q), nrm);
    float* const o = out + (long long)blockIdx.y * ld + 4 * q;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (4 * q + j < w) o[j] = nrm[j];
}

// ---------------------------------------------------------------------------------------------------
// Column means: thread = column.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WPCA_ELT_THREADS) wpca_col_mean_kernel(const float* __restrict__ X, long long ldx, int n, long long P,
                                                                          double* __restrict__ mu) {
    const long long e = (long long)blockIdx.x * WPCA_ELT_THREADS + threadIdx.x;
    if (e >= P) return;
    double s = 0.;
    for (int r = 0; r < n; ++r) s += (double)X[(long long)r * ldx + e];
    mu[e] = s / (double)n;
}

// four consecutive columns of a row from column e on, centred in fp64; columns >= P are zeros
template <bool VEC>
__device__ __forceinline__ f64x4 wpca_centred4(const float* __restrict__ row, const double* __restrict__ mu, long long e, long long P) {
    f64x4 v = {0., 0., 0., 0.};
    if (VEC && e + 4 <= P) {
        v = load4_f64(row + e);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] -= mu[e + j];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (e + j < P) v[j] = (double)row[e + j] - mu[e + j];
    }
    return v;
}

struct WpcaGramArgs {
    const float* Y;  long long ldy;  int m;
    const float* X;  long long ldx;  int n;
    const double* mu;
    long long P;                         // columns of this call
    long long c0;                        // first chunk of this round
    double* part;                        // [chunks of the round][tiles][4][64]
};

// ---------------------------------------------------------------------------------------------------
// One chunk's partial of one tile: D[i = row of Y][j = row of X].  grid.x = tile (mt * NT + nt), grid.y = chunk of the round.
// ---------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(64) wpca_cross_gram_kernel(const WpcaGramArgs a) {
    const int lane = threadIdx.x, li = lane & 15, lg = lane >> 4;
    const int NT = (a.n + 15) / 16;
    const int mt = (int)(blockIdx.x / NT), nt = (int)(blockIdx.x - (unsigned)mt * NT);
    // rows past m / n repeat the last one; never stored
    const float* const yrow = a.Y + (long long)min(mt * 16 + li, a.m - 1) * a.ldy;
    const float* const xrow = a.X + (long long)min(nt * 16 + li, a.n - 1) * a.ldx;
    const long long lo = (a.c0 + blockIdx.y) * WPCA_CHUNK, hi = min(lo + WPCA_CHUNK, a.P);
    f64x4 acc[1] = {{0., 0., 0., 0.}};
    for (long long e0 = lo; e0 < hi; e0 += 16) {
        const long long e = e0 + 4 * lg;
        const f64x4 yv = wpca_centred4<VEC>(yrow, a.mu, e, a.P);
        const f64x4 xv = wpca_centred4<VEC>(xrow, a.mu, e, a.P);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[0] = MFMA64(yv[r], xv[r], acc[0]);
    }
    mfma64_drain(acc);
    // acc[r] = D[i = lg + 4 r][j = li], stored lane-major: the second pass knows the map
    double* const p = a.part + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 256;
#pragma unroll
    for (int r = 0; r < 4; ++r) p[r * 64 + lane] = acc[0][r];
}

// ---------------------------------------------------------------------------------------------------
// C[i][j] += the round's partials in chunk order: thread = output element.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WPCA_ELT_THREADS) wpca_chunk_sum_kernel(const double* __restrict__ part, int chunks, int m, int n,
                                                                           double* __restrict__ C, long long ldc) {
    const long long id = (long long)blockIdx.x * WPCA_ELT_THREADS + threadIdx.x;
    if (id >= (long long)m * n) return;
    const int i = (int)(id / n), j = (int)(id - (long long)i * n);
    const int NT = (n + 15) / 16, tiles = ((m + 15) / 16) * NT;
    const int ii = i & 15, r = ii >> 2, lg = ii & 3;                       // i = lg + 4 r within the tile
    const double* const p = part + ((long long)(i >> 4) * NT + (j >> 4)) * 256 + r * 64 + lg * 16 + (j & 15);
    double acc = C[(long long)i * ldc + j];
    for (int c = 0; c < chunks; ++c) acc += p[(long long)c * tiles * 256];
    C[(long long)i * ldc + j] = acc;
}

// ---------------------------------------------------------------------------------------------------
// The principal axes: thread = column; A [K][n] is read wave-uniformly.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WPCA_ELT_THREADS) wpca_components_kernel(const double* __restrict__ A, int K, const float* __restrict__ X,
                                                                            long long ldx, int n, const double* __restrict__ mu, long long P,
                                                                            double* __restrict__ V, long long ldv) {
    const long long e = (long long)blockIdx.x * WPCA_ELT_THREADS + threadIdx.x;
    if (e >= P) return;
    const double m = mu[e];
    double acc[RBNN_WPCA_MAX_COMPONENTS];
#pragma unroll
    for (int k = 0; k < RBNN_WPCA_MAX_COMPONENTS; ++k) acc[k] = 0.;
    for (int i = 0; i < n; ++i) {
        const double d = (double)X[(long long)i * ldx + e] - m;
#pragma unroll
        for (int k = 0; k < RBNN_WPCA_MAX_COMPONENTS; ++k)
            if (k < K) acc[k] = fma(A[(long long)k * n + i], d, acc[k]);
    }
#pragma unroll
    for (int k = 0; k < RBNN_WPCA_MAX_COMPONENTS; ++k)
        if (k < K) V[(long long)k * ldv + e] = acc[k];
}

// ---- host ----
constexpr long long WPCA_MAX_GRID = 0x7fffffffLL;
inline long long wpca_blocks(long long items) { return (items + WPCA_ELT_THREADS - 1) / WPCA_ELT_THREADS; }
inline long long wpca_tiles(int m, int n) { return (long long)((m + 15) / 16) * ((n + 15) / 16); }
inline long long wpca_chunks(long long P) { return (P + WPCA_CHUNK - 1) / WPCA_CHUNK; }
// rows x stride must stay addressable: the kernels index with 64-bit offsets, the product itself may not overflow
inline bool wpca_rows_ok(int rows, long long ld, long long P) {
    return rows >= 1 && P >= 1 && ld >= P && ld <= (long long)(0x7fffffffffffffffLL / 8) / rows;
}

}  // namespace

// ===================================================================================================
// C-ABI of the weight-space PCA
// ===================================================================================================
extern "C" {

int rbnn_wpca_workspace_query(int32_t m, int32_t n, int64_t P, size_t* min_bytes, size_t* full_bytes) {
    if (!min_bytes || !full_bytes) return RBNN_ERR_NULL;
    if (m < 1 || n < 1 || P < 1) return RBNN_ERR_SHAPE;
    const long long tiles = wpca_tiles(m, n), chunks = wpca_chunks(P);
    if (tiles > WPCA_MAX_GRID || chunks > (long long)(0x7fffffffffffffffLL / 2048) / tiles) return RBNN_ERR_SHAPE;
    *min_bytes = (size_t)tiles * 256 * sizeof(double);
    *full_bytes = (size_t)chunks * *min_bytes;
    return RBNN_OK;
}

int rbnn_wpca_normal_rows(uint64_t key, int32_t r0, int32_t n, int64_t e0, int64_t w, float* out, int64_t ld, void* stream) {
    if (!out) return RBNN_ERR_NULL;
    if (r0 < 0 || n < 1 || n > 65535 || (long long)r0 + n > 0x7fffffffLL || e0 < 0 || (e0 & 3) || w < 1 || !wpca_rows_ok(n, ld, w))
        return RBNN_ERR_SHAPE;
    if (w > (1LL << 34) || e0 > (1LL << 34) - w) return RBNN_ERR_SHAPE;              // the quad index is a 32-bit counter word
    const long long blocks = wpca_blocks((w + 3) / 4);
    if (blocks > WPCA_MAX_GRID) return RBNN_ERR_SHAPE;
    hipLaunchKernelGGL(wpca_normal_rows_kernel, dim3((unsigned)blocks, (unsigned)n), dim3(WPCA_ELT_THREADS), 0, (hipStream_t)stream,
                       (uint32_t)key, (uint32_t)(key >> 32), r0, (long long)e0, (long long)w, out, (long long)ld);
    return launch_status();
}

int rbnn_wpca_col_mean(const float* X, int64_t ldx, int32_t n, int64_t P, double* mu, void* stream) {
    if (!X || !mu) return RBNN_ERR_NULL;
    if (n < 1 || P < 1 || !wpca_rows_ok(n, ldx, P) || wpca_blocks(P) > WPCA_MAX_GRID) return RBNN_ERR_SHAPE;
    hipLaunchKernelGGL(wpca_col_mean_kernel, dim3((unsigned)wpca_blocks(P)), dim3(WPCA_ELT_THREADS), 0, (hipStream_t)stream, X,
                       (long long)ldx, n, (long long)P, mu);
    return launch_status();
}

int rbnn_wpca_cross_gram(const float* Y, int64_t ldy, int32_t m, const float* X, int64_t ldx, int32_t n, const double* mu, int64_t P,
                         double* C, int64_t ldc, double* ws, size_t ws_bytes, void* stream) {
    if (!Y || !X || !mu || !C || !ws) return RBNN_ERR_NULL;
    if (m < 1 || n < 1 || P < 1 || !wpca_rows_ok(m, ldy, P) || !wpca_rows_ok(n, ldx, P) || !wpca_rows_ok(m, ldc, n)) return RBNN_ERR_SHAPE;
    size_t min_bytes = 0, full_bytes = 0;
    const int rc = rbnn_wpca_workspace_query(m, n, P, &min_bytes, &full_bytes);
    if (rc) return rc;
    if (ws_bytes < min_bytes) return RBNN_ERR_SHAPE;
    const long long tiles = wpca_tiles(m, n), chunks = wpca_chunks(P);
    const long long per_round = std::min<long long>(std::min<long long>((long long)(ws_bytes / min_bytes), chunks), 65535);
    const bool vec = aligned16(Y) && aligned16(X) && !(ldy & 3) && !(ldx & 3);
    hipStream_t st = (hipStream_t)stream;
    WpcaGramArgs a = {Y, (long long)ldy, m, X, (long long)ldx, n, mu, (long long)P, 0, ws};
    for (long long c0 = 0; c0 < chunks; c0 += per_round) {
        const int nc = (int)std::min(per_round, chunks - c0);
        a.c0 = c0;
        const dim3 grid((unsigned)tiles, (unsigned)nc);
        if (vec) hipLaunchKernelGGL(wpca_cross_gram_kernel<true>, grid, dim3(64), 0, st, a);
        else     hipLaunchKernelGGL(wpca_cross_gram_kernel<false>, grid, dim3(64), 0, st, a);
        if (launch_status()) return RBNN_ERR_LAUNCH;
        hipLaunchKernelGGL(wpca_chunk_sum_kernel, dim3((unsigned)wpca_blocks((long long)m * n)), dim3(WPCA_ELT_THREADS), 0, st, ws, nc, m, n, C,
                           (long long)ldc);
        if (launch_status()) return RBNN_ERR_LAUNCH;
    }
    return RBNN_OK;
}

int rbnn_wpca_components(const double* A, int32_t k, const float* X, int64_t ldx, int32_t n, const double* mu, int64_t P, double* V,
                         int64_t ldv, void* stream) {
    if (!A || !X || !mu || !V) return RBNN_ERR_NULL;
    if (k < 1 || k > RBNN_WPCA_MAX_COMPONENTS || n < 1 || P < 1 || !wpca_rows_ok(n, ldx, P) || !wpca_rows_ok(k, ldv, P)
        || wpca_blocks(P) > WPCA_MAX_GRID)
        return RBNN_ERR_SHAPE;
    hipLaunchKernelGGL(wpca_components_kernel, dim3((unsigned)wpca_blocks(P)), dim3(WPCA_ELT_THREADS), 0, (hipStream_t)stream, A, k, X,
                       (long long)ldx, n, mu, (long long)P, V, (long long)ldv);
    return launch_status();
}

}  // extern "C"
