// rbnn_chain_diag.inc — per-weight convergence diagnostics of HMC chains (included by rbnn_nn_train.hip beside rbnn_wpca.inc: nothing here
// touches a trainer): what pyro's mcmc.diagnostics() gives per element of every sample site.  The input is the pooled stack of a
// train_hmc(num_chains=C) run as an fp32 matrix X [C * N, P], row c * N + t = draw t of chain c; every weight column is one independent
// problem.  Per column, with x widened to double precision on load (the header states the definitions in full):
//   m_c = (sum_t x[c,t]) / N,  d[c,t] = x[c,t] - m_c              the mean is subtracted BEFORE any product: a chain's draws lie close
//                                                                   together and far from the origin, E[x^2] - m^2 cancels there
//   S[c,k] = sum_{t < N-k} d[c,t] d[c,t+k],  gamma[c,k] = S[c,k] / (N - k)
//   W, V, r_hat, split_r_hat (2C half chains), rho_k, Geyer's initial monotone positive sequence, tau, n_eff, n_pairs; pooled mean and std
//
// chain_diag_columns_kernel<T, VEC>: a block is T lanes and takes T adjacent columns, lane j column e0 + j — every row read of the tile is
// one contiguous piece of the row.  Chain by chain the block stages its [N][T] tile in LDS as fp32 (16-byte loads when VEC, the ragged last
// quad of a row and every unaligned call read scalar; columns past P are zeros and are never stored), so that every input element is read
// from global memory once per call; from then on a lane reads its own column only.  The lane sums its column (t ascending) into the chain mean,
// which it keeps in a register, and forms d = (double)x - m on every read from LDS: d[c,t] is the same value at every use.  The lag sums run
// in blocks of CHAIN_DIAG_LAGS lags: a window of that many d's slides along t (one new d per step), each lag's accumulator takes its
// fma's in ascending t; the d's past the end of the chain are zeros, whose fma's change nothing (steps that stay inside the chain issue
// their 2 L reads together, unguarded).  The accumulators of sum_c gamma[c,k] sit in LDS as doubles — as sum_c S[c,k]: N - k is the
// same for every chain, so the one division waits for the epilogue, which visits the lags up to the stopping pair only —, laid out
// [k][column] like the stage: a wave's lanes read consecutive words, no bank is hit twice.  The means' spread over the chains (and over
// the 2C half chains) is Welford's update in ascending c.  No atomics, no cross-lane operation: the bits of a column's results are a function of
// its C * N values alone, whatever P, the other columns, the row stride, the base alignment (both load paths widen the same fp32 values) and
// the column slabs a caller cuts.
//
// The tile: stage + accumulators take 12 N T bytes.  T is 64 while four blocks, one per SIMD, fit the 160 KiB of a CU together (N <= 53), 32
// while four of those do (N <= 106), 16 beyond — a column costs its N^2 / 2 fma's per chain whatever the tile, so narrow tiles that keep
// every SIMD busy beat a wide one that fills the LDS alone.  N is limited by the 16-wide tile: RBNN_CHAIN_DIAG_MAX_DRAWS = 768 draws take
// 147 456 bytes.  The tile is a function of N alone, and a lane's arithmetic does not depend on it.

#include "rbnn_common.hpp"
#include <algorithm>

namespace {

constexpr int CHAIN_DIAG_LDS_BYTES = 160 * 1024;
constexpr int CHAIN_DIAG_LAGS = 8;
static_assert(12 * RBNN_CHAIN_DIAG_MAX_DRAWS * 16 <= CHAIN_DIAG_LDS_BYTES, "the narrowest tile fits a CU at the cap");
static_assert(RBNN_CHAIN_DIAG_MAX_DRAWS >= 512, "the reference's runs keep a few hundred draws per chain");

struct ChainDiagArgs {
    const float* X;  long long ldx;
    int C, N;  long long P;
    double *mean, *std, *r_hat, *split_r_hat, *tau, *n_eff;
    int* n_pairs;
};

// Welford's running mean and sum of squared deviations of a sequence of values, in the order they arrive
struct ChainDiagSpread {
    double mean = 0., q = 0.;
    int n = 0;
    __device__ __forceinline__ void add(double v) {
        const double dm = v - mean;
        mean += dm / (double)++n;
        q = fma(dm, v - mean, q);
    }
};

// sqrt(V / W) with hmc.split_r_hat's convention for constant sequences
__device__ __forceinline__ double chain_diag_ratio(double V, double W) {
    return W == 0. ? (V == 0. ? 1. : __builtin_inf()) : sqrt(V / W);
}

template <int T, bool VEC>
__global__ void __launch_bounds__(T) chain_diag_columns_kernel(const ChainDiagArgs a) {
    extern __shared__ __attribute__((aligned(16))) float chain_diag_lds[];
    constexpr int QUADS = T / 4, L = CHAIN_DIAG_LAGS;
    const int N = a.N, C = a.C, tid = threadIdx.x, h = N / 2;
    float* const stage = chain_diag_lds;                                         // [N][T] fp32: one chain of the tile
    const float* const mine = stage + tid;
    double* const g = (double*)(chain_diag_lds + (size_t)N * T) + tid;           // [N][T] doubles: sum_c S[c][k], this lane's column
    const long long e0 = (long long)blockIdx.x * T;
    const bool live = e0 + tid < a.P;
    ChainDiagSpread means, halves;
    double msum = 0., s0sum = 0., hsum = 0.;              // sum_c m_c, sum_c S[c,0], sum over the 2C half chains of their gamma_0

    for (int c = 0; c < C; ++c) {
        __syncthreads();                                                         // the previous chain's readers are done
        for (int i = tid; i < N * QUADS; i += T) {
            const int t = i / QUADS, q = i - t * QUADS;
            const long long e = e0 + 4 * q;
            const float* const src = a.X + ((long long)c * N + t) * a.ldx + e;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (VEC && e + 4 <= a.P) {
                v = *(const f32x4*)src;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (e + j < a.P) v[j] = src[j];
            }
            *(f32x4*)(stage + t * T + 4 * q) = v;
        }
        __syncthreads();
        if (!live) continue;

        double s = 0.;
        for (int t = 0; t < N; ++t) s += (double)mine[t * T];
        const double m = s / (double)N;
        msum += m;
        means.add(m);
        auto d = [&](int t) { return t < N ? (double)mine[t * T] - m : 0.; };

        // the two half chains of the split form: the first h and the last h draws
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int t0 = half ? N - h : 0;
            double sh = 0.;
            for (int t = t0; t < t0 + h; ++t) sh += (double)mine[t * T];
            const double mh = sh / (double)h;
            double qh = 0.;
            for (int t = t0; t < t0 + h; ++t) {
                const double dh = (double)mine[t * T] - mh;
                qh = fma(dh, dh, qh);
            }
            hsum += qh / (double)h;
            halves.add(mh);
        }

        // the lag sums, L lags at a time: slot (u + j) % L of the window holds d[t + u + k0 + j] at step t + u
        for (int k0 = 0; k0 < N; k0 += L) {
            double acc[L], w[L];
#pragma unroll
            for (int j = 0; j < L; ++j) { acc[j] = 0.; w[j] = d(k0 + j); }
            int t = 0;
            // whole steps of L draws with every index inside the chain: the 2 L reads go out together, ahead of the L * L fma's
            for (; t + k0 + 2 * L <= N; t += L) {
                double x[L], nw[L];
#pragma unroll
                for (int u = 0; u < L; ++u) {
                    x[u] = (double)mine[(t + u) * T] - m;
                    nw[u] = (double)mine[(t + u + k0 + L) * T] - m;
                }
#pragma unroll
                for (int u = 0; u < L; ++u) {
#pragma unroll
                    for (int j = 0; j < L; ++j) acc[j] = fma(x[u], w[(u + j) % L], acc[j]);
                    w[u] = nw[u];
                }
            }
            // the steps that reach past the end: the same fma's in the same order, zeros beyond the chain
            for (; t < N - k0; t += L) {
#pragma unroll
                for (int u = 0; u < L; ++u) {
                    const double x = d(t + u);
#pragma unroll
                    for (int j = 0; j < L; ++j) acc[j] = fma(x, w[(u + j) % L], acc[j]);
                    w[u] = d(t + u + k0 + L);
                }
            }
            if (k0 == 0) s0sum += acc[0];
#pragma unroll
            for (int j = 0; j < L; ++j) {
                const int k = k0 + j;
                if (k < N) g[k * T] = (c ? g[k * T] : 0.) + acc[j];
            }
        }
    }
    if (!live) return;

    const long long e = e0 + tid;
    const double Cd = (double)C, Nd = (double)N, hd = (double)h;
    if (a.mean) a.mean[e] = msum / Cd;
    if (a.std) a.std[e] = sqrt(fma(Nd, means.q, s0sum) / (Cd * Nd - 1.));
    const double between = C > 1 ? means.q / (Cd - 1.) : 0.;
    auto gamma = [&](int k) { return g[k * T] / (Cd * (double)(N - k)); };        // mean_c gamma[c,k]: N - k is every chain's divisor
    const double W = gamma(0) * Nd / (Nd - 1.);
    const double V = W * (Nd - 1.) / Nd + between;
    if (a.r_hat) a.r_hat[e] = chain_diag_ratio(V, W);
    if (a.split_r_hat) {
        const double Ws = hsum / (2. * Cd) * hd / (hd - 1.);
        a.split_r_hat[e] = chain_diag_ratio(Ws * (hd - 1.) / hd + halves.q / (2. * Cd - 1.), Ws);
    }
    if (!a.tau && !a.n_eff && !a.n_pairs) return;
    double tau = __builtin_nan("");
    int pairs = 0;
    if (W != 0.) {
        // Geyer's initial monotone positive sequence: from the first pair sum <= 0 on every term is zero
        double low = __builtin_inf(), sum = 0.;
        for (pairs = 0; pairs < h; ++pairs) {
            const double even = pairs ? 1. - (W - gamma(2 * pairs)) / V : 1.;
            const double odd = 1. - (W - gamma(2 * pairs + 1)) / V;
            const double Rho = even + odd;
            if (!(Rho > 0.)) break;
            low = fmin(low, Rho);
            sum += low;
        }
        tau = 2. * sum - 1.;
    }
    if (a.tau) a.tau[e] = tau;
    if (a.n_eff) a.n_eff[e] = Cd * Nd / tau;
    if (a.n_pairs) a.n_pairs[e] = pairs;
}

// ---- host ----
inline int chain_diag_tile(int N) {
    if (4 * 12 * N * 64 <= CHAIN_DIAG_LDS_BYTES) return 64;
    if (4 * 12 * N * 32 <= CHAIN_DIAG_LDS_BYTES) return 32;
    return 16;
}
inline size_t chain_diag_block_bytes(int N) { return (size_t)12 * N * chain_diag_tile(N); }
// what both entry points refuse: counts, the cap, rows * stride that would not be addressable
inline int chain_diag_check(int C, int N, long long P) {
    if (C < 1 || N < 4 || N > RBNN_CHAIN_DIAG_MAX_DRAWS || P < 1 || (long long)C * N > 0x7fffffffLL) return RBNN_ERR_SHAPE;
    if ((P + 15) / 16 > 0x7fffffffLL) return RBNN_ERR_SHAPE;
    return RBNN_OK;
}

template <int T, bool VEC>
int chain_diag_launch(const ChainDiagArgs& a, int max_n, hipStream_t st) {
    static unsigned long long done = 0;
    if (!ensure_dynamic_lds((const void*)chain_diag_columns_kernel<T, VEC>, 12 * max_n * T, done)) return RBNN_ERR_LAUNCH;
    hipLaunchKernelGGL((chain_diag_columns_kernel<T, VEC>), dim3((unsigned)((a.P + T - 1) / T)), dim3(T), chain_diag_block_bytes(a.N), st, a);
    return launch_status();
}

}  // namespace

// ===================================================================================================
// C-ABI of the chain diagnostics
// ===================================================================================================
extern "C" {

int rbnn_chain_diag_query(int32_t n_chains, int32_t n_draws, int64_t P, int32_t* max_draws, size_t* lds_bytes) {
    if (max_draws) *max_draws = RBNN_CHAIN_DIAG_MAX_DRAWS;
    const int rc = chain_diag_check(n_chains, n_draws, P);
    if (rc) return rc;
    if (lds_bytes) *lds_bytes = chain_diag_block_bytes(n_draws);
    return RBNN_OK;
}

int rbnn_chain_diag(const float* X, int64_t ldx, int32_t n_chains, int32_t n_draws, int64_t P, double* mean, double* std, double* r_hat,
                    double* split_r_hat, double* tau, double* n_eff, int32_t* n_pairs, void* stream) {
    if (!X) return RBNN_ERR_NULL;
    const int rc = chain_diag_check(n_chains, n_draws, P);
    if (rc) return rc;
    if (ldx < P || ldx > (long long)(0x7fffffffffffffffLL / 8) / ((long long)n_chains * n_draws)) return RBNN_ERR_SHAPE;
    if (!mean && !std && !r_hat && !split_r_hat && !tau && !n_eff && !n_pairs) return RBNN_OK;
    const ChainDiagArgs a = {X, (long long)ldx, n_chains, n_draws, (long long)P, mean, std, r_hat, split_r_hat, tau, n_eff, n_pairs};
    const bool vec = aligned16(X) && !(ldx & 3);
    hipStream_t st = (hipStream_t)stream;
    switch (chain_diag_tile(n_draws)) {
        case 64: return vec ? chain_diag_launch<64, true>(a, 53, st) : chain_diag_launch<64, false>(a, 53, st);
        case 32: return vec ? chain_diag_launch<32, true>(a, 106, st) : chain_diag_launch<32, false>(a, 106, st);
        default: return vec ? chain_diag_launch<16, true>(a, RBNN_CHAIN_DIAG_MAX_DRAWS, st)
                            : chain_diag_launch<16, false>(a, RBNN_CHAIN_DIAG_MAX_DRAWS, st);
    }
}

}  // extern "C"
