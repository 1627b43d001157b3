// rbnn_predictive.inc — posterior-predictive uncertainty and calibration (included by rbnn_nn_train.hip beside rbnn_wpca.inc and
// rbnn_chain_diag.inc: nothing here touches a trainer).  Every forward leaves the per-sample probabilities P [S][N][ldp] in its workspace and
// reduces them to their mean; this reads the same P once more and leaves, per point, what the samples say beyond the mean (the header
// states the definitions in full): entropy of the mean, expected entropy, their difference, the first-maximum prediction with its confidence,
// the share of samples that vote for it, the variance over the samples of its probability, and with labels nll, brier and correct.
//
// predictive_stats_kernel<T, LABELS>: T is P's element type (float: the exact / triple / split / conv forwards; double: the two checkers),
// widened to double on load.  16 adjacent lanes take one point, lane c class column c: a wave covers 4 points and reads, per sample, 4 runs of
// C adjacent elements (256 contiguous bytes of a padded fp32 row group); a block is 16 points.  A lane keeps its class's running sum, Welford
// mean / M2, sum of p ln p and vote count in registers; per sample the only cross-lane work is the first-maximum butterfly over the 16-lane
// row (on T: widening keeps the order).  Samples are loaded PRED_UNROLL at a time ahead of their arithmetic.  At every prefix boundary the
// row forms pbar = sum / S_j and its figures — sums over c run in ascending c, every lane of the row computing the same chain from shuffled
// terms — and lane 0 stores row j of the outputs; the accumulators run on, so P is swept once whatever the prefixes.  A sample's update does
// not know the prefixes, the unroll position or its point's place in the block: the bits of a point's figures are a function of its S x C
// values and the prefix list alone.  Lanes of columns >= C load nothing and enter the maxima as -1; lanes of points >= N shadow point N - 1
// (every lane stays active for the shuffles) and store nothing.
//
// predictive_bins_kernel / predictive_bins_sum_kernel: a block stages RBNN_PREDICTIVE_BLOCK points' bin, confidence, correct, nll and brier in
// LDS; thread b < n_bins then adds the points of bin b in ascending order, three more threads the totals: one partial record of 3 n_bins + 3
// eight-byte sums per block.  The second launch adds the records in ascending block order, one thread per sum.  No atomics anywhere.

#include "rbnn_common.hpp"

namespace {

constexpr int PRED_UNROLL = 4;
constexpr int PRED_THREADS = 256, PRED_POINTS = PRED_THREADS / 16;
static_assert(RBNN_CPAD == 16, "one lane per padded class column");
static_assert(3 * RBNN_PREDICTIVE_MAX_BINS + 3 <= RBNN_PREDICTIVE_BLOCK, "one thread per partial sum");

struct PredictiveArgs {
    const void* P;  long long ss;  int ldp, N, C;
    const int* labels;
    int J, pre[RBNN_PREDICTIVE_MAX_PREFIXES];
    long long os;
    double *entropy, *expected, *mi, *confidence, *agreement, *variance, *nll, *brier;
    int *prediction, *correct;
};

// the first maximum over the 16-lane row of (v, k = its column): every lane ends with the same pair
template <class V> __device__ __forceinline__ void predictive_first_max(V& v, int& k) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) {
        const V ov = __shfl_xor(v, m, 16);
        const int ok = __shfl_xor(k, m, 16);
        if (ov > v || (ov == v && ok < k)) { v = ov; k = ok; }
    }
}

// sum over c < C of the row's terms in ascending c: the same chain in every lane of the row
__device__ __forceinline__ double predictive_row_sum(double term, int C) {
    double acc = 0.;
#pragma unroll
    for (int cc = 0; cc < 16; ++cc) {
        const double t = __shfl(term, cc, 16);
        if (cc < C) acc += t;
    }
    return acc;
}

__device__ __forceinline__ double predictive_plogp(double p) { return p > 0. ? p * log(p) : 0.; }

template <class T, bool LABELS>
__global__ void __launch_bounds__(PRED_THREADS) predictive_stats_kernel(const PredictiveArgs a) {
    const int c = threadIdx.x & 15, C = a.C;
    const long long n = (long long)blockIdx.x * PRED_POINTS + (threadIdx.x >> 4);
    const bool live = n < a.N, mine = c < C;
    const long long row = live ? n : (long long)a.N - 1;
    const T* const src = (const T*)a.P + row * a.ldp + (mine ? c : 0);
    const int y = LABELS ? a.labels[row] : -1;
    double sum = 0., mean = 0., m2 = 0., ee = 0.;
    int votes = 0, s = 0;

    for (int j = 0; j < a.J; ++j) {
        const int end = a.pre[j];
        for (; s < end; s += PRED_UNROLL) {
            T v[PRED_UNROLL];
#pragma unroll
            for (int u = 0; u < PRED_UNROLL; ++u) v[u] = (mine && s + u < end) ? src[(long long)(s + u) * a.ss] : (T)0;
#pragma unroll
            for (int u = 0; u < PRED_UNROLL; ++u) {
                if (s + u >= end) break;                                          // (uniform over the block)
                T best = mine ? v[u] : (T)-1;
                int k = c;
                predictive_first_max(best, k);
                votes += k == c;
                if (mine) {
                    const double p = (double)v[u];
                    sum += p;
                    const double d = p - mean;
                    mean += d / (double)(s + u + 1);
                    m2 = fma(d, p - mean, m2);
                    ee += predictive_plogp(p);
                }
            }
        }
        s = end;

        const double Sd = (double)end;
        const double pb = mine ? sum / Sd : 0.;
        double conf = mine ? pb : -1.;
        int k = c;
        predictive_first_max(conf, k);
        const double H = -predictive_row_sum(predictive_plogp(pb), C);
        const double E = -predictive_row_sum(ee, C) / Sd;
        const double var = __shfl(m2, k, 16) / Sd;
        const int agree = __shfl(votes, k, 16);
        double nll = 0., brier = 0.;
        if (LABELS) {
            const bool named = y >= 0 && y < C;
            const double py = __shfl(pb, y & 15, 16);
            nll = -log(named ? py : 0.);
            const double dlt = pb - (c == y ? 1. : 0.);
            brier = predictive_row_sum(dlt * dlt, C);
        }
        if (live && c == 0) {
            const long long o = (long long)j * a.os + n;
            if (a.entropy) a.entropy[o] = H;
            if (a.expected) a.expected[o] = E;
            if (a.mi) a.mi[o] = H - E;
            if (a.confidence) a.confidence[o] = conf;
            if (a.agreement) a.agreement[o] = (double)agree / Sd;
            if (a.variance) a.variance[o] = var;
            if (a.prediction) a.prediction[o] = k;
            if (LABELS) {
                if (a.nll) a.nll[o] = nll;
                if (a.brier) a.brier[o] = brier;
                if (a.correct) a.correct[o] = k == y;
            }
        }
    }
}

// ---- calibration ----
struct PredictiveBinArgs {
    const double *confidence, *nll, *brier;
    const int* correct;
    int N, n_bins, n_blocks;
    long long* ws;                                    // [n_blocks][3 n_bins + 3] eight-byte sums: count, confidence, correct per bin; nll, brier, correct
    long long* bin_count;  double* bin_confidence;  long long* bin_correct;  double* totals;  long long* n_correct;
};

__device__ __forceinline__ long long predictive_bits(double v) { return __double_as_longlong(v); }

__global__ void __launch_bounds__(RBNN_PREDICTIVE_BLOCK) predictive_bins_kernel(const PredictiveBinArgs a) {
    __shared__ double conf[RBNN_PREDICTIVE_BLOCK], nl[RBNN_PREDICTIVE_BLOCK], br[RBNN_PREDICTIVE_BLOCK];
    __shared__ int bin[RBNN_PREDICTIVE_BLOCK], ok[RBNN_PREDICTIVE_BLOCK];
    const int t = threadIdx.x, nb = a.n_bins;
    const long long i0 = (long long)blockIdx.x * RBNN_PREDICTIVE_BLOCK;
    const int cnt = (int)min((long long)RBNN_PREDICTIVE_BLOCK, (long long)a.N - i0);
    if (t < cnt) {
        const double cf = a.confidence[i0 + t];
        conf[t] = cf;
        bin[t] = min(nb - 1, max(0, (int)ceil(cf * (double)nb) - 1));
        ok[t] = a.correct[i0 + t] != 0;
        nl[t] = a.nll ? a.nll[i0 + t] : 0.;
        br[t] = a.brier ? a.brier[i0 + t] : 0.;
    }
    __syncthreads();
    long long* const rec = a.ws + (long long)blockIdx.x * (3 * nb + 3);
    if (t < nb) {
        long long count = 0, good = 0;
        double sc = 0.;
        for (int i = 0; i < cnt; ++i)
            if (bin[i] == t) { ++count; sc += conf[i]; good += ok[i]; }
        rec[t] = count;
        rec[nb + t] = predictive_bits(sc);
        rec[2 * nb + t] = good;
    } else if (t == RBNN_PREDICTIVE_MAX_BINS || t == RBNN_PREDICTIVE_MAX_BINS + 1) {
        const double* const v = t == RBNN_PREDICTIVE_MAX_BINS ? nl : br;
        double sv = 0.;
        for (int i = 0; i < cnt; ++i) sv += v[i];
        rec[3 * nb + (t - RBNN_PREDICTIVE_MAX_BINS)] = predictive_bits(sv);
    } else if (t == RBNN_PREDICTIVE_MAX_BINS + 2) {
        long long good = 0;
        for (int i = 0; i < cnt; ++i) good += ok[i];
        rec[3 * nb + 2] = good;
    }
}

__global__ void __launch_bounds__(RBNN_PREDICTIVE_BLOCK) predictive_bins_sum_kernel(const PredictiveBinArgs a) {
    const int t = threadIdx.x, nb = a.n_bins, R = 3 * nb + 3;
    if (t >= R) return;
    const bool real = (t >= nb && t < 2 * nb) || t == 3 * nb || t == 3 * nb + 1;          // a double; the others count
    long long cnt = 0;
    double sv = 0.;
    for (int b = 0; b < a.n_blocks; ++b) {
        const long long w = a.ws[(long long)b * R + t];
        if (real) sv += __longlong_as_double(w); else cnt += w;
    }
    if (t < nb) { if (a.bin_count) a.bin_count[t] = cnt; }
    else if (t < 2 * nb) { if (a.bin_confidence) a.bin_confidence[t - nb] = sv; }
    else if (t < 3 * nb) { if (a.bin_correct) a.bin_correct[t - 2 * nb] = cnt; }
    else if (t < 3 * nb + 2) { if (a.totals) a.totals[t - 3 * nb] = sv; }
    else if (a.n_correct) a.n_correct[0] = cnt;
}

// ---- host ----
inline bool predictive_aligned(const void* p, unsigned bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1u)) == 0; }
inline int predictive_bins_check(int N, int n_bins) {
    return (N < 1 || n_bins < 1 || n_bins > RBNN_PREDICTIVE_MAX_BINS) ? RBNN_ERR_SHAPE : RBNN_OK;
}
inline long long predictive_blocks(int N) { return ((long long)N + RBNN_PREDICTIVE_BLOCK - 1) / RBNN_PREDICTIVE_BLOCK; }

template <class T>
int predictive_launch(const PredictiveArgs& a, hipStream_t st) {
    const dim3 grid((unsigned)(((long long)a.N + PRED_POINTS - 1) / PRED_POINTS));
    if (a.labels) hipLaunchKernelGGL((predictive_stats_kernel<T, true>), grid, dim3(PRED_THREADS), 0, st, a);
    else hipLaunchKernelGGL((predictive_stats_kernel<T, false>), grid, dim3(PRED_THREADS), 0, st, a);
    return launch_status();
}

}  // namespace

// ===================================================================================================
// C-ABI of the predictive statistics
// ===================================================================================================
extern "C" {

int rbnn_predictive_stats(const void* P, int32_t elem_type, int64_t sample_stride, int32_t ldp, int32_t n_samples, int32_t n_points,
                          int32_t n_classes, const int32_t* labels, const int32_t* prefixes, int32_t n_prefixes, int64_t out_stride,
                          double* entropy, double* expected_entropy, double* mutual_information, double* confidence, double* agreement,
                          double* variance, double* nll, double* brier, int32_t* prediction, int32_t* correct, void* stream) {
    if (!P || !prefixes) return RBNN_ERR_NULL;
    if (!labels && (nll || brier || correct)) return RBNN_ERR_NULL;
    if (elem_type != RBNN_PREDICTIVE_FLOAT && elem_type != RBNN_PREDICTIVE_DOUBLE) return RBNN_ERR_SHAPE;
    if (n_classes < 2 || n_classes > RBNN_CPAD || n_samples < 1 || n_points < 1 || ldp < n_classes) return RBNN_ERR_SHAPE;
    if (n_prefixes < 1 || n_prefixes > RBNN_PREDICTIVE_MAX_PREFIXES) return RBNN_ERR_SHAPE;
    for (int j = 0; j < n_prefixes; ++j)
        if (prefixes[j] < 1 || prefixes[j] > n_samples || (j && prefixes[j] <= prefixes[j - 1])) return RBNN_ERR_SHAPE;
    if (sample_stride < (long long)n_points * ldp || out_stride < n_points) return RBNN_ERR_SHAPE;
    if (sample_stride > (long long)(0x7fffffffffffffffLL / 8) / n_samples || out_stride > (long long)(0x7fffffffffffffffLL / 8) / n_prefixes)
        return RBNN_ERR_SHAPE;
    const unsigned esz = elem_type == RBNN_PREDICTIVE_DOUBLE ? 8u : 4u;
    if (!predictive_aligned(P, esz) || !predictive_aligned(labels, 4)) return RBNN_ERR_ALIGN;
    for (const double* o : {entropy, expected_entropy, mutual_information, confidence, agreement, variance, nll, brier})
        if (!predictive_aligned(o, 8)) return RBNN_ERR_ALIGN;
    if (!predictive_aligned(prediction, 4) || !predictive_aligned(correct, 4)) return RBNN_ERR_ALIGN;
    if (!entropy && !expected_entropy && !mutual_information && !confidence && !agreement && !variance && !nll && !brier && !prediction && !correct)
        return RBNN_OK;
    PredictiveArgs a = {P, (long long)sample_stride, ldp, n_points, n_classes, labels, n_prefixes, {}, (long long)out_stride,
                        entropy, expected_entropy, mutual_information, confidence, agreement, variance, nll, brier, prediction, correct};
    for (int j = 0; j < n_prefixes; ++j) a.pre[j] = prefixes[j];
    return elem_type == RBNN_PREDICTIVE_DOUBLE ? predictive_launch<double>(a, (hipStream_t)stream) : predictive_launch<float>(a, (hipStream_t)stream);
}

int rbnn_predictive_calibration_query(int32_t n_points, int32_t n_bins, size_t* bytes) {
    if (!bytes) return RBNN_ERR_NULL;
    const int rc = predictive_bins_check(n_points, n_bins);
    if (rc) return rc;
    *bytes = (size_t)predictive_blocks(n_points) * (3 * n_bins + 3) * 8;
    return RBNN_OK;
}

int rbnn_predictive_calibration(const double* confidence, const int32_t* correct, const double* nll, const double* brier, int32_t n_points,
                                int32_t n_bins, int64_t* bin_count, double* bin_confidence, int64_t* bin_correct, double* totals,
                                int64_t* n_correct, void* ws, size_t ws_bytes, void* stream) {
    if (!confidence || !correct || !ws) return RBNN_ERR_NULL;
    const int rc = predictive_bins_check(n_points, n_bins);
    if (rc) return rc;
    const long long blocks = predictive_blocks(n_points);
    if (ws_bytes < (size_t)blocks * (3 * n_bins + 3) * 8) return RBNN_ERR_SHAPE;
    for (const void* p : {(const void*)confidence, (const void*)nll, (const void*)brier, (const void*)bin_count, (const void*)bin_confidence,
                          (const void*)bin_correct, (const void*)totals, (const void*)n_correct, (const void*)ws})
        if (!predictive_aligned(p, 8)) return RBNN_ERR_ALIGN;
    if (!predictive_aligned(correct, 4)) return RBNN_ERR_ALIGN;
    if (!bin_count && !bin_confidence && !bin_correct && !totals && !n_correct) return RBNN_OK;
    const PredictiveBinArgs a = {confidence, nll, brier, correct, n_points, n_bins, (int)blocks, (long long*)ws,
                                 (long long*)bin_count, bin_confidence, (long long*)bin_correct, totals, (long long*)n_correct};
    hipLaunchKernelGGL(predictive_bins_kernel, dim3((unsigned)blocks), dim3(RBNN_PREDICTIVE_BLOCK), 0, (hipStream_t)stream, a);
    if (launch_status()) return RBNN_ERR_LAUNCH;
    hipLaunchKernelGGL(predictive_bins_sum_kernel, dim3(1), dim3(RBNN_PREDICTIVE_BLOCK), 0, (hipStream_t)stream, a);
    return launch_status();
}

}  // extern "C"
