// rbnn_conv_train.hip — deterministic training of ONE conv net of the 1x28x28 geometry (model_nn.py:93-106, 175-219: torch.optim.Adam on
// nn.CrossEntropyLoss()):  Conv2d(1,32,5) -> act -> MaxPool2d(2) -> Conv2d(32,Hc,5) -> act -> MaxPool2d(2, stride 1) -> Flatten -> Linear(49 Hc, C).
//
//      rbnn_conv_train_forward    the exact fp32-MFMA forward of rbnn_conv.hip (one sample, logits out: P1, st1, Q2, st2 stay behind for the
//                                 backward; 3 launches) and the head: CE per point, dZ = (softmax - e_y) / B, correct (1 launch)
//      rbnn_conv_weight_grads     dFw | dFb      = dZ^T [Q2 | 1]                              the strided GEMM of rbnn_train_gemm.hpp
//                                 dO2            = (dZ Fw) gathered through the pool-2 stash, times act'                (conv_do2_kernel)
//                                 dP1            = conv2^T(dO2), per slice of the conv2 channels                        (GEMM, mode G_DP1)
//                                 dO1            = the slices of dP1 added, routed through the pool-1 stash, times act' (conv_route1_kernel)
//                                 dK2 | dK2b     = sum over (point, position) of dO2 x [P1 patch | 1], per batch slice  (GEMM, mode G_DK2)
//                                 dK1 | dK1b     = sum over (point, position) of dO1 x [x patch | 1], per batch slice   (GEMM, mode G_DK1)
//                                 the slices' partial sums added in one fixed order, fp64                               (conv_reduce_kernel)
//                                 conv_weight_grads<ENS> is these seven launches for both forms; the kernels are templates on ENS
//      rbnn_conv_adam_step        torch.optim.Adam's single-tensor formula on the flat buffer: 1 launch                  (nn_adam_kernel<false>)
//      rbnn_conv_train_finalize   the fp32-rounded mean CE of the step, its running sum, the correct predictions: 1 launch (nn_finalize_kernel<false>)
//                                 both kernels are rbnn_nn_step.hpp's, shared with the fc members of rbnn_nn_train.hip, the member index compiled out
//
// and SVI training of one conv GUIDE (model_bnn.py:303-365, the step of rbnn_train.hip around the same forward and weight gradients):
//      rbnn_conv_svi_train_draw     W = loc + sigma * eps for the six tensors: rbnn_svi_draw_flat on views of the flat buffers, 1 launch
//      rbnn_conv_svi_train_forward  the training forward above on W with the SUMMED cross-entropy (dZ = softmax - e_y, no 1 / B): 3 + 1 launches
//      rbnn_conv_svi_weight_grads   the weight gradients above, reading W and writing grad = dCE/dW: 7 launches, the same kernels
//      rbnn_conv_svi_adam_step      rbnn_svi_step.hpp's adam_kernel<Single> over the six conv tensors, each one row of n_elem columns (the
//                                   regenerated eps quad is e / 4, rbnn_svi_draw_flat's counter): loc, raw, sigma, moments, KL partials.  1 launch
//      the step's sums are rbnn_svi_train_finalize (rbnn_train.hip: 1 launch); the accuracy forward is the host's (rbnn_svi_draw_flat of 10
//      weight sets into a resident stack, rbnn_conv_forward on the exact path, rbnn_reduce_samples: 1 + 3 + 1 launches).
//      One SVI step = 1 + 4 + 7 + 1 + 1 = 14 launches without the accuracy forward, 19 with it.
//
// and deterministic training of M conv nets of one shape in LOCKSTEP (model_ensemble.py:69-83 for conv: the members share nothing but their
// shapes, so every launch of the single net's step takes the member as a grid dimension and the launch count does not grow with M):
//      rbnn_conv_ens_stage          member m's B rows of the resident data (rows [M, B], clamped) -> Xs [M B, 784], labels [M B]: 1 launch
//                                   (conv_ens_stage_kernel); no kernel after it sees rows, every heavy kernel works on a packed batch
//      rbnn_conv_ens_forward        the exact forward with S = M samples on the packed batch (conv1_pool_kernel<.., 1> reads row s N + n;
//                                   conv2_pool_kernel and conv_fc_kernel as they are) and conv_head_kernel over M B points: 3 + 1 launches
//      rbnn_conv_ens_weight_grads   the 7 launches above with ENS = true: member = blockIdx.y (train_gemm_kernel<true, false>, conv_do2 /
//                                   _route1_kernel, conv_ens_reduce_kernel) or blockIdx.z (conv_wgrad_gemm_kernel: y is the K slice); partial sums
//                                   [M][slices][...].  The slice counts stay functions of B and Hc alone: member m's sums in the single net's order
//      rbnn_conv_ens_adam_step      nn_adam_kernel<false> over all M n_params elements (element-wise: the members share t and lr): 1 launch
//      rbnn_conv_ens_finalize       nn_finalize_kernel<true>, one block per member: 1 launch
//      One lockstep step = 1 + 4 + 7 + 1 + 1 = 14 launches whatever M is.  The flat buffers are TENSOR-MAJOR (six blocks [M, size of tensor]
//      in state_dict order: rbnn_conv_posterior's stacks, so the forward addresses member m as sample m).
//
// and SVI training of K conv guides of one shape in LOCKSTEP (the SVI step above for every guide in one set of launches; the flat buffers are
// tensor-major as the ensemble's, so the guides are the members of the staging, the forward and the weight gradients):
//      rbnn_conv_svi_guides_draw      W[k] = loc[k] + sigma[k] * eps(keys[k], draw id): svils_draw_kernel<TensorMajor>, the flat draw's bits.  1 launch
//      rbnn_conv_svi_guides_gradient  rbnn_conv_ens_stage, the members' forward with the SUMMED cross-entropy (dZ scale 1), the members' 7
//                                    weight-gradient launches on the view (P = W, grad = grad): 1 + 4 + 7 launches
//      rbnn_conv_svi_guides_adam_step adam_kernel<TensorMajor>: the single guide's Adam + KL text on tensor-major offsets, per-guide key and lr.  1 launch.
//                                    Instantiated and launched in rbnn_svi.hip, not here: a second instance of adam_kernel in THIS unit changes
//                                    the code its adam_kernel<Single> compiles to (profiles/svi_one_family/README.txt)
//      rbnn_conv_svi_guides_accuracy  svils_draw_kernel<TensorMajor> of the K * 10 weight sets under keys[k] ^ key_xor, the exact forward of those nets on
//                                    the K staged batches (conv1_pool_kernel<.., 2>: set k * 10 + s reads guide k's rows; conv2_pool_kernel and
//                                    conv_fc_kernel as they are), conv_svils_acc_sum_kernel: 1 + 3 + 1 launches
//      rbnn_conv_svi_guides_finalize  svils_finalize_kernel<false>, one block per guide: the step's sums and the epoch's end on the device.  1 launch
//      One lockstep SVI step = 1 + 12 + 1 + 1 = 15 launches without the accuracy forward, 20 with it, whatever K is.  A guide that has finished
//      (active[k] == 0) is skipped by the four kernels: nothing of its state is written again.  The draw, Adam + KL and finalize kernels are
//      rbnn_svi_step.hpp's templates, the ones the fc guides of rbnn_svi_lockstep.hip run guide-major.
//
// and the gradient of K HMC chains over conv nets of one shape (the chain's element-wise kernels: rbnn_hmc.hip), the chains as the members:
//      rbnn_conv_hmc_chains_stage     rbnn_conv_ens_stage on the view: 1 launch, once per batch
//      rbnn_conv_hmc_chains_gradient  the members' forward with the SUMMED cross-entropy and their 7 weight-gradient launches on the view
//                                     (P = W, grad = grad): 4 + 7 launches per leapfrog step whatever K is.  No device code of its own.
//
// Parameters, moments and gradients are flat fp32 buffers in state_dict order, unpadded (the convention of the fc trainers).  One stream, no
// atomics, no device->host synchronisation: every output element is one lane's sum in one order, two runs are bit-identical.
// The three conv GEMMs are one kernel text (conv_wgrad_gemm_kernel): 64 x 64 (G_DP1: 64 x 32) output tiles of the fp32 MFMA, K staged 16 at
// a time through LDS (the next stage's operands are fetched into registers while this one's MFMAs run), both operands GATHERED by index
// arithmetic (implicit im2col: nothing is unfolded in memory).  Every contraction is split across blocks (grid dimension y) — dK2 (B 64
// terms) and dK1 (B 576 terms, with a 32 x 26 output) over the batch, dP1 (25 Hc terms) over the conv2 channels — and the slices' partial
// sums are added in a second pass, in increasing order.
#include "rbnn_conv_layout.hpp"
#include "rbnn_train_gemm.hpp"
#include "rbnn_nn_step.hpp"
// rbnn_svi_step.hpp names its argument records as rbnn_nn_step.hpp names its own (AdamArgs): it is read into a namespace of its own here, after
// the core it stands on (rbnn_train_core.hpp: already included above, so only the step's own definitions land in the namespace).
namespace svi {
#include "rbnn_svi_step.hpp"
}

using namespace rbnn_conv_shared;

namespace {

constexpr int O1W = GeoMnist::O1, NO1 = O1W * O1W, DIN = GeoMnist::DIN, IW = GeoMnist::IW;     // 24, 576, 784, 28
constexpr int PP1 = P1W * P1W;                                                                   // 144 pooled conv1 positions
constexpr int N2 = K2 + 1, N1 = 25 + 1;                                                          // columns of a partial: the taps | the bias
constexpr int MAX_SPLITS2 = 16, MAX_SPLITS1 = 128;
constexpr int MAX_POINTS = 65536;
constexpr int DP1_BLOCKS = 2048;                                                                 // blocks the dP1 GEMM aims at (8 per CU)

// points per slice and slices of the two split contractions: functions of B alone, never more than min(B, MAX_SPLITS) slices
inline void slices(int B, int max_splits, int& per, int& n) {
    per = (B + max_splits - 1) / max_splits;
    n = (B + per - 1) / per;
}

// slices of dP1's contraction: groups of 16 conv2 channels (400 products) per slice, as many slices as bring the grid to DP1_BLOCKS
inline void dp1_slices(int B, int Hc, int& per, int& n) {
    const int tiles = (B * PP1 + GT - 1) / GT, groups = Hc / 16;
    const int want = std::min(std::max(DP1_BLOCKS / tiles, 1), groups);
    per = (groups + want - 1) / want;
    n = (groups + per - 1) / per;
}
// floats of the dP1 partial sums for any batch of up to B points: slices <= DP1_BLOCKS 64 / (144 B) and <= Hc / 16, and >= 1
inline size_t dp1_part_floats(int B, int Hc) {
    const size_t point = (size_t)PP1 * C1, all = (size_t)(Hc / 16) * B * point;
    return std::max((size_t)B * point, std::min((size_t)DP1_BLOCKS * GT * C1, all));
}

// ---------------------------------------------------------------------------------------------------
// Head: one thread per point.  CE = logsumexp(z) - z_y, dZ = (softmax(z) - e_y) / B (ce_softmax_grad), correct = (first argmax == y): the
// definitions of train_head_kernel.
// ---------------------------------------------------------------------------------------------------
struct ConvHeadArgs { const float* Z; const int32_t* labels; float *dZ, *ce; int32_t* correct; int B, C; float inv_B; };

__global__ void __launch_bounds__(64) conv_head_kernel(const ConvHeadArgs a) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    float z[RBNN_CPAD], g[RBNN_CPAD];
#pragma unroll
    for (int c = 0; c < RBNN_CPAD; ++c) z[c] = a.Z[(long long)b * RBNN_CPAD + c];
    const int y = a.labels[b];
    ce_softmax_grad<RBNN_CPAD>(z, a.C, y, a.inv_B, g);
    float m = -INFINITY, zy = 0.f;
    int best = 0;
#pragma unroll
    for (int c = 0; c < RBNN_CPAD; ++c)
        if (c < a.C) {
            if (z[c] > m) { m = z[c]; best = c; }                         // strictly greater: the first maximum, as torch.argmax
            if (c == y) zy = z[c];
        }
    float den = 0.f, rest = 0.f;
#pragma unroll
    for (int c = 0; c < RBNN_CPAD; ++c)
        if (c < a.C) { const float e = expf(z[c] - m); den += e; if (c != y) rest += e; }
    a.ce[b] = (zy == m) ? log1pf(rest) : logf(den) - (zy - m);
    a.correct[b] = best == y ? 1 : 0;
#pragma unroll
    for (int c = 0; c < RBNN_CPAD; ++c) a.dZ[(long long)b * RBNN_CPAD + c] = g[c];
}

// ---------------------------------------------------------------------------------------------------
// dO2[b, hc, 8 x 8]: one block = one point x 4 conv2 channels.  Phase 1 (4 x 49 threads): dQ2[f] = sum_c dZ[c] Fw[c, f] times act' (relu /
// leaky: the stash's sign bit; sigmoid / tanh: from the value in Q2) into LDS beside the window's argmax.  Phase 2 (4 x 64 threads), GATHER
// form: pool 2 has stride 1, so a position lies in up to 4 windows; it adds those that selected it in the fixed order (y-1, x-1), (y-1, x),
// (y, x-1), (y, x).
// ---------------------------------------------------------------------------------------------------
// ENS (this kernel, the conv GEMMs and conv_route1_kernel): the lockstep form.  The kernel first moves its argument record to the views of ITS
// member (blockIdx.y; the GEMM: blockIdx.z, y being the K slice) of arrays packed [M, B, .], then runs the single net's text.  The single net's
// instances read none of the arguments behind the record.
struct ConvDo2Args { const float *dZ, *Fw, *Q2; const uint8_t* st2; float* dO2; int Hc, C; };

template <int ACT, bool ENS> __global__ void __launch_bounds__(256) conv_do2_kernel(ConvDo2Args a, const int B) {
    if constexpr (ENS) {                                                   // member blockIdx.y of [M, B, .] and of Fw [M, C, 49 Hc]
        const long long mem = blockIdx.y, pt = mem * B, F = (long long)a.Hc * NP2;
        a.dZ += pt * RBNN_CPAD; a.Fw += mem * a.C * F; a.Q2 += pt * F; a.st2 += pt * F; a.dO2 += pt * a.Hc * NPOS;
    }
    __shared__ float gs[4][NP2];
    __shared__ int as[4][NP2];
    const int t = threadIdx.x, groups = a.Hc >> 2;
    const int b = blockIdx.x / groups, hc0 = 4 * (blockIdx.x % groups);
    const int F = a.Hc * NP2;
    if (t < 4 * NP2) {
        const int hl = t / NP2, p = t % NP2;
        const long long f = (long long)(hc0 + hl) * NP2 + p;
        float dq = 0.f;
        for (int c = 0; c < a.C; ++c) dq = fmaf(a.dZ[(long long)b * RBNN_CPAD + c], a.Fw[(long long)c * F + f], dq);
        const int st = a.st2[(long long)b * F + f];
        float d;
        if (smooth_act<ACT>()) d = act_grad_from_value<ACT>(a.Q2[(long long)b * F + f]);
        else d = (st & 4) ? 1.f : act_neg_slope<ACT>();
        gs[hl][p] = dq * d;
        as[hl][p] = st & 3;
    }
    __syncthreads();
    const int hl = t >> 6, pos = t & 63, y = pos >> 3, x = pos & 7;
    float s = 0.f;
#pragma unroll
    for (int dy = 1; dy >= 0; --dy)
#pragma unroll
        for (int dx = 1; dx >= 0; --dx) {
            const int wy = y - dy, wx = x - dx;                            // the window whose cell (dy, dx) this position is
            if (wy >= 0 && wy < P2W && wx >= 0 && wx < P2W) {
                const int p = wy * P2W + wx;
                if (as[hl][p] == dy * 2 + dx) s += gs[hl][p];
            }
        }
    a.dO2[((long long)b * a.Hc + hc0 + hl) * NPOS + pos] = s;
}

// ---------------------------------------------------------------------------------------------------
// The conv GEMMs  C(m, n) = sum_k A(m, k) B(n, k)  on v_mfma_f32_16x16x4_f32, operands gathered (zero outside [M, N, K]):
//   G_DK2  m = hc, n = (ci, tap) | bias, k = (b, pos of 8 x 8):   A = dO2[b, hc, pos],  B = P1[b, ci, pos + tap] | 1         -> part2[slice]
//   G_DK1  m = c,  n = tap | bias,       k = (b, pos of 24 x 24): A = dO1[b, c, pos],   B = x[b, pos + tap] | 1             -> part1[slice]
//   G_DP1  m = (b, Y, X of 12 x 12), n = ci, k = (hc, tap):       A = dO2[b, hc, (Y, X) - tap] or 0,  B = K2w[hc, ci, tap]           -> partP[slice]
// blockIdx.y = the slice of K; every mode stores its slice's sums [slice, M, N].  Inside a slice the accumulator is folded into a second one
// every 32 stages (512 products): one long fp32 chain would carry sqrt(K) roundings of the running sum.
// ---------------------------------------------------------------------------------------------------
enum { G_DK2 = 0, G_DK1 = 1, G_DP1 = 2 };
struct WgArgs {
    const float *A, *Bsrc;
    float* out;
    int Hc, ldx, M, N, K, kc;                       // kc: the K of one slice
};

template <int MODE> __device__ __forceinline__ float wg_load_a(const WgArgs& g, int m, int k) {
    if (MODE == G_DK2) return g.A[((long long)(k >> 6) * g.Hc + m) * NPOS + (k & 63)];
    if (MODE == G_DK1) { const int b = k / NO1, q = k - b * NO1; return g.A[((long long)b * C1 + m) * NO1 + q]; }
    const int b = m / PP1, pp = m - b * PP1, hc = k / 25, tap = k - hc * 25;
    const int y = pp / P1W - tap / 5, x = pp % P1W - tap % 5;
    return ((unsigned)y < (unsigned)O2W && (unsigned)x < (unsigned)O2W) ? g.A[((long long)b * g.Hc + hc) * NPOS + y * O2W + x] : 0.f;
}
template <int MODE> __device__ __forceinline__ float wg_load_b(const WgArgs& g, int n, int k) {
    if (MODE == G_DK2) {
        if (n == K2) return 1.f;
        const int ci = n / 25, tap = n - ci * 25, pos = k & 63;
        return g.Bsrc[(long long)(k >> 6) * P1SZ + ci * PP1 + (tap / 5 + (pos >> 3)) * P1W + tap % 5 + (pos & 7)];
    }
    if (MODE == G_DK1) {
        if (n == 25) return 1.f;
        const int b = k / NO1, q = k - b * NO1;
        return g.Bsrc[(long long)b * g.ldx + (n / 5 + q / O1W) * IW + n % 5 + q % O1W];
    }
    const int hc = k / 25;
    return g.Bsrc[(long long)hc * K2 + n * 25 + (k - hc * 25)];
}

template <int MODE, bool ENS>
__global__ void __launch_bounds__(256) conv_wgrad_gemm_kernel(WgArgs g, const long long a_mem, const long long b_mem, const long long o_mem) {
    if constexpr (ENS) {                                                   // member blockIdx.z: its operands and its slices [slices][M, N]
        const long long mem = blockIdx.z;
        g.A += mem * a_mem; g.Bsrc += mem * b_mem; g.out += mem * o_mem;
    }
    constexpr int NTN = MODE == G_DP1 ? 2 : 4, TN = 16 * NTN;
    __shared__ float As[GK][GLD], Bs[GK][TN + 4];
    const int tiles_n = (g.N + TN - 1) / TN;
    const int m0 = GT * (blockIdx.x / tiles_n), n0 = TN * (blockIdx.x % tiles_n);
    const int k_begin = blockIdx.y * g.kc, k_end = min(k_begin + g.kc, g.K);
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, li = lane & 15, lg = lane >> 4;
    f32x4 acc[NTN], tot[NTN];
#pragma unroll
    for (int nt = 0; nt < NTN; ++nt) acc[nt] = tot[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int kk = t & 15, r0 = t >> 4;
    float ra[4], rb[NTN];
    auto fetch = [&](int k0) {
        const int k = k0 + kk;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = m0 + r0 + 16 * i;
            ra[i] = (m < g.M && k < k_end) ? wg_load_a<MODE>(g, m, k) : 0.f;
        }
#pragma unroll
        for (int i = 0; i < NTN; ++i) {
            const int n = n0 + r0 + 16 * i;
            rb[i] = (n < g.N && k < k_end) ? wg_load_b<MODE>(g, n, k) : 0.f;
        }
    };
    int stage = 0;
    fetch(k_begin);
    for (int k0 = k_begin; k0 < k_end; k0 += GK, ++stage) {
#pragma unroll
        for (int i = 0; i < 4; ++i) As[kk][r0 + 16 * i] = ra[i];
#pragma unroll
        for (int i = 0; i < NTN; ++i) Bs[kk][r0 + 16 * i] = rb[i];
        __syncthreads();
        if (k0 + GK < k_end) fetch(k0 + GK);
#pragma unroll
        for (int ks = 0; ks < GK / 4; ++ks) {
            const float a = As[4 * ks + lg][16 * wave + li];
#pragma unroll
            for (int nt = 0; nt < NTN; ++nt) acc[nt] = MFMA16(a, Bs[4 * ks + lg][16 * nt + li], acc[nt]);
        }
        __syncthreads();
        if ((stage & 31) == 31) {
#pragma unroll
            for (int nt = 0; nt < NTN; ++nt) { tot[nt] += acc[nt]; acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
        }
    }
    // lane holds C(m0 + 16 wave + 4 lg + r, n0 + 16 nt + li)
#pragma unroll
    for (int nt = 0; nt < NTN; ++nt) {
        tot[nt] += acc[nt];
        const int n = n0 + 16 * nt + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + 16 * wave + 4 * lg + r;
            if (m < g.M && n < g.N) g.out[((long long)blockIdx.y * g.M + m) * g.N + n] = tot[nt][r];
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// dO1[b, ci, 24 x 24]: one thread per (b, pooled position, ci).  dP1 = the slices of partP in increasing order (fp64), times act' (relu /
// leaky: the pool-1 stash's sign bit; sigmoid / tanh: from the value in P1), goes to the cell of its 2 x 2 window that the stash names and
// zero to the other three: pool 1 does not overlap, dO1 is written whole.
// ---------------------------------------------------------------------------------------------------
struct ConvRouteArgs { const float *part, *P1; const uint8_t* st1; float* dO1; long long n; int splits; };

template <int ACT, bool ENS> __global__ void __launch_bounds__(ELT_THREADS) conv_route1_kernel(ConvRouteArgs a, const int B) {
    if constexpr (ENS) {                       // member blockIdx.y of part [M][splits][n], P1 / st1 / dO1 [M, B, .]; a.n: ONE member's elements
        const long long mem = blockIdx.y, pt = mem * B;
        a.part += mem * a.splits * a.n; a.P1 += pt * P1SZ; a.st1 += pt * P1SZ; a.dO1 += pt * C1 * NO1;
    }
    const long long e = (long long)blockIdx.x * ELT_THREADS + threadIdx.x;
    if (e >= a.n) return;
    double s = 0.0;
    for (int sp = 0; sp < a.splits; ++sp) s += (double)a.part[(long long)sp * a.n + e];
    const int ci = (int)(e & (C1 - 1));
    const long long m = e >> 5;
    const int b = (int)(m / PP1), pp = (int)(m - (long long)b * PP1);
    const long long at = (long long)b * P1SZ + ci * PP1 + pp;
    const int st = a.st1[at];
    float d;
    if (smooth_act<ACT>()) d = act_grad_from_value<ACT>(a.P1[at]);
    else d = (st & 4) ? 1.f : act_neg_slope<ACT>();
    const float v = (float)s * d;
    float* const o = a.dO1 + ((long long)b * C1 + ci) * NO1 + (2 * (pp / P1W)) * O1W + 2 * (pp % P1W);
#pragma unroll
    for (int q = 0; q < 4; ++q) o[(q >> 1) * O1W + (q & 1)] = (st & 3) == q ? v : 0.f;
}

// ---------------------------------------------------------------------------------------------------
// The slices' partial sums -> grad: one thread per element of dK2 | dK2b and of dK1 | dK1b, slices in increasing order, fp64.
// ---------------------------------------------------------------------------------------------------
struct ConvRedArgs { const float *part2, *part1; float* grad; int Hc, s2, s1; long long oK2w, oK2b; };

__global__ void __launch_bounds__(ELT_THREADS) conv_reduce_kernel(const ConvRedArgs a) {
    long long e = (long long)blockIdx.x * ELT_THREADS + threadIdx.x;
    const long long n2 = (long long)a.Hc * N2;
    if (e < n2) {
        const int m = (int)(e / N2), n = (int)(e - (long long)m * N2);
        double s = 0.0;
        for (int sp = 0; sp < a.s2; ++sp) s += (double)a.part2[(long long)sp * n2 + e];
        a.grad[n < K2 ? a.oK2w + (long long)m * K2 + n : a.oK2b + m] = (float)s;
        return;
    }
    e -= n2;
    if (e >= C1 * N1) return;
    const int m = (int)e / N1, n = (int)e - m * N1;
    double s = 0.0;
    for (int sp = 0; sp < a.s1; ++sp) s += (double)a.part1[(long long)sp * (C1 * N1) + e];
    a.grad[n < 25 ? m * 25 + n : C1 * 25 + m] = (float)s;
}

// The same sums for member blockIdx.y of part2 [M][s2][Hc, 801] and part1 [M][s1][32, 26], into the member's rows of the tensor-major blocks of
// grad (oK1b, oK2w, oK2b: the starts of the blocks; model.0.weight's is 0).
struct ConvEnsRedArgs { const float *part2, *part1; float* grad; int Hc, s2, s1; long long oK1b, oK2w, oK2b; };

__global__ void __launch_bounds__(ELT_THREADS) conv_ens_reduce_kernel(const ConvEnsRedArgs a) {
    long long e = (long long)blockIdx.x * ELT_THREADS + threadIdx.x;
    const long long mem = blockIdx.y, n2 = (long long)a.Hc * N2;
    if (e < n2) {
        const int m = (int)(e / N2), n = (int)(e - (long long)m * N2);
        const float* const part = a.part2 + mem * a.s2 * n2;
        double s = 0.0;
        for (int sp = 0; sp < a.s2; ++sp) s += (double)part[(long long)sp * n2 + e];
        a.grad[n < K2 ? a.oK2w + (mem * a.Hc + m) * K2 + n : a.oK2b + mem * a.Hc + m] = (float)s;
        return;
    }
    e -= n2;
    if (e >= C1 * N1) return;
    const int m = (int)e / N1, n = (int)e - m * N1;
    const float* const part = a.part1 + mem * a.s1 * (C1 * N1);
    double s = 0.0;
    for (int sp = 0; sp < a.s1; ++sp) s += (double)part[(long long)sp * (C1 * N1) + e];
    a.grad[n < 25 ? (mem * C1 + m) * 25 + n : a.oK1b + mem * C1 + m] = (float)s;
}

// ---------------------------------------------------------------------------------------------------
// The members' batches out of the resident data: one block per packed point (member m, point b).  Row rows[m, b] of X [n_rows, ldx], clamped
// to [0, n_rows) (the fc trainers' rule: a bad index reads a wrong row, never outside X), goes to Xs [M * B, 784] in 16-byte pieces, its
// label to labels [M * B].  No kernel after this one sees rows.
// ---------------------------------------------------------------------------------------------------
struct ConvEnsStageArgs { const float* X; const int32_t *labels, *rows; float* Xs; int32_t* labels_out; int ldx, n_rows; };

__global__ void __launch_bounds__(256) conv_ens_stage_kernel(const ConvEnsStageArgs a) {
    const long long pt = blockIdx.x;
    const int t = threadIdx.x, row = min(max(a.rows[pt], 0), a.n_rows - 1);
    if (t < DIN / 4) *(f32x4*)(a.Xs + pt * DIN + 4 * t) = *(const f32x4*)(a.X + (long long)row * a.ldx + 4 * t);
    if (t == 0) a.labels_out[pt] = a.labels[row];
}

inline int check_conv_net(const rbnn_conv_train_net* n) {
    return n ? check_conv_dims(n->activation, n->in_channels, n->in_width, n->hidden, n->n_classes) : RBNN_ERR_NULL;
}

inline int check_conv_batch(const float* X, int ldx, int B) {
    if (!X) return RBNN_ERR_NULL;
    if (B < 1 || B > MAX_POINTS || ldx < DIN || (ldx & 3)) return RBNN_ERR_SHAPE;
    return aligned16(X) ? RBNN_OK : RBNN_ERR_ALIGN;
}

// the same tiles and slices for every member (grid dimension z): member m's operands at A + m a_mem, Bsrc + m b_mem, its slices at out + m o_mem
template <int MODE, bool ENS>
int wg_launch(const WgArgs& g, int splits, int members, long long a_mem, long long b_mem, long long o_mem, hipStream_t st) {
    constexpr int TN = MODE == G_DP1 ? 32 : 64;
    const int tiles = ((g.M + GT - 1) / GT) * ((g.N + TN - 1) / TN);
    hipLaunchKernelGGL((conv_wgrad_gemm_kernel<MODE, ENS>), dim3(tiles, splits, members), dim3(256), 0, st, g, a_mem, b_mem, o_mem);
    return launch_status();
}

// ---------------------------------------------------------------------------------------------------
// M members in lockstep.  The flat buffers are TENSOR-MAJOR: six blocks [M, size of tensor t] in state_dict order, so block t starts at M times
// the single net's offset and member m's tensor at + m * size — the layout of rbnn_conv_posterior's stacks (K1w [S][32][25], ..., Fb [S][C]):
// the exact forward addresses member m as sample m.  Every block start and every member's K2w / K2b / Fw is 16-byte aligned (Hc % 16 == 0).
// ---------------------------------------------------------------------------------------------------
constexpr int MAX_MEMBERS = 65535;                                                               // the member is a grid dimension (y or z)
constexpr long long MAX_ENS_POINTS = 1LL << 22;                                                  // M B: every packed index stays far inside 32 bits of blocks

inline ConvLayout conv_ens_layout(int Hc, int C, int M) {
    ConvLayout L = conv_layout(Hc, C);
    L.K1w *= M; L.K1b *= M; L.K2w *= M; L.K2b *= M; L.Fw *= M; L.Fb *= M; L.n_params *= M;
    return L;
}

inline int check_conv_ens_net(const rbnn_conv_ens_net* n) {
    if (!n) return RBNN_ERR_NULL;
    const int rc = check_conv_dims(n->activation, n->in_channels, n->in_width, n->hidden, n->n_classes);
    if (rc) return rc;
    return (n->n_members < 1 || n->n_members > MAX_MEMBERS) ? RBNN_ERR_SHAPE : RBNN_OK;
}

inline int check_conv_ens_points(const rbnn_conv_ens_net* n, int B) {
    return (B < 1 || B > MAX_POINTS || (long long)n->n_members * B > MAX_ENS_POINTS) ? RBNN_ERR_SHAPE : RBNN_OK;
}

// the five shape fields every conv net descriptor starts with
template <class To, class From> inline void copy_conv_shape(To& to, const From& from) {
    to.activation = from.activation; to.in_channels = from.in_channels; to.in_width = from.in_width; to.hidden = from.hidden;
    to.n_classes = from.n_classes;
}

// the n_stored nets of a flat buffer (L: conv_layout for one, conv_ens_layout for a tensor-major stack) as the forward's posterior
template <class Net> inline rbnn_conv_posterior conv_posterior_of(const Net& shape, const float* base, const ConvLayout& L, int n_stored) {
    rbnn_conv_posterior p = {};
    copy_conv_shape(p, shape);
    p.n_stored = n_stored;
    p.K1w = base + L.K1w; p.K1b = base + L.K1b; p.K2w = base + L.K2w; p.K2b = base + L.K2b; p.Fw = base + L.Fw; p.Fb = base + L.Fb;
    return p;
}

// the head over the n points of ws->logits (a workspace of either form): the training forwards' last launch
template <class Ws> inline int launch_conv_head(const Ws* ws, const int32_t* labels, int n, int C, float dz_scale, void* stream) {
    const ConvHeadArgs h = {ws->logits, labels, ws->dZ, ws->ce, ws->correct, n, C, dz_scale};
    hipLaunchKernelGGL(conv_head_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, h);
    return launch_status();
}

// what the weight gradients read and write of a workspace, of either form
template <class Ws> inline bool wg_buffers(const Ws* ws) {
    return ws && ws->P1 && ws->st1 && ws->Q2 && ws->st2 && ws->dZ && ws->dO2 && ws->dO1 && ws->part2 && ws->part1 && ws->partP;
}

// The seven launches of the weight gradients, after the entry point's checks.  ENS = false is the single net: M = 1, L = conv_layout, X the
// caller's batch.  ENS = true is M members in lockstep: L = conv_ens_layout, X = ws->Xs with ldx = 784, every array packed [M, B, .], the
// member a grid dimension (y; the conv GEMMs: z) and the partial sums [M][slices][...].  The single net's kernels read no member stride.
template <bool ENS, class Net, class Ws>
int conv_weight_grads(const Net* net, int M, const ConvLayout& L, const float* X, int ldx, int B, const Ws* ws, hipStream_t st) {
    const int Hc = net->hidden, C = net->n_classes;
    const long long F = (long long)Hc * NP2;
    float* const G = net->grad;
    // dFw | dFb: the strided GEMM, its member form with the member as grid dimension y
    GemmArgs ga = {};
    ga.n_prob = 1;
    ga.p[0] = wgrad_prob(ws->dZ, RBNN_CPAD, ws->Q2, F, (long long)B * F, C, (int)F, B, G + L.Fw, G + L.Fb, 0);
    ga.p[0].c_mem = (long long)C * F;
    ga.p[0].bias_mem = C;
    int rc = gemm_launch<ENS>(ga, M, st);
    if (rc) return rc;
    // dO2
    const ConvDo2Args d = {ws->dZ, net->P + L.Fw, ws->Q2, ws->st2, ws->dO2, Hc, C};
    rc = for_activation(net->activation, [&](auto a) {
        hipLaunchKernelGGL((conv_do2_kernel<decltype(a)::value, ENS>), dim3((unsigned)B * (Hc / 4), M), dim3(256), 0, st, d, B);
        return launch_status();
    });
    if (rc) return rc;
    // dP1 = conv2^T(dO2) per slice of the channels, then dO1 through pool 1
    int perP, sP;
    dp1_slices(B, Hc, perP, sP);
    const long long nP = (long long)B * PP1 * C1, dO2_mem = (long long)B * Hc * NPOS;
    WgArgs g = {};
    g.Hc = Hc; g.ldx = ldx;
    g.A = ws->dO2; g.Bsrc = net->P + L.K2w; g.out = ws->partP;
    g.M = B * PP1; g.N = C1; g.K = Hc * 25; g.kc = perP * 400;
    if ((rc = wg_launch<G_DP1, ENS>(g, sP, M, dO2_mem, (long long)Hc * K2, sP * nP, st))) return rc;
    const ConvRouteArgs ro = {ws->partP, ws->P1, ws->st1, ws->dO1, nP, sP};
    rc = for_activation(net->activation, [&](auto a) {
        hipLaunchKernelGGL((conv_route1_kernel<decltype(a)::value, ENS>), dim3(blocks_for(ro.n), M), dim3(ELT_THREADS), 0, st, ro, B);
        return launch_status();
    });
    if (rc) return rc;
    // the two split contractions and their reduction
    int per2, s2, per1, s1;
    slices(B, MAX_SPLITS2, per2, s2);
    slices(B, MAX_SPLITS1, per1, s1);
    g.A = ws->dO2; g.Bsrc = ws->P1; g.out = ws->part2; g.M = Hc; g.N = N2; g.K = B * NPOS; g.kc = per2 * NPOS;
    if ((rc = wg_launch<G_DK2, ENS>(g, s2, M, dO2_mem, (long long)B * P1SZ, (long long)s2 * Hc * N2, st))) return rc;
    g.A = ws->dO1; g.Bsrc = X; g.out = ws->part1; g.M = C1; g.N = N1; g.K = B * NO1; g.kc = per1 * NO1;
    if ((rc = wg_launch<G_DK1, ENS>(g, s1, M, (long long)B * C1 * NO1, (long long)B * ldx, (long long)s1 * C1 * N1, st))) return rc;
    const dim3 red(blocks_for((long long)Hc * N2 + C1 * N1), M);
    if constexpr (ENS) {
        const ConvEnsRedArgs r = {ws->part2, ws->part1, G, Hc, s2, s1, L.K1b, L.K2w, L.K2b};
        hipLaunchKernelGGL(conv_ens_reduce_kernel, red, dim3(ELT_THREADS), 0, st, r);
    } else {                                                               // a kernel of its own: folded into one template, its code changed
        const ConvRedArgs r = {ws->part2, ws->part1, G, Hc, s2, s1, L.K2w, L.K2b};
        hipLaunchKernelGGL(conv_reduce_kernel, red, dim3(ELT_THREADS), 0, st, r);
    }
    return launch_status();
}

// torch.optim.Adam on a whole flat buffer of n_params elements (element-wise: the members of a lockstep buffer share t and lr): 1 launch
template <class Net> int conv_adam_step(const Net* net, long long n_params, int64_t step, double lr, double beta1, double beta2, double adam_eps,
                                        void* stream) {
    if (!net->P || !net->m || !net->v || !net->grad) return RBNN_ERR_NULL;
    if (step < 1) return RBNN_ERR_SHAPE;
    AdamArgs a = {};
    a.n_params = n_params;
    a.P = net->P; a.m = net->m; a.v = net->v; a.grad = net->grad;
    a.s = adam_scalars(step, lr, beta1, beta2, adam_eps);
    hipLaunchKernelGGL(nn_adam_kernel<false>, dim3(blocks_for(a.n_params)), dim3(ELT_THREADS), 0, (hipStream_t)stream, a);
    return launch_status();
}

// ---------------------------------------------------------------------------------------------------
// K SVI guides in lockstep: what joins the members' forward and weight gradients above to the SVI step.  Tensor-major buffers: guide k's segment
// sg of a [K n_params] buffer starts at K sg.off + k sg.cols (svi::TensorMajor; every conv segment is one row of sg.cols columns), and the draw,
// Adam + KL (launched from rbnn_svi.hip) and finalize kernels are rbnn_svi_step.hpp's on that view.  Each returns at once, the whole block, for a guide with active[k] == 0.
// ---------------------------------------------------------------------------------------------------
constexpr int ACC_S = RBNN_SVI_MULTI_ACC_SAMPLES;

// Psum[k, b, :] = sum_s P[k ACC_S + s, b, :], one thread per (point, 4-class quad) of guide blockIdx.y, s = 0, 1, ... in that order: the sum
// reduce_samples_kernel (rbnn_kernels.hip) makes with scale 1.
struct ConvSvilsAccSumArgs { const float* P; const int32_t* active; float* Psum; int B, C; };

__global__ void __launch_bounds__(ELT_THREADS) conv_svils_acc_sum_kernel(const ConvSvilsAccSumArgs a) {
    const int k = blockIdx.y, i = blockIdx.x * ELT_THREADS + threadIdx.x;
    if (a.active[k] == 0 || i >= a.B * 4) return;
    const int b = i >> 2, q = i & 3;
    f32x4 sum = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < ACC_S; ++s) sum += *(const f32x4*)(a.P + (((long long)k * ACC_S + s) * a.B + b) * RBNN_CPAD + 4 * q);
#pragma unroll
    for (int r = 0; r < 4; ++r) if (4 * q + r < a.C) a.Psum[((long long)k * a.B + b) * RBNN_CPAD + 4 * q + r] = sum[r];
}

inline int check_conv_svils_points(const rbnn_conv_svi_guides_net* n, int B) {
    return (B < 1 || B > MAX_POINTS || (long long)n->n_guides * B > MAX_ENS_POINTS) ? RBNN_ERR_SHAPE : RBNN_OK;
}

// the guides as the members of rbnn_conv_ens_*: P = the drawn W, grad = dCE/dW, the first fifteen workspaces
inline rbnn_conv_ens_net conv_svils_members(const rbnn_conv_svi_guides_net* n) {
    rbnn_conv_ens_net e = {};
    copy_conv_shape(e, *n);
    e.n_members = n->n_guides; e.P = n->W; e.grad = n->grad;
    return e;
}
inline rbnn_conv_ens_ws conv_svils_member_ws(const rbnn_conv_svi_guides_ws* w) {
    rbnn_conv_ens_ws e = {};
    e.Xs = w->Xs; e.labels = w->labels; e.logits = w->logits; e.P1 = w->P1; e.st1 = w->st1; e.Q2 = w->Q2; e.st2 = w->st2; e.dZ = w->dZ; e.ce = w->ce;
    e.correct = w->correct; e.dO2 = w->dO2; e.dO1 = w->dO1; e.part2 = w->part2; e.part1 = w->part1; e.partP = w->partP;
    return e;
}

}  // namespace

extern "C" {

int rbnn_conv_train_sizes(const rbnn_conv_train_net* net, int32_t n_points, rbnn_conv_train_bytes* out) {
    const int rc = check_conv_net(net);
    if (rc) return rc;
    if (!out) return RBNN_ERR_NULL;
    if (n_points < 1 || n_points > MAX_POINTS) return RBNN_ERR_SHAPE;
    const size_t B = (size_t)n_points, Hc = (size_t)net->hidden, F = Hc * NP2;
    rbnn_conv_train_bytes z = {};
    z.n_params = conv_layout(net->hidden, net->n_classes).n_params;
    z.logits = z.dZ = B * RBNN_CPAD * sizeof(float);
    z.P1 = B * (size_t)GeoMnist::P1STRIDE;
    z.st1 = B * P1SZ;
    z.Q2 = B * F * sizeof(float);
    z.st2 = B * F;
    z.ce = B * sizeof(float);
    z.correct = B * sizeof(int32_t);
    z.dO2 = B * Hc * NPOS * sizeof(float);
    z.dO1 = B * C1 * NO1 * sizeof(float);
    z.part2 = (size_t)(n_points < MAX_SPLITS2 ? n_points : MAX_SPLITS2) * Hc * N2 * sizeof(float);
    z.part1 = (size_t)(n_points < MAX_SPLITS1 ? n_points : MAX_SPLITS1) * C1 * N1 * sizeof(float);
    z.partP = dp1_part_floats(n_points, net->hidden) * sizeof(float);
    *out = z;
    return RBNN_OK;
}

// The training forward and the head on net->P.  dz_scale multiplies dZ = softmax - e_y: 1 / B for the mean cross-entropy of the deterministic
// trainer, 1 for the summed one of the SVI step.
static int train_forward(const rbnn_conv_train_net* net, const float* X, int32_t ldx, const int32_t* labels, int32_t n_points,
                         const rbnn_conv_train_ws* ws, float dz_scale, void* stream) {
    int rc = check_conv_net(net);
    if (rc) return rc;
    if (!net->P || !labels || !ws || !ws->logits || !ws->P1 || !ws->st1 || !ws->Q2 || !ws->st2 || !ws->dZ || !ws->ce || !ws->correct) return RBNN_ERR_NULL;
    if ((rc = check_conv_batch(X, ldx, n_points))) return rc;
    if (!aligned16(net->P)) return RBNN_ERR_ALIGN;
    const rbnn_conv_posterior p = conv_posterior_of(*net, net->P, conv_layout(net->hidden, net->n_classes), 1);
    rbnn_conv_workspace w = {};
    w.P = ws->logits; w.P1 = ws->P1; w.st1 = ws->st1; w.Q2 = ws->Q2; w.st2 = ws->st2;
    if ((rc = rbnn_conv_forward(&p, X, ldx, n_points, nullptr, 1, RBNN_OUT_LOGITS, &w, stream))) return rc;
    return launch_conv_head(ws, labels, n_points, net->n_classes, dz_scale, stream);
}

int rbnn_conv_train_forward(const rbnn_conv_train_net* net, const float* X, int32_t ldx, const int32_t* labels, int32_t n_points,
                            const rbnn_conv_train_ws* ws, void* stream) {
    return train_forward(net, X, ldx, labels, n_points, ws, 1.f / (float)n_points, stream);       // (refused before it is used when n_points < 1)
}

int rbnn_conv_weight_grads(const rbnn_conv_train_net* net, const float* X, int32_t ldx, int32_t n_points, const rbnn_conv_train_ws* ws,
                           void* stream) {
    int rc = check_conv_net(net);
    if (rc) return rc;
    if (!net->P || !net->grad || !wg_buffers(ws)) return RBNN_ERR_NULL;
    if ((rc = check_conv_batch(X, ldx, n_points))) return rc;
    return conv_weight_grads<false>(net, 1, conv_layout(net->hidden, net->n_classes), X, ldx, n_points, ws, (hipStream_t)stream);
}

int rbnn_conv_adam_step(const rbnn_conv_train_net* net, int64_t step, double lr, double beta1, double beta2, double adam_eps, void* stream) {
    const int rc = check_conv_net(net);
    if (rc) return rc;
    return conv_adam_step(net, conv_layout(net->hidden, net->n_classes).n_params, step, lr, beta1, beta2, adam_eps, stream);
}

int rbnn_conv_train_finalize(const rbnn_conv_train_ws* ws, int32_t n_points, double* stats, void* stream) {
    if (!ws || !ws->ce || !ws->correct || !stats) return RBNN_ERR_NULL;
    if (n_points < 1 || n_points > MAX_POINTS) return RBNN_ERR_SHAPE;
    const FinalArgs a = {ws->ce, ws->correct, stats, n_points};
    hipLaunchKernelGGL(nn_finalize_kernel<false>, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status();
}

// ---------------------------------------------------------------------------------------------------
// The step of M members in lockstep: the launches of the single net's step with the member as a grid dimension, on batches packed [M, B, .].
// Member m's sums are the single net's in the single net's order (the slice counts are functions of B and Hc alone).
// ---------------------------------------------------------------------------------------------------
int rbnn_conv_ens_sizes(const rbnn_conv_ens_net* net, int32_t n_points, rbnn_conv_ens_bytes* out) {
    int rc = check_conv_ens_net(net);
    if (rc) return rc;
    if (!out) return RBNN_ERR_NULL;
    if ((rc = check_conv_ens_points(net, n_points))) return rc;
    rbnn_conv_train_net one = {};
    copy_conv_shape(one, *net);
    rbnn_conv_train_bytes s;
    if ((rc = rbnn_conv_train_sizes(&one, n_points, &s))) return rc;
    const size_t M = (size_t)net->n_members;
    rbnn_conv_ens_bytes z = {};
    z.n_params = s.n_params;
    z.Xs = M * n_points * DIN * sizeof(float);
    z.labels = M * n_points * sizeof(int32_t);
    z.logits = M * s.logits; z.P1 = M * s.P1; z.st1 = M * s.st1; z.Q2 = M * s.Q2; z.st2 = M * s.st2; z.dZ = M * s.dZ; z.ce = M * s.ce;
    z.correct = M * s.correct; z.dO2 = M * s.dO2; z.dO1 = M * s.dO1; z.part2 = M * s.part2; z.part1 = M * s.part1; z.partP = M * s.partP;
    *out = z;
    return RBNN_OK;
}

int rbnn_conv_ens_stage(const rbnn_conv_ens_net* net, const float* X, int32_t ldx, int32_t n_rows, const int32_t* labels, const int32_t* rows,
                        int32_t n_points, const rbnn_conv_ens_ws* ws, void* stream) {
    int rc = check_conv_ens_net(net);
    if (rc) return rc;
    if (!X || !labels || !rows || !ws || !ws->Xs || !ws->labels) return RBNN_ERR_NULL;
    if ((rc = check_conv_ens_points(net, n_points))) return rc;
    if (n_rows < 1 || ldx < DIN || (ldx & 3)) return RBNN_ERR_SHAPE;
    if (!aligned16(X) || !aligned16(ws->Xs)) return RBNN_ERR_ALIGN;
    const ConvEnsStageArgs a = {X, labels, rows, ws->Xs, ws->labels, ldx, n_rows};
    hipLaunchKernelGGL(conv_ens_stage_kernel, dim3((unsigned)(net->n_members * n_points)), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status();
}

// The members' training forward and the head.  dZ = (softmax - e_y) / B for the mean cross-entropy of the deterministic members, softmax - e_y
// (summed) for the summed one of the SVI guides in lockstep.
static int ens_forward(const rbnn_conv_ens_net* net, int32_t n_points, const rbnn_conv_ens_ws* ws, bool summed, void* stream) {
    int rc = check_conv_ens_net(net);
    if (rc) return rc;
    if (!net->P || !ws || !ws->Xs || !ws->labels || !ws->logits || !ws->P1 || !ws->st1 || !ws->Q2 || !ws->st2 || !ws->dZ || !ws->ce || !ws->correct)
        return RBNN_ERR_NULL;
    if ((rc = check_conv_ens_points(net, n_points))) return rc;
    if (!aligned16(net->P)) return RBNN_ERR_ALIGN;
    const int M = net->n_members;
    const rbnn_conv_posterior p = conv_posterior_of(*net, net->P, conv_ens_layout(net->hidden, net->n_classes, M), M);
    if ((rc = validate_conv(&p))) return rc;
    rbnn_conv_workspace w = {};
    w.P = ws->logits; w.P1 = ws->P1; w.st1 = ws->st1; w.Q2 = ws->Q2; w.st2 = ws->st2;
    ConvArgs a = {};
    if ((rc = conv_forward_args(&p, p.K2w, true, ws->Xs, DIN, n_points, nullptr, M, RBNN_OUT_LOGITS, &w, a))) return rc;
    if ((rc = launch_conv_forward_packed(net->activation, a, (hipStream_t)stream))) return rc;
    return launch_conv_head(ws, ws->labels, M * n_points, net->n_classes, summed ? 1.f : 1.f / (float)n_points, stream);
}

int rbnn_conv_ens_forward(const rbnn_conv_ens_net* net, int32_t n_points, const rbnn_conv_ens_ws* ws, void* stream) {
    return ens_forward(net, n_points, ws, false, stream);
}

int rbnn_conv_ens_weight_grads(const rbnn_conv_ens_net* net, int32_t n_points, const rbnn_conv_ens_ws* ws, void* stream) {
    int rc = check_conv_ens_net(net);
    if (rc) return rc;
    if (!net->P || !net->grad || !wg_buffers(ws) || !ws->Xs) return RBNN_ERR_NULL;
    if ((rc = check_conv_ens_points(net, n_points))) return rc;
    const int M = net->n_members;
    return conv_weight_grads<true>(net, M, conv_ens_layout(net->hidden, net->n_classes, M), ws->Xs, DIN, n_points, ws, (hipStream_t)stream);
}

int rbnn_conv_ens_adam_step(const rbnn_conv_ens_net* net, int64_t step, double lr, double beta1, double beta2, double adam_eps, void* stream) {
    const int rc = check_conv_ens_net(net);
    if (rc) return rc;
    return conv_adam_step(net, conv_ens_layout(net->hidden, net->n_classes, net->n_members).n_params, step, lr, beta1, beta2, adam_eps, stream);
}

int rbnn_conv_ens_finalize(const rbnn_conv_ens_net* net, const rbnn_conv_ens_ws* ws, int32_t n_points, double* stats, void* stream) {
    int rc = check_conv_ens_net(net);
    if (rc) return rc;
    if (!ws || !ws->ce || !ws->correct || !stats) return RBNN_ERR_NULL;
    if ((rc = check_conv_ens_points(net, n_points))) return rc;
    const FinalArgs a = {ws->ce, ws->correct, stats, n_points};
    hipLaunchKernelGGL(nn_finalize_kernel<true>, dim3(net->n_members), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status();
}

// ---------------------------------------------------------------------------------------------------
// The SVI step of one conv guide.  The drawn sample W plays the deterministic net's P: the forward and the weight gradients above run on
// a view of the guide (P = W, grad = grad) and launch what they launch for the deterministic trainer.
// ---------------------------------------------------------------------------------------------------
static int conv_svi_view(const rbnn_conv_svi_train_net* g, rbnn_conv_train_net* v) {
    if (!g) return RBNN_ERR_NULL;
    *v = {};
    copy_conv_shape(*v, *g);
    v->P = g->W; v->grad = g->grad;
    return check_conv_net(v);
}

int rbnn_conv_svi_train_sizes(const rbnn_conv_svi_train_net* net, int32_t n_points, int64_t* n_partials, rbnn_conv_train_bytes* out) {
    rbnn_conv_train_net v;
    int rc = conv_svi_view(net, &v);
    if (rc) return rc;
    if ((rc = rbnn_conv_train_sizes(&v, n_points, out))) return rc;
    if (n_partials) *n_partials = blocks_for(conv_svi_layout(v.hidden, v.n_classes).n_quads);
    return RBNN_OK;
}

int rbnn_conv_svi_train_draw(const rbnn_conv_svi_train_net* net, uint64_t key, uint32_t draw_id, void* stream) {
    rbnn_conv_train_net v;
    const int rc = conv_svi_view(net, &v);
    if (rc) return rc;
    if (!net->loc || !net->sigma || !net->W) return RBNN_ERR_NULL;
    const Layout L = conv_svi_layout(v.hidden, v.n_classes);
    rbnn_svi_flat_tensor t[6] = {};
    for (int i = 0; i < 6; ++i) {
        const Seg& s = L.s[i];
        t[i].loc = net->loc + s.off; t[i].sigma = net->sigma + s.off; t[i].out = net->W + s.off;
        t[i].n_elem = t[i].out_sample_stride = s.cols; t[i].tensor_id = s.tensor_id;
    }
    return rbnn_svi_draw_flat(t, 6, 1, nullptr, key, draw_id, stream);
}

int rbnn_conv_svi_train_forward(const rbnn_conv_svi_train_net* net, const float* X, int32_t ldx, const int32_t* labels, int32_t n_points,
                                const rbnn_conv_train_ws* ws, void* stream) {
    rbnn_conv_train_net v;
    const int rc = conv_svi_view(net, &v);
    return rc ? rc : train_forward(&v, X, ldx, labels, n_points, ws, 1.f, stream);
}

int rbnn_conv_svi_weight_grads(const rbnn_conv_svi_train_net* net, const float* X, int32_t ldx, int32_t n_points, const rbnn_conv_train_ws* ws,
                               void* stream) {
    rbnn_conv_train_net v;
    const int rc = conv_svi_view(net, &v);
    return rc ? rc : rbnn_conv_weight_grads(&v, X, ldx, n_points, ws, stream);
}

int rbnn_conv_svi_adam_step(const rbnn_conv_svi_train_net* net, uint64_t key, uint32_t draw_id, int64_t step, double lr, double beta1,
                            double beta2, double adam_eps, float* kl_partials, void* stream) {
    rbnn_conv_train_net v;
    const int rc = conv_svi_view(net, &v);
    if (rc) return rc;
    if (!net->loc || !net->raw || !net->sigma || !net->m_loc || !net->v_loc || !net->m_raw || !net->v_raw || !net->grad || !kl_partials)
        return RBNN_ERR_NULL;
    if (step < 1) return RBNN_ERR_SHAPE;
    svi::AdamArgs a = {};
    a.L = conv_svi_layout(v.hidden, v.n_classes);
    a.loc = net->loc; a.raw = net->raw; a.sigma = net->sigma; a.m_loc = net->m_loc; a.v_loc = net->v_loc; a.m_raw = net->m_raw; a.v_raw = net->v_raw;
    a.grad = net->grad; a.kl_part = kl_partials; a.key = key; a.draw_id = draw_id;
    a.s = adam_scalars(step, lr, beta1, beta2, adam_eps);
    hipLaunchKernelGGL(svi::adam_kernel<svi::Single>, dim3(blocks_for(a.L.n_quads)), dim3(ELT_THREADS), 0, (hipStream_t)stream, a);
    return launch_status();
}

// ---------------------------------------------------------------------------------------------------
// The SVI step of K conv guides in lockstep: the members' stage / forward / weight gradients above on the view (P = W, grad = grad) with the
// summed cross-entropy, around the kernels of the guides (rbnn_conv_svi_guides_adam_step: rbnn_svi.hip).  Every refusal comes before the first launch of an entry point.
// ---------------------------------------------------------------------------------------------------
int rbnn_conv_svi_guides_sizes(const rbnn_conv_svi_guides_net* net, int32_t n_points, rbnn_conv_svi_guides_bytes* out) {
    int rc = check_conv_svils_net(net);
    if (rc) return rc;
    if (!out) return RBNN_ERR_NULL;
    if ((rc = check_conv_svils_points(net, n_points))) return rc;
    const rbnn_conv_ens_net e = conv_svils_members(net);
    rbnn_conv_ens_bytes s;
    if ((rc = rbnn_conv_ens_sizes(&e, n_points, &s))) return rc;
    const size_t KS = (size_t)net->n_guides * ACC_S, SN = KS * n_points, F = (size_t)net->hidden * NP2;
    rbnn_conv_svi_guides_bytes z = {};
    z.n_params = s.n_params;
    z.n_partials = blocks_for(conv_svi_layout(net->hidden, net->n_classes).n_quads);
    z.Xs = s.Xs; z.labels = s.labels; z.logits = s.logits; z.P1 = s.P1; z.st1 = s.st1; z.Q2 = s.Q2; z.st2 = s.st2; z.dZ = s.dZ; z.ce = s.ce;
    z.correct = s.correct; z.dO2 = s.dO2; z.dO1 = s.dO1; z.part2 = s.part2; z.part1 = s.part1; z.partP = s.partP;
    z.acc_W = KS * (size_t)s.n_params * sizeof(float);
    z.acc_P = SN * RBNN_CPAD * sizeof(float);                     // the accuracy forward's buffers: rbnn_conv_workspace_query's for K S samples
    z.acc_P1 = SN * (size_t)GeoMnist::P1STRIDE;
    z.acc_st1 = SN * P1SZ;
    z.acc_Q2 = SN * F * sizeof(float);
    z.acc_st2 = SN * F;
    z.Psum = (size_t)net->n_guides * n_points * RBNN_CPAD * sizeof(float);
    *out = z;
    return RBNN_OK;
}

int rbnn_conv_svi_guides_draw(const rbnn_conv_svi_guides_net* net, const int32_t* active, uint32_t draw_id, void* stream) {
    const int rc = check_conv_svils_net(net);
    if (rc) return rc;
    if (!active || !net->loc || !net->sigma || !net->W || !net->keys) return RBNN_ERR_NULL;
    return svi::guides_draw<svi::TensorMajor>(conv_svi_layout(net->hidden, net->n_classes), conv_svils_guides(net), net->W, active, net->n_guides, 1, 0,
                                              0, draw_id, (hipStream_t)stream);
}

int rbnn_conv_svi_guides_gradient(const rbnn_conv_svi_guides_net* net, const float* X, int32_t ldx, int32_t n_rows, const int32_t* labels,
                                 const int32_t* rows, int32_t n_points, const rbnn_conv_svi_guides_ws* ws, void* stream) {
    int rc = check_conv_svils_net(net);
    if (rc) return rc;
    if (!X || !labels || !rows || !ws || !net->W || !net->grad) return RBNN_ERR_NULL;
    const void* const bufs[] = {ws->Xs, ws->labels, ws->logits, ws->P1, ws->st1, ws->Q2, ws->st2, ws->dZ, ws->ce, ws->correct, ws->dO2, ws->dO1,
                                ws->part2, ws->part1, ws->partP};
    for (const void* b : bufs) if (!b) return RBNN_ERR_NULL;
    if ((rc = check_conv_svils_points(net, n_points))) return rc;
    if (n_rows < 1 || ldx < DIN || (ldx & 3)) return RBNN_ERR_SHAPE;
    if (!aligned16(X) || !aligned16(net->W) || !aligned16(net->grad)) return RBNN_ERR_ALIGN;
    for (const void* b : bufs) if (!aligned16(b)) return RBNN_ERR_ALIGN;
    // nothing below can refuse: the three calls repeat these checks on the member view
    const rbnn_conv_ens_net e = conv_svils_members(net);
    const rbnn_conv_ens_ws w = conv_svils_member_ws(ws);
    if ((rc = rbnn_conv_ens_stage(&e, X, ldx, n_rows, labels, rows, n_points, &w, stream))) return rc;
    if ((rc = ens_forward(&e, n_points, &w, true, stream))) return rc;
    return rbnn_conv_ens_weight_grads(&e, n_points, &w, stream);
}

int rbnn_conv_svi_guides_accuracy(const rbnn_conv_svi_guides_net* net, const int32_t* active, int32_t n_points, uint64_t key_xor, uint32_t draw_id,
                                 const rbnn_conv_svi_guides_ws* ws, void* stream) {
    int rc = check_conv_svils_net(net);
    if (rc) return rc;
    if (!active || !ws || !net->loc || !net->sigma || !net->keys) return RBNN_ERR_NULL;
    const void* const bufs[] = {ws->Xs, ws->acc_W, ws->acc_P, ws->acc_P1, ws->acc_st1, ws->acc_Q2, ws->acc_st2, ws->Psum};
    for (const void* b : bufs) if (!b) return RBNN_ERR_NULL;
    if ((rc = check_conv_svils_points(net, n_points))) return rc;
    for (const void* b : bufs) if (!aligned16(b)) return RBNN_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const int K = net->n_guides, KS = K * ACC_S;
    // the stack of the K S nets: tensor-major over the sets, so set k S + s is sample k S + s of an rbnn_conv_posterior
    float* const W = ws->acc_W;
    const rbnn_conv_posterior p = conv_posterior_of(*net, W, conv_ens_layout(net->hidden, net->n_classes, KS), KS);
    if ((rc = validate_conv(&p))) return rc;
    rbnn_conv_workspace w = {};
    w.P = ws->acc_P; w.P1 = ws->acc_P1; w.st1 = ws->acc_st1; w.Q2 = ws->acc_Q2; w.st2 = ws->acc_st2;
    ConvArgs c = {};
    if ((rc = conv_forward_args(&p, p.K2w, true, ws->Xs, DIN, n_points, nullptr, KS, RBNN_OUT_PROBS, &w, c))) return rc;
    if ((rc = svi::guides_draw<svi::TensorMajor>(conv_svi_layout(net->hidden, net->n_classes), conv_svils_guides(net), W, active, K, ACC_S, 0, key_xor,
                                                 draw_id, st)))
        return rc;
    if ((rc = launch_conv_forward_grouped(net->activation, c, st))) return rc;
    const ConvSvilsAccSumArgs r = {ws->acc_P, active, ws->Psum, n_points, net->n_classes};
    hipLaunchKernelGGL(conv_svils_acc_sum_kernel, dim3(blocks_for(4LL * n_points), K), dim3(ELT_THREADS), 0, st, r);
    return launch_status();
}

int rbnn_conv_svi_guides_finalize(const rbnn_conv_svi_guides_net* net, const int32_t* active, const rbnn_conv_svi_guides_ws* ws, int32_t with_accuracy,
                                 int32_t n_points, const int32_t* epoch_slot, double* epoch_log, int32_t log_rows, void* stream) {
    int rc = check_conv_svils_net(net);
    if (rc) return rc;
    if (!active || !ws || !ws->ce || !ws->labels || (with_accuracy && !ws->Psum) || !net->kl_part || !net->stats || (epoch_slot && !epoch_log))
        return RBNN_ERR_NULL;
    if ((rc = check_conv_svils_points(net, n_points))) return rc;
    svi::GuidesFinalArgs a = {};
    a.n_part = (int)blocks_for(conv_svi_layout(net->hidden, net->n_classes).n_quads);
    if (net->part_stride < a.n_part || log_rows < 0) return RBNN_ERR_SHAPE;
    a.kl_part = net->kl_part; a.ce = ws->ce; a.Psum = with_accuracy ? ws->Psum : nullptr; a.labels = ws->labels; a.live = active;
    a.epoch_slot = epoch_slot; a.stats = net->stats; a.epoch_log = epoch_log; a.part_stride = net->part_stride;
    a.B = n_points; a.C = net->n_classes; a.log_rows = log_rows;
    hipLaunchKernelGGL(svi::svils_finalize_kernel<false>, dim3(net->n_guides), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status();
}

// ---------------------------------------------------------------------------------------------------
// dCE/dW of K HMC chains in one set of launches: the members' stage / forward / weight gradients above on the view (P = W, grad = grad) with
// the summed cross-entropy.  No device code of its own; the chain's element-wise kernels are rbnn_hmc.hip's.  Every refusal comes before the
// first launch of an entry point.
// ---------------------------------------------------------------------------------------------------
static_assert(MAX_MEMBERS == CONV_MAX_CHAINS && MAX_POINTS == CONV_CHAINS_MAX_POINTS && MAX_ENS_POINTS == CONV_CHAINS_MAX_PACKED,
              "the chains are the members of the staging, the forward and the weight gradients");

static rbnn_conv_ens_net conv_chains_members(const rbnn_conv_hmc_chains_net* n) {
    rbnn_conv_ens_net e = {};
    copy_conv_shape(e, *n);
    e.n_members = n->n_chains; e.P = n->W; e.grad = n->grad;
    return e;
}

int64_t rbnn_conv_hmc_chains_sizes(const rbnn_conv_hmc_chains_net* net, int32_t n_points, int64_t* n_quad_partials, int64_t* n_elem_partials,
                                   rbnn_conv_ens_bytes* out) {
    int rc = check_conv_chains_net(net);
    if (rc) return rc;
    const Layout L = conv_svi_layout(net->hidden, net->n_classes);
    if (out) {
        const rbnn_conv_ens_net e = conv_chains_members(net);
        if ((rc = rbnn_conv_ens_sizes(&e, n_points, out))) return rc;
    }
    if (n_quad_partials) *n_quad_partials = blocks_for(L.n_quads);
    if (n_elem_partials) *n_elem_partials = blocks_for(L.n_params);
    return L.n_params;
}

int rbnn_conv_hmc_chains_stage(const rbnn_conv_hmc_chains_net* net, const float* X, int32_t ldx, int32_t n_rows, const int32_t* labels,
                               const int32_t* rows, int32_t n_points, const rbnn_conv_ens_ws* ws, void* stream) {
    const int rc = check_conv_chains_net(net);
    if (rc) return rc;
    const rbnn_conv_ens_net e = conv_chains_members(net);                  // rbnn_conv_ens_stage checks in the documented order and reads neither P nor grad
    return rbnn_conv_ens_stage(&e, X, ldx, n_rows, labels, rows, n_points, ws, stream);
}

int rbnn_conv_hmc_chains_gradient(const rbnn_conv_hmc_chains_net* net, int32_t n_points, const rbnn_conv_ens_ws* ws, void* stream) {
    int rc = check_conv_chains_net(net);
    if (rc) return rc;
    if (!ws || !net->W || !net->grad) return RBNN_ERR_NULL;
    const void* const bufs[] = {ws->Xs, ws->labels, ws->logits, ws->P1, ws->st1, ws->Q2, ws->st2, ws->dZ, ws->ce, ws->correct, ws->dO2, ws->dO1,
                                ws->part2, ws->part1, ws->partP};
    for (const void* b : bufs) if (!b) return RBNN_ERR_NULL;
    if ((rc = check_conv_chains_points(net, n_points))) return rc;
    if (!aligned16(net->W) || !aligned16(net->grad)) return RBNN_ERR_ALIGN;
    for (const void* b : bufs) if (!aligned16(b)) return RBNN_ERR_ALIGN;
    // nothing below can refuse: the two calls repeat these checks on the member view
    const rbnn_conv_ens_net e = conv_chains_members(net);
    if ((rc = ens_forward(&e, n_points, ws, true, stream))) return rc;
    return rbnn_conv_ens_weight_grads(&e, n_points, ws, stream);
}

}  // extern "C"
