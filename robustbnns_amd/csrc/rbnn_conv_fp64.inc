// rbnn_conv_fp64.inc — the fp64 checker of the conv forward and expected input gradient (included by rbnn_conv.hip).
//
// As rbnn_fp64.inc for fc / fc2: the data stay fp32 (K1w .. Fb, X, the attack iterates) and are widened on load, which is exact; every
// operation from the first product to the written result is fp64.  conv2 and conv2^T (98 % of the MACs) run on v_mfma_f64_16x16x4_f64
// with fp64 accumulators, conv1, conv1^T and the head are fp64 FMAs.  No atomics; every result element has one fixed accumulation
// order; one block = one (sample, point), so two runs are bit-identical and a point's result depends neither on N nor on the point
// block it ran in.  Lane maps of the f64 MFMA, the widening loads, act / act' and mfma64_drain: rbnn_fp64_common.hpp.
//
// Pooling: the activated values are compared (as torch does) and the FIRST maximum in row-major window order wins; its index 0..3 is the
// argmax byte.  act' is a function of the pooled VALUE for all four activations (y (1 - y), 1 - y^2, y > 0), so the argmax byte and
// P1 / Q2 are all the backward needs.
//
//   conv1_pool_fp64_kernel      Cin*25 FMAs per output (ci, ky, kx ascending), + bias, act, MaxPool 2        -> P1 [S][N][32][P1W][P1W], arg1
//   conv2_pool_fp64_kernel      implicit GEMM  O2[pos][hc] = sum_k P1[ci(k)][y + ky(k)][x + kx(k)] * W2[hc][k],  k = ci*25 + ky*5 + kx  (800):
//                               A = gathered from the point's P1 image in LDS, B = 16 W2 rows, 16 bytes = 4 K steps per lane;
//                               + bias, act, MaxPool 2 stride 1                                                  -> Q2 [S][N][Hc*NP2], arg2
//   conv_head_fp64_kernel       z[c] = sum_f Q2[f] * Fw[c][f] + Fb[c]: 16 interleaved chains (f = j, j + 16, ...) added in ascending j;
//                               softmax with the maximum subtracted, or logits                                  -> P [S][N][16]
//   conv_backward_fp64_body     the backward of both checkers, written once (a __device__ function; WGRAD picks the tail):
//                               dQ2 = Fw^T dZ (c ascending) * act'(Q2), routed through pool-2 in GATHER form (a conv2 output adds the <= 4
//                               windows that chose it, rows then columns ascending) into a zero-bordered image per 16 channels;
//                               conv2^T as  dP1[pos][ci] = sum_{k = (hc, tap)} dO2pad[hc][Y - ky + 4][X - kx + 4] * W2[hc][ci][tap]
//                               with all accumulators resident over K = Hc*25;  * act'(P1); then
//   conv_input_grad_fp64_kernel   (WGRAD off) pool-1 routing, conv1^T as a gather over (ci, ky, kx ascending)  -> Gs [S][N][Cin*W*W]
//   cwg_backward_dp_kernel        (WGRAD on, rbnn_conv_wgrad_dp.inc) the routed images themselves              -> dO2, dO1
//   conv_sum_samples_fp64_kernel  G[n][d] = scale * sum_s Gs[s][n][d], s ascending;   conv_norms_fp64_kernel: linf / l2 per row (row_norms64)
#include "rbnn_fp64_common.hpp"

namespace {

struct ConvFp64Args {
    const float* X; int ldx; int N;
    const float* K1w; const float* K1b; const float* K2w; const float* K2b; const float* Fw; const float* Fb;
    int Hc; int C; const int* sidx; int S;
    double* P1; uint8_t* arg1;                      // [S][N][32*P1W*P1W]
    double* Q2; uint8_t* arg2;                      // [S][N][Hc*NP2]
    double* P;  int out_kind;                       // [S][N][16]
    const double* dZ; double* Gs;                   // [S][N][16], [S][N][Cin*W*W]   (backward)
};

template <int ACT> __device__ __forceinline__ double act_deriv_value64(double y) { return act_deriv64<ACT>(y, y); }

// ---------------------------------------------------------------------------------------------------
// conv1 + pool: one block = one (sample, point); the image and the sample's 32 x Cin x 25 weights go to LDS in fp64, one thread per
// pooled output runs its four window positions in row-major order.
// ---------------------------------------------------------------------------------------------------
template <int ACT, class G>
__global__ void __launch_bounds__(256) conv1_pool_fp64_kernel(const ConvFp64Args a) {
    __shared__ double xs[G::DIN];
    __shared__ double ws[C1 * G::K1];
    constexpr int PP = G::P1W * G::P1W, II = G::IW * G::IW;
    const int tid = threadIdx.x;
    const long long sn = blockIdx.x;
    const int s = (int)(sn / a.N), n = (int)(sn - (long long)s * a.N);
    const int sw = a.sidx ? a.sidx[s] : s;
    const float* const x = a.X + (long long)n * a.ldx;
    const float* const w = a.K1w + (long long)sw * C1 * G::K1;
    for (int i = tid; i < G::DIN; i += 256) xs[i] = (double)x[i];
    for (int i = tid; i < C1 * G::K1; i += 256) ws[i] = (double)w[i];
    __syncthreads();
    for (int o = tid; o < G::P1SZ; o += 256) {
        const int c = o / PP, p = o - c * PP, py = p / G::P1W, px = p - py * G::P1W;
        const double bias = (double)a.K1b[(long long)sw * C1 + c];
        double best = 0.;
        int arg = 0;
        for (int q = 0; q < 4; ++q) {
            const double* const xq = xs + (2 * py + (q >> 1)) * G::IW + 2 * px + (q & 1);
            double acc = 0.;
            for (int ci = 0; ci < G::CIN; ++ci)
                for (int ky = 0; ky < 5; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 5; ++kx) acc = fma(xq[ci * II + ky * G::IW + kx], ws[c * G::K1 + ci * 25 + ky * 5 + kx], acc);
            const double v = act_fwd64<ACT>(acc + bias);
            if (q == 0 || v > best) { best = v; arg = q; }
        }
        a.P1[sn * G::P1SZ + o] = best;
        a.arg1[sn * G::P1SZ + o] = (uint8_t)arg;
    }
}

// ---------------------------------------------------------------------------------------------------
// conv2 + pool: one block (4 waves) = one (sample, point).  A wave owns 16 output channels at a time with ALL the point's conv2 positions
// (NPT2 = 4 / 7 accumulator tiles; rows past NPOS of the ragged last tile repeat the last position and are never stored), writes the
// activated outputs to its LDS tile and pools them from there.  Dynamic LDS: P1 image, 4 output tiles, the k -> offset table:
// 71 KiB at 1x28x28, 102 KiB at 3x32x32.
// ---------------------------------------------------------------------------------------------------
template <class G> constexpr int conv2_fp64_lds_bytes() { return (G::P1SZ + 4 * 16 * G::NPOS) * 8 + 800 * 4; }

template <int ACT, class G>
__global__ void __launch_bounds__(256) conv2_pool_fp64_kernel(const ConvFp64Args a) {
    extern __shared__ double lds64[];
    constexpr int PP = G::P1W * G::P1W, NPT = G::NPT2;
    double* const p1s = lds64;                                  // [32][P1W][P1W]
    double* const o2s = p1s + G::P1SZ;                          // [4 waves][16 hc][NPOS]
    int* const koff = (int*)(o2s + 4 * 16 * G::NPOS);           // [800]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
    const long long sn = blockIdx.x;
    const int s = (int)(sn / a.N);
    const int sw = a.sidx ? a.sidx[s] : s;
    const long long F = (long long)a.Hc * G::NP2;
    for (int i = tid; i < G::P1SZ; i += 256) p1s[i] = a.P1[sn * G::P1SZ + i];
    for (int k = tid; k < 800; k += 256) {
        const int ci = k / 25, t = k - ci * 25, ky = t / 5, kx = t - ky * 5;
        koff[k] = ci * PP + ky * G::P1W + kx;
    }
    __syncthreads();
    int pbase[NPT];
#pragma unroll
    for (int t = 0; t < NPT; ++t) {
        const int pos = min(t * 16 + li, G::NPOS - 1), y = pos / G::O2W, x = pos - y * G::O2W;
        pbase[t] = y * G::P1W + x;
    }
    const int tiles = a.Hc >> 4;
    for (int t0 = 0; t0 < tiles; t0 += 4) {
        const int ht = t0 + wave;
        const bool active = ht < tiles;                                     // (wave-uniform)
        if (active) {
            f64x4 acc[NPT];
#pragma unroll
            for (int t = 0; t < NPT; ++t) acc[t] = (f64x4){0., 0., 0., 0.};
            const float* const wrow = a.K2w + ((long long)sw * a.Hc + ht * 16 + li) * 800;
            for (int k0 = 0; k0 < 800; k0 += 16) {
                const int k = k0 + 4 * lg;
                const f64x4 bv = load4_f64(wrow + k);
                int off[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) off[r] = koff[k + r];
#pragma unroll
                for (int t = 0; t < NPT; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[t] = MFMA64(p1s[pbase[t] + off[r]], bv[r], acc[t]);
            }
            mfma64_drain(acc);
            // acc[t][r] = conv2 output at position t*16 + lg + 4*r, channel ht*16 + li, without its bias
            const double bias = (double)a.K2b[(long long)sw * a.Hc + ht * 16 + li];
#pragma unroll
            for (int t = 0; t < NPT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int pos = t * 16 + lg + 4 * r;
                    if (pos < G::NPOS) o2s[(wave * 16 + li) * G::NPOS + pos] = act_fwd64<ACT>(acc[t][r] + bias);
                }
        }
        __syncthreads();
        if (active) {
            for (int o = lane; o < 16 * G::NP2; o += 64) {
                const int h = o / G::NP2, p = o - h * G::NP2, py = p / G::P2W, px = p - py * G::P2W;
                const double* const w = o2s + (wave * 16 + h) * G::NPOS + py * G::O2W + px;
                const double v1 = w[1], v2 = w[G::O2W], v3 = w[G::O2W + 1];
                double best = w[0];
                int arg = 0;
                if (v1 > best) { best = v1; arg = 1; }
                if (v2 > best) { best = v2; arg = 2; }
                if (v3 > best) { best = v3; arg = 3; }
                const long long f = sn * F + (long long)(ht * 16 + h) * G::NP2 + p;
                a.Q2[f] = best;
                a.arg2[f] = (uint8_t)arg;
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------
// The head: one block = one (sample, point); thread (class c = tid >> 4, chain j = tid & 15).
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) conv_head_fp64_kernel(const ConvFp64Args a, int NP2) {
    __shared__ double zp[256];
    __shared__ double zl[16];
    const int tid = threadIdx.x, c = tid >> 4, j = tid & 15;
    const long long sn = blockIdx.x;
    const int s = (int)(sn / a.N);
    const int sw = a.sidx ? a.sidx[s] : s;
    const long long F = (long long)a.Hc * NP2;
    double acc = 0.;
    if (c < a.C) {
        const float* const fw = a.Fw + ((long long)sw * a.C + c) * F;
        const double* const q = a.Q2 + sn * F;
        for (long long f = j; f < F; f += 16) acc = fma(q[f], (double)fw[f], acc);
    }
    zp[tid] = acc;
    __syncthreads();
    if (tid < 16) {
        double z = 0.;
        if (tid < a.C) {
            for (int jj = 0; jj < 16; ++jj) z += zp[tid * 16 + jj];
            z += (double)a.Fb[(long long)sw * a.C + tid];
        }
        zl[tid] = z;
    }
    __syncthreads();
    if (tid < 16) {
        double out = zl[tid];
        if (a.out_kind == RBNN_OUT_PROBS) {
            double m = -INFINITY, den = 0.;
            for (int cc = 0; cc < a.C; ++cc) m = fmax(m, zl[cc]);
            for (int cc = 0; cc < a.C; ++cc) den += exp(zl[cc] - m);
            out = exp(out - m) / den;
        }
        a.P[sn * RBNN_CPAD + tid] = (tid < a.C) ? out : 0.;
    }
}

// ---------------------------------------------------------------------------------------------------
// The backward, one text for both of its kernels: one block (4 waves) = one (sample, point).  Wave w owns the P1-position tiles w, w + 4, ...
// (<= MT) x both ci tiles: <= 8 accumulator tiles that live through the whole K = Hc*25 loop.  Per chunk of 16 conv2 channels the block
// builds dQ2 * act' (stage 1), routes it through pool-2 into the interior of the zero-bordered image (stage 2) and runs 25 K blocks of 16.
// Rows past P1W*P1W of the ragged last tile repeat the last position and are never stored.  Behind the K loop dP1 * act'(P1) goes to LDS and
//   WGRAD = false (conv_input_grad_fp64_kernel, ConvFp64Args): pool-1 routing + conv1^T as a gather over the sample's K1 in LDS -> Gs;
//   WGRAD = true  (cwg_backward_dp_kernel of rbnn_conv_wgrad_dp.inc, CwgDpArgs): stage 2 also writes the chunk's routed image to dO2, and the
//                 tail routes dP1 through pool-1 into dO1; K1 is neither loaded nor given room.
// Dynamic LDS: 88 KiB at 1x28x28, 128 KiB at 3x32x32; with WGRAD 82 KiB and 109 KiB.
// ---------------------------------------------------------------------------------------------------
template <class G, bool WGRAD = false> struct BwdFp64Lds {
    static constexpr int PB = G::O2W + 8;                                   // pitch of the image: the gradients with a border of 4
    static constexpr int IMG = 16 * PB * PB, DQ = 16 * G::NP2, K1N = WGRAD ? 0 : C1 * G::K1;
    static constexpr int DOUBLES = IMG + DQ + 16 + G::P1SZ + K1N;
    static constexpr int BYTES = DOUBLES * 8 + 2 * 400 * 4 + G::P1SZ;
};

template <int ACT, class G, bool WGRAD, class Args>
__device__ __forceinline__ void conv_backward_fp64_body(const Args a) {
    extern __shared__ double lds64[];
    using L = BwdFp64Lds<G, WGRAD>;
    constexpr int PB = L::PB, PP = G::P1W * G::P1W, MT = (G::NPT1 + 3) / 4;
    double* const dpad = lds64;                                 // [16 hc][PB][PB]
    double* const dq = dpad + L::IMG;                           // [16 hc][NP2]
    double* const dzs = dq + L::DQ;                             // [16]
    double* const dp1 = dzs + 16;                               // [32][P1W][P1W]: dL/d(conv1 pre-activation at the window's argmax)
    double* const k1 = dp1 + G::P1SZ;                           // [32][Cin*25]  (no room with WGRAD)
    int* const tab_a = (int*)(k1 + L::K1N);                     // [400] k = hl*25 + tap -> offset into the image relative to (Y + 4, X + 4)
    int* const tab_w = tab_a + 400;                             // [400] -> offset into W2 relative to [hc0][ci]
    uint8_t* const a1s = (uint8_t*)(tab_w + 400);               // [32][P1W][P1W]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
    const long long sn = blockIdx.x;
    const int s = (int)(sn / a.N);
    const int sw = a.sidx ? a.sidx[s] : s;
    const long long F = (long long)a.Hc * G::NP2;

    if (tid < 16) dzs[tid] = (tid < a.C) ? a.dZ[sn * RBNN_CPAD + tid] : 0.;
    for (int i = tid; i < L::IMG; i += 256) dpad[i] = 0.;
    if constexpr (!WGRAD)
        for (int i = tid; i < L::K1N; i += 256) k1[i] = (double)a.K1w[(long long)sw * L::K1N + i];
    for (int i = tid; i < G::P1SZ; i += 256) a1s[i] = a.arg1[sn * G::P1SZ + i];
    for (int k = tid; k < 400; k += 256) {
        const int hl = k / 25, tap = k - hl * 25, ky = tap / 5, kx = tap - ky * 5;
        tab_a[k] = hl * PB * PB - ky * PB - kx;
        tab_w[k] = hl * 800 + tap;
    }
    int abase[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int pos = min((wave + 4 * m) * 16 + li, PP - 1), Y = pos / G::P1W, X = pos - Y * G::P1W;
        abase[m] = (Y + 4) * PB + X + 4;
    }
    f64x4 acc[MT * 2];
#pragma unroll
    for (int t = 0; t < MT * 2; ++t) acc[t] = (f64x4){0., 0., 0., 0.};
    __syncthreads();

    for (int hc0 = 0; hc0 < a.Hc; hc0 += 16) {
        // stage 1: dL/d(conv2 pre-activation at the window's argmax) of the chunk's 16*NP2 pooled outputs (contiguous features)
        for (int o = tid; o < L::DQ; o += 256) {
            const long long f = (long long)hc0 * G::NP2 + o;
            double g = 0.;
            for (int c = 0; c < a.C; ++c) g = fma(dzs[c], (double)a.Fw[((long long)sw * a.C + c) * F + f], g);
            dq[o] = g * act_deriv_value64<ACT>(a.Q2[sn * F + f]);
        }
        __syncthreads();
        // stage 2: every conv2 output adds the windows that chose it (window rows, then columns, ascending); the chunk's 16 x NPOS values are
        // contiguous in dO2
        for (int o = tid; o < 16 * G::NPOS; o += 256) {
            const int h = o / G::NPOS, pos = o - h * G::NPOS, y = pos / G::O2W, x = pos - y * G::O2W;
            const uint8_t* const ar = a.arg2 + sn * F + (long long)(hc0 + h) * G::NP2;
            double g = 0.;
            for (int py = y - 1; py <= y; ++py) {
                if (py < 0 || py >= G::P2W) continue;
                for (int px = x - 1; px <= x; ++px) {
                    if (px < 0 || px >= G::P2W) continue;
                    const int p = py * G::P2W + px;
                    if (ar[p] == (y - py) * 2 + (x - px)) g += dq[h * G::NP2 + p];
                }
            }
            dpad[h * PB * PB + (y + 4) * PB + x + 4] = g;
            if constexpr (WGRAD) a.dO2[(sn * a.Hc + hc0) * G::NPOS + o] = g;
        }
        __syncthreads();
        // conv2^T over the chunk: K = 16 channels x 25 taps
        const float* const wb = a.K2w + ((long long)sw * a.Hc + hc0) * 800 + li * 25;
        for (int k0 = 0; k0 < 400; k0 += 16) {
            int ao[4];
            double b0[4], b1[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = k0 + 4 * lg + r, wo = tab_w[k];
                ao[r] = tab_a[k];
                b0[r] = (double)wb[wo];                                     // ci = li
                b1[r] = (double)wb[wo + 16 * 25];                           // ci = 16 + li
            }
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                if (wave + 4 * m >= G::NPT1) continue;                      // (wave-uniform) a tile past the last position tile
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double av = dpad[abase[m] + ao[r]];
                    acc[2 * m] = MFMA64(av, b0[r], acc[2 * m]);
                    acc[2 * m + 1] = MFMA64(av, b1[r], acc[2 * m + 1]);
                }
            }
        }
        // (the next chunk's stage 1 writes dq only; its barrier stands between these reads of the image and stage 2's writes)
    }
    mfma64_drain(acc);
    // acc[2 m + jt][r] = dL/dP1 at position (wave + 4 m)*16 + lg + 4 r, channel jt*16 + li
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int jt = 0; jt < 2; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int tile = wave + 4 * m, pos = tile * 16 + lg + 4 * r;
                if (tile < G::NPT1 && pos < PP) {
                    const int idx = (jt * 16 + li) * PP + pos;
                    dp1[idx] = acc[2 * m + jt][r] * act_deriv_value64<ACT>(a.P1[sn * G::P1SZ + idx]);
                }
            }
    __syncthreads();
    if constexpr (WGRAD) {
        // pool-1 routing: a conv1 output takes its window's gradient where it was the window's argmax, zero elsewhere
        constexpr int OO = G::O1 * G::O1;
        for (int o = tid; o < C1 * OO; o += 256) {
            const int ci = o / OO, rem = o - ci * OO, oy = rem / G::O1, ox = rem - oy * G::O1;
            const int pidx = ci * PP + (oy >> 1) * G::P1W + (ox >> 1);
            a.dO1[sn * (C1 * OO) + o] = (a1s[pidx] == (oy & 1) * 2 + (ox & 1)) ? dp1[pidx] : 0.;
        }
    } else {
        // pool-1 routing + conv1^T, gather form: an input pixel adds the conv1 outputs it fed that were their window's argmax
        constexpr int II = G::IW * G::IW;
        for (int o = tid; o < G::DIN; o += 256) {
            const int cin = o / II, rem = o - cin * II, Y = rem / G::IW, X = rem - Y * G::IW;
            double g = 0.;
            for (int ci = 0; ci < C1; ++ci)
                for (int ky = 0; ky < 5; ++ky) {
                    const int oy = Y - ky;
                    if (oy < 0 || oy >= G::O1) continue;
                    for (int kx = 0; kx < 5; ++kx) {
                        const int ox = X - kx;
                        if (ox < 0 || ox >= G::O1) continue;
                        const int pidx = ci * PP + (oy >> 1) * G::P1W + (ox >> 1);
                        if (a1s[pidx] == (oy & 1) * 2 + (ox & 1)) g = fma(k1[ci * G::K1 + cin * 25 + ky * 5 + kx], dp1[pidx], g);
                    }
                }
            a.Gs[sn * G::DIN + o] = g;
        }
    }
}

template <int ACT, class G>
__global__ void __launch_bounds__(256) conv_input_grad_fp64_kernel(const ConvFp64Args a) { conv_backward_fp64_body<ACT, G, false>(a); }

__global__ void conv_sum_samples_fp64_kernel(const double* __restrict__ Gs, int S, int N, int D, double scale, double* __restrict__ G, int ldg) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // one thread per (n, d); s = 0, 1, ... in order
    if (i >= (long long)N * D) return;
    const long long n = i / D;
    const int d = (int)(i - n * D);
    double sum = 0.;
    for (int s = 0; s < S; ++s) sum += Gs[((long long)s * N + n) * D + d];
    G[n * ldg + d] = sum * scale;
}

__global__ void __launch_bounds__(256) conv_norms_fp64_kernel(const double* __restrict__ G, int ldg, int N, int D, double* __restrict__ linf,
                                                              double* __restrict__ l2) { row_norms64(G, ldg, N, D, linf, l2); }

// what the two device entry points check in common: the descriptor (validate_conv), then the block count (one block per (s, n))
int validate_conv_fp64(const rbnn_conv_posterior* net, int32_t N, int32_t S) {
    const int rc = validate_conv(net);
    if (rc) return rc;
    if (N < 1 || S < 1 || (long long)N * S > 0x7fffffffLL) return RBNN_ERR_SHAPE;
    return RBNN_OK;
}

template <int ACT, class G>
int launch_conv_forward_fp64(const ConvFp64Args& a, hipStream_t st) {
    const dim3 grid((unsigned)((long long)a.S * a.N));
    hipLaunchKernelGGL((conv1_pool_fp64_kernel<ACT, G>), grid, dim3(256), 0, st, a);
    int rc = launch_status();
    if (rc) return rc;
    constexpr int LDSB = conv2_fp64_lds_bytes<G>();
    static unsigned long long attr = 0;                                   // per instantiation, one bit per device
    if (!ensure_dynamic_lds((const void*)conv2_pool_fp64_kernel<ACT, G>, LDSB, attr)) return RBNN_ERR_LAUNCH;
    hipLaunchKernelGGL((conv2_pool_fp64_kernel<ACT, G>), grid, dim3(256), LDSB, st, a);
    if ((rc = launch_status())) return rc;
    hipLaunchKernelGGL(conv_head_fp64_kernel, grid, dim3(256), 0, st, a, (int)G::NP2);
    return launch_status();
}

template <int ACT, class G>
int launch_conv_input_grad_fp64(const ConvFp64Args& a, hipStream_t st) {
    constexpr int LDSB = BwdFp64Lds<G>::BYTES;
    static unsigned long long attr = 0;
    if (!ensure_dynamic_lds((const void*)conv_input_grad_fp64_kernel<ACT, G>, LDSB, attr)) return RBNN_ERR_LAUNCH;
    hipLaunchKernelGGL((conv_input_grad_fp64_kernel<ACT, G>), dim3((unsigned)((long long)a.S * a.N)), dim3(256), LDSB, st, a);
    return launch_status();
}

}  // namespace

// ===================================================================================================
// C-ABI of the conv fp64 checker
// ===================================================================================================
extern "C" {

int rbnn_conv_fp64_workspace_query(const rbnn_conv_posterior* net, int32_t N, int32_t S, size_t* bytes) {
    if (!net || !bytes) return RBNN_ERR_NULL;
    if (net->hidden < 16 || (net->hidden & 15) || N < 1 || S < 1) return RBNN_ERR_SHAPE;
    return for_geometry(net, [&](auto g) {
        using G = decltype(g);
        const size_t SN = (size_t)S * N, F = (size_t)net->hidden * G::NP2;
        bytes[0] = bytes[1] = SN * RBNN_CPAD * sizeof(double);            // P, dZ
        bytes[2] = (size_t)N * RBNN_CPAD * sizeof(double);                // Psum
        bytes[3] = SN * G::P1SZ * sizeof(double);                         // P1
        bytes[4] = SN * G::P1SZ;                                          // arg1
        bytes[5] = SN * F * sizeof(double);                               // Q2
        bytes[6] = SN * F;                                                // arg2
        bytes[7] = SN * G::DIN * sizeof(double);                          // Gs
        return (int)RBNN_OK;
    });
}

int rbnn_conv_forward_fp64(const rbnn_conv_posterior* net, const float* X, int32_t ldx, int32_t N, const int32_t* sidx, int32_t S,
                           int32_t out_kind, double* P, double* P1, uint8_t* arg1, double* Q2, uint8_t* arg2, void* stream) {
    int rc = validate_conv_fp64(net, N, S);
    if (rc) return rc;
    if (!X || !P || !P1 || !arg1 || !Q2 || !arg2) return RBNN_ERR_NULL;
    if (ldx < net->in_channels * net->in_width * net->in_width || (ldx & 3)) return RBNN_ERR_SHAPE;
    if (out_kind != RBNN_OUT_PROBS && out_kind != RBNN_OUT_LOGITS) return RBNN_ERR_UNSUPPORTED;
    if (!aligned16(X) || !aligned16(P) || !aligned16(P1) || !aligned16(Q2)) return RBNN_ERR_ALIGN;
    ConvFp64Args a = {};
    a.X = X; a.ldx = ldx; a.N = N;
    a.K1w = net->K1w; a.K1b = net->K1b; a.K2w = net->K2w; a.K2b = net->K2b; a.Fw = net->Fw; a.Fb = net->Fb;
    a.Hc = net->hidden; a.C = net->n_classes; a.sidx = sidx; a.S = S;
    a.P1 = P1; a.arg1 = arg1; a.Q2 = Q2; a.arg2 = arg2; a.P = P; a.out_kind = out_kind;
    hipStream_t st = (hipStream_t)stream;
    return for_geometry(net, [&](auto g) {
        return for_activation(net->activation, [&](auto act) { return launch_conv_forward_fp64<decltype(act)::value, decltype(g)>(a, st); });
    });
}

int rbnn_conv_input_grad_fp64(const rbnn_conv_posterior* net, const int32_t* sidx, int32_t S, int32_t N, const double* dZ, const double* P1,
                              const uint8_t* arg1, const double* Q2, const uint8_t* arg2, double* Gs, double scale, double* G, int32_t ldg,
                              double* linf, double* l2, void* stream) {
    int rc = validate_conv_fp64(net, N, S);
    if (rc) return rc;
    if (!dZ || !P1 || !arg1 || !Q2 || !arg2 || !Gs || !G) return RBNN_ERR_NULL;
    const int D = net->in_channels * net->in_width * net->in_width;
    if (ldg < D) return RBNN_ERR_SHAPE;
    if (!aligned16(dZ) || !aligned16(P1) || !aligned16(Q2) || !aligned16(Gs)) return RBNN_ERR_ALIGN;
    ConvFp64Args a = {};
    a.N = N; a.K1w = net->K1w; a.K2w = net->K2w; a.Fw = net->Fw;
    a.Hc = net->hidden; a.C = net->n_classes; a.sidx = sidx; a.S = S;
    a.P1 = const_cast<double*>(P1); a.arg1 = const_cast<uint8_t*>(arg1); a.Q2 = const_cast<double*>(Q2); a.arg2 = const_cast<uint8_t*>(arg2);
    a.dZ = dZ; a.Gs = Gs;
    hipStream_t st = (hipStream_t)stream;
    rc = for_geometry(net, [&](auto g) {
        return for_activation(net->activation, [&](auto act) { return launch_conv_input_grad_fp64<decltype(act)::value, decltype(g)>(a, st); });
    });
    if (rc) return rc;
    const long long total = (long long)N * D;
    hipLaunchKernelGGL(conv_sum_samples_fp64_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, Gs, S, N, D, scale, G, ldg);
    if ((rc = launch_status())) return rc;
    if (linf || l2) {
        hipLaunchKernelGGL(conv_norms_fp64_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, G, ldg, N, D, linf, l2);
        rc = launch_status();
    }
    return rc;
}

}  // extern "C"
