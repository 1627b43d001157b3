// rbnn_fp64.inc — the fp64 precision mode of the fc / fc2 forward and expected input gradient (included by rbnn_kernels.hip).
//
// The data stay fp32 (weight stacks, X, the attack iterates) and are widened on load, which is exact; every operation from the first
// product to the written result is fp64.  The contractions over D and over H run on v_mfma_f64_16x16x4_f64 with fp64 accumulators, the
// C-wide ones (hid . W2^T, dZ . W2) are fp64 FMAs.  No atomics, no slabs: every result element is one accumulation chain in a fixed order
// (K ascending; the gradient also samples ascending), so two runs are bit-identical and a point's result depends neither on N nor on
// the point block it ran in.
//
// The f64 MFMA's lane maps, the widening loads, act / act' in fp64 and mfma64_drain: rbnn_fp64_common.hpp (shared with the conv checker).
#include "rbnn_fp64_common.hpp"

namespace {

// ===================================================================================================
// F1: one layer of the stacked forward.  One block (4 waves) = one (16-point tile, sample):
//   pre[n][h] = sum_k A[n][k] * W[s][h][k] + b[s][h]      A operand = the tile's 16 input rows, B operand = 16 W rows; D = [n][h]
// The hidden units go in chunks of 256 (4 waves x 4 tiles of 16).  Every layer stashes act'(pre) in fp64 for the backward.
// LAST = false (fc2 layer 1): the activations go to `hid` [S][N][H] (fp64), the next launch's A operand.
// LAST = true: the activations of a chunk go to LDS and thread (n, c) adds its part of z[n][c] = sum_h hid[n][h] * W2[s][c][h]
// (h ascending across the chunks), then bias and the softmax with the maximum subtracted.
// ===================================================================================================
struct Fwd64Args {
    const void* A;  long long a_sample_stride;  int lda;  int N;         // input rows: X (fp32, shared) or hid (fp64, per sample)
    const float* W; long long w_sample_stride;  int ldw;  int K;         // [S_total][H][ldw]; K = contraction length, a multiple of 4
    const float* b;                                                      // [S_total][H]
    const float* W2;  const float* b2;  int C;  int H;                   // output layer (LAST only)
    const int* sidx;
    double* P;  double* dact;  double* hid;  int out_kind;
};

template <int ACT, typename TA, bool LAST>
__global__ void __launch_bounds__(256) fc_forward_f64_kernel(const Fwd64Args a) {
    constexpr int HC = 256, LDH = HC + 1;
    __shared__ double hidL[LAST ? 16 * LDH : 1];
    __shared__ double zL[LAST ? 256 : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
    const int s = blockIdx.y, n0 = blockIdx.x * 16;
    const int sw = a.sidx ? a.sidx[s] : s;
    const float* const Ws = a.W + (long long)sw * a.w_sample_stride;
    const int na = min(n0 + li, a.N - 1);                      // rows past N repeat the last point; never stored
    const TA* const arow = (const TA*)a.A + (long long)s * a.a_sample_stride + (long long)na * a.lda;
    const int zn = tid >> 4, zc = tid & 15;                    // the logits' thread map: (point of the tile, class)
    double z = 0.;

    for (int hc0 = 0; hc0 < a.H; hc0 += HC) {
        f64x4 acc[4];
        const float* wrow[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            acc[t] = (f64x4){0., 0., 0., 0.};
            wrow[t] = Ws + (long long)min(hc0 + (wave * 4 + t) * 16 + li, a.H - 1) * a.ldw;   // rows past H repeat the last unit; never stored
        }
        for (int k0 = 0; k0 < a.K; k0 += 16) {
            const int k = k0 + 4 * lg;
            const bool in = k < a.K;
            const int kc = in ? k : 0;
            f64x4 av = load4_f64(arow + kc);
            if (!in) av = (f64x4){0., 0., 0., 0.};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (hc0 + (wave * 4 + t) * 16 >= a.H) continue;           // (wave-uniform) a tile wholly past H
                f64x4 bv = load4_f64(wrow[t] + kc);
                if (!in) bv = (f64x4){0., 0., 0., 0.};
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[t] = MFMA64(av[r], bv[r], acc[t]);
            }
        }
        mfma64_drain(acc);
        // ---- epilogue of the chunk: acc[t][r] = pre-activation of point n0 + lg + 4*r, unit hc0 + (4*wave + t)*16 + li, without its bias
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int hl = (wave * 4 + t) * 16 + li, h = hc0 + hl;
            const bool h_ok = h < a.H;
            const double bias = h_ok ? (double)a.b[(long long)sw * a.H + h] : 0.;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int nl = lg + 4 * r, n = n0 + nl;
                const double pre = acc[t][r] + bias;
                const double hv = act_fwd64<ACT>(pre);
                if (h_ok && n < a.N) {
                    const long long o = ((long long)s * a.N + n) * a.H + h;
                    a.dact[o] = act_deriv64<ACT>(pre, hv);
                    if (!LAST) a.hid[o] = hv;
                }
                if (LAST) hidL[nl * LDH + hl] = h_ok ? hv : 0.;
            }
        }
        if (LAST) {
            __syncthreads();
            const int hn = min(HC, a.H - hc0);
            if (zc < a.C) {
                const float* const w2 = a.W2 + ((long long)sw * a.C + zc) * a.H + hc0;
                for (int hh = 0; hh < hn; ++hh) z = fma(hidL[zn * LDH + hh], (double)w2[hh], z);
            }
            __syncthreads();
        }
    }

    if (LAST) {
        z = (zc < a.C) ? z + (double)a.b2[(long long)sw * a.C + zc] : 0.;
        double out = z;
        if (a.out_kind == RBNN_OUT_PROBS) {                    // (uniform over the block)
            zL[tid] = z;
            __syncthreads();
            double m = -INFINITY, den = 0.;
            for (int c = 0; c < a.C; ++c) m = fmax(m, zL[zn * 16 + c]);
            for (int c = 0; c < a.C; ++c) den += exp(zL[zn * 16 + c] - m);
            out = (zc < a.C) ? exp(z - m) / den : 0.;
        }
        const int n = n0 + zn;
        if (n < a.N) a.P[((long long)s * a.N + n) * RBNN_CPAD + zc] = out;
    }
}

// ===================================================================================================
// F2: dL/d(hidden pre-activation) of the layer under the output layer, in place in its act' stash:
//   dact[s][n][h] <- dact[s][n][h] * sum_c dZ[s][n][c] * W2[s][c][h]          (c ascending; one thread per element)
// ===================================================================================================
__global__ void __launch_bounds__(256) dhid_f64_kernel(const double* __restrict__ dZ, const float* __restrict__ W2, const int* __restrict__ sidx,
                                                       long long total, int N, int C, int H, double* __restrict__ dact) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long sn = i / H;
    const int h = (int)(i - sn * H), s = (int)(sn / N);
    const int sw = sidx ? sidx[s] : s;
    double g = 0.;
    for (int c = 0; c < C; ++c) g = fma(dZ[sn * RBNN_CPAD + c], (double)W2[((long long)sw * C + c) * H + h], g);
    dact[i] *= g;
}

// ===================================================================================================
// F3: the backward contractions over the hidden units.  One block = one wave = one (16-point tile, group of DT 16-column tiles):
//   acc[n][j] = sum_s sum_k A[s][n][k] * W[s][k][j]           A operand = dL/d(pre-activation) rows (fp64), B operand = W rows k
// PER_SAMPLE = false (the last step, W = W1): all used samples in ascending order inside one register accumulator,
//   out[n][j] = scale * acc — the expected input gradient; no slabs, no second pass.
// PER_SAMPLE = true (fc2, W = Wm): one sample per block (grid z), out[s][n][j] <- out[s][n][j] * acc, in place in layer 1's act' stash.
// ===================================================================================================
struct Grad64Args {
    const double* A;  int K;                                             // [S][N][K]
    const float* W;   long long w_sample_stride;  int ldw;  int ncols;  // [S_total][K][ldw]; columns < ncols are computed
    const int* sidx;  int S;  int N;
    double* out;  int ldo;  double scale;
};

template <int DT, bool PER_SAMPLE>
__global__ void __launch_bounds__(64) fc_grad_f64_kernel(const Grad64Args a) {
    const int lane = threadIdx.x, li = lane & 15, lg = lane >> 4;
    const int n0 = blockIdx.x * 16, c0 = blockIdx.y * DT * 16;
    const int na = min(n0 + li, a.N - 1);
    int colc[DT];
    f64x4 acc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
        acc[dt] = (f64x4){0., 0., 0., 0.};
        colc[dt] = min(c0 + dt * 16 + li, a.ncols - 1);        // columns past ncols repeat the last one; never stored
    }
    const int s_begin = PER_SAMPLE ? blockIdx.z : 0, s_end = PER_SAMPLE ? s_begin + 1 : a.S;
    for (int s = s_begin; s < s_end; ++s) {
        const int sw = a.sidx ? a.sidx[s] : s;
        const double* const arow = a.A + ((long long)s * a.N + na) * a.K;
        const float* const Ws = a.W + (long long)sw * a.w_sample_stride;
        for (int k0 = 0; k0 < a.K; k0 += 16) {
            const int k = k0 + 4 * lg;
            const bool in = k < a.K;
            const int kc = in ? k : 0;
            f64x4 av = load4_f64(arow + kc);
            if (!in) av = (f64x4){0., 0., 0., 0.};
            const float* const wk = Ws + (long long)kc * a.ldw;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                if (c0 + dt * 16 >= a.ncols) continue;         // (wave-uniform) a tile wholly past the last column
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double b = in ? (double)wk[(long long)r * a.ldw + colc[dt]] : 0.;
                    acc[dt] = MFMA64(av[r], b, acc[dt]);
                }
            }
        }
    }
    mfma64_drain(acc);
    // ---- acc[dt][r] = D[n = n0 + lg + 4*r][j = c0 + dt*16 + li]
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
        const int j = c0 + dt * 16 + li;
        if (j >= a.ncols) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = n0 + lg + 4 * r;
            if (n >= a.N) continue;
            if (PER_SAMPLE) {
                double* const dst = a.out + ((long long)s_begin * a.N + n) * a.ldo + j;
                *dst = *dst * acc[dt][r];
            } else {
                a.out[(long long)n * a.ldo + j] = acc[dt][r] * a.scale;
            }
        }
    }
}

// per-point norms of the finished gradient over its D real columns (row_norms64 of rbnn_fp64_common.hpp)
__global__ void __launch_bounds__(256) norms_f64_kernel(const double* __restrict__ G, int ldg, int N, int D, double* __restrict__ linf,
                                                        double* __restrict__ l2) { row_norms64(G, ldg, N, D, linf, l2); }

// ===================================================================================================
// Element-wise kernels.
// ===================================================================================================
__global__ void reduce_samples_f64_kernel(const double* __restrict__ P, int S, int N, int C, double scale, double* __restrict__ out, int ldo) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;       // one thread per (n, class); s = 0, 1, ... in order
    if (i >= N * RBNN_CPAD) return;
    const int n = i >> 4, c = i & 15;
    if (c >= C) return;
    double sum = 0.;
    for (int s = 0; s < S; ++s) sum += P[((long long)s * N + n) * RBNN_CPAD + c];
    out[(long long)n * ldo + c] = sum * scale;
}

// softmax_backward / ce_softmax_grad of rbnn_common.hpp in fp64: the same cancellation-free forms (the label class of softmax(t) - e_y as
// -(sum of the others), the winning class of p (g - <g, p>) as p sum_k p_k (g_m - g_k)), which sit inside the textbook forms' own rounding
__global__ void loss_dlogits_f64_kernel(int mode, const double* __restrict__ P, const double* __restrict__ Psum, int ldp,
                                        const int* __restrict__ labels, int S, double inv_S, int N, int C, double* __restrict__ dZ) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // one thread per (s, n)
    if (i >= (long long)S * N) return;
    const int n = (int)(i % N), y = labels[n];
    double p[16], t[16], e[16], g[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        p[c] = (c < C) ? P[i * RBNN_CPAD + c] : 0.;
        // what the loss saw: the mean probabilities (the "double softmax"), this sample's probabilities, or the mean logits
        t[c] = (c < C) ? ((mode == RBNN_LOSS_PER_SAMPLE) ? p[c] : Psum[(long long)n * ldp + c] * inv_S) : 0.;
    }
    double m = -INFINITY, den = 0., rest = 0.;
#pragma unroll
    for (int c = 0; c < 16; ++c) if (c < C) m = fmax(m, t[c]);
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        e[c] = (c < C) ? exp(t[c] - m) : 0.;
        den += e[c];
        if (c != y) rest += e[c];
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) g[c] = (c < C) ? ((c == y ? -rest : e[c]) / den) * inv_S : 0.;
    double out[16];
    if (mode == RBNN_LOSS_MEAN_LOGIT) {                        // P holds logits: dZ_s = dL/d(mean logits) / S
#pragma unroll
        for (int c = 0; c < 16; ++c) out[c] = g[c];
    } else {
        double dot = 0., pm = -INFINITY, gm = 0., sm = 0.;
        int im = 0;
#pragma unroll
        for (int c = 0; c < 16; ++c)
            if (c < C) {
                dot += g[c] * p[c];
                if (p[c] > pm) { pm = p[c]; gm = g[c]; im = c; }
            }
#pragma unroll
        for (int k = 0; k < 16; ++k) if (k < C) sm = fma(p[k], gm - g[k], sm);
#pragma unroll
        for (int c = 0; c < 16; ++c) out[c] = (c < C) ? (c == im ? sm : g[c] - dot) * p[c] : 0.;
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) dZ[i * RBNN_CPAD + c] = out[c];
}

// attack_step_kernel's arithmetic on X (fp32, both forms) with the sign read from the fp64 gradient
__global__ void attack_step_f64_kernel(float* __restrict__ X, const float* __restrict__ X0, int ldx, const double* __restrict__ G, int ldg,
                                       const float* __restrict__ alpha, float alpha_scalar, float eps, int project, int N, int D) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // one thread per pixel
    if (i >= (long long)N * D) return;
    const long long n = i / D;
    const int d = (int)(i % D);
    const double g = G[n * ldg + d];
    const float sgn = (g > 0.) ? 1.f : ((g < 0.) ? -1.f : 0.f);              // torch.sign: sign(0) = 0
    const float step = alpha ? alpha[n] : alpha_scalar;
    const float x = X[n * ldx + d];
    float pert = x + step * sgn;
    if (project) {
        const float x0 = X0[n * ldx + d];
        const float eta = fminf(fmaxf(pert - x0, -eps), eps);
        pert = x0 + eta;
    }
    X[n * ldx + d] = fminf(fmaxf(pert, 0.f), 1.f);
}

// ---------------------------------------------------------------------------------------------------
// host-side helpers
// ---------------------------------------------------------------------------------------------------
int validate_net_f64(const rbnn_posterior* net) {
    if (!net || !net->W1 || !net->b1 || !net->W2 || !net->b2) return RBNN_ERR_NULL;
    if (net->arch != RBNN_ARCH_FC && net->arch != RBNN_ARCH_FC2) return RBNN_ERR_UNSUPPORTED;
    if (net->arch == RBNN_ARCH_FC2 && (!net->Wm || !net->bm)) return RBNN_ERR_NULL;
    if (net->activation < RBNN_ACT_RELU || net->activation > RBNN_ACT_TANH) return RBNN_ERR_UNSUPPORTED;
    if (net->in_features < 1 || net->in_stride < net->in_features || (net->in_stride & 15)) return RBNN_ERR_SHAPE;
    if (net->hidden < 4 || (net->hidden & 3)) return RBNN_ERR_SHAPE;             // rows of Wm / W2 and of the fp64 stashes start on 16 bytes
    if (net->n_classes < 1 || net->n_classes > RBNN_CPAD || net->n_stored < 1) return RBNN_ERR_SHAPE;
    if (!aligned16(net->W1) || !aligned16(net->W2)) return RBNN_ERR_ALIGN;
    if (net->arch == RBNN_ARCH_FC2 && !aligned16(net->Wm)) return RBNN_ERR_ALIGN;
    return RBNN_OK;
}

template <typename TA, bool LAST>
int launch_forward_f64(int act, const Fwd64Args& a, int S, hipStream_t st) {
    const dim3 grid((unsigned)((a.N + 15) / 16), (unsigned)S);
    return for_activation(act, [&](auto A) {
        hipLaunchKernelGGL((fc_forward_f64_kernel<decltype(A)::value, TA, LAST>), grid, dim3(256), 0, st, a);
        return launch_status();
    });
}

template <bool PER_SAMPLE>
int launch_grad_f64(const Grad64Args& a, hipStream_t st) {
    const int tiles = (a.ncols + 15) / 16;
    const unsigned nt = (unsigned)((a.N + 15) / 16), z = PER_SAMPLE ? (unsigned)a.S : 1u;
    if (tiles % 7 == 0) hipLaunchKernelGGL((fc_grad_f64_kernel<7, PER_SAMPLE>), dim3(nt, (unsigned)(tiles / 7), z), dim3(64), 0, st, a);
    else                hipLaunchKernelGGL((fc_grad_f64_kernel<4, PER_SAMPLE>), dim3(nt, (unsigned)((tiles + 3) / 4), z), dim3(64), 0, st, a);
    return launch_status();
}

}  // namespace

// ===================================================================================================
// C-ABI of the fp64 mode
// ===================================================================================================
extern "C" {

int rbnn_f64_workspace_query(const rbnn_posterior* net, int32_t N, int32_t S, size_t* bytes) {
    if (!net || !bytes) return RBNN_ERR_NULL;
    if (net->arch != RBNN_ARCH_FC && net->arch != RBNN_ARCH_FC2) return RBNN_ERR_UNSUPPORTED;
    if (net->hidden < 4 || (net->hidden & 3) || N < 1 || S < 1) return RBNN_ERR_SHAPE;
    const size_t SN = (size_t)S * N, H = net->hidden;
    const bool fc2 = net->arch == RBNN_ARCH_FC2;
    bytes[0] = bytes[1] = SN * RBNN_CPAD * sizeof(double);                       // P, dZ
    bytes[2] = (size_t)N * RBNN_CPAD * sizeof(double);                           // Psum
    bytes[3] = SN * H * sizeof(double);                                          // dact1
    bytes[4] = bytes[5] = fc2 ? SN * H * sizeof(double) : 0;                     // hid1, dact2
    return RBNN_OK;
}

int rbnn_fc_forward_f64(const rbnn_posterior* net, const float* X, int32_t ldx, int32_t N, const int32_t* sidx, int32_t S,
                        int32_t out_kind, double* P, double* dact1, double* hid1, double* dact2, void* stream) {
    int rc = validate_net_f64(net);
    if (rc) return rc;
    if (!X || !P || !dact1) return RBNN_ERR_NULL;
    if (N < 1 || S < 1 || S > 65535 || ldx < net->in_stride || (ldx & 3)) return RBNN_ERR_SHAPE;
    if (out_kind != RBNN_OUT_PROBS && out_kind != RBNN_OUT_LOGITS) return RBNN_ERR_UNSUPPORTED;
    if (!aligned16(X) || !aligned16(P) || !aligned16(dact1)) return RBNN_ERR_ALIGN;
    const bool fc2 = net->arch == RBNN_ARCH_FC2;
    hipStream_t st = (hipStream_t)stream;
    const int H = net->hidden;

    Fwd64Args a = {};
    a.A = X; a.a_sample_stride = 0; a.lda = ldx; a.N = N;
    a.W = net->W1; a.w_sample_stride = (long long)H * net->in_stride; a.ldw = net->in_stride; a.K = net->in_stride;
    a.b = net->b1; a.W2 = net->W2; a.b2 = net->b2; a.C = net->n_classes; a.H = H;
    a.sidx = sidx; a.P = P; a.dact = dact1; a.hid = nullptr; a.out_kind = out_kind;
    if (!fc2) return launch_forward_f64<float, true>(net->activation, a, S, st);

    // fc2: layer 1 -> hid1 (+ stash 1), then layer 2 over the per-sample hidden rows -> P (+ stash 2)
    if (!hid1 || !dact2) return RBNN_ERR_NULL;
    if (!aligned16(hid1) || !aligned16(dact2)) return RBNN_ERR_ALIGN;
    a.hid = hid1;
    rc = launch_forward_f64<float, false>(net->activation, a, S, st);
    if (rc) return rc;
    Fwd64Args b = a;
    b.A = hid1; b.a_sample_stride = (long long)N * H; b.lda = H;
    b.W = net->Wm; b.w_sample_stride = (long long)H * H; b.ldw = H; b.K = H;
    b.b = net->bm; b.dact = dact2; b.hid = nullptr;
    return launch_forward_f64<double, true>(net->activation, b, S, st);
}

int rbnn_reduce_samples_f64(const double* P, int32_t S, int32_t N, int32_t C, double scale, double* out, int32_t ldo, void* stream) {
    if (!P || !out) return RBNN_ERR_NULL;
    if (S < 1 || N < 1 || C < 1 || C > RBNN_CPAD || ldo < C) return RBNN_ERR_SHAPE;
    hipLaunchKernelGGL(reduce_samples_f64_kernel, dim3((N * RBNN_CPAD + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, S, N, C, scale, out, ldo);
    return launch_status();
}

int rbnn_loss_dlogits_f64(int32_t mode, const double* P, const double* Psum, int32_t ldp, const int32_t* labels, int32_t S, double inv_S,
                          int32_t N, int32_t C, double* dZ, void* stream) {
    if (!P || !dZ || !labels) return RBNN_ERR_NULL;
    if (mode != RBNN_LOSS_MEAN_PROB && mode != RBNN_LOSS_PER_SAMPLE && mode != RBNN_LOSS_MEAN_LOGIT) return RBNN_ERR_UNSUPPORTED;
    if (mode != RBNN_LOSS_PER_SAMPLE && !Psum) return RBNN_ERR_NULL;
    if (S < 1 || N < 1 || C < 1 || C > RBNN_CPAD || (Psum && ldp < C)) return RBNN_ERR_SHAPE;
    const long long total = (long long)S * N;
    hipLaunchKernelGGL(loss_dlogits_f64_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       mode, P, Psum, ldp, labels, S, inv_S, N, C, dZ);
    return launch_status();
}

int rbnn_fc_input_grad_f64(const rbnn_posterior* net, const int32_t* sidx, int32_t S, int32_t N, const double* dZ, double* dact1,
                           double* dact2, double scale, double* G, int32_t ldg, double* linf, double* l2, void* stream) {
    int rc = validate_net_f64(net);
    if (rc) return rc;
    if (!dZ || !dact1 || !G) return RBNN_ERR_NULL;
    const bool fc2 = net->arch == RBNN_ARCH_FC2;
    if (fc2 && !dact2) return RBNN_ERR_NULL;
    if (N < 1 || S < 1 || S > 65535 || ldg < net->in_stride) return RBNN_ERR_SHAPE;
    if (!aligned16(dact1) || (fc2 && !aligned16(dact2))) return RBNN_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const int H = net->hidden, C = net->n_classes, Dp = net->in_stride;
    const long long total = (long long)S * N * H;
    if ((total + 255) / 256 > 0x7fffffffLL) return RBNN_ERR_SHAPE;

    // dL/d(pre-activation) of the layer under the output layer, in place in its stash
    hipLaunchKernelGGL(dhid_f64_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, dZ, net->W2, sidx, total, N, C, H,
                       fc2 ? dact2 : dact1);
    if ((rc = launch_status())) return rc;
    Grad64Args g = {};
    g.K = H; g.sidx = sidx; g.S = S; g.N = N;
    if (fc2) {                                                 // dact1[s] <- dact1[s] * (dH2[s] . Wm_s)
        g.A = dact2; g.W = net->Wm; g.w_sample_stride = (long long)H * H; g.ldw = H; g.ncols = H;
        g.out = dact1; g.ldo = H; g.scale = 1.;
        if ((rc = launch_grad_f64<true>(g, st))) return rc;
    }
    g.A = dact1; g.W = net->W1; g.w_sample_stride = (long long)H * Dp; g.ldw = Dp; g.ncols = Dp;
    g.out = G; g.ldo = ldg; g.scale = scale;
    if ((rc = launch_grad_f64<false>(g, st))) return rc;
    if (linf || l2) {
        hipLaunchKernelGGL(norms_f64_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, G, ldg, N, net->in_features, linf, l2);
        rc = launch_status();
    }
    return rc;
}

int rbnn_attack_step_f64(float* X, const float* X0, int32_t ldx, const double* G, int32_t ldg, const float* alpha, float alpha_scalar,
                         float eps, int32_t project, int32_t N, int32_t D, void* stream) {
    if (!X || !G || (project && !X0)) return RBNN_ERR_NULL;
    if (N < 1 || D < 1 || ldx < D || ldg < D) return RBNN_ERR_SHAPE;
    const long long total = (long long)N * D;
    hipLaunchKernelGGL(attack_step_f64_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       X, X0, ldx, G, ldg, alpha, alpha_scalar, eps, project, N, D);
    return launch_status();
}

}  // extern "C"
