// rbnn_train.hip — SVI training of the fc / fc2 guides (model_bnn.py:105-136, :303-365): one step of pyro's SVI with TraceMeanField_ELBO and
// pyro.optim.Adam on a batch of B points, entirely on the device:
//
//      rbnn_svi_train_draw      W = loc + sigma * eps           ONE weight sample (pyro.random_module samples once per guide call)
//      rbnn_svi_train_forward   A1 = X W1^T + b1 -> H1 (fc2: -> A2 -> H2), logits, CE per point, dZ = softmax - e_y, and the backward
//                               down to dL/d(pre-activation) of every hidden layer (fc: 2 launches, fc2: 4)
//      rbnn_svi_weight_grads    dW2 = dZ^T H, dWm = dA2^T H1, dW1 = dA1^T X and every bias gradient: ONE launch, fp32 MFMA
//      rbnn_svi_adam_step       per element: eps regenerated, g_loc / g_raw, Adam moments, loc / raw / sigma, KL partial sums
//      rbnn_svi_train_finalize  fixed-order sums of the KL partials and the per-point CE (+ correct predictions of an accuracy forward)
//
// eps is the draw's own generator (rbnn_common.hpp: Rng, the draw_quad layout — quad index r * ceil(cols/4) + c/4, counter (quad, tensor id,
// sample 0, draw id)), so the update regenerates it instead of storing it, and the weights equal what rbnn_svi_draw writes for the same
// (key, draw id) at sample 0.  No atomics anywhere: every sum has one fixed order, two runs are bit-identical.
#include "rbnn_common.hpp"

namespace {

// ---------------------------------------------------------------------------------------------------
// Parameter layout of the flat buffers: the state_dict tensors in order, unpadded, row-major (a bias: one row).
// ---------------------------------------------------------------------------------------------------
struct Seg { long long off, first_quad; int rows, cols, tensor_id; };
struct Layout { Seg s[6]; int n; long long n_params, n_quads; };

Layout layout_of(const rbnn_svi_train_net& n) {
    Layout L = {};
    const int D = n.in_features, H = n.hidden, C = n.n_classes;
    const bool fc2 = n.arch == RBNN_ARCH_FC2;
    const int rows[6] = {H, 1, fc2 ? H : C, 1, C, 1}, cols[6] = {D, H, H, fc2 ? H : C, H, C};
    const int ids[6] = {T_W1, T_B1, fc2 ? T_WM : T_W2, fc2 ? T_BM : T_B2, T_W2, T_B2};
    L.n = fc2 ? 6 : 4;
    long long off = 0, q = 0;
    for (int i = 0; i < L.n; ++i) {
        L.s[i] = {off, q, rows[i], cols[i], ids[i]};
        off += (long long)rows[i] * cols[i];
        q += (long long)rows[i] * ((cols[i] + 3) / 4);
    }
    L.n_params = off; L.n_quads = q;
    return L;
}

constexpr int ELT_THREADS = 256;

__device__ __forceinline__ int seg_of(const Layout& L, long long q) {
    int i = 0;
#pragma unroll
    for (int j = 1; j < 6; ++j) if (j < L.n && q >= L.s[j].first_quad) i = j;
    return i;
}

__device__ __forceinline__ float softplus_f(float r) { return r > 20.f ? r : log1pf(expf(r)); }     // torch.nn.functional.softplus (threshold 20)

__global__ void __launch_bounds__(ELT_THREADS) train_draw_kernel(const Layout L, const float* __restrict__ loc, const float* __restrict__ sigma,
                                                                 float* __restrict__ W, unsigned long long key, uint32_t draw_id) {
    const long long q = (long long)blockIdx.x * ELT_THREADS + threadIdx.x;
    if (q >= L.n_quads) return;
    const Seg sg = L.s[seg_of(L, q)];
    const int Q = (sg.cols + 3) >> 2;
    const long long ql = q - sg.first_quad;
    const int r = (int)(ql / Q), c4 = (int)(ql % Q);
    const Rng rng = {(uint32_t)key, (uint32_t)(key >> 32), 0u, draw_id};
    float w[4];
    draw_quad(rng, sg.tensor_id, loc + sg.off, sigma + sg.off, r, c4, sg.cols, w);
    float* const out = W + sg.off + (long long)r * sg.cols + 4 * c4;
#pragma unroll
    for (int j = 0; j < 4; ++j) if (4 * c4 + j < sg.cols) out[j] = w[j];
}

// ---------------------------------------------------------------------------------------------------
// Strided fp32-MFMA GEMM  C(m, n) = sum_k A(m, k) B(n, k)  over 64 x 64 output tiles, K in stages of 16 staged through LDS (zero outside
// [M, N, K]: any shape, nothing read out of bounds).  Each output element is one lane's accumulator over k in increasing order: no atomics,
// reproducible.  Up to 3 independent problems per launch (the weight gradients of all layers).
// ---------------------------------------------------------------------------------------------------
enum { EPI_STORE = 0, EPI_FWD = 1, EPI_MUL = 2 };

struct GemmProb {
    const float* A; long long a_m, a_k;      // A(m, k) = A[m a_m + k a_k]
    const float* B; long long b_n, b_k;      // B(n, k) = B[n b_n + k b_k]
    int M, N, K;
    int ones_n;                              // >= 0: B(ones_n, k) = 1, so column ones_n is sum_k A(m, k) (a bias gradient) -> bias_out[m]
    float* Cout; long long ldc;              // C(m, n) -> Cout[m ldc + n]
    float* bias_out;
    const float* bias;                       // EPI_FWD: pre = C + bias[n]; Cout = act(pre), Dout = act'(pre)
    float* Dout;
    const float* Dmul;                       // EPI_MUL: Cout = C * Dmul[m ldc + n]
    int epi, act, tiles_n, first_tile;
};
struct GemmArgs { GemmProb p[3]; int n_prob; };

constexpr int GT = 64, GK = 16, GLD = GT + 4;

__device__ __forceinline__ float act_value(int act, float a) {
    if (act == RBNN_ACT_RELU) return a > 0.f ? a : 0.f;
    if (act == RBNN_ACT_LEAKY) return a > 0.f ? a : a * LEAKY_SLOPE;
    if (act == RBNN_ACT_SIGM) return 1.f / (1.f + expf(-a));
    return tanhf(a);
}
// torch's backward of each activation: relu (a > 0), leaky_relu (a > 0 ? 1 : slope), sigmoid h (1 - h), tanh 1 - h^2
__device__ __forceinline__ float act_deriv(int act, float a, float h) {
    if (act == RBNN_ACT_RELU) return a > 0.f ? 1.f : 0.f;
    if (act == RBNN_ACT_LEAKY) return a > 0.f ? 1.f : LEAKY_SLOPE;
    if (act == RBNN_ACT_SIGM) return h * (1.f - h);
    return 1.f - h * h;
}

__global__ void __launch_bounds__(256) train_gemm_kernel(const GemmArgs g) {
    __shared__ float As[GK][GLD], Bs[GK][GLD];
    int pi = 0;
#pragma unroll
    for (int j = 1; j < 3; ++j) if (j < g.n_prob && (int)blockIdx.x >= g.p[j].first_tile) pi = j;
    const GemmProb& p = g.p[pi];
    const int tile = blockIdx.x - p.first_tile, m0 = GT * (tile / p.tiles_n), n0 = GT * (tile % p.tiles_n);
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, li = lane & 15, lg = lane >> 4;
    const int n_real = p.ones_n >= 0 ? p.ones_n : p.N;
    f32x4 acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < p.K; k0 += GK) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = t + 256 * i;
            int mm, kk;
            if (p.a_k == 1) { mm = idx >> 4; kk = idx & 15; } else { mm = idx & 63; kk = idx >> 6; }     // coalesced along the unit stride
            const int m = m0 + mm, k = k0 + kk;
            As[kk][mm] = (m < p.M && k < p.K) ? p.A[m * p.a_m + k * p.a_k] : 0.f;
            int nn, kb;
            if (p.b_k == 1) { nn = idx >> 4; kb = idx & 15; } else { nn = idx & 63; kb = idx >> 6; }
            const int n = n0 + nn, kq = k0 + kb;
            float bv = 0.f;
            if (kq < p.K) {
                if (n < n_real) bv = p.B[n * p.b_n + kq * p.b_k];
                else if (n == p.ones_n) bv = 1.f;
            }
            Bs[kb][nn] = bv;
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < GK / 4; ++ks) {
            const float a = As[4 * ks + lg][16 * wave + li];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[nt] = MFMA16(a, Bs[4 * ks + lg][16 * nt + li], acc[nt]);
        }
        __syncthreads();
    }
    // lane holds C(m0 + 16 wave + 4 lg + r, n0 + 16 nt + li)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int n = n0 + 16 * nt + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + 16 * wave + 4 * lg + r;
            if (m >= p.M || n >= p.N) continue;
            const float v = acc[nt][r];
            if (n == p.ones_n) { p.bias_out[m] = v; continue; }
            const long long o = (long long)m * p.ldc + n;
            if (p.epi == EPI_FWD) {
                const float pre = v + p.bias[n], h = act_value(p.act, pre);
                p.Cout[o] = h;
                p.Dout[o] = act_deriv(p.act, pre, h);
            } else if (p.epi == EPI_MUL) {
                p.Cout[o] = v * p.Dmul[o];
            } else {
                p.Cout[o] = v;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Output layer + loss: one wave per point.  z = H W2^T + b2, CE = logsumexp(z) - z_y (Categorical(logits=log_softmax(z)), summed later),
// dZ = softmax(z) - e_y (ce_softmax_grad at inv_S = 1: the RBNN_LOSS_MEAN_LOGIT gradient at S = 1), dA = (dZ W2) * act'.
// ---------------------------------------------------------------------------------------------------
struct HeadArgs {
    const float *Hl, *Dl, *W2, *b2;
    const int32_t* labels;
    float *dZ, *ce, *dA;
    int B, H, C;
};

__global__ void __launch_bounds__(256) train_head_kernel(const HeadArgs a) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= a.B) return;
    float z[RBNN_CPAD];
#pragma unroll
    for (int c = 0; c < RBNN_CPAD; ++c) z[c] = 0.f;
    const float* hrow = a.Hl + (long long)b * a.H;
    for (int h = lane; h < a.H; h += 64) {
        const float hv = hrow[h];
#pragma unroll
        for (int c = 0; c < RBNN_CPAD; ++c) if (c < a.C) z[c] = fmaf(hv, a.W2[(long long)c * a.H + h], z[c]);
    }
#pragma unroll
    for (int c = 0; c < RBNN_CPAD; ++c) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) z[c] += __shfl_xor(z[c], off, 64);
        if (c < a.C) z[c] += a.b2[c];
    }
    const int y = a.labels[b];
    float g[RBNN_CPAD];
    ce_softmax_grad<RBNN_CPAD>(z, a.C, y, 1.f, g);
    if (lane == 0) {
        float m = -INFINITY, zy = 0.f;
        for (int c = 0; c < a.C; ++c) { m = fmaxf(m, z[c]); if (c == y) zy = z[c]; }
        float den = 0.f, rest = 0.f;
        for (int c = 0; c < a.C; ++c) { const float e = expf(z[c] - m); den += e; if (c != y) rest += e; }
        // label = argmax: CE = log(1 + sum_{c != y} e^(z_c - z_y)) without the cancellation of log(den) - 0
        a.ce[b] = (zy == m) ? log1pf(rest) : logf(den) - (zy - m);
#pragma unroll
        for (int c = 0; c < RBNN_CPAD; ++c) a.dZ[(long long)b * RBNN_CPAD + c] = g[c];
    }
    const float* drow = a.Dl + (long long)b * a.H;
    float* arow = a.dA + (long long)b * a.H;
    for (int h = lane; h < a.H; h += 64) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < RBNN_CPAD; ++c) if (c < a.C) s = fmaf(g[c], a.W2[(long long)c * a.H + h], s);
        arow[h] = s * drow[h];
    }
}

// ---------------------------------------------------------------------------------------------------
// Adam (torch.optim.Adam, single-tensor, defaults but lr) on loc and raw scale, one thread per quad of a tensor:
//   g_loc = dCE/dw + loc,   g_raw = (dCE/dw eps + sigma - 1/sigma) sigmoid(raw)      (TraceMeanField's analytic KL against N(0, 1))
//   m = m + (1 - b1)(g - m),  v = b2 v + (1 - b2) g^2,  p += (-step_size m) / (sqrt(v) / bc2_sqrt + eps_adam),  sigma = softplus(raw)
// and the KL of the PRE-update parameters, -log sigma + (sigma^2 + loc^2) / 2 - 1/2, summed per block in a fixed tree order.
// ---------------------------------------------------------------------------------------------------
struct AdamArgs {
    Layout L;
    float *loc, *raw, *sigma, *m_loc, *v_loc, *m_raw, *v_raw;
    const float* grad;
    float* kl_part;
    unsigned long long key;
    uint32_t draw_id;
    float w1, beta2, w2, adam_eps, step_size, bc2_sqrt;      // w1 = 1 - beta1, w2 = 1 - beta2: formed in double on the host
};

__device__ __forceinline__ void adam_one(float& p, float& m, float& v, float g, const AdamArgs& a) {
    m = fmaf(a.w1, g - m, m);                                // exp_avg.lerp_(grad, 1 - beta1)
    v = fmaf(a.w2, g * g, v * a.beta2);                      // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(v) / a.bc2_sqrt + a.adam_eps;
    p = p + (-a.step_size * m) / denom;                      // param.addcdiv_(exp_avg, denom, value=-step_size)
}

__global__ void __launch_bounds__(ELT_THREADS) adam_kernel(const AdamArgs a) {
    __shared__ float red[ELT_THREADS];
    const long long q = (long long)blockIdx.x * ELT_THREADS + threadIdx.x;
    float kl = 0.f;
    if (q < a.L.n_quads) {
        const Seg sg = a.L.s[seg_of(a.L, q)];
        const int Q = (sg.cols + 3) >> 2;
        const long long ql = q - sg.first_quad;
        const int r = (int)(ql / Q), c4 = (int)(ql % Q);
        const Rng rng = {(uint32_t)a.key, (uint32_t)(a.key >> 32), 0u, a.draw_id};
        float eps[4];
        rng.quad(sg.tensor_id, (uint32_t)(r * Q + c4), eps);
        const long long base = sg.off + (long long)r * sg.cols + 4 * c4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (4 * c4 + j >= sg.cols) continue;
            const long long e = base + j;
            float mu = a.loc[e], rw = a.raw[e];
            const float sd = a.sigma[e], dw = a.grad[e];
            kl += (-logf(sd) + 0.5f * (sd * sd + mu * mu)) - 0.5f;
            const float gl = dw + mu;
            const float sig = 1.f / (1.f + expf(-rw));
            const float gr = (fmaf(dw, eps[j], sd) - 1.f / sd) * sig;
            float ml = a.m_loc[e], vl = a.v_loc[e], mr = a.m_raw[e], vr = a.v_raw[e];
            adam_one(mu, ml, vl, gl, a);
            adam_one(rw, mr, vr, gr, a);
            a.loc[e] = mu; a.raw[e] = rw; a.sigma[e] = softplus_f(rw);
            a.m_loc[e] = ml; a.v_loc[e] = vl; a.m_raw[e] = mr; a.v_raw[e] = vr;
        }
    }
    red[threadIdx.x] = kl;
    __syncthreads();
#pragma unroll
    for (int s = ELT_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.kl_part[blockIdx.x] = red[0];
}

// ---------------------------------------------------------------------------------------------------
// One block: stats[0] = CE + KL of the step, stats[1] += it, stats[2] += #(argmax Psum == label).  Fixed-order sums in fp64.
// ---------------------------------------------------------------------------------------------------
struct FinalArgs {
    const float *kl_part, *ce, *Psum;
    const int32_t* labels;
    double* stats;
    int n_part, B, ldp, C;
};

__global__ void __launch_bounds__(256) finalize_kernel(const FinalArgs a) {
    __shared__ double red[256];
    __shared__ double cnt[256];
    const int t = threadIdx.x;
    double s = 0.0, k = 0.0;
    for (int i = t; i < a.n_part; i += 256) s += (double)a.kl_part[i];
    for (int i = t; i < a.B; i += 256) {
        s += (double)a.ce[i];
        if (a.Psum) {
            const float* row = a.Psum + (long long)i * a.ldp;
            int best = 0;
            for (int c = 1; c < a.C; ++c) if (row[c] > row[best]) best = c;      // the first maximum, as torch.argmax
            k += (best == a.labels[i]) ? 1.0 : 0.0;
        }
    }
    red[t] = s; cnt[t] = k;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) { red[t] += red[t + w]; cnt[t] += cnt[t + w]; }
        __syncthreads();
    }
    if (t == 0) {
        a.stats[0] = red[0];
        a.stats[1] += red[0];
        a.stats[2] += cnt[0];
    }
}

int check_net(const rbnn_svi_train_net* n) {
    if (!n) return RBNN_ERR_NULL;
    if (n->arch != RBNN_ARCH_FC && n->arch != RBNN_ARCH_FC2) return RBNN_ERR_UNSUPPORTED;
    if (n->activation < RBNN_ACT_RELU || n->activation > RBNN_ACT_TANH) return RBNN_ERR_UNSUPPORTED;
    if (n->in_features < 1 || n->hidden < 1 || n->n_classes < 1 || n->n_classes > RBNN_CPAD) return RBNN_ERR_SHAPE;
    if ((long long)n->hidden * n->in_features > (1LL << 30) || (long long)n->hidden * n->hidden > (1LL << 30)) return RBNN_ERR_SHAPE;
    return RBNN_OK;
}

int gemm_launch(GemmArgs& g, hipStream_t st) {
    int tiles = 0;
    for (int i = 0; i < g.n_prob; ++i) {
        GemmProb& p = g.p[i];
        p.tiles_n = (p.N + GT - 1) / GT;
        p.first_tile = tiles;
        tiles += p.tiles_n * ((p.M + GT - 1) / GT);
    }
    hipLaunchKernelGGL(train_gemm_kernel, dim3(tiles), dim3(256), 0, st, g);
    return launch_status();
}

GemmProb fwd_prob(const float* A, long long lda, const float* W, const float* b, int M, int N, int K, float* H, float* D, int act) {
    GemmProb p = {};
    p.A = A; p.a_m = lda; p.a_k = 1; p.B = W; p.b_n = K; p.b_k = 1; p.M = M; p.N = N; p.K = K; p.ones_n = -1;
    p.Cout = H; p.ldc = N; p.bias = b; p.Dout = D; p.epi = EPI_FWD; p.act = act;
    return p;
}

// dW[m, n] = sum_b dA[b, m] src[b, n] (n < N), db[m] = sum_b dA[b, m]
GemmProb wgrad_prob(const float* dA, long long ld_da, const float* src, long long ld_src, int M, int N, int B, float* dW, float* db) {
    GemmProb p = {};
    p.A = dA; p.a_m = 1; p.a_k = ld_da; p.B = src; p.b_n = 1; p.b_k = ld_src; p.M = M; p.N = N + 1; p.K = B; p.ones_n = N;
    p.Cout = dW; p.ldc = N; p.bias_out = db; p.epi = EPI_STORE;
    return p;
}

}  // namespace

extern "C" {

int64_t rbnn_svi_train_sizes(const rbnn_svi_train_net* net, int64_t* n_partials) {
    const int rc = check_net(net);
    if (rc) return rc;
    const Layout L = layout_of(*net);
    if (n_partials) *n_partials = (L.n_quads + ELT_THREADS - 1) / ELT_THREADS;
    return L.n_params;
}

int rbnn_svi_train_draw(const rbnn_svi_train_net* net, uint64_t key, uint32_t draw_id, void* stream) {
    int rc = check_net(net);
    if (rc) return rc;
    if (!net->loc || !net->sigma || !net->W) return RBNN_ERR_NULL;
    const Layout L = layout_of(*net);
    hipLaunchKernelGGL(train_draw_kernel, dim3((unsigned)((L.n_quads + ELT_THREADS - 1) / ELT_THREADS)), dim3(ELT_THREADS), 0, (hipStream_t)stream,
                       L, net->loc, net->sigma, net->W, (unsigned long long)key, draw_id);
    return launch_status();
}

int rbnn_svi_train_forward(const rbnn_svi_train_net* net, const float* X, int32_t ldx, int32_t n_points, const int32_t* labels,
                           const rbnn_svi_train_ws* ws, void* stream) {
    int rc = check_net(net);
    if (rc) return rc;
    if (!X || !labels || !ws || !net->W) return RBNN_ERR_NULL;
    const bool fc2 = net->arch == RBNN_ARCH_FC2;
    if (!ws->hid1 || !ws->dact1 || !ws->dA1 || !ws->dZ || !ws->ce) return RBNN_ERR_NULL;
    if (fc2 && (!ws->hid2 || !ws->dact2 || !ws->dA2)) return RBNN_ERR_NULL;
    if (n_points < 1 || ldx < net->in_features) return RBNN_ERR_SHAPE;
    const Layout L = layout_of(*net);
    const int D = net->in_features, H = net->hidden, C = net->n_classes, B = n_points, act = net->activation;
    hipStream_t st = (hipStream_t)stream;
    const float* W = net->W;
    GemmArgs g = {};
    g.n_prob = 1;
    g.p[0] = fwd_prob(X, ldx, W + L.s[0].off, W + L.s[1].off, B, H, D, ws->hid1, ws->dact1, act);
    if ((rc = gemm_launch(g, st))) return rc;
    if (fc2) {
        g.p[0] = fwd_prob(ws->hid1, H, W + L.s[2].off, W + L.s[3].off, B, H, H, ws->hid2, ws->dact2, act);
        if ((rc = gemm_launch(g, st))) return rc;
    }
    HeadArgs h = {};
    h.Hl = fc2 ? ws->hid2 : ws->hid1; h.Dl = fc2 ? ws->dact2 : ws->dact1;
    h.W2 = W + L.s[L.n - 2].off; h.b2 = W + L.s[L.n - 1].off; h.labels = labels;
    h.dZ = ws->dZ; h.ce = ws->ce; h.dA = fc2 ? ws->dA2 : ws->dA1; h.B = B; h.H = H; h.C = C;
    hipLaunchKernelGGL(train_head_kernel, dim3((B + 3) / 4), dim3(256), 0, st, h);
    if ((rc = launch_status())) return rc;
    if (fc2) {
        // dA1[b, i] = (sum_o dA2[b, o] Wm[o, i]) act'1[b, i]
        GemmProb p = {};
        p.A = ws->dA2; p.a_m = H; p.a_k = 1; p.B = W + L.s[2].off; p.b_n = 1; p.b_k = H; p.M = B; p.N = H; p.K = H; p.ones_n = -1;
        p.Cout = ws->dA1; p.ldc = H; p.Dmul = ws->dact1; p.epi = EPI_MUL;
        g.p[0] = p;
        if ((rc = gemm_launch(g, st))) return rc;
    }
    return RBNN_OK;
}

int rbnn_svi_weight_grads(const rbnn_svi_train_net* net, const float* X, int32_t ldx, int32_t n_points, const rbnn_svi_train_ws* ws,
                          void* stream) {
    int rc = check_net(net);
    if (rc) return rc;
    if (!X || !ws || !net->grad) return RBNN_ERR_NULL;
    const bool fc2 = net->arch == RBNN_ARCH_FC2;
    if (!ws->hid1 || !ws->dA1 || !ws->dZ) return RBNN_ERR_NULL;
    if (fc2 && (!ws->hid2 || !ws->dA2)) return RBNN_ERR_NULL;
    if (n_points < 1 || ldx < net->in_features) return RBNN_ERR_SHAPE;
    const Layout L = layout_of(*net);
    const int D = net->in_features, H = net->hidden, C = net->n_classes, B = n_points;
    float* G = net->grad;
    GemmArgs g = {};
    g.n_prob = fc2 ? 3 : 2;
    g.p[0] = wgrad_prob(ws->dA1, H, X, ldx, H, D, B, G + L.s[0].off, G + L.s[1].off);
    if (fc2) g.p[1] = wgrad_prob(ws->dA2, H, ws->hid1, H, H, H, B, G + L.s[2].off, G + L.s[3].off);
    g.p[g.n_prob - 1] = wgrad_prob(ws->dZ, RBNN_CPAD, fc2 ? ws->hid2 : ws->hid1, H, C, H, B, G + L.s[L.n - 2].off, G + L.s[L.n - 1].off);
    return gemm_launch(g, (hipStream_t)stream);
}

int rbnn_svi_adam_step(const rbnn_svi_train_net* net, uint64_t key, uint32_t draw_id, int64_t step, double lr, double beta1, double beta2,
                       double adam_eps, float* kl_partials, void* stream) {
    int rc = check_net(net);
    if (rc) return rc;
    if (!net->loc || !net->raw || !net->sigma || !net->m_loc || !net->v_loc || !net->m_raw || !net->v_raw || !net->grad || !kl_partials)
        return RBNN_ERR_NULL;
    if (step < 1) return RBNN_ERR_SHAPE;
    AdamArgs a = {};
    a.L = layout_of(*net);
    a.loc = net->loc; a.raw = net->raw; a.sigma = net->sigma; a.m_loc = net->m_loc; a.v_loc = net->v_loc; a.m_raw = net->m_raw; a.v_raw = net->v_raw;
    a.grad = net->grad; a.kl_part = kl_partials; a.key = key; a.draw_id = draw_id;
    // torch's single-tensor Adam takes its scalars (the bias corrections, 1 - beta1, 1 - beta2) in Python floats (double) and hands them to
    // fp32 tensor ops: each is rounded to fp32 once.  (1.f - 0.999f is 1.3e-5 off 0.001: with v << (1 - beta2) g^2 that is 6e-6 of the update.)
    a.w1 = (float)(1.0 - beta1); a.beta2 = (float)beta2; a.w2 = (float)(1.0 - beta2); a.adam_eps = (float)adam_eps;
    a.step_size = (float)(lr / (1.0 - pow(beta1, (double)step)));
    a.bc2_sqrt = (float)sqrt(1.0 - pow(beta2, (double)step));
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((a.L.n_quads + ELT_THREADS - 1) / ELT_THREADS)), dim3(ELT_THREADS), 0, (hipStream_t)stream, a);
    return launch_status();
}

int rbnn_svi_train_finalize(const float* kl_partials, int64_t n_partials, const float* ce, int32_t n_points, const float* Psum, int32_t ldp,
                            const int32_t* labels, int32_t n_classes, double* stats, void* stream) {
    if (!kl_partials || !ce || !stats || (Psum && !labels)) return RBNN_ERR_NULL;
    if (n_partials < 1 || n_partials > 0x7FFFFFFF || n_points < 1 || (Psum && (n_classes < 1 || n_classes > ldp))) return RBNN_ERR_SHAPE;
    FinalArgs a = {kl_partials, ce, Psum, labels, stats, (int)n_partials, n_points, ldp, n_classes};
    hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status();
}

}  // extern "C"
