// rbnn_nn_train.hip — deterministic training of fc / fc2 nets (model_nn.py:175-219: torch.optim.Adam on nn.CrossEntropyLoss()), for M
// independent members of the same shape in LOCKSTEP (model_ensemble.py:69-83 trains them one after the other): every launch of a step covers
// all M members, the member is a grid dimension.
//
//      rbnn_nn_train_forward    A1 = X[rows] W1^T + b1 -> H1 (fc2: -> A2 -> H2), logits, CE per point, dZ = (softmax - e_y) / B (the loss is a
//                               MEAN over the batch), correct/incorrect per point from these logits, and the backward down to
//                               dL/d(pre-activation) of every hidden layer (fc: 2 launches, fc2: 4)
//      rbnn_nn_weight_grads     dW2 = dZ^T H, dWm = dA2^T H1, dW1 = dA1^T X[rows] and every bias gradient of every member: ONE launch
//      rbnn_nn_adam_step        torch.optim.Adam's single-tensor formula on every parameter of every member: one launch
//      rbnn_nn_train_finalize   per member: the fp32-rounded mean CE of the step, its running sum, the correct predictions (fp64, fixed order)
//
// The batch is read from a RESIDENT data matrix through an index array rows [M, B]: each member reads its own batch of its own permutation,
// nothing is copied.  The tile plan of a member does not depend on M and no sum crosses members: member m of a lockstep run is bit-identical
// to the same member trained alone.  No atomics anywhere: every sum has one fixed order.
// The device helpers (act_value, act_deriv, adam_one, the GEMM body) restate rbnn_train.hip's: that unit's code is left as it is.
#include "rbnn_common.hpp"

namespace {

// Parameter layout of one member: the state_dict tensors in order, unpadded, row-major (a bias: one row), as rbnn_train.hip's flat buffers.
struct MLayout { long long off[6]; int n; long long n_params; };

MLayout layout_of(const rbnn_nn_train_net& n) {
    MLayout L = {};
    const int D = n.in_features, H = n.hidden, C = n.n_classes;
    const bool fc2 = n.arch == RBNN_ARCH_FC2;
    const int rows[6] = {H, 1, fc2 ? H : C, 1, C, 1}, cols[6] = {D, H, H, fc2 ? H : C, H, C};
    L.n = fc2 ? 6 : 4;
    long long off = 0;
    for (int i = 0; i < L.n; ++i) {
        L.off[i] = off;
        off += (long long)rows[i] * cols[i];
    }
    L.n_params = off;
    return L;
}

constexpr int ELT_THREADS = 256;

// ---------------------------------------------------------------------------------------------------
// Strided fp32-MFMA GEMM  C(m, n) = sum_k A(m, k) B(n, k)  of member blockIdx.y over 64 x 64 output tiles, K in stages of 16 staged through LDS
// (zero outside [M, N, K]: any shape, nothing read out of bounds).  train_gemm_kernel's tile plan; every operand carries a member stride, and
// the rows of A (a_idx) or the k index of B (b_idx) may go through a per-member index array (the batch gathered from the resident data).
// Each output element is one lane's accumulator over k in increasing order.  Up to 3 independent problems per launch.
// ---------------------------------------------------------------------------------------------------
enum { EPI_STORE = 0, EPI_FWD = 1, EPI_MUL = 2 };

struct GemmProb {
    const float* A; long long a_m, a_k, a_mem;      // A(m, k) = A[mem a_mem + row(m) a_m + k a_k], row(m) = a_idx ? a_idx[mem idx_mem + m] : m
    const float* B; long long b_n, b_k, b_mem;      // B(n, k) = B[mem b_mem + n b_n + row(k) b_k], row(k) = b_idx ? b_idx[mem idx_mem + k] : k
    const int32_t *a_idx, *b_idx;
    long long idx_mem;
    int idx_max;                                    // gathered indices are clamped to [0, idx_max]: a bad index reads a wrong row, never outside X
    int M, N, K;
    int ones_n;                                     // >= 0: B(ones_n, k) = 1, so column ones_n is sum_k A(m, k) (a bias gradient) -> bias_out[m]
    float* Cout; long long ldc, c_mem;              // C(m, n) -> Cout[mem c_mem + m ldc + n]; Dout and Dmul share the layout
    float* bias_out;
    const float* bias;                              // EPI_FWD: pre = C + bias[n]; Cout = act(pre), Dout = act'(pre)
    long long bias_mem;                             // member stride of bias / bias_out
    float* Dout;
    const float* Dmul;                              // EPI_MUL: Cout = C * Dmul
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

__device__ __forceinline__ int gathered(const int32_t* idx, long long at, int i, int idx_max) {
    return idx ? min(max(idx[at + i], 0), idx_max) : i;
}

__global__ void __launch_bounds__(256) nn_train_gemm_kernel(const GemmArgs g) {
    __shared__ float As[GK][GLD], Bs[GK][GLD];
    int pi = 0;
#pragma unroll
    for (int j = 1; j < 3; ++j) if (j < g.n_prob && (int)blockIdx.x >= g.p[j].first_tile) pi = j;
    const GemmProb& p = g.p[pi];
    const long long mem = blockIdx.y;
    const int tile = blockIdx.x - p.first_tile, m0 = GT * (tile / p.tiles_n), n0 = GT * (tile % p.tiles_n);
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, li = lane & 15, lg = lane >> 4;
    const int n_real = p.ones_n >= 0 ? p.ones_n : p.N;
    const float* const A = p.A + mem * p.a_mem;
    const float* const Bm = p.B + mem * p.b_mem;
    const long long idx_at = mem * p.idx_mem;
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
            float av = 0.f;
            if (m < p.M && k < p.K) av = A[(long long)gathered(p.a_idx, idx_at, m, p.idx_max) * p.a_m + k * p.a_k];
            As[kk][mm] = av;
            int nn, kb;
            if (p.b_k == 1) { nn = idx >> 4; kb = idx & 15; } else { nn = idx & 63; kb = idx >> 6; }
            const int n = n0 + nn, kq = k0 + kb;
            float bv = 0.f;
            if (kq < p.K) {
                if (n < n_real) bv = Bm[n * p.b_n + (long long)gathered(p.b_idx, idx_at, kq, p.idx_max) * p.b_k];
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
            if (n == p.ones_n) { p.bias_out[mem * p.bias_mem + m] = v; continue; }
            const long long o = mem * p.c_mem + (long long)m * p.ldc + n;
            if (p.epi == EPI_FWD) {
                const float pre = v + p.bias[mem * p.bias_mem + n], h = act_value(p.act, pre);
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
// Output layer + loss: one wave per (member, point).  z = H W2^T + b2, CE = logsumexp(z) - z_y on train_head_kernel's two branches,
// dZ = (softmax(z) - e_y) / B (ce_softmax_grad at inv_S = 1 / B), correct = (first argmax z == y) as torch.argmax, dA = (dZ W2) * act'.
// ---------------------------------------------------------------------------------------------------
struct HeadArgs {
    const float *Hl, *Dl, *W2, *b2;           // Hl / Dl [M, B, H]; W2 / b2 of member 0, member stride p_mem
    long long p_mem;
    const int32_t *labels, *rows;             // labels of the resident data, rows [M, B] or NULL (point b is row b)
    int idx_max;
    float *dZ, *ce, *dA;
    int32_t* correct;
    int B, H, C;
    float inv_B;
};

__global__ void __launch_bounds__(256) nn_train_head_kernel(const HeadArgs a) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= a.B) return;
    const long long mem = blockIdx.y, pt = mem * a.B + b;
    const float* const W2 = a.W2 + mem * a.p_mem;
    float z[RBNN_CPAD];
#pragma unroll
    for (int c = 0; c < RBNN_CPAD; ++c) z[c] = 0.f;
    const float* hrow = a.Hl + pt * a.H;
    for (int h = lane; h < a.H; h += 64) {
        const float hv = hrow[h];
#pragma unroll
        for (int c = 0; c < RBNN_CPAD; ++c) if (c < a.C) z[c] = fmaf(hv, W2[(long long)c * a.H + h], z[c]);
    }
    const float* const b2 = a.b2 + mem * a.p_mem;
#pragma unroll
    for (int c = 0; c < RBNN_CPAD; ++c) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) z[c] += __shfl_xor(z[c], off, 64);
        if (c < a.C) z[c] += b2[c];
    }
    const int y = a.labels[gathered(a.rows, mem * a.B, b, a.idx_max)];
    float g[RBNN_CPAD];
    ce_softmax_grad<RBNN_CPAD>(z, a.C, y, a.inv_B, g);
    if (lane == 0) {
        float m = -INFINITY, zy = 0.f;
        int best = 0;
        for (int c = 0; c < a.C; ++c) {
            if (z[c] > m) { m = z[c]; best = c; }                     // strictly greater: the first maximum, as torch.argmax
            if (c == y) zy = z[c];
        }
        float den = 0.f, rest = 0.f;
        for (int c = 0; c < a.C; ++c) { const float e = expf(z[c] - m); den += e; if (c != y) rest += e; }
        // label = argmax: CE = log(1 + sum_{c != y} e^(z_c - z_y)) without the cancellation of log(den) - 0
        a.ce[pt] = (zy == m) ? log1pf(rest) : logf(den) - (zy - m);
        a.correct[pt] = best == y ? 1 : 0;
#pragma unroll
        for (int c = 0; c < RBNN_CPAD; ++c) a.dZ[pt * RBNN_CPAD + c] = g[c];
    }
    const float* drow = a.Dl + pt * a.H;
    float* arow = a.dA + pt * a.H;
    for (int h = lane; h < a.H; h += 64) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < RBNN_CPAD; ++c) if (c < a.C) s = fmaf(g[c], W2[(long long)c * a.H + h], s);
        arow[h] = s * drow[h];
    }
}

// ---------------------------------------------------------------------------------------------------
// Adam (torch.optim.Adam, single-tensor, defaults but lr), one thread per parameter of a member:
//   m = m + (1 - b1)(g - m),  v = b2 v + (1 - b2) g^2,  p += (-step_size m) / (sqrt(v) / bc2_sqrt + eps_adam)
// ---------------------------------------------------------------------------------------------------
struct AdamArgs {
    float *P, *m, *v;
    const float* grad;
    long long n_params, member_stride;
    float w1, beta2, w2, adam_eps, step_size, bc2_sqrt;      // w1 = 1 - beta1, w2 = 1 - beta2: formed in double on the host
};

__device__ __forceinline__ void adam_one(float& p, float& m, float& v, float g, const AdamArgs& a) {
    m = fmaf(a.w1, g - m, m);                                // exp_avg.lerp_(grad, 1 - beta1)
    v = fmaf(a.w2, g * g, v * a.beta2);                      // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(v) / a.bc2_sqrt + a.adam_eps;
    p = p + (-a.step_size * m) / denom;                      // param.addcdiv_(exp_avg, denom, value=-step_size)
}

__global__ void __launch_bounds__(ELT_THREADS) nn_adam_kernel(const AdamArgs a) {
    const long long i = (long long)blockIdx.x * ELT_THREADS + threadIdx.x;
    if (i >= a.n_params) return;
    const long long e = (long long)blockIdx.y * a.member_stride + i;
    float p = a.P[e], m = a.m[e], v = a.v[e];
    adam_one(p, m, v, a.grad[e], a);
    a.P[e] = p; a.m[e] = m; a.v[e] = v;
}

// ---------------------------------------------------------------------------------------------------
// One block per member: stats[m] = [fp32-rounded mean CE of the step, += it, += correct predictions].  Fixed-order sums in fp64.
// ---------------------------------------------------------------------------------------------------
struct FinalArgs {
    const float* ce;
    const int32_t* correct;
    double* stats;
    int B;
};

__global__ void __launch_bounds__(256) nn_finalize_kernel(const FinalArgs a) {
    __shared__ double red[256];
    __shared__ double cnt[256];
    const int t = threadIdx.x;
    const long long at = (long long)blockIdx.x * a.B;
    double s = 0.0, k = 0.0;
    for (int i = t; i < a.B; i += 256) {
        s += (double)a.ce[at + i];
        k += (double)a.correct[at + i];
    }
    red[t] = s; cnt[t] = k;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) { red[t] += red[t + w]; cnt[t] += cnt[t + w]; }
        __syncthreads();
    }
    if (t == 0) {
        double* const st = a.stats + 3 * (long long)blockIdx.x;
        const double loss = (double)(float)(red[0] / (double)a.B);      // loss.item() of an fp32 mean
        st[0] = loss;
        st[1] += loss;
        st[2] += cnt[0];
    }
}

int check_net(const rbnn_nn_train_net* n) {
    if (!n) return RBNN_ERR_NULL;
    if (n->arch != RBNN_ARCH_FC && n->arch != RBNN_ARCH_FC2) return RBNN_ERR_UNSUPPORTED;
    if (n->activation < RBNN_ACT_RELU || n->activation > RBNN_ACT_TANH) return RBNN_ERR_UNSUPPORTED;
    if (n->in_features < 1 || n->hidden < 1 || n->n_classes < 1 || n->n_classes > RBNN_CPAD) return RBNN_ERR_SHAPE;
    if ((long long)n->hidden * n->in_features > (1LL << 30) || (long long)n->hidden * n->hidden > (1LL << 30)) return RBNN_ERR_SHAPE;
    if (n->n_members < 1 || n->n_members > 65535) return RBNN_ERR_SHAPE;          // the member is grid dimension y
    return RBNN_OK;
}

int check_batch(const rbnn_nn_train_net* n, const float* X, int ldx, int n_rows, const int32_t* rows, int B) {
    if (!X) return RBNN_ERR_NULL;
    if (B < 1 || n_rows < 1 || ldx < n->in_features) return RBNN_ERR_SHAPE;
    if (!rows && B > n_rows) return RBNN_ERR_SHAPE;                                // rows 0..B-1 of X
    if ((long long)n->n_members * B * n->hidden > (1LL << 40) || n->member_stride < layout_of(*n).n_params) return RBNN_ERR_SHAPE;
    return RBNN_OK;
}

int gemm_launch(GemmArgs& g, int members, hipStream_t st) {
    int tiles = 0;
    for (int i = 0; i < g.n_prob; ++i) {
        GemmProb& p = g.p[i];
        p.tiles_n = (p.N + GT - 1) / GT;
        p.first_tile = tiles;
        tiles += p.tiles_n * ((p.M + GT - 1) / GT);
    }
    hipLaunchKernelGGL(nn_train_gemm_kernel, dim3(tiles, members), dim3(256), 0, st, g);
    return launch_status();
}

// H[mem, b, n] = act(sum_k A[mem, row(b), k] W[mem, n, k] + bias[mem, n]), D = act'
GemmProb fwd_prob(const float* A, long long lda, long long a_mem, const float* W, const float* b, long long p_mem, int M, int N, int K, float* H,
                  float* D, int act) {
    GemmProb p = {};
    p.A = A; p.a_m = lda; p.a_k = 1; p.a_mem = a_mem; p.B = W; p.b_n = K; p.b_k = 1; p.b_mem = p_mem; p.M = M; p.N = N; p.K = K; p.ones_n = -1;
    p.Cout = H; p.ldc = N; p.c_mem = (long long)M * N; p.bias = b; p.bias_mem = p_mem; p.Dout = D; p.epi = EPI_FWD; p.act = act;
    return p;
}

// dW[mem, m, n] = sum_b dA[mem, b, m] src[mem, row(b), n] (n < N), db[mem, m] = sum_b dA[mem, b, m]
GemmProb wgrad_prob(const float* dA, long long ld_da, const float* src, long long ld_src, long long src_mem, int M, int N, int B, float* dW,
                    float* db, long long p_mem) {
    GemmProb p = {};
    p.A = dA; p.a_m = 1; p.a_k = ld_da; p.a_mem = (long long)B * ld_da; p.B = src; p.b_n = 1; p.b_k = ld_src; p.b_mem = src_mem;
    p.M = M; p.N = N + 1; p.K = B; p.ones_n = N;
    p.Cout = dW; p.ldc = N; p.c_mem = p_mem; p.bias_out = db; p.bias_mem = p_mem; p.epi = EPI_STORE;
    return p;
}

}  // namespace

extern "C" {

int64_t rbnn_nn_train_sizes(const rbnn_nn_train_net* net) {
    const int rc = check_net(net);
    if (rc) return rc;
    return layout_of(*net).n_params;
}

int rbnn_nn_train_forward(const rbnn_nn_train_net* net, const float* X, int32_t ldx, int32_t n_rows, const int32_t* labels, const int32_t* rows,
                          int32_t n_points, const rbnn_nn_train_ws* ws, void* stream) {
    int rc = check_net(net);
    if (rc) return rc;
    if (!labels || !ws || !net->P) return RBNN_ERR_NULL;
    if ((rc = check_batch(net, X, ldx, n_rows, rows, n_points))) return rc;
    const bool fc2 = net->arch == RBNN_ARCH_FC2;
    if (!ws->hid1 || !ws->dact1 || !ws->dA1 || !ws->dZ || !ws->ce || !ws->correct) return RBNN_ERR_NULL;
    if (fc2 && (!ws->hid2 || !ws->dact2 || !ws->dA2)) return RBNN_ERR_NULL;
    const MLayout L = layout_of(*net);
    const int D = net->in_features, H = net->hidden, C = net->n_classes, B = n_points, act = net->activation, M = net->n_members;
    const long long ps = net->member_stride, bh = (long long)B * H;
    hipStream_t st = (hipStream_t)stream;
    const float* P = net->P;
    GemmArgs g = {};
    g.n_prob = 1;
    g.p[0] = fwd_prob(X, ldx, 0, P + L.off[0], P + L.off[1], ps, B, H, D, ws->hid1, ws->dact1, act);
    g.p[0].a_idx = rows; g.p[0].idx_mem = B; g.p[0].idx_max = n_rows - 1;
    if ((rc = gemm_launch(g, M, st))) return rc;
    if (fc2) {
        g.p[0] = fwd_prob(ws->hid1, H, bh, P + L.off[2], P + L.off[3], ps, B, H, H, ws->hid2, ws->dact2, act);
        if ((rc = gemm_launch(g, M, st))) return rc;
    }
    HeadArgs h = {};
    h.Hl = fc2 ? ws->hid2 : ws->hid1; h.Dl = fc2 ? ws->dact2 : ws->dact1;
    h.W2 = P + L.off[L.n - 2]; h.b2 = P + L.off[L.n - 1]; h.p_mem = ps; h.labels = labels; h.rows = rows; h.idx_max = n_rows - 1;
    h.dZ = ws->dZ; h.ce = ws->ce; h.correct = ws->correct; h.dA = fc2 ? ws->dA2 : ws->dA1; h.B = B; h.H = H; h.C = C;
    h.inv_B = 1.f / (float)B;
    hipLaunchKernelGGL(nn_train_head_kernel, dim3((B + 3) / 4, M), dim3(256), 0, st, h);
    if ((rc = launch_status())) return rc;
    if (fc2) {
        // dA1[b, i] = (sum_o dA2[b, o] Wm[o, i]) act'1[b, i]
        GemmProb p = {};
        p.A = ws->dA2; p.a_m = H; p.a_k = 1; p.a_mem = bh; p.B = P + L.off[2]; p.b_n = 1; p.b_k = H; p.b_mem = ps; p.M = B; p.N = H; p.K = H;
        p.ones_n = -1; p.Cout = ws->dA1; p.ldc = H; p.c_mem = bh; p.Dmul = ws->dact1; p.epi = EPI_MUL;
        g.p[0] = p;
        if ((rc = gemm_launch(g, M, st))) return rc;
    }
    return RBNN_OK;
}

int rbnn_nn_weight_grads(const rbnn_nn_train_net* net, const float* X, int32_t ldx, int32_t n_rows, const int32_t* rows, int32_t n_points,
                         const rbnn_nn_train_ws* ws, void* stream) {
    int rc = check_net(net);
    if (rc) return rc;
    if (!ws || !net->grad) return RBNN_ERR_NULL;
    if ((rc = check_batch(net, X, ldx, n_rows, rows, n_points))) return rc;
    const bool fc2 = net->arch == RBNN_ARCH_FC2;
    if (!ws->hid1 || !ws->dA1 || !ws->dZ) return RBNN_ERR_NULL;
    if (fc2 && (!ws->hid2 || !ws->dA2)) return RBNN_ERR_NULL;
    const MLayout L = layout_of(*net);
    const int D = net->in_features, H = net->hidden, C = net->n_classes, B = n_points;
    const long long ps = net->member_stride, bh = (long long)B * H;
    float* G = net->grad;
    GemmArgs g = {};
    g.n_prob = fc2 ? 3 : 2;
    g.p[0] = wgrad_prob(ws->dA1, H, X, ldx, 0, H, D, B, G + L.off[0], G + L.off[1], ps);
    g.p[0].b_idx = rows; g.p[0].idx_mem = B; g.p[0].idx_max = n_rows - 1;
    if (fc2) g.p[1] = wgrad_prob(ws->dA2, H, ws->hid1, H, bh, H, H, B, G + L.off[2], G + L.off[3], ps);
    g.p[g.n_prob - 1] = wgrad_prob(ws->dZ, RBNN_CPAD, fc2 ? ws->hid2 : ws->hid1, H, bh, C, H, B, G + L.off[L.n - 2], G + L.off[L.n - 1], ps);
    return gemm_launch(g, net->n_members, (hipStream_t)stream);
}

int rbnn_nn_adam_step(const rbnn_nn_train_net* net, int64_t step, double lr, double beta1, double beta2, double adam_eps, void* stream) {
    int rc = check_net(net);
    if (rc) return rc;
    if (!net->P || !net->m || !net->v || !net->grad) return RBNN_ERR_NULL;
    AdamArgs a = {};
    a.n_params = layout_of(*net).n_params;
    if (step < 1 || net->member_stride < a.n_params) return RBNN_ERR_SHAPE;
    a.P = net->P; a.m = net->m; a.v = net->v; a.grad = net->grad; a.member_stride = net->member_stride;
    // torch's single-tensor Adam takes its scalars (the bias corrections, 1 - beta1, 1 - beta2) in Python floats (double) and hands them to
    // fp32 tensor ops: each is rounded to fp32 once (as rbnn_svi_adam_step)
    a.w1 = (float)(1.0 - beta1); a.beta2 = (float)beta2; a.w2 = (float)(1.0 - beta2); a.adam_eps = (float)adam_eps;
    a.step_size = (float)(lr / (1.0 - pow(beta1, (double)step)));
    a.bc2_sqrt = (float)sqrt(1.0 - pow(beta2, (double)step));
    hipLaunchKernelGGL(nn_adam_kernel, dim3((unsigned)((a.n_params + ELT_THREADS - 1) / ELT_THREADS), net->n_members), dim3(ELT_THREADS), 0,
                       (hipStream_t)stream, a);
    return launch_status();
}

int rbnn_nn_train_finalize(const rbnn_nn_train_net* net, const rbnn_nn_train_ws* ws, int32_t n_points, double* stats, void* stream) {
    int rc = check_net(net);
    if (rc) return rc;
    if (!ws || !ws->ce || !ws->correct || !stats) return RBNN_ERR_NULL;
    if (n_points < 1) return RBNN_ERR_SHAPE;
    FinalArgs a = {ws->ce, ws->correct, stats, n_points};
    hipLaunchKernelGGL(nn_finalize_kernel, dim3(net->n_members), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status();
}

}  // extern "C"
