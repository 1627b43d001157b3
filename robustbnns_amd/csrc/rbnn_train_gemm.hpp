// rbnn_train_gemm.hpp — the forward / backward of an fc / fc2 net on the fp32 MFMA, shared by the units that launch it (rbnn_train.hip,
// rbnn_nn_train.hip, rbnn_hmc.hip, rbnn_svi_lockstep.hip): one strided GEMM kernel and one output-layer + loss kernel, for M independent members in lockstep (grid
// dimension y), and the host side of the lockstep forward / weight gradients.
// Both kernels are templates on LOCKSTEP and SKIP.  LOCKSTEP = false is a single net: member 0, no index arrays — the member strides, a_idx / b_idx / rows and the
// clamp are compiled out (measured: with them the SVI step was 5 % and an HMC transition 5 - 7 % slower than the kernels it had before).
#pragma once
#include "rbnn_train_core.hpp"

namespace {

// ---------------------------------------------------------------------------------------------------
// Strided fp32-MFMA GEMM  C(m, n) = sum_k A(m, k) B(n, k)  of member blockIdx.y over 64 x 64 output tiles, K in stages of 16 staged through LDS
// (zero outside [M, N, K]: any shape, nothing read out of bounds).  Every operand carries a member stride, and the rows of A (a_idx) or the k
// index of B (b_idx) may go through a per-member index array (the batch gathered from the resident data).  Each output element is one lane's
// accumulator over k in increasing order: no atomics, reproducible.  Up to 3 independent problems per launch (the weight gradients of all
// layers).
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
struct GemmArgs {
    GemmProb p[3]; int n_prob;
    // SKIP only: members come in groups of `per` (the 10 accuracy samples of a guide; 1: the member is the group).  A group with
    // counts[group] == 0 has finished: its blocks return at once, nothing of it is read or written.  The members of a group share its row of
    // a_idx / b_idx.
    const int32_t* counts; int per;
};

constexpr int GT = 64, GK = 16, GLD = GT + 4;

template <bool LOCKSTEP> __device__ __forceinline__ int gathered(const int32_t* idx, long long at, int i, int idx_max) {
    return (LOCKSTEP && idx) ? min(max(idx[at + i], 0), idx_max) : i;
}

// SKIP (LOCKSTEP with counts only, launched by rbnn_svi_lockstep.hip alone): a member, or a group of `per` members, with counts == 0 has
// finished; its blocks return at once and its workspaces keep what they held.
template <bool LOCKSTEP, bool SKIP> __global__ void __launch_bounds__(256) train_gemm_kernel(const GemmArgs g) {
    static_assert(LOCKSTEP || !SKIP, "only a lockstep launch has members to skip");
    __shared__ float As[GK][GLD], Bs[GK][GLD];
    long long idx_row = LOCKSTEP ? blockIdx.y : 0;
    if constexpr (SKIP) {
        idx_row = blockIdx.y / g.per;
        if (g.counts[idx_row] == 0) return;
    }
    int pi = 0;
#pragma unroll
    for (int j = 1; j < 3; ++j) if (j < g.n_prob && (int)blockIdx.x >= g.p[j].first_tile) pi = j;
    const GemmProb& p = g.p[pi];
    const long long mem = LOCKSTEP ? blockIdx.y : 0;
    const int tile = blockIdx.x - p.first_tile, m0 = GT * (tile / p.tiles_n), n0 = GT * (tile % p.tiles_n);
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, li = lane & 15, lg = lane >> 4;
    const int n_real = p.ones_n >= 0 ? p.ones_n : p.N;
    const float* const A = p.A + mem * p.a_mem;
    const float* const Bm = p.B + mem * p.b_mem;
    const long long idx_at = idx_row * p.idx_mem;
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
            if (m < p.M && k < p.K) av = A[(long long)gathered<LOCKSTEP>(p.a_idx, idx_at, m, p.idx_max) * p.a_m + k * p.a_k];
            As[kk][mm] = av;
            int nn, kb;
            if (p.b_k == 1) { nn = idx >> 4; kb = idx & 15; } else { nn = idx & 63; kb = idx >> 6; }
            const int n = n0 + nn, kq = k0 + kb;
            float bv = 0.f;
            if (kq < p.K) {
                if (n < n_real) bv = Bm[n * p.b_n + (long long)gathered<LOCKSTEP>(p.b_idx, idx_at, kq, p.idx_max) * p.b_k];
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
// Output layer + loss: one wave per (member, point).  z = H W2^T + b2, CE = logsumexp(z) - z_y (Categorical(logits=log_softmax(z)) /
// nn.CrossEntropyLoss per point), dZ = (softmax(z) - e_y) inv_S (ce_softmax_grad: inv_S = 1 for a summed loss, 1 / B for a mean),
// correct = (first argmax z == y) as torch.argmax, dA = (dZ W2) * act'.
// ---------------------------------------------------------------------------------------------------
struct HeadArgs {
    const float *Hl, *Dl, *W2, *b2;           // Hl / Dl [M, B, H]; W2 / b2 of member 0, member stride p_mem
    long long p_mem;
    const int32_t *labels, *rows;             // labels of the resident data, rows [M, B] or NULL (point b is row b)
    const int32_t* counts;                    // [M] or NULL: member m's own number of points <= B; a point behind it contributes exact zeros
    int idx_max;
    float *dZ, *ce, *dA;
    int32_t* correct;                         // nullable
    int B, H, C;
    float inv_S;
};

template <bool LOCKSTEP, bool SKIP> __global__ void __launch_bounds__(256) train_head_kernel(const HeadArgs a) {
    static_assert(LOCKSTEP || !SKIP, "only a lockstep launch has members to skip");
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= a.B) return;
    const long long mem = LOCKSTEP ? blockIdx.y : 0, pt = mem * a.B + b;
    if constexpr (SKIP) {
        if (a.counts[mem] == 0) return;
    }
    if (LOCKSTEP && a.counts && b >= a.counts[mem]) {                  // not a point of this member: ce, dZ, dA and correct are zero
        if (lane == 0) {
            a.ce[pt] = 0.f;
            if (a.correct) a.correct[pt] = 0;
#pragma unroll
            for (int c = 0; c < RBNN_CPAD; ++c) a.dZ[pt * RBNN_CPAD + c] = 0.f;
        }
        for (int h = lane; h < a.H; h += 64) a.dA[pt * a.H + h] = 0.f;
        return;
    }
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
    const int y = a.labels[gathered<LOCKSTEP>(a.rows, mem * a.B, b, a.idx_max)];
    float g[RBNN_CPAD];
    ce_softmax_grad<RBNN_CPAD>(z, a.C, y, a.inv_S, g);
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
        if (a.correct) a.correct[pt] = best == y ? 1 : 0;
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

template <bool LOCKSTEP, bool SKIP = false> int gemm_launch(GemmArgs& g, int members, hipStream_t st) {
    if (SKIP && (!g.counts || g.per < 1)) return RBNN_ERR_NULL;
    int tiles = 0;
    for (int i = 0; i < g.n_prob; ++i) {
        GemmProb& p = g.p[i];
        p.tiles_n = (p.N + GT - 1) / GT;
        p.first_tile = tiles;
        tiles += p.tiles_n * ((p.M + GT - 1) / GT);
    }
    hipLaunchKernelGGL((train_gemm_kernel<LOCKSTEP, SKIP>), dim3(tiles, LOCKSTEP ? members : 1), dim3(256), 0, st, g);
    return launch_status();
}

// H[mem, b, n] = act(sum_k A[mem, row(b), k] W[mem, n, k] + bias[mem, n]), D = act'
inline GemmProb fwd_prob(const float* A, long long lda, long long a_mem, const float* W, const float* b, long long p_mem, int M, int N, int K,
                         float* H, float* D, int act) {
    GemmProb p = {};
    p.A = A; p.a_m = lda; p.a_k = 1; p.a_mem = a_mem; p.B = W; p.b_n = K; p.b_k = 1; p.b_mem = p_mem; p.M = M; p.N = N; p.K = K; p.ones_n = -1;
    p.Cout = H; p.ldc = N; p.c_mem = (long long)M * N; p.bias = b; p.bias_mem = p_mem; p.Dout = D; p.epi = EPI_FWD; p.act = act;
    return p;
}

// dW[mem, m, n] = sum_b dA[mem, b, m] src[mem, row(b), n] (n < N), db[mem, m] = sum_b dA[mem, b, m]
inline GemmProb wgrad_prob(const float* dA, long long ld_da, const float* src, long long ld_src, long long src_mem, int M, int N, int B,
                           float* dW, float* db, long long p_mem) {
    GemmProb p = {};
    p.A = dA; p.a_m = 1; p.a_k = ld_da; p.a_mem = (long long)B * ld_da; p.B = src; p.b_n = 1; p.b_k = ld_src; p.b_mem = src_mem;
    p.M = M; p.N = N + 1; p.K = B; p.ones_n = N;
    p.Cout = dW; p.ldc = N; p.c_mem = p_mem; p.bias_out = db; p.bias_mem = p_mem; p.epi = EPI_STORE;
    return p;
}

// ---------------------------------------------------------------------------------------------------
// The lockstep forward / backward and weight gradients of an rbnn_nn_train_net on a batch gathered from resident data: what rbnn_nn_train.hip
// (mean CE: inv_S = 1 / B), rbnn_hmc.hip and rbnn_svi_lockstep.hip (summed CE: inv_S = 1, per-member counts) launch.  Those units define RBNN_TRAIN_LOCKSTEP
// before they include this file; a unit that does not never instantiates the LOCKSTEP = true kernels.
// ---------------------------------------------------------------------------------------------------
#ifdef RBNN_TRAIN_LOCKSTEP
struct LockstepBatch {
    const float* X; int ldx, n_rows;          // resident data [n_rows, ldx]
    const int32_t *labels, *rows, *counts;    // labels [n_rows]; rows [M, B] or NULL (rows 0..B-1 for every member); counts [M] or NULL
    int B;
};

inline int check_members(const rbnn_nn_train_net* n) {
    const int rc = check_net(n);
    if (rc) return rc;
    return (n->n_members < 1 || n->n_members > 65535) ? RBNN_ERR_SHAPE : RBNN_OK;      // the member is grid dimension y
}

inline int check_batch(const rbnn_nn_train_net* n, const LockstepBatch& b) {
    if (!b.X) return RBNN_ERR_NULL;
    if (b.B < 1 || b.n_rows < 1 || b.ldx < n->in_features) return RBNN_ERR_SHAPE;
    if (!b.rows && b.B > b.n_rows) return RBNN_ERR_SHAPE;                          // rows 0..B-1 of X
    if ((long long)n->n_members * b.B * n->hidden > (1LL << 40) || n->member_stride < layout_of(*n).n_params) return RBNN_ERR_SHAPE;
    return RBNN_OK;
}

// hidden activations, act', logits, ce, dZ, correct, and the backward to dA1 (fc2: dA2, then dA1): fc 2 launches, fc2 4.
// SKIP (needs counts): every launch leaves out a member with counts[m] == 0 altogether: its workspaces keep what they held, its grad is not
// written.  Without SKIP such a member's head writes zeros (ce, dZ, dA, correct) and its GEMMs run on them.
template <bool SKIP = false>
inline int lockstep_forward(const rbnn_nn_train_net* net, const LockstepBatch& b, const rbnn_nn_train_ws* ws, float inv_S, hipStream_t st) {
    int rc = check_members(net);
    if (rc) return rc;
    if (!b.labels || !ws || !net->P || (SKIP && !b.counts)) return RBNN_ERR_NULL;
    if ((rc = check_batch(net, b))) return rc;
    const bool fc2 = net->arch == RBNN_ARCH_FC2;
    if (!ws->hid1 || !ws->dact1 || !ws->dA1 || !ws->dZ || !ws->ce || !ws->correct) return RBNN_ERR_NULL;
    if (fc2 && (!ws->hid2 || !ws->dact2 || !ws->dA2)) return RBNN_ERR_NULL;
    const Layout L = layout_of(*net);
    const int D = net->in_features, H = net->hidden, C = net->n_classes, B = b.B, act = net->activation, M = net->n_members;
    const long long ps = net->member_stride, bh = (long long)B * H;
    const float* P = net->P;
    GemmArgs g = {};
    g.n_prob = 1; g.counts = b.counts; g.per = 1;
    g.p[0] = fwd_prob(b.X, b.ldx, 0, P + L.s[0].off, P + L.s[1].off, ps, B, H, D, ws->hid1, ws->dact1, act);
    g.p[0].a_idx = b.rows; g.p[0].idx_mem = B; g.p[0].idx_max = b.n_rows - 1;
    if ((rc = gemm_launch<true, SKIP>(g, M, st))) return rc;
    if (fc2) {
        g.p[0] = fwd_prob(ws->hid1, H, bh, P + L.s[2].off, P + L.s[3].off, ps, B, H, H, ws->hid2, ws->dact2, act);
        if ((rc = gemm_launch<true, SKIP>(g, M, st))) return rc;
    }
    HeadArgs h = {};
    h.Hl = fc2 ? ws->hid2 : ws->hid1; h.Dl = fc2 ? ws->dact2 : ws->dact1;
    h.W2 = P + L.s[L.n - 2].off; h.b2 = P + L.s[L.n - 1].off; h.p_mem = ps; h.labels = b.labels; h.rows = b.rows; h.counts = b.counts;
    h.idx_max = b.n_rows - 1;
    h.dZ = ws->dZ; h.ce = ws->ce; h.correct = ws->correct; h.dA = fc2 ? ws->dA2 : ws->dA1; h.B = B; h.H = H; h.C = C;
    h.inv_S = inv_S;
    hipLaunchKernelGGL((train_head_kernel<true, SKIP>), dim3((B + 3) / 4, M), dim3(256), 0, st, h);
    if ((rc = launch_status())) return rc;
    if (fc2) {
        // dA1[b, i] = (sum_o dA2[b, o] Wm[o, i]) act'1[b, i]
        GemmProb p = {};
        p.A = ws->dA2; p.a_m = H; p.a_k = 1; p.a_mem = bh; p.B = P + L.s[2].off; p.b_n = 1; p.b_k = H; p.b_mem = ps; p.M = B; p.N = H; p.K = H;
        p.ones_n = -1; p.Cout = ws->dA1; p.ldc = H; p.c_mem = bh; p.Dmul = ws->dact1; p.epi = EPI_MUL;
        g.p[0] = p;
        if ((rc = gemm_launch<true, SKIP>(g, M, st))) return rc;
    }
    return RBNN_OK;
}

// grad = dL/dP of every tensor of every member (the biases as column sums): one launch
template <bool SKIP = false>
inline int lockstep_weight_grads(const rbnn_nn_train_net* net, const LockstepBatch& b, const rbnn_nn_train_ws* ws, hipStream_t st) {
    int rc = check_members(net);
    if (rc) return rc;
    if (!ws || !net->grad || (SKIP && !b.counts)) return RBNN_ERR_NULL;
    if ((rc = check_batch(net, b))) return rc;
    const bool fc2 = net->arch == RBNN_ARCH_FC2;
    if (!ws->hid1 || !ws->dA1 || !ws->dZ) return RBNN_ERR_NULL;
    if (fc2 && (!ws->hid2 || !ws->dA2)) return RBNN_ERR_NULL;
    const Layout L = layout_of(*net);
    const int D = net->in_features, H = net->hidden, C = net->n_classes, B = b.B;
    const long long ps = net->member_stride, bh = (long long)B * H;
    float* G = net->grad;
    GemmArgs g = {};
    g.n_prob = fc2 ? 3 : 2; g.counts = b.counts; g.per = 1;
    g.p[0] = wgrad_prob(ws->dA1, H, b.X, b.ldx, 0, H, D, B, G + L.s[0].off, G + L.s[1].off, ps);
    g.p[0].b_idx = b.rows; g.p[0].idx_mem = B; g.p[0].idx_max = b.n_rows - 1;
    if (fc2) g.p[1] = wgrad_prob(ws->dA2, H, ws->hid1, H, bh, H, H, B, G + L.s[2].off, G + L.s[3].off, ps);
    g.p[g.n_prob - 1] = wgrad_prob(ws->dZ, RBNN_CPAD, fc2 ? ws->hid2 : ws->hid1, H, bh, C, H, B, G + L.s[L.n - 2].off, G + L.s[L.n - 1].off, ps);
    return gemm_launch<true, SKIP>(g, net->n_members, st);
}
#endif  // RBNN_TRAIN_LOCKSTEP

}  // namespace
