// rbnn_train_gemm.hpp — the forward / backward of an fc / fc2 net on the fp32 MFMA, shared by the units that launch it (rbnn_train.hip,
// rbnn_nn_train.hip, rbnn_hmc.hip, rbnn_svi_lockstep.hip): one strided GEMM kernel and one output-layer + loss kernel, for M independent members in lockstep (grid
// dimension y), and the host side of the lockstep forward / weight gradients.
// Both bodies are templates on LOCKSTEP.  false is a single net: member 0, no index arrays — the member strides, a_idx / b_idx / rows and the
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

// The kernels' text is rbnn_train_kernels.inc, included below once per form: train_gemm_kernel / train_head_kernel, and train_gemm_skip_kernel /
// train_head_skip_kernel, which leave out a finished member (templates: only the unit that launches them, rbnn_svi_lockstep.hip, has them).

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

#define RBNN_GEMM_KERNEL train_gemm_kernel
#define RBNN_HEAD_KERNEL train_head_kernel
#define RBNN_KERNELS_SKIP false
#include "rbnn_train_kernels.inc"
#undef RBNN_GEMM_KERNEL
#undef RBNN_HEAD_KERNEL
#undef RBNN_KERNELS_SKIP
// SKIP (LOCKSTEP with counts only): a member, or a group of `per` members, with counts == 0 has finished; its blocks return at once and its
// workspaces keep what they held
#define RBNN_GEMM_KERNEL train_gemm_skip_kernel
#define RBNN_HEAD_KERNEL train_head_skip_kernel
#define RBNN_KERNELS_SKIP true
#include "rbnn_train_kernels.inc"
#undef RBNN_GEMM_KERNEL
#undef RBNN_HEAD_KERNEL
#undef RBNN_KERNELS_SKIP

template <bool LOCKSTEP, bool SKIP = false> int gemm_launch(GemmArgs& g, int members, hipStream_t st) {
    if (SKIP && (!g.counts || g.per < 1)) return RBNN_ERR_NULL;
    int tiles = 0;
    for (int i = 0; i < g.n_prob; ++i) {
        GemmProb& p = g.p[i];
        p.tiles_n = (p.N + GT - 1) / GT;
        p.first_tile = tiles;
        tiles += p.tiles_n * ((p.M + GT - 1) / GT);
    }
    if constexpr (SKIP) hipLaunchKernelGGL(train_gemm_skip_kernel<LOCKSTEP>, dim3(tiles, members), dim3(256), 0, st, g);
    else hipLaunchKernelGGL(train_gemm_kernel<LOCKSTEP>, dim3(tiles, LOCKSTEP ? members : 1), dim3(256), 0, st, g);
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
    if constexpr (SKIP) hipLaunchKernelGGL(train_head_skip_kernel<true>, dim3((B + 3) / 4, M), dim3(256), 0, st, h);
    else hipLaunchKernelGGL(train_head_kernel<true>, dim3((B + 3) / 4, M), dim3(256), 0, st, h);
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
