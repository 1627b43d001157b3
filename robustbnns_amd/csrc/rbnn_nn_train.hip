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
// The parameter layout (one member's: Layout::s[i].off), the activations, Adam and the fp64 tree are rbnn_train_core.hpp; the GEMM and head
// kernels are rbnn_train_gemm.hpp.
#include "rbnn_train_gemm.hpp"

namespace {

// ---------------------------------------------------------------------------------------------------
// Adam (torch.optim.Adam, single-tensor, defaults but lr), one thread per parameter of a member:
//   m = m + (1 - b1)(g - m),  v = b2 v + (1 - b2) g^2,  p += (-step_size m) / (sqrt(v) / bc2_sqrt + eps_adam)
// ---------------------------------------------------------------------------------------------------
struct AdamArgs {
    float *P, *m, *v;
    const float* grad;
    long long n_params, member_stride;
    AdamScalars s;
};

__global__ void __launch_bounds__(ELT_THREADS) nn_adam_kernel(const AdamArgs a) {
    const long long i = (long long)blockIdx.x * ELT_THREADS + threadIdx.x;
    if (i >= a.n_params) return;
    const long long e = (long long)blockIdx.y * a.member_stride + i;
    float p = a.P[e], m = a.m[e], v = a.v[e];
    adam_one(p, m, v, a.grad[e], a.s);
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
    block_tree64(red, cnt);
    if (t == 0) {
        double* const st = a.stats + 3 * (long long)blockIdx.x;
        const double loss = (double)(float)(red[0] / (double)a.B);      // loss.item() of an fp32 mean
        st[0] = loss;
        st[1] += loss;
        st[2] += cnt[0];
    }
}

int check_members(const rbnn_nn_train_net* n) {
    const int rc = check_net(n);
    if (rc) return rc;
    return (n->n_members < 1 || n->n_members > 65535) ? RBNN_ERR_SHAPE : RBNN_OK;      // the member is grid dimension y
}

int check_batch(const rbnn_nn_train_net* n, const float* X, int ldx, int n_rows, const int32_t* rows, int B) {
    if (!X) return RBNN_ERR_NULL;
    if (B < 1 || n_rows < 1 || ldx < n->in_features) return RBNN_ERR_SHAPE;
    if (!rows && B > n_rows) return RBNN_ERR_SHAPE;                                // rows 0..B-1 of X
    if ((long long)n->n_members * B * n->hidden > (1LL << 40) || n->member_stride < layout_of(*n).n_params) return RBNN_ERR_SHAPE;
    return RBNN_OK;
}

}  // namespace

extern "C" {

int64_t rbnn_nn_train_sizes(const rbnn_nn_train_net* net) {
    const int rc = check_members(net);
    if (rc) return rc;
    return layout_of(*net).n_params;
}

int rbnn_nn_train_forward(const rbnn_nn_train_net* net, const float* X, int32_t ldx, int32_t n_rows, const int32_t* labels, const int32_t* rows,
                          int32_t n_points, const rbnn_nn_train_ws* ws, void* stream) {
    int rc = check_members(net);
    if (rc) return rc;
    if (!labels || !ws || !net->P) return RBNN_ERR_NULL;
    if ((rc = check_batch(net, X, ldx, n_rows, rows, n_points))) return rc;
    const bool fc2 = net->arch == RBNN_ARCH_FC2;
    if (!ws->hid1 || !ws->dact1 || !ws->dA1 || !ws->dZ || !ws->ce || !ws->correct) return RBNN_ERR_NULL;
    if (fc2 && (!ws->hid2 || !ws->dact2 || !ws->dA2)) return RBNN_ERR_NULL;
    const Layout L = layout_of(*net);
    const int D = net->in_features, H = net->hidden, C = net->n_classes, B = n_points, act = net->activation, M = net->n_members;
    const long long ps = net->member_stride, bh = (long long)B * H;
    hipStream_t st = (hipStream_t)stream;
    const float* P = net->P;
    GemmArgs g = {};
    g.n_prob = 1;
    g.p[0] = fwd_prob(X, ldx, 0, P + L.s[0].off, P + L.s[1].off, ps, B, H, D, ws->hid1, ws->dact1, act);
    g.p[0].a_idx = rows; g.p[0].idx_mem = B; g.p[0].idx_max = n_rows - 1;
    if ((rc = gemm_launch<true>(g, M, st))) return rc;
    if (fc2) {
        g.p[0] = fwd_prob(ws->hid1, H, bh, P + L.s[2].off, P + L.s[3].off, ps, B, H, H, ws->hid2, ws->dact2, act);
        if ((rc = gemm_launch<true>(g, M, st))) return rc;
    }
    HeadArgs h = {};
    h.Hl = fc2 ? ws->hid2 : ws->hid1; h.Dl = fc2 ? ws->dact2 : ws->dact1;
    h.W2 = P + L.s[L.n - 2].off; h.b2 = P + L.s[L.n - 1].off; h.p_mem = ps; h.labels = labels; h.rows = rows; h.idx_max = n_rows - 1;
    h.dZ = ws->dZ; h.ce = ws->ce; h.correct = ws->correct; h.dA = fc2 ? ws->dA2 : ws->dA1; h.B = B; h.H = H; h.C = C;
    h.inv_S = 1.f / (float)B;
    hipLaunchKernelGGL(train_head_kernel<true>, dim3((B + 3) / 4, M), dim3(256), 0, st, h);
    if ((rc = launch_status())) return rc;
    if (fc2) {
        // dA1[b, i] = (sum_o dA2[b, o] Wm[o, i]) act'1[b, i]
        GemmProb p = {};
        p.A = ws->dA2; p.a_m = H; p.a_k = 1; p.a_mem = bh; p.B = P + L.s[2].off; p.b_n = 1; p.b_k = H; p.b_mem = ps; p.M = B; p.N = H; p.K = H;
        p.ones_n = -1; p.Cout = ws->dA1; p.ldc = H; p.c_mem = bh; p.Dmul = ws->dact1; p.epi = EPI_MUL;
        g.p[0] = p;
        if ((rc = gemm_launch<true>(g, M, st))) return rc;
    }
    return RBNN_OK;
}

int rbnn_nn_weight_grads(const rbnn_nn_train_net* net, const float* X, int32_t ldx, int32_t n_rows, const int32_t* rows, int32_t n_points,
                         const rbnn_nn_train_ws* ws, void* stream) {
    int rc = check_members(net);
    if (rc) return rc;
    if (!ws || !net->grad) return RBNN_ERR_NULL;
    if ((rc = check_batch(net, X, ldx, n_rows, rows, n_points))) return rc;
    const bool fc2 = net->arch == RBNN_ARCH_FC2;
    if (!ws->hid1 || !ws->dA1 || !ws->dZ) return RBNN_ERR_NULL;
    if (fc2 && (!ws->hid2 || !ws->dA2)) return RBNN_ERR_NULL;
    const Layout L = layout_of(*net);
    const int D = net->in_features, H = net->hidden, C = net->n_classes, B = n_points;
    const long long ps = net->member_stride, bh = (long long)B * H;
    float* G = net->grad;
    GemmArgs g = {};
    g.n_prob = fc2 ? 3 : 2;
    g.p[0] = wgrad_prob(ws->dA1, H, X, ldx, 0, H, D, B, G + L.s[0].off, G + L.s[1].off, ps);
    g.p[0].b_idx = rows; g.p[0].idx_mem = B; g.p[0].idx_max = n_rows - 1;
    if (fc2) g.p[1] = wgrad_prob(ws->dA2, H, ws->hid1, H, bh, H, H, B, G + L.s[2].off, G + L.s[3].off, ps);
    g.p[g.n_prob - 1] = wgrad_prob(ws->dZ, RBNN_CPAD, fc2 ? ws->hid2 : ws->hid1, H, bh, C, H, B, G + L.s[L.n - 2].off, G + L.s[L.n - 1].off, ps);
    return gemm_launch<true>(g, net->n_members, (hipStream_t)stream);
}

int rbnn_nn_adam_step(const rbnn_nn_train_net* net, int64_t step, double lr, double beta1, double beta2, double adam_eps, void* stream) {
    int rc = check_members(net);
    if (rc) return rc;
    if (!net->P || !net->m || !net->v || !net->grad) return RBNN_ERR_NULL;
    AdamArgs a = {};
    a.n_params = layout_of(*net).n_params;
    if (step < 1 || net->member_stride < a.n_params) return RBNN_ERR_SHAPE;
    a.P = net->P; a.m = net->m; a.v = net->v; a.grad = net->grad; a.member_stride = net->member_stride;
    a.s = adam_scalars(step, lr, beta1, beta2, adam_eps);
    hipLaunchKernelGGL(nn_adam_kernel, dim3(blocks_for(a.n_params), net->n_members), dim3(ELT_THREADS), 0,
                       (hipStream_t)stream, a);
    return launch_status();
}

int rbnn_nn_train_finalize(const rbnn_nn_train_net* net, const rbnn_nn_train_ws* ws, int32_t n_points, double* stats, void* stream) {
    int rc = check_members(net);
    if (rc) return rc;
    if (!ws || !ws->ce || !ws->correct || !stats) return RBNN_ERR_NULL;
    if (n_points < 1) return RBNN_ERR_SHAPE;
    FinalArgs a = {ws->ce, ws->correct, stats, n_points};
    hipLaunchKernelGGL(nn_finalize_kernel, dim3(net->n_members), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status();
}

}  // extern "C"
