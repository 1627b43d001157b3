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
// The parameter layout, the activations, Adam and the block reductions are rbnn_train_core.hpp; the Adam + KL kernel and the
// step's sums are rbnn_svi_step.hpp (shared with the guides in lockstep; here the Single view); the forward / backward GEMM and head kernels
// are rbnn_train_gemm.hpp, instantiated here for a single net (LOCKSTEP = false; inv_S = 1: the CE is summed).
#include "rbnn_train_gemm.hpp"
#include "rbnn_svi_step.hpp"

namespace {

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
// One block: stats[0] = CE + KL of the step, stats[1] += it, stats[2] += #(argmax Psum == label).  Fixed-order sums in fp64 (svi_step_sums).
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
    svi_step_sums<false>(a.kl_part, a.n_part, a.ce, a.B, a.Psum, a.ldp, a.C, a.labels, nullptr, 0, red, cnt);
    if (threadIdx.x == 0) {
        a.stats[0] = red[0];
        a.stats[1] += red[0];
        a.stats[2] += cnt[0];
    }
}

}  // namespace

extern "C" {

int64_t rbnn_svi_train_sizes(const rbnn_svi_train_net* net, int64_t* n_partials) {
    const int rc = check_net(net);
    if (rc) return rc;
    const Layout L = layout_of(*net);
    if (n_partials) *n_partials = blocks_for(L.n_quads);
    return L.n_params;
}

int rbnn_svi_train_draw(const rbnn_svi_train_net* net, uint64_t key, uint32_t draw_id, void* stream) {
    int rc = check_net(net);
    if (rc) return rc;
    if (!net->loc || !net->sigma || !net->W) return RBNN_ERR_NULL;
    const Layout L = layout_of(*net);
    hipLaunchKernelGGL(train_draw_kernel, dim3(blocks_for(L.n_quads)), dim3(ELT_THREADS), 0, (hipStream_t)stream,
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
    g.p[0] = fwd_prob(X, ldx, 0, W + L.s[0].off, W + L.s[1].off, 0, B, H, D, ws->hid1, ws->dact1, act);
    if ((rc = gemm_launch<false>(g, 1, st))) return rc;
    if (fc2) {
        g.p[0] = fwd_prob(ws->hid1, H, 0, W + L.s[2].off, W + L.s[3].off, 0, B, H, H, ws->hid2, ws->dact2, act);
        if ((rc = gemm_launch<false>(g, 1, st))) return rc;
    }
    HeadArgs h = {};
    h.Hl = fc2 ? ws->hid2 : ws->hid1; h.Dl = fc2 ? ws->dact2 : ws->dact1;
    h.W2 = W + L.s[L.n - 2].off; h.b2 = W + L.s[L.n - 1].off; h.labels = labels;
    h.dZ = ws->dZ; h.ce = ws->ce; h.dA = fc2 ? ws->dA2 : ws->dA1; h.B = B; h.H = H; h.C = C; h.inv_S = 1.f;
    hipLaunchKernelGGL((train_head_kernel<false, false>), dim3((B + 3) / 4), dim3(256), 0, st, h);
    if ((rc = launch_status())) return rc;
    if (fc2) {
        // dA1[b, i] = (sum_o dA2[b, o] Wm[o, i]) act'1[b, i]
        GemmProb p = {};
        p.A = ws->dA2; p.a_m = H; p.a_k = 1; p.B = W + L.s[2].off; p.b_n = 1; p.b_k = H; p.M = B; p.N = H; p.K = H; p.ones_n = -1;
        p.Cout = ws->dA1; p.ldc = H; p.Dmul = ws->dact1; p.epi = EPI_MUL;
        g.p[0] = p;
        if ((rc = gemm_launch<false>(g, 1, st))) return rc;
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
    g.p[0] = wgrad_prob(ws->dA1, H, X, ldx, 0, H, D, B, G + L.s[0].off, G + L.s[1].off, 0);
    if (fc2) g.p[1] = wgrad_prob(ws->dA2, H, ws->hid1, H, 0, H, H, B, G + L.s[2].off, G + L.s[3].off, 0);
    g.p[g.n_prob - 1] = wgrad_prob(ws->dZ, RBNN_CPAD, fc2 ? ws->hid2 : ws->hid1, H, 0, C, H, B, G + L.s[L.n - 2].off, G + L.s[L.n - 1].off, 0);
    return gemm_launch<false>(g, 1, (hipStream_t)stream);
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
    a.s = adam_scalars(step, lr, beta1, beta2, adam_eps);
    hipLaunchKernelGGL(adam_kernel<Single>, dim3(blocks_for(a.L.n_quads)), dim3(ELT_THREADS), 0, (hipStream_t)stream, a);
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
