// rbnn_svi_lockstep.hip — K SVI guides of ONE net shape trained in lockstep (the step of rbnn_train.hip for every guide in one set of launches;
// the guide is grid dimension y, as the member is in rbnn_nn_train.hip and the chain in rbnn_hmc.hip):
//
//      rbnn_svi_multi_draw       W[k] = loc[k] + sigma[k] * eps(keys[k], draw_id)           what rbnn_svi_train_draw writes for that key
//                                   (svils_draw_kernel<GuideMajor>, rbnn_svi_step.hpp)
//      rbnn_svi_multi_gradient   lockstep_forward(inv_S = 1) + lockstep_weight_grads on the net whose P is W (rbnn_train_gemm.hpp, SKIP form)
//      rbnn_svi_multi_adam_step  adam_kernel<GuideMajor> (rbnn_svi_step.hpp): per-guide key and learning rate, KL partials [K, part_stride]
//      rbnn_svi_multi_accuracy   10 weight sets per guide from the live loc / sigma (rbnn_svi_draw's generator at sample s), the hidden layers of
//                                   the K * 10 nets through the GEMM kernel, then softmax and the sum over the samples per (guide, point)
//      rbnn_svi_multi_finalize   svils_finalize_kernel<true> (rbnn_svi_step.hpp), one block per guide: the step's loss over its counts[k] points,
//                                   the running sums, and the epoch's end on the device
//
// A guide with counts[k] == 0 has finished its epochs: every kernel returns at once for it and nothing of its state is written.  No atomics, no sum
// across guides, and a guide's blocks and tiles do not depend on K: guide k is bit-identical to rbnn_train.hip's entry points running it alone
// (the accuracy forward's logits come from another tile plan than rbnn_fc_forward's: equal within the forward bar, not bit for bit).
#define RBNN_TRAIN_LOCKSTEP
#include "rbnn_train_gemm.hpp"
#include "rbnn_svi_step.hpp"

namespace {

constexpr int ACC_S = RBNN_SVI_MULTI_ACC_SAMPLES;

// ---------------------------------------------------------------------------------------------------
// The accuracy forward's output layer: one wave per (guide, point).  For each of the guide's ACC_S nets z = H W2^T + b2, p = softmax(z);
// Psum[k, b, :] = sum_s p in the order s = 0, 1, ... (what rbnn_reduce_samples sums with scale 1).
// ---------------------------------------------------------------------------------------------------
struct AccHeadArgs {
    const float* Hl;                          // [K * ACC_S, B, H] last hidden layer
    const float *W2, *b2;                     // of member 0 of the [K * ACC_S, p_mem] weight stack
    long long p_mem;
    const int32_t* counts;
    float* Psum;                              // [K, B, RBNN_CPAD]
    int B, H, C;
};

__global__ void __launch_bounds__(256) svils_acc_head_kernel(const AccHeadArgs a) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, k = blockIdx.y;
    if (b >= a.counts[k]) return;                                      // behind the guide's points (all of them once it has finished)
    float ps[RBNN_CPAD];
#pragma unroll
    for (int c = 0; c < RBNN_CPAD; ++c) ps[c] = 0.f;
    for (int s = 0; s < ACC_S; ++s) {
        const long long mem = (long long)k * ACC_S + s;
        const float* const W2 = a.W2 + mem * a.p_mem;
        const float* const b2 = a.b2 + mem * a.p_mem;
        const float* const hrow = a.Hl + (mem * a.B + b) * a.H;
        float z[RBNN_CPAD];
#pragma unroll
        for (int c = 0; c < RBNN_CPAD; ++c) z[c] = 0.f;
        for (int h = lane; h < a.H; h += 64) {
            const float hv = hrow[h];
#pragma unroll
            for (int c = 0; c < RBNN_CPAD; ++c) if (c < a.C) z[c] = fmaf(hv, W2[(long long)c * a.H + h], z[c]);
        }
        float m = -INFINITY;
#pragma unroll
        for (int c = 0; c < RBNN_CPAD; ++c) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) z[c] += __shfl_xor(z[c], off, 64);
            if (c < a.C) { z[c] += b2[c]; m = fmaxf(m, z[c]); }
        }
        float den = 0.f;
#pragma unroll
        for (int c = 0; c < RBNN_CPAD; ++c) { z[c] = (c < a.C) ? expf(z[c] - m) : 0.f; den += z[c]; }
#pragma unroll
        for (int c = 0; c < RBNN_CPAD; ++c) ps[c] += z[c] / den;
    }
    if (lane == 0) {
        float* const out = a.Psum + ((long long)k * a.B + b) * RBNN_CPAD;
#pragma unroll
        for (int c = 0; c < RBNN_CPAD; ++c) if (c < a.C) out[c] = ps[c];
    }
}

int check_guides(const rbnn_nn_train_net* net, const rbnn_svi_multi* g, const Layout& L) {
    if (!g) return RBNN_ERR_NULL;
    if (net->member_stride < L.n_params || g->part_stride < (long long)blocks_for(L.n_quads)) return RBNN_ERR_SHAPE;
    return RBNN_OK;
}

// the grid's y limit holds for the K * ACC_S nets of the accuracy forward, so every entry point takes at most 65535 / ACC_S guides
int check_svils(const rbnn_nn_train_net* net) {
    const int rc = check_net(net);
    if (rc) return rc;
    return (net->n_members < 1 || net->n_members > 65535 / ACC_S) ? RBNN_ERR_SHAPE : RBNN_OK;
}

}  // namespace

extern "C" {

int rbnn_svi_multi_draw(const rbnn_nn_train_net* net, const rbnn_svi_multi* guides, const int32_t* counts, uint32_t draw_id, void* stream) {
    int rc = check_svils(net);
    if (rc) return rc;
    if (!guides || !counts || !net->P || !guides->loc || !guides->sigma || !guides->keys) return RBNN_ERR_NULL;
    const Layout L = layout_of(*net);
    if ((rc = check_guides(net, guides, L))) return rc;
    return guides_draw<GuideMajor>(L, *guides, net->P, counts, net->n_members, 1, net->member_stride, 0, draw_id, (hipStream_t)stream);
}

int rbnn_svi_multi_gradient(const rbnn_nn_train_net* net, const float* X, int32_t ldx, int32_t n_rows, const int32_t* labels,
                               const int32_t* rows, const int32_t* counts, int32_t n_points, const rbnn_nn_train_ws* ws, void* stream) {
    int rc = check_svils(net);
    if (rc) return rc;
    if (!rows || !counts) return RBNN_ERR_NULL;
    const LockstepBatch b = {X, ldx, n_rows, labels, rows, counts, n_points};
    if ((rc = lockstep_forward<true>(net, b, ws, 1.f, (hipStream_t)stream))) return rc;
    return lockstep_weight_grads<true>(net, b, ws, (hipStream_t)stream);
}

int rbnn_svi_multi_adam_step(const rbnn_nn_train_net* net, const rbnn_svi_multi* guides, const int32_t* counts, uint32_t draw_id,
                                int64_t step, const double* lr, double beta1, double beta2, double adam_eps, void* stream) {
    int rc = check_svils(net);
    if (rc) return rc;
    if (!guides || !counts || !lr || !net->grad) return RBNN_ERR_NULL;
    const rbnn_svi_multi& g = *guides;
    if (!g.loc || !g.raw || !g.sigma || !g.m_loc || !g.v_loc || !g.m_raw || !g.v_raw || !g.kl_part || !g.keys) return RBNN_ERR_NULL;
    if (step < 1) return RBNN_ERR_SHAPE;
    const Layout L = layout_of(*net);
    if ((rc = check_guides(net, guides, L))) return rc;
    return guides_adam_step<GuideMajor>(L, g, net->grad, counts, net->n_members, net->member_stride, draw_id, step, lr, beta1, beta2, adam_eps,
                                        (hipStream_t)stream);
}

int rbnn_svi_multi_accuracy(const rbnn_nn_train_net* net, const rbnn_svi_multi* guides, const float* X, int32_t ldx, int32_t n_rows,
                               const int32_t* rows, const int32_t* counts, int32_t n_points, uint64_t key_xor, uint32_t draw_id,
                               const rbnn_svi_multi_acc* acc, void* stream) {
    int rc = check_svils(net);
    if (rc) return rc;
    if (!guides || !X || !rows || !counts || !acc || !guides->loc || !guides->sigma || !guides->keys) return RBNN_ERR_NULL;
    if (!acc->W || !acc->hid1 || !acc->dact || !acc->Psum) return RBNN_ERR_NULL;
    const bool fc2 = net->arch == RBNN_ARCH_FC2;
    if (fc2 && !acc->hid2) return RBNN_ERR_NULL;
    const Layout L = layout_of(*net);
    if ((rc = check_guides(net, guides, L))) return rc;
    const int D = net->in_features, H = net->hidden, C = net->n_classes, B = n_points, act = net->activation, K = net->n_members;
    if (B < 1 || n_rows < 1 || ldx < D || (long long)K * ACC_S * B * H > (1LL << 40)) return RBNN_ERR_SHAPE;
    const long long ps = net->member_stride, bh = (long long)B * H;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = guides_draw<GuideMajor>(L, *guides, acc->W, counts, K, ACC_S, ps, key_xor, draw_id, st))) return rc;
    const float* W = acc->W;
    GemmArgs g = {};
    g.n_prob = 1; g.counts = counts; g.per = ACC_S;
    g.p[0] = fwd_prob(X, ldx, 0, W + L.s[0].off, W + L.s[1].off, ps, B, H, D, acc->hid1, acc->dact, act);
    g.p[0].a_idx = rows; g.p[0].idx_mem = B; g.p[0].idx_max = n_rows - 1;
    if ((rc = gemm_launch<true, true>(g, K * ACC_S, st))) return rc;
    if (fc2) {
        g.p[0] = fwd_prob(acc->hid1, H, bh, W + L.s[2].off, W + L.s[3].off, ps, B, H, H, acc->hid2, acc->dact, act);
        if ((rc = gemm_launch<true, true>(g, K * ACC_S, st))) return rc;
    }
    AccHeadArgs h = {};
    h.Hl = fc2 ? acc->hid2 : acc->hid1; h.W2 = W + L.s[L.n - 2].off; h.b2 = W + L.s[L.n - 1].off; h.p_mem = ps; h.counts = counts;
    h.Psum = acc->Psum; h.B = B; h.H = H; h.C = C;
    hipLaunchKernelGGL(svils_acc_head_kernel, dim3((B + 3) / 4, K), dim3(256), 0, st, h);
    return launch_status();
}

int rbnn_svi_multi_finalize(const rbnn_nn_train_net* net, const rbnn_svi_multi* guides, const float* ce, const float* Psum,
                               const int32_t* labels, int32_t n_rows, const int32_t* rows, const int32_t* counts, int32_t n_points,
                               const int32_t* epoch_slot, double* epoch_log, int32_t log_rows, void* stream) {
    int rc = check_svils(net);
    if (rc) return rc;
    if (!guides || !ce || !rows || !counts || !guides->kl_part || !guides->stats || (Psum && !labels) || (epoch_slot && !epoch_log)) return RBNN_ERR_NULL;
    const Layout L = layout_of(*net);
    if ((rc = check_guides(net, guides, L))) return rc;
    if (n_points < 1 || n_rows < 1 || log_rows < 0) return RBNN_ERR_SHAPE;
    GuidesFinalArgs a = {};
    a.kl_part = guides->kl_part; a.ce = ce; a.Psum = Psum; a.labels = labels; a.rows = rows; a.live = counts; a.epoch_slot = epoch_slot;
    a.stats = guides->stats; a.epoch_log = epoch_log; a.part_stride = guides->part_stride; a.n_part = (int)blocks_for(L.n_quads);
    a.B = n_points; a.C = net->n_classes; a.idx_max = n_rows - 1; a.log_rows = log_rows;
    hipLaunchKernelGGL(svils_finalize_kernel<true>, dim3(net->n_members), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status();
}

}  // extern "C"
