// rbnn_svi_step.hpp — the SVI step's own device code, each kernel written once for the single trainers (rbnn_train.hip, rbnn_conv_train.hip) and
// for K guides in lockstep in both buffer layouts (rbnn_svi_lockstep.hip: guide-major; rbnn_conv_train.hip and, for Adam + KL, rbnn_svi.hip:
// tensor-major): the Adam + KL kernel, the guides' draw, the guides' finalize and the fixed-order fp64 sums of a step.  The kernels are
// templates (as the GEMM and head kernels of rbnn_train_gemm.hpp): a unit emits only the instances it launches.
#pragma once
#include "rbnn_train_core.hpp"

namespace {

// ---------------------------------------------------------------------------------------------------
// A view: base(m, M, stride, sg) is where member m of M's segment sg starts in a per-parameter buffer.  lockstep = false compiles the member
// index, the key / learning-rate arrays and the skip out of adam_kernel.
//   Single       one guide: the segment's offset
//   GuideMajor   [M, stride]: member m's parameters lie together (rbnn_svi_multi_*)
//   TensorMajor  six blocks [M, size of tensor] in state_dict order (rbnn_conv_svi_guides_*: the stacks the conv forward of M nets reads)
// ---------------------------------------------------------------------------------------------------
struct Single {
    static constexpr bool lockstep = false;
    static __device__ __forceinline__ long long base(unsigned, int, long long, const Seg& sg) { return sg.off; }
};
struct GuideMajor {
    static constexpr bool lockstep = true;
    static __device__ __forceinline__ long long base(unsigned m, int, long long stride, const Seg& sg) { return m * stride + sg.off; }
};
struct TensorMajor {
    static constexpr bool lockstep = true;
    static __device__ __forceinline__ long long base(unsigned m, int M, long long, const Seg& sg) {
        return M * sg.off + m * ((long long)sg.rows * sg.cols);
    }
};

// ---------------------------------------------------------------------------------------------------
// Adam (torch.optim.Adam, single-tensor, defaults but lr) on loc and raw scale, one thread per quad of a tensor:
//   g_loc = dCE/dw + loc,   g_raw = (dCE/dw eps + sigma - 1/sigma) sigmoid(raw)      (TraceMeanField's analytic KL against N(0, 1))
//   m = m + (1 - b1)(g - m),  v = b2 v + (1 - b2) g^2,  p += (-step_size m) / (sqrt(v) / bc2_sqrt + eps_adam),  sigma = softplus(raw)
// and the KL of the PRE-update parameters, -log sigma + (sigma^2 + loc^2) / 2 - 1/2, summed per block in a fixed tree order.
// A lockstep view: guide blockIdx.y of n_members under its own key and learning rate, KL partials [K, part_stride]; a guide with live[k] == 0
// has finished and is neither read nor written.  step_size = (float)(lr[k] / bc1) with bc1 = 1 - beta1^t formed by the host in double: the
// IEEE double division rounds as the host's does, so the value is adam_scalars()'s for that lr, bit for bit.
// ---------------------------------------------------------------------------------------------------
struct AdamArgs {
    Layout L;
    float *loc, *raw, *sigma, *m_loc, *v_loc, *m_raw, *v_raw;
    const float* grad;
    float* kl_part;
    unsigned long long key;
    uint32_t draw_id;
    AdamScalars s;
    // lockstep views only
    const unsigned long long* keys;
    const int32_t* live;
    const double* lr;
    double bc1;
    long long member_stride, part_stride;
    int n_members;
};

template <class View> __global__ void __launch_bounds__(ELT_THREADS) adam_kernel(const AdamArgs a) {
    constexpr bool LOCKSTEP = View::lockstep;
    __shared__ float red[ELT_THREADS];
    const long long q = (long long)blockIdx.x * ELT_THREADS + threadIdx.x;
    float kl = 0.f;
    if constexpr (LOCKSTEP) { if (a.live[blockIdx.y] == 0) return; }
    if (q < a.L.n_quads) {
        const Seg sg = a.L.s[seg_of(a.L, q)];
        const int Q = (sg.cols + 3) >> 2;
        const long long ql = q - sg.first_quad;
        const int r = (int)(ql / Q), c4 = (int)(ql % Q);
        const unsigned long long key = LOCKSTEP ? a.keys[blockIdx.y] : a.key;
        const Rng rng = {(uint32_t)key, (uint32_t)(key >> 32), 0u, a.draw_id};
        float eps[4];
        rng.quad(sg.tensor_id, (uint32_t)(r * Q + c4), eps);
        AdamScalars sl = a.s;
        if constexpr (LOCKSTEP) sl.step_size = (float)(a.lr[blockIdx.y] / a.bc1);
        const AdamScalars& s = LOCKSTEP ? sl : a.s;
        const long long base = View::base(blockIdx.y, a.n_members, a.member_stride, sg) + (long long)r * sg.cols + 4 * c4;
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
            adam_one(mu, ml, vl, gl, s);
            adam_one(rw, mr, vr, gr, s);
            a.loc[e] = mu; a.raw[e] = rw; a.sigma[e] = softplus_f(rw);
            a.m_loc[e] = ml; a.v_loc[e] = vl; a.m_raw[e] = mr; a.v_raw[e] = vr;
        }
    }
    block_sum_to(kl, red, a.kl_part + (LOCKSTEP ? blockIdx.y * a.part_stride : 0));
}

// the K guides' Adam + KL step, one launch: g's buffers and grad in the view's layout, each guide under its key, lr[k] and live[k]
template <class View>
int guides_adam_step(const Layout& L, const rbnn_svi_multi& g, const float* grad, const int32_t* live, int K, long long member_stride,
                     uint32_t draw_id, int64_t step, const double* lr, double beta1, double beta2, double adam_eps, hipStream_t st) {
    AdamArgs a = {};
    a.L = L;
    a.loc = g.loc; a.raw = g.raw; a.sigma = g.sigma; a.m_loc = g.m_loc; a.v_loc = g.v_loc; a.m_raw = g.m_raw; a.v_raw = g.v_raw;
    a.grad = grad; a.kl_part = g.kl_part; a.draw_id = draw_id;
    a.s = adam_scalars(step, 1.0, beta1, beta2, adam_eps);            // step_size is formed per guide in the kernel from lr[k] and bc1
    a.keys = (const unsigned long long*)g.keys; a.live = live; a.lr = lr; a.bc1 = 1.0 - pow(beta1, (double)step);
    a.member_stride = member_stride; a.part_stride = g.part_stride; a.n_members = K;
    hipLaunchKernelGGL(adam_kernel<View>, dim3(blocks_for(L.n_quads), K), dim3(ELT_THREADS), 0, st, a);
    return launch_status();
}

// ---------------------------------------------------------------------------------------------------
// The guides' draw, one thread per quad of weight set blockIdx.y = guide * per + sample of K * per sets (per = 1: the training draw at sample
// 0; per > 1: the stack of an accuracy forward, in the view's layout over the sets): W = loc[k] + sigma[k] * eps(keys[k] ^ key_xor, sample,
// draw id), draw_quad's bits.  A guide with live[k] == 0 is skipped, the whole block.
// ---------------------------------------------------------------------------------------------------
struct GuidesDrawArgs {
    Layout L;
    const float *loc, *sigma;
    float* W;
    const unsigned long long* keys;
    const int32_t* live;
    unsigned long long key_xor;
    uint32_t draw_id;
    int per, n_members;
    long long member_stride;
};

template <class View> __global__ void __launch_bounds__(ELT_THREADS) svils_draw_kernel(const GuidesDrawArgs a) {
    const int k = blockIdx.y / a.per, s = blockIdx.y % a.per;
    if (a.live[k] == 0) return;
    const long long q = (long long)blockIdx.x * ELT_THREADS + threadIdx.x;
    if (q >= a.L.n_quads) return;
    const Seg sg = a.L.s[seg_of(a.L, q)];
    const int Q = (sg.cols + 3) >> 2;
    const long long ql = q - sg.first_quad;
    const int r = (int)(ql / Q), c4 = (int)(ql % Q);
    const unsigned long long key = a.keys[k] ^ a.key_xor;
    const Rng rng = {(uint32_t)key, (uint32_t)(key >> 32), (uint32_t)s, a.draw_id};
    const long long go = View::base(k, a.n_members, a.member_stride, sg);
    float w[4];
    draw_quad(rng, sg.tensor_id, a.loc + go, a.sigma + go, r, c4, sg.cols, w);
    float* const out = a.W + View::base(blockIdx.y, a.n_members * a.per, a.member_stride, sg) + (long long)r * sg.cols + 4 * c4;
#pragma unroll
    for (int j = 0; j < 4; ++j) if (4 * c4 + j < sg.cols) out[j] = w[j];
}

template <class View>
int guides_draw(const Layout& L, const rbnn_svi_multi& g, float* W, const int32_t* live, int K, int per, long long member_stride,
                uint64_t key_xor, uint32_t draw_id, hipStream_t st) {
    GuidesDrawArgs a = {};
    a.L = L; a.loc = g.loc; a.sigma = g.sigma; a.W = W; a.keys = (const unsigned long long*)g.keys; a.live = live;
    a.key_xor = key_xor; a.draw_id = draw_id; a.per = per; a.n_members = K; a.member_stride = member_stride;
    hipLaunchKernelGGL(svils_draw_kernel<View>, dim3(blocks_for(L.n_quads), K * per), dim3(ELT_THREADS), 0, st, a);
    return launch_status();
}

// ---------------------------------------------------------------------------------------------------
// One block of 256 threads, fixed-order sums in fp64: red[0] = sum kl_part + sum ce (the step's loss), cnt[0] = #(first argmax Psum == label)
// over the B points.  GATHER: point i's label is labels[rows[i]] (the index clamped into [0, idx_max]), else labels[i].
// ---------------------------------------------------------------------------------------------------
template <bool GATHER>
__device__ __forceinline__ void svi_step_sums(const float* kl_part, int n_part, const float* ce, int B, const float* Psum, int ldp, int C,
                                              const int32_t* labels, const int32_t* rows, int idx_max, double* red, double* cnt) {
    const int t = threadIdx.x;
    double s = 0.0, k = 0.0;
    for (int i = t; i < n_part; i += 256) s += (double)kl_part[i];
    for (int i = t; i < B; i += 256) {
        s += (double)ce[i];
        if (Psum) {
            const float* row = Psum + (long long)i * ldp;
            int best = 0;
            for (int c = 1; c < C; ++c) if (row[c] > row[best]) best = c;      // the first maximum, as torch.argmax
            const int y = GATHER ? labels[min(max(rows[i], 0), idx_max)] : labels[i];
            k += (best == y) ? 1.0 : 0.0;
        }
    }
    red[t] = s; cnt[t] = k;
    block_tree64(red, cnt);
}

// ---------------------------------------------------------------------------------------------------
// The guides' finalize, one block per guide: svi_step_sums over the guide's points, then the epoch's end: epoch_slot[k] in [0, log_rows) ->
// epoch_log[k, slot] = (sum of the step losses, correct predictions) of the epoch that ends with this step, and both accumulators are zeroed.
// GATHER: the guide has live[k] points of the B, their labels read through rows [K, B]; else all B points, labels [K, B] staged.
// ---------------------------------------------------------------------------------------------------
struct GuidesFinalArgs {
    const float *kl_part, *ce, *Psum;
    const int32_t *labels, *rows, *live, *epoch_slot;
    double *stats, *epoch_log;
    long long part_stride;
    int n_part, B, C, idx_max, log_rows;
};

template <bool GATHER> __global__ void __launch_bounds__(256) svils_finalize_kernel(const GuidesFinalArgs a) {
    __shared__ double red[256];
    __shared__ double cnt[256];
    const int k = blockIdx.x, n = a.live[k];
    if (n == 0) return;
    const long long pt = (long long)k * a.B;
    svi_step_sums<GATHER>(a.kl_part + k * a.part_stride, a.n_part, a.ce + pt, GATHER ? n : a.B, a.Psum ? a.Psum + pt * RBNN_CPAD : nullptr, RBNN_CPAD,
                          a.C, GATHER ? a.labels : a.labels + pt, GATHER ? a.rows + pt : nullptr, a.idx_max, red, cnt);
    if (threadIdx.x == 0) {
        double* const st = a.stats + 3LL * k;
        st[0] = red[0];
        const double loss = st[1] + red[0], correct = st[2] + cnt[0];
        const int slot = a.epoch_slot ? a.epoch_slot[k] : -1;
        if (slot >= 0 && slot < a.log_rows) {
            double* const row = a.epoch_log + ((long long)k * a.log_rows + slot) * 2;
            row[0] = loss; row[1] = correct;
            st[1] = 0.0; st[2] = 0.0;
        } else {
            st[1] = loss; st[2] = correct;
        }
    }
}

}  // namespace
