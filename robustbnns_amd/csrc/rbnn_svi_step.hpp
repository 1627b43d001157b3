// rbnn_svi_step.hpp — what the SVI step of the single trainer (rbnn_train.hip) and of the guides in lockstep (rbnn_svi_lockstep.hip) share,
// each defined once: the Adam + KL kernel (a template on LOCKSTEP, as the GEMM and head kernels of rbnn_train_gemm.hpp: a unit emits only the
// form it launches, and false compiles the member index, the key / learning-rate arrays and the skip out) and the fixed-order fp64 sums of a step.
#pragma once
#include "rbnn_train_core.hpp"

namespace {

// ---------------------------------------------------------------------------------------------------
// Adam (torch.optim.Adam, single-tensor, defaults but lr) on loc and raw scale, one thread per quad of a tensor:
//   g_loc = dCE/dw + loc,   g_raw = (dCE/dw eps + sigma - 1/sigma) sigmoid(raw)      (TraceMeanField's analytic KL against N(0, 1))
//   m = m + (1 - b1)(g - m),  v = b2 v + (1 - b2) g^2,  p += (-step_size m) / (sqrt(v) / bc2_sqrt + eps_adam),  sigma = softplus(raw)
// and the KL of the PRE-update parameters, -log sigma + (sigma^2 + loc^2) / 2 - 1/2, summed per block in a fixed tree order.
// LOCKSTEP: guide blockIdx.y of K in [K, member_stride] buffers, under its own key and learning rate; a guide with counts[k] == 0 has finished
// and is neither read nor written.  step_size = (float)(lr[k] / bc1) with bc1 = 1 - beta1^t formed by the host in double: the IEEE double
// division rounds as the host's does, so the value is adam_scalars()'s for that lr, bit for bit.
// ---------------------------------------------------------------------------------------------------
struct AdamArgs {
    Layout L;
    float *loc, *raw, *sigma, *m_loc, *v_loc, *m_raw, *v_raw;
    const float* grad;
    float* kl_part;
    unsigned long long key;
    uint32_t draw_id;
    AdamScalars s;
    // LOCKSTEP only
    const unsigned long long* keys;
    const int32_t* counts;
    const double* lr;
    double bc1;
    long long member_stride, part_stride;
};

template <bool LOCKSTEP> __global__ void __launch_bounds__(ELT_THREADS) adam_kernel(const AdamArgs a) {
    __shared__ float red[ELT_THREADS];
    const long long q = (long long)blockIdx.x * ELT_THREADS + threadIdx.x;
    float kl = 0.f;
    if constexpr (LOCKSTEP) { if (a.counts[blockIdx.y] == 0) return; }
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
        const long long base = (LOCKSTEP ? blockIdx.y * a.member_stride : 0) + sg.off + (long long)r * sg.cols + 4 * c4;
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

}  // namespace
