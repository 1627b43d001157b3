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

// The kernel's text is rbnn_svi_adam_kernel.inc (a unit whose buffers are tensor-major includes it once more under another name).
#define RBNN_SVI_ADAM_KERNEL adam_kernel
#define RBNN_SVI_ADAM_TENSOR_MAJOR 0
#include "rbnn_svi_adam_kernel.inc"
#undef RBNN_SVI_ADAM_KERNEL
#undef RBNN_SVI_ADAM_TENSOR_MAJOR

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
