// rbnn_nn_step.hpp — what the deterministic step of the fc / fc2 members in lockstep (rbnn_nn_train.hip) and of the one conv net
// (rbnn_conv_train.hip) share, each defined once: the Adam kernel on the flat buffers and the step-statistics kernel (templates on LOCKSTEP, as
// the kernels of rbnn_svi_step.hpp and rbnn_train_gemm.hpp: a unit emits only the form it launches, and false compiles the member index out).
#pragma once
#include "rbnn_train_core.hpp"

namespace {

// ---------------------------------------------------------------------------------------------------
// Adam (torch.optim.Adam, single-tensor, defaults but lr), one thread per parameter:
//   m = m + (1 - b1)(g - m),  v = b2 v + (1 - b2) g^2,  p += (-step_size m) / (sqrt(v) / bc2_sqrt + eps_adam)
// LOCKSTEP: member blockIdx.y of [M, member_stride] buffers.
// ---------------------------------------------------------------------------------------------------
struct AdamArgs {
    float *P, *m, *v;
    const float* grad;
    long long n_params, member_stride;                                  // member_stride: LOCKSTEP only
    AdamScalars s;
};

template <bool LOCKSTEP> __global__ void __launch_bounds__(ELT_THREADS) nn_adam_kernel(const AdamArgs a) {
    const long long i = (long long)blockIdx.x * ELT_THREADS + threadIdx.x;
    if (i >= a.n_params) return;
    const long long e = LOCKSTEP ? (long long)blockIdx.y * a.member_stride + i : i;
    float p = a.P[e], m = a.m[e], v = a.v[e];
    adam_one(p, m, v, a.grad[e], a.s);
    a.P[e] = p; a.m[e] = m; a.v[e] = v;
}

// ---------------------------------------------------------------------------------------------------
// One block of 256 threads (LOCKSTEP: per member, blockIdx.x of ce / correct [M, B] and stats [M, 3]):
// stats = [fp32-rounded mean CE of the step, += it, += correct predictions].  Fixed-order sums in fp64.
// ---------------------------------------------------------------------------------------------------
struct FinalArgs {
    const float* ce;
    const int32_t* correct;
    double* stats;
    int B;
};

template <bool LOCKSTEP> __global__ void __launch_bounds__(256) nn_finalize_kernel(const FinalArgs a) {
    __shared__ double red[256];
    __shared__ double cnt[256];
    const int t = threadIdx.x;
    const long long at = LOCKSTEP ? (long long)blockIdx.x * a.B : 0;
    double s = 0.0, k = 0.0;
    for (int i = t; i < a.B; i += 256) {
        s += (double)a.ce[at + i];
        k += (double)a.correct[at + i];
    }
    red[t] = s; cnt[t] = k;
    block_tree64(red, cnt);
    if (t == 0) {
        double* const st = a.stats + (LOCKSTEP ? 3 * (long long)blockIdx.x : 0);
        const double loss = (double)(float)(red[0] / (double)a.B);      // loss.item() of an fp32 mean
        st[0] = loss;
        st[1] += loss;
        st[2] += cnt[0];
    }
}

}  // namespace
