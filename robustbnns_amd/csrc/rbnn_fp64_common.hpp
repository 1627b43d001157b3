// rbnn_fp64_common.hpp — what the fp64 checkers share (rbnn_fp64.inc: fc / fc2, in rbnn_kernels.hip; rbnn_conv_fp64.inc: conv, in rbnn_conv.hip):
// the f64 MFMA and its lane maps, the widening loads, the activations in fp64 and the wait states behind a finished K loop.
//
// Lane maps of the 16x16x4 f64 MFMA (wave64, li = lane & 15, lg = lane >> 4):
//   A operand  a = A[i = li][k = lg]      B operand  b = B[k = lg][j = li]        (as the f32 16x16x4 form, one f64 per lane)
//   C/D        acc[r] = D[i = lg + 4*r][j = li]                                    (NOT the f32 map, which is i = 4*lg + r)
// The k <-> memory-index map of a K step is free as long as A and B agree: step r of a 16-wide K block takes k = lg <-> index 4*lg + r,
// so one 16-byte load of four consecutive fp32 values feeds four K steps.  K is a multiple of 4 (hidden % 4 == 0, D_pad % 16 == 0):
// a lane's four values are inside K together or not at all, and a ragged last block contributes zeros.
#pragma once
#include "rbnn_common.hpp"

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
#define MFMA64(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)
#define LEAKY_SLOPE64 0.01                      // the fp64 oracle's constant: 0.01 as a double, not (double)0.01f (2e-10 apart)

namespace {

template <int ACT> __device__ __forceinline__ double act_fwd64(double a) {
    if (ACT == RBNN_ACT_RELU)  return a > 0. ? a : 0.;
    if (ACT == RBNN_ACT_LEAKY) return a > 0. ? a : a * LEAKY_SLOPE64;
    if (ACT == RBNN_ACT_SIGM)  return 1. / (1. + exp(-a));
    return tanh(a);
}
// torch's backward of each activation from the pre-activation a and the value hv (act_deriv of rbnn_common.hpp, in fp64)
template <int ACT> __device__ __forceinline__ double act_deriv64(double a, double hv) {
    if (ACT == RBNN_ACT_RELU)  return a > 0. ? 1. : 0.;
    if (ACT == RBNN_ACT_LEAKY) return a > 0. ? 1. : LEAKY_SLOPE64;
    if (ACT == RBNN_ACT_SIGM)  return hv * (1. - hv);
    return 1. - hv * hv;
}

// four consecutive K elements widened to fp64 (exact); 16-byte aligned sources
__device__ __forceinline__ f64x4 load4_f64(const float* p) {
    const f32x4 v = *(const f32x4*)p;
    return (f64x4){(double)v[0], (double)v[1], (double)v[2], (double)v[3]};
}
__device__ __forceinline__ f64x4 load4_f64(const double* p) {
    const f64x2 lo = *(const f64x2*)p, hi = *(const f64x2*)(p + 2);
    return (f64x4){lo[0], lo[1], hi[0], hi[1]};
}

// The accumulators of a finished K loop are read by vector instructions: the f64 MFMA's result needs its passes first.  hipcc pads that
// itself; these wait states make the distance independent of what it schedules behind the loop (tools/kernel_resources.py counts it).
// (the empty statements tie the wait to the accumulators: every MFMA has issued before it, every reader comes behind it)
template <int T> __device__ __forceinline__ void mfma64_drain(f64x4 (&acc)[T]) {
#pragma unroll
    for (int t = 0; t < T; ++t) asm volatile("" : "+v"(acc[t]));
    asm volatile("s_nop 15\n\ts_nop 15");
#pragma unroll
    for (int t = 0; t < T; ++t) asm volatile("" : "+v"(acc[t]));
}

// per-point norms of a finished gradient G [N][ldg], the body of norms_f64_kernel and conv_norms_fp64_kernel: one wave per row (blocks of
// whole waves), a fixed butterfly; linf / l2 may each be null
__device__ __forceinline__ void row_norms64(const double* __restrict__ G, int ldg, int N, int D, double* __restrict__ linf,
                                            double* __restrict__ l2) {
    const int n = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (n >= N) return;
    double m = 0., ss = 0.;
    for (int d = lane; d < D; d += 64) {
        const double g = G[(long long)n * ldg + d];
        m = fmax(m, fabs(g));
        ss = fma(g, g, ss);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { m = fmax(m, __shfl_xor(m, o)); ss += __shfl_xor(ss, o); }
    if (lane == 0) {
        if (linf) linf[n] = m;
        if (l2) l2[n] = sqrt(ss);
    }
}

}  // namespace
