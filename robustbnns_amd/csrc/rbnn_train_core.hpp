// rbnn_train_core.hpp — what every unit that trains or samples a net shares (rbnn_train.hip, rbnn_svi_lockstep.hip, rbnn_nn_train.hip,
// rbnn_hmc.hip, rbnn_conv_train.hip), each defined once: the parameter layout of the flat fc / fc2 buffers and its checks, the activations,
// torch's Adam formula with its host-side scalars, and the fixed-order block reductions.  No kernels (a __global__ function is emitted into
// every unit that includes its definition): the GEMM and head kernels are rbnn_train_gemm.hpp, the SVI step's rbnn_svi_step.hpp, the
// deterministic step's (Adam, step statistics) rbnn_nn_step.hpp.
#pragma once
#include "rbnn_common.hpp"

namespace {

// ---------------------------------------------------------------------------------------------------
// Parameter layout of the flat buffers: the state_dict tensors in order, unpadded, row-major (a bias: one row).
// ---------------------------------------------------------------------------------------------------
struct Seg { long long off, first_quad; int rows, cols, tensor_id; };
struct Layout { Seg s[6]; int n; long long n_params, n_quads; };

inline Layout layout_of(int arch, int D, int H, int C) {
    Layout L = {};
    const bool fc2 = arch == RBNN_ARCH_FC2;
    const int rows[6] = {H, 1, fc2 ? H : C, 1, C, 1}, cols[6] = {D, H, H, fc2 ? H : C, H, C};
    const int ids[6] = {T_W1, T_B1, fc2 ? T_WM : T_W2, fc2 ? T_BM : T_B2, T_W2, T_B2};
    L.n = fc2 ? 6 : 4;
    long long off = 0, q = 0;
    for (int i = 0; i < L.n; ++i) {
        L.s[i] = {off, q, rows[i], cols[i], ids[i]};
        off += (long long)rows[i] * cols[i];
        q += (long long)rows[i] * ((cols[i] + 3) / 4);
    }
    L.n_params = off; L.n_quads = q;
    return L;
}

inline int check_dims(int arch, int activation, int D, int H, int C) {
    if (arch != RBNN_ARCH_FC && arch != RBNN_ARCH_FC2) return RBNN_ERR_UNSUPPORTED;
    if (activation < RBNN_ACT_RELU || activation > RBNN_ACT_TANH) return RBNN_ERR_UNSUPPORTED;
    if (D < 1 || H < 1 || C < 1 || C > RBNN_CPAD) return RBNN_ERR_SHAPE;
    if ((long long)H * D > (1LL << 30) || (long long)H * H > (1LL << 30)) return RBNN_ERR_SHAPE;
    return RBNN_OK;
}

// of an rbnn_svi_train_net or an rbnn_nn_train_net
template <class Net> Layout layout_of(const Net& n) { return layout_of(n.arch, n.in_features, n.hidden, n.n_classes); }
template <class Net> int check_net(const Net* n) {
    return n ? check_dims(n->arch, n->activation, n->in_features, n->hidden, n->n_classes) : RBNN_ERR_NULL;
}

constexpr int ELT_THREADS = 256;
inline unsigned blocks_for(long long n) { return (unsigned)((n + ELT_THREADS - 1) / ELT_THREADS); }

__device__ __forceinline__ int seg_of(const Layout& L, long long q) {
    int i = 0;
#pragma unroll
    for (int j = 1; j < 6; ++j) if (j < L.n && q >= L.s[j].first_quad) i = j;
    return i;
}

// ---------------------------------------------------------------------------------------------------
// Element-wise helpers
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ float softplus_f(float r) { return r > 20.f ? r : log1pf(expf(r)); }     // torch.nn.functional.softplus (threshold 20)

// the activation and its derivative (rbnn_common.hpp's act_fwd / act_deriv) for an activation known only at run time
__device__ __forceinline__ float act_value(int act, float a) {
    if (act == RBNN_ACT_RELU) return act_fwd<RBNN_ACT_RELU>(a);
    if (act == RBNN_ACT_LEAKY) return act_fwd<RBNN_ACT_LEAKY>(a);
    if (act == RBNN_ACT_SIGM) return act_fwd<RBNN_ACT_SIGM>(a);
    return act_fwd<RBNN_ACT_TANH>(a);
}
__device__ __forceinline__ float act_deriv(int act, float a, float h) {
    if (act == RBNN_ACT_RELU) return act_deriv<RBNN_ACT_RELU>(a, h);
    if (act == RBNN_ACT_LEAKY) return act_deriv<RBNN_ACT_LEAKY>(a, h);
    if (act == RBNN_ACT_SIGM) return act_deriv<RBNN_ACT_SIGM>(a, h);
    return act_deriv<RBNN_ACT_TANH>(a, h);
}

// torch.optim.Adam, single-tensor, no weight decay:
//   m = m + (1 - b1)(g - m),  v = b2 v + (1 - b2) g^2,  p += (-step_size m) / (sqrt(v) / bc2_sqrt + eps_adam)
struct AdamScalars { float w1, beta2, w2, adam_eps, step_size, bc2_sqrt; };      // w1 = 1 - beta1, w2 = 1 - beta2

// torch's single-tensor Adam takes its scalars (the bias corrections, 1 - beta1, 1 - beta2) in Python floats (double) and hands them to
// fp32 tensor ops: each is rounded to fp32 once.  (1.f - 0.999f is 1.3e-5 off 0.001: with v << (1 - beta2) g^2 that is 6e-6 of the update.)
inline AdamScalars adam_scalars(long long step, double lr, double beta1, double beta2, double adam_eps) {
    return {(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)adam_eps, (float)(lr / (1.0 - pow(beta1, (double)step))),
            (float)sqrt(1.0 - pow(beta2, (double)step))};
}

__device__ __forceinline__ void adam_one(float& p, float& m, float& v, float g, const AdamScalars& a) {
    m = fmaf(a.w1, g - m, m);                                // exp_avg.lerp_(grad, 1 - beta1)
    v = fmaf(a.w2, g * g, v * a.beta2);                      // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(v) / a.bc2_sqrt + a.adam_eps;
    p = p + (-a.step_size * m) / denom;                      // param.addcdiv_(exp_avg, denom, value=-step_size)
}

// ---------------------------------------------------------------------------------------------------
// Block reductions in one fixed tree order (no atomics: two runs are bit-identical)
// ---------------------------------------------------------------------------------------------------
// the sum of v over the ELT_THREADS threads of the block -> out[blockIdx.x]; red may be reused at once
__device__ __forceinline__ void block_sum_to(float v, float* red, float* out) {
    red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int s = ELT_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = red[0];
    __syncthreads();
}

// 256 threads, fp64: red[0] = the sum of red[0..256) for each array given (reduced alongside each other), every thread having written its entries
template <class... T> __device__ __forceinline__ void block_tree64(T*... red) {
    const int t = threadIdx.x;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) ((red[t] += red[t + w]), ...);
        __syncthreads();
    }
}

}  // namespace
