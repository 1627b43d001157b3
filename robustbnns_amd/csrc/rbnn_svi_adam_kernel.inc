// rbnn_svi_adam_kernel.inc — the text of the SVI step's Adam + KL kernel (described in rbnn_svi_step.hpp, which includes it once as the template
// adam_kernel<LOCKSTEP>; rbnn_svi.hip includes it once more).  RBNN_SVI_ADAM_KERNEL names the kernel.  RBNN_SVI_ADAM_TENSOR_MAJOR: the
// lockstep form on TENSOR-MAJOR buffers — six blocks [K, size of tensor], so guide blockIdx.y's segment lies at K * (the segment's offset) +
// k * (its size), not at k * member_stride + offset; K is the kernel's second argument and a.member_stride is not read.  Kernels from one
// text, as rbnn_train_kernels.inc: the instantiations of the template keep their names and their code.

#if RBNN_SVI_ADAM_TENSOR_MAJOR
__global__ void __launch_bounds__(ELT_THREADS) RBNN_SVI_ADAM_KERNEL(const AdamArgs a, const int n_guides) {
    constexpr bool LOCKSTEP = true;
#else
template <bool LOCKSTEP> __global__ void __launch_bounds__(ELT_THREADS) RBNN_SVI_ADAM_KERNEL(const AdamArgs a) {
#endif
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
#if RBNN_SVI_ADAM_TENSOR_MAJOR
        const long long base = n_guides * sg.off + blockIdx.y * ((long long)sg.rows * sg.cols) + (long long)r * sg.cols + 4 * c4;
#else
        const long long base = (LOCKSTEP ? blockIdx.y * a.member_stride : 0) + sg.off + (long long)r * sg.cols + 4 * c4;
#endif
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
