// rbnn_conv_wgrad_kernels.inc — the text of the three per-point kernels of the conv weight gradients (described in rbnn_conv_train.hip, which
// includes this file once per form): RBNN_DO2_KERNEL, RBNN_WGEMM_KERNEL and RBNN_ROUTE1_KERNEL name them.  RBNN_CONV_WG_ENS: the lockstep form —
// the kernel first moves its argument record to the views of ITS member (blockIdx.y; the GEMM: blockIdx.z, y being the K slice) of arrays packed
// [M, B, .], then runs the same text.  Two kernels from one text, as rbnn_train_kernels.inc: the single net's kernels keep their names and their code.

#if RBNN_CONV_WG_ENS
template <int ACT> __global__ void __launch_bounds__(256) RBNN_DO2_KERNEL(ConvDo2Args a, const int B) {
    {                                                                      // member blockIdx.y of [M, B, .] and of Fw [M, C, 49 Hc]
        const long long mem = blockIdx.y, pt = mem * B, F = (long long)a.Hc * NP2;
        a.dZ += pt * RBNN_CPAD; a.Fw += mem * a.C * F; a.Q2 += pt * F; a.st2 += pt * F; a.dO2 += pt * a.Hc * NPOS;
    }
#else
template <int ACT> __global__ void __launch_bounds__(256) RBNN_DO2_KERNEL(const ConvDo2Args a) {
#endif
    __shared__ float gs[4][NP2];
    __shared__ int as[4][NP2];
    const int t = threadIdx.x, groups = a.Hc >> 2;
    const int b = blockIdx.x / groups, hc0 = 4 * (blockIdx.x % groups);
    const int F = a.Hc * NP2;
    if (t < 4 * NP2) {
        const int hl = t / NP2, p = t % NP2;
        const long long f = (long long)(hc0 + hl) * NP2 + p;
        float dq = 0.f;
        for (int c = 0; c < a.C; ++c) dq = fmaf(a.dZ[(long long)b * RBNN_CPAD + c], a.Fw[(long long)c * F + f], dq);
        const int st = a.st2[(long long)b * F + f];
        float d;
        if (smooth_act<ACT>()) d = act_grad_from_value<ACT>(a.Q2[(long long)b * F + f]);
        else d = (st & 4) ? 1.f : act_neg_slope<ACT>();
        gs[hl][p] = dq * d;
        as[hl][p] = st & 3;
    }
    __syncthreads();
    const int hl = t >> 6, pos = t & 63, y = pos >> 3, x = pos & 7;
    float s = 0.f;
#pragma unroll
    for (int dy = 1; dy >= 0; --dy)
#pragma unroll
        for (int dx = 1; dx >= 0; --dx) {
            const int wy = y - dy, wx = x - dx;                            // the window whose cell (dy, dx) this position is
            if (wy >= 0 && wy < P2W && wx >= 0 && wx < P2W) {
                const int p = wy * P2W + wx;
                if (as[hl][p] == dy * 2 + dx) s += gs[hl][p];
            }
        }
    a.dO2[((long long)b * a.Hc + hc0 + hl) * NPOS + pos] = s;
}

#if RBNN_CONV_WG_ENS
template <int MODE> __global__ void __launch_bounds__(256) RBNN_WGEMM_KERNEL(WgArgs g, const long long a_mem, const long long b_mem, const long long o_mem) {
    {                                                                      // member blockIdx.z: its operands and its slices [slices][M, N]
        const long long mem = blockIdx.z;
        g.A += mem * a_mem; g.Bsrc += mem * b_mem; g.out += mem * o_mem;
    }
#else
template <int MODE> __global__ void __launch_bounds__(256) RBNN_WGEMM_KERNEL(const WgArgs g) {
#endif
    constexpr int NTN = MODE == G_DP1 ? 2 : 4, TN = 16 * NTN;
    __shared__ float As[GK][GLD], Bs[GK][TN + 4];
    const int tiles_n = (g.N + TN - 1) / TN;
    const int m0 = GT * (blockIdx.x / tiles_n), n0 = TN * (blockIdx.x % tiles_n);
    const int k_begin = blockIdx.y * g.kc, k_end = min(k_begin + g.kc, g.K);
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, li = lane & 15, lg = lane >> 4;
    f32x4 acc[NTN], tot[NTN];
#pragma unroll
    for (int nt = 0; nt < NTN; ++nt) acc[nt] = tot[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int kk = t & 15, r0 = t >> 4;
    float ra[4], rb[NTN];
    auto fetch = [&](int k0) {
        const int k = k0 + kk;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = m0 + r0 + 16 * i;
            ra[i] = (m < g.M && k < k_end) ? wg_load_a<MODE>(g, m, k) : 0.f;
        }
#pragma unroll
        for (int i = 0; i < NTN; ++i) {
            const int n = n0 + r0 + 16 * i;
            rb[i] = (n < g.N && k < k_end) ? wg_load_b<MODE>(g, n, k) : 0.f;
        }
    };
    int stage = 0;
    fetch(k_begin);
    for (int k0 = k_begin; k0 < k_end; k0 += GK, ++stage) {
#pragma unroll
        for (int i = 0; i < 4; ++i) As[kk][r0 + 16 * i] = ra[i];
#pragma unroll
        for (int i = 0; i < NTN; ++i) Bs[kk][r0 + 16 * i] = rb[i];
        __syncthreads();
        if (k0 + GK < k_end) fetch(k0 + GK);
#pragma unroll
        for (int ks = 0; ks < GK / 4; ++ks) {
            const float a = As[4 * ks + lg][16 * wave + li];
#pragma unroll
            for (int nt = 0; nt < NTN; ++nt) acc[nt] = MFMA16(a, Bs[4 * ks + lg][16 * nt + li], acc[nt]);
        }
        __syncthreads();
        if ((stage & 31) == 31) {
#pragma unroll
            for (int nt = 0; nt < NTN; ++nt) { tot[nt] += acc[nt]; acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
        }
    }
    // lane holds C(m0 + 16 wave + 4 lg + r, n0 + 16 nt + li)
#pragma unroll
    for (int nt = 0; nt < NTN; ++nt) {
        tot[nt] += acc[nt];
        const int n = n0 + 16 * nt + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + 16 * wave + 4 * lg + r;
            if (m < g.M && n < g.N) g.out[((long long)blockIdx.y * g.M + m) * g.N + n] = tot[nt][r];
        }
    }
}

#if RBNN_CONV_WG_ENS
template <int ACT> __global__ void __launch_bounds__(ELT_THREADS) RBNN_ROUTE1_KERNEL(ConvRouteArgs a, const int B) {
    {                                                                      // member blockIdx.y of part [M][splits][n], P1 / st1 / dO1 [M, B, .]; a.n: ONE member's elements
        const long long mem = blockIdx.y, pt = mem * B;
        a.part += mem * a.splits * a.n; a.P1 += pt * P1SZ; a.st1 += pt * P1SZ; a.dO1 += pt * C1 * NO1;
    }
#else
template <int ACT> __global__ void __launch_bounds__(ELT_THREADS) RBNN_ROUTE1_KERNEL(const ConvRouteArgs a) {
#endif
    const long long e = (long long)blockIdx.x * ELT_THREADS + threadIdx.x;
    if (e >= a.n) return;
    double s = 0.0;
    for (int sp = 0; sp < a.splits; ++sp) s += (double)a.part[(long long)sp * a.n + e];
    const int ci = (int)(e & (C1 - 1));
    const long long m = e >> 5;
    const int b = (int)(m / PP1), pp = (int)(m - (long long)b * PP1);
    const long long at = (long long)b * P1SZ + ci * PP1 + pp;
    const int st = a.st1[at];
    float d;
    if (smooth_act<ACT>()) d = act_grad_from_value<ACT>(a.P1[at]);
    else d = (st & 4) ? 1.f : act_neg_slope<ACT>();
    const float v = (float)s * d;
    float* const o = a.dO1 + ((long long)b * C1 + ci) * NO1 + (2 * (pp / P1W)) * O1W + 2 * (pp % P1W);
#pragma unroll
    for (int q = 0; q < 4; ++q) o[(q >> 1) * O1W + (q & 1)] = (st & 3) == q ? v : 0.f;
}
