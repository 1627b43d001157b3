// rbnn_train_kernels.inc — the text of the strided GEMM kernel and of the output-layer + loss kernel, included by rbnn_train_gemm.hpp (which
// describes both) once per form: RBNN_GEMM_KERNEL / RBNN_HEAD_KERNEL name the two kernels, RBNN_KERNELS_SKIP says whether a finished member
// (counts == 0) is skipped.  Two kernels from one text, not one kernel with a second template parameter and not a shared __device__ body: the
// kernels without the skip keep their names and, instruction for instruction, the device code they had.

template <bool LOCKSTEP> __global__ void __launch_bounds__(256) RBNN_GEMM_KERNEL(const GemmArgs g) {
    constexpr bool SKIP = RBNN_KERNELS_SKIP;
    static_assert(LOCKSTEP || !SKIP, "only a lockstep launch has members to skip");
    __shared__ float As[GK][GLD], Bs[GK][GLD];
    long long idx_row = LOCKSTEP ? blockIdx.y : 0;
    if constexpr (SKIP) {
        idx_row = blockIdx.y / g.per;
        if (g.counts[idx_row] == 0) return;
    }
    int pi = 0;
#pragma unroll
    for (int j = 1; j < 3; ++j) if (j < g.n_prob && (int)blockIdx.x >= g.p[j].first_tile) pi = j;
    const GemmProb& p = g.p[pi];
    const long long mem = LOCKSTEP ? blockIdx.y : 0;
    const int tile = blockIdx.x - p.first_tile, m0 = GT * (tile / p.tiles_n), n0 = GT * (tile % p.tiles_n);
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, li = lane & 15, lg = lane >> 4;
    const int n_real = p.ones_n >= 0 ? p.ones_n : p.N;
    const float* const A = p.A + mem * p.a_mem;
    const float* const Bm = p.B + mem * p.b_mem;
    const long long idx_at = idx_row * p.idx_mem;
    f32x4 acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < p.K; k0 += GK) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = t + 256 * i;
            int mm, kk;
            if (p.a_k == 1) { mm = idx >> 4; kk = idx & 15; } else { mm = idx & 63; kk = idx >> 6; }     // coalesced along the unit stride
            const int m = m0 + mm, k = k0 + kk;
            float av = 0.f;
            if (m < p.M && k < p.K) av = A[(long long)gathered<LOCKSTEP>(p.a_idx, idx_at, m, p.idx_max) * p.a_m + k * p.a_k];
            As[kk][mm] = av;
            int nn, kb;
            if (p.b_k == 1) { nn = idx >> 4; kb = idx & 15; } else { nn = idx & 63; kb = idx >> 6; }
            const int n = n0 + nn, kq = k0 + kb;
            float bv = 0.f;
            if (kq < p.K) {
                if (n < n_real) bv = Bm[n * p.b_n + (long long)gathered<LOCKSTEP>(p.b_idx, idx_at, kq, p.idx_max) * p.b_k];
                else if (n == p.ones_n) bv = 1.f;
            }
            Bs[kb][nn] = bv;
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < GK / 4; ++ks) {
            const float a = As[4 * ks + lg][16 * wave + li];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[nt] = MFMA16(a, Bs[4 * ks + lg][16 * nt + li], acc[nt]);
        }
        __syncthreads();
    }
    // lane holds C(m0 + 16 wave + 4 lg + r, n0 + 16 nt + li)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int n = n0 + 16 * nt + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + 16 * wave + 4 * lg + r;
            if (m >= p.M || n >= p.N) continue;
            const float v = acc[nt][r];
            if (n == p.ones_n) { p.bias_out[mem * p.bias_mem + m] = v; continue; }
            const long long o = mem * p.c_mem + (long long)m * p.ldc + n;
            if (p.epi == EPI_FWD) {
                const float pre = v + p.bias[mem * p.bias_mem + n], h = act_value(p.act, pre);
                p.Cout[o] = h;
                p.Dout[o] = act_deriv(p.act, pre, h);
            } else if (p.epi == EPI_MUL) {
                p.Cout[o] = v * p.Dmul[o];
            } else {
                p.Cout[o] = v;
            }
        }
    }
}

template <bool LOCKSTEP> __global__ void __launch_bounds__(256) RBNN_HEAD_KERNEL(const HeadArgs a) {
    constexpr bool SKIP = RBNN_KERNELS_SKIP;
    static_assert(LOCKSTEP || !SKIP, "only a lockstep launch has members to skip");
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= a.B) return;
    const long long mem = LOCKSTEP ? blockIdx.y : 0, pt = mem * a.B + b;
    if constexpr (SKIP) {
        if (a.counts[mem] == 0) return;
    }
    if (LOCKSTEP && a.counts && b >= a.counts[mem]) {                  // not a point of this member: ce, dZ, dA and correct are zero
        if (lane == 0) {
            a.ce[pt] = 0.f;
            if (a.correct) a.correct[pt] = 0;
#pragma unroll
            for (int c = 0; c < RBNN_CPAD; ++c) a.dZ[pt * RBNN_CPAD + c] = 0.f;
        }
        for (int h = lane; h < a.H; h += 64) a.dA[pt * a.H + h] = 0.f;
        return;
    }
    const float* const W2 = a.W2 + mem * a.p_mem;
    float z[RBNN_CPAD];
#pragma unroll
    for (int c = 0; c < RBNN_CPAD; ++c) z[c] = 0.f;
    const float* hrow = a.Hl + pt * a.H;
    for (int h = lane; h < a.H; h += 64) {
        const float hv = hrow[h];
#pragma unroll
        for (int c = 0; c < RBNN_CPAD; ++c) if (c < a.C) z[c] = fmaf(hv, W2[(long long)c * a.H + h], z[c]);
    }
    const float* const b2 = a.b2 + mem * a.p_mem;
#pragma unroll
    for (int c = 0; c < RBNN_CPAD; ++c) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) z[c] += __shfl_xor(z[c], off, 64);
        if (c < a.C) z[c] += b2[c];
    }
    const int y = a.labels[gathered<LOCKSTEP>(a.rows, mem * a.B, b, a.idx_max)];
    float g[RBNN_CPAD];
    ce_softmax_grad<RBNN_CPAD>(z, a.C, y, a.inv_S, g);
    if (lane == 0) {
        float m = -INFINITY, zy = 0.f;
        int best = 0;
        for (int c = 0; c < a.C; ++c) {
            if (z[c] > m) { m = z[c]; best = c; }                     // strictly greater: the first maximum, as torch.argmax
            if (c == y) zy = z[c];
        }
        float den = 0.f, rest = 0.f;
        for (int c = 0; c < a.C; ++c) { const float e = expf(z[c] - m); den += e; if (c != y) rest += e; }
        // label = argmax: CE = log(1 + sum_{c != y} e^(z_c - z_y)) without the cancellation of log(den) - 0
        a.ce[pt] = (zy == m) ? log1pf(rest) : logf(den) - (zy - m);
        if (a.correct) a.correct[pt] = best == y ? 1 : 0;
#pragma unroll
        for (int c = 0; c < RBNN_CPAD; ++c) a.dZ[pt * RBNN_CPAD + c] = g[c];
    }
    const float* drow = a.Dl + pt * a.H;
    float* arow = a.dA + pt * a.H;
    for (int h = lane; h < a.H; h += 64) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < RBNN_CPAD; ++c) if (c < a.C) s = fmaf(g[c], W2[(long long)c * a.H + h], s);
        arow[h] = s * drow[h];
    }
}
