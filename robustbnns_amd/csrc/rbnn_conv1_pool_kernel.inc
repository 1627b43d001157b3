// rbnn_conv1_pool_kernel.inc — the text of conv1_pool_kernel (described in rbnn_conv.hip, which includes it once per form).  RBNN_CONV1_KERNEL
// names the kernel; RBNN_CONV1_PACKED: X is [S * N, ldx] and the block reads its own row s * N + n (every sample has its own batch: the lockstep
// conv trainer), not row n; RBNN_CONV1_PACKED == 2: X is [S / RBNN_SVI_MULTI_ACC_SAMPLES * N, ldx] and the block reads row (s / RBNN_SVI_MULTI_ACC_SAMPLES) * N + n
// (the samples come in groups of that many, every group has its own batch: the accuracy forward of the conv SVI guides in lockstep).  Three
// kernels from one text, as rbnn_train_kernels.inc: the kernel of the attack path keeps its name and its code.

template <int ACT, class G>
__global__ void __launch_bounds__(conv1_threads<G>(), 1) RBNN_CONV1_KERNEL(const ConvArgs a) {
    constexpr int NPP = G::P1W * G::P1W, IW = G::IW, NTH = conv1_threads<G>();
    // Weights in LDS as CHANNEL PAIRS: [c / 2][ci][tap][2] (52 floats per (pair, ci): thirteen aligned float4).  The FMA loop then runs on
    // v_pk_fma_f32 — one instruction = the same tap of two output channels against one broadcast patch value — i.e. at the packed fp32 rate
    // (round 4; the un-packed loop ran at 0.73 of the plain FMA rate: 2.09 ms per C5 pass).  Every output is still one fp32 FMA chain in
    // the same (input channel, ky, kx) order: results are bit-identical.
    constexpr int WROW = 52;
    __shared__ __attribute__((aligned(16))) float wsh[(C1 / 2) * G::CIN * WROW];
    __shared__ __attribute__((aligned(8))) float xsh[G::DIN];
    static_assert(IW % 2 == 0, "patch pairs are 8-byte aligned");
    const long long sn = blockIdx.x;
    const int n = (int)(sn % a.N), s = (int)(sn / a.N), tid = threadIdx.x;
    const int sw = a.sidx ? a.sidx[s] : s;
    for (int e = tid; e < C1 * G::K1; e += NTH) {                        // e = (c, ci, tap) as nn.Conv2d stores it
        const int c = e / G::K1, k = e - c * G::K1;
        wsh[((c >> 1) * G::CIN + k / 25) * WROW + 2 * (k % 25) + (c & 1)] = a.K1w[(long long)sw * C1 * G::K1 + e];
    }
#if RBNN_CONV1_PACKED == 2
    for (int e = tid; e < G::DIN; e += NTH) xsh[e] = a.X[((long long)(s / RBNN_SVI_MULTI_ACC_SAMPLES) * a.N + n) * a.ldx + e];
#elif RBNN_CONV1_PACKED
    for (int e = tid; e < G::DIN; e += NTH) xsh[e] = a.X[sn * a.ldx + e];
#else
    for (int e = tid; e < G::DIN; e += NTH) xsh[e] = a.X[(long long)n * a.ldx + e];
#endif
    __syncthreads();
    constexpr int NH = conv1_halves<G>(), CPT = C1 / NH;                  // channels per thread
    if (tid >= NH * NPP) return;
    const int pos = tid % NPP, c0 = (tid / NPP) * CPT;
    const int py = pos / G::P1W, px = pos % G::P1W;
    // the 6 x 6 patch as 18 aligned PAIRS per input channel: v_pk_fma_f32 broadcasts either half of a pair to both lanes (op_sel), so a patch
    // value costs half a register pair — spelled as a scalar broadcast the compiler kept every value twice (216 registers, two waves per SIMD)
    f32x2 patch[G::CIN][6][3];
#pragma unroll
    for (int ci = 0; ci < G::CIN; ++ci)
#pragma unroll
        for (int y = 0; y < 6; ++y)
#pragma unroll
            for (int j = 0; j < 3; ++j) patch[ci][y][j] = *(const f32x2*)(xsh + ci * (IW * IW) + (2 * py + y) * IW + 2 * px + 2 * j);
    float* const p1 = a.P1 + sn * G::P1SZ + pos;                         // dense [S][N][32][P1W][P1W]
    uint8_t* const st = a.st1 + sn * G::P1SZ + pos;
#pragma unroll 1
    for (int cp = c0 / 2; cp < (c0 + CPT) / 2; ++cp) {
        f32x2 v4[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v4[q] = (f32x2){0.f, 0.f};
#pragma unroll
        for (int ci = 0; ci < G::CIN; ++ci) {                             // channel-major accumulation, taps in (ky, kx) order
            asm volatile("" ::: "memory");                               // keep the three input channels' weight reads from being hoisted together (156 registers)
            const float* const wrow = wsh + (cp * G::CIN + ci) * WROW;
#pragma unroll
            for (int ky = 0; ky < 5; ++ky)
#pragma unroll
                for (int kx = 0; kx < 5; ++kx) {
                    const int tap = ky * 5 + kx;
                    // one 16-byte read per tap pair (it keeps 52 more registers live than 8-byte reads: 252 VGPRs, hence one wave per SIMD in the launch bounds)
                    const f32x4 w4 = *(const f32x4*)(wrow + 4 * (tap >> 1));
                    const f32x2 wv = (tap & 1) ? (f32x2){w4[2], w4[3]} : (f32x2){w4[0], w4[1]};
#pragma unroll
                    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                        for (int dx = 0; dx < 2; ++dx) {
                            // acc.{lo,hi} += w.{lo,hi} * pair.{half}: the broadcast is the instruction's op_sel (written as a vector splat,
                            // the compiler hoisted 108 materialised (p, p) pairs out of the channel loop: 252 registers)
                            const f32x2 pp = patch[ci][dy + ky][(dx + kx) >> 1];
                            // The BROADCAST operand (the patch pair, one half of it for both result lanes) is src0: op_sel / op_sel_hi bit 0.  Rounds 3-5 had it as
                            // src1 (op_sel:[0,1,0]) — a form hipcc itself never emits (it canonicalises a packed-fp32 broadcast onto src0) and that is NOT reliable
                            // on gfx950 when waves of another kernel share the SIMD: with two processes on one GPU the low result lane intermittently took the
                            // other half of the pair (46 of 320 forward calls differed from their own reference; 0 of 320 in this form; profiles/r05w).  The
                            // product is commutative: results are bit-identical to the old form's (one process).
                            if ((dx + kx) & 1) asm("v_pk_fma_f32 %0, %2, %1, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "+v"(v4[dy * 2 + dx]) : "v"(wv), "v"(pp));
                            else               asm("v_pk_fma_f32 %0, %2, %1, %0 op_sel:[0,0,0] op_sel_hi:[0,1,1]" : "+v"(v4[dy * 2 + dx]) : "v"(wv), "v"(pp));
                        }
                }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c = 2 * cp + h;
            const float b = a.K1b[(long long)sw * C1 + c];
            float best = 0.f, best_pre = 0.f;
            int arg = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float pre = v4[q][h] + b, v = smooth_act<ACT>() ? act_fwd<ACT>(pre) : pre;
                if (q == 0 || v > best) { best = v; best_pre = pre; arg = q; }   // first maximum wins (torch max_pool2d)
            }
            p1[c * NPP] = smooth_act<ACT>() ? best : act_fwd<ACT>(best);
            st[c * NPP] = (uint8_t)(arg | (best_pre > 0.f ? 4 : 0));
        }
    }
}
