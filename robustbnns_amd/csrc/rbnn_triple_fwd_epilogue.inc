// rbnn_triple_fwd_epilogue.inc — the epilogue of one h chunk of fc_forward_x3_kernel (rbnn_triple.hip): scale, bias, activation, derivative
// stash, skinny output layer.  It is TEXT, included where `acc` names the chunk's accumulators f32x4 [HTW][NTW] (left zeroed) and `hc0` its first
// hidden unit: inline in the one-chunk pipeline, and as the body of the two-chunk pipeline's per-chunk lambda.  (A lambda shared by both forms
// moves the one-chunk kernels' instructions; as text they stay what they were — profiles/fwd_xonce/README.txt.)
        const int hw0 = hc0 + (wave_h * HTW) * 16;
        unsigned mine[NTW];
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) mine[nt] = 0u;
#pragma unroll
        for (int ht = 0; ht < HTW; ++ht) {
            const int hrow = hw0 + ht * 16 + 4 * lg;           // acc[ht][nt][r] is hidden unit hrow + r
            const f32x4 bias = *(const f32x4*)(a.b + (long long)sw * a.H + hrow);
            f32x4 w2f = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (LAYER2 && li < a.C) w2f = *(const f32x4*)(a.W2 + ((long long)sw * a.C + li) * a.H + hrow);
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) {
                const int n = n0 + (wave_n * NTW + nt) * 16 + li;
                f32x4 v = acc[ht][nt] * out_scale + bias, hv;
                acc[ht][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
                unsigned bits = 0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    bits |= (v[r] > 0.f ? 1u : 0u) << r;
                    hv[r] = act_fwd<ACT>(v[r]);
                }
                if (BITMASK) {
                    unsigned part = bits << (16 * (ht & 1) + 4 * lg);
                    part |= __shfl_xor(part, 16);
                    part |= __shfl_xor(part, 32);
                    if (lg == (ht >> 1)) mine[nt] |= part;
                }
                if (!BITMASK && a.dact && n < a.N) {
                    f32x4 dv;
#pragma unroll
                    for (int r = 0; r < 4; ++r) dv[r] = act_grad_from_value<ACT>(hv[r]);
                    *(f32x4*)(a.dact + ((long long)s * a.N + n) * a.H + hrow) = dv;
                }
                if (LAYER2) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) zacc[nt] = MFMA16(w2f[r], hv[r], zacc[nt]);
                } else {
                    // stage-major fp32 image [S][H/32 stages][N/16 groups][16 points][32 units]: this lane's four units of tile ht are 16 bytes at
                    // byte ((hrow >> 4) & 1) * 64 + lg * 16 of its point's 128-byte row; a tile's 16 points are one 2-KiB block, and the two h tiles of a
                    // stage fill its lines between them — no LDS staging, no split here (layer 2 splits at its operand read)
#ifdef RBNN_X3_L1_ABL_NOSTORE
                    if (n < a.N && hv[0] == 1.2345e-30f) {                 // ablation (timing only): never stored
#else
                    if (n < a.N) {
#endif
                        const long long blk = ((long long)s * HW + (hrow >> 5)) * ((a.N + 15) >> 4) + (n >> 4);
#ifdef RBNN_X3_L1_ABL_SMALL
                        char* const row = a.hid + ((blk * 2048) & 0xFFC00) + (n & 15) * 128 + ((hrow >> 4) & 1) * 64 + lg * 16;   // ablation: all stores into 1 MB
#else
                        char* const row = a.hid + blk * 2048 + (n & 15) * 128 + ((hrow >> 4) & 1) * 64 + lg * 16;
#endif
                        *(f32x4*)row = hv * hid_scale;
                    }
                }
            }
        }
        if (BITMASK && a.mask) {
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) {
                const int n = n0 + (wave_n * NTW + nt) * 16 + li;
                if (lg < HTW / 2 && n < a.N) a.mask[((long long)s * HW + (hw0 >> 5) + lg) * mask_ld(a.N) + n] = mine[nt];
            }
        }
