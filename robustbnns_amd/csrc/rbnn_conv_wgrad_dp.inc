// rbnn_conv_wgrad_dp.inc — the double-precision checker of the conv WEIGHT gradients (included by rbnn_conv.hip behind rbnn_conv_fp64.inc,
// whose forward, workspaces, pooling rule and lane maps it shares).
//
// The loss is the trainers': cross-entropy on the logits.  After that file's forward with logits out:
//   cwg_head_dp_kernel          per (s, n): ce = logsumexp(z) - z_y and dZ = scale (softmax - e_y), the maximum subtracted, the label class
//                               formed as -(sum of the others) / den                                             -> ce [S][N], dZ [S][N][16]
//   cwg_backward_dp_kernel      that file's conv_backward_fp64_body with WGRAD = true: the input gradient's stages up to dP1 * act'(P1), and it
//                               WRITES the routed images instead of running conv1^T                         -> dO2 [S][N][Hc][NPOS], dO1 [S][N][32][O1^2]
//   cwg_dfw_dp_kernel           dFw | dFb = dZ^T [Q2 | 1]                 M = C,  N = Hc NP2 | 1,  K = points
//   cwg_dk2_dp_kernel           dK2 | dK2b = sum dO2 x [P1 patch | 1]     M = Hc, N = 800 | 1,     K = (point, conv2 position), gathered from P1 as
//                               conv2_pool_fp64_kernel gathers
//   cwg_dk1_dp_kernel           dK1 | dK1b = sum dO1 x [x patch | 1]      M = 32, N = Cin 25 | 1,  K = (point, conv1 position)
//
// The three contractions: one wave = one 16 x 16 output tile (a block is one wave).  The wave LOADS its accumulator from the output buffer,
// walks the call's points in ascending order and stores the accumulator back; nothing is atomic.  An MFMA of dK2 / dK1 takes 4 positions of
// ONE point (NPOS and O1^2 are multiples of 4), an MFMA of dFw takes ONE point (k = 0; k = 1 .. 3 are zeros, which add nothing): no MFMA
// straddles a point, so an output element is the same chain of MFMAs wherever the borders of the caller's point blocks fall — bit-identical
// between runs and between point-block sizes once the caller has zeroed the outputs before the first block.  Nothing is tuned: the dK1 grid
// is a handful of waves with a long chain.

namespace {

struct CwgDpArgs {
    const float* X; int ldx; int N;
    const float* K2w; const float* Fw;
    int Hc; int C; const int* sidx; int S;
    const double* P1; const uint8_t* arg1;          // [S][N][32*P1W*P1W]
    const double* Q2; const uint8_t* arg2;          // [S][N][Hc*NP2]
    const double* dZ;                               // [S][N][16]
    double* dO2; double* dO1;                       // [S][N][Hc][NPOS], [S][N][32][O1*O1]
    double* dK1w; double* dK1b; double* dK2w; double* dK2b; double* dFw; double* dFb;
};

// ---------------------------------------------------------------------------------------------------
// The head: one thread per (s, n).
// ---------------------------------------------------------------------------------------------------
__global__ void cwg_head_dp_kernel(const double* __restrict__ Z, const int* __restrict__ labels, int S, int N, int C, double scale,
                                   double* __restrict__ dZ, double* __restrict__ ce) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)S * N) return;
    const int y = labels[(int)(i % N)];
    double z[16], e[16];
    double m = -INFINITY, zy = 0., den = 0., rest = 0.;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        z[c] = (c < C) ? Z[i * RBNN_CPAD + c] : 0.;
        if (c < C) m = fmax(m, z[c]);
        if (c == y) zy = z[c];
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        e[c] = (c < C) ? exp(z[c] - m) : 0.;
        den += e[c];
        if (c != y) rest += e[c];
    }
    // the label at the maximum: den = 1 + rest exactly as torch's log_softmax sees it, and log1p keeps a tiny CE
    ce[i] = (zy == m) ? log1p(rest) : (m - zy) + log(den);
#pragma unroll
    for (int c = 0; c < 16; ++c) dZ[i * RBNN_CPAD + c] = (c < C) ? ((c == y ? -rest : e[c]) / den) * scale : 0.;
}

// Backward to dO2 and dO1: the backward body of rbnn_conv_fp64.inc with its WGRAD switch on (see there).
template <int ACT, class G>
__global__ void __launch_bounds__(256) cwg_backward_dp_kernel(const CwgDpArgs a) { conv_backward_fp64_body<ACT, G, true>(a); }

// ---------------------------------------------------------------------------------------------------
// dFw | dFb: wave = (sample, 16 head features f0 .. f0 + 15), or the sample's bias tile (column 0 = the ones).  D[i = class][j = feature].
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) cwg_dfw_dp_kernel(const CwgDpArgs a, int NP2) {
    const int lane = threadIdx.x, li = lane & 15, lg = lane >> 4;
    const long long F = (long long)a.Hc * NP2;
    const int tiles = (int)(F >> 4) + 1;
    const int s = (int)(blockIdx.x / tiles), tile = (int)(blockIdx.x - (long long)s * tiles);
    const bool bias = tile == tiles - 1;                                    // (wave-uniform)
    const long long f = bias ? 0 : (long long)tile * 16 + li;
    f64x4 acc[1];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int c = lg + 4 * r;
        acc[0][r] = (c >= a.C) ? 0. : bias ? (li == 0 ? a.dFb[(long long)s * a.C + c] : 0.) : a.dFw[((long long)s * a.C + c) * F + f];
    }
    const double* const dz = a.dZ + (long long)s * a.N * RBNN_CPAD + li;
    const double* const q = a.Q2 + (long long)s * a.N * F + f;
    const bool feeds = lg == 0;                                             // one point per MFMA: k = 0
    const double one = (li == 0) ? 1. : 0.;
    for (int n = 0; n < a.N; ++n) {
        double av = 0., bv = 0.;
        if (feeds) {
            av = (li < a.C) ? dz[(long long)n * RBNN_CPAD] : 0.;
            bv = bias ? one : q[(long long)n * F];
        }
        acc[0] = MFMA64(av, bv, acc[0]);
    }
    mfma64_drain(acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int c = lg + 4 * r;
        if (c >= a.C) continue;
        if (!bias) a.dFw[((long long)s * a.C + c) * F + f] = acc[0][r];
        else if (li == 0) a.dFb[(long long)s * a.C + c] = acc[0][r];
    }
}

// ---------------------------------------------------------------------------------------------------
// dK2 | dK2b: wave = (sample, 16 conv2 channels, 16 of the 800 columns k = ci*25 + ky*5 + kx — or the bias tile, column 0 = the ones).
// D[i = channel][j = column].  A 16-position group is 4 MFMAs: step r takes k = lg <-> position 16 g + 4 lg + r, so a lane reads 4
// consecutive dO2 values at once; positions past the last whole group (NPOS = 100) go 4 to an MFMA, k = lg <-> position.
// ---------------------------------------------------------------------------------------------------
template <class G>
__global__ void __launch_bounds__(64) cwg_dk2_dp_kernel(const CwgDpArgs a) {
    constexpr int PP = G::P1W * G::P1W, NG = G::NPOS / 16, NTAIL = (G::NPOS - NG * 16) / 4, CT = 800 / 16 + 1;
    static_assert(G::NPOS % 4 == 0, "an MFMA takes 4 positions of one point");
    const int lane = threadIdx.x, li = lane & 15, lg = lane >> 4;
    const int per_s = (a.Hc >> 4) * CT;
    const int s = (int)(blockIdx.x / per_s), rem = (int)(blockIdx.x - (long long)s * per_s), ht = rem / CT, ct = rem - ht * CT;
    const bool bias = ct == CT - 1;                                         // (wave-uniform)
    const int col = bias ? 0 : ct * 16 + li;
    const int ci = col / 25, tap = col - ci * 25, ky = tap / 5, kx = tap - ky * 5;
    const int koff = ci * PP + ky * G::P1W + kx;
    const double one = (li == 0) ? 1. : 0.;
    int poff[NG][4], toff[NTAIL > 0 ? NTAIL : 1];
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int pos = g * 16 + 4 * lg + r, y = pos / G::O2W, x = pos - y * G::O2W;
            poff[g][r] = y * G::P1W + x;
        }
#pragma unroll
    for (int t = 0; t < NTAIL; ++t) {
        const int pos = NG * 16 + t * 4 + lg, y = pos / G::O2W, x = pos - y * G::O2W;
        toff[t] = y * G::P1W + x;
    }
    f64x4 acc[1];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long row = (long long)s * a.Hc + ht * 16 + lg + 4 * r;
        acc[0][r] = bias ? (li == 0 ? a.dK2b[row] : 0.) : a.dK2w[row * 800 + col];
    }
    const double* arow = a.dO2 + ((long long)s * a.N * a.Hc + ht * 16 + li) * G::NPOS;
    const double* img = a.P1 + (long long)s * a.N * G::P1SZ + koff;
    for (int n = 0; n < a.N; ++n, arow += (long long)a.Hc * G::NPOS, img += G::P1SZ) {
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const f64x4 av = load4_f64(arow + g * 16 + 4 * lg);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double p = img[poff[g][r]];
                acc[0] = MFMA64(av[r], bias ? one : p, acc[0]);
            }
        }
#pragma unroll
        for (int t = 0; t < NTAIL; ++t) {
            const double p = img[toff[t]];
            acc[0] = MFMA64(arow[NG * 16 + t * 4 + lg], bias ? one : p, acc[0]);
        }
    }
    mfma64_drain(acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long row = (long long)s * a.Hc + ht * 16 + lg + 4 * r;
        if (!bias) a.dK2w[row * 800 + col] = acc[0][r];
        else if (li == 0) a.dK2b[row] = acc[0][r];
    }
}

// ---------------------------------------------------------------------------------------------------
// dK1 | dK1b: wave = (sample, 16 of the 32 conv1 channels, 16 of the columns [the Cin*25 taps k = cin*25 + ky*5 + kx | the ones | zeros]).
// D[i = channel][j = column].  O1^2 is a multiple of 16 and O1 of 4: step r of a 16-position group takes k = lg <-> position 16 g + 4 lg + r,
// four neighbours in one image row.
// ---------------------------------------------------------------------------------------------------
template <class G> constexpr int cwg_dk1_col_tiles() { return (G::K1 + 1 + 15) / 16; }

template <class G>
__global__ void __launch_bounds__(64) cwg_dk1_dp_kernel(const CwgDpArgs a) {
    constexpr int OO = G::O1 * G::O1, II = G::IW * G::IW, NG = OO / 16, CT = cwg_dk1_col_tiles<G>();
    static_assert(OO % 16 == 0 && G::O1 % 4 == 0, "whole 16-position groups; 4 neighbours share a row");
    const int lane = threadIdx.x, li = lane & 15, lg = lane >> 4;
    const int s = (int)(blockIdx.x / (2 * CT)), rem = (int)(blockIdx.x - s * (2 * CT)), rt = rem / CT, ct = rem - rt * CT;
    const int col = ct * 16 + li;
    const bool is_tap = col < G::K1, is_one = col == G::K1;
    const int kc = is_tap ? col : 0, cin = kc / 25, tap = kc - cin * 25, ky = tap / 5, kx = tap - ky * 5;
    const int xoff = cin * II + ky * G::IW + kx;
    f64x4 acc[1];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long row = (long long)s * C1 + rt * 16 + lg + 4 * r;
        acc[0][r] = is_tap ? a.dK1w[row * G::K1 + col] : is_one ? a.dK1b[row] : 0.;
    }
    const double* arow = a.dO1 + ((long long)s * a.N * C1 + rt * 16 + li) * OO;
    for (int n = 0; n < a.N; ++n, arow += (long long)C1 * OO) {
        const float* const xp = a.X + (long long)n * a.ldx + xoff;
#pragma unroll 4
        for (int g = 0; g < NG; ++g) {
            const int p0 = g * 16 + 4 * lg, oy = p0 / G::O1, ox = p0 - oy * G::O1;
            const f64x4 av = load4_f64(arow + p0);
            const float* const xr = xp + oy * G::IW + ox;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double v = (double)xr[r];
                acc[0] = MFMA64(av[r], is_tap ? v : is_one ? 1. : 0., acc[0]);
            }
        }
    }
    mfma64_drain(acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long row = (long long)s * C1 + rt * 16 + lg + 4 * r;
        if (is_tap) a.dK1w[row * G::K1 + col] = acc[0][r];
        else if (is_one) a.dK1b[row] = acc[0][r];
    }
}

template <int ACT, class G>
int launch_cwg_backward_dp(const CwgDpArgs& a, hipStream_t st) {
    constexpr int LDSB = BwdFp64Lds<G, true>::BYTES;
    static unsigned long long attr = 0;                                   // per instantiation, one bit per device
    if (!ensure_dynamic_lds((const void*)cwg_backward_dp_kernel<ACT, G>, LDSB, attr)) return RBNN_ERR_LAUNCH;
    hipLaunchKernelGGL((cwg_backward_dp_kernel<ACT, G>), dim3((unsigned)((long long)a.S * a.N)), dim3(256), LDSB, st, a);
    return launch_status();
}

template <class G>
int launch_cwg_contractions_dp(const CwgDpArgs& a, hipStream_t st) {
    const long long fw_tiles = ((long long)a.Hc * G::NP2 >> 4) + 1, k2_tiles = (long long)(a.Hc >> 4) * (800 / 16 + 1);
    hipLaunchKernelGGL(cwg_dfw_dp_kernel, dim3((unsigned)(a.S * fw_tiles)), dim3(64), 0, st, a, (int)G::NP2);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL((cwg_dk2_dp_kernel<G>), dim3((unsigned)(a.S * k2_tiles)), dim3(64), 0, st, a);
    if ((rc = launch_status())) return rc;
    hipLaunchKernelGGL((cwg_dk1_dp_kernel<G>), dim3((unsigned)(a.S * 2 * cwg_dk1_col_tiles<G>())), dim3(64), 0, st, a);
    return launch_status();
}

}  // namespace

// ===================================================================================================
// C-ABI of the weight-gradient checker
// ===================================================================================================
extern "C" {

int rbnn_conv_wgrad_dp_workspace_query(const rbnn_conv_posterior* net, int32_t N, int32_t S, size_t* bytes) {
    if (!net || !bytes) return RBNN_ERR_NULL;
    if (net->hidden < 16 || (net->hidden & 15) || N < 1 || S < 1) return RBNN_ERR_SHAPE;
    return for_geometry(net, [&](auto g) {
        using G = decltype(g);
        const size_t SN = (size_t)S * N;
        bytes[0] = SN * sizeof(double);                                   // ce
        bytes[1] = SN * net->hidden * G::NPOS * sizeof(double);           // dO2
        bytes[2] = SN * C1 * G::O1 * G::O1 * sizeof(double);              // dO1
        return (int)RBNN_OK;
    });
}

int rbnn_conv_head_ce_dp(const double* Z, const int32_t* labels, int32_t S, int32_t N, int32_t C, double scale, double* dZ, double* ce,
                         void* stream) {
    if (!Z || !labels || !dZ || !ce) return RBNN_ERR_NULL;
    if (N < 1 || S < 1 || (long long)N * S > 0x7fffffffLL || C < 1 || C > RBNN_CPAD) return RBNN_ERR_SHAPE;
    if (!aligned16(Z) || !aligned16(dZ)) return RBNN_ERR_ALIGN;
    if (Z == dZ) return RBNN_ERR_UNSUPPORTED;
    const long long total = (long long)S * N;
    hipLaunchKernelGGL(cwg_head_dp_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, Z, labels, S, N, C, scale,
                       dZ, ce);
    return launch_status();
}

int rbnn_conv_weight_grads_dp(const rbnn_conv_posterior* net, const float* X, int32_t ldx, const int32_t* sidx, int32_t S, int32_t N,
                              const double* dZ, const double* P1, const uint8_t* arg1, const double* Q2, const uint8_t* arg2, double* dO2,
                              double* dO1, double* dK1w, double* dK1b, double* dK2w, double* dK2b, double* dFw, double* dFb, void* stream) {
    int rc = validate_conv_fp64(net, N, S);
    if (rc) return rc;
    if (!X || !dZ || !P1 || !arg1 || !Q2 || !arg2 || !dO2 || !dO1 || !dK1w || !dK1b || !dK2w || !dK2b || !dFw || !dFb) return RBNN_ERR_NULL;
    if (ldx < net->in_channels * net->in_width * net->in_width || (ldx & 3)) return RBNN_ERR_SHAPE;
    // one wave per output tile, the samples along the same grid axis: the largest grid is dFw's
    if ((long long)S * (((long long)net->hidden * 81 >> 4) + 1) > 0x7fffffffLL) return RBNN_ERR_SHAPE;
    if (!aligned16(X) || !aligned16(dZ) || !aligned16(P1) || !aligned16(Q2) || !aligned16(dO2) || !aligned16(dO1)) return RBNN_ERR_ALIGN;
    CwgDpArgs a = {};
    a.X = X; a.ldx = ldx; a.N = N; a.K2w = net->K2w; a.Fw = net->Fw;
    a.Hc = net->hidden; a.C = net->n_classes; a.sidx = sidx; a.S = S;
    a.P1 = P1; a.arg1 = arg1; a.Q2 = Q2; a.arg2 = arg2; a.dZ = dZ; a.dO2 = dO2; a.dO1 = dO1;
    a.dK1w = dK1w; a.dK1b = dK1b; a.dK2w = dK2w; a.dK2b = dK2b; a.dFw = dFw; a.dFb = dFb;
    hipStream_t st = (hipStream_t)stream;
    return for_geometry(net, [&](auto g) {
        using G = decltype(g);
        const int rb = for_activation(net->activation, [&](auto act) { return launch_cwg_backward_dp<decltype(act)::value, G>(a, st); });
        return rb ? rb : launch_cwg_contractions_dp<G>(a, st);
    });
}

}  // extern "C"
