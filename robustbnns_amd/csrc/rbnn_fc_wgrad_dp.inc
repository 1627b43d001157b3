// rbnn_fc_wgrad_dp.inc — the double-precision checker of the fc / fc2 WEIGHT gradients (included by rbnn_kernels.hip behind rbnn_fp64.inc,
// whose forward, input gradient, workspaces and lane maps it shares).
//
// The loss is the trainers': cross-entropy on the logits.  After that file's forward with logits out, rbnn_conv_head_ce_dp (geometry-free)
// has turned the logits into per-point CE and dZ = scale (softmax - e_y), and rbnn_fc_input_grad_f64 has turned the act' stashes into
// dL/d(pre-activation) of every hidden layer: dact1 (and, fc2, dact2).  What is left:
//   fwg_hidden_dp_kernel        hidL[s][n][h] = act(A[s][n][:] . W[s][h][:] + b[s][h]): the activations of the LAST hidden layer, which the
//                               forward keeps in LDS only.  fc: A = X (fp32), W = W1; fc2: A = hid1 (fp64), W = Wm      -> hidL [S][N][H]
//   fwg_contract_dp_kernel      out[s][m][j] += sum_n A[s][n][m] * B[s or shared][n][j],  ob[s][m] += sum_n A[s][n][m]        K = points
//                               dW2 | db2 = dZ^T [hidL | 1];  fc2: dWm | dbm = dact2^T [hid1 | 1];  dW1 | db1 = dact1^T [X | 1]
//
// The contraction: one wave = one 16 x 16 output tile of one sample (a block is one wave), or the sample's bias tile of 16 rows (column 0 =
// the ones).  The wave LOADS its accumulator from the output buffer, walks the call's points in ascending order and stores the accumulator
// back; nothing is atomic.  Step r of a 16-point tile takes k = lg <-> point 16 g + 4 lg + r; points past the last one contribute zeros.
// The caller's point blocks are multiples of 16 points, so a tile of a block is a tile of the whole batch and an output element is the same
// chain of MFMAs wherever the borders of the blocks fall — bit-identical between runs and between point-block sizes once the caller has
// zeroed the outputs before the first block.  Nothing is tuned: the loads of a step are two scalars per lane.

namespace {

struct FwgHiddenArgs {
    const void* A;  long long a_sample_stride;  int lda;  int N;         // input rows: X (fp32, shared) or hid1 (fp64, per sample)
    const float* W; long long w_sample_stride;  int ldw;  int K;         // [S_total][H][ldw]; K = contraction length, a multiple of 4
    const float* b; int H;                                               // [S_total][H]
    const int* sidx;
    double* hid;                                                         // [S][N][H]
};

// ---------------------------------------------------------------------------------------------------
// The last hidden layer's activations: wave = (16-point tile, 4 tiles of 16 units, sample).  D[i = point][j = unit], the K loop of
// fc_forward_f64_kernel (rbnn_fp64.inc).
// ---------------------------------------------------------------------------------------------------
template <int ACT, typename TA>
__global__ void __launch_bounds__(64) fwg_hidden_dp_kernel(const FwgHiddenArgs a) {
    constexpr int HT = 4;
    const int lane = threadIdx.x, li = lane & 15, lg = lane >> 4;
    const int n0 = blockIdx.x * 16, h0 = blockIdx.y * HT * 16, s = blockIdx.z;
    const int sw = a.sidx ? a.sidx[s] : s;
    const float* const Ws = a.W + (long long)sw * a.w_sample_stride;
    const int na = min(n0 + li, a.N - 1);                      // rows past N repeat the last point; never stored
    const TA* const arow = (const TA*)a.A + (long long)s * a.a_sample_stride + (long long)na * a.lda;
    f64x4 acc[HT];
    const float* wrow[HT];
#pragma unroll
    for (int t = 0; t < HT; ++t) {
        acc[t] = (f64x4){0., 0., 0., 0.};
        wrow[t] = Ws + (long long)min(h0 + t * 16 + li, a.H - 1) * a.ldw;      // rows past H repeat the last unit; never stored
    }
    for (int k0 = 0; k0 < a.K; k0 += 16) {
        const int k = k0 + 4 * lg;
        const bool in = k < a.K;
        const int kc = in ? k : 0;
        f64x4 av = load4_f64(arow + kc);
        if (!in) av = (f64x4){0., 0., 0., 0.};
#pragma unroll
        for (int t = 0; t < HT; ++t) {
            if (h0 + t * 16 >= a.H) continue;                  // (wave-uniform) a tile wholly past H
            f64x4 bv = load4_f64(wrow[t] + kc);
            if (!in) bv = (f64x4){0., 0., 0., 0.};
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[t] = MFMA64(av[r], bv[r], acc[t]);
        }
    }
    mfma64_drain(acc);
    // ---- acc[t][r] = pre-activation of point n0 + lg + 4*r, unit h0 + t*16 + li, without its bias
#pragma unroll
    for (int t = 0; t < HT; ++t) {
        const int h = h0 + t * 16 + li;
        if (h >= a.H) continue;
        const double bias = (double)a.b[(long long)sw * a.H + h];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = n0 + lg + 4 * r;
            if (n < a.N) a.hid[((long long)s * a.N + n) * a.H + h] = act_fwd64<ACT>(acc[t][r] + bias);
        }
    }
}

struct FwgContractArgs {
    const double* A;  int lda;  int M;                                   // [S][N][lda]; columns m < M are the output's rows
    const void* B;  long long b_sample_stride;  int ldb;  int J;         // [S or shared][N][ldb] (fp32 or fp64); columns j < J the output's columns
    int N;
    double* out;  double* ob;                                            // [S][M][J], [S][M]: added to
};

// ---------------------------------------------------------------------------------------------------
// out | ob += A^T [B | 1]: wave = (sample, 16 rows m, 16 columns j — or the bias tile, column 0 = the ones).  D[i = m][j].
// ---------------------------------------------------------------------------------------------------
template <typename TB>
__global__ void __launch_bounds__(64) fwg_contract_dp_kernel(const FwgContractArgs a) {
    const int lane = threadIdx.x, li = lane & 15, lg = lane >> 4;
    const int jt_n = (a.J + 15) / 16 + 1, per_s = ((a.M + 15) / 16) * jt_n;
    const int s = (int)(blockIdx.x / per_s), rem = (int)(blockIdx.x - (long long)s * per_s), mt = rem / jt_n, jt = rem - mt * jt_n;
    const bool bias = jt == jt_n - 1;                                       // (wave-uniform)
    const int j = bias ? 0 : jt * 16 + li;
    const bool j_ok = bias ? li == 0 : j < a.J;
    f64x4 acc[1];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long row = (long long)s * a.M + mt * 16 + lg + 4 * r;
        const bool ok = j_ok && mt * 16 + lg + 4 * r < a.M;
        acc[0][r] = !ok ? 0. : bias ? a.ob[row] : a.out[row * a.J + j];
    }
    // rows past M and columns past J repeat the last one; never stored
    const double* const ap = a.A + (long long)s * a.N * a.lda + min(mt * 16 + li, a.M - 1);
    const TB* const bp = (const TB*)a.B + (long long)s * a.b_sample_stride + min(j, a.J - 1);
    const double one = (li == 0) ? 1. : 0.;
    for (int n0 = 0; n0 < a.N; n0 += 16) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = n0 + 4 * lg + r;
            const bool in = n < a.N;
            const int nc = in ? n : 0;
            const double av = in ? ap[(long long)nc * a.lda] : 0.;
            const double bv = bias ? one : in ? (double)bp[(long long)nc * a.ldb] : 0.;
            acc[0] = MFMA64(av, bv, acc[0]);
        }
    }
    mfma64_drain(acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long row = (long long)s * a.M + mt * 16 + lg + 4 * r;
        if (!j_ok || mt * 16 + lg + 4 * r >= a.M) continue;
        if (bias) a.ob[row] = acc[0][r];
        else a.out[row * a.J + j] = acc[0][r];
    }
}

long long fwg_contract_waves(const FwgContractArgs& a, int S) { return (long long)S * ((a.M + 15) / 16) * ((a.J + 15) / 16 + 1); }

template <typename TB>
int launch_fwg_contract_dp(const FwgContractArgs& a, int S, hipStream_t st) {
    hipLaunchKernelGGL((fwg_contract_dp_kernel<TB>), dim3((unsigned)fwg_contract_waves(a, S)), dim3(64), 0, st, a);
    return launch_status();
}

// what the three entry points ask of the net and the counts
int validate_fwg_dp(const rbnn_posterior* net, int N, int S) {
    const int rc = validate_net_f64(net);
    if (rc) return rc;
    if (N < 1 || S < 1 || S > 65535 || (long long)N * S > 0x7fffffffLL) return RBNN_ERR_SHAPE;
    return RBNN_OK;
}

}  // namespace

// ===================================================================================================
// C-ABI of the fc / fc2 weight-gradient checker
// ===================================================================================================
extern "C" {

int rbnn_fc_wgrad_dp_workspace_query(const rbnn_posterior* net, int32_t N, int32_t S, size_t* bytes) {
    if (!net || !bytes) return RBNN_ERR_NULL;
    if (net->arch != RBNN_ARCH_FC && net->arch != RBNN_ARCH_FC2) return RBNN_ERR_UNSUPPORTED;
    if (net->hidden < 4 || (net->hidden & 3) || N < 1 || S < 1 || (long long)N * S > 0x7fffffffLL) return RBNN_ERR_SHAPE;
    const size_t SN = (size_t)S * N;
    bytes[0] = SN * sizeof(double);                                              // ce
    bytes[1] = SN * net->hidden * sizeof(double);                                // hidL
    return RBNN_OK;
}

int rbnn_fc_hidden_dp(const rbnn_posterior* net, const float* X, int32_t ldx, const int32_t* sidx, int32_t S, int32_t N, const double* hid1,
                      double* hidL, void* stream) {
    int rc = validate_fwg_dp(net, N, S);
    if (rc) return rc;
    const bool fc2 = net->arch == RBNN_ARCH_FC2;
    if (!X || !hidL || (fc2 && !hid1)) return RBNN_ERR_NULL;
    if (ldx < net->in_stride || (ldx & 3)) return RBNN_ERR_SHAPE;
    if (!aligned16(X) || !aligned16(hidL) || (fc2 && !aligned16(hid1))) return RBNN_ERR_ALIGN;
    const int H = net->hidden;
    FwgHiddenArgs a = {};
    a.N = N; a.H = H; a.sidx = sidx; a.hid = hidL;
    if (fc2) {
        a.A = hid1; a.a_sample_stride = (long long)N * H; a.lda = H;
        a.W = net->Wm; a.w_sample_stride = (long long)H * H; a.ldw = H; a.K = H; a.b = net->bm;
    } else {
        a.A = X; a.a_sample_stride = 0; a.lda = ldx;
        a.W = net->W1; a.w_sample_stride = (long long)H * net->in_stride; a.ldw = net->in_stride; a.K = net->in_stride; a.b = net->b1;
    }
    const dim3 grid((unsigned)((N + 15) / 16), (unsigned)((H + 63) / 64), (unsigned)S);
    hipStream_t st = (hipStream_t)stream;
    return for_activation(net->activation, [&](auto act) {
        if (fc2) hipLaunchKernelGGL((fwg_hidden_dp_kernel<decltype(act)::value, double>), grid, dim3(64), 0, st, a);
        else     hipLaunchKernelGGL((fwg_hidden_dp_kernel<decltype(act)::value, float>), grid, dim3(64), 0, st, a);
        return launch_status();
    });
}

int rbnn_fc_weight_grads_dp(const rbnn_posterior* net, const float* X, int32_t ldx, int32_t S, int32_t N, const double* dZ,
                            const double* dact1, const double* hid1, const double* dact2, const double* hidL, double* dW1, double* db1,
                            double* dWm, double* dbm, double* dW2, double* db2, void* stream) {
    int rc = validate_fwg_dp(net, N, S);
    if (rc) return rc;
    const bool fc2 = net->arch == RBNN_ARCH_FC2;
    if (!X || !dZ || !dact1 || !hidL || !dW1 || !db1 || !dW2 || !db2) return RBNN_ERR_NULL;
    if (fc2 && (!hid1 || !dact2 || !dWm || !dbm)) return RBNN_ERR_NULL;
    if (ldx < net->in_stride || (ldx & 3)) return RBNN_ERR_SHAPE;
    if (!aligned16(X) || !aligned16(dZ) || !aligned16(dact1) || !aligned16(hidL)) return RBNN_ERR_ALIGN;
    if (fc2 && (!aligned16(hid1) || !aligned16(dact2))) return RBNN_ERR_ALIGN;
    const int H = net->hidden, C = net->n_classes, D = net->in_features;
    hipStream_t st = (hipStream_t)stream;

    FwgContractArgs out = {}, mid = {}, in = {};
    out.A = dZ; out.lda = RBNN_CPAD; out.M = C;
    out.B = hidL; out.b_sample_stride = (long long)N * H; out.ldb = H; out.J = H; out.N = N; out.out = dW2; out.ob = db2;
    mid.A = dact2; mid.lda = H; mid.M = H;
    mid.B = hid1; mid.b_sample_stride = (long long)N * H; mid.ldb = H; mid.J = H; mid.N = N; mid.out = dWm; mid.ob = dbm;
    in.A = dact1; in.lda = H; in.M = H;
    in.B = X; in.b_sample_stride = 0; in.ldb = ldx; in.J = D; in.N = N; in.out = dW1; in.ob = db1;
    // one wave per output tile, the samples along the same grid axis
    if (fwg_contract_waves(out, S) > 0x7fffffffLL || fwg_contract_waves(mid, S) > 0x7fffffffLL || fwg_contract_waves(in, S) > 0x7fffffffLL)
        return RBNN_ERR_SHAPE;

    if ((rc = launch_fwg_contract_dp<double>(out, S, st))) return rc;
    if (fc2 && (rc = launch_fwg_contract_dp<double>(mid, S, st))) return rc;
    return launch_fwg_contract_dp<float>(in, S, st);
}

}  // extern "C"
