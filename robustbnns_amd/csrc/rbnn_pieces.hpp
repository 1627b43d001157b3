// rbnn_pieces.hpp — the host side the two fp16-piece modes share: "split" carries an operand as two fp16 pieces (rbnn_split.hip), "triple" as
// three (rbnn_triple.hip).  One design at two widths: rbnn_split_images / rbnn_triple_images hold the same fields in the same order, the entry
// points take the same arguments and make the same checks in the same order.  This header states that common part once — the gradient kernels'
// argument record, the body of rbnn_fc_input_grad_*, the checked launches of the image builders, the validation and argument filling of the two
// forwards.  What stays in each file is what the modes really differ in: the kernels, their tile plans, and the geometry of the images.
// Host code only (plus the plain argument record the gradient kernels take by value).
#pragma once
#include "rbnn_common.hpp"

#define GEN_Q (-17)                                            // |generator| <= 16 * 2^14 * 2^14 = 2^32  ->  |dA| <= 2^15 < fp16 max

namespace {

// Arguments of fc_grad_split_kernel / fc_grad_x3_kernel
struct GradPieceArgs {
    const char* dzg;  long long n_pad;  const float* gscale;  const uint32_t* mask;
    const char* W1c;  int ldc;                                  // split- / triple-cols image, ldc columns
    const char* W2g;                                            // generator image [S_total][H/16][1 KiB (split) / 2 KiB (triple)]
    int H;  int HW;  const int* sidx;  int S;  int chunk;  int nchunks;
    int N;  int NT;  int ND;  int Dt;
    float* out;  int ldo;  float out_scale;                     // slabs [nchunks][N][ldo]; out_scale = 2^-(e_w2 + GEN_Q + e_w1)
    // fc2.  GRAD_FC2_STEP1 (one sample per block): out = dhid1 [S][N][H] = act'(A1) * (dA2 . Wm), KEPT SCALED (x out_scale, no per-point
    // un-scaling): it is the fp32 source of step 2's A operand.  GRAD_FC2_STEP2: A operand read from `amem` and split in registers.
    const uint32_t* omask;  int OHW;                            // step 1: stash of the layer below [S][H/32][N_pad]
    const float* amem;                                          // step 2: [S][N][H]
    const float* dact;  const float* odact;                     // sigmoid / tanh: act' as fp32 [S][N][H] (this layer / the layer below)
};
enum { GRAD_FC = 0, GRAD_FC2_STEP1 = 1, GRAD_FC2_STEP2 = 2 };

// ---------------------------------------------------------------------------------------------------
// Image builders: rbnn_split_rows / rbnn_triple_rows(_grouped), rbnn_*_cols, rbnn_*_w2gen.  `extra`: the triple rows kernel's `grouped`.
// ---------------------------------------------------------------------------------------------------
inline bool exp_in_range(int e) { return e >= -100 && e <= 100; }

template <class Kernel, class... Extra>
int launch_rows_image(Kernel kernel, const float* src, int64_t rows, int32_t cols, int32_t ld_src, int32_t scale_exp, const rbnn_dev_scale* dev_scale,
                      void* dst, int32_t ld_dst, void* stream, Extra... extra) {
    if (!src || !dst) return RBNN_ERR_NULL;
    if (rows < 1 || cols < 1 || ld_src < cols || ld_dst < cols || (ld_dst & 31)) return RBNN_ERR_SHAPE;
    if (!exp_in_range(scale_exp)) return RBNN_ERR_SHAPE;
    if (!aligned16(dst)) return RBNN_ERR_ALIGN;
    const int groups = ld_dst / 8;
    const long long total = (long long)rows * groups;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       src, (long long)rows, cols, ld_src, ldexpf(1.f, scale_exp), dev_scale, (uint4*)dst, groups, extra...);
    return launch_status();
}

template <class Kernel>
int launch_cols_image(Kernel kernel, const float* W, int64_t n_mats, int32_t rows, int32_t cols, int32_t ld_src, int32_t scale_exp, void* dst,
                      int32_t ld_dst, void* stream) {
    if (!W || !dst) return RBNN_ERR_NULL;
    if (n_mats < 1 || rows < 32 || (rows & 31) || cols < 1 || ld_src < cols || ld_dst < cols || (ld_dst & 15)) return RBNN_ERR_SHAPE;
    if (!exp_in_range(scale_exp)) return RBNN_ERR_SHAPE;
    if (!aligned16(dst)) return RBNN_ERR_ALIGN;
    const long long total = (long long)n_mats * (rows / 32) * 4 * ld_dst;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       W, (long long)n_mats, rows, cols, ld_src, ldexpf(1.f, scale_exp), (uint4*)dst, ld_dst);
    return launch_status();
}

// units: 16-byte units of the image per 16 hidden rows (split 64, triple 128)
template <class Kernel>
int launch_w2gen_image(Kernel kernel, int units, const float* W2, int32_t n_mats, int32_t C, int32_t H, int32_t scale_exp, void* dst, void* stream) {
    if (!W2 || !dst) return RBNN_ERR_NULL;
    if (n_mats < 1 || C < 1 || C > 10 || H < 16 || (H & 15)) return RBNN_ERR_SHAPE;
    if (!exp_in_range(scale_exp)) return RBNN_ERR_SHAPE;
    if (!aligned16(dst)) return RBNN_ERR_ALIGN;
    const long long total = (long long)n_mats * (H / 16) * units;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       W2, n_mats, C, H, ldexpf(1.f, scale_exp), (uint4*)dst);
    return launch_status();
}

// ---------------------------------------------------------------------------------------------------
// rbnn_fc_forward_split / rbnn_fc_forward_triple: the checks of both, in their order, and the fields FwdSplitArgs and FwdX3Args share — `l1` for
// layer 1 and, fc2, `l2` for layer 2 (a copy of l1 with the operands of the middle layer).  The caller names what its mode differs in:
//   X, ldx       the input image and its row length (the triple call has no ldx argument: its image is built with the weight image's)
//   hid          fc2's hidden image (split: ws->hid1; triple: tws->hid_triple)
//   elem_bytes   bytes per image element (4 / 6);  n_round: the image holds N + n_round rows at most (triple: whole 16-row groups)
// and afterwards fills the geometry fields of its own record (x_sample_bytes of layer 2; triple: x_group_bytes / x_stage_bytes).
// ---------------------------------------------------------------------------------------------------
template <class Args, class Images>
int fc_forward_pieces_args(const rbnn_posterior* net, const Images* im, const void* X, int32_t ldx, void* hid, int elem_bytes, int n_round,
                           int32_t x_exp, const rbnn_dev_scale* dev_scales, int32_t N, const int32_t* sidx, int32_t S, int32_t out_kind,
                           const rbnn_workspace* ws, Args& l1, Args& l2) {
    if (!net || !im || !X || !ws || !ws->P || !im->W1_rows) return RBNN_ERR_NULL;
    if (!net->b1 || !net->W2 || !net->b2) return RBNN_ERR_NULL;
    if (net->arch != RBNN_ARCH_FC && net->arch != RBNN_ARCH_FC2) return RBNN_ERR_UNSUPPORTED;
    if (net->activation < RBNN_ACT_RELU || net->activation > RBNN_ACT_TANH) return RBNN_ERR_UNSUPPORTED;
    const bool fc2 = net->arch == RBNN_ARCH_FC2, bm = net->activation == RBNN_ACT_RELU || net->activation == RBNN_ACT_LEAKY;
    const int H = net->hidden, ld = im->ld_rows;
    if (H < 128 || (H % 128) || ld < net->in_features || (ld & 31) || ldx != ld) return RBNN_ERR_SHAPE;
    if (net->n_classes < 1 || net->n_classes > RBNN_CPAD || N < 1 || S < 1) return RBNN_ERR_SHAPE;
    // the kernels address a sample's weight image and the input image with 32-bit byte offsets from a 64-bit base
    const long long B = elem_bytes, lim = 1LL << 32, NR = (long long)N + n_round;
    if (H * B * ld >= lim || NR * ld * B >= lim || NR * H * B >= lim) return RBNN_ERR_SHAPE;
    if (out_kind != RBNN_OUT_PROBS && out_kind != RBNN_OUT_LOGITS) return RBNN_ERR_UNSUPPORTED;
    if (!aligned16(X) || !aligned16(im->W1_rows) || !aligned16(ws->P) || !aligned16(net->b1) || !aligned16(net->W2)) return RBNN_ERR_ALIGN;
    if (fc2 && (!im->Wm_rows || !net->bm || !hid || (bm ? !ws->mask2 : !ws->dact2))) return RBNN_ERR_NULL;
    if (fc2 && (!aligned16(im->Wm_rows) || !aligned16(hid) || !aligned16(net->bm))) return RBNN_ERR_ALIGN;
    Args& a = l1;
    a.X = (const char*)X; a.ldx = ld; a.N = N; a.x_sample_bytes = 0;
    a.W = (const char*)im->W1_rows; a.w_sample_bytes = H * B * ld; a.ldw = ld; a.KT = ld / 32;
    a.b = net->b1; a.W2 = net->W2; a.b2 = net->b2; a.C = net->n_classes; a.H = H;
    a.sidx = sidx; a.S = S; a.out_scale = ldexpf(1.f, -((dev_scales ? 0 : x_exp) + im->w1_exp)); a.x_ds = dev_scales;
    a.P = ws->P; a.mask = ws->mask1; a.dact = ws->dact1; a.out_kind = out_kind;
    if (!fc2) return RBNN_OK;
    // fc2: layer 1 -> hidden activations as an image in `hid`, scaled by 2^h1_exp (the caller bounds |h|: max_h sum_d |W1[h,d]| * max|x| +
    // max|b1|; record [1] of rbnn_input_scales on the device); layer 2 reads it per sample
    a.hid = (char*)hid; a.hid_scale = ldexpf(1.f, im->h1_exp); a.hid_ds = dev_scales ? dev_scales + 1 : nullptr;
    Args& b = l2;
    b = a;
    b.X = (const char*)hid; b.ldx = H;
    b.W = (const char*)im->Wm_rows; b.w_sample_bytes = H * B * H; b.ldw = H; b.KT = H / 32;
    b.b = net->bm; b.out_scale = ldexpf(1.f, -((dev_scales ? 0 : im->h1_exp) + im->wm_exp));
    b.x_ds = dev_scales ? dev_scales + 1 : nullptr; b.hid_ds = nullptr;
    b.mask = ws->mask2; b.dact = ws->dact2; b.hid = nullptr;
    return RBNN_OK;
}

// ---------------------------------------------------------------------------------------------------
// rbnn_fc_input_grad_split / rbnn_fc_input_grad_triple.  The mode names
//   dz_kernel     builder of the dZ generator image from ws->dZ
//   dz_optional   ws->dZ == NULL is allowed: pws->dZ_gen / g_scale are already built (rbnn_step_tail_triple)
//   launch        launch(integral_constant<int, GRAD_*>, activation, args, stream): its tile-plan chooser
// ---------------------------------------------------------------------------------------------------
template <class Images, class PieceWs, class DzKernel, class Launch>
int fc_input_grad_pieces(const rbnn_posterior* net, const Images* im, const int32_t* sidx, int32_t S, int32_t N, int32_t chunk,
                         const rbnn_workspace* ws, const PieceWs* pws, int32_t* n_slabs_out, void* stream, DzKernel dz_kernel, bool dz_optional,
                         Launch launch) {
    if (!net || !im || !ws || !pws || (!dz_optional && !ws->dZ) || !ws->slabs) return RBNN_ERR_NULL;
    if (!im->W1_cols || !im->W2_gen || !pws->dZ_gen || !pws->g_scale) return RBNN_ERR_NULL;
    if (net->arch != RBNN_ARCH_FC && net->arch != RBNN_ARCH_FC2) return RBNN_ERR_UNSUPPORTED;
    if (net->activation < RBNN_ACT_RELU || net->activation > RBNN_ACT_TANH) return RBNN_ERR_UNSUPPORTED;
    const bool fc2 = net->arch == RBNN_ARCH_FC2, bm = net->activation == RBNN_ACT_RELU || net->activation == RBNN_ACT_LEAKY;
    if (bm ? !ws->mask1 : !ws->dact1) return RBNN_ERR_NULL;
    if (fc2 && (bm ? !ws->mask2 : !ws->dact2)) return RBNN_ERR_NULL;
    const int H = net->hidden, Dp = net->in_stride, C = net->n_classes;
    if (H < 128 || (H % 128) || C < 1 || C > 10 || N < 1 || S < 1) return RBNN_ERR_SHAPE;
    if (im->ld_cols != Dp || (Dp & 15)) return RBNN_ERR_SHAPE;
    if (!aligned16(im->W1_cols) || !aligned16(im->W2_gen) || !aligned16(pws->dZ_gen) || !aligned16(ws->dZ)) return RBNN_ERR_ALIGN;
    if (fc2 && (!im->Wm_cols || !ws->dhid1)) return RBNN_ERR_NULL;
    if (fc2 && (!aligned16(im->Wm_cols) || !aligned16(ws->dhid1))) return RBNN_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    if (chunk <= 0) {                                           // the exact mode's slab plan (same workspace)
        rbnn_workspace_sizes q;
        const int rc = rbnn_workspace_query(net, N, S, 0, &q);
        if (rc) return rc;
        chunk = q.chunk;
    }
    if (chunk > S) chunk = S;
    const int nchunks = (S + chunk - 1) / chunk;
    if (n_slabs_out) *n_slabs_out = nchunks;
    const long long n_pad = mask_ld(N);
    if (ws->dZ) {
        hipLaunchKernelGGL(dz_kernel, dim3((unsigned)(n_pad / 16)), dim3(256), 0, st, ws->dZ, S, N, n_pad, C, (uint4*)pws->dZ_gen, pws->g_scale);
        if (hipGetLastError() != hipSuccess) return RBNN_ERR_LAUNCH;
    }
    GradPieceArgs g = {};
    g.dzg = (const char*)pws->dZ_gen; g.n_pad = n_pad; g.gscale = pws->g_scale;
    g.W2g = (const char*)im->W2_gen;
    g.H = H; g.HW = H / 32; g.sidx = sidx; g.S = S; g.N = N;
    if (!fc2) {
        g.mask = ws->mask1; g.dact = ws->dact1; g.W1c = (const char*)im->W1_cols; g.ldc = im->ld_cols; g.Dt = Dp / 16;
        g.chunk = chunk; g.nchunks = nchunks; g.out = ws->slabs; g.ldo = Dp;
        g.out_scale = ldexpf(1.f, -(im->w2_exp + GEN_Q + im->w1_exp));
        return launch(std::integral_constant<int, GRAD_FC>{}, net->activation, g, st);
    }
    // fc2 step 1, one sample per block: dhid1[s] = act'(A1_s) * ((act'(A2_s) * (dZ_s . W3_s)) . Wm_s), kept scaled:
    //   stored = dhid1 * 2^(e(n) + e_w3 + GEN_Q + e_wm - Q2),  Q2 = 14 + ceil(log2 H): |dA2 scaled| <= 2^15, |Wm scaled| <= 2^14, K = H
    //   => |stored| <= 2^15: in fp16 range, ready to be split as step 2's A operand
    int q2 = 14;
    while ((1 << (q2 - 14)) < H) ++q2;
    g.mask = ws->mask2; g.dact = ws->dact2; g.odact = ws->dact1; g.W1c = (const char*)im->Wm_cols; g.ldc = H; g.Dt = H / 16;
    g.chunk = 1; g.nchunks = S; g.out = ws->dhid1; g.ldo = H; g.out_scale = ldexpf(1.f, -q2);
    g.omask = ws->mask1; g.OHW = H / 32;
    const int rc = launch(std::integral_constant<int, GRAD_FC2_STEP1>{}, net->activation, g, st);
    if (rc) return rc;
    // fc2 step 2: slabs[k] = sum_{s in chunk k} dhid1[s] . W1_s; acc = g * 2^(e(n) + e_w3 + GEN_Q + e_wm - Q2 + e_w1)
    GradPieceArgs h = g;
    h.amem = ws->dhid1; h.W1c = (const char*)im->W1_cols; h.ldc = im->ld_cols; h.Dt = Dp / 16;
    h.chunk = chunk; h.nchunks = nchunks; h.out = ws->slabs; h.ldo = Dp;
    h.out_scale = ldexpf(1.f, -(im->w2_exp + GEN_Q + im->wm_exp - q2 + im->w1_exp));
    return launch(std::integral_constant<int, GRAD_FC2_STEP2>{}, net->activation, h, st);
}

}  // namespace
