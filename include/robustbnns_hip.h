/*
 * robustbnns_hip.h — C-ABI of the MI355X (gfx950) Bayesian attack / expected-loss-gradient
 * hot path.  Plain pointers and sizes only: no torch types, no C++ in the signatures.
 *
 * The reference (ginevracoal/robustBNNs) has NO native boundary for this path: it is a
 * Python loop nest that dispatches stock torch ops with batch 1.  Each entry point below
 * therefore cites the Python statements it replaces (file:line in the reference); the
 * reference-side binding a maintainer would add is the ctypes stub in INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc / torch.empty(device="cuda")) unless
 *     marked [host]; all floating-point data is IEEE fp32, row-major, 16-byte aligned;
 *   - `stream` is a hipStream_t passed as void*; every call is asynchronous on it,
 *     re-entrant, keeps no global state and allocates nothing: the caller owns every buffer;
 *   - return value: RBNN_OK (0) or a negative rbnn_status; nothing throws;
 *   - a *posterior* is S_total stacked weight samples (HMC chain / SVI draws / ensemble
 *     members); `sample_idx` (int32[S], may be NULL = 0..S-1) selects which stored samples
 *     a call uses, in order — model_bnn.py:246-252 (`seeds` index the stored samples).
 *
 * Padding contract (lets every kernel run whole 16-wide MFMA tiles, no tail code in the
 * K loops): D_pad = round_up(D,16) is the row stride of X, W1 and of gradient buffers;
 * columns [D, D_pad) are ZERO.  hidden is 32, 64 or a multiple of 128 for the fc / fc2
 * kernels (the reference only allows powers of two >= 16, model_nn.py:39-40; 16 is
 * zero-padded to 32 by the host, which is exact: a padded unit has zero outgoing weights;
 * the fp32 kernels take every hidden size the triple kernels take).  n_classes <= 16.
 */
#ifndef ROBUSTBNNS_HIP_H
#define ROBUSTBNNS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RBNN_ABI_VERSION 10
#define RBNN_CPAD 16               /* class axis of P / dZ buffers is padded to 16 floats */

typedef enum rbnn_status {
    RBNN_OK = 0,
    RBNN_ERR_NULL = -1,            /* required pointer is NULL                      */
    RBNN_ERR_SHAPE = -2,           /* dimension violates the padding contract       */
    RBNN_ERR_UNSUPPORTED = -3,     /* arch / activation / mode not implemented      */
    RBNN_ERR_LAUNCH = -4,          /* HIP reported an error at launch               */
    RBNN_ERR_ALIGN = -5            /* pointer not 16-byte aligned                   */
} rbnn_status;

/* model_nn.py:66-75 */
typedef enum rbnn_activation { RBNN_ACT_RELU = 0, RBNN_ACT_LEAKY = 1, RBNN_ACT_SIGM = 2, RBNN_ACT_TANH = 3 } rbnn_activation;
/* model_nn.py:77-91 */
typedef enum rbnn_arch { RBNN_ARCH_FC = 0, RBNN_ARCH_FC2 = 1 } rbnn_arch;

/* What the stacked forward leaves in `P`:
 *   RBNN_OUT_PROBS  softmax(logits)  — BNN.forward, model_bnn.py:133-134, :253-255
 *   RBNN_OUT_LOGITS raw logits       — NN.forward / Ensemble_NN.forward, model_nn.py:139, model_ensemble.py:64 */
typedef enum rbnn_out_kind { RBNN_OUT_PROBS = 0, RBNN_OUT_LOGITS = 1 } rbnn_out_kind;

/* Which loss the input gradient is taken of:
 *   RBNN_LOSS_MEAN_PROB   CE(mean_s p_s, y)        fgsm/pgd on a BNN   adversarialAttacks.py:74-78, :97-101
 *   RBNN_LOSS_PER_SAMPLE  mean_s CE(p_s, y)        loss_gradient       lossGradients.py:29-40
 *   RBNN_LOSS_MEAN_LOGIT  CE(mean_s z_s, y)        fgsm/pgd on NN / Ensemble_NN (P holds logits)
 *   RBNN_LOSS_UPSTREAM    caller supplies dL/d(mean_s p_s) [N,C] (autograd hook on BNN.forward: the softmax backward is applied)
 *   RBNN_LOSS_UPSTREAM_LOGIT  caller supplies dL/d(mean_s z_s) [N,C] (autograd hook on NN / Ensemble_NN.forward: P holds logits) */
typedef enum rbnn_loss_mode { RBNN_LOSS_MEAN_PROB = 0, RBNN_LOSS_PER_SAMPLE = 1, RBNN_LOSS_MEAN_LOGIT = 2, RBNN_LOSS_UPSTREAM = 3,
                              RBNN_LOSS_UPSTREAM_LOGIT = 4 } rbnn_loss_mode;

/* Stacked posterior of a fully-connected net (model_nn.py:77-91; state_dict keys in comments). */
typedef struct rbnn_posterior {
    int32_t arch;                  /* rbnn_arch                                                  */
    int32_t activation;            /* rbnn_activation                                            */
    int32_t in_features;           /* D  (784 MNIST, 2 half-moons)                               */
    int32_t in_stride;             /* D_pad, multiple of 16: row stride of W1                    */
    int32_t hidden;                /* H: 32, 64 or a multiple of 128                             */
    int32_t n_classes;             /* C <= 16                                                    */
    int32_t n_stored;              /* S_total                                                    */
    int32_t reserved;
    const float *W1, *b1;          /* model.1.weight [S_total,H,D_pad], model.1.bias [S_total,H] */
    const float *Wm, *bm;          /* fc2 only: model.3.weight [S_total,H,H], model.3.bias       */
    const float *W2, *b2;          /* output layer (model.3 for fc, model.5 for fc2): [S_total,C,H], [S_total,C] */
    /* rbnn_pack_rows4() images of W1 / Wm: [S_total, H/4, cols, 4] — four consecutive hidden units interleaved per
     * column, so the backward GEMM's B operand (4 K steps of one column) is one 16-byte LDS read.  Required by
     * rbnn_fc_input_grad (Wm_pack4 for fc2 only); the forward reads the plain row-major W1 / Wm. */
    const float *W1_pack4, *Wm_pack4;
} rbnn_posterior;

/* Caller-owned scratch for one (N, S) problem; sizes from rbnn_workspace_query(). */
typedef struct rbnn_workspace {
    float    *P;                   /* [S,N,16]      per-sample probabilities (or logits)         */
    float    *dZ;                  /* [S,N,16]      dL/dlogits per sample                        */
    uint32_t *mask1;               /* [S,H/32,N_pad] bit h%32 of word [s][h/32][n] = (pre-activation > 0); N_pad = round_up(N,256) */
    float    *dact1;               /* [S,N,H]       act'(pre-activation), sigm/tanh only         */
    float    *hid1;                /* [S,N,H]       fc2: first hidden activations                */
    uint32_t *mask2;               /* fc2: as mask1 for the second hidden layer                  */
    float    *dact2;               /* fc2, sigm/tanh                                             */
    float    *dhid1;               /* [S,N,H]       fc2: dL/d(pre-activation 1)                  */
    float    *slabs;               /* [n_slabs,N,D_pad] partial input gradients                  */
} rbnn_workspace;

typedef struct rbnn_workspace_sizes {  /* bytes; 0 = not needed for this posterior */
    size_t P, dZ, mask1, dact1, hid1, mask2, dact2, dhid1, slabs;
    int32_t n_slabs;               /* slabs rbnn_fc_input_grad will write for (S, chunk)         */
    int32_t chunk;                 /* samples accumulated per slab (chosen if chunk<=0 passed)   */
} rbnn_workspace_sizes;

int rbnn_abi_version(void);
/* 0 for a product build.  Bit 0: a translation unit of this library was compiled with a timing-only ablation switch (RBNN_ABL,
 * RBNN_*_ABL_*, RBNN_FAST_BUILD — csrc/rbnn_common.hpp; such kernels compute WRONG results by design and need -DRBNN_ALLOW_ABLATION
 * to compile at all).  robustbnns_amd._hip.load() refuses a library whose flags are not 0 unless RBNN_ALLOW_ABLATION=1. */
int rbnn_build_flags(void);
const char *rbnn_strerror(int status);

/* Sizes of every workspace buffer for N points x S used samples.  chunk<=0: library picks. [host] */
int rbnn_workspace_query(const rbnn_posterior *net, int32_t n_points, int32_t n_samples,
                         int32_t chunk, rbnn_workspace_sizes *out);

/* Stacked per-sample forward: for every used sample s, P[s] = softmax(NN_s(X)) (or logits),
 * and the activation-derivative stash the backward needs.
 * Replaces: the `for seed in seeds: net.forward(inputs); softmax` loop, model_bnn.py:251-255,
 * with NN.forward = model_nn.py:126-141 (fc :77-82, fc2 :84-91), batched over all N points.
 * X: [N, ldx], ldx >= D_pad, multiple of 4. */
int rbnn_fc_forward(const rbnn_posterior *net, const float *X, int32_t ldx, int32_t n_points,
                    const int32_t *sample_idx, int32_t n_samples, int32_t out_kind,
                    const rbnn_workspace *ws, void *stream);

/* out[n,c] = scale * sum_s P[s,n,c]   (c < C; out row stride ldo floats).
 * Replaces torch.stack(preds).mean(0), model_bnn.py:257 (scale = 1/S); with scale = 1 it is the
 * local partial sum that the multi-GPU path all-reduces. */
int rbnn_reduce_samples(const float *P, int32_t n_samples, int32_t n_points, int32_t n_classes,
                        float scale, float *out, int32_t ldo, void *stream);

/* dZ[s,n,:] = dL/dlogits_s for the chosen loss; `Psum` [N,ldp] is sum_s P[s] over ALL samples of
 * the job (after the all-reduce when samples are sharded), `inv_S` = 1/(total samples),
 * `labels` int32[N] (argmax of the one-hot, lossGradients.py:23, adversarialAttacks.py:120),
 * `G_up` [N,ldp] only for RBNN_LOSS_UPSTREAM / RBNN_LOSS_UPSTREAM_LOGIT.
 * Replaces CrossEntropyLoss()(output,label) + the softmax part of loss.backward():
 * adversarialAttacks.py:76-78, :99-101; lossGradients.py:34-36 (closed form). */
int rbnn_loss_dlogits(int32_t mode, const float *P, const float *Psum, int32_t ldp, const float *G_up,
                      const int32_t *labels, int32_t n_samples, float inv_S, int32_t n_points,
                      int32_t n_classes, float *dZ, void *stream);

/* Partial expected input gradients: slabs[k,n,:] = sum_{s in chunk k} dA_s[n,:] . W1_s, with
 * dA_s = act'(A_s) * (dZ_s . W2_s) built on the fly from ws->dZ and the stash of rbnn_fc_forward.
 * Replaces the rest of loss.backward() down to image.grad (adversarialAttacks.py:78-79, :101;
 * lossGradients.py:36-40).  Writes *n_slabs_out slabs of [N, D_pad] into ws->slabs. [n_slabs_out: host] */
int rbnn_fc_input_grad(const rbnn_posterior *net, const int32_t *sample_idx, int32_t n_samples,
                       int32_t n_points, int32_t chunk, const rbnn_workspace *ws,
                       int32_t *n_slabs_out, void *stream);

/* out[n,d] = scale * sum_k slabs[k,n,d]  (d < D_pad; out row stride ldo).
 * Replaces torch.stack(loss_gradients,0).mean(0), lossGradients.py:40 (1/S is already in dZ). */
int rbnn_sum_slabs(const float *slabs, int32_t n_slabs, int32_t n_points, int32_t d_pad, float scale,
                   float *out, int32_t ldo, void *stream);

/* rbnn_sum_slabs with the norms of every point's result fused into the same pass (no second read of the gradients):
 * linf[n] = max_{d<D} |out[n,d]|, l2[n] = sqrt(sum_{d<D} out[n,d]^2)  (fp32, fixed summation order: reproducible).
 * Replaces np.max(np.abs(g)) / np.linalg.norm(g) per image in compute_vanishing_norms_idxs, lossGradients.py:91-94,102-105
 * (and plot_gradients_components.py:73-79).  `out` is bit-identical to rbnn_sum_slabs'. */
int rbnn_sum_slabs_norms(const float *slabs, int32_t n_slabs, int32_t n_points, int32_t d_pad, int32_t in_features, float scale,
                         float *out, int32_t ldo, float *linf, float *l2, void *stream);

/* alpha[n] = 2 / max_d X0[n,d]   — adversarialAttacks.py:89 (per image, from the clean image). */
int rbnn_pgd_alpha(const float *X0, int32_t ldx, int32_t n_points, int32_t in_features,
                   float *alpha, void *stream);

/* One attack step on all points, g = sum_k G[k] (n_slabs partial gradients, slab stride in floats):
 *   project == 0 (FGSM):  X = clamp(X + step*sign(g), 0, 1)                      adversarialAttacks.py:81-82
 *   project == 1 (PGD):   X = clamp(X0 + clamp(X + step*sign(g) - X0, -eps, eps), 0, 1)   :103-105
 * step = alpha[n] if alpha != NULL else alpha_scalar.  X is updated in place (X0 untouched);
 * only columns d < D are touched. */
int rbnn_attack_step(float *X, const float *X0, int32_t ldx, const float *G, int32_t n_slabs,
                     size_t slab_stride, int32_t ldg, const float *alpha, float alpha_scalar,
                     float eps, int32_t project, int32_t n_points, int32_t in_features, void *stream);

/* attack_evaluation's reductions, adversarialAttacks.py:179,186 (argmax == label counts) and
 * :30-51,60 (softmax applied again to the outputs, 1 - Linf difference).
 * out_orig/out_adv: [N,ldp] forward outputs (mean probs, or logits for NN/ensemble).
 * counts: int32[2] = {#correct original, #correct adversarial}, zeroed by this call; rob: [N]. */
int rbnn_eval_metrics(const float *out_orig, const float *out_adv, int32_t ldp, const int32_t *labels,
                      int32_t n_points, int32_t n_classes, int32_t *counts, float *rob, void *stream);

/* out[(r/4), c, r%4] = W[r, c] for a row-major [rows, cols] matrix (rows % 4 == 0): the packed weight image that
 * rbnn_fc_input_grad reads (rows = S_total*H of W1 [cols = D_pad] or of Wm [cols = H]).  One-off layout
 * transform at posterior-load time; no counterpart in the reference. */
int rbnn_pack_rows4(const float *W, int64_t rows, int32_t cols, float *out, void *stream);

/* A power-of-two operand scale that lives in DEVICE memory, so that the split images of data-dependent operands (the
 * inputs, and the activations they bound) need no device->host round trip: value * scale = hi + lo, scale = 2^exp. */
typedef struct rbnn_dev_scale {
    uint32_t absmax_bits;          /* bit pattern of the bound the exponent was derived from                    */
    int32_t  exp;                  /* 14 - ceil(log2(bound)), clamped to [-100, 100]; 0 for a zero / non-finite bound */
    float    scale;                /* 2^exp                                                                     */
    float    inv_scale;            /* 2^-exp                                                                    */
} rbnn_dev_scale;

/* out[0] <- scale of the inputs:        bound0 = max(floor_abs, max_{r,c<cols} |X[r,c]|)
 * out[1] <- scale of what they bound:   bound1 = min(cap, mul * bound0 + add)
 * (fc2: the layer-1 activations, mul = max_h sum_d |W1[h,d]|, add = max|b1|, cap = 1 for sigmoid / tanh else +inf;
 * conv: the pooled conv1 activations).  floor_abs = 1 when later iterates are clamp(., 0, 1) of something
 * (adversarialAttacks.py:105), else 0.  No counterpart in the reference (it computes in fp32).  Asynchronous on `stream`. */
int rbnn_input_scales(const float *X, int64_t rows, int32_t cols, int32_t ld, float floor_abs, float mul, float add,
                      float cap, rbnn_dev_scale *out, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * `conv` architecture (model_nn.py:93-106): Conv2d(Cin,32,5) -> act -> MaxPool2d(2) -> Conv2d(32,Hc,5) -> act ->
 * MaxPool2d(2, stride 1) -> Flatten -> Linear(NP2*Hc, C), all four activations (:66-75).  state_dict keys: model.0.*
 * model.3.* model.7.* (SURVEY 8a row a1).  Two input geometries:
 *   1x28x28  mnist / fashion_mnist — the only inputs the reference's conv accepts (:95-96) and sizes its head for (:106:
 *            NP2 = 49); pinned by the reference-generated fixtures;
 *   3x32x32  CIFAR-shaped (BASELINE.json configs[4]): NP2 = 81, a BUILD-DEFINED head (Hc/16 * 3072 of :106 would be wrong,
 *            SURVEY 8a note) — parity unpinned, checked against the fp64 oracle only.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct rbnn_conv_posterior {
    int32_t activation;            /* rbnn_activation                                              */
    int32_t hidden;                /* Hc = conv2 output channels, multiple of 16                   */
    int32_t n_classes;             /* C <= 16                                                      */
    int32_t n_stored;              /* S_total                                                      */
    int32_t in_channels;           /* Cin: 1 or 3                                                  */
    int32_t in_width;              /* square input width: 28 (Cin = 1) or 32 (Cin = 3); X rows hold Cin*W*W floats */
    const float *K1w, *K1b;        /* model.0.weight [S_total,32,Cin,5,5], model.0.bias [S_total,32] */
    const float *K2w, *K2b;        /* model.3.weight [S_total,Hc,32,5,5], model.3.bias [S_total,Hc] */
    const float *Fw, *Fb;          /* model.7.weight [S_total,C,NP2*Hc], model.7.bias [S_total,C]  */
    const float *K2w_ci;           /* [S_total,32,Hc/16,25,16]: model.3.weight regrouped [ci][hc block][tap][hc%16] (backward only) */
} rbnn_conv_posterior;

typedef struct rbnn_conv_workspace {
    float   *P, *dZ;               /* [S,N,16]                                                     */
    float   *P1;                   /* pooled+activated conv1 output, dense fp32 [S,N,32,P1W,P1W] (P1W = 12 / 14), or the 24 KiB split image per
                                      (s,n); sized by rbnn_conv_workspace_query (whole 1-KiB pieces per point)               */
    uint8_t *st1;                  /* [S,N,32*P1W*P1W] pool-1 stash: argmax (bits 0-1) | pre-activation > 0 (bit 2) */
    float   *Q2;                   /* [S,N,Hc*NP2]    pooled+activated conv2 output (the Linear's input) */
    uint8_t *st2;                  /* [S,N,Hc*NP2]    pool-2 stash, same encoding                  */
    float   *G;                    /* [S,N,Cin*W*W]   per-sample input gradients (backward)        */
} rbnn_conv_workspace;

typedef struct rbnn_conv_workspace_sizes { size_t P, dZ, P1, st1, Q2, st2, G; } rbnn_conv_workspace_sizes;

int rbnn_conv_workspace_query(const rbnn_conv_posterior *net, int32_t n_points, int32_t n_samples,
                              rbnn_conv_workspace_sizes *out);

/* Stacked per-sample forward of the conv net: P[s] = softmax(NN_s(X)) (or logits) + the two pooling stashes.
 * Replaces the sample loop of BNN.forward (model_bnn.py:251-255) with NN.forward = model_nn.py:98-106,126-141.
 * X: [N, ldx], 16-byte aligned (RBNN_ERR_ALIGN otherwise), ldx >= Cin*W*W, multiple of 4 (RBNN_ERR_SHAPE otherwise). */
int rbnn_conv_forward(const rbnn_conv_posterior *net, const float *X, int32_t ldx, int32_t n_points,
                      const int32_t *sample_idx, int32_t n_samples, int32_t out_kind,
                      const rbnn_conv_workspace *ws, void *stream);

/* Per-sample input gradients of the conv net: G[s,n,:] = dL_s/dx_n for the dZ left in ws->dZ by rbnn_loss_dlogits
 * (sum them with rbnn_sum_slabs(G, S, N, Cin*W*W, ...)).  Replaces loss.backward() through model_nn.py:98-106. */
int rbnn_conv_input_grad(const rbnn_conv_posterior *net, const int32_t *sample_idx, int32_t n_samples,
                         int32_t n_points, const rbnn_conv_workspace *ws, void *stream);

/* rbnn_conv_forward in split-half precision (the technique of the fc split mode applied to conv2, 98 % of the MACs; 1x28x28
 * inputs, relu / leaky only — RBNN_ERR_UNSUPPORTED otherwise):
 * K2_rows = rbnn_split_rows image of model.3.weight regrouped [S_total*Hc, 25 taps * 32 ci] (K tap-major) holding W * 2^k2_exp;
 * the pooled conv1 activations are carried as value * 2^p1_exp = hi + lo (the caller bounds them: |P1| <= max_c(sum|K1w_c| *
 * max|x| + |K1b_c|)).  ws->P1 holds the 24 KiB split image per (sample, point) (rbnn_conv_workspace_query sizes it);
 * same outputs as rbnn_conv_forward, and rbnn_conv_input_grad follows it unchanged.  p1_dev_scale != NULL: record [1] of
 * rbnn_input_scales, read on the device instead of p1_exp.  X: as for rbnn_conv_forward (16-byte aligned, ldx a multiple of 4). */
int rbnn_conv_forward_split(const rbnn_conv_posterior *net, const void *K2_rows, int32_t k2_exp, int32_t p1_exp,
                            const rbnn_dev_scale *p1_dev_scale, const float *X, int32_t ldx,
                            int32_t n_points, const int32_t *sample_idx, int32_t n_samples, int32_t out_kind,
                            const rbnn_conv_workspace *ws, void *stream);

/* rbnn_conv_forward with conv2 in the triple-split ("f16x6") mode (both geometries, all four activations): full-width fp32 operands as three
 * fp16 pieces, six exact product terms per product on the f16 matrix pipe, fp32 accumulation (see the triple-split section below).
 * K2_triple = rbnn_triple_rows image of model.3.weight regrouped [S_total*Hc, 25 taps * 32 ci] (K tap-major) holding W * 2^k2_exp;
 * the pooled conv1 activations (computed in fp32 by the exact conv1 kernel into ws->P1) are split on the fly, scaled by 2^p1_exp or
 * by record [1] of rbnn_input_scales (p1_dev_scale != NULL).  Same outputs as rbnn_conv_forward; rbnn_conv_input_grad follows it unchanged.
 * X: as for rbnn_conv_forward (16-byte aligned, ldx >= Cin*W*W and a multiple of 4: its conv1 reads each image row as float4). */
int rbnn_conv_forward_triple(const rbnn_conv_posterior *net, const void *K2_triple, int32_t k2_exp, int32_t p1_exp,
                             const rbnn_dev_scale *p1_dev_scale, const float *X, int32_t ldx, int32_t n_points,
                             const int32_t *sample_idx, int32_t n_samples, int32_t out_kind,
                             const rbnn_conv_workspace *ws, void *stream);

/* rbnn_conv_input_grad with conv2^T in the triple-split mode (both geometries, all four activations), DENSE form: conv2^T as one GEMM per tap
 * over the conv2 OUTPUT positions (64 at 1x28x28: one pass; 100 at 3x32x32: two passes over 64 + 36 positions whose col2im contributions
 * meet in wave-private partial images) — T[tap][ci][pos] = sum_hc W[hc][ci][tap] * dO2[hc][pos], every MFMA useful — + a col2im, instead of
 * a gather over a zero-padded gradient image (the fp32 and split kernels' form: 36-39 % of its MFMAs multiply padding; the triple kernel of
 * that form, rbnn_conv_input_grad_triple, was removed in ABI 9).  K2_dense = triple image of model.3.weight * 2^k2_exp regrouped
 * [S_total, ceil(Hc/32) K steps, 25 taps, 2 tiles of 16 ci][3 pieces][4 chunks of 8 hc][16 ci][8 hc] halves (hc zero-padded to a multiple of
 * 32; a piece = 1 KiB, fragment-major: the kernel loads it straight into the MFMA's A registers), as rbnn_conv_weight_images writes it; fw_l1 = max_f sum_c |model.7.weight[c, f]| bounds the routed gradients (a per-(sample, point) power-of-two scale is derived from
 * it and max|dZ|).  Same G as rbnn_conv_input_grad. */
int rbnn_conv_input_grad_dense(const rbnn_conv_posterior *net, const void *K2_dense, int32_t k2_exp, float fw_l1,
                               const int32_t *sample_idx, int32_t n_samples, int32_t n_points,
                               const rbnn_conv_workspace *ws, void *stream);

/* Both triple images of model.3.weight from the fp32 stack K2w [n_samples][hidden][32 ci x 25 taps] (nn.Conv2d's order) in one launch, at the
 * scale 2^k2_exp: K2_rows = what rbnn_conv_forward_triple reads (rbnn_triple_rows_grouped of the tap-major regrouping), K2_dense = what
 * rbnn_conv_input_grad_dense reads; either may be NULL.  Bit-identical to building them through rbnn_triple_rows and permuted copies; a
 * redrawable SVI stack calls it after every draw (robustbnns_amd/conv.py::ConvStackedPosterior.redraw). */
int rbnn_conv_weight_images(const float *K2w, int32_t n_samples, int32_t hidden, int32_t k2_exp, void *K2_rows, void *K2_dense, void *stream);

/* rbnn_conv_input_grad with conv2^T in split-half precision.  K2_bwd = rbnn_split_rows image of model.3.weight regrouped
 * [S_total*32 ci, (Hc/16 chunks) * 13 tap pairs * 4 * 8]: element (ci; chunk, t, lg, j) = W[hc = 16*chunk + 8*(lg&1) + j, ci,
 * tap = 2t + (lg>>1)] * 2^k2_exp (0 for the padded 26th tap); fw_l1 = max_f sum_c |model.7.weight[c, f]| bounds the routed
 * gradients (a per-(sample, point) power-of-two scale is derived from it and max|dZ|).  Same G as rbnn_conv_input_grad. */
int rbnn_conv_input_grad_split(const rbnn_conv_posterior *net, const void *K2_bwd, int32_t k2_exp, float fw_l1,
                               const int32_t *sample_idx, int32_t n_samples, int32_t n_points,
                               const rbnn_conv_workspace *ws, void *stream);

/* W[s,i] = loc[i] + softplus(scale_raw[i]) * eps[s,i]   — the SVI guide's draw, model_bnn.py:124-130
 * (Normal(loc, softplus(scale)).rsample()).  PARITY UNPINNED: pyro-ppl 1.3.0 is not available;
 * eps is supplied by the caller.  out row stride ld_out >= n_elem (lets W1 be written D_pad-strided
 * by calling once per row block). */
int rbnn_svi_materialize(const float *loc, const float *scale_raw, const float *eps, int64_t n_elem,
                         int32_t n_samples, float *out, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Split-half precision mode ("f16x3") of the fc forward / input-gradient contractions.  No counterpart in the
 * reference (it computes in fp32): every fp32 operand v is carried as v * 2^e = hi + lo with hi, lo fp16, products
 * are hi*hi' + hi*lo' + lo*hi' on the f16 matrix pipe with fp32 accumulation (2^-22 per product; the parity tests
 * hold this mode to the same 1e-5 bar as the exact mode).  hidden % 128 == 0, <= 10 classes; arch fc and fc2, all four activations.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct rbnn_split_images {
    const void *W1_rows;           /* rbnn_split_rows image of W1 viewed as [S_total*H, D] rows: [S_total,H,ld_rows/8,2,8] halves */
    const void *W1_cols;           /* rbnn_split_cols image of W1 (backward B operand): [S_total,H/32,4,2,ld_cols,8] halves        */
    const void *W2_gen;            /* rbnn_split_w2gen image of W2 (backward dA generator): [S_total,H/16,64,8] halves             */
    int32_t ld_rows;               /* columns per row of W1_rows, multiple of 32, >= D                                            */
    int32_t ld_cols;               /* columns of W1_cols = in_stride (D_pad)                                                      */
    int32_t w1_exp;                /* W1_rows and W1_cols hold W1 * 2^w1_exp                                                      */
    int32_t w2_exp;                /* W2_gen holds W2 * 2^w2_exp                                                                  */
    /* fc2: */
    const void *Wm_rows;           /* rbnn_split_rows image of Wm viewed as [S_total*H, H] rows, holding Wm * 2^wm_exp (forward)   */
    const void *Wm_cols;           /* rbnn_split_cols image of Wm [S_total,H/32,4,2,H,8] (backward step 1); W2_gen is then built    */
                                   /* from the OUTPUT layer (model.5), w2_exp its exponent                                        */
    int32_t wm_exp;
    int32_t h1_exp;                /* layer-1 activations are carried as h * 2^h1_exp = hi + lo in ws->hid1; set per call from the  */
                                   /* bound max_h sum_d |W1[h,d]| * max|x| + max|b1|                                              */
} rbnn_split_images;

/* per-problem scratch of the split mode */
typedef struct rbnn_split_workspace {
    void  *X_split;                /* [N, ld_rows] split-rows image of the current inputs (caller fills it with rbnn_split_rows) */
    void  *dZ_gen;                 /* [S, N_pad, 64 B] dA-generator image of dZ, written by rbnn_fc_input_grad_split              */
    float *g_scale;                /* [N_pad] per-point 2^-e(n) of that image                                                     */
} rbnn_split_workspace;
typedef struct rbnn_split_workspace_sizes { size_t X_split, dZ_gen, g_scale; } rbnn_split_workspace_sizes;

int rbnn_split_workspace_query(const rbnn_posterior *net, const rbnn_split_images *sp, int32_t n_points,
                               int32_t n_samples, rbnn_split_workspace_sizes *out);


/* dst[r, g, 0, :] = fp16(v), dst[r, g, 1, :] = fp16(v - hi) for v = src[r, 8g..8g+7] * 2^scale_exp (0 past `cols`):
 * the split-rows image [rows, ld_dst/8, 2, 8] halves of a row-major fp32 matrix.  ld_dst % 32 == 0.
 * The caller picks scale_exp so that max|v| * 2^scale_exp <= 2^14; with dev_scale != NULL the scale is read from that device
 * record instead (rbnn_input_scales) and scale_exp is ignored. */
int rbnn_split_rows(const float *src, int64_t rows, int32_t cols, int32_t ld_src, int32_t scale_exp,
                    const rbnn_dev_scale *dev_scale, void *dst, int32_t ld_dst, void *stream);

/* Split-cols image of n_mats row-major [rows, ld_src] matrices (rows % 32 == 0):
 * dst[m, hb, lg, p, d, j] = (p ? lo : hi) of W[m, 32*hb + 16*(j>>2) + 4*lg + (j&3), d] * 2^scale_exp, 8 halves j per
 * 16-byte unit, ld_dst columns (% 16 == 0, zero past `cols`).  One-off at posterior load. */
int rbnn_split_cols(const float *W, int64_t n_mats, int32_t rows, int32_t cols, int32_t ld_src, int32_t scale_exp,
                    void *dst, int32_t ld_dst, void *stream);

/* dA-generator image of the output layer W2 [n_mats, C, H] (C <= 10): per 16 hidden units one 1-KiB tile holding,
 * per MFMA lane, the W2 side (hi, lo, hi) of the 30 K slots 10*p + c.  One-off at posterior load. */
int rbnn_split_w2gen(const float *W2, int32_t n_mats, int32_t n_classes, int32_t hidden, int32_t scale_exp, void *dst,
                     void *stream);

/* rbnn_fc_forward in split precision: same outputs (ws->P, ws->mask1 / ws->dact1), inputs as split-rows images:
 * X_split = rbnn_split_rows(X, N, D, ldx_src, x_exp, ., ldx) with ldx == sp->ld_rows.  dev_scales != NULL: the two records
 * of rbnn_input_scales — [0] replaces x_exp, [1] replaces sp->h1_exp (fc2) — read on the device. */
int rbnn_fc_forward_split(const rbnn_posterior *net, const rbnn_split_images *sp, const void *X_split, int32_t ldx,
                          int32_t x_exp, const rbnn_dev_scale *dev_scales, int32_t n_points, const int32_t *sample_idx,
                          int32_t n_samples, int32_t out_kind, const rbnn_workspace *ws, void *stream);

/* rbnn_fc_input_grad in split precision: same slabs (ws->slabs, already un-scaled), from ws->dZ and ws->mask1.
 * n_classes <= 10 (fc2: two steps through ws->dhid1).  Re-scales dZ per point (2^e(n), so vanishing gradients keep their 22 bits). */
int rbnn_fc_input_grad_split(const rbnn_posterior *net, const rbnn_split_images *sp, const int32_t *sample_idx,
                             int32_t n_samples, int32_t n_points, int32_t chunk, const rbnn_workspace *ws,
                             const rbnn_split_workspace *sws, int32_t *n_slabs_out, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Triple-split mode ("f16x6") of the fc forward / input-gradient contractions: fp32 operands at FULL width on the f16
 * matrix pipe.  No counterpart in the reference (it computes in fp32).  v * 2^e = p0 + p1 + p2 with p_i fp16 — exact,
 * bit for bit, for |v| >= 2^-15 * max|tensor| (3 x 11 significand bits cover fp32's 24; within 2^-39 * max|tensor| below
 * that) — and a*b = a0*b2 + a2*b0 + a1*b1 + a1*b0 + a0*b1 + a0*b0 (six f16 MFMAs, exact terms; the dropped terms are
 * <= 2^-32 |a*b|), accumulated in fp32: the only rounding left is the fp32 accumulation, as in rbnn_fc_forward / rbnn_fc_input_grad.
 * Architectures fc and fc2, hidden % 128 == 0, all four activations, <= 10 classes in the input gradient.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct rbnn_triple_images {
    const void *W1_rows;           /* rbnn_triple_rows_grouped image of W1 viewed as [S_total*H, D] rows: [S_total*H/16,ld_rows/32,3,16,32] halves */
    const void *W1_cols;           /* rbnn_triple_cols image of W1 (backward B operand): [S_total,H/32,4,3,ld_cols,8] halves         */
    const void *W2_gen;            /* rbnn_triple_w2gen image of the OUTPUT layer (backward dA generator): [S_total,H/16,2,64,8] halves */
    int32_t ld_rows;               /* columns per row of W1_rows, multiple of 32, >= D                                              */
    int32_t ld_cols;               /* columns of W1_cols = in_stride (D_pad)                                                        */
    int32_t w1_exp;                /* W1_rows and W1_cols hold W1 * 2^w1_exp                                                        */
    int32_t w2_exp;                /* W2_gen holds the output layer * 2^w2_exp                                                      */
    /* fc2: */
    const void *Wm_rows;           /* rbnn_triple_rows_grouped image of Wm viewed as [S_total*H, H] rows, holding Wm * 2^wm_exp (forward) */
    const void *Wm_cols;           /* rbnn_triple_cols image of Wm [S_total,H/32,4,3,H,8] (backward step 1)                         */
    int32_t wm_exp;
    int32_t h1_exp;                /* layer-1 activations are carried as h * 2^h1_exp = p0 + p1 + p2 in tws->hid_triple; set from the */
                                   /* bound max_h sum_d |W1[h,d]| * max|x| + max|b1| (or record [1] of rbnn_input_scales)           */
} rbnn_triple_images;

/* per-problem scratch of the triple mode */
typedef struct rbnn_triple_workspace {
    void  *X_triple;               /* [ceil16(N), ld_rows] grouped triple-rows image of the current inputs (rbnn_triple_rows_grouped) */
    void  *dZ_gen;                 /* [S, N_pad, 64 B] dA-generator image of dZ, written by rbnn_fc_input_grad_triple               */
    float *g_scale;                /* [N_pad] per-point 2^-e(n) of that image                                                       */
    void  *hid_triple;             /* fc2: the hidden activations x 2^h1_exp as FP32, [S, H/32 stages, ceil(N/16) groups, 16 points, 32 units] (ABI 9; until then three fp16 pieces); layer 2 splits at its operand read */
} rbnn_triple_workspace;
typedef struct rbnn_triple_workspace_sizes { size_t X_triple, dZ_gen, g_scale, hid_triple; } rbnn_triple_workspace_sizes;

int rbnn_triple_workspace_query(const rbnn_posterior *net, const rbnn_triple_images *tp, int32_t n_points,
                                int32_t n_samples, rbnn_triple_workspace_sizes *out);

/* dst[r, k, p, :] = piece p (p0 = fp16(v), p1 = fp16(v - p0), p2 = fp16(v - p0 - p1)) of v = src[r, 32k..32k+31] * 2^scale_exp
 * (0 past `cols`): the triple-rows image [rows, ld_dst/32, 3, 32] halves.  ld_dst % 32 == 0.  scale_exp / dev_scale as rbnn_split_rows. */
int rbnn_triple_rows(const float *src, int64_t rows, int32_t cols, int32_t ld_src, int32_t scale_exp,
                     const rbnn_dev_scale *dev_scale, void *dst, int32_t ld_dst, void *stream);

/* The same pieces in the GROUPED order the fc forward kernel reads (W1_rows, Wm_rows, X_triple): 16 consecutive rows share one 3-KiB block
 * per K stage, dst[r / 16, k, p, r % 16, :] — [rows/16, ld_dst/32, 3, 16, 32] halves.  A 16-row group then sits in memory exactly as in the
 * kernel's stage tile, so its three LDS-DMA pieces (1 KiB apart on both sides) share one address and one M0 write.  Rows past `rows` in the
 * last group are left untouched: size dst for ceil(rows / 16) * 16 rows.  Same arguments as rbnn_triple_rows. */
int rbnn_triple_rows_grouped(const float *src, int64_t rows, int32_t cols, int32_t ld_src, int32_t scale_exp,
                             const rbnn_dev_scale *dev_scale, void *dst, int32_t ld_dst, void *stream);

/* Triple-cols image of n_mats row-major [rows, ld_src] matrices (rows % 32 == 0):
 * dst[m, hb, lg, p, d, j] = piece p of W[m, 32*hb + 16*(j>>2) + 4*lg + (j&3), d] * 2^scale_exp.  One-off at posterior load. */
int rbnn_triple_cols(const float *W, int64_t n_mats, int32_t rows, int32_t cols, int32_t ld_src, int32_t scale_exp,
                     void *dst, int32_t ld_dst, void *stream);

/* dA-generator image of the output layer W2 [n_mats, C, H] (C <= 10): per 16 hidden units one 2-KiB tile = the W2 side of the
 * two chained generator MFMAs (K-slot plan in rbnn_triple.hip).  One-off at posterior load. */
int rbnn_triple_w2gen(const float *W2, int32_t n_mats, int32_t n_classes, int32_t hidden, int32_t scale_exp, void *dst,
                      void *stream);

/* rbnn_fc_forward on triple images: same outputs (ws->P, ws->mask1 / ws->dact1; fc2: ws->mask2 / ws->dact2).  tws->X_triple =
 * rbnn_triple_rows_grouped(X, N, D, ., x_exp, ., tp->ld_rows); dev_scales != NULL: the two records of rbnn_input_scales — [0] replaces
 * x_exp, [1] replaces tp->h1_exp (fc2) — read on the device. */
int rbnn_fc_forward_triple(const rbnn_posterior *net, const rbnn_triple_images *tp, const rbnn_triple_workspace *tws,
                           int32_t x_exp, const rbnn_dev_scale *dev_scales, int32_t n_points, const int32_t *sample_idx,
                           int32_t n_samples, int32_t out_kind, const rbnn_workspace *ws, void *stream);

/* rbnn_fc_input_grad on triple images: same slabs (ws->slabs, already un-scaled), from ws->dZ and ws->mask1 (fc2: two steps
 * through ws->dhid1, with ws->mask2).  Re-scales dZ per point (2^e(n)) like rbnn_fc_input_grad_split. */
int rbnn_fc_input_grad_triple(const rbnn_posterior *net, const rbnn_triple_images *tp, const int32_t *sample_idx,
                              int32_t n_samples, int32_t n_points, int32_t chunk, const rbnn_workspace *ws,
                              const rbnn_triple_workspace *tws, int32_t *n_slabs_out, void *stream);

/* The tail of a step between the two GEMM calls, fused (round 4): what rbnn_reduce_samples (scale 1) + rbnn_loss_dlogits + the dZ re-scaling
 * inside rbnn_fc_input_grad_triple compute, in ONE launch, bit for bit — P [n_samples][n_points][16] in, tws->dZ_gen / tws->g_scale out;
 * the fp32 dZ buffer is not written at all.  mode: RBNN_LOSS_MEAN_PROB (adversarialAttacks.py:74-78), RBNN_LOSS_PER_SAMPLE
 * (lossGradients.py:29-40) or RBNN_LOSS_MEAN_LOGIT (ensemble / NN); inv_S as rbnn_loss_dlogits.  Psum_out (nullable): sum_s P [n_points][ldo].
 * rbnn_fc_input_grad_triple called afterwards with ws->dZ == NULL takes the image as given (it skips its own re-scaling launch).
 * Single-GPU only: the sample-sharded step needs its all-reduce between the sum and the loss (AttackEngine._step_sharded). */
int rbnn_step_tail_triple(int32_t mode, const float *P, const int32_t *labels, int32_t n_samples, float inv_S, int32_t n_points,
                          int32_t n_classes, float *Psum_out, int32_t ldo, const rbnn_triple_workspace *tws, void *stream);

/* rbnn_attack_step + rbnn_triple_rows_grouped of the NEW iterate in one pass (bit-identical X and image): inside a PGD loop
 * (adversarialAttacks.py:95-105) the next iteration's forward then needs no image-builder launch.  dev_scale: record [0] of
 * rbnn_input_scales (computed once per attack with floor_abs = 1); X_triple: ceil16(n_points) x ld_rows grouped image. */
int rbnn_attack_step_triple(float *X, const float *X0, int32_t ldx, const float *G, int32_t n_slabs, size_t slab_stride, int32_t ldg,
                            const float *alpha, float alpha_scalar, float eps, int32_t project, int32_t n_points, int32_t in_features,
                            const rbnn_dev_scale *dev_scale, void *X_triple, int32_t ld_rows, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * The SVI guide's draw written IN PLACE into a stacked posterior and all of its weight images, one launch, no eps tensor.
 * Replaces the per-forward pyro.random_module(basenet, Normal(loc, softplus(scale)))() of model_bnn.py:121-136 called S times per
 * prediction (:222-232): W[s] = loc + sigma * eps(s) for every tensor of the net (sigma = softplus(raw scale)), eps = Box-Muller of
 * Philox4x32-10(counter = (element quad, tensor id, s or 0, draw_id), key = sample_keys[s] or key).  PARITY UNPINNED against
 * pyro-ppl 1.3.0's RNG stream (the package is not available to check it against).
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct rbnn_svi_guide {    /* device pointers to the variational parameters, UNPADDED row-major as the param store holds them;     */
                                   /* *_scale = the STANDARD DEVIATION softplus(raw `<key>_scale`) (model_bnn.py:127), taken once per guide */
    const float *W1_loc, *W1_scale;   /* model.1.weight_loc, softplus(model.1.weight_scale)  [hidden, in_features]                   */
    const float *b1_loc, *b1_scale;   /* model.1.bias                  [hidden]                                                      */
    const float *Wm_loc, *Wm_scale;   /* fc2: model.3.weight           [hidden, hidden]                                              */
    const float *bm_loc, *bm_scale;   /* fc2: model.3.bias             [hidden]                                                      */
    const float *W2_loc, *W2_scale;   /* output layer weight           [n_classes, hidden]                                           */
    const float *b2_loc, *b2_scale;   /* output layer bias             [n_classes]                                                   */
    int32_t hidden;                   /* the net's own hidden size (<= net->hidden: 16 is stored padded to 32, padding stays zero)   */
    int32_t reserved;
} rbnn_svi_guide;

/* Writes samples [0, n_samples) of `net`: W1 b1 (Wm bm) W2 b2 — the pointers are const in rbnn_posterior because every other entry
 * point only reads them; this one writes through them — plus W1_pack4 / Wm_pack4 when non-NULL, plus, when `tp` is non-NULL, the
 * triple images W1_rows, W1_cols, W2_gen (Wm_rows, Wm_cols) at the scales tp->w1_exp / w2_exp / wm_exp, which the caller fixes per
 * guide from the bound |w| <= |loc| + RBNN_SVI_EPS_MAX * sigma.  sample_keys: device array of n_samples 64-bit keys (one
 * seed per sample: model_bnn.py:222-226) or NULL (all samples under `key`, the sample index in the counter).  Asynchronous on `stream`. */
#define RBNN_SVI_EPS_MAX 6.77f
int rbnn_svi_draw(const rbnn_posterior *net, const rbnn_triple_images *tp, const rbnn_svi_guide *guide, int32_t n_samples,
                  const uint64_t *sample_keys, uint64_t key, uint32_t draw_id, void *stream);
/* The same draw for a caller that is about to run the TRIPLE kernels only: W1 (Wm) are written as their triple images (12 B per weight), not
 * as the fp32 stack + its pack_rows4 image (8 B per weight: 40 % of rbnn_svi_draw's writes, read by no triple kernel); b1 (bm) W2 b2 and the W2
 * generator image as always.  Whoever needs the fp32 W1 / Wm later calls rbnn_svi_draw with the same (key, draw_id): the same weights
 * (robustbnns_amd.posterior.StackedPosterior.materialize).  tp must not be NULL. */
int rbnn_svi_draw_images(const rbnn_posterior *net, const rbnn_triple_images *tp, const rbnn_svi_guide *guide, int32_t n_samples,
                         const uint64_t *sample_keys, uint64_t key, uint32_t draw_id, void *stream);
/* 1 when rbnn_svi_draw covers this posterior (fc / fc2; W2 [n_classes, hidden] fits the 160 KB of LDS it is staged in; with triple
 * images: n_classes <= 10, hidden % 128 == 0) — the host falls back to rbnn_svi_materialize + a new stack otherwise. */
int rbnn_svi_draw_supported(const rbnn_posterior *net, int32_t with_triple_images);

/* The same draw for tensors of any shape (the conv architecture: model.0 / .3 / .7 weights and biases), written IN PLACE into the fp32
 * stack: out[s, e] = loc[e] + sigma[e] * eps, eps of element e = component e % 4 of the Philox block with counter
 * (e / 4, tensor_id, s — or 0 when sample_keys is given —, draw_id).  One launch for up to 8 tensors and all samples; images derived
 * from the stack (the regrouped / triple images of the conv2 weights) are rebuilt by their builders (robustbnns_amd/conv.py). */
typedef struct rbnn_svi_flat_tensor {
    const float *loc, *sigma;         /* [n_elem] variational mean and standard deviation softplus(raw scale) */
    float *out;                       /* [n_samples, out_sample_stride] destination, first n_elem of each row  */
    int64_t n_elem, out_sample_stride;
    int32_t tensor_id, reserved;
} rbnn_svi_flat_tensor;
int rbnn_svi_draw_flat(const rbnn_svi_flat_tensor *tensors, int32_t n_tensors, int32_t n_samples, const uint64_t *sample_keys, uint64_t key,
                       uint32_t draw_id, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Low-dimensional nets (in_features <= 16, n_classes <= 10; half-moons: 2 -> H -> 2) — arch fc: the WHOLE hot path in one launch.
 * One call = what a sequence of rbnn_fc_forward, rbnn_reduce_samples, rbnn_loss_dlogits, rbnn_fc_input_grad, rbnn_sum_slabs(_norms),
 * rbnn_pgd_alpha and `iters` x rbnn_attack_step computes, i.e. for every point the loop nest adversarialAttacks.py:118 -> :95 ->
 * model_bnn.py:251 (attack), lossGradients.py:20-40 (gradient) or model_bnn.py:243-258 (forward), in fp32 FMA arithmetic.
 *   op RBNN_LOWDIM_FORWARD   out[N, ldo]  = out_scale * sum_s (probabilities | logits per out_kind) of the samples
 *   op RBNN_LOWDIM_GRADIENT  out[N, ldo]  = out_scale * sum_s dL_s/dx for loss_mode (MEAN_PROB, PER_SAMPLE, MEAN_LOGIT; inv_S as
 *                            rbnn_loss_dlogits), linf / l2 (nullable): the per-point norms of that gradient (lossGradients.py:91-105)
 *   op RBNN_LOWDIM_ATTACK    out[N, ldo]  = the iterate after `iters` steps from X towards the eps-ball around X0 (project != 0) or one
 *                            FGSM step (project == 0); step size alpha[n], or 2 / max(X0[n]) when alpha_per_image
 *                            (adversarialAttacks.py:89), or alpha_scalar
 * P_scratch: [n_samples, n_points, 16] floats (required for MEAN_PROB gradients / attacks).  sample_idx as rbnn_fc_forward.
 * ------------------------------------------------------------------------------------------------------------ */
/* fc2 (round 4; the reference's half-moons grid, grid_search_halfMoons.py:159-169: 2 -> H -> H -> 2, 250 HMC samples): hidden in
 * {32, 64, 128, 256, 512}, in_stride == 16, Wm_pack4 required.  The H x H layer is a GEMM over the points of a sample (fp32 MFMA), so
 * samples spread over the CUs and the mean over samples couples all blocks between forward and backward: one call issues, back to
 * back on `stream`, per iteration: forward kernel, sum over samples, backward kernel, slab sum + step (4 launches; 2 for the
 * per-sample loss) — csrc/rbnn_lowdim.hip.  relu / leaky: the forward kernel leaves one sign bit per hidden unit and (sample, point)
 * and the backward kernel starts at dL/dlogits; sigmoid / tanh and the per-sample loss (which has no forward launch): the backward
 * kernel recomputes the forward.  Same arguments and results as for fc, except that P_scratch must hold rbnn_lowdim_scratch_bytes()
 * bytes (per-sample outputs, per-sample gradient slabs, the sum over samples, the sign bits), is always required, and for
 * RBNN_LOWDIM_ATTACK `out` must not alias X (the iterate is kept in `out`: iteration 0 reads X with row stride ldx, every later one reads
 * `out` with ITS row stride ldo — the two strides are independent, a compact out beside a padded X is legal; X0 always has X's stride). */
typedef enum rbnn_lowdim_op { RBNN_LOWDIM_FORWARD = 0, RBNN_LOWDIM_GRADIENT = 1, RBNN_LOWDIM_ATTACK = 2 } rbnn_lowdim_op;
int rbnn_lowdim_supported(const rbnn_posterior *net);      /* 1 when rbnn_lowdim_run covers this posterior */
size_t rbnn_lowdim_scratch_bytes(const rbnn_posterior *net, int32_t n_points, int32_t n_samples);   /* bytes of P_scratch (0: bad arguments) */
int rbnn_lowdim_run(const rbnn_posterior *net, int32_t op, int32_t loss_mode, int32_t out_kind, const float *X, const float *X0,
                    int32_t ldx, int32_t n_points, const int32_t *sample_idx, int32_t n_samples, const int32_t *labels, float inv_S,
                    float out_scale, float eps, const float *alpha, float alpha_scalar, int32_t alpha_per_image, int32_t project,
                    int32_t iters, float *P_scratch, float *out, int32_t ldo, float *linf, float *l2, void *stream);

/* rbnn_svi_draw + rbnn_lowdim_run in ONE launch (arch fc, small posteriors: every block generates the weights of all samples of the call into its
 * LDS cache from the guide — loc + sigma * eps(key or sample_keys[s], draw_id, tensor, sample, quad), rbnn_svi_draw's generator, the same
 * weights — instead of copying them from the stack).  The stack is NOT written: a caller that needs it afterwards runs rbnn_svi_draw with the
 * same (key, draw_id) (robustbnns_amd.posterior.StackedPosterior.materialize).  BASELINE config 1 (half-moons, SVI): a redraw + an FGSM pass
 * was two launches at the launch floor.  rbnn_lowdim_fused_draw_supported: 1 when the call's samples fit the kernel's 60 KB weight cache. */
int rbnn_lowdim_fused_draw_supported(const rbnn_posterior *net, int32_t n_points, int32_t n_samples);
int rbnn_lowdim_run_svi(const rbnn_posterior *net, const rbnn_svi_guide *guide, const uint64_t *sample_keys, uint64_t key, uint32_t draw_id,
                        int32_t op, int32_t loss_mode, int32_t out_kind, const float *X, const float *X0, int32_t ldx, int32_t n_points,
                        const int32_t *sample_idx, int32_t n_samples, const int32_t *labels, float inv_S, float out_scale, float eps,
                        const float *alpha, float alpha_scalar, int32_t alpha_per_image, int32_t project, int32_t iters, float *P_scratch,
                        float *out, int32_t ldo, float *linf, float *l2, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * SVI training of fc / fc2 guides (csrc/rbnn_train.hip).  One training step of model_bnn.py:303-365 (SVI with TraceMeanField_ELBO and
 * pyro.optim.Adam) on a batch of B points: draw ONE weight sample, loss L = sum_b CE(z_b, y_b) + sum KL(N(loc, sigma) || N(0, 1)), its
 * gradients, one torch.optim.Adam step on every loc and raw scale.  Issued in this order on one stream:
 *   draw -> train_forward -> weight_grads -> adam_step -> [accuracy forward] -> train_finalize.
 * Parameters live in FLAT buffers of n_params floats: the state_dict tensors in order (model.1.weight [H, D], model.1.bias [H],
 * (fc2: model.3.weight [H, H], model.3.bias [H],) output weight [C, H], output bias [C]), unpadded, row-major.  eps is rbnn_svi_draw's
 * generator at sample 0 (counter (quad, tensor id, 0, draw_id), quad = r * ceil(cols/4) + c/4): the same (key, draw_id) gives the same
 * weights as rbnn_svi_draw's sample 0, and the update regenerates eps instead of storing it.  No atomics: two runs are bit-identical.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct rbnn_svi_train_net {
    int32_t arch;                  /* rbnn_arch                                                                    */
    int32_t activation;            /* rbnn_activation                                                              */
    int32_t in_features, hidden, n_classes;    /* D (any), H (the net's own, unpadded), C <= 16                    */
    int32_t reserved;
    float *loc, *raw, *sigma;      /* [n_params] variational mean, raw scale, sigma = softplus(raw) (written by the update)   */
    float *m_loc, *v_loc, *m_raw, *v_raw;      /* [n_params] Adam moments (zero before the first step)             */
    float *W;                      /* [n_params] the drawn weight sample                                           */
    float *grad;                   /* [n_params] dCE/dW of the step                                                */
} rbnn_svi_train_net;

typedef struct rbnn_svi_train_ws { /* caller-owned, for up to B points                                              */
    float *hid1, *dact1, *dA1;     /* [B, H] layer-1 activations, act'(pre-activation), dL/d(pre-activation)      */
    float *hid2, *dact2, *dA2;     /* [B, H] fc2 only: the same for the second hidden layer                       */
    float *dZ;                     /* [B, 16] dL/dlogits                                                           */
    float *ce;                     /* [B] cross-entropy per point                                                  */
} rbnn_svi_train_ws;

/* [host] n_params (the flat buffers' length); *n_partials (nullable) = the KL partial sums rbnn_svi_adam_step writes.  < 0: rbnn_status. */
int64_t rbnn_svi_train_sizes(const rbnn_svi_train_net *net, int64_t *n_partials);
/* W = loc + sigma * eps(key, draw_id): one launch. */
int rbnn_svi_train_draw(const rbnn_svi_train_net *net, uint64_t key, uint32_t draw_id, void *stream);
/* The training forward on W: hidden activations, act', logits, ce[b] = CE(z_b, labels[b]), dZ = softmax(z) - e_y (summed CE: no 1/B), and
 * the backward to dA1 (fc2: dA2, then dA1) — fc 2 launches, fc2 4.  X [B, ldx] fp32 (ldx >= D), labels int32[B] in [0, C). */
int rbnn_svi_train_forward(const rbnn_svi_train_net *net, const float *X, int32_t ldx, int32_t n_points, const int32_t *labels,
                           const rbnn_svi_train_ws *ws, void *stream);
/* grad = dCE/dW of every tensor (dW1 = dA1^T X, dWm = dA2^T H1, dW2 = dZ^T H, the biases as column sums): one launch, fp32 MFMA. */
int rbnn_svi_weight_grads(const rbnn_svi_train_net *net, const float *X, int32_t ldx, int32_t n_points, const rbnn_svi_train_ws *ws,
                          void *stream);
/* One torch.optim.Adam step (single-tensor formula, no weight decay) on loc and raw with g_loc = grad + loc,
 * g_raw = (grad * eps + sigma - 1/sigma) * sigmoid(raw), eps regenerated from (key, draw_id); `step` = the step number t >= 1 of the
 * bias corrections.  Writes loc, raw, sigma = softplus(raw), the moments, and kl_partials[i] = the KL of the PRE-update parameters
 * summed over block i (n_partials of rbnn_svi_train_sizes).  lr, the betas and eps are doubles (ABI 10), as torch's Python floats: the
 * step size lr / (1 - beta1^t), sqrt(1 - beta2^t) and the weights 1 - beta1, 1 - beta2 are formed in double and rounded to fp32 ONCE, as
 * torch's scalar arguments are (1 - 0.999f in fp32 is 1.3e-5 off 0.001). */
int rbnn_svi_adam_step(const rbnn_svi_train_net *net, uint64_t key, uint32_t draw_id, int64_t step, double lr, double beta1, double beta2,
                       double adam_eps, float *kl_partials, void *stream);
/* One block, fixed order, fp64: stats[0] = sum kl_partials + sum_b ce[b] (the step's loss), stats[1] += stats[0]; Psum [B, ldp] (nullable:
 * sum over samples of the accuracy forward's probabilities): stats[2] += #{b : first argmax_c Psum[b, c] == labels[b]}. */
int rbnn_svi_train_finalize(const float *kl_partials, int64_t n_partials, const float *ce, int32_t n_points, const float *Psum, int32_t ldp,
                            const int32_t *labels, int32_t n_classes, double *stats, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Deterministic training of fc / fc2 nets (csrc/rbnn_nn_train.hip): torch.optim.Adam on nn.CrossEntropyLoss() (model_nn.py:175-219), for
 * n_members independent nets of the same shape in LOCKSTEP (the deep ensemble of model_ensemble.py:69-83): every launch covers all members.
 * Issued in this order on one stream:  train_forward -> weight_grads -> adam_step -> train_finalize.
 * Parameters, Adam moments and gradients are flat per-member buffers in the layout of the SVI trainer above (state_dict order, unpadded,
 * row-major); member m sits at m * member_stride floats.  The batch of member m is rows[m, 0..B) of a RESIDENT data matrix X [n_rows, ldx]
 * (int32 indices; labels go through the same indices); rows == NULL: rows 0..B-1 of X for every member (a staged batch).  An index outside
 * [0, n_rows) is clamped into it.  Workspaces are packed [n_members, B, .] for the call's B.  No atomics, no sum across members: member m
 * of a lockstep run is bit-identical to that member run alone, and two runs are bit-identical.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct rbnn_nn_train_net {
    int32_t arch;                  /* rbnn_arch                                                                    */
    int32_t activation;            /* rbnn_activation                                                              */
    int32_t in_features, hidden, n_classes;    /* D (any), H (any), C <= 16                                        */
    int32_t n_members;             /* M, 1 .. 65535                                                                */
    float *P;                      /* [M, member_stride] parameters                                                */
    float *m, *v;                  /* [M, member_stride] Adam moments (zero before the first step)                 */
    float *grad;                   /* [M, member_stride] dL/dP of the step (L = mean CE of the member's batch)     */
    int64_t member_stride;         /* floats between members, >= n_params                                          */
} rbnn_nn_train_net;

typedef struct rbnn_nn_train_ws {  /* caller-owned, for M members x up to B points                                  */
    float *hid1, *dact1, *dA1;     /* [M, B, H] layer-1 activations, act'(pre-activation), dL/d(pre-activation)   */
    float *hid2, *dact2, *dA2;     /* [M, B, H] fc2 only: the same for the second hidden layer                    */
    float *dZ;                     /* [M, B, 16] dL/dlogits = (softmax - e_y) / B                                  */
    float *ce;                     /* [M, B] cross-entropy per point                                               */
    int32_t *correct;              /* [M, B] 1 where the first maximum of the training forward's logits is the label */
} rbnn_nn_train_ws;

/* [host] n_params of one member (the least member_stride).  < 0: rbnn_status. */
int64_t rbnn_nn_train_sizes(const rbnn_nn_train_net *net);
/* The training forward of every member on its batch: hidden activations, act', logits, ce, dZ, correct, and the backward to dA1
 * (fc2: dA2, then dA1): fc 2 launches, fc2 4.  labels: int32 [n_rows] in [0, C), indexed like X. */
int rbnn_nn_train_forward(const rbnn_nn_train_net *net, const float *X, int32_t ldx, int32_t n_rows, const int32_t *labels, const int32_t *rows,
                          int32_t n_points, const rbnn_nn_train_ws *ws, void *stream);
/* grad = dL/dP of every tensor of every member (the biases as column sums): one launch, fp32 MFMA. */
int rbnn_nn_weight_grads(const rbnn_nn_train_net *net, const float *X, int32_t ldx, int32_t n_rows, const int32_t *rows, int32_t n_points,
                         const rbnn_nn_train_ws *ws, void *stream);
/* One torch.optim.Adam step (single-tensor formula, no weight decay) on P of every member; `step` = the step number t >= 1 of the bias
 * corrections.  The scalars are doubles and each derived one is rounded to fp32 once, as in the SVI update above. */
int rbnn_nn_adam_step(const rbnn_nn_train_net *net, int64_t step, double lr, double beta1, double beta2, double adam_eps, void *stream);
/* One block per member, fixed order, fp64: stats[m] = [the fp32-rounded mean of ce[m, :] (the step's loss), += it, += sum correct[m, :]]. */
int rbnn_nn_train_finalize(const rbnn_nn_train_net *net, const rbnn_nn_train_ws *ws, int32_t n_points, double *stats, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * HMC over the weights of an fc / fc2 net (csrc/rbnn_hmc.hip): pyro's HMC(model, step_size, num_steps) under MCMC as model_bnn.py:260-301
 * calls it.  Position q = the flat parameter buffer of the SVI trainer above; U(q) = sum_b CE(z_b(q), y_b) + 1/2 sum q^2, grad U = dCE/dW + q.
 * dCE/dW is rbnn_svi_train_forward + rbnn_svi_weight_grads on an rbnn_svi_train_net whose W is the trajectory's position and whose grad
 * receives dCE/dW (the other pointers of that struct are not read).  One transition, issued in this order on one stream:
 *   momentum -> leapfrog_update(OPEN) -> { train_forward -> weight_grads -> leapfrog_update(MID, or CLOSE after the last step) } x L
 *            -> decide -> commit        (a leapfrog step: fc 2 + 1 + 1 launches, fc2 4 + 1 + 1)
 * The chain's scalars live in a device-side block of RBNN_HMC_STATE doubles (indices RBNN_HMC_ST_*); every element-wise kernel reads the
 * step size from it.  Acceptance uniform of transition i: component 0 of the Philox4x32-10 block with counter (i, 0, 0, 0) under
 * key ^ RBNN_HMC_UNIF_KEY, times 2^-32.  Momentum: rbnn_svi_draw's counter layout at sample 0 with draw id = the caller's draw_id.
 * No atomics: two runs with the same key are bit-identical.  Every rbnn_hmc_* entry point checks the net as rbnn_svi_train_forward does
 * (RBNN_ERR_UNSUPPORTED for an arch or activation outside it).
 * ------------------------------------------------------------------------------------------------------------ */
#define RBNN_HMC_STATE 16
#define RBNN_HMC_LOG 8            /* doubles per log row: eps used, dH, accept_prob, accepted, u, U', K', K */
#define RBNN_HMC_UNIF_KEY 0xE7037ED1A0B428DBull
#define RBNN_HMC_SEARCH_KEY 0xA0761D6478BD642Full   /* xor-ed into the key by the CALLER for the step-size search's momenta */
enum { RBNN_HMC_ST_EPS = 0, RBNN_HMC_ST_U = 1, RBNN_HMC_ST_T = 2, RBNN_HMC_ST_GBAR = 3, RBNN_HMC_ST_XBAR = 4, RBNN_HMC_ST_MU = 5,
       RBNN_HMC_ST_DH = 6, RBNN_HMC_ST_ACC_PROB = 7, RBNN_HMC_ST_ACCEPTED = 8, RBNN_HMC_ST_UNIF = 9, RBNN_HMC_ST_U_NEW = 10,
       RBNN_HMC_ST_K_NEW = 11, RBNN_HMC_ST_K_OLD = 12 };
enum { RBNN_HMC_OPEN = 0, RBNN_HMC_MID = 1, RBNN_HMC_CLOSE = 2, RBNN_HMC_KICK = 3, RBNN_HMC_DRIFT = 4, RBNN_HMC_ENERGY = 5 };
enum { RBNN_HMC_DECIDE_INIT = 0, RBNN_HMC_DECIDE_PROBE = 1, RBNN_HMC_DECIDE_TRANSITION = 2 };

typedef struct rbnn_hmc_chain {
    float *q_cur, *g_cur;          /* [n_params] the chain's position and dCE/dW there (U is state[RBNN_HMC_ST_U])  */
    float *r;                      /* [n_params] momentum                                                          */
    float *m_inv;                  /* [n_params] diagonal inverse mass                                             */
    float *w_mean, *w_m2;          /* [n_params] Welford mean and M2 of the position (zero at a window's start)    */
    float *k0_part;                /* [n_quad_partials] partial sums of K at the trajectory's start               */
    float *k1_part, *p_part;       /* [n_elem_partials] partial sums of K' and of 1/2 sum q'^2                     */
    double *state;                 /* [RBNN_HMC_STATE]                                                             */
    double *log;                   /* [log_rows, RBNN_HMC_LOG], nullable                                           */
    float *samples;                /* [sample_rows, n_params], nullable                                            */
    int64_t log_rows, sample_rows;
} rbnn_hmc_chain;

/* [host] n_params; the lengths of k0_part and of k1_part / p_part (nullable).  < 0: rbnn_status. */
int64_t rbnn_hmc_sizes(const rbnn_svi_train_net *net, int64_t *n_quad_partials, int64_t *n_elem_partials);
/* r = eps_n(key, draw_id) * rsqrt(m_inv), k0_part: one launch. */
int rbnn_hmc_momentum(const rbnn_svi_train_net *net, const rbnn_hmc_chain *chain, uint64_t key, uint32_t draw_id, void *stream);
/* One element-wise launch on net->W / net->grad / chain->r with eps = state[RBNN_HMC_ST_EPS].  OPEN: r -= eps/2 (g_cur + q_cur),
 * W = q_cur + eps m_inv r.  MID: r -= eps/2 (grad + W) twice, W += eps m_inv r.  CLOSE: r -= eps/2 (grad + W), then k1_part / p_part.
 * KICK: CLOSE's half kick alone.  DRIFT: W += eps m_inv r.  ENERGY: k1_part / p_part of (W, r) as they stand. */
int rbnn_hmc_leapfrog_update(const rbnn_svi_train_net *net, const rbnn_hmc_chain *chain, int32_t phase, void *stream);
/* One block, fp64, fixed order: U' = sum ce + sum p_part, K' = sum k1_part, K = sum k0_part.  INIT: state U = U'.  PROBE: state dH only
 * (dH = (U' + K') - (U + K), NaN -> +inf).  TRANSITION: accept_prob = min(1, exp(-dH)), u, accepted = u < accept_prob (then U = U'), the
 * log row `transition`, and, if adapt, one dual-averaging update that writes the next step size (exp(x), at a window's end exp(xbar)). */
int rbnn_hmc_decide(const rbnn_svi_train_net *net, const rbnn_hmc_chain *chain, const float *ce, int32_t n_points, uint64_t key,
                    int64_t transition, int32_t mode, int32_t adapt, int32_t window_end, void *stream);
/* One launch: if accepted (or force) q_cur = W, g_cur = grad — a rejection writes neither; welford_n > 0: the Welford update number
 * welford_n of the window with the position after the decision; sample_row >= 0: that row of samples = the position after the decision. */
int rbnn_hmc_commit(const rbnn_svi_train_net *net, const rbnn_hmc_chain *chain, int32_t force, int32_t welford_n, int64_t sample_row,
                    void *stream);
/* One launch: m_inv = (n / (n + 5)) M2 / (n - 1) + 1e-3 * 5 / (n + 5) for a window of n_window >= 2 positions, then mean = M2 = 0. */
int rbnn_hmc_window_end(const rbnn_svi_train_net *net, const rbnn_hmc_chain *chain, int32_t n_window, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * K independent HMC chains over nets of ONE shape in LOCKSTEP (csrc/rbnn_hmc.hip; additive, ABI 10): every launch covers all K chains, the
 * chain is grid dimension y, as the member is in the deterministic trainer above.  The net is an rbnn_nn_train_net: P = the trajectory
 * positions [K, member_stride], grad = dCE/dW [K, member_stride], n_members = K, member_stride = chain_stride (m and v are not read).
 * Every per-parameter buffer of the chain block is [K, chain_stride], the partial sums [K, qpart_stride] / [K, epart_stride] (at least the
 * lengths the sizes query above reports), state [K, RBNN_HMC_STATE], log [K, log_rows, RBNN_HMC_LOG], samples [K, sample_rows, n_params].
 * Per chain: its key (keys[k]), its step size (its state block), its number of leapfrog steps (steps[k]), whether a launch touches it at all
 * (active[k]) and its own number of points (counts[k] <= n_points; the points behind it contribute exact zeros).  No sum crosses chains, no
 * atomics, a chain's block and tile plan does not depend on K: chain k is bit-identical to the single-chain entry points running it alone.
 * One transition on one stream:  momentum -> update(OPEN) -> { gradient -> update(step s) } x max_k steps[k] -> decide -> commit.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct rbnn_hmc_lockstep {
    float *q_cur, *g_cur, *r, *m_inv, *w_mean, *w_m2;      /* [K, chain_stride], each as in rbnn_hmc_chain; rbnn_conv_hmc_chains_*: tensor-major, chain_stride == n_params */
    float *k0_part;                /* [K, qpart_stride]                                                            */
    float *k1_part, *p_part;       /* [K, epart_stride]                                                            */
    double *state;                 /* [K, RBNN_HMC_STATE]                                                          */
    double *log;                   /* [K, log_rows, RBNN_HMC_LOG], nullable                                        */
    float *samples;                /* [K, sample_rows, n_params], nullable                                         */
    const uint64_t *keys;          /* [K] on the device: chain k's key                                             */
    const int32_t *active;         /* [K] on the device, nullable (all active): 0 = this launch neither reads nor writes chain k */
    const int32_t *steps;          /* [K] on the device, nullable: chain k's leapfrog steps of this trajectory (update with step >= 0) */
    int64_t chain_stride, qpart_stride, epart_stride, log_rows, sample_rows;
} rbnn_hmc_lockstep;

/* dCE/dW (summed CE) and ce [K, n_points] of every chain at net->P: the lockstep training forward (fc 2 launches, fc2 4) + the weight
 * gradients (1).  Chain k's batch is rows[k, 0..n_points) of the resident X [n_rows, ldx] (indices clamped into [0, n_rows); rows == NULL:
 * rows 0..n_points-1 for every chain); labels int32 [n_rows].  counts (nullable) [K]: for b >= counts[k] ce, dZ, dA and correct are 0.
 * ws is packed [K, n_points, .].  active is NOT consulted: an inactive chain's trajectory buffers are scratch. */
int rbnn_hmc_lockstep_gradient(const rbnn_nn_train_net *net, const float *X, int32_t ldx, int32_t n_rows, const int32_t *labels,
                               const int32_t *rows, const int32_t *counts, int32_t n_points, const rbnn_nn_train_ws *ws, void *stream);
/* The momentum draw of every active chain under keys[k] ^ key_xor with draw id draw_ids[k] (device, nullable: draw_id for every chain). */
int rbnn_hmc_lockstep_momentum(const rbnn_nn_train_net *net, const rbnn_hmc_lockstep *chains, uint64_t key_xor, uint32_t draw_id,
                               const uint32_t *draw_ids, void *stream);
/* step < 0: the single chain's update `phase` on every active chain.  step >= 0 (needs steps): leapfrog step `step` of trajectories of
 * different lengths: MID for chains with step + 1 < steps[k], CLOSE at step + 1 == steps[k], nothing for step >= steps[k]. */
int rbnn_hmc_lockstep_update(const rbnn_nn_train_net *net, const rbnn_hmc_lockstep *chains, int32_t phase, int32_t step, void *stream);
/* The single chain's decision, one block per active chain: ce [K, n_points], summed over the chain's first counts[k] (nullable: n_points)
 * entries; the uniform under keys[k]. */
int rbnn_hmc_lockstep_decide(const rbnn_nn_train_net *net, const rbnn_hmc_lockstep *chains, const float *ce, const int32_t *counts,
                             int32_t n_points, int64_t transition, int32_t mode, int32_t adapt, int32_t window_end, void *stream);
/* The single chain's commit on every active chain, each by its own decision; sample_row >= 0: that row of every chain's stack. */
int rbnn_hmc_lockstep_commit(const rbnn_nn_train_net *net, const rbnn_hmc_lockstep *chains, int32_t force, int32_t welford_n,
                             int64_t sample_row, void *stream);
/* The single chain's window end on every active chain. */
int rbnn_hmc_lockstep_window_end(const rbnn_nn_train_net *net, const rbnn_hmc_lockstep *chains, int32_t n_window, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * K SVI guides of ONE net shape trained in LOCKSTEP (csrc/rbnn_svi_lockstep.hip; additive, ABI 10): the SVI step above for every guide in
 * one set of launches, the guide is grid dimension y.  The net is an rbnn_nn_train_net: P = the drawn weights W [K, member_stride], grad =
 * dCE/dW [K, member_stride], n_members = K <= 65535 / RBNN_SVI_MULTI_ACC_SAMPLES (m and v are not read).  Every per-parameter buffer of the
 * guide block is [K, member_stride] in the layout of rbnn_svi_train_net.  Guide k's batch is rows[k, 0..counts[k]) of the resident data
 * X [n_rows, ldx] (indices clamped into [0, n_rows)); the entries of rows behind counts[k] must still be valid rows (their activations are
 * computed and multiplied by exact zeros).  counts[k] == 0: the guide has finished, every kernel skips it and nothing of its state is written.
 * One step on one stream:  draw -> gradient -> adam_step -> [accuracy] -> finalize.  No atomics, no sum across guides, a guide's block and
 * tile plan does not depend on K: guide k is bit-identical to the single-guide entry points running it alone on the same batches.
 * ------------------------------------------------------------------------------------------------------------ */
#define RBNN_SVI_MULTI_ACC_SAMPLES 10

typedef struct rbnn_svi_multi {
    float *loc, *raw, *sigma, *m_loc, *v_loc, *m_raw, *v_raw;      /* [K, member_stride], each as in rbnn_svi_train_net     */
    float *kl_part;                /* [K, part_stride] KL partial sums of the update (part_stride >= n_partials of rbnn_svi_train_sizes) */
    double *stats;                 /* [K, 3] step loss, running sum of the epoch's losses, running correct predictions */
    const uint64_t *keys;          /* [K] on the device: guide k's key                                              */
    int64_t part_stride;
} rbnn_svi_multi;

typedef struct rbnn_svi_multi_acc {     /* caller-owned buffers of the accuracy forward, S = RBNN_SVI_MULTI_ACC_SAMPLES         */
    float *W;                      /* [K * S, member_stride] the drawn weight sets, guide-major                     */
    float *hid1, *hid2;            /* [K * S, B, H] hidden activations (hid2: fc2 only)                             */
    float *dact;                   /* [K * S, B, H] scratch                                                         */
    float *Psum;                   /* [K, B, 16] sum over the S samples of the softmax probabilities                */
} rbnn_svi_multi_acc;

/* net->P[k] = loc[k] + sigma[k] * eps(keys[k], draw_id): exactly what rbnn_svi_train_draw writes for (keys[k], draw_id).  One launch. */
int rbnn_svi_multi_draw(const rbnn_nn_train_net *net, const rbnn_svi_multi *guides, const int32_t *counts, uint32_t draw_id,
                           void *stream);
/* The training forward (summed CE: no 1 / B) and the weight gradients of every guide at net->P: fc 2 + 1 launches, fc2 4 + 1.  ws is packed
 * [K, n_points, .]; for b >= counts[k] ce, dZ, dA and correct are 0.  rows and counts are required. */
int rbnn_svi_multi_gradient(const rbnn_nn_train_net *net, const float *X, int32_t ldx, int32_t n_rows, const int32_t *labels,
                               const int32_t *rows, const int32_t *counts, int32_t n_points, const rbnn_nn_train_ws *ws, void *stream);
/* rbnn_svi_adam_step on every guide, each with its own key and its own learning rate lr[k] (device, double [K]): step_size[k] =
 * (float)(lr[k] / (1 - beta1^step)), an IEEE double division of the host's 1 - beta1^step, so bit for bit the single guide's.  One launch. */
int rbnn_svi_multi_adam_step(const rbnn_nn_train_net *net, const rbnn_svi_multi *guides, const int32_t *counts, uint32_t draw_id,
                                int64_t step, const double *lr, double beta1, double beta2, double adam_eps, void *stream);
/* The accuracy forward of every guide on its own batch: S weight sets from the live loc / sigma with rbnn_svi_draw's generator at
 * (keys[k] ^ key_xor, draw_id, sample s) into acc->W, the hidden layers of the K * S nets, and Psum[k, b, :] = sum_s softmax(z_s).
 * fc 3 launches, fc2 4, whatever K. */
int rbnn_svi_multi_accuracy(const rbnn_nn_train_net *net, const rbnn_svi_multi *guides, const float *X, int32_t ldx, int32_t n_rows,
                               const int32_t *rows, const int32_t *counts, int32_t n_points, uint64_t key_xor, uint32_t draw_id,
                               const rbnn_svi_multi_acc *acc, void *stream);
/* One block per guide, fixed order, fp64: rbnn_svi_train_finalize's sums over the guide's counts[k] points of ce [K, n_points] and Psum
 * [K, n_points, 16] (nullable) into stats[k].  epoch_slot (device int32 [K], nullable): a guide with epoch_slot[k] in [0, log_rows) ends an
 * epoch with this step: epoch_log[k, slot] = (sum of the epoch's step losses, correct predictions) and both running sums restart at 0. */
int rbnn_svi_multi_finalize(const rbnn_nn_train_net *net, const rbnn_svi_multi *guides, const float *ce, const float *Psum,
                               const int32_t *labels, int32_t n_rows, const int32_t *rows, const int32_t *counts, int32_t n_points,
                               const int32_t *epoch_slot, double *epoch_log, int32_t log_rows, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Deterministic training of ONE conv net of the 1x28x28 geometry (csrc/rbnn_conv_train.hip): torch.optim.Adam on nn.CrossEntropyLoss()
 * (model_nn.py:175-219) for Conv2d(1,32,5) -> act -> MaxPool2d(2) -> Conv2d(32,Hc,5) -> act -> MaxPool2d(2, stride 1) -> Flatten ->
 * Linear(49 Hc, C), all four activations.  Issued in this order on one stream:  train_forward -> weight_grads -> adam_step -> train_finalize.
 * Parameters, Adam moments and gradients are flat buffers in state_dict order (model.0.weight, model.0.bias, model.3.weight, model.3.bias,
 * model.7.weight, model.7.bias), unpadded, row-major in nn.Conv2d's / nn.Linear's element order: the tensors start at floats 0, 800, 832,
 * 832 + 800 Hc, 832 + 801 Hc, 832 + 801 Hc + 49 Hc C.  The batch is a staged matrix X [B, ldx] (16-byte aligned, ldx >= 784 and a multiple
 * of 4) with int32 labels [B].  The forward is the exact fp32-MFMA conv forward above with one sample and logits out; the backward reads
 * the stashes it leaves.  No atomics and no device->host synchronisation: every sum has one fixed order, two runs are bit-identical.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct rbnn_conv_train_net {
    int32_t activation;            /* rbnn_activation                                                              */
    int32_t in_channels, in_width; /* 1, 28 (anything else: RBNN_ERR_UNSUPPORTED)                                  */
    int32_t hidden;                /* Hc = conv2 output channels, a multiple of 16                                 */
    int32_t n_classes;             /* C in [1, 16]                                                                 */
    int32_t reserved;
    float *P;                      /* [n_params] parameters (16-byte aligned)                                      */
    float *m, *v;                  /* [n_params] Adam moments (zero before the first step)                         */
    float *grad;                   /* [n_params] dL/dP of the step (L = mean CE of the batch)                      */
} rbnn_conv_train_net;

typedef struct rbnn_conv_train_ws {   /* caller-owned, for up to B points; every buffer 16-byte aligned             */
    float   *logits;               /* [B, 16]                                                                      */
    float   *P1;                   /* [B, 32, 12, 12] pooled + activated conv1 output (allocated 24 KiB per point) */
    uint8_t *st1;                  /* [B, 32 * 144] pool-1 stash (the encoding of rbnn_conv_workspace)             */
    float   *Q2;                   /* [B, 49 Hc] pooled + activated conv2 output                                   */
    uint8_t *st2;                  /* [B, 49 Hc] pool-2 stash                                                      */
    float   *dZ;                   /* [B, 16] dL/dlogits = (softmax - e_y) / B                                     */
    float   *ce;                   /* [B] cross-entropy per point                                                  */
    int32_t *correct;              /* [B] 1 where the first maximum of the logits is the label                     */
    float   *dO2;                  /* [B, Hc, 8, 8] dL/d(conv2 pre-activation)                                     */
    float   *dO1;                  /* [B, 32, 24, 24] dL/d(conv1 pre-activation)                                   */
    float   *part2;                /* [splits2, Hc, 801] partial sums of dK2 | dK2b over slices of the batch       */
    float   *part1;                /* [splits1, 32, 26] partial sums of dK1 | dK1b                                 */
    float   *partP;                /* [splitsP, B, 144, 32] partial sums of dL/d(pooled conv1 output) over slices of the conv2 channels */
} rbnn_conv_train_ws;

typedef struct rbnn_conv_train_bytes {   /* n_params and the bytes of every rbnn_conv_train_ws buffer for B points */
    int64_t n_params;
    size_t logits, P1, st1, Q2, st2, dZ, ce, correct, dO2, dO1, part2, part1, partP;
} rbnn_conv_train_bytes;

/* [host] n_params and the workspace sizes for n_points points. */
int rbnn_conv_train_sizes(const rbnn_conv_train_net *net, int32_t n_points, rbnn_conv_train_bytes *out);
/* The training forward (conv1 + pool, conv2 + pool, Linear: 3 launches) and the head (1 launch): logits, ce, dZ, correct.  labels: int32
 * [n_points] in [0, C). */
int rbnn_conv_train_forward(const rbnn_conv_train_net *net, const float *X, int32_t ldx, const int32_t *labels, int32_t n_points,
                            const rbnn_conv_train_ws *ws, void *stream);
/* grad = dL/dP of all six tensors (fp32 MFMA; every conv contraction is split across blocks and the partial sums added in a second,
 * fixed-order pass): 7 launches. */
int rbnn_conv_weight_grads(const rbnn_conv_train_net *net, const float *X, int32_t ldx, int32_t n_points, const rbnn_conv_train_ws *ws,
                           void *stream);
/* One torch.optim.Adam step (single-tensor formula, no weight decay) on P; `step` = the step number t >= 1 of the bias corrections; the
 * formula and roundings of rbnn_nn_adam_step. */
int rbnn_conv_adam_step(const rbnn_conv_train_net *net, int64_t step, double lr, double beta1, double beta2, double adam_eps, void *stream);
/* One block, fixed order, fp64: stats = [the fp32-rounded mean of ce (the step's loss), += it, += sum correct]. */
int rbnn_conv_train_finalize(const rbnn_conv_train_ws *ws, int32_t n_points, double *stats, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * SVI training of ONE conv guide of the 1x28x28 geometry (csrc/rbnn_conv_train.hip; additive, ABI 10): the SVI step of rbnn_svi_train_net
 * above (model_bnn.py:303-365: one weight sample, L = sum_b CE(z_b, y_b) + sum KL(N(loc, sigma) || N(0, 1)), one torch.optim.Adam step on
 * every loc and raw scale) around the conv training forward and the conv weight gradients.  Issued in this order on one stream:
 *   conv_svi_train_draw -> conv_svi_train_forward -> conv_svi_weight_grads -> conv_svi_adam_step -> [accuracy forward] -> rbnn_svi_train_finalize.
 * The nine buffers are flat [n_params] in rbnn_conv_train_net's layout: model.0.weight, model.0.bias, model.3.weight, model.3.bias,
 * model.7.weight, model.7.bias.  eps is rbnn_svi_draw_flat's generator at sample 0: element e of tensor i (tensor ids 0..5 in that order)
 * is component e % 4 of the Philox block with counter (e / 4, i, 0, draw_id), so W equals sample 0 of a stack redrawn by
 * rbnn_svi_draw_flat with the same (key, draw_id) bit for bit, and the update regenerates eps instead of storing it.  The workspace is
 * rbnn_conv_train_ws: correct is written by the head and not read by the step, dZ = softmax - e_y (the SUMMED cross-entropy).  No atomics,
 * no device->host synchronisation: two runs are bit-identical.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct rbnn_conv_svi_train_net {
    int32_t activation;            /* rbnn_activation                                                              */
    int32_t in_channels, in_width; /* 1, 28 (anything else: RBNN_ERR_UNSUPPORTED)                                  */
    int32_t hidden;                /* Hc = conv2 output channels, a multiple of 16 in [16, 4096]                   */
    int32_t n_classes;             /* C in [1, 16]                                                                 */
    int32_t reserved;
    float *loc, *raw, *sigma;      /* [n_params] variational mean, raw scale, sigma = softplus(raw) (written by the update); 16-byte aligned */
    float *m_loc, *v_loc, *m_raw, *v_raw;      /* [n_params] Adam moments (zero before the first step)             */
    float *W;                      /* [n_params] the drawn weight sample (16-byte aligned)                         */
    float *grad;                   /* [n_params] dCE/dW of the step                                                */
} rbnn_conv_svi_train_net;

/* [host] out->n_params and the bytes of every rbnn_conv_train_ws buffer for n_points points (what rbnn_conv_train_sizes reports);
 * *n_partials (nullable) = the KL partial sums rbnn_conv_svi_adam_step writes. */
int rbnn_conv_svi_train_sizes(const rbnn_conv_svi_train_net *net, int32_t n_points, int64_t *n_partials, rbnn_conv_train_bytes *out);
/* W = loc + sigma * eps(key, draw_id) for the six tensors: one launch (rbnn_svi_draw_flat on views of the flat buffers). */
int rbnn_conv_svi_train_draw(const rbnn_conv_svi_train_net *net, uint64_t key, uint32_t draw_id, void *stream);
/* rbnn_conv_train_forward on W with the summed cross-entropy: logits, ce[b], dZ = softmax(z) - e_y (no 1 / B), correct.  3 + 1 launches. */
int rbnn_conv_svi_train_forward(const rbnn_conv_svi_train_net *net, const float *X, int32_t ldx, const int32_t *labels, int32_t n_points,
                                const rbnn_conv_train_ws *ws, void *stream);
/* rbnn_conv_weight_grads reading W and writing grad = dCE/dW of all six tensors: 7 launches. */
int rbnn_conv_svi_weight_grads(const rbnn_conv_svi_train_net *net, const float *X, int32_t ldx, int32_t n_points, const rbnn_conv_train_ws *ws,
                               void *stream);
/* rbnn_svi_adam_step on the six conv tensors (each one row of n_elem columns: the regenerated eps quad is e / 4, the draw's own counter):
 * loc, raw, sigma, the four moment buffers, and kl_partials[i] = the KL of the PRE-update parameters summed over block i.  One launch. */
int rbnn_conv_svi_adam_step(const rbnn_conv_svi_train_net *net, uint64_t key, uint32_t draw_id, int64_t step, double lr, double beta1,
                            double beta2, double adam_eps, float *kl_partials, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * HMC over the weights of ONE conv net of the 1x28x28 geometry (csrc/rbnn_hmc.hip; additive, ABI 10): the six single-chain entry points
 * rbnn_hmc_* above with an rbnn_conv_svi_train_net in place of the rbnn_svi_train_net, on the same rbnn_hmc_chain and with their semantics
 * word for word: U(q) = sum_b CE(z_b(q), y_b) + 1/2 sum q^2, grad U = dCE/dW + q; the phases OPEN / MID / CLOSE / KICK / DRIFT / ENERGY; the
 * decide modes INIT / PROBE / TRANSITION; the state block's RBNN_HMC_ST_* indices; RBNN_HMC_UNIF_KEY and RBNN_HMC_SEARCH_KEY.  Position q =
 * the flat parameter buffer of rbnn_conv_train_net's layout.  Of the net, W is the trajectory's position and grad receives dCE/dW =
 * rbnn_conv_svi_train_forward + rbnn_conv_svi_weight_grads at W (the summed cross-entropy); the other pointers are not read.  One transition,
 * issued in this order on one stream:
 *   momentum -> leapfrog_update(OPEN) -> { conv_svi_train_forward -> conv_svi_weight_grads -> leapfrog_update(MID, or CLOSE after the last
 *   step) } x L -> decide -> commit        (a leapfrog step: 4 + 7 + 1 = 12 launches; a transition with L steps: 1 + 1 + 12 L + 1 + 1)
 * Momentum: libm normals (logf / sincospif, as rbnn_hmc_momentum), element e of tensor i (tensor ids 0..5 in state_dict order) from component
 * e % 4 of the Philox block with counter (e / 4, i, 0, draw_id) — rbnn_conv_svi_train_draw's counter layout.  The kernels are the single
 * chain's own: no atomics, one stream, no device->host synchronisation, two runs with the same key are bit-identical.  Every entry point
 * checks the net before any HIP call, as the conv SVI entry points do: a geometry other than 1 / 28 or an activation outside the four is
 * RBNN_ERR_UNSUPPORTED, hidden not a multiple of 16 in [16, 4096] or n_classes outside [1, 16] RBNN_ERR_SHAPE, a null pointer RBNN_ERR_NULL,
 * a phase or mode out of range RBNN_ERR_UNSUPPORTED.  Several chains of one net shape: rbnn_conv_hmc_chains_* at the end of this header.
 * ------------------------------------------------------------------------------------------------------------ */
/* [host] n_params; the lengths of k0_part and of k1_part / p_part (nullable).  < 0: rbnn_status. */
int64_t rbnn_conv_hmc_sizes(const rbnn_conv_svi_train_net *net, int64_t *n_quad_partials, int64_t *n_elem_partials);
/* rbnn_hmc_momentum on the six conv tensors: one launch. */
int rbnn_conv_hmc_momentum(const rbnn_conv_svi_train_net *net, const rbnn_hmc_chain *chain, uint64_t key, uint32_t draw_id, void *stream);
/* rbnn_hmc_leapfrog_update on net->W / net->grad / chain->r: one launch. */
int rbnn_conv_hmc_leapfrog_update(const rbnn_conv_svi_train_net *net, const rbnn_hmc_chain *chain, int32_t phase, void *stream);
/* rbnn_hmc_decide; ce = the conv workspace's per-point cross-entropy of the trajectory's end: one launch, one block. */
int rbnn_conv_hmc_decide(const rbnn_conv_svi_train_net *net, const rbnn_hmc_chain *chain, const float *ce, int32_t n_points, uint64_t key,
                         int64_t transition, int32_t mode, int32_t adapt, int32_t window_end, void *stream);
/* rbnn_hmc_commit: one launch. */
int rbnn_conv_hmc_commit(const rbnn_conv_svi_train_net *net, const rbnn_hmc_chain *chain, int32_t force, int32_t welford_n, int64_t sample_row,
                         void *stream);
/* rbnn_hmc_window_end: one launch. */
int rbnn_conv_hmc_window_end(const rbnn_conv_svi_train_net *net, const rbnn_hmc_chain *chain, int32_t n_window, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Deterministic training of M conv nets of one shape in LOCKSTEP (csrc/rbnn_conv_train.hip; additive, ABI 10): the step of
 * rbnn_conv_train_net above for the members of a deep ensemble (model_ensemble.py:69-83), the member a grid dimension of every launch.
 * Issued in this order on one stream:  conv_ens_stage -> conv_ens_forward -> conv_ens_weight_grads -> conv_ens_adam_step -> conv_ens_finalize:
 * 1 + 4 + 7 + 1 + 1 = 14 launches whatever M is.  Member m computes what rbnn_conv_train_* compute for that net on rows[m] of the data, bit
 * for bit.  The four flat buffers are TENSOR-MAJOR: six blocks [M, size of tensor t] in state_dict order (model.0.weight [M, 800],
 * model.0.bias [M, 32], model.3.weight [M, 800 Hc], model.3.bias [M, Hc], model.7.weight [M, 49 Hc C], model.7.bias [M, C]), block t at M
 * times the single net's offset — the stacks of rbnn_conv_posterior.  The batches are gathered from resident data X [n_rows, ldx] (16-byte
 * aligned, ldx >= 784 and a multiple of 4) with int32 labels [n_rows] by int32 rows [M, B]; an index outside [0, n_rows) is clamped.  The
 * workspaces are packed [M, B, .] for the call's B.  No atomics and no device->host synchronisation: two runs are bit-identical.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct rbnn_conv_ens_net {
    int32_t activation;            /* rbnn_activation                                                              */
    int32_t in_channels, in_width; /* 1, 28 (anything else: RBNN_ERR_UNSUPPORTED)                                  */
    int32_t hidden;                /* Hc = conv2 output channels, a multiple of 16 in [16, 4096]                   */
    int32_t n_classes;             /* C in [1, 16]                                                                 */
    int32_t n_members;             /* M in [1, 65535], M B <= 2^22                                                 */
    float *P;                      /* [M n_params] parameters, tensor-major (16-byte aligned)                      */
    float *m, *v;                  /* [M n_params] Adam moments (zero before the first step)                       */
    float *grad;                   /* [M n_params] dL/dP of the step (L = every member's mean CE of its batch)     */
} rbnn_conv_ens_net;

typedef struct rbnn_conv_ens_ws {     /* caller-owned, for up to B points per member; every buffer 16-byte aligned  */
    float   *Xs;                   /* [M B, 784] the members' gathered batches                                     */
    int32_t *labels;               /* [M B] their labels                                                           */
    float   *logits;               /* the buffers of rbnn_conv_train_ws, each with a leading member dimension      */
    float   *P1;
    uint8_t *st1;
    float   *Q2;
    uint8_t *st2;
    float   *dZ;                   /* [M, B, 16] (softmax - e_y) / B                                               */
    float   *ce;                   /* [M, B]                                                                       */
    int32_t *correct;              /* [M, B]                                                                       */
    float   *dO2;
    float   *dO1;
    float   *part2;                /* [M, splits2, Hc, 801]; the slice counts are those of the single net           */
    float   *part1;                /* [M, splits1, 32, 26]                                                         */
    float   *partP;                /* [M, splitsP, B, 144, 32]                                                     */
} rbnn_conv_ens_ws;

typedef struct rbnn_conv_ens_bytes {  /* n_params of ONE member and the bytes of every rbnn_conv_ens_ws buffer for B points per member */
    int64_t n_params;
    size_t Xs, labels, logits, P1, st1, Q2, st2, dZ, ce, correct, dO2, dO1, part2, part1, partP;
} rbnn_conv_ens_bytes;

/* [host] n_params of one member (rbnn_conv_train_sizes') and the workspace sizes: M times the single net's, Xs and labels beside them. */
int rbnn_conv_ens_sizes(const rbnn_conv_ens_net *net, int32_t n_points, rbnn_conv_ens_bytes *out);
/* Xs[m, b] = X[rows[m, b]], labels[m, b] = labels[rows[m, b]] (indices clamped to [0, n_rows)): 1 launch.  No later call sees rows. */
int rbnn_conv_ens_stage(const rbnn_conv_ens_net *net, const float *X, int32_t ldx, int32_t n_rows, const int32_t *labels, const int32_t *rows,
                        int32_t n_points, const rbnn_conv_ens_ws *ws, void *stream);
/* rbnn_conv_train_forward of every member on its staged batch: 3 + 1 launches. */
int rbnn_conv_ens_forward(const rbnn_conv_ens_net *net, int32_t n_points, const rbnn_conv_ens_ws *ws, void *stream);
/* rbnn_conv_weight_grads of every member: 7 launches. */
int rbnn_conv_ens_weight_grads(const rbnn_conv_ens_net *net, int32_t n_points, const rbnn_conv_ens_ws *ws, void *stream);
/* rbnn_conv_adam_step on all M n_params elements (the members share step and lr): 1 launch. */
int rbnn_conv_ens_adam_step(const rbnn_conv_ens_net *net, int64_t step, double lr, double beta1, double beta2, double adam_eps, void *stream);
/* One block per member: stats [M, 3] = rbnn_conv_train_finalize's three figures of every member. */
int rbnn_conv_ens_finalize(const rbnn_conv_ens_net *net, const rbnn_conv_ens_ws *ws, int32_t n_points, double *stats, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * K SVI guides of ONE conv net shape (1x28x28) trained in LOCKSTEP (csrc/rbnn_conv_train.hip; the Adam + KL step: csrc/rbnn_svi.hip; additive, ABI 10): the step of
 * rbnn_conv_svi_train_net above for every guide in one set of launches whose count does not depend on K, the guide a grid dimension of each.
 * Issued in this order on one stream:  conv_svi_guides_draw -> conv_svi_guides_gradient -> conv_svi_guides_adam_step -> [conv_svi_guides_accuracy]
 * -> conv_svi_guides_finalize: 1 + (1 + 4 + 7) + 1 + [1 + 3 + 1] + 1 = 15 launches without the accuracy forward, 20 with it.  The nine flat
 * buffers are TENSOR-MAJOR as rbnn_conv_ens_net's: six blocks [K, size of tensor t] in state_dict order, block t at K times the single
 * guide's offset — the stacks of rbnn_conv_posterior, so the exact conv forward addresses guide k as sample k.  All guides of a step share its
 * point count B: guide k's batch is rows[k, 0..B) of the resident data (indices clamped into [0, n_rows)), and the slice plans of the three
 * conv GEMMs are the single guide's for B.  Guide k computes what the rbnn_conv_svi_train_* entry points, ConvStackedPosterior's redraw under
 * keys[k] ^ key_xor, rbnn_conv_forward, rbnn_reduce_samples and rbnn_svi_train_finalize compute for that guide alone on those rows, bit for bit.
 * active (device int32 [K]): a guide with active[k] == 0 has finished its epochs; the kernels that write its state (draw, Adam + KL, the
 * accuracy draw and sum, finalize) return at once for it, so its loc, raw, sigma, moments, kl_part, stats, epoch_log rows, W and accuracy
 * weight sets are never written again (its batch is still staged and the workspaces, packed by the call's B, are written: they hold nothing
 * that outlives a step).
 * No atomics, no sum across guides, no device->host synchronisation; a guide's blocks and tiles do not depend on K.
 * Every entry point checks, before any launch: net NULL, then the descriptor (geometry / activation: RBNN_ERR_UNSUPPORTED; hidden, n_classes,
 * n_guides outside [1, 65535 / RBNN_SVI_MULTI_ACC_SAMPLES]: RBNN_ERR_SHAPE), then NULL pointers, then shapes (n_points, K n_points <= 2^22,
 * ldx, n_rows, part_stride, step), then 16-byte alignment.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct rbnn_conv_svi_guides_net {
    int32_t activation;            /* rbnn_activation                                                              */
    int32_t in_channels, in_width; /* 1, 28 (anything else: RBNN_ERR_UNSUPPORTED)                                  */
    int32_t hidden;                /* Hc = conv2 output channels, a multiple of 16 in [16, 4096]                   */
    int32_t n_classes;             /* C in [1, 16]                                                                 */
    int32_t n_guides;              /* K in [1, 6553], K B <= 2^22                                                  */
    float *loc, *raw, *sigma;      /* [K n_params] tensor-major: mean, raw scale, sigma = softplus(raw); 16-byte aligned */
    float *m_loc, *v_loc, *m_raw, *v_raw;      /* [K n_params] Adam moments (zero before the first step)           */
    float *W;                      /* [K n_params] the drawn weight samples (16-byte aligned)                      */
    float *grad;                   /* [K n_params] dCE/dW of the step                                              */
    float *kl_part;                /* [K, part_stride] KL partial sums of the update                               */
    double *stats;                 /* [K, 3] step loss, running sum of the epoch's losses, running correct predictions */
    const uint64_t *keys;          /* [K] on the device: guide k's key                                             */
    int64_t part_stride;           /* >= n_partials of rbnn_conv_svi_guides_sizes                                   */
} rbnn_conv_svi_guides_net;

typedef struct rbnn_conv_svi_guides_ws {  /* caller-owned, for up to B points per guide; every buffer 16-byte aligned */
    float   *Xs;                   /* the buffers of rbnn_conv_ens_ws, the guide in the member's place              */
    int32_t *labels;
    float   *logits;
    float   *P1;
    uint8_t *st1;
    float   *Q2;
    uint8_t *st2;
    float   *dZ;                   /* [K, B, 16] softmax - e_y (the SUMMED cross-entropy)                          */
    float   *ce;                   /* [K, B]                                                                       */
    int32_t *correct;              /* [K, B] written by the head, not read by the step                             */
    float   *dO2;
    float   *dO1;
    float   *part2;
    float   *part1;
    float   *partP;
    float   *acc_W;                /* [K S n_params] the accuracy forward's weight sets, S = RBNN_SVI_MULTI_ACC_SAMPLES: tensor-major over K S sets, set k S + s */
    float   *acc_P;                /* [K S, B, 16] their softmax probabilities                                     */
    float   *acc_P1;               /* [K S, B, .] the buffers of rbnn_conv_workspace for K S samples of B points   */
    uint8_t *acc_st1;
    float   *acc_Q2;
    uint8_t *acc_st2;
    float   *Psum;                 /* [K, B, 16] sum over the S samples of the probabilities, s = 0, 1, ... in that order */
} rbnn_conv_svi_guides_ws;

typedef struct rbnn_conv_svi_guides_bytes {  /* of ONE guide: n_params, n_partials; the bytes of every rbnn_conv_svi_guides_ws buffer for B points per guide */
    int64_t n_params, n_partials;
    size_t Xs, labels, logits, P1, st1, Q2, st2, dZ, ce, correct, dO2, dO1, part2, part1, partP, acc_W, acc_P, acc_P1, acc_st1, acc_Q2, acc_st2, Psum;
} rbnn_conv_svi_guides_bytes;

/* [host] n_params and n_partials of one guide (rbnn_conv_svi_train_sizes'), and the workspace sizes: K times the single guide's, Xs and
 * labels beside them as in rbnn_conv_ens_sizes, and the accuracy forward's (K S samples of B points: the large term).  Linear in K. */
int rbnn_conv_svi_guides_sizes(const rbnn_conv_svi_guides_net *net, int32_t n_points, rbnn_conv_svi_guides_bytes *out);
/* W[k] = loc[k] + sigma[k] * eps(keys[k], draw_id) for the six tensors of every active guide: exactly what rbnn_conv_svi_train_draw writes
 * for (keys[k], draw_id).  One launch. */
int rbnn_conv_svi_guides_draw(const rbnn_conv_svi_guides_net *net, const int32_t *active, uint32_t draw_id, void *stream);
/* rbnn_conv_ens_stage of rows [K, n_points], the exact forward with the guide as sample and the head of the SUMMED cross-entropy (dZ =
 * softmax - e_y), the seven weight-gradient launches of rbnn_conv_ens_weight_grads reading W and writing grad: 1 + 4 + 7 launches. */
int rbnn_conv_svi_guides_gradient(const rbnn_conv_svi_guides_net *net, const float *X, int32_t ldx, int32_t n_rows, const int32_t *labels,
                                 const int32_t *rows, int32_t n_points, const rbnn_conv_svi_guides_ws *ws, void *stream);
/* rbnn_conv_svi_adam_step on every active guide, each with its own key and learning rate lr[k] (device, double [K]): step_size[k] =
 * (float)(lr[k] / (1 - beta1^step)), an IEEE double division of the host's 1 - beta1^step, so bit for bit the single guide's.  One launch. */
int rbnn_conv_svi_guides_adam_step(const rbnn_conv_svi_guides_net *net, const int32_t *active, uint32_t draw_id, int64_t step,
                                  const double *lr, double beta1, double beta2, double adam_eps, void *stream);
/* The accuracy forward of every active guide on the batch rbnn_conv_svi_guides_gradient staged: S weight sets per guide from the live loc /
 * sigma with rbnn_svi_draw_flat's generator at (keys[k] ^ key_xor, draw_id, sample s) into acc_W, the exact conv forward of the K S nets
 * (set k S + s reads guide k's n_points rows), Psum[k, b, :] = sum_s softmax(z_s).  1 + 3 + 1 launches. */
int rbnn_conv_svi_guides_accuracy(const rbnn_conv_svi_guides_net *net, const int32_t *active, int32_t n_points, uint64_t key_xor,
                                 uint32_t draw_id, const rbnn_conv_svi_guides_ws *ws, void *stream);
/* One block per active guide, fixed order, fp64: rbnn_svi_train_finalize's sums over the guide's n_points points of ws->ce and (with_accuracy
 * != 0) ws->Psum against ws->labels into stats[k].  epoch_slot (device int32 [K], nullable): a guide with epoch_slot[k] in [0, log_rows) ends
 * an epoch with this step: epoch_log[k, slot] = (sum of the epoch's step losses, correct predictions) and both running sums restart at 0. */
int rbnn_conv_svi_guides_finalize(const rbnn_conv_svi_guides_net *net, const int32_t *active, const rbnn_conv_svi_guides_ws *ws,
                                 int32_t with_accuracy, int32_t n_points, const int32_t *epoch_slot, double *epoch_log, int32_t log_rows,
                                 void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * K independent HMC chains over conv nets of ONE shape (1x28x28) with every launch covering all of them (the element-wise kernels:
 * csrc/rbnn_hmc.hip; staging and gradient: csrc/rbnn_conv_train.hip; additive, ABI 10): the transition of rbnn_conv_hmc_* above for K chains,
 * the chain a grid dimension of each launch, as rbnn_hmc_lockstep_* run K fc / fc2 chains.  One transition on one stream:
 *   momentum -> update(OPEN) -> { gradient -> update(step s) } x max_k steps[k] -> decide -> commit
 *   (a leapfrog step: 4 + 7 + 1 = 12 launches; a transition with L = max_k steps[k] steps: 1 + 1 + 12 L + 1 + 1, whatever K is)
 * after ONE conv_hmc_chains_stage of the chains' batches (1 launch, once per batch, not per leapfrog step).
 * Layout.  The chain block is an rbnn_hmc_lockstep with chain_stride == n_params REQUIRED, and its six per-parameter buffers (q_cur, g_cur,
 * r, m_inv, w_mean, w_m2), like the net's W and grad, are TENSOR-MAJOR exactly as rbnn_conv_ens_net's P: six blocks [K, size of tensor t] in
 * state_dict order, block t at K times the single net's offset of tensor t, chain k's tensor at + k * (size of tensor t) — the stacks of
 * rbnn_conv_posterior, so the exact conv forward addresses chain k as sample k.  Everything else is chain-major as in rbnn_hmc_lockstep:
 * the partial sums [K, qpart_stride] / [K, epart_stride], state [K, RBNN_HMC_STATE], log [K, log_rows, RBNN_HMC_LOG] and samples
 * [K, sample_rows, n_params], each sample row FLAT in state_dict order: a row is the single chain's row.
 * Per chain: its key (keys[k]), its step size (its state block), its number of leapfrog steps (steps[k]) and whether a launch touches it at
 * all (active[k]).  All chains of a call share the point count B: chain k's batch is rows[k, 0..B) of the resident data (indices clamped into
 * [0, n_rows)), and the slice plans of the three conv GEMMs are the single chain's for B (there is no counts argument).  The workspace is
 * rbnn_conv_ens_ws, packed [K, B, .] for the call's B, with the sizes of rbnn_conv_ens_sizes.
 * A block of the element-wise kernels covers the same quads (momentum) or the same 256 flat elements (update, commit, window end) of the
 * single chain's layout as the single kernel's block of that index, writes the same partial sum in the same order, and draws from the same
 * Philox counter (e / 4, tensor id, 0, draw id) under keys[k] ^ key_xor; no sum crosses chains, no atomics, no device->host synchronisation:
 * chain k is bit-identical to rbnn_conv_hmc_* + rbnn_conv_svi_train_forward + rbnn_conv_svi_weight_grads running that chain alone on its rows.
 * Every entry point checks, before any launch: net NULL, then the descriptor (geometry / activation: RBNN_ERR_UNSUPPORTED; hidden, n_classes,
 * n_chains outside [1, 65535]: RBNN_ERR_SHAPE), then NULL pointers, then shapes (chain_stride != n_params, the strides of the partial sums,
 * n_points, K n_points <= 2^22, ldx, n_rows, transition, welford_n, sample_row, n_window < 2), then a phase or mode out of range
 * (RBNN_ERR_UNSUPPORTED) and step >= 0 without steps (RBNN_ERR_NULL), then 16-byte alignment of W, grad, X and the workspace buffers.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct rbnn_conv_hmc_chains_net {
    int32_t activation;            /* rbnn_activation                                                              */
    int32_t in_channels, in_width; /* 1, 28 (anything else: RBNN_ERR_UNSUPPORTED)                                  */
    int32_t hidden;                /* Hc = conv2 output channels, a multiple of 16 in [16, 4096]                   */
    int32_t n_classes;             /* C in [1, 16]                                                                 */
    int32_t n_chains;              /* K in [1, 65535], K B <= 2^22                                                 */
    float *W;                      /* [K n_params] the trajectory positions, tensor-major (16-byte aligned)        */
    float *grad;                   /* [K n_params] dCE/dW there, tensor-major (16-byte aligned)                    */
} rbnn_conv_hmc_chains_net;

/* [host] n_params of one chain; the lengths of k0_part and of k1_part / p_part of one chain (rbnn_conv_hmc_sizes'); out: the workspace sizes
 * for n_points points per chain (rbnn_conv_ens_sizes' for K members).  Every out-pointer is nullable; n_points is checked only when out is
 * given.  < 0: rbnn_status. */
int64_t rbnn_conv_hmc_chains_sizes(const rbnn_conv_hmc_chains_net *net, int32_t n_points, int64_t *n_quad_partials, int64_t *n_elem_partials,
                                   rbnn_conv_ens_bytes *out);
/* rbnn_conv_ens_stage of rows [K, n_points]: ws->Xs[k, b] = X[rows[k, b]], ws->labels[k, b] = labels[rows[k, b]].  1 launch. */
int rbnn_conv_hmc_chains_stage(const rbnn_conv_hmc_chains_net *net, const float *X, int32_t ldx, int32_t n_rows, const int32_t *labels,
                               const int32_t *rows, int32_t n_points, const rbnn_conv_ens_ws *ws, void *stream);
/* dCE/dW (summed CE) into net->grad and ce [K, n_points] of every chain at net->W on the staged batches: the exact forward with the chain
 * as the sample, the head with dZ = softmax - e_y, the seven weight-gradient launches of rbnn_conv_ens_weight_grads: 4 + 7 launches.
 * active is NOT consulted: an inactive or finished chain's trajectory buffers are scratch. */
int rbnn_conv_hmc_chains_gradient(const rbnn_conv_hmc_chains_net *net, int32_t n_points, const rbnn_conv_ens_ws *ws, void *stream);
/* rbnn_hmc_lockstep_momentum: the momentum draw of every active chain under keys[k] ^ key_xor with draw id draw_ids[k] (device, nullable:
 * draw_id for every chain).  1 launch. */
int rbnn_conv_hmc_chains_momentum(const rbnn_conv_hmc_chains_net *net, const rbnn_hmc_lockstep *chains, uint64_t key_xor, uint32_t draw_id,
                                  const uint32_t *draw_ids, void *stream);
/* rbnn_hmc_lockstep_update: step < 0: the single chain's update `phase` on every active chain; step >= 0 (needs steps): MID for chains with
 * step + 1 < steps[k], CLOSE at step + 1 == steps[k], nothing for step >= steps[k].  1 launch. */
int rbnn_conv_hmc_chains_update(const rbnn_conv_hmc_chains_net *net, const rbnn_hmc_lockstep *chains, int32_t phase, int32_t step, void *stream);
/* rbnn_hmc_lockstep_decide without counts: one fp64 block per active chain over ce [K, n_points] (ws->ce), the uniform under keys[k].  1 launch. */
int rbnn_conv_hmc_chains_decide(const rbnn_conv_hmc_chains_net *net, const rbnn_hmc_lockstep *chains, const float *ce, int32_t n_points,
                                int64_t transition, int32_t mode, int32_t adapt, int32_t window_end, void *stream);
/* rbnn_hmc_lockstep_commit: the single chain's commit on every active chain, each by its own decision; sample_row >= 0: that row of every
 * chain's stack.  1 launch. */
int rbnn_conv_hmc_chains_commit(const rbnn_conv_hmc_chains_net *net, const rbnn_hmc_lockstep *chains, int32_t force, int32_t welford_n,
                                int64_t sample_row, void *stream);
/* rbnn_hmc_lockstep_window_end: the single chain's window end on every active chain.  1 launch. */
int rbnn_conv_hmc_chains_window_end(const rbnn_conv_hmc_chains_net *net, const rbnn_hmc_lockstep *chains, int32_t n_window, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * fp64 precision mode of the fc / fc2 forward and expected input gradient (csrc/rbnn_fp64.inc): the checker at workload size.
 * The DATA stay fp32 — the posterior exactly as rbnn_posterior holds it, X, the attack iterates — and are widened on load, which
 * is exact; every operation from the first product to the written result is fp64: the contractions over D and H on
 * v_mfma_f64_16x16x4_f64 with fp64 accumulators, bias and activation (leaky slope 0.01 as a double), softmax with the maximum
 * subtracted, the three label losses, act', the sum over samples, the norms.  No atomics and one fixed accumulation order per result
 * element (K ascending, samples ascending): two runs are bit-identical, and a point's result depends neither on n_points nor on the
 * 16-point tile or point block it ran in.  All four activations, n_classes <= 16, hidden a multiple of 4 (RBNN_ERR_SHAPE otherwise;
 * none of the 32 / 64 / k*128 rule of the fp32 kernels), n_samples <= 65535.  No counterpart in the reference (it computes in fp32).
 * Every buffer below is fp64, caller-owned, 16-byte aligned; per-sample buffers are indexed by POSITION in the call (0 .. n_samples-1),
 * the weights by sample_idx.
 * ------------------------------------------------------------------------------------------------------------ */
#define RBNN_F64_WS_BUFFERS 6
/* bytes[0 .. 5] <- sizes of P [S,N,16], dZ [S,N,16], Psum [N,16], dact1 [S,N,H], hid1 [S,N,H] (fc2, else 0), dact2 [S,N,H] (fc2, else 0)
 * for N points x S used samples. [host; bytes: host array of RBNN_F64_WS_BUFFERS] */
int rbnn_f64_workspace_query(const rbnn_posterior *net, int32_t n_points, int32_t n_samples, size_t *bytes);

/* rbnn_fc_forward in fp64: P[s] = softmax(NN_s(X)) (or logits; columns >= C are 0) and the stash act'(pre-activation) of every hidden
 * layer: dact1 (and, fc2, dact2; hid1 takes the first hidden activations between the two launches).  X: fp32 [N, ldx], ldx >= D_pad,
 * multiple of 4, columns [D, D_pad) zero.  fc: 1 launch, fc2: 2. */
int rbnn_fc_forward_f64(const rbnn_posterior *net, const float *X, int32_t ldx, int32_t n_points, const int32_t *sample_idx,
                        int32_t n_samples, int32_t out_kind, double *P, double *dact1, double *hid1, double *dact2, void *stream);

/* rbnn_reduce_samples in fp64: out[n,c] = scale * sum_s P[s,n,c], s = 0, 1, ... in that order (c < C; out row stride ldo doubles). */
int rbnn_reduce_samples_f64(const double *P, int32_t n_samples, int32_t n_points, int32_t n_classes, double scale, double *out,
                            int32_t ldo, void *stream);

/* rbnn_loss_dlogits in fp64 for the three label losses (RBNN_LOSS_MEAN_PROB — the double softmax —, RBNN_LOSS_PER_SAMPLE,
 * RBNN_LOSS_MEAN_LOGIT; the upstream modes of the autograd hook: RBNN_ERR_UNSUPPORTED).  inv_S multiplies every dZ, the per-sample
 * loss included (the 1/S of lossGradients.py:40 is folded in here).  Psum [N,ldp]: sum_s P[s], not needed for RBNN_LOSS_PER_SAMPLE. */
int rbnn_loss_dlogits_f64(int32_t mode, const double *P, const double *Psum, int32_t ldp, const int32_t *labels, int32_t n_samples,
                          double inv_S, int32_t n_points, int32_t n_classes, double *dZ, void *stream);

/* rbnn_fc_input_grad + rbnn_sum_slabs_norms in fp64: G[n,d] = scale * sum_s (dA_s[n,:] . W1_s)[d] for d < D_pad (row stride ldg
 * doubles), the samples summed in ascending order inside one accumulator: no slabs.  linf / l2 (nullable, [N]): the norms of every
 * row over d < D.  CONSUMES the stash: dact1 (and dact2) of rbnn_fc_forward_f64 are overwritten with dL/d(pre-activation) — one
 * backward per forward.  fc: 2 launches, fc2: 3; + 1 with norms. */
int rbnn_fc_input_grad_f64(const rbnn_posterior *net, const int32_t *sample_idx, int32_t n_samples, int32_t n_points, const double *dZ,
                           double *dact1, double *dact2, double scale, double *G, int32_t ldg, double *linf, double *l2, void *stream);

/* rbnn_attack_step with the SIGN read from an fp64 gradient G [N, ldg]: X, X0, alpha, eps and the arithmetic on X are that call's
 * (fp32, both the FGSM and the PGD form) — given equal signs the images are bit-equal to its. */
int rbnn_attack_step_f64(float *X, const float *X0, int32_t ldx, const double *G, int32_t ldg, const float *alpha, float alpha_scalar,
                         float eps, int32_t project, int32_t n_points, int32_t in_features, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * fp64 checker of the conv forward and expected input gradient (csrc/rbnn_conv_fp64.inc): the conv half of the section above, behind
 * entry points of its own (the precision switch keeps refusing conv posteriors).  The DATA stay fp32 — the posterior exactly as
 * rbnn_conv_posterior holds it (K2w_ci is not read), X, the attack iterates — and are widened on load; every operation from the first
 * product to the written result is fp64: conv2 and conv2^T (implicit GEMMs, K = 800 and K = 25 Hc) on v_mfma_f64_16x16x4_f64 with fp64
 * accumulators, conv1, conv1^T and the head in fp64 FMAs, bias, activation (leaky slope 0.01 as a double), softmax with the maximum
 * subtracted.  Pooling compares the activated values and takes the FIRST maximum in row-major window order (torch's rule); act' is
 * taken from the pooled value.  No atomics, one fixed accumulation order per result element, one block per (sample, point): two runs
 * are bit-identical, and a point's result depends neither on n_points nor on the point block it ran in.  Both geometries, all four
 * activations, hidden a multiple of 16, n_classes <= 16, n_points * n_samples < 2^31.  No counterpart in the reference.
 * P, dZ, Psum have the layout of the fc section, so rbnn_reduce_samples_f64, rbnn_loss_dlogits_f64 and rbnn_attack_step_f64 serve
 * unchanged.  Buffers are caller-owned; the fp64 ones 16-byte aligned; per-sample buffers are indexed by POSITION in the call, the
 * weights by sample_idx.  Every argument is checked on the host before any launch: a null pointer RBNN_ERR_NULL; a geometry other
 * than 28 / 1 or 32 / 3, an activation or an out_kind outside the enums RBNN_ERR_UNSUPPORTED; hidden, n_classes, the counts, ldx
 * below Cin*W*W or not a multiple of 4, ldg below Cin*W*W RBNN_ERR_SHAPE; a misaligned X or fp64 buffer RBNN_ERR_ALIGN.
 * ------------------------------------------------------------------------------------------------------------ */
#define RBNN_CONV_FP64_WS_BUFFERS 8
/* bytes[0 .. 7] <- sizes of P [S,N,16], dZ [S,N,16], Psum [N,16], P1 [S,N,32*P1W*P1W] (fp64), arg1 [S,N,32*P1W*P1W] (bytes),
 * Q2 [S,N,Hc*NP2] (fp64), arg2 [S,N,Hc*NP2] (bytes), Gs [S,N,Cin*W*W] (fp64, per-sample input gradients) for N points x S used
 * samples. [host; bytes: host array of RBNN_CONV_FP64_WS_BUFFERS] */
int rbnn_conv_fp64_workspace_query(const rbnn_conv_posterior *net, int32_t n_points, int32_t n_samples, size_t *bytes);

/* rbnn_conv_forward in fp64: P[s] = softmax(NN_s(X)) (or logits; columns >= C are 0), the pooled activations P1 and Q2 and the
 * argmax byte (0..3, row-major in the window) of every pooled output.  X: fp32 [N, ldx].  3 launches. */
int rbnn_conv_forward_fp64(const rbnn_conv_posterior *net, const float *X, int32_t ldx, int32_t n_points, const int32_t *sample_idx,
                           int32_t n_samples, int32_t out_kind, double *P, double *P1, uint8_t *arg1, double *Q2, uint8_t *arg2,
                           void *stream);

/* rbnn_conv_input_grad + the sum over samples + the norms in fp64, from the dZ that rbnn_loss_dlogits_f64 left and the forward's
 * P1 / arg1 / Q2 / arg2 (read only: several backwards may follow one forward): Gs[s,n,:] = dL_s/dx_n, then
 * G[n,d] = scale * sum_s Gs[s,n,d] with s ascending (row stride ldg doubles), linf / l2 (nullable, [N]) the norms of every row.
 * 2 launches; + 1 with norms. */
int rbnn_conv_input_grad_fp64(const rbnn_conv_posterior *net, const int32_t *sample_idx, int32_t n_samples, int32_t n_points,
                              const double *dZ, const double *P1, const uint8_t *arg1, const double *Q2, const uint8_t *arg2,
                              double *Gs, double scale, double *G, int32_t ldg, double *linf, double *l2, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Weight gradients of the conv nets in double precision (csrc/rbnn_conv_wgrad_dp.inc): the checker of the conv trainers' gradients,
 * behind the forward of the section above.  The loss is the trainers' cross-entropy ON THE LOGITS, ce = logsumexp(z) - z_y (not the
 * attack path's loss on probabilities).  After the section's forward with RBNN_OUT_LOGITS: the head below turns the logits into
 * per-point CE and dZ = scale (softmax - e_y); the weight-gradient call runs dZ -> dQ2 -> dO2 -> conv2^T -> dO1 with one block per
 * (sample, point) as the input-gradient call does, writes dO2 and dO1 (dL/d(pre-activation) of both convolutions), and contracts over
 * the points:  dFw | dFb = dZ^T [Q2 | 1],  dK2w | dK2b = sum_{n,pos} dO2 x [P1 patch | 1],  dK1w | dK1b = sum_{n,pos} dO1 x [x patch | 1],
 * all three on v_mfma_f64_16x16x4_f64.  No atomics.  Every output tile of 16 x 16 belongs to one wave, which LOADS its accumulator
 * from the output buffer, walks the call's points in ascending order and stores it back: the six outputs ACCUMULATE, the caller zeroes
 * them before the first point block, and an output element is the same chain of operations wherever the borders of the point blocks
 * fall — bit-identical between runs and between any two point-block sizes.  (An MFMA of dK2 / dK1 takes 4 positions of ONE point,
 * one of dFw takes ONE point.)  Both geometries, all four activations, hidden a multiple of 16, n_classes <= 16,
 * n_points * n_samples < 2^31.  The outputs are indexed by POSITION in the call and have the state_dict's layouts:
 * dK1w [S,32,Cin*25], dK1b [S,32], dK2w [S,Hc,800], dK2b [S,Hc], dFw [S,C,Hc*NP2], dFb [S,C].  Argument checks as in the section above.
 * ------------------------------------------------------------------------------------------------------------ */
#define RBNN_CONV_WGRAD_DP_WS_BUFFERS 3
/* bytes[0 .. 2] <- sizes of ce [S,N], dO2 [S,N,Hc,NPOS], dO1 [S,N,32,O1*O1] (all doubles; NPOS = conv2's output positions, O1 = conv1's
 * output width) for N points x S used samples. [host; bytes: host array of RBNN_CONV_WGRAD_DP_WS_BUFFERS] */
int rbnn_conv_wgrad_dp_workspace_query(const rbnn_conv_posterior *net, int32_t n_points, int32_t n_samples, size_t *bytes);

/* The training head: Z [S,N,16] logits (columns >= C ignored) -> ce[s,n] = logsumexp(z) - z_y (unscaled) and
 * dZ[s,n,c] = scale * (softmax(z)_c - [c = y]) with the maximum subtracted and the label class formed as -(sum of the others) / den
 * (columns >= C are 0).  labels [N], each in [0, C): the caller's to check.  dZ may not alias Z.  1 launch. */
int rbnn_conv_head_ce_dp(const double *Z, const int32_t *labels, int32_t n_samples, int32_t n_points, int32_t n_classes, double scale,
                         double *dZ, double *ce, void *stream);

/* The weight gradients of n_points points, ADDED to the six outputs (see above).  X: fp32 [N, ldx] as in the forward; dZ of the head;
 * P1 / arg1 / Q2 / arg2 of the forward (read only); dO2, dO1: workspaces of the query, written.  4 launches. */
int rbnn_conv_weight_grads_dp(const rbnn_conv_posterior *net, const float *X, int32_t ldx, const int32_t *sample_idx, int32_t n_samples,
                              int32_t n_points, const double *dZ, const double *P1, const uint8_t *arg1, const double *Q2,
                              const uint8_t *arg2, double *dO2, double *dO1, double *dK1w, double *dK1b, double *dK2w, double *dK2b,
                              double *dFw, double *dFb, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Weight gradients of the fc / fc2 nets in double precision (csrc/rbnn_fc_wgrad_dp.inc): the checker of the gradients of the SVI, Adam
 * and HMC trainers, behind the forward and input gradient of the fc section above.  The loss is the trainers' cross-entropy ON THE
 * LOGITS.  The sequence per point block: rbnn_fc_forward_f64 with RBNN_OUT_LOGITS; rbnn_conv_head_ce_dp (it knows no geometry) turns
 * the logits into per-point CE and dZ = scale (softmax - e_y); rbnn_fc_hidden_dp writes the activations of the LAST hidden layer,
 * which the forward keeps on the chip; rbnn_fc_input_grad_f64 turns the act' stashes into dL/d(pre-activation) of every hidden layer
 * (its G is a by-product); rbnn_fc_weight_grads_dp contracts over the points on v_mfma_f64_16x16x4_f64:
 *   dW2 | db2 = dZ^T [hidL | 1],   fc2: dWm | dbm = dact2^T [hid1 | 1],   dW1 | db1 = dact1^T [X | 1].
 * No atomics.  Every output tile of 16 x 16 belongs to one wave, which LOADS its accumulator from the output buffer, walks the call's
 * points in ascending order (an MFMA takes 4 points of one 16-point tile, points past the last contribute zeros) and stores it back:
 * the six outputs ACCUMULATE, the caller zeroes them before the first point block, and with point blocks that are multiples of 16
 * points an output element is the same chain of operations wherever the borders of the blocks fall — bit-identical between runs and
 * between point-block sizes.  All four activations, n_classes <= 16, hidden a multiple of 4, n_samples <= 65535,
 * n_points * n_samples < 2^31.  The outputs are indexed by POSITION in the call and have the state_dict's layouts with the
 * descriptor's hidden and the UNPADDED in_features: dW1 [S,H,D], db1 [S,H], dWm [S,H,H], dbm [S,H] (fc2, else not read), dW2 [S,C,H],
 * db2 [S,C].  A hidden unit the caller padded the net with has act(0) != 0 under the sigmoid: its columns of dWm and dW2 are not zero,
 * the caller's to drop.  Every argument is checked on the host before any launch: a null pointer RBNN_ERR_NULL; ldx below in_stride
 * or not a multiple of 4 and the counts RBNN_ERR_SHAPE; a misaligned X or fp64 input RBNN_ERR_ALIGN; the net as in the fc section.
 * ------------------------------------------------------------------------------------------------------------ */
#define RBNN_FC_WGRAD_DP_WS_BUFFERS 2
/* bytes[0 .. 1] <- sizes of ce [S,N] and hidL [S,N,H] (doubles) for N points x S used samples.
 * [host; bytes: host array of RBNN_FC_WGRAD_DP_WS_BUFFERS] */
int rbnn_fc_wgrad_dp_workspace_query(const rbnn_posterior *net, int32_t n_points, int32_t n_samples, size_t *bytes);

/* hidL[s,n,h] = act(A[s,n,:] . W_s[h,:] + b_s[h]) in fp64 on the f64 MFMA.  fc: A = X (fp32 [N, ldx] as in the forward), W = W1;
 * fc2: A = hid1 of rbnn_fc_forward_f64 (fc: not read), W = Wm.  1 launch. */
int rbnn_fc_hidden_dp(const rbnn_posterior *net, const float *X, int32_t ldx, const int32_t *sample_idx, int32_t n_samples,
                      int32_t n_points, const double *hid1, double *hidL, void *stream);

/* The weight gradients of n_points points, ADDED to the six outputs (see above).  dZ of the head; dact1 (and dact2) as
 * rbnn_fc_input_grad_f64 left them; hid1 of the forward and hidL of rbnn_fc_hidden_dp.  Reads no weight: there is no sample_idx.
 * fc (hid1, dact2, dWm, dbm not read): 2 launches, fc2: 3. */
int rbnn_fc_weight_grads_dp(const rbnn_posterior *net, const float *X, int32_t ldx, int32_t n_samples, int32_t n_points,
                            const double *dZ, const double *dact1, const double *hid1, const double *dact2, const double *hidL,
                            double *dW1, double *db1, double *dWm, double *dbm, double *dW2, double *db2, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Weight-space PCA of posterior samples (csrc/rbnn_wpca.inc): the numerical half of the reference's test_multimodal.py, which
 * projects the flattened samples of HMC posteriors and 1000 draws of the N(0, I) prior onto two principal components with
 * sklearn's PCA on the host.  With n rows of P weights, n << P, PCA is the n x n Gram matrix of the centred rows, contracted
 * over P, and an n x n eigenproblem (the host's).  Rows are fp32 with their own row strides (in elements, >= the columns of the
 * call) and need 4-byte alignment only; every product and sum is double precision, the Gram contraction on
 * v_mfma_f64_16x16x4_f64, and the mean is subtracted in double precision BEFORE the product.  The caller sweeps P in column
 * slabs whose borders are multiples of RBNN_WPCA_CHUNK and passes pointers offset to the slab: every call below sees columns
 * [0, P) of its own pointers.  No atomics; two runs are bit-identical; the bits of C[i,j] are a function of row i of Y, row j of
 * X, mu and the total column count alone — not of m, n, the other rows, the workspace or the slabs.  Every argument is checked on
 * the host before any launch: a null pointer RBNN_ERR_NULL; a count below 1, a stride below the columns, e0 not a multiple of 4,
 * more than RBNN_WPCA_MAX_COMPONENTS components, a workspace below the minimum, a size whose product overflows RBNN_ERR_SHAPE.
 * ------------------------------------------------------------------------------------------------------------ */
#define RBNN_WPCA_CHUNK 2048          /* columns of one partial sum of the Gram contraction */
#define RBNN_WPCA_TENSOR 0x57504341   /* the Philox counter word of the prior's rows ("WPCA") */
#define RBNN_WPCA_MAX_COMPONENTS 16

/* The workspace of rbnn_wpca_cross_gram for Y [m, P] against X [n, P]: one chunk's partials of every 16 x 16 tile,
 * min = ceil(m/16) ceil(n/16) 256 doubles, which the call needs at least; full = ceil(P / RBNN_WPCA_CHUNK) of them, with which it
 * runs one round.  [host] */
int rbnn_wpca_workspace_query(int32_t m, int32_t n, int64_t P, size_t *min_bytes, size_t *full_bytes);

/* out[r - r0, e - e0] (fp32, row stride ld >= w) for rows r0 .. r0 + n and columns e0 .. e0 + w of the prior's matrix: the standard
 * normal of Philox4x32-10 counter (e / 4, RBNN_WPCA_TENSOR, r, 0) under the 64-bit key, component e % 4, through the SVI draw's
 * Box-Muller.  A value depends on (key, r, e) only.  n <= 65535 per call, e0 + w <= 2^34.  1 launch. */
int rbnn_wpca_normal_rows(uint64_t key, int32_t r0, int32_t n, int64_t e0, int64_t w, float *out, int64_t ld, void *stream);

/* mu[e] = (sum_r X[r, e]) / n in double precision, r ascending, e < P.  1 launch. */
int rbnn_wpca_col_mean(const float *X, int64_t ldx, int32_t n, int64_t P, double *mu, void *stream);

/* C[i, j] += sum_{e < P} (Y[i, e] - mu[e]) (X[j, e] - mu[e]) for Y [m, P], X [n, P], C [m, ldc >= n] doubles: the caller zeroes C
 * before the first slab.  One wave per 16 x 16 tile and chunk starts from zero and sums its chunk in a fixed column order; a round
 * is as many chunks as ws (ws_bytes, at least the query's minimum) holds; a second launch per round adds the round's partials to C
 * in chunk order.  2 launches per round. */
int rbnn_wpca_cross_gram(const float *Y, int64_t ldy, int32_t m, const float *X, int64_t ldx, int32_t n, const double *mu, int64_t P,
                         double *C, int64_t ldc, double *ws, size_t ws_bytes, void *stream);

/* V[c, e] = sum_i A[c, i] (X[i, e] - mu[e]) for A [k, n] doubles, k <= RBNN_WPCA_MAX_COMPONENTS, i ascending, V [k, ldv >= P]
 * doubles: the principal axes when A = (u / sqrt(lambda))^T.  1 launch. */
int rbnn_wpca_components(const double *A, int32_t k, const float *X, int64_t ldx, int32_t n, const double *mu, int64_t P, double *V,
                         int64_t ldv, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Per-weight convergence diagnostics of HMC chains (csrc/rbnn_chain_diag.inc): split R-hat and effective sample size per
 * element, what pyro's mcmc.diagnostics() gives per element of every sample site (pyro's ops.stats formulas).  X is the pooled
 * stack of a run of C chains of N draws as fp32 [C * N, ldx >= P], row c * N + t = draw t of chain c, 4-byte alignment; every
 * column is one independent problem, computed by one lane in double precision with plain FMAs:
 *    m_c = (sum_t x[c,t]) / N,  d[c,t] = x[c,t] - m_c             (subtracted before any product)
 *    S[c,k] = sum_{t < N-k} d[c,t] d[c,t+k],  gamma[c,k] = S[c,k] / (N - k)
 *    W = mean_c(gamma[c,0]) N / (N - 1),  V = W (N - 1) / N  (+ the unbiased variance over c of m_c when C > 1)
 *    r_hat = sqrt(V / W);  split_r_hat: the same on the 2C sequences of length h = N / 2, the first h and the last h draws of
 *    each chain (the middle draw of an odd N is dropped): hmc.split_r_hat's value for a [C, N] input
 *    rho_0 = 1,  rho_k = 1 - (W - mean_c gamma[c,k]) / V,  Rho_p = rho_2p + rho_2p+1 for p < N / 2
 *    Rho'_p = min_{q <= p} max(Rho_q, 0)  (Geyer's initial monotone positive sequence)
 *    tau = -1 + 2 sum_p Rho'_p,  n_eff = C N / tau,  n_pairs = the first p with Rho_p <= 0, or N / 2
 *    mean, std: over all C N draws, std unbiased
 * A constant column (W == 0): r_hat and split_r_hat are 1 when V == 0 too and inf otherwise, tau and n_eff NaN, n_pairs 0.
 * Nothing else is clamped: a tau <= 0 of short chains gives the n_eff the formula gives.  Every sum runs in ascending t, then
 * ascending c; no atomics; two runs are bit-identical, and the bits of a column's results are a function of its C N values alone —
 * not of P, the other columns, ldx, the alignment of X or the column slabs of the caller.  Every input element is read from
 * global memory once.  Checked on the host before any launch: X null RBNN_ERR_NULL; C < 1, N < 4,
 * N > RBNN_CHAIN_DIAG_MAX_DRAWS, P < 1, C N >= 2^31, ldx < P or a size whose product overflows RBNN_ERR_SHAPE.
 * ------------------------------------------------------------------------------------------------------------ */
#define RBNN_CHAIN_DIAG_MAX_DRAWS 768   /* draws per chain: 12 N bytes of LDS per column, 16 columns per block at this N */

/* max_draws = RBNN_CHAIN_DIAG_MAX_DRAWS (written whatever the shape); lds_bytes = what a block of rbnn_chain_diag takes at this
 * n_draws: 12 n_draws T with T = 64 (n_draws <= 53), 32 (<= 106) or 16 columns.  Either pointer may be null.  [host] */
int rbnn_chain_diag_query(int32_t n_chains, int32_t n_draws, int64_t P, int32_t *max_draws, size_t *lds_bytes);

/* The seven results per column, doubles [P] (n_pairs: int32 [P]); an output that is null is not written.  1 launch. */
int rbnn_chain_diag(const float *X, int64_t ldx, int32_t n_chains, int32_t n_draws, int64_t P,
                    double *mean, double *std, double *r_hat, double *split_r_hat,
                    double *tau, double *n_eff, int32_t *n_pairs, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Posterior-predictive uncertainty and calibration (csrc/rbnn_predictive.inc): what the per-sample probabilities P [S][N][ldp] that
 * every forward leaves in its workspace say beyond their mean.  P is fp32 (the exact, triple, split and conv forwards) or double
 * precision (the two checkers): elem_type names which, RBNN_PREDICTIVE_FLOAT or RBNN_PREDICTIVE_DOUBLE.  Element (s, n, c) lies at
 * P + s * sample_stride + n * ldp + c (strides in elements, ldp >= C, sample_stride >= N * ldp); columns c >= C are never read.
 * For one point, with p_s[c] the probabilities of sample s, widened to double precision on load — everything from the first sum on
 * is double precision —, natural logarithms and 0 ln 0 = 0:
 *    pbar[c] = (sum_s p_s[c]) / S                                  s ascending
 *    entropy             H = -sum_c pbar[c] ln pbar[c]             c ascending         (total uncertainty)
 *    expected_entropy    E = -(sum_c (sum_s p_s[c] ln p_s[c])) / S s, then c ascending (aleatoric part)
 *    mutual_information  H - E, as that difference; nothing is clamped                 (epistemic part)
 *    prediction          the first maximum of pbar over c < C (torch's argmax rule), int32
 *    confidence          pbar[prediction]
 *    agreement           (double)(number of s whose own first-maximum class == prediction) / (double)S
 *    variance            the population variance over s of p_s[prediction]: Welford's update per class in ascending s
 *                        (d = p - mean; mean += d / (s + 1); M2 += d (p - mean)), M2[prediction] / S — never E[x^2] - m^2
 *    with labels y:      nll = -ln pbar[y] (+inf when pbar[y] == 0), brier = sum_c (pbar[c] - [c == y])^2, c ascending,
 *                        correct = (prediction == y), int32.  A label outside [0, C) names no class: pbar[y] counts as 0.
 * Prefixes: a call takes 1 .. RBNN_PREDICTIVE_MAX_PREFIXES strictly ascending lengths 1 <= S_1 < ... < S_J <= S (a host array) and
 * writes row j of every output, at out + j * out_stride (out_stride >= N, in elements), for the first S_j samples — in ONE pass
 * over P; the bits of row j are those of a call with the single prefix S_j.  Samples past S_J are not read.
 * Calibration bins the points by confidence into n_bins intervals (lo, hi]:
 *    b = min(n_bins - 1, max(0, (int)ceil(confidence * n_bins) - 1))          in double precision, exactly as written
 * and gives per bin the count, the sum of confidence and the number correct, and over all points the sum of nll, the sum of brier
 * and the number correct: RBNN_PREDICTIVE_BLOCK points at a time in ascending order, then the blocks in ascending order.
 * No atomics; two runs are bit-identical; the bits of a point's figures are a function of its own S x C values and the prefix list
 * alone — not of N, the other points, the strides or the alignment of P.  Checked on the host before any launch: a null pointer
 * RBNN_ERR_NULL (outputs excepted: one that is null is not written; nll, brier and correct need labels); n_classes outside
 * 2 .. RBNN_CPAD, a count below 1, ldp < C, sample_stride < N * ldp, out_stride < N, more than RBNN_PREDICTIVE_MAX_PREFIXES
 * prefixes or prefixes not strictly ascending in 1 .. S, n_bins outside 1 .. RBNN_PREDICTIVE_MAX_BINS, a workspace below the
 * query's, an unknown elem_type or a size whose product overflows RBNN_ERR_SHAPE; P or an output off its element's alignment
 * RBNN_ERR_ALIGN.
 * ------------------------------------------------------------------------------------------------------------ */
#define RBNN_PREDICTIVE_FLOAT 0
#define RBNN_PREDICTIVE_DOUBLE 1
#define RBNN_PREDICTIVE_MAX_PREFIXES 8
#define RBNN_PREDICTIVE_MAX_BINS 64
#define RBNN_PREDICTIVE_BLOCK 256     /* points of one partial sum of the calibration */

/* Row j < n_prefixes of every output (doubles; prediction and correct int32) <- the figures of the first prefixes[j] samples.
 * labels: int32 [N] on the device, or null.  prefixes: host array.  1 launch. */
int rbnn_predictive_stats(const void *P, int32_t elem_type, int64_t sample_stride, int32_t ldp, int32_t n_samples, int32_t n_points,
                          int32_t n_classes, const int32_t *labels, const int32_t *prefixes, int32_t n_prefixes, int64_t out_stride,
                          double *entropy, double *expected_entropy, double *mutual_information, double *confidence,
                          double *agreement, double *variance, double *nll, double *brier, int32_t *prediction, int32_t *correct,
                          void *stream);

/* bytes <- the workspace of rbnn_predictive_calibration: ceil(N / RBNN_PREDICTIVE_BLOCK) blocks of 3 n_bins + 3 partial sums of 8
 * bytes.  [host] */
int rbnn_predictive_calibration_query(int32_t n_points, int32_t n_bins, size_t *bytes);

/* confidence (doubles) and correct (int32) of N points, nll and brier (doubles) or null -> bin_count, bin_correct (int64 [n_bins]),
 * bin_confidence (doubles [n_bins]), totals (doubles [2]: the sums of nll and brier, 0 where the input is null) and n_correct
 * (int64 [1]).  ws: 8-byte aligned device memory of at least the query's size.  2 launches. */
int rbnn_predictive_calibration(const double *confidence, const int32_t *correct, const double *nll, const double *brier,
                                int32_t n_points, int32_t n_bins, int64_t *bin_count, double *bin_confidence, int64_t *bin_correct,
                                double *totals, int64_t *n_correct, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ROBUSTBNNS_HIP_H */
