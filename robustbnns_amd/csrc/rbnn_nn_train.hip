// rbnn_nn_train.hip — deterministic training of fc / fc2 nets (model_nn.py:175-219: torch.optim.Adam on nn.CrossEntropyLoss()), for M
// independent members of the same shape in LOCKSTEP (model_ensemble.py:69-83 trains them one after the other): every launch of a step covers
// all M members, the member is a grid dimension.
//
//      rbnn_nn_train_forward    A1 = X[rows] W1^T + b1 -> H1 (fc2: -> A2 -> H2), logits, CE per point, dZ = (softmax - e_y) / B (the loss is a
//                               MEAN over the batch), correct/incorrect per point from these logits, and the backward down to
//                               dL/d(pre-activation) of every hidden layer (fc: 2 launches, fc2: 4)
//      rbnn_nn_weight_grads     dW2 = dZ^T H, dWm = dA2^T H1, dW1 = dA1^T X[rows] and every bias gradient of every member: ONE launch
//      rbnn_nn_adam_step        torch.optim.Adam's single-tensor formula on every parameter of every member: one launch
//      rbnn_nn_train_finalize   per member: the fp32-rounded mean CE of the step, its running sum, the correct predictions (fp64, fixed order)
//
// The batch is read from a RESIDENT data matrix through an index array rows [M, B]: each member reads its own batch of its own permutation,
// nothing is copied.  The tile plan of a member does not depend on M and no sum crosses members: member m of a lockstep run is bit-identical
// to the same member trained alone.  No atomics anywhere: every sum has one fixed order.
// The parameter layout (one member's: Layout::s[i].off), the activations, Adam's formula and the fp64 tree are rbnn_train_core.hpp; the GEMM
// and head kernels are rbnn_train_gemm.hpp; the Adam and step-statistics kernels are rbnn_nn_step.hpp (shared with the conv net of
// rbnn_conv_train.hip), launched here as <true>: the member is a grid dimension.
#define RBNN_TRAIN_LOCKSTEP
#include "rbnn_train_gemm.hpp"
#include "rbnn_nn_step.hpp"

extern "C" {

int64_t rbnn_nn_train_sizes(const rbnn_nn_train_net* net) {
    const int rc = check_members(net);
    if (rc) return rc;
    return layout_of(*net).n_params;
}

int rbnn_nn_train_forward(const rbnn_nn_train_net* net, const float* X, int32_t ldx, int32_t n_rows, const int32_t* labels, const int32_t* rows,
                          int32_t n_points, const rbnn_nn_train_ws* ws, void* stream) {
    const LockstepBatch b = {X, ldx, n_rows, labels, rows, nullptr, n_points};
    return lockstep_forward(net, b, ws, 1.f / (float)n_points, (hipStream_t)stream);      // n_points < 1 is refused before inv_S is used
}

int rbnn_nn_weight_grads(const rbnn_nn_train_net* net, const float* X, int32_t ldx, int32_t n_rows, const int32_t* rows, int32_t n_points,
                         const rbnn_nn_train_ws* ws, void* stream) {
    const LockstepBatch b = {X, ldx, n_rows, nullptr, rows, nullptr, n_points};
    return lockstep_weight_grads(net, b, ws, (hipStream_t)stream);
}

int rbnn_nn_adam_step(const rbnn_nn_train_net* net, int64_t step, double lr, double beta1, double beta2, double adam_eps, void* stream) {
    int rc = check_members(net);
    if (rc) return rc;
    if (!net->P || !net->m || !net->v || !net->grad) return RBNN_ERR_NULL;
    AdamArgs a = {};
    a.n_params = layout_of(*net).n_params;
    if (step < 1 || net->member_stride < a.n_params) return RBNN_ERR_SHAPE;
    a.P = net->P; a.m = net->m; a.v = net->v; a.grad = net->grad; a.member_stride = net->member_stride;
    a.s = adam_scalars(step, lr, beta1, beta2, adam_eps);
    hipLaunchKernelGGL(nn_adam_kernel<true>, dim3(blocks_for(a.n_params), net->n_members), dim3(ELT_THREADS), 0,
                       (hipStream_t)stream, a);
    return launch_status();
}

int rbnn_nn_train_finalize(const rbnn_nn_train_net* net, const rbnn_nn_train_ws* ws, int32_t n_points, double* stats, void* stream) {
    int rc = check_members(net);
    if (rc) return rc;
    if (!ws || !ws->ce || !ws->correct || !stats) return RBNN_ERR_NULL;
    if (n_points < 1) return RBNN_ERR_SHAPE;
    FinalArgs a = {ws->ce, ws->correct, stats, n_points};
    hipLaunchKernelGGL(nn_finalize_kernel<true>, dim3(net->n_members), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status();
}

}  // extern "C"

// the weight-space PCA of posterior samples: entry points of its own, nothing of the trainers' (see the file's header for why it sits here)
#include "rbnn_wpca.inc"
// ... and the per-weight diagnostics of HMC chains, for the same reason
#include "rbnn_chain_diag.inc"
// ... and the posterior-predictive uncertainty and calibration kernels
#include "rbnn_predictive.inc"
