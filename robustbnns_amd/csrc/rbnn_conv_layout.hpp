// rbnn_conv_layout.hpp — the flat parameter layout of a conv net of the 1x28x28 geometry and its shape checks, each stated once for the units
// that train or sample one (rbnn_conv_train.hip: the deterministic, SVI and ensemble trainers; rbnn_svi.hip: the Adam + KL step of the conv SVI
// guides in lockstep; rbnn_hmc.hip: the conv chain).  Host code only.
#pragma once
#include "rbnn_conv_common.hpp"
#include "rbnn_train_core.hpp"

namespace {

constexpr int CONV_MAX_HIDDEN = 4096;

// offsets of the six tensors in state_dict order (model.0.weight, model.0.bias, model.3.weight, model.3.bias, model.7.weight, model.7.bias)
struct ConvLayout { long long K1w, K1b, K2w, K2b, Fw, Fb, n_params; };
inline ConvLayout conv_layout(int Hc, int C) {
    using namespace rbnn_conv_shared;
    ConvLayout L;
    L.K1w = 0; L.K1b = C1 * 25; L.K2w = L.K1b + C1; L.K2b = L.K2w + (long long)Hc * K2; L.Fw = L.K2b + Hc;
    L.Fb = L.Fw + (long long)C * NP2 * Hc; L.n_params = L.Fb + C;
    return L;
}

// the six tensors as the segments of the SVI step's / the HMC chain's Layout: each ONE row of n_elem columns, tensor ids 0..5 in state_dict order
inline Layout conv_svi_layout(int Hc, int C) {
    const ConvLayout c = conv_layout(Hc, C);
    const long long off[7] = {c.K1w, c.K1b, c.K2w, c.K2b, c.Fw, c.Fb, c.n_params};
    Layout L = {};
    L.n = 6;
    long long q = 0;
    for (int i = 0; i < 6; ++i) {
        const int n = (int)(off[i + 1] - off[i]);
        L.s[i] = {off[i], q, 1, n, i};
        q += (n + 3) / 4;
    }
    L.n_params = c.n_params; L.n_quads = q;
    return L;
}

// the descriptor fields every conv training / sampling net struct starts with
inline int check_conv_dims(int activation, int in_channels, int in_width, int hidden, int n_classes) {
    if (activation < RBNN_ACT_RELU || activation > RBNN_ACT_TANH) return RBNN_ERR_UNSUPPORTED;
    if (in_channels != 1 || in_width != rbnn_conv_shared::GeoMnist::IW) return RBNN_ERR_UNSUPPORTED;
    if (hidden < 16 || (hidden & 15) || hidden > CONV_MAX_HIDDEN || n_classes < 1 || n_classes > RBNN_CPAD) return RBNN_ERR_SHAPE;
    return RBNN_OK;
}

// the descriptor of K SVI guides in lockstep (rbnn_conv_train.hip; rbnn_svi.hip: the launch of their Adam + KL step): the K * RBNN_SVI_MULTI_ACC_SAMPLES nets of
// the accuracy forward are a grid dimension, so every entry point takes at most 65535 / RBNN_SVI_MULTI_ACC_SAMPLES guides
constexpr int CONV_SVI_MAX_GUIDES = 65535 / RBNN_SVI_MULTI_ACC_SAMPLES;
inline int check_conv_svils_net(const rbnn_conv_svi_guides_net* n) {
    if (!n) return RBNN_ERR_NULL;
    const int rc = check_conv_dims(n->activation, n->in_channels, n->in_width, n->hidden, n->n_classes);
    if (rc) return rc;
    return (n->n_guides < 1 || n->n_guides > CONV_SVI_MAX_GUIDES) ? RBNN_ERR_SHAPE : RBNN_OK;
}
// the guides' own buffers as the record the host helpers of rbnn_svi_step.hpp take
inline rbnn_svi_multi conv_svils_guides(const rbnn_conv_svi_guides_net* n) {
    return {n->loc, n->raw, n->sigma, n->m_loc, n->v_loc, n->m_raw, n->v_raw, n->kl_part, n->stats, n->keys, n->part_stride};
}

// the descriptor and the point count of K HMC chains in one set of launches (rbnn_conv_train.hip: staging and gradient; rbnn_hmc.hip: the chain's
// element-wise kernels): the chain is a grid dimension, and the packed batches obey the members' limits of rbnn_conv_train.hip
constexpr int CONV_MAX_CHAINS = 65535;
constexpr int CONV_CHAINS_MAX_POINTS = 65536;                        // rbnn_conv_train.hip's MAX_POINTS
constexpr long long CONV_CHAINS_MAX_PACKED = 1LL << 22;              // its MAX_ENS_POINTS: K B
inline int check_conv_chains_net(const rbnn_conv_hmc_chains_net* n) {
    if (!n) return RBNN_ERR_NULL;
    const int rc = check_conv_dims(n->activation, n->in_channels, n->in_width, n->hidden, n->n_classes);
    if (rc) return rc;
    return (n->n_chains < 1 || n->n_chains > CONV_MAX_CHAINS) ? RBNN_ERR_SHAPE : RBNN_OK;
}
inline int check_conv_chains_points(const rbnn_conv_hmc_chains_net* n, int B) {
    return (B < 1 || B > CONV_CHAINS_MAX_POINTS || (long long)n->n_chains * B > CONV_CHAINS_MAX_PACKED) ? RBNN_ERR_SHAPE : RBNN_OK;
}

}  // namespace
