// rbnn_hmc.hip — Hamiltonian Monte Carlo over the weights of an fc / fc2 net (model_bnn.py:260-301: pyro's HMC(model, step_size, num_steps) under
// MCMC(num_samples, warmup_steps)), everything around the potential's gradient.  The position q is the flat parameter buffer of rbnn_train.hip
// (state_dict order, unpadded, row-major), U(q) = sum_b CE(z_b(q), y_b) + 1/2 sum q^2, grad U = dCE/dW + q: dCE/dW is rbnn_svi_train_forward +
// rbnn_svi_weight_grads, called on an rbnn_svi_train_net whose W is the trajectory's position and whose grad receives dCE/dW.
//
//      rbnn_hmc_momentum        r = eps_n rsqrt(m_inv), per-block partial sums of K = 1/2 sum m_inv r^2
//      rbnn_hmc_leapfrog_update one element-wise launch: OPEN (half kick + drift from the cached position), MID (the closing half kick of step k,
//                               the opening half kick and the drift of step k + 1), CLOSE (the last half kick, partial sums of K' and 1/2 sum q^2),
//                               and the plain KICK / DRIFT / ENERGY pieces the fused ones are tested against
//      rbnn_hmc_decide          one block, fp64, fixed order: U', K', dH, accept_prob, u, the decision, dual averaging, the next step size, the log row
//      rbnn_hmc_commit          keeps or replaces the cached position / gradient by the decision, Welford mean / M2, the sample stack's row
//      rbnn_hmc_window_end      m_inv from Welford's M2, then the Welford reset
//
// Randomness.  Momentum: the SVI draw's counter layout (rbnn_common.hpp: Philox4x32-10 counter (quad, tensor id, 0, draw id), quad =
// r * ceil(cols/4) + c/4, components (0,1) and (2,3) Box-Muller pairs of u = (x + 0.5) 2^-32) under the caller's key, draw id = the transition —
// with libm's logf / sincospif instead of the hardware approximations (one launch per transition: accuracy is free here).  The step-size search
// passes key ^ RBNN_HMC_SEARCH_KEY and a draw id counting its tries.  The acceptance uniform of transition i: component 0 of the Philox block
// with counter (i, 0, 0, 0) under key ^ RBNN_HMC_UNIF_KEY, u = x0 2^-32 in [0, 1), exact in fp64.
// No atomics anywhere: every sum has one fixed order, two runs with the same key are bit-identical.
// The parameter layout, its checks and the block reductions are rbnn_train_core.hpp's.  Every entry point refuses what the forward it depends on
// refuses, an out-of-range activation included (RBNN_ERR_UNSUPPORTED).
//
// K chains of one net shape in LOCKSTEP (rbnn_hmc_lockstep_*): the chain is grid dimension y of every launch, as the member is in
// rbnn_nn_train.hip.  dCE/dW of all chains is the lockstep training forward + weight gradients of rbnn_train_gemm.hpp with inv_S = 1 on an
// rbnn_nn_train_net whose P is the trajectory positions; the element-wise and decision kernels run the single chain's device functions on
// chain k's view of the shared buffers.  Per chain: its key, step size (its state block), trajectory length (steps[k]), activity (active[k])
// and number of points (counts[k]).  Chain k is bit-identical to that chain alone.
//
// ONE chain over a CONV net of the 1x28x28 geometry (rbnn_conv_hmc_*): the single chain's kernels, launched on the conv Layout of
// rbnn_conv_layout.hpp — six tensors of one row each, so element e of tensor i draws component e % 4 of the Philox block with counter
// (e / 4, i, 0, draw id), rbnn_conv_svi_*'s counter layout.  dCE/dW is rbnn_conv_svi_train_forward + rbnn_conv_svi_weight_grads on an
// rbnn_conv_svi_train_net whose W is the trajectory's position and whose grad receives dCE/dW.  No device code of its own.
//
// K chains over conv nets of one shape (rbnn_conv_hmc_chains_*): the chain is grid dimension y, the per-parameter buffers are tensor-major (the
// stacks the conv forward and weight gradients of K nets work on: rbnn_conv_hmc_chains_stage / _gradient in rbnn_conv_train.hip).  Chain k is bit-identical to the single conv chain.
//
// Both lockstep forms are ONE set of kernels and one host body per operation: lockstep_momentum / _update / _commit / _window_end_kernel<View>
// call the bodies below with the single chain's flat index on chain k's buffers, and the view (ChainMajor, TensorMajor) says where those lie
// and how its entry points' checks differ; the decision, which touches no per-parameter buffer, is lockstep_decide_kernel for both.
#define RBNN_TRAIN_LOCKSTEP
#include "rbnn_train_gemm.hpp"
#include "rbnn_conv_layout.hpp"

namespace {

// four standard normals from one Philox block, normal4's pairing on libm's logf / sincospif
__device__ __forceinline__ void normal4_libm(const uint32_t x[4], float n[4]) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const float u1 = fminf(((float)x[2 * p] + 0.5f) * 2.3283064365386963e-10f, 0.99999994f);
        const float u2 = ((float)x[2 * p + 1] + 0.5f) * 2.3283064365386963e-10f;
        const float r = sqrtf(-2.f * logf(u1));
        float sn, cs;
        sincospif(2.f * u2, &sn, &cs);
        n[2 * p] = r * cs; n[2 * p + 1] = r * sn;
    }
}

// ---------------------------------------------------------------------------------------------------
// The bodies, each defined once: the single-chain kernels call them with the caller's chain, the lockstep kernels with the view of chain
// blockIdx.y (chain_of).  A chain's arithmetic and reduction orders are therefore the same code in both.
// ---------------------------------------------------------------------------------------------------
// quad q of the momentum draw: r = eps_n rsqrt(m_inv) -> this thread's share of K = 1/2 sum m_inv r^2
__device__ __forceinline__ float momentum_quad(const Layout& L, const rbnn_hmc_chain& c, long long q, unsigned long long key, uint32_t draw_id) {
    float k = 0.f;
    if (q < L.n_quads) {
        const Seg sg = L.s[seg_of(L, q)];
        const int Q = (sg.cols + 3) >> 2;
        const long long ql = q - sg.first_quad;
        const int r = (int)(ql / Q), c4 = (int)(ql % Q);
        uint32_t x[4];
        philox4x32_10((uint32_t)(r * Q + c4), (uint32_t)sg.tensor_id, 0u, draw_id, (uint32_t)key, (uint32_t)(key >> 32), x);
        float eps[4];
        normal4_libm(x, eps);
        const long long base = sg.off + (long long)r * sg.cols + 4 * c4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (4 * c4 + j >= sg.cols) continue;
            const float mi = c.m_inv[base + j], rv = eps[j] * rsqrtf(mi);
            c.r[base + j] = rv;
            k += 0.5f * mi * rv * rv;
        }
    }
    return k;
}

// element i of one update phase; CLOSE and ENERGY leave this thread's shares of K' and 1/2 sum q'^2 in kin / pot
__device__ __forceinline__ void update_element(long long i, long long n, float* __restrict__ W, const float* __restrict__ grad,
                                               const rbnn_hmc_chain& c, int phase, float& kin, float& pot) {
    const float e = (float)c.state[RBNN_HMC_ST_EPS], he = 0.5f * e;
    if (i < n) {
        const float mi = c.m_inv[i];
        float r = c.r[i];
        if (phase == RBNN_HMC_OPEN) {
            float q = c.q_cur[i];
            r = fmaf(-he, c.g_cur[i] + q, r);
            q = fmaf(e * mi, r, q);
            W[i] = q; c.r[i] = r;
        } else if (phase == RBNN_HMC_MID) {
            float q = W[i];
            const float gu = grad[i] + q;
            r = fmaf(-he, gu, r);                       // the closing half kick of step k
            r = fmaf(-he, gu, r);                       // the opening half kick of step k + 1: the same two roundings as the plain sequence
            q = fmaf(e * mi, r, q);
            W[i] = q; c.r[i] = r;
        } else if (phase == RBNN_HMC_KICK || phase == RBNN_HMC_CLOSE) {
            const float q = W[i];
            r = fmaf(-he, grad[i] + q, r);
            c.r[i] = r;
            kin = 0.5f * mi * r * r; pot = 0.5f * q * q;
        } else if (phase == RBNN_HMC_DRIFT) {
            W[i] = fmaf(e * mi, r, W[i]);
        } else {                                        // RBNN_HMC_ENERGY
            const float q = W[i];
            kin = 0.5f * mi * r * r; pot = 0.5f * q * q;
        }
    }
}

__global__ void __launch_bounds__(ELT_THREADS) hmc_momentum_kernel(const Layout L, const rbnn_hmc_chain c, unsigned long long key, uint32_t draw_id) {
    __shared__ float red[ELT_THREADS];
    const float k = momentum_quad(L, c, (long long)blockIdx.x * ELT_THREADS + threadIdx.x, key, draw_id);
    block_sum_to(k, red, c.k0_part);
}

__global__ void __launch_bounds__(ELT_THREADS) hmc_update_kernel(long long n, float* __restrict__ W, const float* __restrict__ grad,
                                                                 const rbnn_hmc_chain c, int phase) {
    __shared__ float red[ELT_THREADS];
    float kin = 0.f, pot = 0.f;
    update_element((long long)blockIdx.x * ELT_THREADS + threadIdx.x, n, W, grad, c, phase, kin, pot);
    if (phase == RBNN_HMC_CLOSE || phase == RBNN_HMC_ENERGY) {
        block_sum_to(kin, red, c.k1_part);
        block_sum_to(pot, red, c.p_part);
    }
}

// the sum of a[0..n) + b[0..m) in fp64: thread t takes elements t, t + 256, ..., then one tree
__device__ __forceinline__ double block_sum64(const float* a, long long n, const float* b, long long m, double* red) {
    const int t = threadIdx.x;
    double s = 0.0;
    for (long long i = t; i < n; i += 256) s += (double)a[i];
    for (long long i = t; i < m; i += 256) s += (double)b[i];
    red[t] = s;
    block_tree64(red);
    const double out = red[0];
    __syncthreads();
    return out;
}

struct DecideArgs {
    rbnn_hmc_chain c;
    const float* ce;
    long long n_points, n_qpart, n_epart, transition;
    unsigned long long key;
    int mode, adapt, window_end;
};

// one block of 256 threads decides one chain
__device__ __forceinline__ void decide_chain(const DecideArgs& a, double* red) {
    const double U1 = block_sum64(a.ce, a.n_points, a.c.p_part, a.n_epart, red);
    const double K1 = block_sum64(a.c.k1_part, a.n_epart, nullptr, 0, red);
    const double K0 = block_sum64(a.c.k0_part, a.n_qpart, nullptr, 0, red);
    if (threadIdx.x != 0) return;
    double* const st = a.c.state;
    st[RBNN_HMC_ST_U_NEW] = U1; st[RBNN_HMC_ST_K_NEW] = K1; st[RBNN_HMC_ST_K_OLD] = K0;
    if (a.mode == RBNN_HMC_DECIDE_INIT) { st[RBNN_HMC_ST_U] = U1; return; }
    double dH = (U1 + K1) - (st[RBNN_HMC_ST_U] + K0);
    if (dH != dH) dH = INFINITY;                                     // NaN counts as +inf
    st[RBNN_HMC_ST_DH] = dH;
    if (a.mode == RBNN_HMC_DECIDE_PROBE) return;
    const double ap = fmin(1.0, exp(-dH));
    const unsigned long long ukey = a.key ^ RBNN_HMC_UNIF_KEY;
    uint32_t x[4];
    philox4x32_10((uint32_t)a.transition, 0u, 0u, 0u, (uint32_t)ukey, (uint32_t)(ukey >> 32), x);
    const double u = (double)x[0] * 2.3283064365386963e-10;         // x0 2^-32, exact
    const bool acc = u < ap;
    const double eps_used = st[RBNN_HMC_ST_EPS];
    if (acc) st[RBNN_HMC_ST_U] = U1;
    st[RBNN_HMC_ST_ACC_PROB] = ap; st[RBNN_HMC_ST_ACCEPTED] = acc ? 1.0 : 0.0; st[RBNN_HMC_ST_UNIF] = u;
    if (a.adapt) {
        // dual averaging (target 0.8, t0 = 10, kappa = 0.75, gamma = 0.05) on log eps
        const double t = st[RBNN_HMC_ST_T] + 1.0, g = 0.8 - ap;
        const double gbar = (1.0 - 1.0 / (t + 10.0)) * st[RBNN_HMC_ST_GBAR] + g / (t + 10.0);
        const double xx = st[RBNN_HMC_ST_MU] - (sqrt(t) / 0.05) * gbar;
        const double eta = pow(t, -0.75);
        const double xbar = (1.0 - eta) * st[RBNN_HMC_ST_XBAR] + eta * xx;
        st[RBNN_HMC_ST_T] = t; st[RBNN_HMC_ST_GBAR] = gbar; st[RBNN_HMC_ST_XBAR] = xbar;
        st[RBNN_HMC_ST_EPS] = exp(a.window_end ? xbar : xx);
    }
    if (a.c.log && a.transition < a.c.log_rows) {
        double* const row = a.c.log + a.transition * RBNN_HMC_LOG;
        row[0] = eps_used; row[1] = dH; row[2] = ap; row[3] = acc ? 1.0 : 0.0; row[4] = u; row[5] = U1; row[6] = K1; row[7] = K0;
    }
}

__global__ void __launch_bounds__(256) hmc_decide_kernel(const DecideArgs a) {
    __shared__ double red[256];
    decide_chain(a, red);
}

__device__ __forceinline__ void commit_element(long long i, const float* __restrict__ W, const float* __restrict__ grad, const rbnn_hmc_chain& c,
                                               int force, float welford_n, float* __restrict__ row) {
    const bool acc = force || c.state[RBNN_HMC_ST_ACCEPTED] != 0.0;
    float q = c.q_cur[i];
    if (acc) {                                                       // a rejection writes nothing: position and gradient stay bit for bit
        q = W[i];
        c.q_cur[i] = q; c.g_cur[i] = grad[i];
    }
    if (welford_n > 0.f) {
        float mean = c.w_mean[i];
        const float d = q - mean;
        mean += d / welford_n;
        c.w_mean[i] = mean;
        c.w_m2[i] = fmaf(d, q - mean, c.w_m2[i]);
    }
    if (row) row[i] = q;
}

__global__ void __launch_bounds__(ELT_THREADS) hmc_commit_kernel(long long n, const float* __restrict__ W, const float* __restrict__ grad,
                                                                 const rbnn_hmc_chain c, int force, float welford_n, float* __restrict__ row) {
    const long long i = (long long)blockIdx.x * ELT_THREADS + threadIdx.x;
    if (i >= n) return;
    commit_element(i, W, grad, c, force, welford_n, row);
}

__device__ __forceinline__ void window_end_element(long long i, const rbnn_hmc_chain& c, float scale, float shift) {
    c.m_inv[i] = fmaf(scale, c.w_m2[i], shift);
    c.w_mean[i] = 0.f; c.w_m2[i] = 0.f;
}

__global__ void __launch_bounds__(ELT_THREADS) hmc_window_end_kernel(long long n, const rbnn_hmc_chain c, float scale, float shift) {
    const long long i = (long long)blockIdx.x * ELT_THREADS + threadIdx.x;
    if (i >= n) return;
    window_end_element(i, c, scale, shift);
}

// ---------------------------------------------------------------------------------------------------
// K chains behind every launch: the chain is grid dimension y.  Chain k's key is keys[k]; with active != NULL a chain whose entry is 0 is
// neither read nor written (its blocks return at once, before any barrier).  No sum crosses chains and a chain's block plan does not depend
// on K: chain k is bit-identical to that chain alone.  The partial sums, state, log and samples of chain k lie at k times their stride; where
// its per-parameter buffers (and its part of W / grad) lie is the VIEW's answer, the one thing the two layouts differ in.
// ---------------------------------------------------------------------------------------------------
struct Chains {
    rbnn_hmc_lockstep s;
    float* W;                                  // the trajectory positions and dCE/dW [K, chain_stride]
    const float* grad;
    long long n_params;
};

__device__ __forceinline__ bool chain_active(const Chains& a) { return !a.s.active || a.s.active[blockIdx.y] != 0; }

// chain blockIdx.y's view, its per-parameter buffers shifted by `shift` (not read by the decision)
__device__ __forceinline__ rbnn_hmc_chain chain_of(const Chains& a, long long shift) {
    const long long k = blockIdx.y;
    rbnn_hmc_chain c;
    c.q_cur = a.s.q_cur + shift; c.g_cur = a.s.g_cur + shift; c.r = a.s.r + shift; c.m_inv = a.s.m_inv + shift;
    c.w_mean = a.s.w_mean + shift; c.w_m2 = a.s.w_m2 + shift;
    c.k0_part = a.s.k0_part + k * a.s.qpart_stride;
    c.k1_part = a.s.k1_part + k * a.s.epart_stride; c.p_part = a.s.p_part + k * a.s.epart_stride;
    c.state = a.s.state + k * RBNN_HMC_STATE;
    c.log = a.s.log ? a.s.log + k * a.s.log_rows * RBNN_HMC_LOG : nullptr;
    c.samples = a.s.samples ? a.s.samples + k * a.s.sample_rows * a.n_params : nullptr;
    c.log_rows = a.s.log_rows; c.sample_rows = a.s.sample_rows;
    return c;
}

__device__ __forceinline__ int seg_of_element(const Layout& L, long long i) {
    int s = 0;
#pragma unroll
    for (int j = 1; j < 6; ++j) if (j < L.n && i >= L.s[j].off) s = j;
    return s;
}

// A view: shift(a, L, i, quad) is what to add to the single chain's flat index i (a quad of the momentum draw, else an element) to reach
// chain blockIdx.y's value in a per-parameter buffer, W or grad; the host members say how the entry points of that layout differ.
//
// CHAIN-MAJOR (rbnn_hmc_lockstep_*): [K, chain_stride], the net an rbnn_nn_train_net whose P / grad are the trajectory buffers.
struct ChainMajor {
    using Net = rbnn_nn_train_net;
    static constexpr bool nulls_before_shapes = false;           // a missing W / grad / further pointer is refused behind the block's shapes
    static __device__ __forceinline__ long long shift(const Chains& a, const Layout&, long long, bool) {
        return (long long)blockIdx.y * a.s.chain_stride;
    }
    static int net(const Net* n, Layout* L, Chains* a, int* K) {
        const int rc = check_members(n);
        if (rc) return rc;
        *L = layout_of(*n); a->W = n->P; a->grad = n->grad; *K = n->n_members;
        return RBNN_OK;
    }
    static bool stride_ok(const Net* n, const Layout& L, long long stride) { return stride >= L.n_params && n->member_stride == stride; }
    static int points(const Net*, int n_points) { return n_points < 1 ? RBNN_ERR_SHAPE : RBNN_OK; }
};

// TENSOR-MAJOR (rbnn_conv_hmc_chains_*): six blocks [K, size of tensor], block t at K times the single chain's offset of tensor t, as the conv
// forward and weight gradients of K nets need them (rbnn_conv_hmc_chains_stage / _gradient in rbnn_conv_train.hip).  A thread finds the
// segment of its quad / element in the single chain's layout and shifts by  K off_t + k size_t - off_t : a block covers the quads / elements
// of the single kernel's block of that index (a block that straddles two tensors has threads with different shifts) and writes the same
// partial sum.  There is no room between chains, and the point count has the conv workspace's limits.
struct TensorMajor {
    using Net = rbnn_conv_hmc_chains_net;
    static constexpr bool nulls_before_shapes = true;
    static __device__ __forceinline__ long long shift(const Chains&, const Layout& L, long long i, bool quad) {
        const Seg& sg = L.s[quad ? seg_of(L, i) : seg_of_element(L, i)];
        return ((long long)gridDim.y - 1) * sg.off + (long long)blockIdx.y * sg.cols;
    }
    static int net(const Net* n, Layout* L, Chains* a, int* K) {
        const int rc = check_conv_chains_net(n);
        if (rc) return rc;
        *L = conv_svi_layout(n->hidden, n->n_classes); a->W = n->W; a->grad = n->grad; *K = n->n_chains;
        return RBNN_OK;
    }
    static bool stride_ok(const Net*, const Layout& L, long long stride) { return stride == L.n_params; }
    static int points(const Net* n, int n_points) { return check_conv_chains_points(n, n_points); }
};

template <class View>
__global__ void __launch_bounds__(ELT_THREADS) lockstep_momentum_kernel(const Layout L, const Chains a, unsigned long long key_xor, uint32_t draw_id,
                                                                        const uint32_t* __restrict__ draw_ids) {
    __shared__ float red[ELT_THREADS];
    if (!chain_active(a)) return;
    const long long q = (long long)blockIdx.x * ELT_THREADS + threadIdx.x;
    const rbnn_hmc_chain c = chain_of(a, View::shift(a, L, q, true));
    const float k = momentum_quad(L, c, q, a.s.keys[blockIdx.y] ^ key_xor, draw_ids ? draw_ids[blockIdx.y] : draw_id);
    block_sum_to(k, red, c.k0_part);
}

// step < 0: `phase` for every active chain.  step >= 0: leapfrog step `step` of chains with their own lengths steps[k]: MID while
// step + 1 < steps[k], CLOSE at step + 1 == steps[k], nothing behind it.
template <class View>
__global__ void __launch_bounds__(ELT_THREADS) lockstep_update_kernel(const Layout L, const Chains a, int phase, int step) {
    __shared__ float red[ELT_THREADS];
    if (!chain_active(a)) return;
    if (step >= 0) {
        const int Lk = a.s.steps[blockIdx.y];
        if (step >= Lk) return;
        phase = step + 1 < Lk ? RBNN_HMC_MID : RBNN_HMC_CLOSE;
    }
    const long long i = (long long)blockIdx.x * ELT_THREADS + threadIdx.x, shift = View::shift(a, L, i, false);
    const rbnn_hmc_chain c = chain_of(a, shift);
    float kin = 0.f, pot = 0.f;
    update_element(i, a.n_params, a.W + shift, a.grad + shift, c, phase, kin, pot);
    if (phase == RBNN_HMC_CLOSE || phase == RBNN_HMC_ENERGY) {
        block_sum_to(kin, red, c.k1_part);
        block_sum_to(pot, red, c.p_part);
    }
}

struct LockstepDecide {
    Chains a;
    const float* ce;                           // [K, n_points]
    const int32_t* counts;                     // [K] or NULL
    long long n_points, n_qpart, n_epart, transition;
    int mode, adapt, window_end;
};

// the decision touches no per-parameter buffer: one kernel for both layouts
__global__ void __launch_bounds__(256) lockstep_decide_kernel(const LockstepDecide d) {
    __shared__ double red[256];
    if (!chain_active(d.a)) return;
    const long long k = blockIdx.y;
    DecideArgs a;
    a.c = chain_of(d.a, 0);
    a.ce = d.ce + k * d.n_points;
    a.n_points = d.counts ? min((long long)max(d.counts[k], 0), d.n_points) : d.n_points;
    a.n_qpart = d.n_qpart; a.n_epart = d.n_epart; a.transition = d.transition; a.key = d.a.s.keys[k];
    a.mode = d.mode; a.adapt = d.adapt; a.window_end = d.window_end;
    decide_chain(a, red);
}

template <class View>
__global__ void __launch_bounds__(ELT_THREADS) lockstep_commit_kernel(const Layout L, const Chains a, int force, float welford_n, long long sample_row) {
    const long long i = (long long)blockIdx.x * ELT_THREADS + threadIdx.x;
    if (i >= a.n_params || !chain_active(a)) return;
    const long long shift = View::shift(a, L, i, false);
    const rbnn_hmc_chain c = chain_of(a, shift);
    commit_element(i, a.W + shift, a.grad + shift, c, force, welford_n, sample_row >= 0 ? c.samples + sample_row * a.n_params : nullptr);
}

template <class View>
__global__ void __launch_bounds__(ELT_THREADS) lockstep_window_end_kernel(const Layout L, const Chains a, float scale, float shift_m) {
    const long long i = (long long)blockIdx.x * ELT_THREADS + threadIdx.x;
    if (i >= a.n_params || !chain_active(a)) return;
    window_end_element(i, chain_of(a, View::shift(a, L, i, false)), scale, shift_m);
}

// ---------------------------------------------------------------------------------------------------
// The range tests and the window-end scalars of every form, each stated once.
// ---------------------------------------------------------------------------------------------------
// the buffers every chain block needs; rbnn_hmc_chain and rbnn_hmc_lockstep name them alike
template <class Block> bool chain_block_null(const Block& c) {
    return !c.q_cur || !c.g_cur || !c.r || !c.m_inv || !c.w_mean || !c.w_m2 || !c.k0_part || !c.k1_part || !c.p_part || !c.state;
}

int check_chain(const rbnn_hmc_chain* c) { return (!c || chain_block_null(*c)) ? RBNN_ERR_NULL : RBNN_OK; }

int check_phase(int phase) { return (phase < RBNN_HMC_OPEN || phase > RBNN_HMC_ENERGY) ? RBNN_ERR_UNSUPPORTED : RBNN_OK; }

int check_decision(long long transition, int mode) {
    if (transition < 0) return RBNN_ERR_SHAPE;
    return (mode < RBNN_HMC_DECIDE_INIT || mode > RBNN_HMC_DECIDE_TRANSITION) ? RBNN_ERR_UNSUPPORTED : RBNN_OK;
}

int check_commit(const float* samples, long long sample_rows, long long sample_row, int welford_n) {
    if (sample_row >= 0) {
        if (!samples) return RBNN_ERR_NULL;
        if (sample_row >= sample_rows) return RBNN_ERR_SHAPE;
    }
    return welford_n < 0 ? RBNN_ERR_SHAPE : RBNN_OK;
}

// m_inv = (n / (n + 5)) M2 / (n - 1) + 1e-3 * 5 / (n + 5): the two scalars are formed in double and rounded to fp32 once
struct WindowEnd { float scale, shift; };
int window_end_scalars(int n_window, WindowEnd* out) {
    if (n_window < 2) return RBNN_ERR_SHAPE;
    const double w = (double)n_window;
    *out = {(float)(w / ((w + 5.0) * (w - 1.0))), (float)(1e-3 * 5.0 / (w + 5.0))};
    return RBNN_OK;
}

// ---------------------------------------------------------------------------------------------------
// One chain: what the fc / fc2 entry points (rbnn_hmc_*) and the conv ones (rbnn_conv_hmc_*) do once their net has become a Layout and the
// trajectory's buffers.  The checks keep the order of the entry points' documentation; nothing is launched before all of them have passed.
// ---------------------------------------------------------------------------------------------------
// the layout of an fc / fc2 net, or of a conv net of the 1x28x28 geometry (six tensors of one row each: rbnn_conv_svi_*'s counter layout)
int chain_layout(const rbnn_svi_train_net* net, Layout* L) {
    const int rc = check_net(net);
    if (!rc) *L = layout_of(*net);
    return rc;
}
int chain_layout(const rbnn_conv_svi_train_net* net, Layout* L) {
    if (!net) return RBNN_ERR_NULL;
    const int rc = check_conv_dims(net->activation, net->in_channels, net->in_width, net->hidden, net->n_classes);
    if (!rc) *L = conv_svi_layout(net->hidden, net->n_classes);
    return rc;
}

template <class Net> int64_t chain_sizes(const Net* net, int64_t* n_quad_partials, int64_t* n_elem_partials) {
    Layout L;
    const int rc = chain_layout(net, &L);
    if (rc) return rc;
    if (n_quad_partials) *n_quad_partials = blocks_for(L.n_quads);
    if (n_elem_partials) *n_elem_partials = blocks_for(L.n_params);
    return L.n_params;
}

template <class Net> int chain_momentum(const Net* net, const rbnn_hmc_chain* chain, uint64_t key, uint32_t draw_id, void* stream) {
    Layout L;
    int rc = chain_layout(net, &L);
    if (rc || (rc = check_chain(chain))) return rc;
    hipLaunchKernelGGL(hmc_momentum_kernel, dim3(blocks_for(L.n_quads)), dim3(ELT_THREADS), 0, (hipStream_t)stream, L, *chain,
                       (unsigned long long)key, draw_id);
    return launch_status();
}

template <class Net> int chain_update(const Net* net, const rbnn_hmc_chain* chain, int32_t phase, void* stream) {
    Layout L;
    int rc = chain_layout(net, &L);
    if (rc || (rc = check_chain(chain))) return rc;
    if (!net->W || !net->grad) return RBNN_ERR_NULL;
    if ((rc = check_phase(phase))) return rc;
    const long long n = L.n_params;
    hipLaunchKernelGGL(hmc_update_kernel, dim3(blocks_for(n)), dim3(ELT_THREADS), 0, (hipStream_t)stream, n, net->W, net->grad, *chain, (int)phase);
    return launch_status();
}

template <class Net> int chain_decide(const Net* net, const rbnn_hmc_chain* chain, const float* ce, int32_t n_points, uint64_t key,
                                      int64_t transition, int32_t mode, int32_t adapt, int32_t window_end, void* stream) {
    Layout L;
    int rc = chain_layout(net, &L);
    if (rc || (rc = check_chain(chain))) return rc;
    if (!ce) return RBNN_ERR_NULL;
    if (n_points < 1) return RBNN_ERR_SHAPE;
    if ((rc = check_decision(transition, mode))) return rc;
    DecideArgs a = {};
    a.c = *chain; a.ce = ce; a.n_points = n_points; a.n_qpart = blocks_for(L.n_quads); a.n_epart = blocks_for(L.n_params);
    a.transition = transition; a.key = key; a.mode = mode; a.adapt = adapt; a.window_end = window_end;
    hipLaunchKernelGGL(hmc_decide_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status();
}

template <class Net> int chain_commit(const Net* net, const rbnn_hmc_chain* chain, int32_t force, int32_t welford_n, int64_t sample_row,
                                      void* stream) {
    Layout L;
    int rc = chain_layout(net, &L);
    if (rc || (rc = check_chain(chain))) return rc;
    if (!net->W || !net->grad) return RBNN_ERR_NULL;
    if ((rc = check_commit(chain->samples, chain->sample_rows, sample_row, welford_n))) return rc;
    const long long n = L.n_params;
    hipLaunchKernelGGL(hmc_commit_kernel, dim3(blocks_for(n)), dim3(ELT_THREADS), 0, (hipStream_t)stream, n, net->W, net->grad, *chain, (int)force,
                       (float)welford_n, sample_row >= 0 ? chain->samples + sample_row * n : nullptr);
    return launch_status();
}

template <class Net> int chain_window_end(const Net* net, const rbnn_hmc_chain* chain, int32_t n_window, void* stream) {
    Layout L;
    int rc = chain_layout(net, &L);
    WindowEnd w;
    if (rc || (rc = check_chain(chain)) || (rc = window_end_scalars(n_window, &w))) return rc;
    const long long n = L.n_params;
    hipLaunchKernelGGL(hmc_window_end_kernel, dim3(blocks_for(n)), dim3(ELT_THREADS), 0, (hipStream_t)stream, n, *chain, w.scale, w.shift);
    return launch_status();
}

// ---------------------------------------------------------------------------------------------------
// K chains: what the chain-major entry points (rbnn_hmc_lockstep_*) and the tensor-major ones (rbnn_conv_hmc_chains_*) do once the view has
// turned their net into a Layout, the trajectory's buffers and K.  Each keeps the order of its header section's refusals.
// ---------------------------------------------------------------------------------------------------
struct Lockstep { Layout L; Chains a; int K; };

// net NULL and the descriptor, the chain block's NULL pointers, its shapes.  trajectory: the call reads the net's W / grad; more: one further
// pointer of the call, needed when `need_more`: refused where the view's section says, in front of the shapes or behind them.
template <class View>
int lockstep_args(const typename View::Net* net, const rbnn_hmc_lockstep* c, bool trajectory, bool need_more, const void* more, Lockstep* out) {
    const int rc = View::net(net, &out->L, &out->a, &out->K);
    if (rc) return rc;
    if (!c || chain_block_null(*c) || !c->keys) return RBNN_ERR_NULL;
    const bool missing = (trajectory && (!out->a.W || !out->a.grad)) || (need_more && !more);
    if (View::nulls_before_shapes && missing) return RBNN_ERR_NULL;
    const Layout& L = out->L;
    if (!View::stride_ok(net, L, c->chain_stride)) return RBNN_ERR_SHAPE;
    if (c->qpart_stride < (long long)blocks_for(L.n_quads) || c->epart_stride < (long long)blocks_for(L.n_params)) return RBNN_ERR_SHAPE;
    if (c->log_rows < 0 || c->sample_rows < 0) return RBNN_ERR_SHAPE;
    if (missing) return RBNN_ERR_NULL;
    out->a.s = *c; out->a.n_params = L.n_params;
    return RBNN_OK;
}

template <class View>
int lockstep_momentum(const typename View::Net* net, const rbnn_hmc_lockstep* chains, uint64_t key_xor, uint32_t draw_id, const uint32_t* draw_ids,
                      void* stream) {
    Lockstep l = {};
    const int rc = lockstep_args<View>(net, chains, false, false, nullptr, &l);
    if (rc) return rc;
    hipLaunchKernelGGL(lockstep_momentum_kernel<View>, dim3(blocks_for(l.L.n_quads), l.K), dim3(ELT_THREADS), 0, (hipStream_t)stream, l.L, l.a,
                       (unsigned long long)key_xor, draw_id, draw_ids);
    return launch_status();
}

template <class View>
int lockstep_update(const typename View::Net* net, const rbnn_hmc_lockstep* chains, int32_t phase, int32_t step, void* stream) {
    Lockstep l = {};
    int rc = lockstep_args<View>(net, chains, true, false, nullptr, &l);
    if (rc) return rc;
    if (step >= 0 && !chains->steps) return RBNN_ERR_NULL;
    if (step < 0 && (rc = check_phase(phase))) return rc;
    hipLaunchKernelGGL(lockstep_update_kernel<View>, dim3(blocks_for(l.a.n_params), l.K), dim3(ELT_THREADS), 0, (hipStream_t)stream, l.L, l.a,
                       (int)phase, (int)step);
    return launch_status();
}

// counts: NULL for every chain on all n_points points (the tensor-major form has no counts)
template <class View>
int lockstep_decide(const typename View::Net* net, const rbnn_hmc_lockstep* chains, const float* ce, const int32_t* counts, int32_t n_points,
                    int64_t transition, int32_t mode, int32_t adapt, int32_t window_end, void* stream) {
    Lockstep l = {};
    int rc = lockstep_args<View>(net, chains, false, true, ce, &l);
    if (rc || (rc = View::points(net, n_points)) || (rc = check_decision(transition, mode))) return rc;
    LockstepDecide d = {};
    d.a = l.a; d.ce = ce; d.counts = counts; d.n_points = n_points; d.n_qpart = blocks_for(l.L.n_quads); d.n_epart = blocks_for(l.L.n_params);
    d.transition = transition; d.mode = mode; d.adapt = adapt; d.window_end = window_end;
    hipLaunchKernelGGL(lockstep_decide_kernel, dim3(1, l.K), dim3(256), 0, (hipStream_t)stream, d);
    return launch_status();
}

template <class View>
int lockstep_commit(const typename View::Net* net, const rbnn_hmc_lockstep* chains, int32_t force, int32_t welford_n, int64_t sample_row,
                    void* stream) {
    Lockstep l = {};
    int rc = lockstep_args<View>(net, chains, true, sample_row >= 0, chains ? chains->samples : nullptr, &l);
    if (rc || (rc = check_commit(chains->samples, chains->sample_rows, sample_row, welford_n))) return rc;
    hipLaunchKernelGGL(lockstep_commit_kernel<View>, dim3(blocks_for(l.a.n_params), l.K), dim3(ELT_THREADS), 0, (hipStream_t)stream, l.L, l.a,
                       (int)force, (float)welford_n, (long long)sample_row);
    return launch_status();
}

template <class View> int lockstep_window_end(const typename View::Net* net, const rbnn_hmc_lockstep* chains, int32_t n_window, void* stream) {
    Lockstep l = {};
    WindowEnd w;
    int rc = lockstep_args<View>(net, chains, false, false, nullptr, &l);
    if (rc || (rc = window_end_scalars(n_window, &w))) return rc;
    hipLaunchKernelGGL(lockstep_window_end_kernel<View>, dim3(blocks_for(l.a.n_params), l.K), dim3(ELT_THREADS), 0, (hipStream_t)stream, l.L, l.a,
                       w.scale, w.shift);
    return launch_status();
}


}  // namespace

extern "C" {

int64_t rbnn_hmc_sizes(const rbnn_svi_train_net* net, int64_t* n_quad_partials, int64_t* n_elem_partials) {
    return chain_sizes(net, n_quad_partials, n_elem_partials);
}
int rbnn_hmc_momentum(const rbnn_svi_train_net* net, const rbnn_hmc_chain* chain, uint64_t key, uint32_t draw_id, void* stream) {
    return chain_momentum(net, chain, key, draw_id, stream);
}
int rbnn_hmc_leapfrog_update(const rbnn_svi_train_net* net, const rbnn_hmc_chain* chain, int32_t phase, void* stream) {
    return chain_update(net, chain, phase, stream);
}
int rbnn_hmc_decide(const rbnn_svi_train_net* net, const rbnn_hmc_chain* chain, const float* ce, int32_t n_points, uint64_t key,
                    int64_t transition, int32_t mode, int32_t adapt, int32_t window_end, void* stream) {
    return chain_decide(net, chain, ce, n_points, key, transition, mode, adapt, window_end, stream);
}
int rbnn_hmc_commit(const rbnn_svi_train_net* net, const rbnn_hmc_chain* chain, int32_t force, int32_t welford_n, int64_t sample_row,
                    void* stream) {
    return chain_commit(net, chain, force, welford_n, sample_row, stream);
}
int rbnn_hmc_window_end(const rbnn_svi_train_net* net, const rbnn_hmc_chain* chain, int32_t n_window, void* stream) {
    return chain_window_end(net, chain, n_window, stream);
}

// ---- one chain over a conv net of the 1x28x28 geometry: the same kernels on the conv Layout ----
int64_t rbnn_conv_hmc_sizes(const rbnn_conv_svi_train_net* net, int64_t* n_quad_partials, int64_t* n_elem_partials) {
    return chain_sizes(net, n_quad_partials, n_elem_partials);
}
int rbnn_conv_hmc_momentum(const rbnn_conv_svi_train_net* net, const rbnn_hmc_chain* chain, uint64_t key, uint32_t draw_id, void* stream) {
    return chain_momentum(net, chain, key, draw_id, stream);
}
int rbnn_conv_hmc_leapfrog_update(const rbnn_conv_svi_train_net* net, const rbnn_hmc_chain* chain, int32_t phase, void* stream) {
    return chain_update(net, chain, phase, stream);
}
int rbnn_conv_hmc_decide(const rbnn_conv_svi_train_net* net, const rbnn_hmc_chain* chain, const float* ce, int32_t n_points, uint64_t key,
                         int64_t transition, int32_t mode, int32_t adapt, int32_t window_end, void* stream) {
    return chain_decide(net, chain, ce, n_points, key, transition, mode, adapt, window_end, stream);
}
int rbnn_conv_hmc_commit(const rbnn_conv_svi_train_net* net, const rbnn_hmc_chain* chain, int32_t force, int32_t welford_n, int64_t sample_row,
                         void* stream) {
    return chain_commit(net, chain, force, welford_n, sample_row, stream);
}
int rbnn_conv_hmc_window_end(const rbnn_conv_svi_train_net* net, const rbnn_hmc_chain* chain, int32_t n_window, void* stream) {
    return chain_window_end(net, chain, n_window, stream);
}

// ---- K chains in lockstep ----
int rbnn_hmc_lockstep_gradient(const rbnn_nn_train_net* net, const float* X, int32_t ldx, int32_t n_rows, const int32_t* labels,
                               const int32_t* rows, const int32_t* counts, int32_t n_points, const rbnn_nn_train_ws* ws, void* stream) {
    const LockstepBatch b = {X, ldx, n_rows, labels, rows, counts, n_points};
    if (net && !net->grad) return RBNN_ERR_NULL;                                     // before the forward is launched
    const int rc = lockstep_forward(net, b, ws, 1.f, (hipStream_t)stream);
    return rc ? rc : lockstep_weight_grads(net, b, ws, (hipStream_t)stream);
}

int rbnn_hmc_lockstep_momentum(const rbnn_nn_train_net* net, const rbnn_hmc_lockstep* chains, uint64_t key_xor, uint32_t draw_id,
                               const uint32_t* draw_ids, void* stream) {
    return lockstep_momentum<ChainMajor>(net, chains, key_xor, draw_id, draw_ids, stream);
}
int rbnn_hmc_lockstep_update(const rbnn_nn_train_net* net, const rbnn_hmc_lockstep* chains, int32_t phase, int32_t step, void* stream) {
    return lockstep_update<ChainMajor>(net, chains, phase, step, stream);
}
int rbnn_hmc_lockstep_decide(const rbnn_nn_train_net* net, const rbnn_hmc_lockstep* chains, const float* ce, const int32_t* counts,
                             int32_t n_points, int64_t transition, int32_t mode, int32_t adapt, int32_t window_end, void* stream) {
    return lockstep_decide<ChainMajor>(net, chains, ce, counts, n_points, transition, mode, adapt, window_end, stream);
}
int rbnn_hmc_lockstep_commit(const rbnn_nn_train_net* net, const rbnn_hmc_lockstep* chains, int32_t force, int32_t welford_n, int64_t sample_row,
                             void* stream) {
    return lockstep_commit<ChainMajor>(net, chains, force, welford_n, sample_row, stream);
}
int rbnn_hmc_lockstep_window_end(const rbnn_nn_train_net* net, const rbnn_hmc_lockstep* chains, int32_t n_window, void* stream) {
    return lockstep_window_end<ChainMajor>(net, chains, n_window, stream);
}

// ---- K chains over conv nets: tensor-major buffers (staging and gradient: rbnn_conv_train.hip) ----
int rbnn_conv_hmc_chains_momentum(const rbnn_conv_hmc_chains_net* net, const rbnn_hmc_lockstep* chains, uint64_t key_xor, uint32_t draw_id,
                                  const uint32_t* draw_ids, void* stream) {
    return lockstep_momentum<TensorMajor>(net, chains, key_xor, draw_id, draw_ids, stream);
}
int rbnn_conv_hmc_chains_update(const rbnn_conv_hmc_chains_net* net, const rbnn_hmc_lockstep* chains, int32_t phase, int32_t step, void* stream) {
    return lockstep_update<TensorMajor>(net, chains, phase, step, stream);
}
int rbnn_conv_hmc_chains_decide(const rbnn_conv_hmc_chains_net* net, const rbnn_hmc_lockstep* chains, const float* ce, int32_t n_points,
                                int64_t transition, int32_t mode, int32_t adapt, int32_t window_end, void* stream) {
    return lockstep_decide<TensorMajor>(net, chains, ce, nullptr, n_points, transition, mode, adapt, window_end, stream);
}
int rbnn_conv_hmc_chains_commit(const rbnn_conv_hmc_chains_net* net, const rbnn_hmc_lockstep* chains, int32_t force, int32_t welford_n,
                                int64_t sample_row, void* stream) {
    return lockstep_commit<TensorMajor>(net, chains, force, welford_n, sample_row, stream);
}
int rbnn_conv_hmc_chains_window_end(const rbnn_conv_hmc_chains_net* net, const rbnn_hmc_lockstep* chains, int32_t n_window, void* stream) {
    return lockstep_window_end<TensorMajor>(net, chains, n_window, stream);
}

}  // extern "C"
