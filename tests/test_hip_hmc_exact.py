"""GPU tests (-m gpu) that hold HMC (csrc/rbnn_hmc.hip, robustbnns_amd/hmc.py) to properties that are true whoever wrote them down, not to
tests/hmc_restate.py (which the same hand wrote): the leapfrog against the closed form of a harmonic oscillator, time reversal, stationarity
of N(0, I) under a non-unit mass, what adaptation must achieve on a known posterior, Welford against a two-pass fp64 variance, and a
non-finite trajectory as a plain rejection.  The closed forms and inputs are tests/hmc_exact_cases.py (numpy fp64, nothing of the restatement's).
Every bound is an existing hmc_restate.BOUND entry, a new MEASURED_FP32 entry x 4, or a stated statistical condition with the fp64
restatement's own CPU figure beside it."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import hmc_exact_cases as HX
import hmc_restate as HR
from hmc_restate import BOUND

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("built_library")]
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"


def _relmax(a, b):
    """max |a - b| over max |b| in fp64 (b: the reference)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _one_class_sampler(arch, c, eps, steps, key, **kw):
    from robustbnns_amd.hmc import HmcSampler
    s = HmcSampler(arch, "tanh", (1, 2, 1), 1, c["q0"], eps, steps, DEV, key, batch_size=8, **kw)
    assert s.n_params == c["n"]
    return s


def _one_class_lockstep(q0s, eps, steps, keys, **kw):
    from robustbnns_amd.hmc import LockstepHmc
    return LockstepHmc("fc", "tanh", (1, 2, 1), 1, q0s, eps, steps, DEV, keys, batch_size=8, **kw)


# ---- a. the leapfrog against the closed form ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 6, 10])
@pytest.mark.parametrize("arch", ["fc", "fc2"])
def test_leapfrog_matches_the_harmonic_oscillator(arch, L):
    """One class: dCE/dW = 0 exactly, so every coordinate is a harmonic oscillator with omega^2 = m_inv[i] and L steps are the L-th power of a
    2 x 2 matrix (hmc_exact_cases.leapfrog_closed_form).  m_inv is a hand-set mix of 0.25, 1 and 4: a momentum scaled by the wrong power of
    m_inv, or a drift without it, is off by factors of 2 to 16 here.  Fused and plain updates, K' and 1/2 sum q'^2 from the partial sums."""
    c = HX.one_class_case(arch)
    s = _one_class_sampler(arch, c, HX.EPS, L, 1, adapt_step_size=False)
    s.m_inv.copy_(c["m_inv"])
    s.stage(c["x"].to(DEV), c["lab"].to(DEV))
    assert s.read_state()["eps"] == HX.EPS
    q1, r1, K1, P1 = HX.leapfrog_closed_form(s.q_cur.cpu().numpy(), c["r0"].numpy(), c["m_inv"].numpy(), HX.EPS, L)
    assert _relmax(q1, s.q_cur.cpu().numpy()) > 0.05                             # the trajectory goes somewhere
    for fused in (True, False):
        s.r.copy_(c["r0"])
        s.leapfrog(L, fused=fused)
        torch.cuda.synchronize()
        assert bool((s.grad == 0).all()) and bool((s.g_cur == 0).all()), "dCE/dW of a one-class net is not exactly zero"
        assert bool((s.ws_t["ce"][:8] == 0).all()), "CE of a one-class net is not exactly zero"
        eq, er = _relmax(s.W.cpu().numpy(), q1), _relmax(s.r.cpu().numpy(), r1)
        K, P = float(s.k1_part.double().sum()), float(s.p_part.double().sum())
        eK, eP = abs(K - K1) / K1, abs(P - P1) / P1
        print(f"[{arch} L {L} {'fused' if fused else 'plain'}] q {eq:.2e} ({eq / BOUND['leapfrog_q']:.2f} x bound)  r {er:.2e} ({er / BOUND['leapfrog_r']:.2f} x)"
              f"  K' {eK:.2e} ({eK / BOUND['K']:.2f} x)  1/2 sum q'^2 {eP:.2e} ({eP / BOUND['U']:.2f} x)")
        assert eq <= BOUND["leapfrog_q"] and er <= BOUND["leapfrog_r"]
        assert eK <= BOUND["K"] and eP <= BOUND["U"]


# ---- b. time reversal -----------------------------------------------------------------------------------------------------------------
def test_time_reversal_on_a_real_net():
    """fc2 / tanh, D 10, H 32, C 3, B 37 (hmc_restate.REVERSE_CASE, a LEAP_CASES shape with a non-unit mass): 10 steps, the momentum negated, 10
    more steps return to the start.  Bound: 4 x the restatement's own fp32 CPU round trip (MEASURED_FP32["reverse_q"] = 1.79e-07 of max |q|)."""
    from robustbnns_amd.hmc import HmcSampler
    arch, act, D, H, Cn, B, L, _ = HR.REVERSE_CASE
    c = HR.leap_case(*HR.REVERSE_CASE)
    s = HmcSampler(arch, act, (1, D, 1), Cn, c["q0"], c["eps"], L, DEV, HR.LEAP_KEY, batch_size=B)
    s.m_inv.copy_(c["m_inv"])
    s.stage(c["x"].to(DEV), c["lab"].to(DEV))
    start = s.q_cur.clone()
    s._momentum(HR.LEAP_KEY, 0)
    r0 = s.r.clone()
    s.leapfrog(L)
    s._commit(force=True)                                                        # the end point becomes the chain's position and gradient
    there = _relmax(s.q_cur.cpu().numpy(), start.cpu().numpy())
    s.r.neg_()
    s.leapfrog(L)
    torch.cuda.synchronize()
    back, rback = _relmax(s.W.cpu().numpy(), start.cpu().numpy()), _relmax((-s.r).cpu().numpy(), r0.cpu().numpy())
    print(f"out {there:.2e} of max |q|; back {back:.2e} ({back / BOUND['reverse_q']:.2f} x bound)  momentum {rback:.2e}")
    assert there > 1000 * BOUND["reverse_q"], "the trajectory did not move"
    assert back <= BOUND["reverse_q"]


# ---- c. stationarity under a non-unit mass --------------------------------------------------------------------------------------------
def test_a_stationary_start_stays_standard_normal_under_a_non_unit_mass():
    """16 chains in lockstep on the one-class fc net, each started at an exact N(0, I) draw, the hand-set m_inv of (a), no adaptation, eps 0.25,
    L 6, 200 samples: the start is stationary, so every sample is N(0, I) whatever the mass — IF the momentum is drawn as N(0, 1 / m_inv).
    Conditions: pooled mean of q^2 within 0.03 of 1, pooled mean of q within 0.03 of 0 (16 x 200 x 65 values).
    The fp64 restatement on these keys and starts (CPU): mean q^2 0.9972, mean q -0.0047 (both within 0.015); with its momentum mutated to
    eps_n sqrt(m_inv) the same run gives mean q^2 2.4674 — far outside the cap.  The m_inv = 4 coordinates turn by 3.0 rad a transition
    (q -> -q nearly), so their q^2 mixes slowly: over 8 other start seeds the restatement's mean q^2 ranged 0.967 ... 1.023.  The seed is
    fixed, and the kernels follow the restatement's chain; a wrong power of m_inv moves the figure by 1.4."""
    c = HX.one_class_case("fc")
    q0s = HX.stationary_starts(16)
    ls = _one_class_lockstep(q0s, HX.EPS, 6, HX.STATIONARY_KEYS, adapt_step_size=False, adapt_mass_matrix=False)
    ls.m_inv.copy_(c["m_inv"].expand(16, -1))
    ls.run(c["x"].to(DEV), c["lab"].to(DEV), 200, 0)
    S = ls.samples_t[:, :200].cpu().double()
    assert all(L == [6] * 200 for L in ls.L_log) and bool(torch.isfinite(S).all())
    q2, q1 = float(S.square().mean()), float(S.mean())
    acc = float(np.mean([np.mean(a) for a in ls.accept_prob_log]))
    print(f"pooled mean q^2 {q2:.4f}  mean q {q1:+.5f}  mean accept_prob {acc:.3f}")
    assert abs(q2 - 1) <= 0.03 and abs(q1) <= 0.03
    assert torch.equal(ls.m_inv.cpu(), c["m_inv"].expand(16, -1)), "m_inv moved without adaptation"


# ---- d. adaptation does its job -------------------------------------------------------------------------------------------------------
def test_warmup_ends_at_a_step_size_that_samples_the_known_posterior():
    """hmc_exact_cases.ADAPT: 16 chains from Uniform(-2, 2) on the one-class fc net (posterior exactly N(0, I)), step size 0.1, num_steps 10,
    warmup 150, 200 samples.  Every chain's mean accept_prob over the sampling phase must lie in [0.7, 0.98] (dual averaging aims at 0.8),
    the pooled mean q^2 within 0.05 of 1, every m_inv positive and finite.  With the step-size search also run after the LAST warmup window
    (this project before it kept exp(xbar) there) chains sampled at a power-of-two probe result, some past the leapfrog stability limit.
    The fp64 restatement as it is now, on these exact inputs (CPU): accept 0.8668 ... 0.9270 (mean 0.899), step sizes 0.398 ... 0.560, mean q^2
    0.9834, m_inv 0.143 ... 2.49; with the search after the last window put back: accept 9.6e-09 ... 0.968 (mean 0.356), step sizes 0.28 ... 1.88.
    Chain 0 also runs alone: bit equality with the lockstep chain stays asserted."""
    from robustbnns_amd.hmc import HmcSampler
    A = HX.ADAPT
    c = HX.one_class_case("fc")
    q0s = HX.adapt_starts(16)
    x, lab = c["x"].to(DEV), c["lab"].to(DEV)
    ls = _one_class_lockstep(q0s, A["step_size"], A["num_steps"], A["keys"])
    ls.run(x, lab, A["samples"], A["warmup"])
    W = A["warmup"]
    acc = [float(np.mean(a[W:])) for a in ls.accept_prob_log]
    eps = [e[-1] for e in ls.eps_log]
    S = ls.samples_t[:, :A["samples"]].cpu().double()
    q2 = float(S.square().mean())
    print(f"accept_prob over the sampling phase {min(acc):.4f} ... {max(acc):.4f} (mean {np.mean(acc):.4f})  step sizes {min(eps):.3f} ... {max(eps):.3f}"
          f"  pooled mean q^2 {q2:.4f}  searches per chain {sorted(set(len(t) for t in ls.search_log))}")
    assert all(len(t) == 3 for t in ls.search_log), "the search runs before the first transition and after the start and middle windows only"
    assert all(A["accept"][0] <= a <= A["accept"][1] for a in acc), acc
    assert abs(q2 - 1) <= A["q2"]
    assert bool(torch.isfinite(ls.m_inv).all()) and bool((ls.m_inv > 0).all())
    # the sampling phase runs at the last window's exp(xbar): what the state block holds, and constant
    assert all(e[W:] == [e[W]] * A["samples"] for e in ls.eps_log) and eps == [s["eps"] for s in ls.read_state()]
    s = HmcSampler("fc", "tanh", (1, 2, 1), 1, q0s[0], A["step_size"], A["num_steps"], DEV, A["keys"][0], batch_size=8)
    s.run(x, lab, A["samples"], A["warmup"])
    assert torch.equal(ls.samples_t[0, :A["samples"]], s.samples_t[:A["samples"]]) and torch.equal(ls.log[0], s.log)
    assert torch.equal(ls.m_inv[0], s.m_inv) and torch.equal(ls.q_cur[0], s.q_cur) and ls.L_log[0] == s.L_log
    assert ls.search_log[0] == s.search_log and ls.read_state()[0]["eps"] == s.read_state()["eps"]


# ---- e. Welford, directly -------------------------------------------------------------------------------------------------------------
def test_welford_far_from_zero_against_a_two_pass_variance():
    """300 rows q_t = 1000 + 0.01 N(0, 1) in fp32 over the 65 parameters: each is copied into W and committed with welford_n = t, then the window
    ends.  Reference: the fp64 two-pass mean / M2 of those rows and the m_inv formula.  Bound: 4 x the deviation of the same recurrence run in
    fp32 on the CPU (MEASURED_FP32: welford_mean 4.03e-07, welford_m_inv 3.79e-03 of the max — the rows are 1e5 standard deviations from
    zero, so each q - mean carries the rounding of `mean` at 1000).  A slip in the recurrence (d / n with another n, d^2 in place of
    d (q - mean')) is off by percents and more; an fp32 sum of squares is off by 2.7e+03 times M2 here, orders of magnitude."""
    from robustbnns_amd import _hip
    c = HX.one_class_case("fc")
    s = _one_class_sampler("fc", c, 0.1, 1, 1)
    rows = HX.welford_rows(300, s.n_params)
    mean64, m264, minv64 = HX.welford_reference(rows)
    dev_rows = rows.to(DEV)
    for t in range(300):
        s.W.copy_(dev_rows[t])
        s._commit(force=True, welford_n=t + 1)
    em, e2 = _relmax(s.w_mean.cpu().numpy(), mean64), _relmax(s.w_m2.cpu().numpy(), m264)
    assert torch.equal(s.q_cur, dev_rows[299])
    _hip.check(s.k.lib.rbnn_hmc_window_end(C.byref(s.net), C.byref(s.chain), 300, s._st()), "rbnn_hmc_window_end")
    torch.cuda.synchronize()
    ev = _relmax(s.m_inv.cpu().numpy(), minv64)
    print(f"mean {em:.2e} ({em / BOUND['welford_mean']:.2f} x bound)  M2 {e2:.2e}  m_inv {ev:.2e} ({ev / BOUND['welford_m_inv']:.2f} x bound)")
    assert em <= BOUND["welford_mean"] and ev <= BOUND["welford_m_inv"] and e2 <= BOUND["welford_m_inv"] * 1.2   # M2 is m_inv's varying 5/6
    assert bool((s.w_mean == 0).all()) and bool((s.w_m2 == 0).all()), "the window end did not reset Welford's state"


# ---- f. a non-finite trajectory is a rejection ----------------------------------------------------------------------------------------
F_CASE = ("fc2", "tanh", 32, 200, 0.002, 5)          # hmc_restate.TRANSITION_CASES' accepted fc2 case


def _f_single(key):
    from robustbnns_amd.hmc import HmcSampler
    arch, act, H, n, eps, L = F_CASE
    q0, x, lab = HR.transition_case(arch, act, H, n)
    s = HmcSampler(arch, act, (1, 2, 1), 2, q0, eps, L, DEV, key, batch_size=n)
    s.stage(x.to(DEV), lab.to(DEV))
    return s


def _assert_rejected_as_infinite(st):
    assert st["dH"] == math.inf and st["accept_prob"] == 0.0 and st["accepted"] == 0.0, st
    assert math.isfinite(st["eps"]) and st["eps"] > 0, st["eps"]


def test_a_non_finite_trajectory_is_rejected_and_leaves_no_trace():
    """Transition 0 at a step size of 1e30 (K' and 1/2 sum q'^2 overflow, the net's forward sees infinite weights): dH = +inf, accept_prob 0,
    rejected, position / cached gradient / cached U bit for bit as before, and dual averaging (adapt = 1) leaves a finite positive step
    size.  Transition 1 at the sane step size then ends where a sampler that never made the bad transition ends, bit for bit."""
    arch, act, H, n, eps, L = F_CASE
    s = _f_single(22)
    before = (s.q_cur.clone(), s.g_cur.clone(), s.read_state()["U"])
    s._set_state(eps=1e30)
    s.transition(0, L, adapt=True)
    st = s.read_state()
    print(f"bad transition: dH {st['dH']} accept_prob {st['accept_prob']} U' {st['U_new']} K' {st['K_new']} next eps {st['eps']:.4g}")
    _assert_rejected_as_infinite(st)
    assert not math.isfinite(st["U_new"]) and not math.isfinite(st["K_new"])
    assert torch.equal(s.q_cur, before[0]) and torch.equal(s.g_cur, before[1]) and st["U"] == before[2]
    s._set_state(eps=eps)
    s.transition(1, L)
    clean = _f_single(22)
    clean.transition(1, L)
    a, b = s.read_state(), clean.read_state()
    assert b["accepted"] == 1.0 and not torch.equal(clean.q_cur, before[0]), "the sane transition was meant to be accepted"
    assert a["accepted"] == 1.0 and a["dH"] == b["dH"] and a["U"] == b["U"]
    assert torch.equal(s.q_cur, clean.q_cur) and torch.equal(s.g_cur, clean.g_cur)


def test_a_non_finite_trajectory_of_one_lockstep_chain_leaves_the_others_alone():
    """The same for chain 1 of a lockstep trio: chains 0 and 2 are what they are in a trio without the bad step size, bit for bit, and chain 1's
    next transition equals the single chain that never saw it."""
    from robustbnns_amd import _hip
    from robustbnns_amd.hmc import LockstepHmc
    arch, act, H, n, eps, L = F_CASE
    q0, x, lab = HR.transition_case(arch, act, H, n)
    names = ("q_cur", "g_cur", "r", "m_inv", "state", "k0_part", "k1_part", "p_part")

    def trio(bad):
        ls = LockstepHmc(arch, act, (1, 2, 1), 2, [q0] * 3, eps, L, DEV, (21, 22, 23), batch_size=n)
        ls.set_data(x.to(DEV), lab.to(DEV))
        ls.stage()
        start = {k: getattr(ls, k).clone() for k in names}
        if bad:
            ls._set_state(eps=[eps, 1e30, eps])
        ls.transition(0, L, adapt=True)
        return ls, start

    ls, start = trio(True)
    ref, _ = trio(False)
    torch.cuda.synchronize()
    st = ls.read_state()
    _assert_rejected_as_infinite(st[1])
    for k in ("q_cur", "g_cur"):
        assert torch.equal(getattr(ls, k)[1], start[k][1]), f"{k} of the rejected chain changed"
    assert st[1]["U"] == float(start["state"][1, _hip.HMC_ST["U"]]), "the cached U of the rejected chain changed"
    for j in (0, 2):
        for k in names:
            assert torch.equal(getattr(ls, k)[j], getattr(ref, k)[j]), f"chain {j}: {k} differs from the trio without the bad step size"
        assert math.isfinite(st[j]["dH"])
    ls._set_state(eps=eps)
    ls.transition(1, L)
    clean = _f_single(22)
    clean.transition(1, L)
    a, b = ls.read_state()[1], clean.read_state()
    assert b["accepted"] == 1.0 and a["accepted"] == 1.0 and a["dH"] == b["dH"] and a["U"] == b["U"]
    assert torch.equal(ls.q_cur[1], clean.q_cur) and torch.equal(ls.g_cur[1], clean.g_cur)
