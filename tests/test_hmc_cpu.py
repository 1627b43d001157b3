"""CPU tests (-m "not gpu") of HMC (tests/hmc_restate.py, robustbnns_amd/hmc.py): the restatement's own properties — reversibility, the
second-order energy error, the window schedule, dual averaging against a from-the-formula loop, and that a seeded chain samples N(0, I) on
a net whose likelihood is constant —, the guards of HmcSampler / BNN.train_hmc / BNN.train, and the ABI (additive entry points, no scratch)."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import hmc_restate as HR
import svi_restate as R
from robustbnns_amd import _hip, hmc
from robustbnns_amd.grid_search_halfMoons import MoonsBNN, _train
from robustbnns_amd.model_bnn import BNN

pytestmark = pytest.mark.usefixtures("built_library")


def _net(arch, D, H, Cn, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return {k: scale * (torch.rand(*s, generator=g) * 4 - 2) for k, s in R.shapes_of(arch, D, H, Cn).items()}


def _moons(n, seed=3):
    x, y = R.two_moons(n, 0.1, seed)
    return x, y.argmax(-1)


@pytest.mark.parametrize("arch,act", [("fc", "tanh"), ("fc2", "leaky")])
def test_leapfrog_is_reversible(arch, act):
    """L steps, negate r, L steps returns (q, -r) within fp64 round-off."""
    x, lab = _moons(40)
    rs = HR.Restatement(arch, act, _net(arch, 2, 8, 2, 1, 0.5), x, lab, 0.01, 10, key=11)
    r0 = rs.momentum(rs.key, 0)
    q1, r1, g1, _ = rs.leapfrog(rs.q, r0, rs.g, 10)
    q2, r2, _, _ = rs.leapfrog(q1, -r1, g1, 10)
    eq, er = float((q2 - rs.q).abs().max()), float((r2 + r0).abs().max())
    print(f"[{arch} {act}] |q - q0| {eq:.1e}  |r + r0| {er:.1e}")
    assert eq < 1e-12 and er < 1e-11          # ~100 operations of size <= 50 per element at 1.1e-16 each


def test_energy_error_is_second_order():
    """For L eps fixed, |dH(eps)| / |dH(eps / 2)| lies in [3, 5] (a second-order integrator: 4 in the limit).  tanh: a smooth potential."""
    x, lab = _moons(50)
    rs = HR.Restatement("fc", "tanh", _net("fc", 2, 8, 2, 2, 0.5), x, lab, 0.01, 10, key=5)
    r0 = rs.momentum(rs.key, 0)
    dH = []
    for eps, L in ((0.01, 10), (0.005, 20)):
        _, r1, _, U1 = rs.leapfrog(rs.q, r0, rs.g, L, eps)
        dH.append((U1 + rs.kinetic(r1)) - (rs.U + rs.kinetic(r0)))
    ratio = abs(dH[0]) / abs(dH[1])
    print(f"dH(0.01) = {dH[0]:.3e}  dH(0.005) = {dH[1]:.3e}  ratio {ratio:.3f}")
    assert 3.0 <= ratio <= 5.0


@pytest.mark.parametrize("warmup,want", [
    (0, []), (10, [(0, 10, "start")]), (19, [(0, 19, "start")]),
    (20, [(0, 3, "start"), (3, 18, "middle"), (18, 20, "end")]),
    (50, [(0, 7, "start"), (7, 45, "middle"), (45, 50, "end")]),
    (100, [(0, 15, "start"), (15, 90, "middle"), (90, 100, "end")]),
    (150, [(0, 75, "start"), (75, 100, "middle"), (100, 150, "end")]),
    (500, [(0, 75, "start"), (75, 100, "middle"), (100, 150, "middle"), (150, 250, "middle"), (250, 450, "middle"), (450, 500, "end")])])
def test_window_schedule(warmup, want):
    for fn in (HR.windows, hmc.windows):                       # the restatement's and the sampler's
        w = fn(warmup)
        assert w == want, (fn.__module__, w)
        assert [a for a, _, _ in w] == [0] * bool(w) + [b for _, b, _ in w[:-1]] and (not w or w[-1][1] == warmup)     # tiles [0, warmup)


def test_dual_averaging_matches_the_formula():
    rng = np.random.RandomState(0)
    probs = np.clip(rng.beta(4, 1.5, size=60), 0, 1)
    eps0 = 0.03
    st = {"t": 0.0, "gbar": 0.0, "xbar": 0.0, "mu": math.log(10 * eps0)}
    mu, G, xb = np.log(10 * eps0), 0.0, 0.0
    for n, p in enumerate(probs, start=1):
        xx, xbar = HR.dual_averaging_update(st, float(p))
        G = (1 - 1 / (n + 10)) * G + (0.8 - p) / (n + 10)
        x_np = mu - np.sqrt(n) / 0.05 * G
        xb = (1 - n ** -0.75) * xb + n ** -0.75 * x_np
        assert abs(xx - x_np) <= 1e-13 * max(1, abs(x_np)) and abs(xbar - xb) <= 1e-13 * max(1, abs(xb)), n
    assert math.exp(xb) < 10 * eps0          # the sequence's mean is below the target 0.8: the averaged step size went down from exp(mu)


def test_restatement_samples_a_standard_normal_when_the_likelihood_is_constant():
    """One class: CE = 0 for every q, so the target is N(0, I) over the 17 parameters of a 2 -> 4 -> 1 fc net.  eps = 0.1, 16 steps (trajectory
    1.6, about pi / 2: successive positions nearly uncorrelated, cos 1.6 = -0.03), no adaptation, 1500 samples from a Uniform(-2, 2) start.
    Pooled over the 17 x 1500 values: the mean must lie within 4 / sqrt(n) of 0, the variance within 4 sqrt(2 / n) of 1.
    Observed here: mean -0.0007 (0.12 standard errors), variance 0.9918 (0.93 standard errors), acceptance 1.00."""
    torch.manual_seed(0)
    shapes = R.shapes_of("fc", 2, 4, 1)
    q0 = HR.initial_position(shapes)
    x = torch.randn(5, 2)
    rs = HR.Restatement("fc", "tanh", q0, x, torch.zeros(5, dtype=torch.long), 0.1, 16, key=2024, adapt_step_size=False)
    S = rs.run(1500, 0)
    n = S.numel()
    mean, var = float(S.mean()), float(S.var())
    acc = sum(r["accepted"] for r in rs.log) / len(rs.log)
    print(f"mean {mean:+.4f} ({abs(mean) * n ** 0.5:.2f} se)  var {var:.4f} ({abs(var - 1) / (2 / n) ** 0.5:.2f} se)  acceptance {acc:.2f}")
    assert all(r["L"] == 16 for r in rs.log)
    assert abs(mean) <= 4 / n ** 0.5 and abs(var - 1) <= 4 * (2 / n) ** 0.5


@pytest.mark.parametrize("arch", ["fc", "fc2"])
@pytest.mark.parametrize("L", [1, 6, 10])
def test_restatement_leapfrog_matches_the_harmonic_oscillator(arch, L):
    """The one-class net of tests/hmc_exact_cases.py: dCE/dW = 0, so L leapfrog steps under a diagonal mass are the L-th power of a 2 x 2 matrix
    per coordinate (numpy, nothing of the restatement's).  The fp64 restatement must equal it to 1e-12: ~60 operations of size <= 10 an element."""
    import hmc_exact_cases as HX
    c = HX.one_class_case(arch)
    rs = HR.Restatement(arch, "tanh", c["q0"], c["x"], c["lab"], HX.EPS, L, key=1, adapt_step_size=False)
    rs.m_inv = c["m_inv"].double()
    assert float(rs.g.abs().max()) == 0.0 and rs.U == float(0.5 * (rs.q * rs.q).sum())
    q1, r1, K1, P1 = HX.leapfrog_closed_form(rs.q.numpy(), c["r0"].numpy(), c["m_inv"].numpy(), HX.EPS, L)
    q, r, g, U = rs.leapfrog(rs.q, c["r0"].double(), rs.g, L)
    eq, er = float(np.abs(q.numpy() - q1).max()), float(np.abs(r.numpy() - r1).max())
    print(f"[{arch} L {L}] |q - closed form| {eq:.1e}  |r - closed form| {er:.1e}  K' {abs(rs.kinetic(r) - K1):.1e}  U' {abs(U - P1):.1e}")
    assert eq <= 1e-12 and er <= 1e-12 and float(g.abs().max()) == 0.0
    assert abs(rs.kinetic(r) - K1) <= 1e-12 * K1 and abs(U - P1) <= 1e-12 * P1


def test_restatement_warmup_ends_at_a_step_size_that_samples_the_known_posterior():
    """The adaptation condition of tests/test_hip_hmc_exact.py on the fp64 restatement, 4 of its 16 chains: every chain's mean accept_prob over the
    sampling phase in [0.7, 0.98], pooled mean q^2 within 0.05 of 1, m_inv positive and finite, and three searches (none after the last
    window).  Measured here: 0.8894 ... 0.9270, mean q^2 0.9624; with the search after the last window as well the 16 chains ranged from
    9.6e-09 to 0.968."""
    import hmc_exact_cases as HX
    A, c = HX.ADAPT, HX.one_class_case("fc")
    acc, S = [], []
    for q0, key in zip(HX.adapt_starts(4), A["keys"]):
        rs = HR.Restatement("fc", "tanh", q0, c["x"], c["lab"], A["step_size"], A["num_steps"], key)
        S.append(rs.run(A["samples"], A["warmup"]))
        acc.append(float(np.mean([r["accept_prob"] for r in rs.log[A["warmup"]:]])))
        assert len(rs.search_log) == 3 and bool(torch.isfinite(rs.m_inv).all()) and bool((rs.m_inv > 0).all())
        assert rs.log[-1]["eps"] == rs.adapt_log[-1][0] == rs.eps                # sampling runs at the last window's exp(xbar)
    q2 = float(torch.stack(S).square().mean())
    print(f"accept_prob over the sampling phase {min(acc):.4f} ... {max(acc):.4f}  pooled mean q^2 {q2:.4f}")
    assert all(A["accept"][0] <= a <= A["accept"][1] for a in acc), acc
    assert abs(q2 - 1) <= A["q2"]


def test_initial_position_is_uniform_within_the_radius():
    torch.manual_seed(1)
    a = hmc.initial_position(list(R.shapes_of("fc2", 2, 32, 2).items()))
    torch.manual_seed(1)
    b = HR.initial_position(R.shapes_of("fc2", 2, 32, 2))
    v = torch.cat([t.reshape(-1) for t in a.values()])
    assert all(torch.equal(a[k], b[k]) for k in a) and float(v.abs().max()) <= 2 and abs(float(v.mean())) < 0.15 and float(v.std()) > 1.0


def test_guards():
    q0 = _net("fc", 2, 8, 2, 0)
    with pytest.raises(NotImplementedError, match="no CPU compute path"):
        hmc.HmcSampler("fc", "leaky", (1, 2, 1), 2, q0, 0.01, 10, "cpu", 1)
    with pytest.raises(NotImplementedError, match="conv"):
        hmc.HmcSampler("conv", "leaky", (1, 28, 28), 10, q0, 0.01, 10, "cuda:0", 1)
    x, y = R.two_moons(16, 0.1, 0)
    loader = torch.utils.data.DataLoader(list(zip(x, y)), batch_size=8)
    svi = MoonsBNN(16, "leaky", "fc", "svi", 1, 0.01, None, None, 16, (1, 2, 1), 2)
    with pytest.raises(ValueError, match="train_hmc"):
        svi.train_hmc(loader, "cuda:0", "out/")
    net = MoonsBNN(16, "leaky", "fc", "hmc", None, None, 5, 5, 16, (1, 2, 1), 2)
    with pytest.raises(NotImplementedError, match="train_hmc"):            # train() keeps refusing HMC, and names the new method
        net.train(loader, "cuda:0", "out/")
    with pytest.raises(NotImplementedError, match="no CPU compute path"):
        net.train_hmc(loader, "cpu", "out/")
    with pytest.raises(NotImplementedError, match="conv"):
        BNN("mnist", 16, "leaky", "conv", "hmc", None, None, 5, 5, (1, 28, 28), 10).train_hmc(loader, "cuda:0", "out/")
    with pytest.raises(NotImplementedError, match="conv"):
        _train(16, "leaky", "conv", "hmc", None, None, 5, 5, 16, 1, "out/", "cuda:0", x_train=x, y_train=y)
    assert not os.path.exists("out")                                         # a refusal writes nothing


def test_hmc_entry_points_are_additive_and_validate_without_a_gpu():
    import ctypes as C
    names = {"rbnn_hmc_sizes", "rbnn_hmc_momentum", "rbnn_hmc_leapfrog_update", "rbnn_hmc_decide", "rbnn_hmc_commit", "rbnn_hmc_window_end"}
    assert names <= set(_hip.SIGNATURES) and _hip.ABI_VERSION == 10
    hdr = open(_hip.HEADER_PATH).read()
    for name, i in _hip.HMC_ST.items():                                      # the state block's indices as the header declares them
        assert re.search(r"RBNN_HMC_ST_\w+ = %d\b" % i, hdr), name
    assert f"RBNN_HMC_STATE {_hip.HMC_STATE}" in hdr and f"RBNN_HMC_LOG {_hip.HMC_LOG}" in hdr
    assert f"0x{_hip.HMC_UNIF_KEY:016X}ull" in hdr and f"0x{_hip.HMC_SEARCH_KEY:016X}ull" in hdr
    assert (HR.UNIF_KEY, HR.SEARCH_KEY) == (_hip.HMC_UNIF_KEY, _hip.HMC_SEARCH_KEY)
    lib = _hip.load()
    net = _hip.SviTrainNet()
    net.arch, net.activation, net.in_features, net.hidden, net.n_classes = 1, 1, 2, 32, 2
    nq, ne = C.c_int64(0), C.c_int64(0)
    n = 2 * 32 + 32 + 32 * 32 + 32 + 2 * 32 + 2
    assert lib.rbnn_hmc_sizes(C.byref(net), C.byref(nq), C.byref(ne)) == n
    assert ne.value == -(-n // 256) and nq.value == -(-(32 + 8 + 32 * 8 + 8 + 2 * 8 + 1) // 256)
    net.n_classes = 17
    assert lib.rbnn_hmc_sizes(C.byref(net), None, None) < 0
    net.n_classes = 2
    ch = _hip.HmcChain()                                                      # every pointer NULL: refused before any launch
    assert lib.rbnn_hmc_momentum(C.byref(net), C.byref(ch), 1, 0, None) == -1
    assert lib.rbnn_hmc_leapfrog_update(C.byref(net), C.byref(ch), 0, None) == -1
    assert lib.rbnn_hmc_commit(C.byref(net), C.byref(ch), 0, 0, -1, None) == -1
    assert lib.rbnn_hmc_window_end(C.byref(net), C.byref(ch), 25, None) == -1
    assert lib.rbnn_hmc_decide(C.byref(net), C.byref(ch), None, 4, 1, 0, 2, 0, 0, None) == -1
    assert lib.rbnn_hmc_momentum(None, C.byref(ch), 1, 0, None) == -1


def test_hmc_kernels_use_no_scratch():
    """Every kernel of csrc/rbnn_hmc.hip holds everything in registers (read from the code objects of the built library: no GPU)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources as KR
    if not os.path.exists(KR.READELF):
        pytest.skip("llvm-readelf not in this image")
    res = {n: r for n, r in KR.kernel_resources().items() if re.search(r"hmc_\w+_kernel", n)}
    assert len(res) == 5, sorted(res)
    bad = {n: (r["scratch"], r["spill_vgpr"]) for n, r in res.items() if r["scratch"] or r["spill_vgpr"]}
    assert not bad, bad
