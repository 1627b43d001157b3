"""GPU tests (-m gpu) of HMC (csrc/rbnn_hmc.hip, robustbnns_amd/hmc.py, BNN.train_hmc): every comparison is against tests/hmc_restate.py in
fp64, within hmc_restate.BOUND (4 x the deviation of the restatement's own fp32 run on the CPU, see there).  Leapfrog (fused against plain
and against fp64), single transitions (accepted and rejected), full runs with warmup on half-moons (every decision, every L), bit-identical
reruns, no device->host sync while sampling, the launch count of a step, BNN.train_hmc end to end, and what the kernels must not touch."""
import glob
import math
import os

import pytest
import torch
from torch.utils.data import DataLoader

import hmc_restate as HR
import svi_restate as R
from hmc_restate import BOUND

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("built_library")]
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"


def _sampler(arch, act, D, Cn, q0, eps, steps, key, B, **kw):
    from robustbnns_amd.hmc import HmcSampler
    return HmcSampler(arch, act, (1, D, 1), Cn, q0, eps, steps, DEV, key, batch_size=B, **kw)


@pytest.mark.parametrize("case", HR.LEAP_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_leapfrog_fused_equals_plain_and_fp64(case):
    """relu / leaky cases: the points of the batch within hmc_restate.KINK of a relu crossing somewhere on the fp64 trajectory are taken out by
    hmc_restate.leap_case (the gradient of U jumps there); at most 5 % of the batch over the L + 1 positions of a trajectory (the SVI gradient
    tests allow 1 % at their one position; see leap_case), printed.  The fused updates must equal the plain sequence BIT FOR BIT."""
    arch, act, D, H, Cn, B, L, unit = case
    c = HR.leap_case(*case)
    assert c["dropped"] <= 0.05 * B, c["dropped"]
    rs = HR.Restatement(arch, act, c["q0"], c["x"], c["lab"], c["eps"], L, HR.LEAP_KEY)
    rs.m_inv = c["m_inv"].double()
    r0 = rs.momentum(HR.LEAP_KEY, 0)
    q64, r64, g64, U64 = rs.leapfrog(rs.q, r0, rs.g, L)
    s = _sampler(arch, act, D, Cn, c["q0"], c["eps"], L, HR.LEAP_KEY, 2)           # batch_size 2: the workspaces grow
    s.m_inv.copy_(c["m_inv"])
    s.stage(c["x"].to(DEV), c["lab"].to(DEV))
    # the momentum draw against the oracle's generator: three libm calls at <= 2 ulp and three roundings per element, < 1e-6 of max |r|
    s._momentum(HR.LEAP_KEY, 0)
    em = HR.relmax(s.r.cpu(), r0)
    s.r.copy_(r0.float())
    s.leapfrog(L)
    qf, rf, gf = s.W.clone(), s.r.clone(), s.grad.clone()
    kf, pf = s.k1_part.clone(), s.p_part.clone()
    s.r.copy_(r0.float())
    s.leapfrog(L, fused=False)
    torch.cuda.synchronize()
    eq, er = HR.relmax(qf.cpu(), q64), HR.relmax(rf.cpu(), r64)
    pq, pr = HR.relmax(s.W.cpu(), qf.cpu()), HR.relmax(s.r.cpu(), rf.cpu())
    same = torch.equal(s.W, qf) and torch.equal(s.r, rf) and torch.equal(s.grad, gf) and torch.equal(s.k1_part, kf) and torch.equal(s.p_part, pf)
    print(f"[{case}] points taken out {c['dropped']}  momentum {em:.1e}  q {eq:.2e} ({eq / BOUND['leapfrog_q']:.2f} x bound)  r {er:.2e} ({er / BOUND['leapfrog_r']:.2f} x bound)"
          f"  fused vs plain: q {pq:.1e} r {pr:.1e} bit-identical {same}")
    assert em < 1e-6
    assert same and pq == 0.0 and pr == 0.0, "the fused leapfrog updates differ from the plain kick / drift / kick sequence"
    assert eq <= BOUND["leapfrog_q"] and er <= BOUND["leapfrog_r"]


@pytest.mark.parametrize("case", HR.TRANSITION_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_transition_matches_fp64(case):
    name, arch, act, H, n, eps, L, key = case
    q0, x, lab = HR.transition_case(arch, act, H, n)
    rs = HR.Restatement(arch, act, q0, x, lab, eps, L, key, adapt_step_size=False)
    U0 = rs.U
    rec = rs.transition(0)
    assert rec["accepted"] == (name == "accept")
    s = _sampler(arch, act, 2, 2, q0, eps, L, key, n, adapt_step_size=False)
    s.stage(x.to(DEV), lab.to(DEV))
    before = (s.q_cur.clone(), s.g_cur.clone(), s.read_state()["U"])
    s.transition(0, L)
    st = s.read_state()
    scale = HR.energy_scale(rec)
    eU0, eU, eK = abs(before[2] - U0) / abs(U0), abs(st["U_new"] - rec["U_new"]) / abs(rec["U_new"]), max(
        abs(st["K_new"] - rec["K_new"]) / rec["K_new"], abs(st["K_old"] - rec["K_old"]) / rec["K_old"])
    eH, eA = abs(st["dH"] - rec["dH"]) / scale, abs(st["accept_prob"] - rec["accept_prob"])
    print(f"[{name} {arch}] U0 {eU0:.1e} U' {eU:.1e} ({eU / BOUND['U']:.2f} x bound)  K {eK:.1e} ({eK / BOUND['K']:.2f} x)  dH {st['dH']:.4e} vs {rec['dH']:.4e}:"
          f" {eH:.1e} of the scale {scale:.0f} ({eH / BOUND['dH']:.2f} x)  accept_prob {eA:.1e}  u {st['u']} accepted {st['accepted']}")
    assert st["u"] == rec["u"]                                        # the uniform is exact: x0 2^-32 in fp64
    assert eU0 <= BOUND["U"] and eU <= BOUND["U"] and eK <= BOUND["K"] and eH <= BOUND["dH"]
    assert eA <= BOUND["dH"] * scale                                  # |d min(1, e^-x)| <= |dx|
    assert bool(st["accepted"]) == rec["accepted"]
    if rec["accepted"]:
        assert HR.relmax(s.q_cur.cpu(), rec["q_end"]) <= BOUND["leapfrog_q"] and st["U"] == st["U_new"]
    else:                                                             # position, cached gradient and cached U: bit for bit as before
        assert torch.equal(s.q_cur, before[0]) and torch.equal(s.g_cur, before[1]) and st["U"] == before[2]


RUN_KEYS = {c[:3]: c[8] for c in HR.RUN_CASES}


@pytest.mark.parametrize("case", HR.RUN_CASES, ids=lambda c: f"{c[0]}-{c[2]}")
def test_full_run_on_half_moons(case):
    """Warmup 24 (windows [0, 3) start, [3, 22) middle, [22, 24) end: all three kinds) + 20 samples.  The case's key is one for which the fp64
    restatement's own margins hold at EVERY transition (asserted first); no transition is excluded."""
    arch, act, H, n, eps, steps, warmup, samples, key, seed = case
    assert [k for _, _, k in HR.windows(warmup)] == ["start", "middle", "end"] and samples >= 20
    rs, S64 = HR._run(case, key, torch.float64)
    m, sm, f = HR.run_margins_ok(rs, BOUND)
    print(f"[{arch}-{H} key {key}] fp64 margins in units of their bar: decision {m:.2f}  search {sm:.2f}  L {f:.2f}")
    assert min(m, sm, f) > 1
    q0, x, lab = HR.run_case(arch, act, H, n, seed)
    s = _sampler(arch, act, 2, 2, q0, eps, steps, key, n)
    stack = s.run(x.to(DEV), lab.to(DEV), samples, warmup)
    S = torch.cat([stack[k].reshape(samples, -1) for k in s.keys], 1).cpu()
    assert s.accepted_log == [r["accepted"] for r in rs.log], "a decision differs"
    assert s.L_log == [r["L"] for r in rs.log], "an L differs"
    assert [len(t) for t in s.search_log] == [len(t) for t in rs.search_log], "a step-size search took another number of tries"
    assert all(abs(a[0] - b[0]) <= BOUND["eps"] * b[0] for ta, tb in zip(s.search_log, rs.search_log) for a, b in zip(ta, tb))
    ee = max(abs(a - r["eps"]) / r["eps"] for a, r in zip(s.eps_log, rs.log))
    eh = max(abs(a - r["dH"]) / HR.energy_scale(r) for a, r in zip(s.dH_log, rs.log) if math.isfinite(r["dH"]))
    em, es = HR.relmax(s.m_inv.cpu(), rs.m_inv), HR.relmax(S, S64)
    print(f"   eps {ee:.1e} ({ee / BOUND['eps']:.2f} x bound)  m_inv {em:.1e} ({em / BOUND['m_inv']:.2f} x)  samples {es:.1e} ({es / BOUND['samples']:.2f} x)"
          f"  dH {eh:.1e} of the scale ({eh / BOUND['dH']:.2f} x)  L {sorted(set(s.L_log))}  accepted {sum(s.accepted_log)}/{len(s.accepted_log)}")
    # dH is held to its bound in the single-transition test; along a chain the positions drift apart within THEIR bound and dH with them: printed only
    assert ee <= BOUND["eps"] and em <= BOUND["m_inv"] and es <= BOUND["samples"]


def _short_run(key, sync_check=False):
    q0, x, lab = HR.run_case("fc2", "leaky", 32, 128, 5)
    s = _sampler("fc2", "leaky", 2, 2, q0, 0.01, 10, key, 128)
    stack = s.run(x.to(DEV), lab.to(DEV), 6, 20)
    return s, torch.cat([stack[k].reshape(6, -1) for k in s.keys], 1).clone()


def test_rerun_is_bit_identical_and_the_key_matters():
    a, Sa = _short_run(77)
    b, Sb = _short_run(77)
    c, Sc = _short_run(78)
    assert torch.equal(Sa, Sb) and torch.equal(a.log, b.log) and torch.equal(a.m_inv, b.m_inv)
    assert not torch.equal(Sa, Sc)


def test_sampling_makes_no_device_to_host_sync():
    s, _ = _short_run(5)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        s.sample(26, 6)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(s.samples_t).all())


@pytest.mark.parametrize("arch,fwd", [("fc", 2), ("fc2", 4)])
def test_launches_per_leapfrog_step(arch, fwd):
    """A step is the training forward (fc 2 launches, fc2 4: rbnn_svi_train_forward's documented count), the weight gradients (1) and ONE
    fused update; a trajectory adds the opening update, a transition the momentum draw, the decision and the commit."""
    q0, x, lab = HR.transition_case(arch, "leaky", 32, 64)
    s = _sampler(arch, "leaky", 2, 2, q0, 0.001, 10, 3, 64, adapt_step_size=False)
    s.stage(x.to(DEV), lab.to(DEV))
    n0 = s.launches
    s.leapfrog(7)
    assert s.launches - n0 == 1 + 7 * (fwd + 1 + 1)
    n0 = s.launches
    s.transition(0, 5)
    assert s.launches - n0 == 3 + 1 + 5 * (fwd + 1 + 1)


def test_nothing_behind_the_bounds_is_read_or_written():
    """Every buffer of the chain is a view into a NaN-poisoned slab with a guard zone behind it: a transition with Welford, a window end and a
    sample row leave every guard zone NaN (nothing written) and every result finite (nothing read)."""
    import ctypes as C
    from robustbnns_amd import _hip
    q0, x, lab = HR.transition_case("fc2", "tanh", 96, 37)
    s = _sampler("fc2", "tanh", 2, 2, q0, 0.002, 5, 9, 37, adapt_step_size=False)
    G = 512
    slabs = {}

    def guarded(t, fill=None):
        slab = torch.full((t.numel() + G,), float("nan"), dtype=t.dtype, device=DEV)
        slab[:t.numel()].copy_(t.reshape(-1))
        slabs[len(slabs)] = (slab, t.numel())
        return slab[:t.numel()].view(t.shape)

    for name in ("W", "grad", "q_cur", "g_cur", "r", "m_inv", "w_mean", "w_m2", "k0_part", "k1_part", "p_part", "state"):
        setattr(s, name, guarded(getattr(s, name)))
    s.net.W, s.net.grad = s.W.data_ptr(), s.grad.data_ptr()
    s.log_t = guarded(torch.zeros(2, _hip.HMC_LOG, dtype=torch.float64, device=DEV))
    s.samples_t = guarded(torch.zeros(2, s.n_params, device=DEV))
    s._bind()
    s._ensure(37)
    for k in list(s.ws_t):
        s.ws_t[k] = guarded(s.ws_t[k])
    s.X, s.labels = guarded(s.X), s.labels
    ws = _hip.SviTrainWs()
    for k in _hip.SVI_TRAIN_WS_KEYS:
        setattr(ws, k, _hip.ptr(s.ws_t.get(k)))
    s.ws = ws
    s.stage(x.to(DEV), lab.to(DEV))
    s.transition(0, 3, False, False, 1, 0)
    s.transition(1, 3, False, False, 2, 1)
    _hip.check(s.k.lib.rbnn_hmc_window_end(C.byref(s.net), C.byref(s.chain), 2, s._st()), "rbnn_hmc_window_end")
    assert s.k.lib.rbnn_hmc_commit(C.byref(s.net), C.byref(s.chain), 0, 0, 2, s._st()) != 0        # a row behind the stack is refused
    torch.cuda.synchronize()
    for i, (slab, n) in slabs.items():
        assert bool(torch.isnan(slab[n:]).all()), f"buffer {i}: its guard zone was written"
    for name in ("q_cur", "g_cur", "r", "m_inv", "samples_t", "log_t"):
        assert bool(torch.isfinite(getattr(s, name)).all()), name
    assert bool(torch.isfinite(s.state[:13]).all()) and bool((s.m_inv > 0).all())


def test_train_hmc_predictions_match_the_fp64_replay(tmp_path):
    """BNN.train_hmc against hmc_restate.replay_train_hmc, which replays its draws from the CPU generator (the loader's iterator, the initial
    position, the key, the resampling indices) and runs the chain of the last batch in fp64.  The data seed (hmc_restate.E2E) is one at which
    the replay's margins hold at every transition (asserted first, with the decision margin taken in dH: the chain starts at Uniform(-2, 2),
    where some trajectories diverge and are rejected at dH of 1e5 and more).  Held-out points whose fp64 top-2 gap is within twice the
    prediction bar (hmc_restate.e2e_prediction_bar) are left out; their share is printed and must be at most 1 %."""
    from robustbnns_amd.grid_search_halfMoons import MoonsBNN
    E = HR.E2E
    x, y, xt, yt = HR.e2e_case(E["data_seed"])
    r64, S64, p64, key = HR.e2e_replay(E["data_seed"])
    _, _, p32, _ = HR.e2e_replay(E["data_seed"], torch.float32)
    m = HR.run_margins_ok(r64, BOUND, in_dH=True)
    bar = HR.e2e_prediction_bar(p32, p64)
    compared = R.top2_gap(p64) > 2 * bar
    share = 1.0 - float(compared.float().mean())
    print(f"[data seed {E['data_seed']} key {key:#x}] fp64 margins in units of their bar: decision {m[0]:.2f} search {m[1]:.2f} L {m[2]:.2f};"
          f"  prediction bar {bar:.2e}, excluded share {share:.3f}")
    assert min(m) > 1 and share <= 0.01
    net = MoonsBNN(E["hidden"], "leaky", "fc2", "hmc", None, None, E["n_samples"], E["warmup"], E["n_inputs"], (1, 2, 1), 2)
    net.train_hmc(DataLoader(list(zip(x, y)), batch_size=1024, shuffle=False), DEV, rel_path=str(tmp_path) + "/")
    h = net.hmc_history
    assert h["key"] == key, "train_hmc drew another key than the replay"
    assert h["accepted"] == [r["accepted"] for r in r64.log] and h["L"] == [r["L"] for r in r64.log]
    p = net.forward(xt.to(DEV), n_samples=E["n_samples"]).cpu().double()
    dev = float((p - p64).abs().max())
    wrong = int((p.argmax(-1) != p64.argmax(-1))[compared].sum())
    print(f"   max |p - fp64| {dev:.2e} ({dev / bar:.2f} x the prediction bar)  differing predictions among the compared {int(compared.sum())} points: {wrong}")
    assert wrong == 0


def test_train_hmc_end_to_end(tmp_path):
    """MoonsBNN.train_hmc -> n_samples files -> a fresh MoonsBNN.load: forward is bit-identical; then serial_train over a 2 x 1 grid and the
    existing serial_compute_grads on what it wrote."""
    from robustbnns_amd.grid_search_halfMoons import MoonsBNN, serial_compute_grads, serial_train
    x, y = R.two_moons(256, 0.1, 7)
    xt, yt = R.two_moons(64, 0.1, 8)
    loader = DataLoader(list(zip(x, y)), batch_size=1024, shuffle=False)
    path = str(tmp_path) + "/"
    args = (32, "leaky", "fc2", "hmc", None, None, 20, 24, 256, (1, 2, 1), 2)
    net = MoonsBNN(*args)
    net.train_hmc(loader, DEV, rel_path=path)
    files = glob.glob(os.path.join(path, net.name, "*.pt"))
    assert len(files) == 20
    h = net.hmc_history
    assert len(h["eps"]) == len(h["L"]) == len(h["accepted"]) == 24 + 21 and 0 < sum(h["accepted"][24:]) and bool((h["m_inv"] > 0).all())
    again = MoonsBNN(*args)
    again.load(DEV, rel_path=path)
    p0, p1 = net.forward(xt.to(DEV), n_samples=20), again.forward(xt.to(DEV), n_samples=20)
    assert torch.equal(p0, p1) and bool(torch.isfinite(p0).all())
    acc = float((p0.argmax(-1).cpu() == yt.argmax(-1)).float().mean())
    print(f"held-out accuracy of the 20-sample chain after 24 warmup transitions: {acc:.2f}; acceptance {sum(h['accepted'][24:])}/21")
    # the same chain a second time: train_hmc seeds itself, so the files are reproduced bit for bit
    twice = MoonsBNN(*args)
    twice.train_hmc(loader, DEV, rel_path=str(tmp_path) + "/b/")
    assert torch.equal(twice.forward(xt.to(DEV), n_samples=20), p0)
    grid = ([32, 64], ["leaky"], ["fc2"], ["hmc"], [None], [None], [10], [20], [256], [5])
    nets = serial_train(*grid, path, x_train=x, y_train=y, device=DEV)
    assert len(nets) == 2
    out = serial_compute_grads(*grid, path, xt, yt, device=DEV)
    assert len(out) == 2 and all(v.shape[0] == 64 for v in out.values())
