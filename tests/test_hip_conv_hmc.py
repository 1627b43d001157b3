"""GPU tests (-m gpu) of HMC over conv nets (the rbnn_conv_hmc_* entry points of csrc/rbnn_hmc.hip, robustbnns_amd/conv_hmc.py,
BNN.train_hmc_conv) against tests/conv_hmc_restate.py in fp64, within conv_hmc_restate.BOUND (4 x the deviation of the restatement's own fp32
run on the CPU).  The gradient against the conv SVI trainer's bit for bit, the momentum draw, leapfrog (fused against plain, and against fp64
on tie-free batches), an accepted and a rejected transition, a short full run held to what is exact or continuous across pooling ties,
bit-identical reruns, no device->host sync while sampling, the launch count of a step, canaries behind every buffer, BNN.train_hmc_conv end
to end.  Every check prints its worst figure in units of its bar."""
import glob
import math
import os

import pytest
import torch
from torch.utils.data import DataLoader

import conv_hmc_restate as M
import conv_svi_restate as V
import hmc_restate as HR
from conv_hmc_restate import BOUND

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("built_library")]
DEV = "cuda:0"
FORWARD_BAR = HR.FORWARD_BAR


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu() if t.dtype == torch.float32 else t.detach().cpu().clone()


def _sampler(act, Cn, q0, eps, steps, key, B, **kw):
    from robustbnns_amd.conv_hmc import ConvHmcSampler
    return ConvHmcSampler(act, (1, 28, 28), Cn, q0, eps, steps, DEV, key, batch_size=B, **kw)


@pytest.mark.parametrize("Hc,act,B,Cn", [V.GRAD_CASES[0], V.GRAD_CASES[3]])
def test_gradient_is_the_conv_svi_trainers_bit_for_bit(Hc, act, B, Cn):
    """The position set to a ConvSviTrainer's drawn W on the same batch: grad and ce are that trainer's, bit for bit (the same two entry
    points on the same buffers' contents)."""
    from robustbnns_amd.conv_svi_train import ConvSviTrainer
    c = V.grad_case(Hc, act, B, Cn)
    tr = ConvSviTrainer(act, (1, 28, 28), Cn, c["loc"], c["raw"], 0.01, DEV, V.GRAD_KEY, batch_size=B)
    tr.t = V.GRAD_DRAW
    x, lab = c["x"].to(DEV), c["lab"].to(DEV)
    tr.gradients(x, lab)
    s = _sampler(act, Cn, c["loc"], 1e-3, 2, 1, max(1, B // 2), adapt_step_size=False)        # smaller than B: the workspaces grow
    s.stage(x, lab)
    s.W.copy_(tr.W)
    s._gradient()
    torch.cuda.synchronize()
    assert s.n_params == tr.n_params and s.keys == tr.keys
    assert torch.equal(s.grad, tr.grad) and torch.equal(s.ws_t["ce"][:B], tr.ws_t["ce"][:B])
    assert float(s.grad.abs().max()) > 0 and bool(torch.isfinite(s.grad).all())
    print(f"[conv-hmc gradient Hc={Hc} {act} B={B} C={Cn}] grad [{s.n_params}] and ce [{B}] bit-identical to ConvSviTrainer's; excluded: nothing")


@pytest.mark.parametrize("unit", [True, False], ids=["unit-mass", "hand-set-mass"])
def test_momentum_draw_matches_the_restatement(unit):
    """r = eps_n / sqrt(m_inv) with the oracle's eps in the conv counter layout, C = 3 (the last tensor a partial quad): within 1e-6 of
    max |r| (three libm calls at <= 2 ulp and three roundings an element: the fc test's bar); K = 1/2 sum m_inv r^2 from k0_part within 1e-6."""
    Hc, act, B, Cn, L, eps = M.LEAP_CASES[1]
    c = M.choose_batch(Hc, act, B, Cn, L, eps)
    rs = M.Restatement(act, c["q0"], c["x"], c["lab"], eps, L, M.LEAP_KEY)
    s = _sampler(act, Cn, c["q0"], eps, L, M.LEAP_KEY, B, adapt_step_size=False)
    if not unit:
        m_inv = 0.25 + 4 * torch.rand(rs.q.numel(), generator=torch.Generator().manual_seed(3))
        m_inv[::7] = 1e-3
        rs.m_inv = m_inv.double()
        s.m_inv.copy_(m_inv)
    worst = 0.0
    for key, draw in ((M.LEAP_KEY, 0), (M.LEAP_KEY ^ HR.SEARCH_KEY, 5)):
        r64 = rs.momentum(key, draw)
        s._momentum(key, draw)
        torch.cuda.synchronize()
        em = HR.relmax(s.r.cpu(), r64)
        ek = abs(float(s.k0_part.double().sum()) - rs.kinetic(r64)) / rs.kinetic(r64)
        worst = max(worst, em)
        assert em < 1e-6 and ek < 1e-6, (em, ek)
    print(f"[conv-hmc momentum {'unit' if unit else 'hand-set'} m_inv] worst {worst:.2e} of max |r| (bar 1e-6)")


@pytest.mark.parametrize("case", M.LEAP_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_leapfrog_fused_equals_plain_and_fp64(case):
    """On the tie-free batch conv_hmc_restate.choose_batch took for the case (tests/test_conv_hmc_cpu.py holds the selection to its
    conditions): the fused updates equal the plain kick / drift / gradient / kick sequence BIT FOR BIT, and the end point is the fp64
    restatement's within leapfrog_q / leapfrog_r."""
    Hc, act, B, Cn, L, eps = case
    c = M.choose_batch(*case)
    assert c["clean"]
    q64, r64, _, _ = c["end"]
    s = _sampler(act, Cn, c["q0"], eps, L, M.LEAP_KEY, max(1, B // 2), adapt_step_size=False)
    s.stage(c["x"].to(DEV), c["lab"].to(DEV))
    s.r.copy_(c["r0"].float())
    s.leapfrog(L)
    qf, rf, gf, kf, pf = (t.clone() for t in (s.W, s.r, s.grad, s.k1_part, s.p_part))
    s.r.copy_(c["r0"].float())
    s.leapfrog(L, fused=False)
    torch.cuda.synchronize()
    eq, er = HR.relmax(qf.cpu(), q64), HR.relmax(rf.cpu(), r64)
    same = all(torch.equal(a, b) for a, b in ((s.W, qf), (s.r, rf), (s.grad, gf), (s.k1_part, kf), (s.p_part, pf)))
    print(f"[conv-hmc leapfrog {case}] dropped {c['dropped']} / {c['pool']} in {c['rounds']} rounds  q {eq:.2e} ({eq / BOUND['leapfrog_q']:.2f} x bound)"
          f"  r {er:.2e} ({er / BOUND['leapfrog_r']:.2f} x bound)  fused vs plain bit-identical {same}")
    assert same, "the fused leapfrog updates differ from the plain kick / drift / kick sequence"
    assert eq <= BOUND["leapfrog_q"] and er <= BOUND["leapfrog_r"]


@pytest.mark.parametrize("case", M.TRANSITION_CASES, ids=lambda c: c[0])
def test_transition_matches_fp64(case):
    name, Hc, act, B, Cn, L, eps, key = case
    c, U0, rec = M.transition_case(*case)
    assert rec["accepted"] == (name == "accept")
    s = _sampler(act, Cn, c["q0"], eps, L, key, B, adapt_step_size=False)
    s.stage(c["x"].to(DEV), c["lab"].to(DEV))
    before = (s.q_cur.clone(), s.g_cur.clone(), s.read_state()["U"])
    s.transition(0, L)
    st = s.read_state()
    scale = HR.energy_scale(rec)
    eU0, eU = abs(before[2] - U0) / abs(U0), abs(st["U_new"] - rec["U_new"]) / abs(rec["U_new"])
    eK = max(abs(st["K_new"] - rec["K_new"]) / rec["K_new"], abs(st["K_old"] - rec["K_old"]) / rec["K_old"])
    eH, eA = abs(st["dH"] - rec["dH"]) / scale, abs(st["accept_prob"] - rec["accept_prob"])
    print(f"[conv-hmc {name}] U0 {eU0:.1e} U' {eU:.1e} ({eU / BOUND['U']:.2f} x bound)  K {eK:.1e} ({eK / BOUND['K']:.2f} x)  dH {st['dH']:.4e} vs "
          f"{rec['dH']:.4e}: {eH:.1e} of the scale {scale:.0f} ({eH / BOUND['dH']:.2f} x)  accept_prob {eA:.1e}  u {st['u']} accepted {st['accepted']}")
    assert st["u"] == rec["u"]                                        # the uniform is exact: x0 2^-32 in fp64
    assert eU0 <= BOUND["U"] and eU <= BOUND["U"] and eK <= BOUND["K"] and eH <= BOUND["dH"]
    assert eA <= BOUND["dH"] * scale                                  # |d min(1, e^-x)| <= |dx|
    assert bool(st["accepted"]) == rec["accepted"]
    if rec["accepted"]:
        assert HR.relmax(s.q_cur.cpu(), rec["q_end"]) <= BOUND["leapfrog_q"] and st["U"] == st["U_new"]
    else:                                                             # position, cached gradient and cached U: bit for bit as before
        assert torch.equal(s.q_cur, before[0]) and torch.equal(s.g_cur, before[1]) and st["U"] == before[2]


_RUNS = {}


def _short_run(key, tag=0):
    """The short full run of conv_hmc_restate.RUN under `key` (computed once per (key, tag)): (sampler, stack [samples, n_params])."""
    if (key, tag) not in _RUNS:
        R = M.RUN
        q0, x, lab = M.run_inputs()
        s = _sampler(R["act"], R["C"], q0, R["eps"], R["steps"], key, R["B"])
        stack = s.run(x.to(DEV), lab.to(DEV), R["samples"], R["warmup"])
        _RUNS[(key, tag)] = (s, torch.cat([stack[k].reshape(R["samples"], -1) for k in s.keys], 1).clone())
    return _RUNS[(key, tag)]


def test_short_full_run_keeps_what_is_exact_or_continuous():
    """Warmup 24 (windows [0, 3) start, [3, 22) middle, [22, 24) end: all three kinds) + 6 samples.  Over 30 transitions no batch is tie-free,
    so no trajectory is compared with fp64; the run is held to what does not depend on which side of a tie fp32 falls: the decisions follow
    from the logged figures, the lengths from the logged step sizes, and U — continuous across ties and kinks — logged by the transition
    that produced a stored sample (every accepted sampling transition among them) is the fp64 potential at the device's OWN stored sample
    within the U bound.  (A chain adapted over 24 transitions may reject all 6 sampling ones: the stack then repeats the last position warmup
    accepted, whose logged U' is compared.)"""
    R = M.RUN
    s, S = _short_run(R["key"])
    q0, x, lab = M.run_inputs()
    total = R["warmup"] + R["samples"]
    log = s.log
    assert tuple(log.shape) == (total, 8) and [k for _, _, k in HR.windows(R["warmup"])] == ["start", "middle", "end"]
    assert bool(torch.isfinite(S).all()) and bool(torch.isfinite(s.m_inv).all()) and bool((s.m_inv > 0).all())
    assert len(s.search_log) == 3, "one search before the first transition and one behind every window but the last"
    traj = R["eps"] * R["steps"]
    worst_ap = 0.0
    for i in range(total):
        eps, dH, ap, acc, u = (float(log[i, j]) for j in range(5))
        assert u == HR.uniform(s.key, i) and bool(acc) == (u < ap) == s.accepted_log[i], i
        ref = min(1.0, math.exp(-dH)) if dH > -700 else 1.0
        worst_ap = max(worst_ap, abs(ap - ref) / max(ref, 1e-300))
        assert abs(ap - ref) <= 4 * 2.0 ** -52 * ref, (i, ap, ref)          # two correctly rounded-to-an-ulp fp64 exponentials
        assert s.L_log[i] == max(1, int(traj / eps)) and s.eps_log[i] == eps, i
    # Row `row` of the stack is the position after transition warmup + row: the end point of the LAST ACCEPTED transition j <= warmup + row
    # (a sampling one, or — while the sampling phase has only rejected — a warmup one), whose logged U' is therefore U at that row.
    worst_U, compared = 0.0, set()
    for row in range(R["samples"]):
        i = R["warmup"] + row
        j = max((t for t in range(i + 1) if s.accepted_log[t]), default=None)
        if not s.accepted_log[i] and row > 0:
            assert torch.equal(S[row], S[row - 1]), "a rejected transition moved the chain"
        if j is not None and j not in compared:
            U64 = M.potential_at(S[row], s.shapes, x, lab, R["act"])
            worst_U = max(worst_U, abs(float(log[j, 5]) - U64) / abs(U64))
            compared.add(j)
    U_end = M.potential_at(s.q_cur, s.shapes, x, lab, R["act"])
    worst_U = max(worst_U, abs(s.read_state()["U"] - U_end) / abs(U_end))                 # the chain's cached U at its final position
    n_acc = sum(s.accepted_log[R["warmup"]:])
    print(f"[conv-hmc run key {R['key']}] {total} transitions, L {sorted(set(s.L_log))}, eps {s.eps_log[0]:.2e} .. {s.eps_log[-1]:.2e}, accepted "
          f"{sum(s.accepted_log)}/{total} ({n_acc} of the {R['samples']} sampling ones); accept_prob vs exp(-dH) {worst_ap:.1e}; logged U' of transitions "
          f"{sorted(compared)} and the cached U vs fp64 U at the device's own positions: {worst_U:.2e} ({worst_U / BOUND['U']:.2f} x bound)")
    assert compared, "no transition of the run was accepted: no stored sample has a logged U'"
    assert worst_U <= BOUND["U"]


def test_rerun_is_bit_identical_and_the_key_matters():
    R = M.RUN
    (a, Sa), (b, Sb), (c, Sc) = _short_run(R["key"]), _short_run(R["key"], 1), _short_run(R["key"] + 1)
    assert a is not b and torch.equal(Sa, Sb) and torch.equal(a.log, b.log) and torch.equal(a.m_inv, b.m_inv) and a.L_log == b.L_log
    assert torch.equal(a.q_cur, b.q_cur) and torch.equal(a.g_cur, b.g_cur) and torch.equal(a.state, b.state)
    assert not torch.equal(Sa, Sc)


def test_sampling_makes_no_device_to_host_sync():
    R = M.RUN
    s, _ = _short_run(R["key"] + 2)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        s.sample(R["warmup"] + R["samples"], R["samples"])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(s.samples_t).all())


def test_launches_per_leapfrog_step():
    """A step is the conv training forward (3 + 1 launches), the conv weight gradients (7) and ONE fused update: 12; a trajectory adds the
    opening update, a transition the momentum draw, the decision and the commit."""
    q0, x, lab = M.run_inputs()
    s = _sampler("tanh", M.RUN["C"], q0, 1e-3, 10, 3, M.RUN["B"], adapt_step_size=False)
    s.stage(x.to(DEV), lab.to(DEV))
    n0 = s.launches
    s.leapfrog(7)
    assert s.launches - n0 == 1 + 7 * 12
    n0 = s.launches
    s.transition(0, 5)
    assert s.launches - n0 == 1 + 1 + 12 * 5 + 1 + 1
    n0 = s.launches
    s.refresh()
    assert s.launches - n0 == 11 + 1 + 1 + 1


CANARY = {torch.float32: float("nan"), torch.float64: float("nan"), torch.uint8: 255, torch.int32: 0x7FFFFFFF}
PAD = 64                       # elements behind every buffer
CHAIN_BUFFERS = ("W", "grad", "q_cur", "g_cur", "r", "m_inv", "w_mean", "w_m2", "k0_part", "k1_part", "p_part", "state", "log_t", "samples_t")


def _padded(t):
    """A copy of the contiguous tensor t at the front of an allocation with PAD canary elements behind it -> (view, tail)."""
    big = torch.full((t.numel() + PAD,), CANARY[t.dtype], dtype=t.dtype, device=t.device)
    big[:t.numel()].copy_(t.reshape(-1))
    return big[:t.numel()].view(t.shape), big[t.numel():]


def _canaried_transitions(act, B, Cn, canaries):
    """Two transitions with Welford updates and sample rows, then a window end, of a sampler sized for exactly B points; canaries: every chain
    buffer, the log, the stack, the staged batch and every workspace are moved to the front of allocations with PAD canary elements (NaN; 255
    in the stash bytes; an impossible class in the labels) behind them.  -> (results' bit patterns, the tails)."""
    from robustbnns_amd import _hip
    g = torch.Generator().manual_seed(100 + B)
    x, lab = torch.rand(B, 1, 28, 28, generator=g), torch.randint(0, Cn, (B,), generator=g)
    s = _sampler(act, Cn, M.start_position(16, Cn), 1e-3, 2, 9, B, adapt_step_size=False)
    s.log_t = torch.zeros(2, _hip.HMC_LOG, dtype=torch.float64, device=DEV)
    s.samples_t = torch.zeros(2, s.n_params, device=DEV)
    tails = {}
    if canaries:
        for name in CHAIN_BUFFERS + ("X", "labels"):
            view, tails[name] = _padded(getattr(s, name))
            setattr(s, name, view)
        for k in list(s.ws_t):
            s.ws_t[k], tails["ws_" + k] = _padded(s.ws_t[k])
        s.net.W, s.net.grad = s.W.data_ptr(), s.grad.data_ptr()
        s.ws = _hip.fill(_hip.ConvTrainWs, s.ws_t)
    s._bind()
    s.stage(x.to(DEV), lab.to(DEV))
    assert s.Bmax == B
    s.transition(0, 2, False, False, 1, 0)
    s.transition(1, 2, False, False, 2, 1)
    s._window_end(2)
    torch.cuda.synchronize()
    res = {name: _bits(getattr(s, name)) for name in CHAIN_BUFFERS if name != "state"}
    res["state"], res["ce"] = _bits(s.state[:13]), _bits(s.ws_t["ce"][:B])
    for name in ("q_cur", "g_cur", "r", "m_inv", "samples_t", "ce", "W", "grad"):
        assert bool(torch.isfinite(res[name].view(torch.float32)).all()), name
    assert bool(torch.isfinite(res["state"]).all()) and bool(torch.isfinite(res["log_t"]).all()) and bool((s.m_inv > 0).all())
    return res, tails


@pytest.mark.parametrize("act,B", [("leaky", 5), ("relu", 65)])
def test_nothing_behind_the_bounds_is_read_or_written(act, B):
    """B = 5 and B = 65 with C = 3 (the bias tensor a partial quad at the end of every flat buffer), buffers sized for exactly B points.  Read:
    the results are bit-identical with and without NaN behind every buffer.  Written: every canary element is still a canary afterwards."""
    clean, _ = _canaried_transitions(act, B, 3, False)
    dirty, tails = _canaried_transitions(act, B, 3, True)
    for name in clean:
        assert torch.equal(clean[name], dirty[name]), f"{name} depends on memory behind the bounds"
    for name, tail in tails.items():
        intact = torch.isnan(tail).all() if tail.dtype.is_floating_point else (tail == CANARY[tail.dtype]).all()
        assert bool(intact) and tail.numel() == PAD, f"a launch wrote behind {name}"
    print(f"[conv-hmc bounds {act} B={B} C=3] {len(clean)} results bit-identical and finite with canaries behind {len(tails)} buffers, every canary "
          f"intact; excluded: nothing")


def test_train_hmc_conv_end_to_end(tmp_path):
    """BNN.train_hmc_conv on 16 random points in batches of 8 (n_samples 3, warmup 4): the n_samples files load back into a fresh BNN whose
    forward is the trained net's bit for bit and lies within the forward bar of the fp64 mean softmax at the device's OWN stack; a second
    run reproduces the stack; hmc_history has train_hmc's keys; train_hmc keeps refusing the net.  The chain is four warmup transitions away
    from Uniform(-2, 2), where logits are near 90 and an fp32 forward is about 1e-5 off fp64 whoever computes it: the data seed is the first at
    which torch's own fp32 forward on the CPU keeps half the bar (conv_hmc_restate.E2E; tests/test_conv_hmc_cpu.py holds the rule).  On the
    seed tried first, 11, torch's fp32 forward was 1.32e-05 off and this forward 1.07e-05."""
    from robustbnns_amd.model_bnn import BNN
    E = M.E2E
    x, y = M.e2e_data()
    loader = DataLoader(list(zip(x, y)), batch_size=E["batch"], shuffle=False)
    make = lambda: BNN("mnist", E["Hc"], E["act"], "conv", "hmc", None, None, E["n_samples"], E["warmup"], (1, 28, 28), E["C"],
                       step_size=E["step_size"], num_steps=E["num_steps"])
    net, path = make(), str(tmp_path) + "/"
    net.train_hmc_conv(loader, DEV, rel_path=path)
    assert len(glob.glob(os.path.join(path, net.name, "*.pt"))) == E["n_samples"]
    h = net.hmc_history
    batch_samples = int(E["n_samples"] / (E["n"] // E["batch"])) + 1
    assert set(h) == {"eps", "L", "dH", "accept_prob", "accepted", "m_inv", "key", "resampled"}
    assert len(h["eps"]) == len(h["L"]) == len(h["dH"]) == len(h["accept_prob"]) == len(h["accepted"]) == E["warmup"] + batch_samples
    assert tuple(h["resampled"].shape) == (E["n_samples"],) and int(h["resampled"].max()) < batch_samples and bool((h["m_inv"] > 0).all())
    again = make()
    again.load(DEV, rel_path=path)
    p0, p1 = net.forward(x.to(DEV), n_samples=E["n_samples"]), again.forward(x.to(DEV), n_samples=E["n_samples"])
    stack = {k: torch.stack([again.posterior.state_dict(i)[k] for i in range(E["n_samples"])]) for k in M.KEYS}
    p64 = M.predict(stack, x, E["act"])
    dev = float((p1.cpu().double() - p64).abs().max())
    print(f"[conv-hmc train_hmc_conv] L {h['L']} accepted {h['accepted']} eps {h['eps'][0]:.2e} .. {h['eps'][-1]:.2e}; forward of the loaded chain vs "
          f"the fp64 mean softmax at its own stack: {dev:.2e} ({dev / FORWARD_BAR:.2f} x the forward bar)")
    assert torch.equal(p0, p1) and bool(torch.isfinite(p0).all())
    assert dev <= FORWARD_BAR
    twice = make()
    twice.train_hmc_conv(loader, DEV, rel_path=str(tmp_path) + "/b/")
    assert all(torch.equal(twice.posterior.state_dict(i)[k], net.posterior.state_dict(i)[k]) for i in range(E["n_samples"]) for k in M.KEYS)
    assert twice.hmc_history["key"] == h["key"] and twice.hmc_history["accepted"] == h["accepted"]
    with pytest.raises(NotImplementedError, match="train_hmc_conv"):
        net.train_hmc(loader, DEV, rel_path=path)
