"""GPU tests (-m gpu) of K HMC chains in lockstep (csrc/rbnn_hmc.hip rbnn_hmc_lockstep_*, hmc.LockstepHmc, BNN.train_hmc(num_chains=K),
grid_search_halfMoons.lockstep_train).  The governing property: chain k of a lockstep run is BIT-IDENTICAL to hmc.HmcSampler running that
chain alone — every comparison below is torch.equal / list equality, there is no tolerance anywhere.  The single chain itself is held to
the fp64 restatement by tests/test_hip_hmc.py."""
import ctypes as C
import functools
import glob
import os

import pytest
import torch
from torch.utils.data import DataLoader

import hmc_restate as HR
import svi_restate as R

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("built_library")]
DEV = "cuda:0"
WARMUP, SAMPLES = 20, 6


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"


# Case A: the sizes of test_hip_hmc.py's _short_run.  The keys are three for which the fp64 restatement (tests/hmc_restate.py, on the CPU)
# takes [2, 4, 6], [2, 4, 7] and [2, 4, 5] tries in its three step-size searches (before the first transition, after the start and the middle
# window; none after the last) and L of 13 / 6 / 6, 5 / 2 / 28 and 3 / 60 / 6 at transitions 6, 10 and 16 of warmup, so the `active` and
# `steps` masks are exercised; the test asserts both on the single-chain GPU runs before it compares anything.
KEYS_A = (70, 73, 76)


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (arch, act, D, Cn, [q0 per chain], x, labels, step size, num_steps, keys)"""
    if name == "A":
        q0, x, lab = HR.run_case("fc2", "leaky", 32, 128, 5)
        return "fc2", "leaky", 2, 2, [q0] * 3, x, lab, 0.01, 10, KEYS_A
    # Case B: fc / tanh, D = 17, H = 96, C = 3, B = 32: ragged tiles in M (32 of 64), N (96 = 64 + 32) and K (17 = 16 + 1)
    g = torch.Generator().manual_seed(17)
    x, lab = torch.randn(32, 17, generator=g), torch.randint(0, 3, (32,), generator=g)
    q0s = [{k: 0.5 * (torch.rand(*s, generator=g) * 2 - 1) for k, s in R.shapes_of("fc", 17, 96, 3).items()} for _ in range(3)]
    return "fc", "tanh", 17, 3, q0s, x, lab, 0.01, 10, (5, 6, 7)


def _single(arch, act, D, Cn, q0, eps, steps, key, x, lab, samples=SAMPLES, warmup=WARMUP):
    from robustbnns_amd.hmc import HmcSampler
    s = HmcSampler(arch, act, (1, D, 1), Cn, q0, eps, steps, DEV, key, batch_size=int(x.shape[0]))
    stack = s.run(x.to(DEV), lab.to(DEV), samples, warmup)
    return s, torch.cat([stack[k].reshape(samples, -1) for k in s.keys], 1).clone()


def _lockstep(arch, act, D, Cn, q0s, eps, steps, keys, B, **kw):
    from robustbnns_amd.hmc import LockstepHmc
    return LockstepHmc(arch, act, (1, D, 1), Cn, q0s, eps, steps, DEV, keys, batch_size=B, **kw)


def _assert_chain_equals_single(ls, stacks, k, s, S, samples=SAMPLES):
    Sk = torch.cat([stacks[k][key].reshape(samples, -1) for key in ls.keys], 1)
    assert ls.L_log[k] == s.L_log, f"chain {k}: an L differs"
    assert ls.accepted_log[k] == s.accepted_log, f"chain {k}: a decision differs"
    assert [len(t) for t in ls.search_log[k]] == [len(t) for t in s.search_log], f"chain {k}: a search took another number of tries"
    assert ls.search_log[k] == s.search_log, f"chain {k}: a search try differs"
    assert torch.equal(ls.log[k], s.log), f"chain {k}: the log differs"
    assert torch.equal(Sk, S), f"chain {k}: the sample stack differs"
    for name in ("m_inv", "q_cur", "g_cur"):
        assert torch.equal(getattr(ls, name)[k], getattr(s, name)), f"chain {k}: {name} differs"
    a, b = ls.read_state()[k], s.read_state()
    assert a["U"] == b["U"] and a["eps"] == b["eps"], (k, a, b)
    assert ls.eps_log[k] == s.eps_log and ls.dH_log[k] == s.dH_log


@pytest.mark.parametrize("name", ["A", "B"])
def test_every_chain_equals_the_single_chain_bit_for_bit(name):
    arch, act, D, Cn, q0s, x, lab, eps, steps, keys = _case(name)
    singles = [_single(arch, act, D, Cn, q0s[k], eps, steps, keys[k], x, lab) for k in range(3)]
    tries = [[len(t) for t in s.search_log] for s, _ in singles]
    print(f"[case {name}] single chains: search tries {tries}  L of the sampling phase {[s.L_log[-1] for s, _ in singles]}")
    if name == "A":                                                          # the masks are exercised
        assert not (singles[0][0].L_log == singles[1][0].L_log == singles[2][0].L_log), "the three chains have the same L at every transition"
        assert not (tries[0] == tries[1] == tries[2]), "the three chains' searches take the same number of tries"
    ls = _lockstep(arch, act, D, Cn, q0s, eps, steps, keys, int(x.shape[0]))
    stacks = ls.run(x.to(DEV), lab.to(DEV), SAMPLES, WARMUP)
    for k, (s, S) in enumerate(singles):
        _assert_chain_equals_single(ls, stacks, k, s, S)


def _ragged():
    """200 resident half-moons points; three chains of one key and start position on 128, 100 and 37 of them through distinct rows (37 ends
    inside a 16-wide K stage of the weight-gradient GEMM, 100 inside a 64-wide tile); the rows behind a chain's count hold other valid points."""
    q0, _, _ = HR.run_case("fc2", "leaky", 32, 128, 5)
    x, y = R.two_moons(200, 0.1, 7)
    g = torch.Generator().manual_seed(3)
    rows = torch.stack([torch.randperm(200, generator=g)[:128] for _ in range(3)]).to(torch.int32)
    return q0, x, y.argmax(-1), rows, (128, 100, 37)


def test_ragged_batches_equal_the_single_chain_on_its_own_points():
    q0, x, lab, rows, counts = _ragged()
    ls = _lockstep("fc2", "leaky", 2, 2, [q0] * 3, 0.01, 10, [77] * 3, 128)
    ls.set_data(x.to(DEV), lab.to(DEV))
    stacks = ls.run(rows=rows, counts=counts, num_samples=SAMPLES, warmup=WARMUP)
    for k in range(3):
        sel = rows[k, :counts[k]].long()
        s, S = _single("fc2", "leaky", 2, 2, q0, 0.01, 10, 77, x[sel], lab[sel])
        _assert_chain_equals_single(ls, stacks, k, s, S)
    assert not torch.equal(ls.samples_t[0], ls.samples_t[1])                 # the data differ, so the chains do


def test_an_inactive_chain_is_neither_read_nor_written():
    arch, act, D, Cn, q0s, x, lab, eps, steps, keys = _case("A")
    ls = _lockstep(arch, act, D, Cn, q0s, eps, steps, keys, 128)
    ls.run(x.to(DEV), lab.to(DEV), 2, 3)
    names = ("q_cur", "g_cur", "r", "m_inv", "w_mean", "w_m2", "state", "log_t", "samples_t", "k0_part", "k1_part", "p_part")
    before = {n: getattr(ls, n).clone() for n in names}
    ls.set_active([True, False, True])
    ls.transition(4, [3, 2, 5], adapt=True, window_end=False, welford_n=1, sample_row=1)
    from robustbnns_amd import _hip
    _hip.check(ls.k.lib.rbnn_hmc_lockstep_window_end(C.byref(ls.net), C.byref(ls.chain), 2, ls._st()), "rbnn_hmc_lockstep_window_end")
    torch.cuda.synchronize()
    for n in names:
        assert torch.equal(getattr(ls, n)[1], before[n][1]), f"{n} of the inactive chain changed"
    for k in (0, 2):                                                         # the others did move
        assert not torch.equal(ls.r[k], before["r"][k]) and not torch.equal(ls.m_inv[k], before["m_inv"][k])
        assert not torch.equal(ls.log_t[k, 4], before["log_t"][k, 4])


@pytest.mark.parametrize("arch,fwd", [("fc", 2), ("fc2", 4)])
def test_launches_of_a_transition_do_not_depend_on_the_number_of_chains(arch, fwd):
    from robustbnns_amd.hmc import HmcSampler
    q0, x, lab = HR.transition_case(arch, "leaky", 32, 64)
    s = HmcSampler(arch, "leaky", (1, 2, 1), 2, q0, 0.001, 10, DEV, 3, adapt_step_size=False, batch_size=64)
    s.stage(x.to(DEV), lab.to(DEV))
    n0 = s.launches
    s.transition(0, 5)
    single = s.launches - n0
    assert single == 3 + 1 + 5 * (fwd + 1 + 1)
    for K, Ls in ((1, [5]), (3, [2, 5, 3])):
        ls = _lockstep(arch, "leaky", 2, 2, [q0] * K, 0.001, 10, list(range(3, 3 + K)), 64, adapt_step_size=False)
        ls.set_data(x.to(DEV), lab.to(DEV))
        ls.stage()
        n0 = ls.launches
        ls.transition(0, Ls)
        assert ls.launches - n0 == single, (K, ls.launches - n0)


def test_sampling_makes_no_device_to_host_sync():
    arch, act, D, Cn, q0s, x, lab, eps, steps, keys = _case("A")
    ls = _lockstep(arch, act, D, Cn, q0s, eps, steps, keys, 128)
    ls.run(x.to(DEV), lab.to(DEV), SAMPLES, WARMUP)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ls.sample(WARMUP + SAMPLES, SAMPLES)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ls.samples_t).all())


def test_nothing_outside_the_buffers_is_written():
    """Every buffer the kernels write is a view into a poisoned slab with a guard zone on BOTH sides: two transitions with Welford, a window
    end and sample rows, K = 3 with ragged counts, leave every guard zone as it was and every result finite."""
    from robustbnns_amd import _hip
    q0, x, lab, rows, counts = _ragged()
    q0 = {k: 0.25 * v for k, v in q0.items()}
    ls = _lockstep("fc2", "leaky", 2, 2, [q0] * 3, 0.002, 5, [9, 10, 11], 128, adapt_step_size=False)
    G, slabs = 512, []

    def guarded(t):
        poison = float("nan") if t.is_floating_point() else -7
        slab = torch.full((t.numel() + 2 * G,), poison, dtype=t.dtype, device=DEV)
        slab[G:G + t.numel()].copy_(t.reshape(-1))
        slabs.append((slab, t.numel(), poison))
        return slab[G:G + t.numel()].view(t.shape)

    for name in ("W", "grad", "q_cur", "g_cur", "r", "m_inv", "w_mean", "w_m2", "k0_part", "k1_part", "p_part", "state"):
        setattr(ls, name, guarded(getattr(ls, name)))
    ls.log_t = guarded(torch.zeros(3, 2, _hip.HMC_LOG, dtype=torch.float64, device=DEV))
    ls.samples_t = guarded(torch.zeros(3, 2, ls.n_params, device=DEV))
    ls._bind()
    ls._ensure(128)
    for k in list(ls.ws_t):
        ls.ws_t[k] = guarded(ls.ws_t[k])
    ls.ws = _hip.NnTrainWs()
    for k in _hip.NN_TRAIN_WS_KEYS:
        setattr(ls.ws, k, _hip.ptr(ls.ws_t.get(k)))
    ls.set_data(x.to(DEV), lab.to(DEV))
    ls.stage(rows, counts)
    ls.transition(0, [3, 1, 2], False, False, 1, 0)
    ls.transition(1, [2, 3, 1], False, False, 2, 1)
    _hip.check(ls.k.lib.rbnn_hmc_lockstep_window_end(C.byref(ls.net), C.byref(ls.chain), 2, ls._st()), "rbnn_hmc_lockstep_window_end")
    assert ls.k.lib.rbnn_hmc_lockstep_commit(C.byref(ls.net), C.byref(ls.chain), 0, 0, 2, ls._st()) != 0       # a row behind the stacks is refused
    torch.cuda.synchronize()
    for i, (slab, n, poison) in enumerate(slabs):
        edge = torch.cat([slab[:G], slab[G + n:]])
        ok = torch.isnan(edge).all() if slab.is_floating_point() else (edge == poison).all()
        assert bool(ok), f"buffer {i}: a guard zone was written"
    for name in ("q_cur", "g_cur", "r", "m_inv", "samples_t", "log_t"):
        assert bool(torch.isfinite(getattr(ls, name)).all()), name
    assert bool(torch.isfinite(ls.state[:, :13]).all()) and bool((ls.m_inv > 0).all())


def _moons_net(n_inputs=128):
    from robustbnns_amd.grid_search_halfMoons import MoonsBNN
    return MoonsBNN(32, "leaky", "fc2", "hmc", None, None, 5, 5, n_inputs, (1, 2, 1), 2)


def test_train_hmc_with_two_chains(tmp_path):
    x, y = R.two_moons(128, 0.1, 7)
    xt, _ = R.two_moons(64, 0.1, 8)
    loader = DataLoader(list(zip(x, y)), batch_size=1024, shuffle=False)
    one = _moons_net()
    one.train_hmc(loader, DEV, rel_path=str(tmp_path) + "/one/")
    # the num_chains = 1 run's own stack: the same chain again (train_hmc seeds itself), kept before the resampling
    from robustbnns_amd.hmc import HmcSampler
    x_batch, y_batch, batch_samples, q0, key = _moons_net()._hmc_prologue(loader, DEV)
    assert key == one.hmc_history["key"] and batch_samples == 6
    s = HmcSampler("fc2", "leaky", (1, 2, 1), 2, q0, one.step_size, one.num_steps, DEV, key, batch_size=128)
    stack1 = s.run(x_batch.to(DEV), y_batch.to(DEV).argmax(-1), batch_samples, 5)
    assert s.accepted_log == one.hmc_history["accepted"] and s.eps_log == one.hmc_history["eps"]
    two = _moons_net()
    path = str(tmp_path) + "/two/"
    two.train_hmc(loader, DEV, rel_path=path, num_chains=2)
    h = two.hmc_history
    for k, v in stack1.items():
        assert tuple(h["stack"][k].shape[:1]) == (2 * batch_samples,)
        assert torch.equal(h["stack"][k][:batch_samples], v), f"chain 0 is not the single chain: {k}"
        assert not torch.equal(h["stack"][k][batch_samples:], v)
    assert h["key"] == key and h["chains"][0]["key"] == key and h["chains"][1]["key"] != key
    assert h["accepted"] == one.hmc_history["accepted"] and len(h["chains"]) == 2
    assert int(h["resampled"].max()) < 2 * batch_samples and torch.isfinite(torch.tensor(h["r_hat_U"]))
    assert len(glob.glob(os.path.join(path, two.name, "*.pt"))) == 5
    again = _moons_net()
    again.load(DEV, rel_path=path)
    p = again.forward(xt.to(DEV), n_samples=5)
    assert bool(torch.isfinite(p).all()) and torch.allclose(p.sum(-1), torch.ones(64, device=DEV), atol=1e-5)
    with pytest.raises(ValueError, match="num_chains"):
        two.train_hmc(loader, DEV, rel_path=path, num_chains=0)


def test_lockstep_train_saves_what_serial_train_saves(tmp_path):
    from robustbnns_amd.grid_search_halfMoons import lockstep_train, serial_train
    x, y = R.two_moons(160, 0.1, 7)
    grid = ([32], ["leaky"], ["fc2"], ["hmc"], [None], [None], [5], [5], [96, 160], [5])
    a = serial_train(*grid, str(tmp_path) + "/serial/", x_train=x, y_train=y, device=DEV)
    b = lockstep_train(*grid, str(tmp_path) + "/lockstep/", x_train=x, y_train=y, device=DEV)
    assert list(a) == list(b) and len(a) == 2
    for name in a:
        assert a[name].hmc_history["key"] == b[name].hmc_history["key"]
        assert a[name].hmc_history["accepted"] == b[name].hmc_history["accepted"] and a[name].hmc_history["L"] == b[name].hmc_history["L"]
        assert torch.equal(a[name].hmc_history["resampled"], b[name].hmc_history["resampled"])
        fa = sorted(glob.glob(os.path.join(str(tmp_path), "serial", name, "*.pt")))
        fb = sorted(glob.glob(os.path.join(str(tmp_path), "lockstep", name, "*.pt")))
        assert len(fa) == 5 and [os.path.basename(f) for f in fa] == [os.path.basename(f) for f in fb]
        for pa, pb in zip(fa, fb):
            sa, sb = torch.load(pa, map_location="cpu"), torch.load(pb, map_location="cpu")
            assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa), (name, os.path.basename(pa))
