"""GPU tests (-m gpu) of several conv HMC chains behind every launch (the rbnn_conv_hmc_chains_* entry points of csrc/rbnn_hmc.hip and
csrc/rbnn_conv_train.hip, conv_hmc.ConvLockstepHmc, BNN.train_hmc_conv(num_chains=K, group)).  The governing property: chain k is BIT-IDENTICAL
to conv_hmc.ConvHmcSampler running that chain alone on its rows — every comparison below is equality of bits or of integers, there is no
tolerance anywhere.  The single chain itself is held to the fp64 restatement by tests/test_hip_conv_hmc.py, its gradient by
tests/test_hip_conv_train*.py.

Shapes.  Hc 16, C 3: the smallest net, whose model.7.bias of 3 floats puts chains 1 and 2 of every later block at addresses that are no
16-byte multiples; Hc 48, C 10: three 16-channel groups.  B in {1, 5, 8, 65}: one point, no multiple of 4, conv_hmc_restate.RUN's, one past a
64-row tile.  K = 3 (odd), another start position, key and step size per chain.  The tensors' offsets (800, 832, ...) are no multiples of 256
apart, so blocks of the element-wise kernels straddle tensor borders at every one of these shapes."""
import ctypes as C
import glob
import os

import pytest
import torch
from torch.utils.data import DataLoader

import conv_hmc_restate as M
import conv_svi_restate as V

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("built_library")]
DEV = "cuda:0"
K = 3
WARMUP, SAMPLES = M.RUN["warmup"], M.RUN["samples"]                            # 24 + 6: all three window kinds, two searches, mass adaptation
RUN_STEPS = 40                  # trajectories of 0.04, 0.08 and 0.02 for the three step sizes, so that the step sizes warmup adapts to give the chains different L
TM = ("W", "grad", "q_cur", "g_cur", "r", "_m_inv", "w_mean", "w_m2")          # ConvLockstepHmc's tensor-major buffers, by attribute
PARTS = ("k0_part", "k1_part", "p_part")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"


def _bits(t):
    t = t.detach().contiguous()
    return (t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t).cpu().clone()


def _same(a, b):
    """Equality of bits (NaN patterns included) and of shape."""
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and bool((a == b).all())


def _differing(a, b):
    return int((_bits(a).reshape(-1) != _bits(b).reshape(-1)).sum())


def _q0s(Hc, Cn):
    return [V.guide(Hc, Cn, M.Q0_SEED + 10 * k)[0] for k in range(K)]


def _data(B, Cn, seed, n=None):
    g = torch.Generator().manual_seed(seed)
    n = B if n is None else n
    return torch.rand(n, 1, 28, 28, generator=g), torch.randint(0, Cn, (n,), generator=g)


def _single(act, Cn, q0, eps, steps, key, B, **kw):
    from robustbnns_amd.conv_hmc import ConvHmcSampler
    return ConvHmcSampler(act, (1, 28, 28), Cn, q0, eps, steps, DEV, key, batch_size=B, **kw)


def _lockstep(act, Cn, q0s, eps, steps, keys, B, **kw):
    from robustbnns_amd.conv_hmc import ConvLockstepHmc
    return ConvLockstepHmc(act, (1, 28, 28), Cn, q0s, eps, steps, DEV, keys, batch_size=B, **kw)


def _flat_stack(s, stack, samples):
    return torch.cat([stack[k].reshape(samples, -1) for k in s.keys], 1).clone()


def _assert_chain_equals_single(ls, stacks, k, s, S, samples, what):
    """The issue's list: sample stack, log, m_inv, q_cur, g_cur, state, L_log, search_log, eps_log — 0 differing elements."""
    Sk = _flat_stack(ls, stacks[k], samples)
    diffs = {"stack": _differing(Sk, S), "log": _differing(ls.log[k], s.log), "m_inv": _differing(ls.m_inv[k], s.m_inv),
             "q_cur": _differing(ls.chain_flat(ls.q_cur, k), s.q_cur), "g_cur": _differing(ls.chain_flat(ls.g_cur, k), s.g_cur),
             "state": _differing(ls.state[k], s.state)}
    print(f"[{what} chain {k}] differing elements {diffs}; L {sorted(set(s.L_log))}, search tries {[len(t) for t in s.search_log]}, "
          f"eps {s.eps_log[0]:.2e} .. {s.eps_log[-1]:.2e}")
    assert not any(diffs.values()), (k, diffs)
    assert ls.L_log[k] == s.L_log, f"chain {k}: an L differs"
    assert ls.search_log[k] == s.search_log, f"chain {k}: a search try differs"
    assert ls.eps_log[k] == s.eps_log and ls.dH_log[k] == s.dH_log and ls.accepted_log[k] == s.accepted_log
    assert tuple(ls.m_inv.shape) == (ls.K, ls.n_params) and tuple(s.m_inv.shape) == (ls.n_params,)


@pytest.mark.parametrize("Hc,act,B,Cn", [(16, "tanh", 8, 10), (16, "leaky", 5, 3)])
def test_every_chain_equals_the_single_chain_bit_for_bit(Hc, act, B, Cn):
    q0s, keys, sizes = _q0s(Hc, Cn), [M.RUN["key"], M.RUN["key"] + 4, M.RUN["key"] + 9], [1e-3, 2e-3, 5e-4]
    x, lab = M.run_inputs()[1:] if (B, Cn) == (M.RUN["B"], M.RUN["C"]) else _data(B, Cn, 40 + B)
    singles = []
    for k in range(K):
        s = _single(act, Cn, q0s[k], sizes[k], RUN_STEPS, keys[k], B)
        singles.append((s, _flat_stack(s, s.run(x.to(DEV), lab.to(DEV), SAMPLES, WARMUP), SAMPLES)))
    # the masks are exercised: the chains' adapted step sizes, their trajectory lengths and their searches differ
    assert len({tuple(s.eps_log) for s, _ in singles}) == K, "two chains adapted to the same step sizes"
    assert not (singles[0][0].L_log == singles[1][0].L_log == singles[2][0].L_log), "the three chains have the same L at every transition"
    assert all(len(s.search_log) == 3 for s, _ in singles)
    ls = _lockstep(act, Cn, q0s, sizes, RUN_STEPS, keys, B)
    stacks = ls.run(x.to(DEV), lab.to(DEV), SAMPLES, WARMUP)
    assert tuple(ls.samples_t.shape) == (K, SAMPLES, ls.n_params) and tuple(ls.log.shape) == (K, WARMUP + SAMPLES, 8)
    for k, (s, S) in enumerate(singles):
        _assert_chain_equals_single(ls, stacks, k, s, S, SAMPLES, f"conv-hmc chains run Hc={Hc} {act} B={B} C={Cn}")
    assert not _same(ls.samples_t[0], ls.samples_t[1])


@pytest.mark.parametrize("Hc,act,B,Cn", [(48, "sigm", 65, 10), (16, "relu", 1, 10)])
def test_trajectories_of_different_lengths_equal_the_single_chains(Hc, act, B, Cn):
    """leapfrog([1, 3, 2]) without adaptation: each chain's W, r, grad, k1_part and p_part are the single chain's after leapfrog(n)."""
    Ls, q0s, keys, sizes = [1, 3, 2], _q0s(Hc, Cn), [5, 6, 7], [1e-3, 2e-3, 5e-4]
    x, lab = _data(B, Cn, 60 + B)
    ls = _lockstep(act, Cn, q0s, sizes, 4, keys, B, adapt_step_size=False)
    ls.set_data(x.to(DEV), lab.to(DEV))
    ls.stage()
    ls._draw(0)
    assert ls.leapfrog(Ls) == Ls
    torch.cuda.synchronize()
    worst = {}
    for k in range(K):
        s = _single(act, Cn, q0s[k], sizes[k], 4, keys[k], B, adapt_step_size=False)
        s.stage(x.to(DEV), lab.to(DEV))
        s._draw(0)
        s.leapfrog(Ls[k])
        torch.cuda.synchronize()
        for name in ("W", "r", "grad"):
            worst[name] = max(worst.get(name, 0), _differing(ls.chain_flat(getattr(ls, name), k), getattr(s, name)))
        for name in ("k1_part", "p_part", "k0_part"):
            worst[name] = max(worst.get(name, 0), _differing(getattr(ls, name)[k], getattr(s, name)))
        assert _same(ls.ws_t["ce"][k * B:(k + 1) * B], s.ws_t["ce"][:B]), k
        assert float(s.r.abs().max()) > 0 and float(s.grad.abs().max()) > 0
    print(f"[conv-hmc chains leapfrog {Ls} Hc={Hc} {act} B={B} C={Cn}] worst differing elements over the chains {worst}")
    assert not any(worst.values()), worst


def test_chains_on_their_own_rows_equal_the_single_chain_on_those_points():
    """32 resident points, rows [3, 8] (chain 1's with repeated indices): chain k is the single chain on data[rows[k]]."""
    act, Cn, B, warmup, samples = "tanh", 10, 8, 4, 2
    q0s, keys = _q0s(16, Cn), [31, 32, 33]
    x, lab = _data(B, Cn, 9, n=32)
    g = torch.Generator().manual_seed(2)
    rows = torch.stack([torch.randperm(32, generator=g)[:B], torch.tensor([4, 4, 17, 0, 31, 17, 4, 9]), torch.randperm(32, generator=g)[:B]]).to(torch.int32)
    ls = _lockstep(act, Cn, q0s, 1e-3, 4, keys, B)
    ls.set_data(x.to(DEV), lab.to(DEV))
    with pytest.raises(ValueError, match="rows"):
        ls.stage(rows[:2])
    stacks = ls.run(rows=rows, num_samples=samples, warmup=warmup)
    assert ls.B == B
    for k in range(K):
        sel = rows[k].long()
        s = _single(act, Cn, q0s[k], 1e-3, 4, keys[k], B)
        S = _flat_stack(s, s.run(x[sel].to(DEV), lab[sel].to(DEV), samples, warmup), samples)
        _assert_chain_equals_single(ls, stacks, k, s, S, samples, "conv-hmc chains rows")
    assert not _same(ls.ws_t["ce"][:B], ls.ws_t["ce"][B:2 * B])                # the data differ, so the chains do


def _set_chain(ls, buf, k, values):
    """Chain k's values of a tensor-major buffer <- the flat [n_params] values in state_dict order."""
    off = src = 0
    for size in ls.blocks:
        buf[off + k * size:off + (k + 1) * size] = values[src:src + size]
        off, src = off + ls.K * size, src + size


def _activity_run(mask):
    """Momentum, update(OPEN), gradient, update(CLOSE), decide, commit, window end on K = 3 chains (Hc 16, C 3, B 5), chain 1's nine chain
    buffers, state, log and sample rows filled with a recognisable pattern first.  -> (sampler, the pattern per buffer)"""
    from robustbnns_amd import _hip
    act, Cn, B = "leaky", 3, 5
    x, lab = _data(B, Cn, 21)
    ls = _lockstep(act, Cn, _q0s(16, Cn), [1e-3, 2e-3, 5e-4], 4, [11, 12, 13], B)
    ls.log_t = torch.zeros(K, 2, _hip.HMC_LOG, dtype=torch.float64, device=DEV)
    ls.samples_t = torch.zeros(K, 2, ls.n_params, device=DEV)
    ls._bind()
    ls.set_data(x.to(DEV), lab.to(DEV))
    ls.stage()
    # recognisable, and of a size a chain can run on (the all-active run moves chain 1 from them): positions, gradients and momenta of
    # 1e-2 at most, inverse masses in [0.5, 0.75], the state block's step size 1e-3 (1 + 1 / 64)
    n, pattern = ls.n_params, {}
    ramp = (torch.arange(n, dtype=torch.float32, device=DEV) % 251) - 125.0
    for i, name in enumerate(TM[2:]):                                          # the six per-parameter chain buffers
        pattern[name] = 0.5 + (ramp + 125.0) * 1e-3 if name == "_m_inv" else ramp * 1e-5 * (i + 1)
        _set_chain(ls, getattr(ls, name), 1, pattern[name])
    for i, name in enumerate(PARTS + ("log_t", "samples_t")):
        t = getattr(ls, name)[1]
        pattern[name] = (torch.arange(t.numel(), device=DEV) % 127 + (i + 1) * 2000).to(t.dtype).reshape(t.shape)
        t.copy_(pattern[name])
    pattern["state"] = torch.tensor([1e-3 * (1 + 1 / 64), 12345.0, 3.0, 0.25, -6.5, -4.5] + [7000.0 + j for j in range(6, _hip.HMC_STATE)],
                                    dtype=torch.float64, device=DEV)
    ls.state[1].copy_(pattern["state"])
    ls.set_active(mask)
    ls._draw(0)
    ls._update(_hip.HMC_OPEN)
    ls._gradient()
    ls._update(_hip.HMC_CLOSE)
    ls._decide(_hip.HMC_DECIDE_TRANSITION, 0, True, False)
    ls._commit(False, 1, 0)
    ls._window_end(2)
    torch.cuda.synchronize()
    return ls, pattern


def test_an_inactive_chain_is_neither_read_nor_written():
    masked, pattern = _activity_run([True, False, True])
    full, _ = _activity_run(None)
    for name in TM[2:]:
        assert _same(masked.chain_flat(getattr(masked, name), 1), pattern[name]), f"{name} of the inactive chain changed"
    for name in ("r", "_m_inv", "w_mean", "w_m2"):                             # written whatever the decision is (the window end zeroes Welford's)
        assert not _same(full.chain_flat(getattr(full, name), 1), pattern[name]), f"{name} of an active chain 1 did not move"
    for name in PARTS + ("state", "log_t", "samples_t"):
        assert _same(getattr(masked, name)[1], pattern[name]), f"{name} of the inactive chain changed"
    for name in PARTS + ("state",):
        assert not _same(getattr(full, name)[1], pattern[name]), f"{name} of an active chain 1 did not move"
    assert not _same(full.log_t[1, 0], pattern["log_t"][0]) and not _same(full.samples_t[1, 0], pattern["samples_t"][0])
    for k in (0, 2):                                                           # the others equal the all-active run
        for name in TM:
            assert _same(masked.chain_flat(getattr(masked, name), k), full.chain_flat(getattr(full, name), k)), (name, k)
        for name in PARTS + ("state", "log_t", "samples_t"):
            assert _same(getattr(masked, name)[k], getattr(full, name)[k]), (name, k)
        assert float(masked.chain_flat(masked.r, k).abs().max()) > 0
    print("[conv-hmc chains activity] chain 1 of 3 inactive: its 9 chain buffers, state, log and sample rows keep their bits; chains 0 and 2 "
          "equal the all-active run in 8 per-parameter buffers, 3 partial sums, state, log and samples")


@pytest.mark.parametrize("n_chains,Ls", [(1, [5]), (3, [2, 5, 3])])
def test_launches_of_a_transition_do_not_depend_on_the_number_of_chains(n_chains, Ls):
    q0, x, lab = M.run_inputs()
    ls = _lockstep("tanh", M.RUN["C"], [q0] * n_chains, 1e-3, 10, list(range(3, 3 + n_chains)), M.RUN["B"], adapt_step_size=False)
    ls.set_data(x.to(DEV), lab.to(DEV))
    n0 = ls.launches
    ls.stage()
    assert ls.launches - n0 == 1 + 11 + 1 + 1 + 1
    n0 = ls.launches
    ls.refresh()
    assert ls.launches - n0 == 11 + 1 + 1 + 1
    n0 = ls.launches
    assert ls.transition(0, Ls) == Ls
    assert ls.launches - n0 == 1 + 1 + 12 * max(Ls) + 1 + 1
    n0 = ls.launches
    ls.leapfrog(7)
    assert ls.launches - n0 == 1 + 7 * 12
    torch.cuda.synchronize()


def test_sampling_makes_no_device_to_host_sync():
    q0, x, lab = M.run_inputs()
    ls = _lockstep("tanh", M.RUN["C"], _q0s(16, M.RUN["C"]), 1e-3, 4, [1, 2, 3], M.RUN["B"])
    ls.run(x.to(DEV), lab.to(DEV), 3, 4)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ls.sample(4 + 3, 3)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ls.samples_t).all())


CANARY = {torch.float32: float("nan"), torch.float64: float("nan"), torch.uint8: 255, torch.int32: 0x7FFFFFFF, torch.int64: 0x7FFFFFFFFFFFFFFF}
PAD = 64                       # elements behind every buffer
CHAIN_BUFFERS = TM + PARTS + ("state", "log_t", "samples_t")
PER_CHAIN = ("keys_t", "steps_t", "active_t", "draw_ids_t")


def _padded(t):
    """A copy of the contiguous tensor t at the front of an allocation with PAD canary elements behind it -> (view, tail)."""
    big = torch.full((t.numel() + PAD,), CANARY[t.dtype], dtype=t.dtype, device=t.device)
    big[:t.numel()].copy_(t.reshape(-1))
    return big[:t.numel()].view(t.shape), big[t.numel():]


def _canaried_transitions(canaries):
    """K = 3, Hc 16, C 3, B 5, buffers sized for exactly B points per chain: a probe of the step-size search with chain 2 frozen (draw_ids and
    active are read), then two transitions of different lengths with Welford updates and sample rows, then a window end.  canaries: every
    buffer of the chain block, W, grad, the per-chain device values, the resident data, the rows and every workspace are moved to the front
    of allocations with PAD canary elements behind them.  -> (results' bit patterns, the tails)"""
    from robustbnns_amd import _hip
    act, Cn, B = "leaky", 3, 5
    x, lab = _data(B, Cn, 100 + B, n=12)
    rows = torch.tensor([[0, 3, 5, 7, 11], [1, 1, 2, 10, 4], [6, 8, 9, 0, 2]], dtype=torch.int32, device=DEV)
    ls = _lockstep(act, Cn, _q0s(16, Cn), [1e-3, 2e-3, 5e-4], 2, [9, 10, 11], B, adapt_step_size=False)
    ls.log_t = torch.zeros(K, 2, _hip.HMC_LOG, dtype=torch.float64, device=DEV)
    ls.samples_t = torch.zeros(K, 2, ls.n_params, device=DEV)
    ls.set_data(x.to(DEV), lab.to(DEV))
    tails = {}
    if canaries:
        for name in CHAIN_BUFFERS + PER_CHAIN + ("X", "labels"):
            view, tails[name] = _padded(getattr(ls, name))
            setattr(ls, name, view)
        rows, tails["rows"] = _padded(rows)
        for k in list(ls.ws_t):
            ls.ws_t[k], tails["ws_" + k] = _padded(ls.ws_t[k])
        ls.ws = _hip.fill(_hip.ConvEnsWs, ls.ws_t)
    ls._bind()
    ls.stage(rows)
    assert ls.Bmax == B and ls.rows_t.data_ptr() == rows.data_ptr()
    ls.set_active([True, True, False])
    ls._searches = [3, 1, 0]
    ls._draw(None)
    ls.leapfrog(1)
    ls._decide(_hip.HMC_DECIDE_PROBE)
    ls.set_active(None)
    ls.transition(0, [2, 1, 3], False, False, 1, 0)
    ls.transition(1, [1, 3, 2], False, False, 2, 1)
    ls._window_end(2)
    torch.cuda.synchronize()
    res = {name: _bits(getattr(ls, name)) for name in CHAIN_BUFFERS if name != "state"}
    res["state"], res["ce"] = _bits(ls.state[:, :13]), _bits(ls.ws_t["ce"][:K * B])
    for name in ("q_cur", "g_cur", "r", "_m_inv", "samples_t", "W", "grad"):
        assert bool(torch.isfinite(getattr(ls, name)).all()), name
    assert bool(torch.isfinite(ls.state[:, :13]).all()) and bool(torch.isfinite(ls.log_t).all()) and bool((ls._m_inv > 0).all())
    assert not _same(ls.m_inv, torch.ones(K, ls.n_params))                     # the window end wrote every chain's inverse mass
    return res, tails


def test_nothing_behind_the_bounds_is_read_or_written():
    """Read: the results are bit-identical with and without canaries behind every buffer (two runs).  Written: every canary element is still
    a canary afterwards."""
    clean, _ = _canaried_transitions(False)
    dirty, tails = _canaried_transitions(True)
    for name in clean:
        assert torch.equal(clean[name], dirty[name]), f"{name} depends on memory behind the bounds"
    for name, tail in tails.items():
        intact = torch.isnan(tail).all() if tail.dtype.is_floating_point else (tail == CANARY[tail.dtype]).all()
        assert bool(intact) and tail.numel() == PAD, f"a launch wrote behind {name}"
    assert len(tails) == len(CHAIN_BUFFERS) + len(PER_CHAIN) + 3 + 15
    print(f"[conv-hmc chains bounds leaky K=3 B=5 C=3] {len(clean)} results bit-identical and finite with canaries behind {len(tails)} buffers, "
          f"every canary intact; excluded: nothing")


# BNN.train_hmc_conv: Hc 16, 8 points in one batch, warmup 5, 5 samples (batch_samples 6); conv_hmc_restate.E2E's step size and trajectory,
# with which a chain started at Uniform(-2, 2) stays short
E = M.E2E
N_POINTS, T_WARMUP, T_SAMPLES = 8, 5, 5
HISTORY_LISTS = ("eps", "L", "dH", "accept_prob", "accepted", "key")


def _bnn():
    from robustbnns_amd.model_bnn import BNN
    return BNN("mnist", E["Hc"], E["act"], "conv", "hmc", None, None, T_SAMPLES, T_WARMUP, (1, 28, 28), E["C"], step_size=E["step_size"],
               num_steps=E["num_steps"])


def _loader():
    x, y = M.e2e_data()
    return x[:N_POINTS], DataLoader(list(zip(x[:N_POINTS], y[:N_POINTS])), batch_size=N_POINTS, shuffle=False)


def _assert_same_history(a, b, what):
    for name in HISTORY_LISTS:
        assert a[name] == b[name], (what, name)
    assert torch.equal(a["m_inv"], b["m_inv"]), (what, "m_inv")


def test_train_hmc_conv_with_two_chains(tmp_path):
    from robustbnns_amd.conv_hmc import ConvLockstepHmc
    from robustbnns_amd.flat_params import state_shapes
    from robustbnns_amd.hmc import LOG_COLUMNS, initial_position, split_r_hat
    from robustbnns_amd.svi_train import draw_key
    x, loader = _loader()
    one = _bnn()
    one.train_hmc_conv(loader, DEV, rel_path=str(tmp_path) + "/one/")
    assert set(one.hmc_history) == {"eps", "L", "dH", "accept_prob", "accepted", "m_inv", "key", "resampled"}
    two, path = _bnn(), str(tmp_path) + "/two/"
    two.train_hmc_conv(loader, DEV, rel_path=path, num_chains=2)
    h = two.hmc_history
    # the same two chains again, from the same host draws (train_hmc_conv seeds itself): their stacks before the resampling, their logs
    probe = _bnn()
    x_batch, y_batch, batch_samples, q0, key = probe._hmc_prologue(loader, DEV)
    q0s, keys = [q0, initial_position(state_shapes(probe.basenet))], [key, draw_key()]
    assert batch_samples == T_SAMPLES + 1 and key == one.hmc_history["key"] == h["key"] and keys[1] == h["chains"][1]["key"] != key
    ls = ConvLockstepHmc(E["act"], (1, 28, 28), E["C"], q0s, probe.step_size, probe.num_steps, DEV, keys, batch_size=N_POINTS)
    stacks = ls.run(x_batch.to(DEV), y_batch.to(DEV).argmax(-1), batch_samples, T_WARMUP)
    from robustbnns_amd.conv_hmc import ConvHmcSampler
    s = ConvHmcSampler(E["act"], (1, 28, 28), E["C"], q0, probe.step_size, probe.num_steps, DEV, key, batch_size=N_POINTS)
    stack1 = s.run(x_batch.to(DEV), y_batch.to(DEV).argmax(-1), batch_samples, T_WARMUP)
    assert s.accepted_log == one.hmc_history["accepted"] and s.eps_log == one.hmc_history["eps"]
    for k, v in stack1.items():
        assert tuple(h["stack"][k].shape[:1]) == (2 * batch_samples,)
        assert _same(h["stack"][k][:batch_samples], v), f"chain 0 is not the num_chains = 1 chain: {k}"
        assert _same(h["stack"][k][batch_samples:], stacks[1][k]) and not _same(h["stack"][k][batch_samples:], v)
    _assert_same_history(h, {**one.hmc_history}, "chain 0 against num_chains = 1")
    assert len(h["chains"]) == 2 and h["chains"][0]["accepted"] == h["accepted"]
    assert set(h) == set(one.hmc_history) | {"stack", "chains", "r_hat_U"}
    U = ls.log[:, T_WARMUP:, LOG_COLUMNS.index("U_new")]
    assert tuple(U.shape) == (2, batch_samples) and h["r_hat_U"] == split_r_hat(U) and torch.isfinite(torch.tensor(h["r_hat_U"]))
    assert tuple(h["resampled"].shape) == (T_SAMPLES,) and int(h["resampled"].max()) < 2 * batch_samples
    print(f"[conv-hmc train_hmc_conv num_chains=2] chain 0 == the single chain's stack bit for bit; r_hat_U {h['r_hat_U']:.4f}; L of chain 0 "
          f"{h['L']}, of chain 1 {h['chains'][1]['L']}")
    assert len(glob.glob(os.path.join(path, two.name, "*.pt"))) == T_SAMPLES
    again = _bnn()
    again.load(DEV, rel_path=path)
    p0, p1 = two.forward(x.to(DEV), n_samples=T_SAMPLES), again.forward(x.to(DEV), n_samples=T_SAMPLES)
    assert torch.equal(p0, p1) and bool(torch.isfinite(p1).all()) and torch.allclose(p1.sum(-1), torch.ones(N_POINTS, device=DEV), atol=1e-5)
    with pytest.raises(ValueError, match="num_chains"):
        two.train_hmc_conv(loader, DEV, rel_path=path, num_chains=0)


def test_grouping_changes_no_bits(tmp_path):
    """num_chains = 3 in groups of 3 (one sampler), 1 (three, one after the other) and 2 (groups of 2 and 1): equal stacks and histories."""
    _, loader = _loader()
    runs = {}
    for group in (3, 1, 2):
        net = _bnn()
        net.train_hmc_conv(loader, DEV, rel_path=f"{tmp_path}/g{group}/", num_chains=3, group=group)
        runs[group] = net
    ref = runs[3].hmc_history
    assert len(ref["chains"]) == 3 and len({c["key"] for c in ref["chains"]}) == 3
    for group in (1, 2):
        h = runs[group].hmc_history
        for k in ref["stack"]:
            assert _same(h["stack"][k], ref["stack"][k]), (group, k)
        _assert_same_history(h, ref, f"group {group}")
        for a, b in zip(h["chains"], ref["chains"]):
            _assert_same_history(a, b, f"group {group}")
        assert h["r_hat_U"] == ref["r_hat_U"] and torch.equal(h["resampled"], ref["resampled"])
        for i in range(T_SAMPLES):
            assert all(torch.equal(runs[group].posterior.state_dict(i)[k], runs[3].posterior.state_dict(i)[k]) for k in M.KEYS), (group, i)
    default = _bnn()                                                           # group=None: everything fits the budget at this size
    default.train_hmc_conv(loader, DEV, rel_path=f"{tmp_path}/gd/", num_chains=3)
    _assert_same_history(default.hmc_history, ref, "the default group")
    assert all(_same(default.hmc_history["stack"][k], ref["stack"][k]) for k in ref["stack"])
