"""Host tier of HMC over conv nets (robustbnns_amd/conv_hmc.py, BNN.train_hmc_conv, the rbnn_conv_hmc_* entry points of csrc/rbnn_hmc.hip): the six
names in the header, in _hip.SIGNATURES and in the library under the unchanged ABI number, their host-side argument checks, every refusal
with nothing loaded, the restatement (tests/conv_hmc_restate.py) against a finite difference of its own potential, the batch selection of the
GPU tier against its conditions, its bounds measured again, and the resources of the kernels a transition launches.  No HIP compute here."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

import conv_hmc_restate as M
import conv_restate as CR
import hmc_restate as HR
from robustbnns_amd import _hip
from robustbnns_amd.conv_train import CONV_KEYS

pytestmark = pytest.mark.usefixtures("built_library")
NAMES = ["rbnn_conv_hmc_sizes", "rbnn_conv_hmc_momentum", "rbnn_conv_hmc_leapfrog_update", "rbnn_conv_hmc_decide", "rbnn_conv_hmc_commit",
         "rbnn_conv_hmc_window_end"]
OK, ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED = 0, -1, -2, -3


def test_the_six_entry_points_are_additive_under_abi_10():
    lib = _hip.load()
    header = open(_hip.HEADER_PATH).read()
    declared = set(re.findall(r"\b(rbnn_\w+)\s*\(", header))
    assert re.search(r"#define RBNN_ABI_VERSION 10\b", header) and _hip.ABI_VERSION == 10 and lib.rbnn_abi_version() == 10
    for name in NAMES:
        assert name in declared and name in _hip.SIGNATURES and hasattr(lib, name), name
    assert declared == set(_hip.SIGNATURES)
    assert len(_hip.HMC_ST) == 13 and (HR.UNIF_KEY, HR.SEARCH_KEY) == (_hip.HMC_UNIF_KEY, _hip.HMC_SEARCH_KEY)      # no state entry, no key added
    assert M.KEYS == CONV_KEYS


def _net(hidden=16, n_classes=10, activation=1, in_channels=1, in_width=28):
    net = _hip.ConvSviTrainNet()
    net.activation, net.in_channels, net.in_width, net.hidden, net.n_classes = activation, in_channels, in_width, hidden, n_classes
    return net


def test_sizes_follow_the_flat_conv_layout():
    lib, nq, ne = _hip.load(), C.c_int64(0), C.c_int64(0)
    for Hc, Cn in ((16, 3), (48, 10), (1024, 10), (4096, 16)):
        numels = [int(torch.Size(s).numel()) for s in M.V.shapes_of(Hc, Cn).values()]
        assert lib.rbnn_conv_hmc_sizes(C.byref(_net(Hc, Cn)), C.byref(nq), C.byref(ne)) == sum(numels) == 832 + 801 * Hc + 49 * Hc * Cn + Cn
        assert ne.value == -(-sum(numels) // 256) and nq.value == -(-sum(-(-n // 4) for n in numels) // 256)     # one thread per quad of a tensor
    assert lib.rbnn_conv_hmc_sizes(C.byref(_net()), None, None) == 832 + 801 * 16 + 49 * 160 + 10                # both lengths are nullable


def test_entry_points_validate_their_arguments_on_the_host():
    """Every refusal comes back as its status code before anything is launched (there is no device here to launch on); no call below is valid."""
    lib = _hip.load()
    buf = torch.zeros(64, dtype=torch.float64)
    base = buf.data_ptr()
    chain = _hip.HmcChain()
    for name in _hip.HmcChain._pointers_:
        setattr(chain, name, base)
    chain.log_rows, chain.sample_rows = 2, 2
    ch = C.byref(chain)
    calls = {"momentum": lambda n, c=ch: lib.rbnn_conv_hmc_momentum(n, c, 1, 0, None),
             "update": lambda n, c=ch, phase=0: lib.rbnn_conv_hmc_leapfrog_update(n, c, phase, None),
             "decide": lambda n, c=ch, ce=base, B=4, i=0, mode=2: lib.rbnn_conv_hmc_decide(n, c, ce, B, 1, i, mode, 0, 0, None),
             "commit": lambda n, c=ch, w=0, row=-1: lib.rbnn_conv_hmc_commit(n, c, 0, w, row, None),
             "window_end": lambda n, c=ch, w=25: lib.rbnn_conv_hmc_window_end(n, c, w, None)}
    bad_nets = [(_net(in_width=32), ERR_UNSUPPORTED), (_net(in_channels=3), ERR_UNSUPPORTED), (_net(activation=-1), ERR_UNSUPPORTED),
                (_net(activation=4), ERR_UNSUPPORTED), (_net(hidden=24), ERR_SHAPE), (_net(hidden=0), ERR_SHAPE), (_net(hidden=4112), ERR_SHAPE),
                (_net(n_classes=0), ERR_SHAPE), (_net(n_classes=17), ERR_SHAPE)]
    for net, status in bad_nets:
        assert lib.rbnn_conv_hmc_sizes(C.byref(net), None, None) == status
        for name, call in calls.items():
            assert call(C.byref(net)) == status, (name, status)
    assert lib.rbnn_conv_hmc_sizes(None, None, None) == ERR_NULL
    good = _net()
    good.W = good.grad = base
    g = C.byref(good)
    empty = C.byref(_hip.HmcChain())                                           # every pointer NULL
    for name, call in calls.items():
        assert call(None) == ERR_NULL and call(g, None) == ERR_NULL and call(g, empty) == ERR_NULL, name
    for field in ("q_cur", "r", "m_inv", "k0_part", "p_part", "state"):        # one missing chain buffer is enough
        one = _hip.HmcChain()
        for name in _hip.HmcChain._pointers_:
            setattr(one, name, None if name == field else base)
        assert calls["momentum"](g, C.byref(one)) == ERR_NULL and calls["commit"](g, C.byref(one)) == ERR_NULL, field
    assert calls["update"](g, phase=-1) == ERR_UNSUPPORTED and calls["update"](g, phase=6) == ERR_UNSUPPORTED
    assert calls["decide"](g, mode=-1) == ERR_UNSUPPORTED and calls["decide"](g, mode=3) == ERR_UNSUPPORTED
    assert calls["decide"](g, ce=None) == ERR_NULL
    assert calls["decide"](g, B=0) == ERR_SHAPE and calls["decide"](g, i=-1) == ERR_SHAPE
    assert calls["commit"](g, row=2) == ERR_SHAPE and calls["commit"](g, w=-1) == ERR_SHAPE                      # a row behind the stack; a negative count
    assert calls["window_end"](g, w=1) == ERR_SHAPE
    chain.samples = None
    assert calls["commit"](g, row=0) == ERR_NULL
    chain.samples = base
    nowhere = _net()                                                           # the trajectory's buffers are the net's W / grad
    assert calls["update"](C.byref(nowhere)) == ERR_NULL and calls["commit"](C.byref(nowhere)) == ERR_NULL


def test_guards_fire_with_nothing_loaded_and_no_state_changed(monkeypatch, tmp_path):
    from torch.utils.data import DataLoader, TensorDataset
    from robustbnns_amd import conv_hmc, hmc
    from robustbnns_amd.grid_search_halfMoons import _train
    from robustbnns_amd.model_bnn import BNN
    launched = []
    monkeypatch.setattr(_hip, "HipKernels", lambda: launched.append(1))
    monkeypatch.setattr(_hip, "load", lambda: launched.append(2))
    monkeypatch.chdir(tmp_path)
    x, y = torch.rand(8, 1, 28, 28), torch.eye(10)[torch.arange(8)]
    loader = DataLoader(TensorDataset(x, y), batch_size=4)
    bnn = lambda arch, inf="hmc", shape=(1, 28, 28): BNN("mnist", 16, "leaky", arch, inf, 1 if inf == "svi" else None, 0.01 if inf == "svi" else None,
                                                         None if inf == "svi" else 5, None if inf == "svi" else 2, shape, 10)
    conv, fc, fc2, svi, cifar = bnn("conv"), bnn("fc"), bnn("fc2"), bnn("conv", "svi"), bnn("conv", shape=(3, 32, 32))
    q0 = M.start_position(16, 10)
    torch.manual_seed(5)
    rng = torch.get_rng_state()
    rel = str(tmp_path) + "/out/"
    with pytest.raises(ValueError, match="inference"):
        svi.train_hmc_conv(loader, "cuda:0", rel)
    for net in (fc, fc2):
        with pytest.raises(ValueError, match=r"\btrain_hmc\b"):
            net.train_hmc_conv(loader, "cuda:0", rel)
    with pytest.raises(NotImplementedError, match="no CPU compute path"):
        conv.train_hmc_conv(loader, "cpu", rel)
    with pytest.raises(NotImplementedError, match="1x28x28"):
        cifar.train_hmc_conv(loader, "cuda:0", rel)
    with pytest.raises(NotImplementedError, match="no CPU compute path"):
        conv_hmc.ConvHmcSampler("leaky", (1, 28, 28), 10, q0, 0.01, 10, "cpu", 1)
    with pytest.raises(NotImplementedError, match="1x28x28"):
        conv_hmc.ConvHmcSampler("leaky", (3, 32, 32), 10, q0, 0.01, 10, "cuda:0", 1)
    # the pinned refusals still raise, and name the method that samples a conv chain
    for call in (lambda: conv.train_hmc(loader, "cuda:0", rel), lambda: hmc.HmcSampler("conv", "leaky", (1, 28, 28), 10, q0, 0.01, 10, "cuda:0", 1),
                 lambda: hmc.LockstepHmc("conv", "leaky", (1, 28, 28), 10, [q0], 0.01, 10, "cuda:0", [1]),
                 lambda: _train(16, "leaky", "conv", "hmc", None, None, 5, 5, 16, 1, rel, "cuda:0", x_train=x, y_train=y)):
        with pytest.raises(NotImplementedError, match="train_hmc_conv"):
            call()
    with pytest.raises(NotImplementedError, match=r"train_hmc\b.*train_hmc_conv"):
        conv.train_conv(loader, "cuda:0", rel)
    with pytest.raises(NotImplementedError, match="train_hmc_conv"):
        conv.train(loader, "cuda:0", rel)
    assert not launched and torch.equal(rng, torch.get_rng_state())
    for net in (conv, fc, fc2, svi, cifar):
        assert not hasattr(net, "device") and not hasattr(net, "hmc_history") and net.svi_loc is None and net.posterior is None
    assert not os.listdir(tmp_path)


@pytest.mark.parametrize("case,met", list(zip(M.LEAP_CASES, M.SELECTION)), ids=lambda v: "-".join(str(e) for e in v))
def test_batch_selection_keeps_its_conditions(case, met):
    """choose_batch on a leapfrog case: the loop ends within MAX_ROUNDS rounds, at most two thirds of the pool is dropped, B clean points remain
    (none discontinuous at any of the L + 1 positions of the fp64 trajectory, checked again here), and the rounds / drops are the recorded ones."""
    Hc, act, B, Cn, L, eps = case
    c = M.choose_batch(*case)
    print(f"[conv-hmc selection {case}] rounds {c['rounds']}  dropped {c['dropped']} / {c['pool']}")
    assert c["clean"] and c["rounds"] <= M.MAX_ROUNDS == 16 and c["pool"] == 6 * B + 16 and 3 * c["dropped"] <= 2 * c["pool"]
    assert len(c["x"]) == len(c["lab"]) == B and 0 <= int(c["lab"].min()) and int(c["lab"].max()) < Cn
    assert (c["rounds"], c["dropped"], c["pool"]) == met
    rs = M.Restatement(act, c["q0"], c["x"], c["lab"], eps, L, M.LEAP_KEY)
    q, r, g = rs.q, c["r0"], rs.g
    assert torch.equal(r, rs.momentum(M.LEAP_KEY, 0))
    for step in range(L + 1):
        assert not bool(CR.discontinuous(c["x"], rs.unflat(q), act).any()), step
        q, r, g, _ = rs.leapfrog(q, r, g, 1)


def test_cases_cover_what_they_are_chosen_for():
    Hcs, acts, Bs, Cs = (set(c[i] for c in M.LEAP_CASES) for i in range(4))
    assert Hcs == {16, 48} and acts == {"relu", "leaky", "sigm", "tanh"} and {1, 5, 65} <= Bs and {3, 10} <= Cs
    assert (48, "leaky", 65, 3) not in {c[:4] for c in M.LEAP_CASES}
    assert [k for _, _, k in HR.windows(M.RUN["warmup"])] == ["start", "middle", "end"]


def test_bounds_are_four_times_the_restatements_own_fp32_deviation():
    """MEASURED_FP32 measured again, on the CPU (torch, never the code under test).  The leapfrog figures do not depend on torch's thread
    count; U, K and dH are fp32 sums over 21 514 elements whose order does (conv_hmc_restate records the worst of five thread counts), so
    their lower edge is a quarter of the record, not a half."""
    w = M.measure()
    print(f"[conv-hmc bounds] measured {w}  recorded {M.MEASURED_FP32}")
    assert M.FACTOR == 4.0 and all(M.BOUND[k] == 4.0 * v for k, v in M.MEASURED_FP32.items())
    for name, low in (("leapfrog_q", 0.5), ("leapfrog_r", 0.5), ("U", 0.25), ("K", 0.25), ("dH", 0.25)):
        assert low * M.MEASURED_FP32[name] <= w[name] <= 1.01 * M.MEASURED_FP32[name], (name, w[name])
    _, _, acc = M.transition_case(*M.TRANSITION_CASES[0])
    _, _, rej = M.transition_case(*M.TRANSITION_CASES[1])
    assert acc["accepted"] and not rej["accepted"]
    # both decisions rest on margins far above the dH bound: |dH - (-log u)| in units of the bound times the energy scale
    import math
    for rec in (acc, rej):
        assert abs(rec["dH"] + math.log(rec["u"])) > 100 * M.BOUND["dH"] * HR.energy_scale(rec)


def test_end_to_end_case_is_one_where_an_fp32_forward_can_meet_the_forward_bar():
    """The rule behind conv_hmc_restate.E2E's data seed, on the reference alone: at the fp64 replay's stack torch's own fp32 forward on the
    CPU is within half the 1e-5 forward bar at this seed and at no smaller one.  The replay's trajectories stay short (the GPU test's cost)."""
    for seed in range(M.E2E["seed"] + 1):
        rs, stack, x = M.e2e_replay(seed)
        dev = M.torch_fp32_forward_deviation(stack, x, M.E2E["act"])
        print(f"[conv-hmc e2e data seed {seed}] torch fp32 forward vs fp64 at the replay's stack: {dev:.2e}; L {[r['L'] for r in rs.log]}")
        assert (dev <= 0.5 * HR.FORWARD_BAR) == (seed == M.E2E["seed"]), (seed, dev)
    assert len(rs.log) == M.E2E["warmup"] + 2 and max(r["L"] for r in rs.log) <= 8 and any(r["accepted"] for r in rs.log[M.E2E["warmup"]:])
    assert tuple(stack["model.7.weight"].shape) == (M.E2E["n_samples"], M.E2E["C"], 49 * M.E2E["Hc"])


def test_potential_gradient_is_the_finite_difference_of_U():
    """dCE/dW + q of the restatement against the central difference (U(q + h e_i) - U(q - h e_i)) / 2h in fp64, at three coordinates of each
    of the six tensors, on the tie-free batch of the first leapfrog case (tanh: U is smooth there).  h = 1e-5: truncation h^2 U''' / 6 is
    below 1e-9 at these scales and the roundoff of the difference 2 ulp(U) / 2h = 1e-9; the bar is 1e-6 of max(1, largest |gradient|)."""
    case = M.LEAP_CASES[0]
    c = M.choose_batch(*case)
    rs = M.Restatement(case[1], c["q0"], c["x"], c["lab"], case[5], case[4], M.LEAP_KEY)
    grad = rs.g + rs.q
    h, off, worst = 1e-5, 0, 0.0
    scale = max(1.0, float(grad.abs().max()))
    for k in M.KEYS:
        n = int(torch.Size(rs.shapes[k]).numel())
        for i in sorted({off, off + n // 2, off + n - 1}):
            e = torch.zeros_like(rs.q)
            e[i] = h
            fd = (rs.potential(rs.q + e)[0] - rs.potential(rs.q - e)[0]) / (2 * h)
            worst = max(worst, abs(fd - float(grad[i])) / scale)
        off += n
    assert off == rs.q.numel()
    print(f"[conv-hmc restatement] grad U vs central differences at 3 coordinates of each tensor: worst {worst:.2e} of {scale:.3f}")
    assert worst <= 1e-6


def test_momentum_restatement_divides_the_flat_draw_by_the_root_of_the_inverse_mass():
    case = M.LEAP_CASES[1]                                                     # C = 3: the bias tensor is a partial quad
    c = M.choose_batch(*case)
    rs = M.Restatement(case[1], c["q0"], c["x"], c["lab"], case[5], case[4], M.LEAP_KEY)
    eps = rs.momentum(7, 3)
    ref = torch.cat([v[0].reshape(-1) for v in M.V.draw_eps(rs.shapes, 7, 3).values()])
    assert torch.equal(eps, ref)
    rs.m_inv = 0.5 + torch.rand(rs.q.numel(), dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    assert torch.equal(rs.momentum(7, 3), ref / torch.sqrt(rs.m_inv)) and abs(rs.kinetic(rs.momentum(7, 3)) - float(0.5 * (ref * ref).sum())) < 1e-9


def test_kernels_of_a_conv_hmc_transition_use_no_scratch():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources as KR
    if not os.path.exists(KR.READELF):
        pytest.skip("llvm-readelf not in this image")
    step = (r"conv1_pool_kernel<\d, rbnn_conv_shared::Geo<1, 28>, 0>|conv2_pool_kernel<\d, rbnn_conv_shared::Geo<1, 28> >|::conv_fc_kernel\(|::conv_(head|reduce)_kernel\(|"
            r"::conv_(do2|wgrad_gemm|route1)_kernel<\d, false>|::train_gemm_kernel<false, false>|::hmc_(momentum|update|decide|commit|window_end)_kernel\(")
    res = {n: r for n, r in KR.kernel_resources().items() if re.search(step, n)}
    # conv1 / conv2 x 4 activations, the Linear, the head, the strided GEMM (dFw), do2 and route1 x 4, the conv GEMM in 3 modes, the partial
    # sums' reduction, and the chain's five kernels
    assert len(res) == 8 + 1 + 1 + 1 + 8 + 3 + 1 + 5, sorted(res)
    bad = {n: (r["scratch"], r["spill_vgpr"]) for n, r in res.items() if r["scratch"] or r["spill_vgpr"]}
    assert not bad, bad
