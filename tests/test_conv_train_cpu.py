"""Host tier of deterministic conv training (robustbnns_amd/conv_train.py, csrc/rbnn_conv_train.hip): the new entry points in the header, in
_hip.SIGNATURES and in the library under the unchanged ABI number, their host-side argument checks, the restatement (tests/conv_restate.py)
against itself, the inputs of the GPU tier against their own caps, the condition and the spread of the trajectory case, the guards, and the
new kernels' resources.  No HIP compute is called here."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

import conv_restate as CR
import nn_restate as NR
from robustbnns_amd import _hip, model_nn

pytestmark = pytest.mark.usefixtures("built_library")
NAMES = ["rbnn_conv_train_sizes", "rbnn_conv_train_forward", "rbnn_conv_weight_grads", "rbnn_conv_adam_step", "rbnn_conv_train_finalize"]
OK, ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED, ERR_ALIGN = 0, -1, -2, -3, -5


def test_new_entry_points_are_additive_under_abi_10():
    lib = _hip.load()
    header = open(_hip.HEADER_PATH).read()
    declared = set(re.findall(r"\b(rbnn_\w+)\s*\(", header))
    assert re.search(r"#define RBNN_ABI_VERSION 10\b", header) and _hip.ABI_VERSION == 10 and lib.rbnn_abi_version() == 10
    for name in NAMES:
        assert name in declared and name in _hip.SIGNATURES and hasattr(lib, name), name
    assert declared == set(_hip.SIGNATURES)


def _net(hidden=32, n_classes=10):
    net = _hip.ConvTrainNet()
    net.activation, net.in_channels, net.in_width, net.hidden, net.n_classes = 1, 1, 28, hidden, n_classes
    return net


def test_sizes_follow_the_flat_layout():
    lib, out = _hip.load(), _hip.ConvTrainBytes()
    for Hc, Cn, B in ((16, 10, 1), (48, 3, 65), (512, 10, 128)):
        assert lib.rbnn_conv_train_sizes(C.byref(_net(Hc, Cn)), B, C.byref(out)) == OK
        sd = CR.fresh_params("leaky", Hc, Cn, 0)
        assert list(sd) == CR.KEYS and out.n_params == sum(v.numel() for v in sd.values()) == 832 + 801 * Hc + 49 * Hc * Cn + Cn
        assert out.logits == out.dZ == 64 * B and out.ce == out.correct == 4 * B and out.P1 >= 4 * 4608 * B and out.st1 == 4608 * B
        assert out.Q2 == 4 * 49 * Hc * B and out.st2 == 49 * Hc * B and out.dO2 == 4 * 64 * Hc * B and out.dO1 == 4 * 32 * 576 * B
        assert out.part2 == 4 * min(B, 16) * Hc * 801 and out.part1 == 4 * min(B, 128) * 32 * 26
        assert 4 * 4608 * B <= out.partP <= 4 * 4608 * B * (Hc // 16)


def test_entry_points_validate_their_arguments_on_the_host():
    """Every refusal comes back as its status code before anything is launched (there is no device here to launch on)."""
    lib, out = _hip.load(), _hip.ConvTrainBytes()
    assert lib.rbnn_conv_train_sizes(None, 8, C.byref(out)) == ERR_NULL and lib.rbnn_conv_train_sizes(C.byref(_net()), 8, None) == ERR_NULL
    for field, bad, rc in (("hidden", 8, ERR_SHAPE), ("hidden", 0, ERR_SHAPE), ("hidden", 40, ERR_SHAPE), ("n_classes", 0, ERR_SHAPE), ("n_classes", 17, ERR_SHAPE),
                           ("activation", 4, ERR_UNSUPPORTED), ("activation", -1, ERR_UNSUPPORTED), ("in_channels", 3, ERR_UNSUPPORTED),
                           ("in_width", 32, ERR_UNSUPPORTED)):
        net = _net()
        setattr(net, field, bad)
        assert lib.rbnn_conv_train_sizes(C.byref(net), 8, C.byref(out)) == rc, (field, bad)
        assert lib.rbnn_conv_adam_step(C.byref(net), 1, 0.01, 0.9, 0.999, 1e-8, None) == rc, (field, bad)
    cifar = _net()
    cifar.in_channels, cifar.in_width = 3, 32
    assert lib.rbnn_conv_train_sizes(C.byref(cifar), 8, C.byref(out)) == ERR_UNSUPPORTED
    assert lib.rbnn_conv_train_sizes(C.byref(_net()), 0, C.byref(out)) == ERR_SHAPE
    # host memory stands in for the buffers: every call below is refused before a pointer is followed
    buf = (C.c_float * 4096)()
    base = C.addressof(buf)
    base += (-base) % 16
    net, ws = _net(), _hip.ConvTrainWs()
    fwd = lambda n, X, ldx, lab, B, w: lib.rbnn_conv_train_forward(C.byref(n), X, ldx, lab, B, C.byref(w) if w is not None else None, None)
    wg = lambda n, X, ldx, B, w: lib.rbnn_conv_weight_grads(C.byref(n), X, ldx, B, C.byref(w) if w is not None else None, None)
    assert fwd(net, base, 784, base, 4, ws) == ERR_NULL and wg(net, base, 784, 4, ws) == ERR_NULL                  # P, grad and the workspaces are NULL
    for name in ("P", "m", "v", "grad"):
        setattr(net, name, base)
    assert fwd(net, base, 784, base, 4, ws) == ERR_NULL and wg(net, base, 784, 4, ws) == ERR_NULL and fwd(net, base, 784, base, 4, None) == ERR_NULL
    for k in _hip.CONV_TRAIN_WS_KEYS:
        setattr(ws, k, base)
    assert fwd(net, None, 784, base, 4, ws) == ERR_NULL and fwd(net, base, 784, None, 4, ws) == ERR_NULL and wg(net, None, 784, 4, ws) == ERR_NULL
    for call in (lambda X, ldx, B: fwd(net, X, ldx, base, B, ws), lambda X, ldx, B: wg(net, X, ldx, B, ws)):
        assert call(base, 784, 0) == ERR_SHAPE and call(base, 784, -3) == ERR_SHAPE
        assert call(base, 780, 4) == ERR_SHAPE and call(base, 786, 4) == ERR_SHAPE                                   # below 784; not a multiple of 4
        assert call(base + 4, 784, 4) == ERR_ALIGN
    assert lib.rbnn_conv_adam_step(C.byref(net), 0, 0.01, 0.9, 0.999, 1e-8, None) == ERR_SHAPE
    assert lib.rbnn_conv_adam_step(C.byref(_net()), 1, 0.01, 0.9, 0.999, 1e-8, None) == ERR_NULL
    assert lib.rbnn_conv_train_finalize(None, 4, base, None) == ERR_NULL and lib.rbnn_conv_train_finalize(C.byref(ws), 4, None, None) == ERR_NULL
    assert lib.rbnn_conv_train_finalize(C.byref(_hip.ConvTrainWs()), 4, base, None) == ERR_NULL
    assert lib.rbnn_conv_train_finalize(C.byref(ws), 0, base, None) == ERR_SHAPE


@pytest.mark.parametrize("Hc,act,B,Cn", CR.GRAD_CASES)
def test_restatement_holds_against_itself_and_the_case_stays_inside_its_caps(Hc, act, B, Cn):
    """torch's own fp32 autograd meets the GPU tier's bar against the fp64 evaluation of the same case (per tensor 1e-5 max|fp64 gradient|,
    per-point CE, loss).  What the case leaves out is decided by the fp64 evaluation alone: at most one third of the pool at a kink or a
    pooling tie (so B points always remain; dropped points are never scored), at most 2 % of the scored points within the argmax margin."""
    c = CR.grad_case(Hc, act, B, Cn)
    ref, r32 = c["ref"], CR.autograd(c, act, torch.float32)
    assert c["n_pool"] == 3 * B + 8 and 3 * c["n_drop"] <= c["n_pool"] and len(c["lab"]) == B == len(c["x"])
    assert not bool(CR.discontinuous(c["x"], c["params"], act).any())
    assert ref["n_marginal"] <= 0.02 * B, ref["n_marginal"]
    assert int(c["lab"].max()) < Cn and int(c["lab"].min()) >= 0
    if B >= 8:
        assert 0 < int(ref["log1p"].sum()) < B                               # both branches of the head's CE
    worst = 0.0
    for k, g64 in ref["grad"].items():
        gmax = float(g64.abs().max())
        assert gmax > 0
        worst = max(worst, float((r32["grad"][k] - g64).abs().max()) / (1e-5 * gmax))
    e = float(((r32["ce"] - ref["ce"]).abs() / (1e-5 * ref["ce"].clamp_min(1.0))).max())
    print(f"[conv-restate Hc={Hc} {act} B={B} C={Cn}] torch fp32 vs fp64: worst gradient error {worst:.3f} x bar, per-point CE {e:.3f} x bar; dropped "
          f"{c['n_drop']} of {c['n_pool']} pool points; {ref['n_marginal']} marginal")
    assert worst <= 1.0 and e <= 1.0 and abs(r32["loss"] - ref["loss"]) <= 1e-5 * abs(ref["loss"])


def _regime(B, Hc, name):
    """(several units per slice, a last slice shorter than the others, one slice) of one GEMM's plan."""
    per, n = CR.slice_plan(B, Hc)[name]
    units = CR.plan_units(B, Hc)[name]
    assert n >= 1 and (n - 1) * per < units <= n * per, (B, Hc, name, per, n)       # the slices share out every unit, none is empty
    return per > 1, units % per != 0, n == 1


SHIPPED_SHAPES = [(128, 512), (100, 512), (100, 1024), (5000, 512), (5000, 1024)]   # (B, Hc) of the conv workloads: never run by a test


def test_slice_plan_regimes_are_reached_and_the_buffers_cover_the_plan():
    """1. The regime cases reach what conv_restate claims of them: the plans themselves, and for each of the three GEMMs a slice of several
    units, a ragged last slice and a slice of at least 32 stages (the fold) somewhere; for dP1 the one-slice plan too.
    2. The plan of every shipped shape lies in a regime some gradient case covers.  A regime is (several units per slice, one slice); a case
    with a ragged last slice covers the plan without one as well (the same walk, the clamp at K idle), never the other way round.
    3. rbnn_conv_train_sizes covers the plan of EVERY batch b <= B (the trainers reuse buffers sized for B at smaller batches, where dP1 takes
    more slices), for B in 1..600, 1000, 5000, 65536 and six Hc: a running maximum over b makes the check exhaustive, not a spread."""
    want = {(144, "tanh", 129, 10): {"dP1": (2, 5), "dK2": (9, 15), "dK1": (2, 65)}, (80, "relu", 300, 10): {"dP1": (2, 3), "dK2": (19, 16), "dK1": (3, 100)},
            (48, "leaky", 500, 3): {"dP1": (3, 1), "dK2": (32, 16), "dK1": (4, 125)}, (16, "sigm", 129, 2): {"dP1": (1, 1), "dK2": (9, 15), "dK1": (2, 65)}}
    assert list(want) == CR.REGIME_CASES and all(c in CR.GRAD_CASES for c in CR.REGIME_CASES)
    for (Hc, act, B, Cn), plan in want.items():
        assert CR.slice_plan(B, Hc) == plan, (Hc, B, CR.slice_plan(B, Hc))
    assert CR.plan_stages(129, 144) == {"dP1": 50, "dK2": 36, "dK1": 72} and CR.plan_stages(500, 48) == {"dP1": 75, "dK2": 128, "dK1": 144}
    assert -(-129 * CR.PP1 // CR.TILE_M) == 291 and (129 * CR.PP1) % CR.TILE_M and 144 % CR.TILE_M                   # ragged M tiles of dP1 and of dK2
    assert CR.plan_floats(129, 144) == {"partP": 5 * 129 * 144 * 32, "part2": 15 * 144 * 801, "part1": 65 * 32 * 26}
    for name in ("dP1", "dK2", "dK1"):
        regs = [_regime(B, Hc, name) for Hc, _, B, _ in CR.REGIME_CASES]
        assert any(r[0] for r in regs), f"{name}: no case with several units per slice"
        assert any(r[0] and r[1] for r in regs), f"{name}: no case with a ragged last slice"
        assert any(CR.plan_stages(B, Hc)[name] >= CR.FOLD_STAGES for Hc, _, B, _ in CR.REGIME_CASES), f"{name}: no case in which the fold fires"
    assert any(_regime(B, Hc, "dP1")[2] and _regime(B, Hc, "dP1")[0] for Hc, _, B, _ in CR.REGIME_CASES), "dP1: no one-slice plan of several groups"
    assert any(CR.plan_stages(B, Hc)["dP1"] >= 2 * CR.FOLD_STAGES for Hc, _, B, _ in CR.REGIME_CASES)                  # two folds in one slice
    assert any(CR.plan_stages(B, Hc)["dK2"] % CR.FOLD_STAGES == 0 for Hc, _, B, _ in CR.REGIME_CASES)                  # a fold on the last stage
    # 2. the shipped shapes
    for name in ("dP1", "dK2", "dK1"):
        covered = {(r[0], r[2]) for r in (_regime(B, Hc, name) for Hc, _, B, _ in CR.GRAD_CASES)}
        ragged = {(r[0], r[2]) for r in (_regime(B, Hc, name) for Hc, _, B, _ in CR.GRAD_CASES) if r[1]}
        for B, Hc in SHIPPED_SHAPES:
            several, rag, one = _regime(B, Hc, name)
            assert (several, one) in (ragged if rag else covered), f"{name} at B={B} Hc={Hc}: plan {CR.slice_plan(B, Hc)[name]} in a regime no case covers"
            if name == "dP1":
                assert one or several, (B, Hc)
    assert CR.slice_plan(128, 512)["dP1"] == (5, 7) and CR.slice_plan(100, 512)["dP1"] == (4, 8) and CR.slice_plan(5000, 512)["dP1"] == (32, 1)
    assert CR.slice_plan(5000, 512)["dK2"] == (313, 16) and CR.slice_plan(5000, 512)["dK1"] == (40, 125) and CR.slice_plan(128, 512)["dK2"] == (8, 16)
    # 3. the buffers
    lib, out = _hip.load(), _hip.ConvTrainBytes()
    Bs = list(range(1, 601)) + [1000, 5000, 65536]
    n_checked, tightest = 0, float("inf")
    for Hc in (16, 48, 80, 144, 512, 1024):
        need, b_at, run, b = {}, {"partP": 0, "part2": 0, "part1": 0}, {"partP": 0, "part2": 0, "part1": 0}, 0
        for B in Bs:
            while b < B:                                                   # the largest need of any batch up to B, and the batch that has it
                b += 1
                for k, v in CR.plan_floats(b, Hc).items():
                    if 4 * v > run[k]:
                        run[k], b_at[k] = 4 * v, b
            need[B] = dict(run)
            assert lib.rbnn_conv_train_sizes(C.byref(_net(Hc, 10)), B, C.byref(out)) == OK
            for k in ("partP", "part2", "part1"):
                assert getattr(out, k) >= need[B][k], f"{k} sized for B={B} at Hc={Hc} holds {getattr(out, k)} bytes; a batch of {b_at[k]} writes {need[B][k]}"
                tightest = min(tightest, getattr(out, k) / need[B][k])
                n_checked += 1
    print(f"[conv-restate slice plan] {len(CR.REGIME_CASES)} regime cases reach their plans; {len(SHIPPED_SHAPES)} shipped shapes in covered regimes; "
          f"{n_checked} buffer sizes cover every batch up to theirs (tightest: {tightest:.3f} x the need)")


def test_trajectory_case_meets_no_pooling_tie_and_has_a_small_spread():
    """The condition of the end-to-end GPU test, on the fp64 run: no batch point of any step within TIE of a pooling tie (tanh: no kink).  The
    spread then is rounding alone: every one of the four summation orders stays below 2e-5, a third of the least spread (7e-5 .. 3e-4) of runs
    that pass a tie."""
    r64, before, n_tie, spread, spreads = CR.traj_reference()
    per = -(-CR.TRAJ["N"] // CR.TRAJ["batch"])
    assert len(before) == CR.TRAJ["epochs"] * per and CR.TRAJ["act"] == "tanh" and CR.TRAJ["N"] % CR.TRAJ["batch"]
    print(f"[conv-restate trajectory seed {CR.TRAJ_SEED}] {len(before)} steps, {n_tie} batch points within {CR.TIE} of a pooling tie; spread {spread:.3e} "
          f"(per order: {', '.join(f'{s:.3e}' for s in spreads)}); {sum(r64.n_marginal)} marginal points")
    assert n_tie == 0
    assert len(spreads) == CR.TRAJ_ORDERS and 0 < min(spreads) and spread == max(spreads) < 2e-5


def test_guards_fire_with_nothing_constructed(monkeypatch):
    from torch.utils.data import DataLoader, TensorDataset
    from robustbnns_amd import conv_train
    launched = []
    monkeypatch.setattr(_hip, "HipKernels", lambda: launched.append(1))
    x, y = torch.rand(8, 1, 28, 28), torch.eye(10)[torch.arange(8)]
    loader = DataLoader(TensorDataset(x, y), batch_size=4)
    conv = model_nn.NN("mnist", (1, 28, 28), 10, 16, "leaky", "conv", 0.01, 1)
    fc = model_nn.NN("mnist", (1, 28, 28), 10, 16, "leaky", "fc", 0.01, 1)
    before = {k: v.clone() for k, v in conv.state_dict().items()}
    torch.manual_seed(5)
    rng = torch.get_rng_state()
    with pytest.raises(NotImplementedError, match="no CPU compute path"):
        conv.train_conv(loader, "cpu")
    with pytest.raises(NotImplementedError, match="no CPU compute path"):
        conv_train.ConvNnTrainer("leaky", (1, 28, 28), 10, conv.state_dict(), 0.01, "cpu")
    with pytest.raises(NotImplementedError, match="1x28x28"):
        conv_train.ConvNnTrainer("leaky", (3, 32, 32), 10, conv.state_dict(), 0.01, "cuda:0")
    conv.input_shape = (3, 32, 32)
    with pytest.raises(NotImplementedError, match="1x28x28"):
        conv.train_conv(loader, "cuda:0", seed=3, save=False)
    conv.input_shape = (1, 28, 28)
    with pytest.raises(ValueError, match="train"):
        fc.train_conv(loader, "cuda:0")
    with pytest.raises(NotImplementedError, match="conv"):
        conv.train(loader, "cuda:0")                                        # NN.train keeps refusing conv
    assert not launched and torch.equal(rng, torch.get_rng_state()) and not hasattr(conv, "device") and not hasattr(fc, "device")
    assert all(torch.equal(v, before[k]) for k, v in conv.state_dict().items())


def test_conv_training_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources as KR
    if not os.path.exists(KR.READELF):
        pytest.skip("llvm-readelf not in this image")
    res = {n: r for n, r in KR.kernel_resources().items()
           if re.search(r"::(conv_(head|reduce)_kernel\(|conv_(do2|wgrad_gemm|route1)_kernel<\d, false>|nn_(adam|finalize)_kernel<false>|"
                        r"train_gemm_kernel<false, false>)", n)}
    # head, reduce, adam, finalize (rbnn_nn_step.hpp's, for one net), do2 and route1 x 4 activations, the GEMM in its 3 modes, and the strided GEMM (dFw)
    assert len(res) == 4 + 8 + 3 + 1, sorted(res)
    bad = {n: (r["scratch"], r["spill_vgpr"]) for n, r in res.items() if r["scratch"] or r["spill_vgpr"]}
    assert not bad, bad
