"""Host tier of conv SVI guides in lockstep (robustbnns_amd/conv_svi_train.ConvLockstepSvi, model_bnn.train_conv_svi_lockstep, the
rbnn_conv_svi_guides_* entry points of csrc/rbnn_conv_train.hip): the new names in the header, in _hip.SIGNATURES and in the library under the
unchanged ABI number, the host-side argument checks of every entry point in their documented order, the sizes (linear in K, the single guide's
at K = 1), the group size against a hand-computed budget, the tensor-major layout and the schedule on the CPU, the guards, the pinned refusals
of the fc forms, and the new kernels' resources.  No HIP compute is called here."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

import conv_svi_restate as V
from robustbnns_amd import _hip, model_bnn

pytestmark = pytest.mark.usefixtures("built_library")
NAMES = ["rbnn_conv_svi_guides_" + n for n in ("sizes", "draw", "gradient", "adam_step", "accuracy", "finalize")]
OK, ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED, ERR_ALIGN = 0, -1, -2, -3, -5
ADAM = (0.9, 0.999, 1e-8, None)
S = 10


def test_new_entry_points_are_additive_under_abi_10():
    lib = _hip.load()
    header = open(_hip.HEADER_PATH).read()
    declared = set(re.findall(r"\b(rbnn_\w+)\s*\(", header))
    assert re.search(r"#define RBNN_ABI_VERSION 10\b", header) and _hip.ABI_VERSION == 10 and lib.rbnn_abi_version() == 10
    for name in NAMES:
        assert name in declared and name in _hip.SIGNATURES and hasattr(lib, name), name
    assert declared == set(_hip.SIGNATURES)
    for struct in ("rbnn_conv_svi_guides_net", "rbnn_conv_svi_guides_ws", "rbnn_conv_svi_guides_bytes"):
        assert re.search(r"\}\s*" + struct + r"\s*;", header) and struct in _hip.STRUCTS.values(), struct
    assert _hip.CONV_SVI_LOCKSTEP_WS_KEYS[:15] == _hip.CONV_ENS_WS_KEYS
    assert _hip.CONV_SVI_LOCKSTEP_WS_KEYS[15:] == ("acc_W", "acc_P", "acc_P1", "acc_st1", "acc_Q2", "acc_st2", "Psum")
    assert [n for n, _ in _hip.ConvSviLockstepNet._fields_][:6] == ["activation", "in_channels", "in_width", "hidden", "n_classes", "n_guides"]
    assert _hip.ConvSviLockstepNet._pointers_ == ("loc", "raw", "sigma", "m_loc", "v_loc", "m_raw", "v_raw", "W", "grad", "kl_part", "stats", "keys")
    assert _hip.SVI_MULTI_ACC_SAMPLES == S


def _net(hidden=32, n_classes=10, guides=3):
    net = _hip.ConvSviLockstepNet()
    net.activation, net.in_channels, net.in_width, net.hidden, net.n_classes, net.n_guides = 1, 1, 28, hidden, n_classes, guides
    net.part_stride = 1 << 20
    return net


def _single(hidden, n_classes):
    net = _hip.ConvSviTrainNet()
    net.activation, net.in_channels, net.in_width, net.hidden, net.n_classes = 1, 1, 28, hidden, n_classes
    return net


def _calls(lib):
    """name -> f(net, active, ws, base, **overrides): every device entry point with host memory standing in for the device arrays."""
    ref = lambda x: C.byref(x) if x is not None else None
    return {
        "draw": lambda n, act, w, b: lib.rbnn_conv_svi_guides_draw(ref(n), act, 0, None),
        "gradient": lambda n, act, w, b, X="b", ldx=784, n_rows=8, lab="b", rows="b", B=4: lib.rbnn_conv_svi_guides_gradient(
            ref(n), b if X == "b" else X, ldx, n_rows, b if lab == "b" else lab, b if rows == "b" else rows, B, ref(w), None),
        "adam_step": lambda n, act, w, b, step=1, lr="b": lib.rbnn_conv_svi_guides_adam_step(ref(n), act, 0, step, b if lr == "b" else lr, *ADAM),
        "accuracy": lambda n, act, w, b, B=4: lib.rbnn_conv_svi_guides_accuracy(ref(n), act, B, 0, 0, ref(w), None),
        "finalize": lambda n, act, w, b, B=4, slot=None, log=None, log_rows=0: lib.rbnn_conv_svi_guides_finalize(ref(n), act, ref(w), 1, B, slot, log,
                                                                                                              log_rows, None),
    }


def test_every_entry_point_refuses_bad_arguments_on_the_host_in_the_documented_order():
    """NULL net, then the descriptor (geometry / activation: UNSUPPORTED; hidden, classes, K: SHAPE), then NULL pointers, then shapes, then
    alignment; every refusal comes back as its status code before anything is launched (there is no device here to launch on)."""
    lib, out = _hip.load(), _hip.ConvSviLockstepBytes()
    calls = _calls(lib)
    buf = (C.c_float * 4096)()
    base = C.addressof(buf)
    base += (-base) % 16
    assert lib.rbnn_conv_svi_guides_sizes(None, 8, C.byref(out)) == ERR_NULL and lib.rbnn_conv_svi_guides_sizes(C.byref(_net()), 8, None) == ERR_NULL
    for name, f in calls.items():
        assert f(None, base, _hip.ConvSviLockstepWs(), base) == ERR_NULL, name
    # the descriptor is judged before any pointer: every pointer is NULL here
    for field, bad, rc in (("activation", 4, ERR_UNSUPPORTED), ("activation", -1, ERR_UNSUPPORTED), ("in_channels", 3, ERR_UNSUPPORTED),
                           ("in_width", 32, ERR_UNSUPPORTED), ("hidden", 8, ERR_SHAPE), ("hidden", 40, ERR_SHAPE), ("hidden", 4112, ERR_SHAPE),
                           ("n_classes", 0, ERR_SHAPE), ("n_classes", 17, ERR_SHAPE), ("n_guides", 0, ERR_SHAPE), ("n_guides", -2, ERR_SHAPE),
                           ("n_guides", 6554, ERR_SHAPE)):
        net = _net()
        setattr(net, field, bad)
        assert lib.rbnn_conv_svi_guides_sizes(C.byref(net), 8, C.byref(out)) == rc, (field, bad)
        for name, f in calls.items():
            assert f(net, None, None, None) == rc, (name, field, bad)
    assert lib.rbnn_conv_svi_guides_sizes(C.byref(_net(guides=6553)), 8, C.byref(out)) == OK
    # NULL pointers come before shapes: B = 0 with something missing is still ERR_NULL
    net, ws = _net(), _hip.ConvSviLockstepWs()
    for name, f in calls.items():
        assert f(net, base, ws, base) == ERR_NULL, name                       # the net's buffers
        assert f(net, base, None, base) == ERR_NULL or name in ("draw", "adam_step"), name
    for k in net._pointers_:
        setattr(net, k, base)
    for name, f in calls.items():
        assert f(net, None, ws, base) == ERR_NULL or name == "gradient", name   # active
    for name in ("gradient", "accuracy", "finalize"):
        assert calls[name](net, base, ws, base) == ERR_NULL, name                  # the workspaces
        assert calls[name](net, base, ws, base, B=0) == ERR_NULL, name
    for k in _hip.CONV_SVI_LOCKSTEP_WS_KEYS:
        setattr(ws, k, base)
    g = calls["gradient"]
    assert g(net, base, ws, base, X=None) == ERR_NULL and g(net, base, ws, base, lab=None) == ERR_NULL and g(net, base, ws, base, rows=None) == ERR_NULL
    assert calls["adam_step"](net, base, ws, base, lr=None) == ERR_NULL
    assert calls["finalize"](net, base, ws, base, slot=base, log=None) == ERR_NULL
    for k in ("Xs", "partP", "ce"):
        setattr(ws, k, None)
        assert g(net, base, ws, base) == ERR_NULL, k
        setattr(ws, k, base)
    for k in ("acc_W", "acc_st2", "Psum", "Xs"):
        setattr(ws, k, None)
        assert calls["accuracy"](net, base, ws, base) == ERR_NULL, k
        setattr(ws, k, base)
    # shapes
    for B in (0, -3, 65537):
        for name in ("gradient", "accuracy", "finalize"):
            assert calls[name](net, base, ws, base, B=B) == ERR_SHAPE, (name, B)
        assert lib.rbnn_conv_svi_guides_sizes(C.byref(net), B, C.byref(out)) == ERR_SHAPE
    big = _net(guides=6553)
    for k in big._pointers_:
        setattr(big, k, base)
    assert 6553 * 641 > 2 ** 22 >= 6553 * 640
    assert lib.rbnn_conv_svi_guides_sizes(C.byref(big), 641, C.byref(out)) == ERR_SHAPE and lib.rbnn_conv_svi_guides_sizes(C.byref(big), 640, C.byref(out)) == OK
    for name in ("gradient", "accuracy", "finalize"):
        assert calls[name](big, base, ws, base, B=641) == ERR_SHAPE, name             # K B past 2^22
    assert g(net, base, ws, base, ldx=780) == ERR_SHAPE and g(net, base, ws, base, ldx=786) == ERR_SHAPE and g(net, base, ws, base, n_rows=0) == ERR_SHAPE
    assert calls["adam_step"](net, base, ws, base, step=0) == ERR_SHAPE
    assert calls["finalize"](net, base, ws, base, slot=base, log=base, log_rows=-1) == ERR_SHAPE
    net.part_stride = 1                                                            # below the n_partials of this shape
    assert calls["adam_step"](net, base, ws, base) == ERR_SHAPE and calls["finalize"](net, base, ws, base) == ERR_SHAPE
    net.part_stride = 1 << 20
    # alignment comes last
    assert g(net, base, ws, base, X=base + 4) == ERR_ALIGN
    for k in ("Xs", "dO1", "part1"):
        setattr(ws, k, base + 4)
        assert g(net, base, ws, base) == ERR_ALIGN, k
        setattr(ws, k, base)
    for k in ("acc_W", "acc_P", "acc_Q2", "Psum", "Xs"):
        setattr(ws, k, base + 4)
        assert calls["accuracy"](net, base, ws, base) == ERR_ALIGN, k
        assert calls["accuracy"](net, base, ws, base, B=0) == ERR_SHAPE, k           # the shape is judged before the alignment
        setattr(ws, k, base)
    net.W = base + 4
    assert g(net, base, ws, base) == ERR_ALIGN and g(net, base, ws, base, ldx=780) == ERR_SHAPE
    net.W = base


@pytest.mark.parametrize("Hc", [16, 48])
def test_sizes_are_linear_in_k_and_the_single_guides_at_k_1(Hc):
    lib, one, single, n_part = _hip.load(), _hip.ConvSviLockstepBytes(), _hip.ConvTrainBytes(), C.c_int64(0)
    for Cn, B in ((10, 1), (3, 65), (10, 129)):
        assert lib.rbnn_conv_svi_guides_sizes(C.byref(_net(Hc, Cn, 1)), B, C.byref(one)) == OK
        assert lib.rbnn_conv_svi_train_sizes(C.byref(_single(Hc, Cn)), B, C.byref(n_part), C.byref(single)) == OK
        assert one.n_params == single.n_params == 832 + 801 * Hc + 49 * Hc * Cn + Cn and one.n_partials == n_part.value
        for k in _hip.CONV_TRAIN_WS_KEYS:
            assert getattr(one, k) == getattr(single, k), k
        assert one.Xs == 4 * 784 * B and one.labels == 4 * B and one.Psum == 4 * 16 * B
        # the accuracy forward's: rbnn_conv_workspace_query's for S samples of B points, and S weight sets
        F = 49 * Hc
        assert (one.acc_W, one.acc_P, one.acc_P1, one.acc_st1, one.acc_Q2, one.acc_st2) == (
            4 * S * one.n_params, 4 * 16 * S * B, 24576 * S * B, 4608 * S * B, 4 * F * S * B, F * S * B)
        for K in (2, 7, 33):
            out = _hip.ConvSviLockstepBytes()
            assert lib.rbnn_conv_svi_guides_sizes(C.byref(_net(Hc, Cn, K)), B, C.byref(out)) == OK
            assert out.n_params == one.n_params and out.n_partials == one.n_partials
            for k in _hip.CONV_SVI_LOCKSTEP_WS_KEYS:
                assert getattr(out, k) == K * getattr(one, k), (k, K)


def test_guide_group_fits_a_hand_computed_budget(monkeypatch):
    """conv-1024, 10 classes, B = 128: one guide's bytes by hand from the documented shapes (dK2 in 16 slices, dK1 in 128, dP1's partial sums
    capped at 2048 tiles of 64 x 32), the accuracy forward's the large term; the helper divides the budget by it."""
    from robustbnns_amd.conv_svi_train import conv_svi_lockstep_group
    Hc, Cn, B = 1024, 10, 128
    n = 832 + 801 * Hc + 49 * Hc * Cn + Cn
    F = 49 * Hc
    point = 4 * 784 + 4 + 4 * 16 + 24576 + 4608 + 4 * F + F + 4 * 16 + 4 + 4 + 4 * Hc * 64 + 4 * 32 * 576      # Xs .. dO1 per point
    parts = 4 * 16 * Hc * 801 + 4 * 128 * 32 * 26 + 4 * 2048 * 64 * 32                                         # part2, part1, partP
    acc = 4 * S * n + S * B * (4 * 16 + 24576 + 4608 + 4 * F + F) + 4 * 16 * B
    per = B * point + parts + acc + 9 * 4 * n
    assert acc > 0.6 * per                                                                                      # the large term
    monkeypatch.delenv("RBNN_CONV_WS_GB", raising=False)
    assert conv_svi_lockstep_group("leaky", 16, 10, 100, B) == 100
    assert conv_svi_lockstep_group("leaky", Hc, Cn, 1000, B) == int(48 * 2 ** 30 // per)
    assert conv_svi_lockstep_group("leaky", Hc, Cn, 100, B, budget_gb=4.0) == int(4 * 2 ** 30 // per) >= 3
    monkeypatch.setenv("RBNN_CONV_WS_GB", "0.001")
    assert conv_svi_lockstep_group("leaky", Hc, Cn, 100, B) == 1
    monkeypatch.setenv("RBNN_CONV_WS_GB", "2")
    g = conv_svi_lockstep_group("leaky", Hc, Cn, 100, B)
    assert g * per <= 2 * 2 ** 30 < (g + 1) * per
    assert conv_svi_lockstep_group("leaky", 16, 10, 10 ** 6, 1, budget_gb=10 ** 6) == 6553                      # never past the grid's limit


def test_trainer_layout_is_tensor_major_and_the_schedule_marks_finished_guides(monkeypatch):
    """ConvLockstepSvi's flat order on the CPU with the kernels' handle replaced: unflat(buf, k) returns guide k's tensors, block t holds the
    guides' tensor t one after the other, sigma = softplus(raw); the schedule of epochs (1, 3, 2) over 20 points at B = 8."""
    from robustbnns_amd import conv_svi_train as M

    class _Lib:
        @staticmethod
        def rbnn_conv_svi_guides_sizes(net, B, out):
            return _hip.load().rbnn_conv_svi_guides_sizes(net, B, out)

    class _K:
        lib = _Lib()

    monkeypatch.setattr(_hip, "HipKernels", _K)
    monkeypatch.setattr(M, "check_conv_trainable", lambda *a: None)
    monkeypatch.setattr(_hip, "CONV_SVI_LOCKSTEP_WS_KEYS", ("Psum",))
    guides = [V.guide(16, 10, s) for s in (1, 2, 3)]
    tr = M.ConvLockstepSvi("leaky", (1, 28, 28), 10, [g[0] for g in guides], [g[1] for g in guides], [0.01, 0.02, 0.03], "cpu", [5, 6, 2 ** 64 - 1], 4)
    assert tr.K == 3 and tuple(tr.loc.shape) == (3 * tr.n_params,) and tuple(tr.stats.shape) == (3, 3) and tr.keys_t.tolist() == [5, 6, -1]
    assert tuple(tr.acc_W.shape) == (30 * tr.n_params,) and tr.lr_t.dtype == torch.float64
    off = 0
    for key in V.KEYS:
        size = guides[0][0][key].numel()
        for k in range(3):
            assert torch.equal(tr.unflat(tr.loc, k)[key], guides[k][0][key]) and torch.equal(tr.unflat(tr.raw, k)[key], guides[k][1][key]), (key, k)
            assert torch.equal(tr.loc[off + k * size:off + (k + 1) * size], guides[k][0][key].reshape(-1)), (key, k)
            # (the CPU's vectorised softplus rounds the lanes of a vector and its scalar tail differently: an ulp, not bits, on this tier)
            assert torch.allclose(tr.unflat(tr.sigma, k)[key], torch.nn.functional.softplus(guides[k][1][key]), rtol=1e-6, atol=0), (key, k)
        off += 3 * size
    sch = M.ConvLockstepSvi.schedule(20, (1, 3, 2), 8)
    assert tuple(sch["active"].shape) == (9, 3) and sch["active"].dtype == torch.int32
    assert sch["active"].T.tolist() == [[1] * 3 + [0] * 6, [1] * 9, [1] * 6 + [0] * 3]
    assert sch["count"].max(1).values.tolist() == [8, 8, 4] * 3 and sch["slot"][:, 1].tolist() == [-1, -1, 0, -1, -1, 1, -1, -1, 2]
    assert sch["slot"][:, 0].tolist() == [-1, -1, 0] + [-1] * 6
    with pytest.raises(ValueError, match="share one point count"):
        M.ConvLockstepSvi.schedule([20, 19, 20], (1, 1, 1), 8)
    with pytest.raises(ValueError, match="set_data"):
        tr.step(torch.zeros(3, 4, dtype=torch.int32))
    for bad in (dict(raws=[guides[0][1]]), dict(keys=[1]), dict(lrs=[0.1, 0.2]), dict(batch_size=0)):
        kw = dict(locs=[g[0] for g in guides], raws=[g[1] for g in guides], lrs=0.01, keys=[1, 2, 3], batch_size=4)
        kw.update(bad)
        with pytest.raises(ValueError):
            M.ConvLockstepSvi("leaky", (1, 28, 28), 10, kw["locs"], kw["raws"], kw["lrs"], "cpu", kw["keys"], kw["batch_size"])
    other = V.guide(32, 10, 4)
    with pytest.raises(ValueError, match="another net shape"):
        M.ConvLockstepSvi("leaky", (1, 28, 28), 10, [guides[0][0], other[0]], [guides[0][1], other[1]], 0.01, "cpu", [1, 2], 4)


def _bnn(arch="conv", inference="svi", epochs=1, lr=0.01, hidden=16, shape=(1, 28, 28)):
    return model_bnn.BNN("mnist", hidden, "leaky", arch, inference, epochs, lr, 5, 5, shape, 10)


def test_train_conv_svi_lockstep_refuses_up_front_and_touches_nothing(monkeypatch):
    launched = []
    monkeypatch.setattr(_hip, "HipKernels", lambda: launched.append(1))
    monkeypatch.setattr(_hip, "load", lambda: launched.append(2))
    x, y = torch.rand(8, 1, 28, 28), torch.eye(10)[torch.arange(8)]
    nets = {"a": _bnn(), "b": _bnn(lr=0.02), "hmc": _bnn(inference="hmc"), "fc": _bnn(arch="fc"), "wide": _bnn(hidden=32, lr=0.03),
            "cifar": _bnn(shape=(3, 32, 32), lr=0.04), "twin": _bnn()}
    torch.manual_seed(5)
    rng = torch.get_rng_state()
    T = model_bnn.train_conv_svi_lockstep
    with pytest.raises(NotImplementedError, match="SVI only.*train_hmc_conv"):
        T([nets["a"], nets["hmc"]], x, y, "cuda:0")
    with pytest.raises(ValueError, match="conv architecture.*'fc'.*train_svi_lockstep"):
        T([nets["a"], nets["fc"]], x, y, "cuda:0")
    with pytest.raises(NotImplementedError, match="no CPU compute path"):
        T([nets["a"], nets["b"]], x, y, "cpu")
    with pytest.raises(NotImplementedError, match="1x28x28"):
        T([nets["a"], nets["cifar"]], x, y, "cuda:0")
    with pytest.raises(ValueError, match="share one net shape"):
        T([nets["a"], nets["wide"]], x, y, "cuda:0")
    with pytest.raises(ValueError, match="overwrite each other"):
        T([nets["a"], nets["b"], nets["twin"]], x, y, "cuda:0")
    with pytest.raises(ValueError, match="at least one net"):
        T([], x, y, "cuda:0")
    with pytest.raises(ValueError, match="group >= 1"):
        T([nets["a"], nets["b"]], x, y, "cuda:0", group=0)
    assert not launched and torch.equal(rng, torch.get_rng_state())
    for net in nets.values():
        assert net.svi_loc is None and net.svi_scale is None and not hasattr(net, "device") and not hasattr(net, "training_history")


def test_the_fc_forms_keep_refusing_conv_nets_as_before():
    from robustbnns_amd.svi_train import LockstepSvi
    loc, raw = V.guide(16, 10, 0)
    with pytest.raises(NotImplementedError, match=r"SVI training covers fc and fc2, not 'conv'"):
        LockstepSvi("conv", "leaky", (1, 28, 28), 10, [loc], [raw], 0.01, "cuda:0", [1])
    x, y = torch.rand(8, 1, 28, 28), torch.eye(10)[torch.arange(8)]
    net = _bnn()
    with pytest.raises(NotImplementedError, match=r"SVI training covers fc and fc2, not 'conv'"):
        model_bnn.train_svi_lockstep([net], x, y, [8], "cuda:0")
    with pytest.raises(NotImplementedError, match="conv"):
        net.train(None, "cuda:0")
    assert net.svi_loc is None and not hasattr(net, "device")


def test_conv_svi_lockstep_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources as KR
    if not os.path.exists(KR.READELF):
        pytest.skip("llvm-readelf not in this image")
    res = {n: r for n, r in KR.kernel_resources().items() if re.search(r"::(conv_svils_\w+_kernel|svils_draw_kernel<.*TensorMajor>|svils_finalize_kernel<false>|adam_kernel<.*TensorMajor>|"
                                                                             r"conv1_pool_kernel<\d, rbnn_conv_shared::Geo<1, 28>, 2>)", n)}
    # draw, Adam + KL, the sum over the accuracy samples, finalize; the grouped conv1 x 4 activations
    assert len(res) == 4 + 4, sorted(res)
    bad = {n: (r["scratch"], r["spill_vgpr"]) for n, r in res.items() if r["scratch"] or r["spill_vgpr"]}
    assert not bad, bad
