"""Host tier of deep ensembles of conv nets in lockstep (robustbnns_amd/conv_train.ConvEnsembleTrainer, Ensemble_NN.train_conv, the rbnn_conv_ens_*
entry points of csrc/rbnn_conv_train.hip): the new names in the header, in _hip.SIGNATURES and in the library under the unchanged ABI number,
the sizes against the tensor-major layout, the host-side argument checks, the member-group size, the guards, and the new kernels'
resources.  No HIP compute is called here."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

import conv_restate as CR
from robustbnns_amd import _hip, model_ensemble

pytestmark = pytest.mark.usefixtures("built_library")
NAMES = ["rbnn_conv_ens_sizes", "rbnn_conv_ens_stage", "rbnn_conv_ens_forward", "rbnn_conv_ens_weight_grads", "rbnn_conv_ens_adam_step",
         "rbnn_conv_ens_finalize"]
OK, ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED, ERR_ALIGN = 0, -1, -2, -3, -5
ADAM = (0.01, 0.9, 0.999, 1e-8, None)


def test_new_entry_points_are_additive_under_abi_10():
    lib = _hip.load()
    header = open(_hip.HEADER_PATH).read()
    declared = set(re.findall(r"\b(rbnn_\w+)\s*\(", header))
    assert re.search(r"#define RBNN_ABI_VERSION 10\b", header) and _hip.ABI_VERSION == 10 and lib.rbnn_abi_version() == 10
    for name in NAMES:
        assert name in declared and name in _hip.SIGNATURES and hasattr(lib, name), name
    assert declared == set(_hip.SIGNATURES)
    assert _hip.CONV_ENS_WS_KEYS == ("Xs", "labels") + _hip.CONV_TRAIN_WS_KEYS
    assert [n for n, _ in _hip.ConvEnsNet._fields_][:6] == ["activation", "in_channels", "in_width", "hidden", "n_classes", "n_members"]
    assert _hip.ConvEnsNet._pointers_ == ("P", "m", "v", "grad")


def _net(hidden=32, n_classes=10, members=3):
    net = _hip.ConvEnsNet()
    net.activation, net.in_channels, net.in_width, net.hidden, net.n_classes, net.n_members = 1, 1, 28, hidden, n_classes, members
    return net


def _single(hidden, n_classes):
    net = _hip.ConvTrainNet()
    net.activation, net.in_channels, net.in_width, net.hidden, net.n_classes = 1, 1, 28, hidden, n_classes
    return net


@pytest.mark.parametrize("Hc", [16, 48])
def test_sizes_follow_the_tensor_major_layout(Hc):
    """n_params is one member's (rbnn_conv_train_sizes'), every byte count M times the single net's, Xs and labels beside them; the six blocks
    [M, size of tensor] start at M times the single net's offsets, 16-byte aligned for every M, and so does every member's tensor of the three
    the forward reads 16 bytes at a time (model.3.weight, model.3.bias, model.7.weight)."""
    lib, out, one = _hip.load(), _hip.ConvEnsBytes(), _hip.ConvTrainBytes()
    for M, Cn, B in ((1, 10, 1), (3, 10, 65), (7, 3, 100)):
        assert lib.rbnn_conv_ens_sizes(C.byref(_net(Hc, Cn, M)), B, C.byref(out)) == OK
        assert lib.rbnn_conv_train_sizes(C.byref(_single(Hc, Cn)), B, C.byref(one)) == OK
        assert out.n_params == one.n_params == 832 + 801 * Hc + 49 * Hc * Cn + Cn
        for k in _hip.CONV_TRAIN_WS_KEYS:
            assert getattr(out, k) == M * getattr(one, k), k
        assert out.Xs == 4 * 784 * M * B and out.labels == 4 * M * B
        sizes = [v.numel() for v in CR.fresh_params("leaky", Hc, Cn, 0).values()]
        assert sum(sizes) == out.n_params
        off = 0
        for key, size in zip(CR.KEYS, sizes):
            assert (4 * off) % 16 == 0, (key, M)                                              # the block's start
            if key in ("model.3.weight", "model.3.bias", "model.7.weight"):
                assert (4 * size) % 16 == 0, key                                              # so every member's tensor inside it
            off += M * size
        assert off == M * out.n_params


def test_trainer_layout_is_tensor_major(monkeypatch):
    """ConvEnsembleTrainer's flat order, on the CPU with the kernels' handle replaced: unflat(buf, k) returns member k's tensors, and block t
    holds the members' tensor t one after the other."""
    from robustbnns_amd import conv_train

    class _Lib:
        @staticmethod
        def rbnn_conv_ens_sizes(net, B, out):
            return _hip.load().rbnn_conv_ens_sizes(net, B, out)

    class _K:
        lib = _Lib()

    monkeypatch.setattr(_hip, "HipKernels", _K)
    monkeypatch.setattr(conv_train, "check_conv_trainable", lambda *a: None)
    monkeypatch.setattr(_hip, "CONV_ENS_WS_KEYS", ())
    params = [CR.fresh_params("leaky", 16, 10, s) for s in (1, 2, 3)]
    tr = conv_train.ConvEnsembleTrainer("leaky", CR.SHAPE, 10, params, 0.01, "cpu", batch_size=4)
    assert tr.M == 3 and tuple(tr.P.shape) == (3 * tr.n_params,) and tuple(tr.stats.shape) == (3, 3) and tuple(tr.grad.shape) == tuple(tr.P.shape)
    off = 0
    for key in CR.KEYS:
        size = params[0][key].numel()
        for k in range(3):
            assert torch.equal(tr.unflat(tr.P, k)[key], params[k][key]), (key, k)
            assert torch.equal(tr.P[off + k * size:off + (k + 1) * size], params[k][key].reshape(-1)), (key, k)
        off += 3 * size
    assert [list(p) for p in tr.params()] == [CR.KEYS] * 3


def test_entry_points_validate_their_arguments_on_the_host():
    """Every refusal comes back as its status code before anything is launched (there is no device here to launch on)."""
    lib, out = _hip.load(), _hip.ConvEnsBytes()
    assert lib.rbnn_conv_ens_sizes(None, 8, C.byref(out)) == ERR_NULL and lib.rbnn_conv_ens_sizes(C.byref(_net()), 8, None) == ERR_NULL
    for field, bad, rc in (("hidden", 8, ERR_SHAPE), ("hidden", 40, ERR_SHAPE), ("n_classes", 0, ERR_SHAPE), ("n_classes", 17, ERR_SHAPE),
                           ("n_members", 0, ERR_SHAPE), ("n_members", -1, ERR_SHAPE), ("n_members", 65536, ERR_SHAPE),
                           ("activation", 4, ERR_UNSUPPORTED), ("in_channels", 3, ERR_UNSUPPORTED), ("in_width", 32, ERR_UNSUPPORTED)):
        net = _net()
        setattr(net, field, bad)
        assert lib.rbnn_conv_ens_sizes(C.byref(net), 8, C.byref(out)) == rc, (field, bad)
        assert lib.rbnn_conv_ens_adam_step(C.byref(net), 1, *ADAM) == rc, (field, bad)
        assert lib.rbnn_conv_ens_forward(C.byref(net), 4, None, None) == rc, (field, bad)
        assert lib.rbnn_conv_ens_weight_grads(C.byref(net), 4, None, None) == rc, (field, bad)
        assert lib.rbnn_conv_ens_finalize(C.byref(net), None, 4, None, None) == rc, (field, bad)
        assert lib.rbnn_conv_ens_stage(C.byref(net), None, 784, 8, None, None, 4, None, None) == rc, (field, bad)
    assert lib.rbnn_conv_ens_sizes(C.byref(_net()), 0, C.byref(out)) == ERR_SHAPE
    assert lib.rbnn_conv_ens_sizes(C.byref(_net(members=65535)), 100, C.byref(out)) == ERR_SHAPE          # M B past 2^22
    assert lib.rbnn_conv_ens_sizes(C.byref(_net(members=65535)), 64, C.byref(out)) == OK
    # host memory stands in for the buffers: every call below is refused before a pointer is followed
    buf = (C.c_float * 4096)()
    base = C.addressof(buf)
    base += (-base) % 16
    net, ws = _net(), _hip.ConvEnsWs()
    stage = lambda n, X, ldx, n_rows, lab, rows, B, w: lib.rbnn_conv_ens_stage(C.byref(n), X, ldx, n_rows, lab, rows, B, C.byref(w) if w is not None else None, None)
    fwd = lambda n, B, w: lib.rbnn_conv_ens_forward(C.byref(n), B, C.byref(w) if w is not None else None, None)
    wg = lambda n, B, w: lib.rbnn_conv_ens_weight_grads(C.byref(n), B, C.byref(w) if w is not None else None, None)
    fin = lambda n, w, B, stats: lib.rbnn_conv_ens_finalize(C.byref(n), C.byref(w) if w is not None else None, B, stats, None)
    assert fwd(net, 4, ws) == ERR_NULL and wg(net, 4, ws) == ERR_NULL and stage(net, base, 784, 8, base, base, 4, ws) == ERR_NULL      # P, grad, the workspaces: NULL
    assert lib.rbnn_conv_ens_adam_step(C.byref(net), 1, *ADAM) == ERR_NULL
    for name in ("P", "m", "v", "grad"):
        setattr(net, name, base)
    assert fwd(net, 4, ws) == ERR_NULL and wg(net, 4, ws) == ERR_NULL and fwd(net, 4, None) == ERR_NULL and wg(net, 4, None) == ERR_NULL
    assert stage(net, base, 784, 8, base, base, 4, None) == ERR_NULL and fin(net, None, 4, base) == ERR_NULL and fin(net, ws, 4, base) == ERR_NULL
    for k in _hip.CONV_ENS_WS_KEYS:
        setattr(ws, k, base)
    assert stage(net, None, 784, 8, base, base, 4, ws) == ERR_NULL and stage(net, base, 784, 8, None, base, 4, ws) == ERR_NULL
    assert stage(net, base, 784, 8, base, None, 4, ws) == ERR_NULL and fin(net, ws, 4, None) == ERR_NULL
    for B in (0, -3):
        assert stage(net, base, 784, 8, base, base, B, ws) == ERR_SHAPE and fwd(net, B, ws) == ERR_SHAPE and wg(net, B, ws) == ERR_SHAPE
        assert fin(net, ws, B, base) == ERR_SHAPE
    assert stage(net, base, 780, 8, base, base, 4, ws) == ERR_SHAPE and stage(net, base, 786, 8, base, base, 4, ws) == ERR_SHAPE      # below 784; not a multiple of 4
    assert stage(net, base, 784, 0, base, base, 4, ws) == ERR_SHAPE
    assert stage(net, base + 4, 784, 8, base, base, 4, ws) == ERR_ALIGN
    ws.Xs = base + 4
    assert stage(net, base, 784, 8, base, base, 4, ws) == ERR_ALIGN and fwd(net, 4, ws) == ERR_ALIGN
    ws.Xs = base
    net.P = base + 4
    assert fwd(net, 4, ws) == ERR_ALIGN
    net.P = base
    assert lib.rbnn_conv_ens_adam_step(C.byref(net), 0, *ADAM) == ERR_SHAPE


def test_member_group_fits_the_workspace_budget(monkeypatch):
    """All members when they fit RBNN_CONV_WS_GB, else the largest group that does, never fewer than one; the size is linear in M."""
    from robustbnns_amd.conv_train import conv_ensemble_group
    lib, out = _hip.load(), _hip.ConvEnsBytes()
    assert lib.rbnn_conv_ens_sizes(C.byref(_net(1024, 10, 1)), 100, C.byref(out)) == OK
    per = sum(getattr(out, k) for k in _hip.CONV_ENS_WS_KEYS) + 16 * out.n_params
    assert 0.05 * 2 ** 30 < per < 0.3 * 2 ** 30                                               # "on the order of 0.1 GB per member"
    monkeypatch.delenv("RBNN_CONV_WS_GB", raising=False)
    assert conv_ensemble_group("leaky", 16, 10, 100, 100) == 100
    assert conv_ensemble_group("leaky", 1024, 10, 100, 100) == min(100, int(48 * 2 ** 30 // per))
    assert conv_ensemble_group("leaky", 1024, 10, 100, 100, budget_gb=1.0) == int(2 ** 30 // per) >= 3
    monkeypatch.setenv("RBNN_CONV_WS_GB", "0.001")
    assert conv_ensemble_group("leaky", 1024, 10, 100, 100) == 1
    monkeypatch.setenv("RBNN_CONV_WS_GB", "2")
    g = conv_ensemble_group("leaky", 1024, 10, 100, 100)
    assert g * per <= 2 * 2 ** 30 < (g + 1) * per


def test_guards_fire_with_nothing_constructed(monkeypatch):
    from robustbnns_amd import conv_train
    launched = []
    monkeypatch.setattr(_hip, "HipKernels", lambda: launched.append(1))
    monkeypatch.setattr(_hip, "load", lambda: launched.append(2))
    x, y = torch.rand(8, 1, 28, 28), torch.eye(10)[torch.arange(8)]
    conv = model_ensemble.Ensemble_NN("mnist", 16, "leaky", "conv", 1, 0.01, (1, 28, 28), 10, 2)
    fc = model_ensemble.Ensemble_NN("mnist", 16, "leaky", "fc", 1, 0.01, (1, 28, 28), 10, 2)
    torch.manual_seed(5)
    rng = torch.get_rng_state()
    with pytest.raises(ValueError, match="train"):
        fc.train_conv(x, y, "cuda:0")
    with pytest.raises(NotImplementedError, match="no CPU compute path"):
        conv.train_conv(x, y, "cpu")
    with pytest.raises(NotImplementedError, match="no CPU compute path"):
        conv_train.ConvEnsembleTrainer("leaky", (1, 28, 28), 10, [CR.fresh_params("leaky", 16, 10, 0)], 0.01, "cpu")
    with pytest.raises(NotImplementedError, match="1x28x28"):
        conv_train.ConvEnsembleTrainer("leaky", (3, 32, 32), 10, [CR.fresh_params("leaky", 16, 10, 0)], 0.01, "cuda:0")
    conv.input_shape = (3, 32, 32)
    with pytest.raises(NotImplementedError, match="1x28x28"):
        conv.train_conv(x, y, "cuda:0")
    conv.input_shape = (1, 28, 28)
    with pytest.raises(NotImplementedError, match=r"conv.*Ensemble_NN\.train_conv"):
        conv.train(x, y, "cuda:0")                                          # Ensemble_NN.train keeps refusing conv, and names the entry point
    assert not launched and torch.equal(rng, torch.get_rng_state())
    assert conv.ensemble_models == {} and fc.ensemble_models == {} and not hasattr(conv, "device") and not hasattr(fc, "device")


def test_conv_ensemble_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources as KR
    if not os.path.exists(KR.READELF):
        pytest.skip("llvm-readelf not in this image")
    res = {n: r for n, r in KR.kernel_resources().items()
           if re.search(r"::(conv_ens_(stage|reduce)_kernel|conv_(do2|route1|wgrad_gemm)_kernel<\d, true>|conv1_pool_kernel<\d, rbnn_conv_shared::Geo<1, 28>, 1>|"
                        r"nn_finalize_kernel<true>|train_gemm_kernel<true, false>)", n)}
    # stage, reduce, do2 and route1 x 4 activations, the GEMM in its 3 modes, the packed conv1 x 4 activations, the per-member statistics and strided GEMM
    assert len(res) == 2 + 8 + 3 + 4 + 2, sorted(res)
    bad = {n: (r["scratch"], r["spill_vgpr"]) for n, r in res.items() if r["scratch"] or r["spill_vgpr"]}
    assert not bad, bad
