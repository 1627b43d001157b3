"""Host tier of several conv HMC chains behind every launch (robustbnns_amd/conv_hmc.ConvLockstepHmc, BNN.train_hmc_conv(num_chains, group), the
rbnn_conv_hmc_chains_* entry points of csrc/rbnn_hmc.hip and csrc/rbnn_conv_train.hip): the eight names in the header, in _hip.SIGNATURES and in
the library under the unchanged ABI number, the sizes against the single chain's and the ensemble's, the host-side argument checks of every
entry point in their documented order, every guard with nothing loaded, the tensor-major layout helper, the group size, and the resources of
the four new kernels.  No HIP compute is called here."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

import conv_hmc_restate as M
from robustbnns_amd import _hip

pytestmark = pytest.mark.usefixtures("built_library")
PREFIX = "rbnn_conv_hmc_chains_"
NAMES = [PREFIX + n for n in ("sizes", "stage", "gradient", "momentum", "update", "decide", "commit", "window_end")]
OK, ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED, ERR_ALIGN = 0, -1, -2, -3, -5
N16 = 832 + 801 * 16 + 49 * 16 * 10 + 10                                       # n_params of Hc 16, C 10


def test_the_eight_entry_points_are_additive_under_abi_10():
    lib = _hip.load()
    header = open(_hip.HEADER_PATH).read()
    declared = set(re.findall(r"\b(rbnn_\w+)\s*\(", header))
    assert re.search(r"#define RBNN_ABI_VERSION 10\b", header) and _hip.ABI_VERSION == 10 and lib.rbnn_abi_version() == 10
    for name in NAMES:
        assert name in declared and name in _hip.SIGNATURES and hasattr(lib, name), name
    assert declared == set(_hip.SIGNATURES)
    assert sorted(n for n in declared if n.startswith(PREFIX)) == sorted(NAMES)
    assert not [n for n in NAMES if "lockstep" in n or "svi_multi" in n]
    # the struct, field by field in order, against its ctypes class
    fields = re.search(r"typedef struct rbnn_conv_hmc_chains_net \{(.*?)\} rbnn_conv_hmc_chains_net;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    in_header = re.findall(r"\*?\b([A-Za-z_0-9]+)\s*[,;]", fields)
    assert in_header == [f[0] for f in _hip.ConvHmcChainsNet._fields_] == ["activation", "in_channels", "in_width", "hidden", "n_classes", "n_chains",
                                                                          "W", "grad"]
    assert _hip.ConvHmcChainsNet._pointers_ == ("W", "grad") and _hip.STRUCTS["ConvHmcChainsNet"] == "rbnn_conv_hmc_chains_net"
    assert [t for _, t in _hip.ConvHmcChainsNet._fields_] == [C.c_int32] * 6 + [C.c_void_p] * 2
    assert "Conv chains in lockstep are not built" not in header


def _net(hidden=16, n_classes=10, chains=3, activation=1, in_channels=1, in_width=28):
    net = _hip.ConvHmcChainsNet()
    net.activation, net.in_channels, net.in_width, net.hidden, net.n_classes, net.n_chains = activation, in_channels, in_width, hidden, n_classes, chains
    return net


def _single(hidden, n_classes):
    net = _hip.ConvSviTrainNet()
    net.activation, net.in_channels, net.in_width, net.hidden, net.n_classes = 1, 1, 28, hidden, n_classes
    return net


def _members(hidden, n_classes, members):
    net = _hip.ConvEnsNet()
    net.activation, net.in_channels, net.in_width, net.hidden, net.n_classes, net.n_members = 1, 1, 28, hidden, n_classes, members
    return net


def test_sizes_are_the_single_chains_and_the_ensembles():
    lib = _hip.load()
    nq, ne, nq1, ne1 = (C.c_int64(0) for _ in range(4))
    for Hc, Cn in ((16, 3), (48, 10), (1024, 10), (4096, 16)):
        for K, B in ((1, 1), (3, 65), (8, 128)):
            out, ens = _hip.ConvEnsBytes(), _hip.ConvEnsBytes()
            n = lib.rbnn_conv_hmc_chains_sizes(C.byref(_net(Hc, Cn, K)), B, C.byref(nq), C.byref(ne), C.byref(out))
            assert n == lib.rbnn_conv_hmc_sizes(C.byref(_single(Hc, Cn)), C.byref(nq1), C.byref(ne1)) == 832 + 801 * Hc + 49 * Hc * Cn + Cn
            assert (nq.value, ne.value) == (nq1.value, ne1.value) and ne.value == -(-n // 256)
            assert lib.rbnn_conv_ens_sizes(C.byref(_members(Hc, Cn, K)), B, C.byref(ens)) == OK
            for name, _ in _hip.ConvEnsBytes._fields_:
                assert getattr(out, name) == getattr(ens, name), (name, Hc, Cn, K, B)
            assert out.n_params == n and out.ce == 4 * K * B
    # every out-pointer is nullable, and without the workspace sizes the point count is not looked at
    assert lib.rbnn_conv_hmc_chains_sizes(C.byref(_net()), 0, None, None, None) == N16
    assert lib.rbnn_conv_hmc_chains_sizes(C.byref(_net()), -5, C.byref(nq), None, None) == N16 and nq.value > 0
    assert lib.rbnn_conv_hmc_chains_sizes(C.byref(_net()), 4, None, C.byref(ne), None) == N16 and ne.value == -(-N16 // 256)
    out = _hip.ConvEnsBytes()
    assert lib.rbnn_conv_hmc_chains_sizes(C.byref(_net()), 4, None, None, C.byref(out)) == N16 and out.n_params == N16
    for B in (0, -5, 65537):
        assert lib.rbnn_conv_hmc_chains_sizes(C.byref(_net()), B, None, None, C.byref(out)) == ERR_SHAPE
    assert lib.rbnn_conv_hmc_chains_sizes(None, 4, None, None, None) == ERR_NULL


def _chains(base, n=N16, nq=None, ne=None):
    ch = _hip.HmcLockstep()
    for name in _hip.HmcLockstep._pointers_:
        setattr(ch, name, base)
    ch.chain_stride, ch.qpart_stride, ch.epart_stride = n, 1 << 20 if nq is None else nq, 1 << 20 if ne is None else ne
    ch.log_rows, ch.sample_rows = 2, 2
    return ch


def _calls(lib):
    """name -> f(net, chains, ws, base, **overrides): the seven device entry points with host memory standing in for the device arrays."""
    ref = lambda x: C.byref(x) if x is not None else None
    p = lambda v, b: b if v == "b" else v
    return {
        "stage": lambda n, ch, w, b, X="b", ldx=784, n_rows=8, lab="b", rows="b", B=4: lib.rbnn_conv_hmc_chains_stage(
            ref(n), p(X, b), ldx, n_rows, p(lab, b), p(rows, b), B, ref(w), None),
        "gradient": lambda n, ch, w, b, B=4: lib.rbnn_conv_hmc_chains_gradient(ref(n), B, ref(w), None),
        "momentum": lambda n, ch, w, b: lib.rbnn_conv_hmc_chains_momentum(ref(n), ref(ch), 0, 0, None, None),
        "update": lambda n, ch, w, b, phase=0, step=-1: lib.rbnn_conv_hmc_chains_update(ref(n), ref(ch), phase, step, None),
        "decide": lambda n, ch, w, b, ce="b", B=4, i=0, mode=2: lib.rbnn_conv_hmc_chains_decide(ref(n), ref(ch), p(ce, b), B, i, mode, 0, 0, None),
        "commit": lambda n, ch, w, b, wn=0, row=-1: lib.rbnn_conv_hmc_chains_commit(ref(n), ref(ch), 0, wn, row, None),
        "window_end": lambda n, ch, w, b, nw=25: lib.rbnn_conv_hmc_chains_window_end(ref(n), ref(ch), nw, None),
    }


CHAIN_CALLS = ("momentum", "update", "decide", "commit", "window_end")


def test_every_entry_point_refuses_bad_arguments_on_the_host_in_the_documented_order():
    """NULL net, then the descriptor (geometry / activation: UNSUPPORTED; hidden, classes, K: SHAPE), then NULL pointers, then shapes, then
    phase / mode (UNSUPPORTED) and a step without lengths (NULL), then alignment; every refusal comes back as its status code before anything
    is launched (there is no device here to launch on), so no call below is valid."""
    lib = _hip.load()
    calls = _calls(lib)
    buf = (C.c_float * 4096)()
    base = C.addressof(buf)
    base += (-base) % 16
    for name, f in calls.items():
        assert f(None, _chains(base), _hip.ConvEnsWs(), base) == ERR_NULL, name
    # the descriptor is judged before any pointer: every pointer is NULL here
    for kw, rc in ((dict(in_width=32), ERR_UNSUPPORTED), (dict(in_channels=3), ERR_UNSUPPORTED), (dict(activation=-1), ERR_UNSUPPORTED),
                   (dict(activation=4), ERR_UNSUPPORTED), (dict(hidden=24), ERR_SHAPE), (dict(hidden=0), ERR_SHAPE), (dict(hidden=4112), ERR_SHAPE),
                   (dict(n_classes=0), ERR_SHAPE), (dict(n_classes=17), ERR_SHAPE), (dict(chains=0), ERR_SHAPE), (dict(chains=65536), ERR_SHAPE)):
        assert lib.rbnn_conv_hmc_chains_sizes(C.byref(_net(**kw)), 4, None, None, None) == rc, kw
        for name, f in calls.items():
            assert f(_net(**kw), None, None, None) == rc, (name, kw)
    assert lib.rbnn_conv_hmc_chains_sizes(C.byref(_net(chains=65535)), 4, None, None, None) == N16
    # NULL pointers come before shapes: a bad shape with something missing is still ERR_NULL
    net, ws, ch = _net(), _hip.ConvEnsWs(), _chains(base)
    bad_shape = _chains(base, n=N16 - 1)
    for name in CHAIN_CALLS:
        assert calls[name](net, None, ws, base) == ERR_NULL, name                                   # no chain block
        assert calls[name](net, _hip.HmcLockstep(), ws, base) == ERR_NULL, name                     # an empty one
    for field in ("q_cur", "g_cur", "r", "m_inv", "w_mean", "w_m2", "k0_part", "k1_part", "p_part", "state", "keys"):   # each missing pointer
        one = _chains(base, n=N16 - 1)
        setattr(one, field, None)
        for name in CHAIN_CALLS:
            assert calls[name](net, one, ws, base) == ERR_NULL, (name, field)
    for name in ("update", "commit"):                                                              # the trajectory's buffers are the net's
        assert calls[name](net, bad_shape, ws, base) == ERR_NULL, name
        for missing in ("W", "grad"):
            half = _net()
            half.W = half.grad = base
            setattr(half, missing, None)
            assert calls[name](half, bad_shape, ws, base) == ERR_NULL, (name, missing)
    assert calls["decide"](net, bad_shape, ws, base, ce=None) == ERR_NULL
    no_stack = _chains(base, n=N16 - 1)
    no_stack.samples = None
    net.W = net.grad = base
    assert calls["commit"](net, no_stack, ws, base, row=0) == ERR_NULL                              # a sample row without a stack
    assert calls["commit"](net, no_stack, ws, base, row=-1) == ERR_SHAPE                            # (without a row the stack is not needed)
    s = calls["stage"]
    assert s(net, ch, None, base) == ERR_NULL and s(net, ch, ws, base, B=0) == ERR_NULL             # the workspace; Xs / labels
    assert calls["gradient"](net, ch, None, base) == ERR_NULL and calls["gradient"](net, ch, ws, base, B=0) == ERR_NULL
    for k in _hip.CONV_ENS_WS_KEYS:
        setattr(ws, k, base)
    assert s(net, ch, ws, base, X=None, B=0) == ERR_NULL and s(net, ch, ws, base, lab=None) == ERR_NULL and s(net, ch, ws, base, rows=None) == ERR_NULL
    for k in _hip.CONV_ENS_WS_KEYS:
        setattr(ws, k, None)
        assert calls["gradient"](net, ch, ws, base, B=0) == ERR_NULL, k
        setattr(ws, k, base)
    for missing in ("W", "grad"):
        half = _net()
        half.W = half.grad = base
        setattr(half, missing, None)
        assert calls["gradient"](half, ch, ws, base, B=0) == ERR_NULL, missing
    # shapes
    for name in CHAIN_CALLS:
        for n in (N16 - 1, N16 + 1):                                                                # tensor-major: chain_stride is n_params
            assert calls[name](net, _chains(base, n=n), ws, base) == ERR_SHAPE, (name, n)
        nq, ne = C.c_int64(0), C.c_int64(0)
        assert lib.rbnn_conv_hmc_chains_sizes(C.byref(net), 0, C.byref(nq), C.byref(ne), None) == N16
        assert calls[name](net, _chains(base, nq=nq.value - 1), ws, base) == ERR_SHAPE and calls[name](net, _chains(base, ne=ne.value - 1), ws, base) == ERR_SHAPE
        for field in ("log_rows", "sample_rows"):
            one = _chains(base)
            setattr(one, field, -1)
            assert calls[name](net, one, ws, base) == ERR_SHAPE, (name, field)
    exact = _chains(base, nq=nq.value, ne=ne.value)                                                 # the least strides pass: phase 6 is what is refused
    assert calls["update"](net, exact, ws, base, phase=6) == ERR_UNSUPPORTED
    for B in (0, -3, 65537):
        assert s(net, ch, ws, base, B=B) == ERR_SHAPE and calls["gradient"](net, ch, ws, base, B=B) == ERR_SHAPE, B
        assert calls["decide"](net, ch, ws, base, B=B) == ERR_SHAPE, B
    big = _net(chains=65535)
    big.W = big.grad = base
    assert 65535 * 65 > 2 ** 22 >= 65535 * 64
    out = _hip.ConvEnsBytes()
    assert lib.rbnn_conv_hmc_chains_sizes(C.byref(big), 65, None, None, C.byref(out)) == ERR_SHAPE
    assert lib.rbnn_conv_hmc_chains_sizes(C.byref(big), 64, None, None, C.byref(out)) == N16
    for name in ("stage", "gradient", "decide"):
        assert calls[name](big, ch, ws, base, B=65) == ERR_SHAPE, name                              # K B past 2^22
    assert s(net, ch, ws, base, ldx=780) == ERR_SHAPE and s(net, ch, ws, base, ldx=786) == ERR_SHAPE and s(net, ch, ws, base, n_rows=0) == ERR_SHAPE
    assert calls["decide"](net, ch, ws, base, i=-1) == ERR_SHAPE
    assert calls["commit"](net, ch, ws, base, wn=-1) == ERR_SHAPE
    assert calls["commit"](net, ch, ws, base, row=2) == ERR_SHAPE                                   # a row behind the stacks of 2 rows
    assert calls["window_end"](net, ch, ws, base, nw=1) == ERR_SHAPE
    # phase / mode, and a step without the chains' lengths: after the shapes
    for phase in (-1, 6):
        assert calls["update"](net, ch, ws, base, phase=phase) == ERR_UNSUPPORTED
        assert calls["update"](net, _chains(base, n=N16 + 1), ws, base, phase=phase) == ERR_SHAPE
    for mode in (-1, 3):
        assert calls["decide"](net, ch, ws, base, mode=mode) == ERR_UNSUPPORTED
        assert calls["decide"](net, ch, ws, base, mode=mode, B=0) == ERR_SHAPE
    no_steps = _chains(base)
    no_steps.steps = None
    assert calls["update"](net, no_steps, ws, base, phase=1, step=0) == ERR_NULL
    assert calls["update"](net, no_steps, ws, base, phase=6, step=-1) == ERR_UNSUPPORTED
    no_steps.chain_stride = N16 + 1
    assert calls["update"](net, no_steps, ws, base, phase=1, step=0) == ERR_SHAPE
    # alignment comes last
    assert s(net, ch, ws, base, X=base + 4) == ERR_ALIGN and s(net, ch, ws, base, X=base + 4, n_rows=0) == ERR_SHAPE
    ws.Xs = base + 4
    assert s(net, ch, ws, base) == ERR_ALIGN
    ws.Xs = base
    for k in ("Xs", "dO1", "part1", "ce"):
        setattr(ws, k, base + 4)
        assert calls["gradient"](net, ch, ws, base) == ERR_ALIGN, k
        setattr(ws, k, base)
    for field in ("W", "grad"):                                                                     # a misaligned W
        setattr(net, field, base + 4)
        assert calls["gradient"](net, ch, ws, base) == ERR_ALIGN and calls["gradient"](net, ch, ws, base, B=0) == ERR_SHAPE, field
        setattr(net, field, base)


def test_guards_fire_with_nothing_loaded_and_no_state_changed(monkeypatch, tmp_path):
    from torch.utils.data import DataLoader, TensorDataset
    from robustbnns_amd import conv_hmc
    from robustbnns_amd.model_bnn import BNN
    launched = []
    monkeypatch.setattr(_hip, "HipKernels", lambda: launched.append(1))
    monkeypatch.setattr(_hip, "load", lambda: launched.append(2))
    monkeypatch.chdir(tmp_path)
    x, y = torch.rand(8, 1, 28, 28), torch.eye(10)[torch.arange(8)]
    loader = DataLoader(TensorDataset(x, y), batch_size=4)
    conv = BNN("mnist", 16, "leaky", "conv", "hmc", None, None, 5, 2, (1, 28, 28), 10)
    q0 = M.start_position(16, 10)
    torch.manual_seed(5)
    rng = torch.get_rng_state()
    rel = str(tmp_path) + "/out/"
    make = lambda q0s, keys, device="cuda:0", shape=(1, 28, 28): conv_hmc.ConvLockstepHmc("leaky", shape, 10, q0s, 0.01, 10, device, keys)
    with pytest.raises(NotImplementedError, match="no CPU compute path"):
        make([q0, q0], [1, 2], device="cpu")
    with pytest.raises(NotImplementedError, match="1x28x28"):
        make([q0, q0], [1, 2], shape=(3, 32, 32))
    with pytest.raises(ValueError, match="one key per chain"):
        make([q0, q0], [1])
    with pytest.raises(ValueError, match="at least one chain"):
        make([], [])
    with pytest.raises(ValueError, match="at most 65535 chains"):
        make([q0] * 65536, list(range(65536)))
    for bad in (0, -1):
        with pytest.raises(ValueError, match="num_chains"):
            conv.train_hmc_conv(loader, "cuda:0", rel, num_chains=bad)
    with pytest.raises(ValueError, match="group"):
        conv.train_hmc_conv(loader, "cuda:0", rel, group=0)
    with pytest.raises(ValueError, match="group"):
        conv.train_hmc_conv(loader, "cuda:0", rel, num_chains=2, group=3)
    with pytest.raises(NotImplementedError, match="no CPU compute path"):
        conv.train_hmc_conv(loader, "cpu", rel, num_chains=2)
    assert not launched and torch.equal(rng, torch.get_rng_state())
    assert not hasattr(conv, "device") and not hasattr(conv, "hmc_history") and conv.svi_loc is None and conv.posterior is None
    assert not os.listdir(tmp_path)


def test_layout_helper_round_trip_is_the_identity():
    """flat [K, n] -> tensor-major -> chain_flat(k) for (Hc 16, C 3, K 3) on CPU tensors, and block t of the tensor-major buffer holds the
    chains' tensor t one after the other."""
    from robustbnns_amd.conv_hmc import chain_flat, tensor_major
    K, blocks = 3, [int(torch.Size(s).numel()) for s in M.V.shapes_of(16, 3).values()]
    n = sum(blocks)
    assert blocks == [800, 32, 800 * 16, 16, 49 * 16 * 3, 3] and n == 832 + 801 * 16 + 49 * 16 * 3 + 3
    flat = torch.arange(K * n, dtype=torch.float32).reshape(K, n)
    tm = tensor_major(flat, blocks)
    assert tuple(tm.shape) == (K * n,) and sorted(tm.tolist()) == flat.reshape(-1).tolist()
    for k in range(K):
        assert torch.equal(chain_flat(tm, k, blocks, K), flat[k])
    off = 0
    for t, size in enumerate(blocks):                                         # block t starts at K times the single net's offset
        assert sum(blocks[:t]) * K == off
        for k in range(K):
            assert torch.equal(tm[off + k * size:off + (k + 1) * size], flat[k, sum(blocks[:t]):sum(blocks[:t]) + size]), (t, k)
        off += K * size
    assert torch.equal(tensor_major(flat[:1], blocks), flat[0])               # one chain: the single chain's flat buffer


def test_chain_group_follows_the_budget(monkeypatch):
    from robustbnns_amd.conv_hmc import TENSOR_MAJOR, conv_hmc_chains_group
    lib, Hc, Cn, B = _hip.load(), 1024, 10, 5000
    ens = _hip.ConvEnsBytes()
    assert lib.rbnn_conv_ens_sizes(C.byref(_members(Hc, Cn, 1)), B, C.byref(ens)) == OK
    per = sum(getattr(ens, k) for k in _hip.CONV_ENS_WS_KEYS) + len(TENSOR_MAJOR) * 4 * ens.n_params
    assert len(TENSOR_MAJOR) == 8 and per > 2 ** 30                            # several GB per chain at the reference's batch
    monkeypatch.delenv("RBNN_CONV_WS_GB", raising=False)
    assert conv_hmc_chains_group("leaky", 16, 10, 7, 8) == 7                   # everything fits: K
    assert conv_hmc_chains_group("leaky", Hc, Cn, 1000, B) == int(48 * 2 ** 30 // per) >= 1
    groups = [conv_hmc_chains_group("leaky", Hc, Cn, 64, B, budget_gb=gb) for gb in (0.001, 1, 4, 16, 48, 96, 10 ** 4)]
    assert groups == sorted(groups) and groups[0] == 1 and groups[-1] == 64    # monotone in the budget, at least 1, at most K
    monkeypatch.setenv("RBNN_CONV_WS_GB", "16")
    g = conv_hmc_chains_group("leaky", Hc, Cn, 64, B)
    assert g * per <= 16 * 2 ** 30 < (g + 1) * per
    assert conv_hmc_chains_group("leaky", 16, 10, 10 ** 6, 1, budget_gb=10 ** 6) == 65535          # never past the grid's limit,
    assert conv_hmc_chains_group("leaky", 16, 10, 10 ** 6, 128, budget_gb=10 ** 6) == 2 ** 22 // 128      # nor past 2^22 packed points


def test_the_four_new_kernels_use_no_scratch():
    """The tensor-major instances of the four lockstep kernel templates of csrc/rbnn_hmc.hip (what the conv chains launch), and the chain-major
    instances beside them: exactly four each, no scratch, no spilled VGPRs."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources as KR
    if not os.path.exists(KR.READELF):
        pytest.skip("llvm-readelf not in this image")
    for view in ("TensorMajor", "ChainMajor"):
        name = r"::lockstep_(\w+)_kernel<\(anonymous namespace\)::" + view + r">\("
        res = {n: r for n, r in KR.kernel_resources().items() if re.search(name, n)}
        assert sorted(re.search(name, n).group(1) for n in res) == ["commit", "momentum", "update", "window_end"], sorted(res)
        bad = {n: (r["scratch"], r["spill_vgpr"]) for n, r in res.items() if r["scratch"] or r["spill_vgpr"]}
        assert not bad, bad
