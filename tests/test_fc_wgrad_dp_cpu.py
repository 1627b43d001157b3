"""Host side of the fp64 fc / fc2 weight-gradient checker (no GPU): the three C-ABI additions and their argument checks, what
AttackEngine.weight_gradients refuses before anything is launched, and the resources of its kernels read from the built library.
Everything here fails on a tree without the feature: the method, the include file and the three C names do not exist there."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

from robustbnns_amd import _hip
from robustbnns_amd.engine import AttackEngine

pytestmark = pytest.mark.usefixtures("built_library")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"rbnn_fc_wgrad_dp_workspace_query", "rbnn_fc_hidden_dp", "rbnn_fc_weight_grads_dp"}
VP, I32 = C.c_void_p, C.c_int32


class Recorder:
    """Stands where the kernels stand and records every call made through it: `calls` stays empty while nothing is launched."""
    calls = []

    def __getattr__(self, name):
        return lambda *a, **k: Recorder.calls.append(name)


class Post:
    """As much of a StackedPosterior as the engine's constructor and the refusals read."""

    def __init__(self, arch="fc"):
        self.arch, self.device, self.S, self.C, self.D, self.Dp, self.H, self.Hp = arch, torch.device("cuda"), 4, 10, 784, 784, 512, 512
        self.triple_supported, self.split_supported = (lambda: False), (lambda: False)


@pytest.fixture
def recorder(monkeypatch):
    Recorder.calls = []
    monkeypatch.setattr(_hip, "HipKernels", Recorder)
    monkeypatch.delenv("RBNN_PRECISION", raising=False)
    return Recorder


def test_header_declares_the_three_entry_points_and_the_abi_is_unchanged():
    import __graft_entry__ as G
    hdr = open(_hip.HEADER_PATH).read()
    declared = set(re.findall(r"\b(rbnn_\w+)\s*\(", hdr))
    assert NAMES <= declared and NAMES <= set(_hip.SIGNATURES)
    # the fences of the other host tests
    assert not [n for n in NAMES if "f64" in n or ("conv" in n and "fp64" in n) or "svi_multi" in n or "lockstep" in n]
    assert "#define RBNN_ABI_VERSION 10" in hdr and _hip.ABI_VERSION == 10 and _hip.load().rbnn_abi_version() == 10
    assert len(G.SOURCES) == 12 and any(d.endswith("rbnn_fc_wgrad_dp.inc") for d in G.DEPS)
    src = open(os.path.join(G.CSRC, "rbnn_kernels.hip")).read()
    assert src.index('#include "rbnn_fp64.inc"') < src.index('#include "rbnn_fc_wgrad_dp.inc"')
    assert _hip.F64_WS_BUFFERS == 6 and _hip.FC_WGRAD_DP_WS_BUFFERS == len(_hip.FC_WGRAD_DP_WS_KEYS) == 2
    assert _hip.FC_WGRAD_DP_WS_KEYS == ("ce", "hidL")
    assert _hip.FC_WGRAD_DP_OUT_KEYS == ("dW1", "db1", "dWm", "dbm", "dW2", "db2")
    fp = C.POINTER(_hip.Posterior)
    assert _hip.SIGNATURES["rbnn_fc_wgrad_dp_workspace_query"] == (I32, [fp, I32, I32, VP])
    assert _hip.SIGNATURES["rbnn_fc_hidden_dp"] == (I32, [fp, VP, I32, VP, I32, I32, VP, VP, VP])
    assert _hip.SIGNATURES["rbnn_fc_weight_grads_dp"] == (I32, [fp, VP, I32, I32, I32] + [VP] * 12)
    for m in ("fc_wgrad_dp_workspace_sizes", "fc_hidden_dp", "fc_weight_grads_dp"):
        assert callable(getattr(_hip.HipKernels, m))


def _net(arch=0, H=40, D=50, c=7, weights=True):
    net = _hip.Posterior()
    net.arch, net.activation, net.in_features, net.in_stride, net.hidden, net.n_classes, net.n_stored = arch, 1, D, (D + 15) // 16 * 16, H, c, 5
    if weights:
        for k in ("W1", "b1", "W2", "b2") + (("Wm", "bm") if arch == 1 else ()):
            setattr(net, k, 4096)
    return net


@pytest.mark.parametrize("arch,H", [(0, 40), (1, 512)])
def test_workspace_query_follows_the_formula(arch, H):
    """N points x S samples, doubles: the per-point CE and the activations of the last hidden layer — the same for fc and fc2."""
    N, S = 33, 5
    out = (C.c_size_t * 2)()
    assert _hip.load().rbnn_fc_wgrad_dp_workspace_query(C.byref(_net(arch, H, 784, 10, weights=False)), N, S, out) == 0
    assert list(out) == [S * N * 8, S * N * H * 8]


def test_every_argument_error_returns_its_code_before_any_launch():
    """Fake pointers: a call that got past the checks would fault."""
    lib, p = _hip.load(), 4096
    out = (C.c_size_t * 2)()
    q = lib.rbnn_fc_wgrad_dp_workspace_query
    assert q(None, 4, 2, out) == _hip.ERR_NULL and q(C.byref(_net()), 4, 2, None) == _hip.ERR_NULL
    bad = _net()
    bad.arch = 2
    assert q(C.byref(bad), 4, 2, out) == _hip.ERR_UNSUPPORTED
    assert q(C.byref(_net(H=42)), 4, 2, out) == _hip.ERR_SHAPE and q(C.byref(_net()), 0, 2, out) == _hip.ERR_SHAPE
    assert q(C.byref(_net()), 4, 0, out) == _hip.ERR_SHAPE and q(C.byref(_net()), 1 << 20, 1 << 12, out) == _hip.ERR_SHAPE

    def hidden(net, X=p, ldx=64, S=2, N=4, hid1=p, hidL=p):
        return lib.rbnn_fc_hidden_dp(C.byref(net), X, ldx, None, S, N, hid1, hidL, None)

    wbufs = ("dZ", "dact1", "hid1", "dact2", "hidL", "dW1", "db1", "dWm", "dbm", "dW2", "db2")

    def wg(net, X=p, ldx=64, S=2, N=4, **kw):
        b = {k: p for k in wbufs}
        b.update(kw)
        return lib.rbnn_fc_weight_grads_dp(C.byref(net), X, ldx, S, N, *(b[k] for k in wbufs), None)

    for call in (hidden, wg):
        # what validate_net_f64 refuses, with its code
        assert call(_net(weights=False)) == _hip.ERR_NULL                                                # no weights
        net = _net(1)
        net.Wm = None
        assert call(net) == _hip.ERR_NULL                                                                # fc2 without Wm
        net = _net()
        net.arch = 2
        assert call(net) == _hip.ERR_UNSUPPORTED
        net = _net()
        net.activation = 9
        assert call(net) == _hip.ERR_UNSUPPORTED
        assert call(_net(H=42)) == _hip.ERR_SHAPE and call(_net(c=17)) == _hip.ERR_SHAPE
        net = _net()
        net.W1 = p + 4
        assert call(net) == _hip.ERR_ALIGN
        # the counts, ldx, X
        for arch in (0, 1):
            net = _net(arch)
            assert call(net, N=0) == _hip.ERR_SHAPE and call(net, S=0) == _hip.ERR_SHAPE and call(net, S=65536) == _hip.ERR_SHAPE
            assert call(net, N=1 << 20, S=1 << 12) == _hip.ERR_SHAPE
            assert call(net, X=None) == _hip.ERR_NULL
            assert call(net, ldx=48) == _hip.ERR_SHAPE and call(net, ldx=66) == _hip.ERR_SHAPE            # below in_stride; not a multiple of 4
            assert call(net, X=p + 8) == _hip.ERR_ALIGN

    assert hidden(_net(), hidL=None) == _hip.ERR_NULL and hidden(_net(1), hid1=None) == _hip.ERR_NULL
    assert hidden(_net(), hidL=p + 8) == _hip.ERR_ALIGN and hidden(_net(1), hid1=p + 8) == _hip.ERR_ALIGN
    for k in ("dZ", "dact1", "hidL", "dW1", "db1", "dW2", "db2"):
        assert wg(_net(), **{k: None}) == _hip.ERR_NULL, k
    for k in wbufs:
        assert wg(_net(1), **{k: None}) == _hip.ERR_NULL, k
    for k in ("dZ", "dact1", "hidL"):
        assert wg(_net(), **{k: p + 8}) == _hip.ERR_ALIGN, k
    for k in ("dZ", "dact1", "hid1", "dact2", "hidL"):
        assert wg(_net(1), **{k: p + 8}) == _hip.ERR_ALIGN, k


@pytest.mark.parametrize("precision", ["exact", "triple"])
def test_weight_gradients_runs_under_fp64_only(recorder, precision):
    post = Post()
    post.triple_supported = lambda: True
    eng = AttackEngine(post, kernels=recorder(), precision=precision)
    assert eng.precision == precision
    Recorder.calls = []
    with pytest.raises(_hip.HipError, match=r"precision='fp64'"):
        eng.weight_gradients(torch.rand(3, 1, 28, 28), torch.tensor([0, 9, 4]), 4)
    assert recorder.calls == []


@pytest.mark.parametrize("arch", ["fc", "fc2"])
def test_weight_gradients_refuses_before_anything_is_launched(recorder, arch):
    eng = AttackEngine(Post(arch), kernels=recorder(), precision="fp64")
    x, y = torch.rand(3, 1, 28, 28), torch.tensor([0, 9, 4])
    with pytest.raises(_hip.HipError, match=r"fp64.*requires_grad"):
        eng.weight_gradients(x.clone().requires_grad_(True), y, 4)
    for reduction in ("none", "Sum", None):
        with pytest.raises(_hip.HipError, match=r"fp64.*reduction"):
            eng.weight_gradients(x, y, 4, reduction=reduction)
    for bad in (torch.tensor([0, 10, 4]), torch.tensor([0, -1, 4])):
        with pytest.raises(_hip.HipError, match=r"fp64.*labels in \[0, 10\)"):
            eng.weight_gradients(x, bad, 4)
    with pytest.raises(_hip.HipError, match=r"fp64.*at least one point"):
        eng.weight_gradients(x[:0], y[:0], 4)
    assert recorder.calls == []


def test_weight_gradient_kernels_use_no_scratch_and_fit_the_lds():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    if not os.path.exists(KR.READELF):
        pytest.skip("llvm-readelf not in this image")
    res = KR.kernel_resources()
    new = {n: r for n, r in res.items() if re.search(r"::fwg_\w+_dp_kernel", n)}
    kinds = sorted(re.search(r"fwg_(\w+)_dp_kernel", n).group(1) for n in new)
    # the hidden activations: 4 activations x (fc: X in fp32, fc2: hid1 in fp64); the contraction: B in fp32 (X) or in fp64
    assert kinds == ["contract"] * 2 + ["hidden"] * 8, sorted(new)
    for n, r in new.items():
        assert r["scratch"] == 0 and r["spill_vgpr"] == 0 and r["lds"] <= 160 * 1024, (n, r)
    # the pinned sets of the fp64 mode are as they were: no new *_f64_kernel
    assert len([n for n in res if "f64_kernel" in n]) == 21
    assert not [n for n in new if "f64" in n or "fp64" in n]
