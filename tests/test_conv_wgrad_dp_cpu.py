"""Host side of the fp64 conv weight-gradient checker (no GPU): the three C-ABI additions and their argument checks, what
ConvFp64Engine.weight_gradients refuses before anything is launched, and the resources of its kernels read from the built library.
Everything here but the two tests of what stays as it was (precision='fp64' refusing conv, the present kernel counts) fails on a tree without
the feature: the method, the include file and the three C names do not exist there."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

from robustbnns_amd import _hip

pytestmark = pytest.mark.usefixtures("built_library")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"rbnn_conv_wgrad_dp_workspace_query", "rbnn_conv_head_ce_dp", "rbnn_conv_weight_grads_dp"}
VP, I32, F64 = C.c_void_p, C.c_int32, C.c_double


class Recorder:
    """Stands where the kernels stand and records every call made through it: `calls` stays empty while nothing is launched."""
    calls = []

    def __getattr__(self, name):
        return lambda *a, **k: Recorder.calls.append(name)


class Post:
    """As much of a ConvStackedPosterior as the engine's constructor and the refusals read."""

    def __init__(self):
        self.arch, self.device, self.S, self.C, self.D, self.Dp, self.H = "conv", torch.device("cuda"), 4, 10, 784, 784, 64


@pytest.fixture
def recorder(monkeypatch):
    Recorder.calls = []
    monkeypatch.setattr(_hip, "HipKernels", Recorder)
    return Recorder


def test_header_declares_the_three_entry_points_and_the_abi_is_unchanged():
    import __graft_entry__ as G
    hdr = open(_hip.HEADER_PATH).read()
    declared = set(re.findall(r"\b(rbnn_\w+)\s*\(", hdr))
    assert NAMES <= declared and NAMES <= set(_hip.SIGNATURES)
    assert not [n for n in NAMES if "fp64" in n or "f64" in n or "svi_multi" in n or "lockstep" in n]      # the fences of the other host tests
    assert "#define RBNN_ABI_VERSION 10" in hdr and _hip.ABI_VERSION == 10 and _hip.load().rbnn_abi_version() == 10
    assert len(G.SOURCES) == 12 and any(d.endswith("rbnn_conv_wgrad_dp.inc") for d in G.DEPS)
    src = open(os.path.join(G.CSRC, "rbnn_conv.hip")).read()
    assert src.index('#include "rbnn_conv_fp64.inc"') < src.index('#include "rbnn_conv_wgrad_dp.inc"')
    assert _hip.CONV_FP64_WS_BUFFERS == 8 and _hip.CONV_WGRAD_DP_WS_BUFFERS == len(_hip.CONV_WGRAD_DP_WS_KEYS) == 3
    assert _hip.CONV_WGRAD_DP_WS_KEYS == ("ce", "dO2", "dO1")
    cp = C.POINTER(_hip.ConvPosterior)
    assert _hip.SIGNATURES["rbnn_conv_wgrad_dp_workspace_query"] == (I32, [cp, I32, I32, VP])
    assert _hip.SIGNATURES["rbnn_conv_head_ce_dp"] == (I32, [VP, VP, I32, I32, I32, F64, VP, VP, VP])
    assert _hip.SIGNATURES["rbnn_conv_weight_grads_dp"] == (I32, [cp, VP, I32, VP, I32, I32] + [VP] * 14)
    for m in ("conv_wgrad_dp_workspace_sizes", "conv_head_ce_dp", "conv_weight_grads_dp"):
        assert callable(getattr(_hip.HipKernels, m))


def _net(cin, w, hc=48, c=10):
    net = _hip.ConvPosterior()
    net.activation, net.hidden, net.n_classes, net.n_stored, net.in_channels, net.in_width = 1, hc, c, 5, cin, w
    return net


@pytest.mark.parametrize("cin,w", [(1, 28), (3, 32)])
def test_workspace_query_follows_the_formula(cin, w):
    """N points x S samples, all doubles: the per-point CE; dL/d(conv2 pre-activation), Hc channels of O2W^2 positions; dL/d(conv1
    pre-activation), 32 channels of O1^2 positions.  O1 = W - 4, O2W = O1 / 2 - 4."""
    lib, N, S, hc = _hip.load(), 7, 3, 48
    o1 = w - 4
    npos = (o1 // 2 - 4) ** 2
    out = (C.c_size_t * 3)()
    assert lib.rbnn_conv_wgrad_dp_workspace_query(C.byref(_net(cin, w, hc)), N, S, out) == 0
    assert list(out) == [S * N * 8, S * N * hc * npos * 8, S * N * 32 * o1 * o1 * 8]
    assert (npos, o1 * o1) == ((64, 576) if w == 28 else (100, 784))
    # the issue's figure: about 0.65 MB per (sample, point) at Hc = 512 on 1x28x28, the forward's workspaces included
    assert lib.rbnn_conv_wgrad_dp_workspace_query(C.byref(_net(1, 28, 512)), 1, 1, out) == 0
    fwd = (C.c_size_t * 8)()
    assert lib.rbnn_conv_fp64_workspace_query(C.byref(_net(1, 28, 512)), 1, 1, fwd) == 0
    assert 0.6e6 < sum(out) + sum(fwd) < 0.7e6


def test_every_argument_error_returns_its_code_before_any_launch():
    """Fake pointers: a call that got past the checks would fault."""
    lib, p = _hip.load(), 4096
    out = (C.c_size_t * 3)()
    q = lib.rbnn_conv_wgrad_dp_workspace_query
    assert q(None, 4, 2, out) == _hip.ERR_NULL and q(C.byref(_net(1, 28)), 4, 2, None) == _hip.ERR_NULL
    assert q(C.byref(_net(1, 32)), 4, 2, out) == _hip.ERR_UNSUPPORTED and q(C.byref(_net(3, 28)), 4, 2, out) == _hip.ERR_UNSUPPORTED
    assert q(C.byref(_net(1, 28, hc=40)), 4, 2, out) == _hip.ERR_SHAPE and q(C.byref(_net(1, 28)), 0, 2, out) == _hip.ERR_SHAPE
    assert q(C.byref(_net(1, 28)), 4, 0, out) == _hip.ERR_SHAPE

    def head(Z=p, labels=p, S=2, N=4, Cn=10, dZ=2 * p, ce=3 * p):
        return lib.rbnn_conv_head_ce_dp(Z, labels, S, N, Cn, 1.0, dZ, ce, None)
    for k in ("Z", "labels", "dZ", "ce"):
        assert head(**{k: None}) == _hip.ERR_NULL, k
    assert head(N=0) == _hip.ERR_SHAPE and head(S=0) == _hip.ERR_SHAPE and head(N=1 << 20, S=1 << 12) == _hip.ERR_SHAPE
    assert head(Cn=0) == _hip.ERR_SHAPE and head(Cn=17) == _hip.ERR_SHAPE
    assert head(Z=p + 8) == _hip.ERR_ALIGN and head(dZ=2 * p + 8) == _hip.ERR_ALIGN
    assert head(dZ=p) == _hip.ERR_UNSUPPORTED                                                                # in place

    bufs = ("X", "dZ", "P1", "a1", "Q2", "a2", "dO2", "dO1", "dK1w", "dK1b", "dK2w", "dK2b", "dFw", "dFb")

    def wg(net, ldx=784, N=4, S=2, **kw):
        b = {k: p for k in bufs}
        b.update(kw)
        return lib.rbnn_conv_weight_grads_dp(C.byref(net), b["X"], ldx, None, S, N, *(b[k] for k in bufs[1:]), None)

    assert wg(_net(1, 28)) == _hip.ERR_NULL                                                                  # no weights

    def full(cin=1, w=28, hc=48, c=10):
        net = _net(cin, w, hc, c)
        for k in ("K1w", "K1b", "K2w", "K2b", "Fw", "Fb"):
            setattr(net, k, p)
        return net
    assert wg(full(1, 32)) == _hip.ERR_UNSUPPORTED and wg(full(3, 28)) == _hip.ERR_UNSUPPORTED              # a geometry other than 28 / 1 or 32 / 3
    assert wg(full(hc=40)) == _hip.ERR_SHAPE and wg(full(hc=8)) == _hip.ERR_SHAPE                           # hidden not a multiple of 16
    assert wg(full(c=17)) == _hip.ERR_SHAPE                                                                 # C > 16
    assert wg(full(), N=0) == _hip.ERR_SHAPE and wg(full(), N=1 << 20, S=1 << 12) == _hip.ERR_SHAPE
    net = full()
    net.activation = 9
    assert wg(net) == _hip.ERR_UNSUPPORTED
    net = full()
    for k in bufs:
        assert wg(net, **{k: None}) == _hip.ERR_NULL, k
    assert wg(net, ldx=780) == _hip.ERR_SHAPE and wg(net, ldx=786) == _hip.ERR_SHAPE                         # below Cin*W*W; not a multiple of 4
    assert wg(full(3, 32), ldx=3068) == _hip.ERR_SHAPE
    for k in ("X", "dZ", "P1", "Q2", "dO2", "dO1"):
        assert wg(net, **{k: p + 8}) == _hip.ERR_ALIGN, k


def test_weight_gradients_refuses_before_anything_is_launched(recorder):
    from robustbnns_amd.conv_fp64 import ConvFp64Engine
    eng = ConvFp64Engine(Post(), kernels=recorder())
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


def test_precision_fp64_still_refuses_conv(recorder):
    from robustbnns_amd.engine import AttackEngine
    post = Post()
    post.triple_supported, post.split_supported = (lambda: False), (lambda: False)
    with pytest.raises(_hip.HipError, match=r"fp64.*conv.*ConvFp64Engine"):
        AttackEngine(post, kernels=recorder(), precision="fp64")
    assert recorder.calls == []


def _resources():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    if not os.path.exists(KR.READELF):
        pytest.skip("llvm-readelf not in this image")
    return KR.kernel_resources()


def test_weight_gradient_kernels_use_no_scratch_and_fit_the_lds():
    new = {n: r for n, r in _resources().items() if re.search(r"::cwg_\w+_dp_kernel", n)}
    kinds = sorted(re.search(r"cwg_(\w+)_dp_kernel", n).group(1) for n in new)
    # the backward: 4 activations x 2 geometries; dK2, dK1: per geometry; the head and dFw: one each
    assert kinds == ["backward"] * 8 + ["dfw"] + ["dk1"] * 2 + ["dk2"] * 2 + ["head"], sorted(new)
    for n, r in new.items():
        assert r["scratch"] == 0 and r["spill_vgpr"] == 0 and r["lds"] <= 160 * 1024, (n, r)
    # the backward takes its LDS at launch (dynamic): the size the launcher asks for, restated from rbnn_conv_wgrad_dp.inc
    for w in (28, 32):
        p1w = (w - 4) // 2
        o2w, np2, p1sz = p1w - 4, (p1w - 5) ** 2, 32 * p1w * p1w
        assert (16 * (o2w + 8) ** 2 + 16 * np2 + 16 + p1sz) * 8 + 2 * 400 * 4 + p1sz <= 160 * 1024, w


def test_the_present_kernel_counts_are_unchanged():
    res = _resources()
    assert len([n for n in res if "conv" in n and "fp64" in n]) == 27
    assert len([n for n in res if "f64_kernel" in n]) == 21
    assert not [n for n in res if "cwg_" in n and ("fp64" in n or "f64_kernel" in n)]
