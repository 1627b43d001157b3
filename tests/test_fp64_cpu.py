"""Host side of the fp64 precision mode (no GPU): the C-ABI additions, how the mode is selected and refused, and the resources of its kernels
read from the built library.  Everything here fails on a tree without the mode (precision='fp64' is a ValueError there)."""
import os
import re
import sys

import pytest
import torch

from robustbnns_amd import _hip
from robustbnns_amd.engine import AttackEngine

pytestmark = pytest.mark.usefixtures("built_library")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"rbnn_f64_workspace_query", "rbnn_fc_forward_f64", "rbnn_reduce_samples_f64", "rbnn_loss_dlogits_f64", "rbnn_fc_input_grad_f64",
         "rbnn_attack_step_f64"}


class Recorder:
    """Stands where the kernels stand and records every call made through it: `calls` stays empty while nothing is launched."""
    calls = []

    def __getattr__(self, name):
        return lambda *a, **k: Recorder.calls.append(name)


class OtherKernels:
    """Kernels that are not _hip.HipKernels (the CPU fake of the orchestration tests is one); records into the same list."""
    __getattr__ = Recorder.__getattr__


class Post:
    """As much of a StackedPosterior as the engine's constructor and forward() read."""

    def __init__(self, arch="fc", device="cuda", triple=False, split=False):
        self.arch, self.device, self.S, self.C, self.D, self.Dp, self.Hp = arch, torch.device(device), 4, 10, 784, 784, 512
        self.triple_supported, self.split_supported = (lambda: triple), (lambda: split)


@pytest.fixture
def recorder(monkeypatch):
    """_hip.HipKernels replaced by the recorder (as the conv host tests do): an engine built with `Recorder()` passes for the HIP kernels."""
    Recorder.calls = []
    monkeypatch.setattr(_hip, "HipKernels", Recorder)
    monkeypatch.delenv("RBNN_PRECISION", raising=False)
    return Recorder


def test_header_declares_the_fp64_entry_points_and_the_abi_is_unchanged():
    import __graft_entry__ as G
    hdr = open(_hip.HEADER_PATH).read()
    declared = set(re.findall(r"\b(rbnn_\w+)\s*\(", hdr))
    assert NAMES <= declared and NAMES <= set(_hip.SIGNATURES)
    assert {n for n in declared if "f64" in n} == NAMES
    assert not [n for n in NAMES if "svi_multi" in n or "lockstep" in n]
    assert "#define RBNN_ABI_VERSION 10" in hdr and _hip.ABI_VERSION == 10 and _hip.load().rbnn_abi_version() == 10
    assert len(G.SOURCES) == 12 and any(d.endswith("rbnn_fp64.inc") for d in G.DEPS)
    assert _hip.F64_WS_BUFFERS == len(_hip.F64_WS_KEYS) == 6
    import ctypes as C
    assert _hip.SIGNATURES["rbnn_f64_workspace_query"] == (C.c_int32, [C.POINTER(_hip.Posterior), C.c_int32, C.c_int32, C.c_void_p])
    assert _hip.SIGNATURES["rbnn_reduce_samples_f64"][1][4] is C.c_double and _hip.SIGNATURES["rbnn_loss_dlogits_f64"][1][6] is C.c_double


def test_workspace_query_and_validation_before_any_launch():
    """Sizes of the six fp64 buffers, and the refusals of the entry points on descriptors / arguments they do not take (fake pointers: a
    call that got past the checks would fault)."""
    import ctypes as C
    lib = _hip.load()
    net = _hip.Posterior()
    net.arch, net.activation, net.in_features, net.in_stride, net.hidden, net.n_classes, net.n_stored = 0, 1, 784, 784, 512, 10, 5
    out = (C.c_size_t * 6)()
    assert lib.rbnn_f64_workspace_query(C.byref(net), 33, 5, out) == 0
    assert list(out) == [5 * 33 * 16 * 8, 5 * 33 * 16 * 8, 33 * 16 * 8, 5 * 33 * 512 * 8, 0, 0]
    net.arch = 1
    assert lib.rbnn_f64_workspace_query(C.byref(net), 33, 5, out) == 0 and list(out)[3:] == [5 * 33 * 512 * 8] * 3
    assert lib.rbnn_f64_workspace_query(C.byref(net), 33, 5, None) == _hip.ERR_NULL
    net.hidden = 42                                                          # rows of Wm / W2 must start on 16 bytes
    assert lib.rbnn_f64_workspace_query(C.byref(net), 33, 5, out) == _hip.ERR_SHAPE
    net.hidden, net.arch = 40, 0                                             # a ragged hidden size is fine: 40 % 4 == 0
    assert lib.rbnn_f64_workspace_query(C.byref(net), 1, 1, out) == 0
    p = 4096
    assert lib.rbnn_fc_forward_f64(C.byref(net), p, 784, 4, None, 1, 0, p, p, None, None, None) == _hip.ERR_NULL      # no weights
    for k in ("W1", "b1", "W2", "b2"):
        setattr(net, k, p)
    assert lib.rbnn_fc_forward_f64(C.byref(net), None, 784, 4, None, 1, 0, p, p, None, None, None) == _hip.ERR_NULL
    assert lib.rbnn_fc_forward_f64(C.byref(net), p, 780, 4, None, 1, 0, p, p, None, None, None) == _hip.ERR_SHAPE      # ldx < D_pad
    assert lib.rbnn_fc_forward_f64(C.byref(net), p, 784, 4, None, 1, 7, p, p, None, None, None) == _hip.ERR_UNSUPPORTED
    assert lib.rbnn_fc_forward_f64(C.byref(net), p + 4, 784, 4, None, 1, 0, p, p, None, None, None) == _hip.ERR_ALIGN
    net.arch = 1                                                             # fc2 without Wm / bm
    assert lib.rbnn_fc_forward_f64(C.byref(net), p, 784, 4, None, 1, 0, p, p, p, p, None) == _hip.ERR_NULL
    net.arch = 0
    assert lib.rbnn_fc_input_grad_f64(C.byref(net), None, 1, 4, None, p, None, 1.0, p, 784, None, None, None) == _hip.ERR_NULL
    assert lib.rbnn_fc_input_grad_f64(C.byref(net), None, 1, 4, p, p, None, 1.0, p, 780, None, None, None) == _hip.ERR_SHAPE
    assert lib.rbnn_loss_dlogits_f64(_hip.LOSS_UPSTREAM, p, p, 16, p, 1, 1.0, 4, 10, p, None) == _hip.ERR_UNSUPPORTED  # the autograd hook's modes
    assert lib.rbnn_loss_dlogits_f64(_hip.LOSS_MEAN_PROB, p, None, 16, p, 1, 1.0, 4, 10, p, None) == _hip.ERR_NULL
    assert lib.rbnn_reduce_samples_f64(p, 1, 4, 17, 1.0, p, 16, None) == _hip.ERR_SHAPE
    assert lib.rbnn_attack_step_f64(p, None, 784, p, 784, None, 0.1, 0.3, 1, 4, 784, None) == _hip.ERR_NULL            # PGD form without x0
    assert lib.rbnn_attack_step_f64(p, None, 784, p, 780, None, 0.1, 0.3, 0, 4, 784, None) == _hip.ERR_SHAPE


def test_fp64_is_selected_by_argument_and_by_environment(recorder, monkeypatch):
    assert AttackEngine(Post(), kernels=recorder(), precision="fp64").precision == "fp64"
    assert AttackEngine(Post("fc2"), kernels=recorder(), precision="FP64").precision == "fp64"
    monkeypatch.setenv("RBNN_PRECISION", "fp64")
    assert AttackEngine(Post(), kernels=recorder()).precision == "fp64"
    assert AttackEngine(Post(), kernels=recorder(), precision="exact").precision == "exact"     # the argument still wins over the variable
    with pytest.raises(ValueError, match="fp64"):                                               # an unknown word: still a ValueError, which now lists fp64
        AttackEngine(Post(), kernels=recorder(), precision="fp128")
    assert set(recorder.calls) <= {"lowdim_supported"}                                          # (the question 'exact' asks on its way; fp64 asks nothing)


@pytest.mark.parametrize("triple", [False, True])
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("arch", ["fc", "fc2"])
def test_auto_and_fast_never_resolve_to_fp64(recorder, arch, split, triple):
    for want in ("auto", "fast", None):
        assert AttackEngine(Post(arch, triple=triple, split=split), kernels=recorder(), precision=want).precision in ("exact", "triple", "split")


def test_the_four_refusals_name_fp64_and_launch_nothing(recorder, monkeypatch):
    with pytest.raises(_hip.HipError, match=r"fp64.*conv"):                                     # a conv posterior (ConvEngine builds through this constructor)
        AttackEngine(Post("conv"), kernels=recorder(), precision="fp64")
    from robustbnns_amd.conv import ConvEngine
    with pytest.raises(_hip.HipError, match=r"fp64.*conv"):
        ConvEngine(Post("conv"), kernels=recorder(), precision="fp64")
    import torch.distributed as dist
    with monkeypatch.context() as m:
        m.setattr(dist, "get_world_size", lambda group=None: 2)
        with pytest.raises(_hip.HipError, match=r"fp64.*one GPU"):                              # a process group of more than one rank
            AttackEngine(Post(), kernels=recorder(), group=object(), precision="fp64")
    with pytest.raises(_hip.HipError, match=r"fp64.*CPU device"):                               # a CPU device ...
        AttackEngine(Post(device="cpu"), kernels=recorder(), precision="fp64")
    with pytest.raises(_hip.HipError, match=r"fp64.*substitute kernels"):                       # ... or kernels that are not the HIP kernels
        AttackEngine(Post(), kernels=OtherKernels(), precision="fp64")
    eng = AttackEngine(Post(), kernels=recorder(), precision="fp64")
    x = torch.rand(3, 1, 28, 28, requires_grad=True)
    with pytest.raises(_hip.HipError, match=r"fp64.*autograd hook"):                            # the autograd hook: never answered in fp32
        eng.forward(x, 4)
    with pytest.raises(_hip.HipError, match=r"fp64.*upstream"):
        eng.gradient(None, None, None, 4, _hip.LOSS_UPSTREAM, G_up=torch.zeros(3, 16))
    with pytest.raises(_hip.HipError, match=r"fp64.*label losses"):
        eng.fp64.gradient(None, None, None, 4, _hip.LOSS_UPSTREAM)
    assert recorder.calls == []


def test_point_blocks_follow_the_workspace_budget(recorder, monkeypatch):
    """RBNN_FP64_WS_GB bounds the fp64 workspaces of a block; blocks are whole 16-point tiles, never less than one."""
    eng = AttackEngine(Post(), kernels=recorder(), precision="fp64")
    per_point = 100 * (2 * 16 + 512) * 8 + 16 * 8
    eng.fp64.sizes = [lambda post, N, S: {"all": N * per_point}]
    monkeypatch.delenv("RBNN_FP64_WS_GB", raising=False)
    assert eng.fp64.point_block(100) == 4 * 2 ** 30 // per_point // 16 * 16 == 9856
    assert eng.fp64.point_blocks(10000, 100) == [(0, 9856), (9856, 10000)]
    monkeypatch.setenv("RBNN_FP64_WS_GB", "1e-6")
    assert eng.fp64.point_block(100) == 16 and eng.fp64.point_blocks(33, 100) == [(0, 16), (16, 32), (32, 33)]


def test_the_shared_fp64_rules_have_one_definition_each():
    """One definition each: os.environ.get("RBNN_FP64_WS_GB" occurs once over robustbnns_amd/*.py, in fp64_core.ws_budget; the conv backward's
    stage-2 routing line occurs once over robustbnns_amd/csrc/, in rbnn_conv_fp64.inc's conv_backward_fp64_body."""
    import glob
    pkg = os.path.join(ROOT, "robustbnns_amd")

    def holders(patterns, needle):
        files = sorted(f for p in patterns for f in glob.glob(os.path.join(pkg, p)))
        return {os.path.basename(f): n for f in files if (n := open(f).read().count(needle))}
    csrc = ("csrc/*.hip", "csrc/*.hpp", "csrc/*.inc")
    assert holders(("*.py",), 'os.environ.get("RBNN_FP64_WS_GB"') == {"fp64_core.py": 1}
    assert holders(csrc, "if (ar[p] == (y - py) * 2 + (x - px))") == {"rbnn_conv_fp64.inc": 1}
    assert holders(csrc, "conv_backward_fp64_body<") == {"rbnn_conv_fp64.inc": 1, "rbnn_conv_wgrad_dp.inc": 1}      # the two one-line kernels
    assert holders(csrc, "ss = fma(g, g, ss)") == {"rbnn_fp64_common.hpp": 1}                                        # the row norms


def test_fp64_kernels_use_no_scratch_and_fit_the_lds():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    if not os.path.exists(KR.READELF):
        pytest.skip("llvm-readelf not in this image")
    new = {n: r for n, r in KR.kernel_resources().items() if "f64_kernel" in n}
    kinds = {re.search(r"(\w+_f64_kernel)", n).group(1) for n in new}
    assert kinds == {"fc_forward_f64_kernel", "fc_grad_f64_kernel", "dhid_f64_kernel", "norms_f64_kernel", "reduce_samples_f64_kernel",
                     "loss_dlogits_f64_kernel", "attack_step_f64_kernel"}, kinds
    assert len(new) == 4 * 3 + 4 + 5, sorted(new)            # forward: 4 activations x (fc, fc2 layer 1, fc2 layer 2); gradient: 2 widths x 2 forms
    for n, r in new.items():
        assert r["scratch"] == 0 and r["spill_vgpr"] == 0 and r["lds"] <= 160 * 1024, (n, r)
    assert max(r["lds"] for r in new.values()) > 0            # the forward's hidden chunk does live in LDS: the reader sees it
