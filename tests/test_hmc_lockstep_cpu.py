"""CPU tests (-m "not gpu") of the lockstep HMC chains: the guards of hmc.LockstepHmc / BNN.train_hmc(num_chains) / lockstep_train,
hmc.split_r_hat against its closed form, the additive C-ABI (header, SIGNATURES, host-side argument checks) and the kernels' resources."""
import ctypes as C
import math
import os
import re
import sys

import pytest
import torch

import svi_restate as R
from robustbnns_amd import _hip, hmc
from robustbnns_amd.grid_search_halfMoons import MoonsBNN, lockstep_train

pytestmark = pytest.mark.usefixtures("built_library")

NAMES = {"rbnn_hmc_lockstep_gradient", "rbnn_hmc_lockstep_momentum", "rbnn_hmc_lockstep_update", "rbnn_hmc_lockstep_decide",
         "rbnn_hmc_lockstep_commit", "rbnn_hmc_lockstep_window_end"}


def _net(arch, D, H, Cn, seed):
    g = torch.Generator().manual_seed(seed)
    return {k: torch.rand(*s, generator=g) * 4 - 2 for k, s in R.shapes_of(arch, D, H, Cn).items()}


def test_guards():
    q0 = _net("fc", 2, 8, 2, 0)
    with pytest.raises(NotImplementedError, match="no CPU compute path"):
        hmc.LockstepHmc("fc", "leaky", (1, 2, 1), 2, [q0, q0], 0.01, 10, "cpu", [1, 2])
    with pytest.raises(NotImplementedError, match="conv"):
        hmc.LockstepHmc("conv", "leaky", (1, 28, 28), 10, [q0, q0], 0.01, 10, "cuda:0", [1, 2])
    with pytest.raises(ValueError, match="one key per chain"):
        hmc.LockstepHmc("fc", "leaky", (1, 2, 1), 2, [q0, q0], 0.01, 10, "cuda:0", [1])
    with pytest.raises(ValueError, match="at least one chain"):
        hmc.LockstepHmc("fc", "leaky", (1, 2, 1), 2, [], 0.01, 10, "cuda:0", [])
    x, y = R.two_moons(16, 0.1, 0)
    loader = torch.utils.data.DataLoader(list(zip(x, y)), batch_size=8)
    net = MoonsBNN(16, "leaky", "fc", "hmc", None, None, 5, 5, 16, (1, 2, 1), 2)
    for bad in (0, -1):
        with pytest.raises(ValueError, match="num_chains"):
            net.train_hmc(loader, "cuda:0", "out/", num_chains=bad)
    with pytest.raises(NotImplementedError, match="no CPU compute path"):
        net.train_hmc(loader, "cpu", "out/", num_chains=2)
    grid = ([16], ["leaky"], ["fc"], ["hmc"], [None], [None], [5], [5], [16], [5])
    with pytest.raises(NotImplementedError, match="no CPU compute path"):
        lockstep_train(*grid, "out/", x_train=x, y_train=y, device="cpu")
    with pytest.raises(NotImplementedError, match="conv"):
        lockstep_train([16], ["leaky"], ["conv"], ["hmc"], [None], [None], [5], [5], [16], [5], "out/", x_train=x, y_train=y, device="cuda:0")
    assert not os.path.exists("out")                                         # a refusal writes nothing


def test_split_r_hat():
    g = torch.Generator().manual_seed(0)
    row = torch.randn(40, generator=g, dtype=torch.float64)
    # identical chains whose halves agree: a sequence followed by itself, K times -> every half-sequence is the same, B = 0
    same = torch.cat([row[:20], row[:20]]).repeat(3, 1)
    assert hmc.split_r_hat(same) == pytest.approx(math.sqrt(19 / 20), abs=1e-15)
    # ... which tends to 1 with the length; exactly 1 for constant chains
    assert hmc.split_r_hat(torch.ones(2, 8)) == 1.0
    # by hand, 2 x 4: halves (1, 2), (3, 4), (2, 4), (6, 8): h = 2, variances 1/2, 1/2, 2, 2 -> W = 5/4; means 3/2, 7/2, 3, 7 with mean 15/4:
    # var = ((9/4)^2 + (1/4)^2 + (3/4)^2 + (13/4)^2) / 3 = (260 / 16) / 3 = 65/12 = B / h.  R-hat^2 = (W / 2 + 65/12) / W = 1/2 + 13/3 = 29/6
    v = torch.tensor([[1.0, 2.0, 3.0, 4.0], [2.0, 4.0, 6.0, 8.0]])
    assert hmc.split_r_hat(v) == pytest.approx(math.sqrt(29 / 6), rel=1e-14)
    # an odd length drops the middle draw: (1, 2 | x | 3, 4)
    v5 = torch.tensor([[1.0, 2.0, 99.0, 3.0, 4.0], [2.0, 4.0, -99.0, 6.0, 8.0]])
    assert hmc.split_r_hat(v5) == pytest.approx(math.sqrt(29 / 6), rel=1e-14)
    # identical long chains, and chains of one stationary law: 1 within the figure's own noise; a chain many standard deviations apart: far above
    a = torch.randn(4, 400, generator=g, dtype=torch.float64)
    assert abs(hmc.split_r_hat(a[:1].repeat(4, 1)) - 1) < 0.05
    assert abs(hmc.split_r_hat(a) - 1) < 0.05
    a[0] += 10
    assert hmc.split_r_hat(a) > 2
    with pytest.raises(ValueError):
        hmc.split_r_hat(torch.zeros(2, 3))


def test_lockstep_entry_points_are_additive_and_validate_without_a_gpu():
    assert NAMES <= set(_hip.SIGNATURES) and _hip.ABI_VERSION == 10
    hdr = open(_hip.HEADER_PATH).read()
    assert "#define RBNN_ABI_VERSION 10" in hdr
    new = {n for n in re.findall(r"\b(rbnn_\w+)\s*\(", hdr) if "lockstep" in n}
    assert new == NAMES, new ^ NAMES                                         # every new header symbol has its signature
    fields = re.search(r"typedef struct rbnn_hmc_lockstep \{(.*?)\} rbnn_hmc_lockstep;", hdr, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    declared = [n for n in re.findall(r"\*?\b([a-z_0-9]+)\s*[,;]", fields)]
    assert declared == [f[0] for f in _hip.HmcLockstep._fields_], declared   # the struct, field by field in order
    lib = _hip.load()
    net = _hip.NnTrainNet()
    net.arch, net.activation, net.in_features, net.hidden, net.n_classes, net.n_members = 1, 1, 2, 32, 2, 3
    n = 2 * 32 + 32 + 32 * 32 + 32 + 2 * 32 + 2
    net.member_stride = n
    ch = _hip.HmcLockstep()                                                  # every pointer NULL: refused before any launch
    ws = _hip.NnTrainWs()
    assert lib.rbnn_hmc_lockstep_gradient(C.byref(net), None, 2, 8, None, None, None, 4, C.byref(ws), None) == -1
    assert lib.rbnn_hmc_lockstep_momentum(C.byref(net), C.byref(ch), 0, 0, None, None) == -1
    assert lib.rbnn_hmc_lockstep_update(C.byref(net), C.byref(ch), 0, -1, None) == -1
    assert lib.rbnn_hmc_lockstep_decide(C.byref(net), C.byref(ch), None, None, 4, 0, 2, 0, 0, None) == -1
    assert lib.rbnn_hmc_lockstep_commit(C.byref(net), C.byref(ch), 0, 0, -1, None) == -1
    assert lib.rbnn_hmc_lockstep_window_end(C.byref(net), C.byref(ch), 25, None) == -1
    assert lib.rbnn_hmc_lockstep_momentum(None, C.byref(ch), 0, 0, None, None) == -1
    assert lib.rbnn_hmc_lockstep_momentum(C.byref(net), None, 0, 0, None, None) == -1
    # non-NULL (never dereferenced: every call below is refused on the host) pointers, then each shape rule
    buf = (C.c_double * 8)()
    for name, _ in _hip.HmcLockstep._fields_[:13]:
        setattr(ch, name, C.addressof(buf))
    ch.chain_stride, ch.qpart_stride, ch.epart_stride = n, 2, 5
    net.P = net.grad = C.addressof(buf)
    shape, unsupported = -2, -3
    assert lib.rbnn_strerror(shape) != lib.rbnn_strerror(unsupported)
    for field, bad in (("chain_stride", n - 1), ("chain_stride", n + 1), ("qpart_stride", 1), ("epart_stride", 4), ("log_rows", -1)):
        keep = getattr(ch, field)
        setattr(ch, field, bad)
        assert lib.rbnn_hmc_lockstep_momentum(C.byref(net), C.byref(ch), 0, 0, None, None) == shape, (field, bad)
        setattr(ch, field, keep)
    for members in (0, 65536):
        net.n_members = members
        assert lib.rbnn_hmc_lockstep_commit(C.byref(net), C.byref(ch), 0, 0, -1, None) == shape
    net.n_members = 3
    assert lib.rbnn_hmc_lockstep_update(C.byref(net), C.byref(ch), 6, -1, None) == unsupported
    ch.steps = None
    assert lib.rbnn_hmc_lockstep_update(C.byref(net), C.byref(ch), 1, 0, None) == -1          # a step needs the chains' lengths
    assert lib.rbnn_hmc_lockstep_window_end(C.byref(net), C.byref(ch), 1, None) == shape
    assert lib.rbnn_hmc_lockstep_commit(C.byref(net), C.byref(ch), 0, -1, -1, None) == shape
    assert lib.rbnn_hmc_lockstep_commit(C.byref(net), C.byref(ch), 0, 0, 0, None) == shape   # a sample row behind the (empty) stacks
    ch.samples = None
    assert lib.rbnn_hmc_lockstep_commit(C.byref(net), C.byref(ch), 0, 0, 0, None) == -1      # a sample row without a stack
    assert lib.rbnn_hmc_lockstep_decide(C.byref(net), C.byref(ch), C.addressof(buf), None, 0, 0, 2, 0, 0, None) == shape
    assert lib.rbnn_hmc_lockstep_decide(C.byref(net), C.byref(ch), C.addressof(buf), None, 4, 0, 3, 0, 0, None) == unsupported
    net.activation = 4
    assert lib.rbnn_hmc_lockstep_momentum(C.byref(net), C.byref(ch), 0, 0, None, None) == unsupported


def test_lockstep_kernels_use_no_scratch():
    """Every lockstep kernel of csrc/rbnn_hmc.hip, and the lockstep GEMM / head kernels it launches, hold everything in registers (read from the
    code objects of the built library: no GPU)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources as KR
    if not os.path.exists(KR.READELF):
        pytest.skip("llvm-readelf not in this image")
    res = {n: r for n, r in KR.kernel_resources().items() if re.search(r"::(lockstep_\w+_kernel|train_(gemm|head)_kernel<true, false>)", n)}
    assert len(res) == 11, sorted(res)     # four element-wise templates in two views, the decision, the GEMM and the head
    bad = {n: (r["scratch"], r["spill_vgpr"]) for n, r in res.items() if r["scratch"] or r["spill_vgpr"]}
    assert not bad, bad
