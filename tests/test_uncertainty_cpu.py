"""Host side of the predictive uncertainty (no GPU): the three C-ABI additions, their generated signatures and argument checks, the one
translation unit that holds them, what uncertainty.py and the engines refuse before the library is loaded, the resources of the new kernels
read from the built library, and tests/uncertainty_restate.py against a plain float64 torch formula, its bin rule at exact edges and the AUROC
with ties against a count of every pair.  Everything but the restatement tests fails on a tree without the feature: the module, the include
file and the C names do not exist there (the restatement file does not either)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

import uncertainty_restate as R
from robustbnns_amd import _hip

pytestmark = pytest.mark.usefixtures("built_library")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"rbnn_predictive_stats", "rbnn_predictive_calibration_query", "rbnn_predictive_calibration"}
VP, I32, I64, SZ = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t


def test_header_declares_the_entry_points_and_the_abi_is_unchanged():
    import __graft_entry__ as G
    hdr = open(_hip.HEADER_PATH).read()
    declared = set(re.findall(r"\b(rbnn_\w+)\s*\(", hdr))
    assert NAMES <= declared and NAMES <= set(_hip.SIGNATURES)
    assert {n for n in declared if n.startswith("rbnn_predictive")} == NAMES
    # the fences of the other host tests
    assert not [n for n in NAMES if re.search("f64|fp64|svi_multi|lockstep|cwg_|wpca|chain_diag", n)
                or n.startswith(("rbnn_wpca_", "rbnn_conv_hmc_", "rbnn_chain_diag"))]
    assert "#define RBNN_ABI_VERSION 10" in hdr and _hip.ABI_VERSION == 10 and _hip.load().rbnn_abi_version() == 10
    assert len(G.SOURCES) == 12 and any(d.endswith("rbnn_predictive.inc") for d in G.DEPS)
    units = [s for s in G.SOURCES if '#include "rbnn_predictive.inc"' in open(s).read()]
    assert len(units) == 1                                                        # one translation unit holds it
    # every constant of the section surfaces in the generated bindings
    consts = dict(re.findall(r"#define RBNN_(PREDICTIVE_\w+)\s+(\d+)", hdr))
    assert set(consts) == {"PREDICTIVE_FLOAT", "PREDICTIVE_DOUBLE", "PREDICTIVE_MAX_PREFIXES", "PREDICTIVE_MAX_BINS", "PREDICTIVE_BLOCK"}
    for k, v in consts.items():
        assert getattr(_hip, k) == int(v), k
    assert (_hip.PREDICTIVE_MAX_PREFIXES, _hip.PREDICTIVE_MAX_BINS) == (8, 64)
    # no struct came with it; the element type of P is an argument, not a suffix
    assert not [s for s in _hip.HEADER.structs if "predictive" in s]
    assert _hip.SIGNATURES["rbnn_predictive_stats"] == (I32, [VP, I32, I64, I32, I32, I32, I32, VP, VP, I32, I64] + [VP] * 10 + [VP])
    assert _hip.SIGNATURES["rbnn_predictive_calibration_query"] == (I32, [I32, I32, VP])
    assert _hip.SIGNATURES["rbnn_predictive_calibration"] == (I32, [VP, VP, VP, VP, I32, I32, VP, VP, VP, VP, VP, VP, SZ, VP])
    assert len(_hip.HipKernels.PREDICTIVE_OUTPUTS) == 10


def test_every_argument_error_returns_its_code_before_any_launch():
    """Fake pointers: a call that got past the checks would fault."""
    lib, p = _hip.load(), 4096
    NULL, SHAPE, ALIGN = _hip.ERR_NULL, _hip.ERR_SHAPE, _hip.ERR_ALIGN

    def stats(P=p, elem=_hip.PREDICTIVE_FLOAT, ss=5 * 16, ldp=16, S=7, N=5, Cn=10, labels=p, pre=(1, 3, 7), J=None, os_=5, outs=None):
        arr = None if pre is None else (I32 * max(1, len(pre)))(*pre)
        outs = [p] * 10 if outs is None else outs
        return lib.rbnn_predictive_stats(P, elem, ss, ldp, S, N, Cn, labels, arr, len(pre or ()) if J is None else J, os_, *outs, None)
    assert stats(P=None) == NULL and stats(pre=None, J=1) == NULL
    assert stats(labels=None) == NULL                                       # nll, brier and correct need labels
    for bad in (dict(Cn=1), dict(Cn=17, ldp=17, ss=5 * 17), dict(Cn=0), dict(S=0), dict(N=0), dict(N=-3), dict(ldp=9), dict(ss=5 * 16 - 1), dict(os_=4),
                dict(pre=(), J=0), dict(pre=tuple(range(1, 10)), S=9), dict(pre=(3, 3)), dict(pre=(3, 1)), dict(pre=(0, 1)), dict(pre=(1, 8)),
                dict(elem=2), dict(elem=-1), dict(ss=2 ** 62), dict(os_=2 ** 62)):
        assert stats(**bad) == SHAPE, bad
    assert stats(P=p + 2) == ALIGN and stats(P=p + 4, elem=_hip.PREDICTIVE_DOUBLE) == ALIGN and stats(labels=p + 2) == ALIGN
    for i in range(10):
        outs = [p] * 10
        outs[i] = p + (4 if i < 8 else 2)                                   # a double output on a 4-byte border, an int32 one on a 2-byte border
        assert stats(outs=outs) == ALIGN, i
    # with every output null there is nothing to launch; without labels the label outputs must be null
    assert stats(outs=[None] * 10) == 0 and stats(labels=None, outs=[None] * 10) == 0

    need = SZ(0)
    assert lib.rbnn_predictive_calibration_query(4099, 15, C.byref(need)) == 0 and need.value == 17 * 48 * 8
    assert lib.rbnn_predictive_calibration_query(1, 1, C.byref(need)) == 0 and need.value == 6 * 8
    assert lib.rbnn_predictive_calibration_query(1, 1, None) == NULL

    def cal(conf=p, ok=p, nll=p, brier=p, N=300, nb=15, outs=(p,) * 5, ws=p, ws_bytes=2 * 48 * 8):
        return lib.rbnn_predictive_calibration(conf, ok, nll, brier, N, nb, *outs, ws, ws_bytes, None)
    assert cal(conf=None) == NULL and cal(ok=None) == NULL and cal(ws=None) == NULL
    for bad in (dict(N=0), dict(nb=0), dict(nb=65), dict(nb=-1), dict(ws_bytes=2 * 48 * 8 - 1), dict(N=513)):
        assert cal(**bad) == SHAPE, bad
        if "ws_bytes" not in bad and bad != dict(N=513):
            assert lib.rbnn_predictive_calibration_query(bad.get("N", 300), bad.get("nb", 15), C.byref(need)) == SHAPE, bad
    assert cal(conf=p + 4) == ALIGN and cal(ok=p + 2) == ALIGN and cal(ws=p + 4) == ALIGN and cal(outs=(p, p + 4, p, p, p)) == ALIGN
    assert cal(outs=(None,) * 5) == 0


@pytest.fixture
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the library was loaded before the refusal")
    monkeypatch.setattr(_hip, "load", refuse)


class _CpuNet:
    device = "cpu"


class _Engine:
    """What the engine-level refusals read."""
    def __init__(self, world=1, device="cpu"):
        self.world, self.device, self.k = world, torch.device(device), object()
        self.post = type("P", (), {"S": 8, "C": 10})()


def test_refusals_fire_before_the_library_is_loaded(no_library):
    from robustbnns_amd import uncertainty as U
    assert U.FIELDS == R.FIELDS and U.PredictiveUncertainty._fields == R.FIELDS
    x = torch.zeros(4, 1, 28, 28)
    with pytest.raises(NotImplementedError, match=r"MI355X kernels only \(device 'cpu'\).*load the net on 'cuda'"):
        U.predictive_uncertainty(_CpuNet(), x, 3)
    with pytest.raises(NotImplementedError, match=r"MI355X kernels only \(device 'cpu'\)"):
        U.engine_uncertainty(_Engine(), x, 3)
    with pytest.raises(NotImplementedError, match=r"MI355X kernels only"):
        U.engine_sample_outputs(_Engine(), x, 3)
    with pytest.raises(NotImplementedError, match=r"process group \(world size 2\).*single-GPU engine"):
        U.engine_uncertainty(_Engine(world=2, device="cuda"), x, 3)
    with pytest.raises(NotImplementedError, match=r"process group"):
        U.engine_sample_outputs(_Engine(world=2, device="cuda"), x, 3)
    with pytest.raises(ValueError, match="avg_posterior=True is one net of mean weights, not a distribution.*leave avg_posterior False"):
        U.predictive_uncertainty(_CpuNet(), x, 3, avg_posterior=True)
    for bad, word in (([], "empty"), ([3, 2], "strictly ascending"), ([2, 2], "strictly ascending"), ([0, 2], "leaves 1 .. n_samples = 5"),
                      ([2, 6], "leaves 1 .. n_samples = 5"), (list(range(1, 10)), "holds 9 lengths, one call takes 8")):
        with pytest.raises(ValueError, match=word):
            U.engine_uncertainty(_Engine(), x, 9 if len(bad) == 9 else 5, n_samples_list=bad)
    assert U.check_prefixes(5, None) == [5] and U.check_prefixes(5, (1, 3, 5)) == [1, 3, 5]
    with pytest.raises(ValueError, match="n_samples >= 1"):
        U.engine_uncertainty(_Engine(), x, 0)
    with pytest.raises(ValueError, match="y holds 3 labels for 4 points"):
        U.engine_uncertainty(_Engine(), x, 3, y=torch.zeros(3, dtype=torch.long))
    with pytest.raises(ValueError, match="y holds 5 labels for 4 points"):
        U.engine_uncertainty(_Engine(), x, 3, y=torch.zeros(5, 10))
    z = torch.zeros(4, dtype=torch.float64)
    unc = U.PredictiveUncertainty(z, z, z, z, z, z, z, z, z.int(), z.int())
    for nb in (0, 65, -2):
        with pytest.raises(ValueError, match=rf"1 <= n_bins <= 64, not {nb}"):
            U.calibration(unc, nb)
    with pytest.raises(ValueError, match="needs the figures that labels give"):
        U.calibration(unc._replace(correct=None, nll=None, brier=None))
    with pytest.raises(ValueError, match="pick a row"):
        U.calibration(U.PredictiveUncertainty(*(f.reshape(1, 4) for f in unc)))
    with pytest.raises(NotImplementedError, match="MI355X kernels only"):
        U.calibration(unc)


def test_the_new_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    if not os.path.exists(KR.READELF):
        pytest.skip("llvm-readelf not in this image")
    res = KR.kernel_resources()
    new = {n: r for n, r in res.items() if re.search(r"::predictive_\w+_kernel", n)}
    stats = sorted(re.search(r"predictive_stats_kernel<(\w+), (\w+)>", n).groups() for n in new if "stats" in n)
    assert stats == [("double", "false"), ("double", "true"), ("float", "false"), ("float", "true")], sorted(new)
    assert len(new) == 6 and sum("predictive_bins_kernel" in n for n in new) == 1 and sum("predictive_bins_sum_kernel" in n for n in new) == 1
    for n, r in new.items():
        assert r["scratch"] == 0 and r["spill_vgpr"] == 0 and r["lds"] <= 16 * 1024, (n, r)
    assert not [n for n in new if re.search("f64|fp64|wpca|cwg_|lockstep|svi_multi|chain_diag", n)]


def torch_formula(P, Cn, S, y):
    """The definitions as a user would write them in float64 torch."""
    p = torch.from_numpy(np.asarray(P)[:S, :, :Cn].astype(np.float64))
    pbar = p.mean(0)
    ent = lambda q: -(torch.where(q > 0, q * torch.log(torch.where(q > 0, q, torch.ones_like(q))), torch.zeros_like(q))).sum(-1)
    pred = pbar.argmax(-1)
    rows = torch.arange(p.shape[1])
    yt = torch.from_numpy(np.asarray(y).astype(np.int64))
    out = {"entropy": ent(pbar), "expected_entropy": ent(p).mean(0), "confidence": pbar[rows, pred], "prediction": pred.int(),
           "agreement": (p.argmax(-1) == pred).double().sum(0) / S, "variance": p[:, rows, pred].var(0, unbiased=False),
           "nll": -torch.log(pbar[rows, yt]), "brier": ((pbar - torch.nn.functional.one_hot(yt, Cn)) ** 2).sum(-1), "correct": (pred == yt).int()}
    out["mutual_information"] = out["entropy"] - out["expected_entropy"]
    return {k: v.numpy() for k, v in out.items()}


@pytest.mark.parametrize("S,N,C_", [(1, 1, 2), (3, 5, 10), (7, 67, 10), (100, 130, 10), (64, 300, 3)])
def test_the_restatement_is_the_plain_formula(S, N, C_):
    """tests/uncertainty_restate.py against float64 torch on its own planted inputs, at the bars the device is held to (float64 against
    longdouble stayed within 0.04 of them when the bars were derived)."""
    P, y = R.planted(S, N, C_)
    ref = R.restate(P, C_, S, y)
    worst = R.check(torch_formula(P, C_, S, y), ref, S, C_, f"{(S, N, C_)}")
    print(f"[uncertainty restate] {(S, N, C_)}: float64 torch against longdouble, worst error / bar {worst}")
    assert np.isinf(ref.nll).any() == (N > 1)                                  # the planted pbar[y] == 0
    assert (np.asarray(P)[:, :, :C_] == 0).any() == (N > 3)                       # exact zeros: scale 30 in float32, one-hot rows
    # a prefix is the call of that length
    if S >= 3:
        a, b = R.restate(P, C_, 3, y), R.restate(P[:3], C_, 3, y)
        assert all((getattr(a, f) == getattr(b, f)).all() or f == "nll" for f in R.FIELDS)


def test_dyadic_ties_take_the_first_maximum():
    P, y = R.dyadic()
    r = R.restate(P, 4, 8, y)
    assert r.prediction[:6].tolist() == [0, 1, 2, 0, 1, 3]
    assert r.agreement[:6].tolist() == [1.0, 1.0, 0.5, 0.5, 1.0, 1.0]
    assert r.confidence[:6].astype(np.float64).tolist() == [0.25, 0.5, 0.5, 0.25, 0.375, 1.0]
    assert abs(r.variance[2] - 0.25) < 1e-17 and r.variance[0] == 0 and r.mutual_information[2] == r.entropy[2] and r.expected_entropy[2] == 0


def test_the_bin_rule_at_exact_edges():
    from robustbnns_amd import uncertainty as U
    for nb in (1, 4, 10, 15, 64):
        for k in range(nb + 1):
            edge = k / nb                                                   # the float64 nearest the edge: (lo, hi] puts it in the bin below
            want = min(nb - 1, max(0, int(np.ceil(np.float64(edge) * nb)) - 1))
            assert R.bin_of(edge, nb) == U.bin_of(edge, nb) == want, (nb, k)
            if nb in (4, 64):                                               # k / nb and the product are exact: the edge belongs to bin k - 1
                assert want == max(0, k - 1), (nb, k)
                assert R.bin_of(np.nextafter(edge, 2.0), nb) == min(nb - 1, k), (nb, k)
        assert R.bin_of(0.0, nb) == 0 and R.bin_of(1.0, nb) == nb - 1 and R.bin_of(1e-300, nb) == 0
    conf = np.array([0.0, 0.25, 0.25000001, 0.5, 0.75, 1.0, 0.9])
    ok = np.array([1, 0, 1, 1, 0, 1, 1])
    c = R.calibrate(conf, ok, np.zeros(7), np.zeros(7), 4)
    assert c.count.tolist() == [2, 2, 1, 2] and c.good.tolist() == [1, 2, 0, 2] and c.n_correct == 5
    host = U.calibration_from_sums(c.count, c.sconf.astype(np.float64), c.good, np.array([7.0, 3.5]), 5, 7)
    assert abs(host["ece"] - c.ece) <= 1e-15 and abs(host["mce"] - c.mce) <= 1e-15 and host["accuracy"] == 5 / 7
    assert host["nll"] == 1.0 and host["brier"] == 0.5 and host["bins"]["count"].tolist() == [2, 2, 1, 2]
    assert list(host["bins"].columns) == ["lo", "hi", "count", "confidence", "accuracy"]
    empty = U.calibration_from_sums(np.array([0, 3]), np.array([0.0, 2.7]), np.array([0, 3]), np.array([0.0, 0.0]), 3, 3)
    assert np.isnan(empty["bins"]["confidence"][0]) and abs(empty["ece"] - 0.1) < 1e-15 and abs(empty["mce"] - 0.1) < 1e-15


def test_auroc_shares_ranks_among_ties():
    from robustbnns_amd import uncertainty as U
    rng = np.random.default_rng(4)
    for n0, n1, levels in ((1, 1, 2), (7, 5, 3), (40, 33, 6), (50, 50, 1000), (20, 30, 1)):
        neg, pos = rng.integers(0, levels, n0) / levels, (rng.integers(0, levels, n1) + (levels > 1)) / levels
        got = U.auroc(torch.from_numpy(neg), torch.from_numpy(pos))
        assert abs(got - R.auroc_pairs(neg, pos)) <= 1e-14, (n0, n1, levels)
    assert U.auroc(torch.zeros(4), torch.zeros(9)) == 0.5 and U.auroc(torch.zeros(3), torch.ones(2)) == 1.0
    assert U.auroc(torch.ones(3), torch.zeros(2)) == 0.0
    with pytest.raises(ValueError, match="at least one score of each class"):
        U.auroc(torch.zeros(0), torch.ones(2))
