"""Host side of the chain diagnostics (no GPU): the two C-ABI additions, their generated signatures and their argument checks, the tile and
LDS formula of the query, what chain_diagnostics refuses before the library is loaded, the resources of the new kernels read from the built
library, and the restatement of tests/chain_diag_restate.py against hmc.split_r_hat.
Everything but the last fails on a tree without the feature: the module, the include file and the C names do not exist there."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

import chain_diag_restate as R
from robustbnns_amd import _hip

pytestmark = pytest.mark.usefixtures("built_library")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"rbnn_chain_diag_query", "rbnn_chain_diag"}
VP, I32, I64, SZ = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t
LDS = 160 * 1024


def test_header_declares_the_entry_points_and_the_abi_is_unchanged():
    import __graft_entry__ as G
    hdr = open(_hip.HEADER_PATH).read()
    declared = set(re.findall(r"\b(rbnn_\w+)\s*\(", hdr))
    assert NAMES <= declared and NAMES <= set(_hip.SIGNATURES)
    assert {n for n in declared if n.startswith("rbnn_chain_diag")} == NAMES
    # the fences of the other host tests
    assert not [n for n in NAMES if re.search("f64|fp64|svi_multi|lockstep|cwg_|wpca", n) or n.startswith(("rbnn_wpca_", "rbnn_conv_hmc_"))]
    assert "#define RBNN_ABI_VERSION 10" in hdr and _hip.ABI_VERSION == 10 and _hip.load().rbnn_abi_version() == 10
    assert len(G.SOURCES) == 12 and any(d.endswith("rbnn_chain_diag.inc") for d in G.DEPS)
    units = [s for s in G.SOURCES if '#include "rbnn_chain_diag.inc"' in open(s).read()]
    assert len(units) == 1                                                        # one translation unit holds it
    assert _hip.CHAIN_DIAG_MAX_DRAWS >= 512
    assert _hip.SIGNATURES["rbnn_chain_diag_query"] == (I32, [I32, I32, I64, VP, VP])
    assert _hip.SIGNATURES["rbnn_chain_diag"] == (I32, [VP, I64, I32, I32, I64, VP, VP, VP, VP, VP, VP, VP, VP])


def test_query_gives_the_cap_and_a_tile_that_fits_the_lds():
    """12 N T bytes per block — the fp32 stage and the fp64 lag accumulators of T columns — with T = 64 or 32 while four blocks fit a CU
    together and 16 beyond; within 160 KiB up to the cap."""
    lib = _hip.load()
    cap, lds = I32(0), SZ(0)
    for n in (4, 5, 53, 54, 106, 107, 250, 512, _hip.CHAIN_DIAG_MAX_DRAWS):
        assert lib.rbnn_chain_diag_query(3, n, 669706, C.byref(cap), C.byref(lds)) == 0
        T = 64 if 4 * 12 * n * 64 <= LDS else 32 if 4 * 12 * n * 32 <= LDS else 16
        assert cap.value == _hip.CHAIN_DIAG_MAX_DRAWS and lds.value == 12 * n * T <= LDS, n
    assert 12 * _hip.CHAIN_DIAG_MAX_DRAWS * 16 <= LDS
    # either output may be left out; the cap is written even when the shape is refused
    assert lib.rbnn_chain_diag_query(3, 64, 100, None, None) == 0
    cap = I32(0)
    assert lib.rbnn_chain_diag_query(3, _hip.CHAIN_DIAG_MAX_DRAWS + 1, 100, C.byref(cap), None) == _hip.ERR_SHAPE
    assert cap.value == _hip.CHAIN_DIAG_MAX_DRAWS


def test_every_argument_error_returns_its_code_before_any_launch():
    """Fake pointers: a call that got past the checks would fault."""
    lib, p = _hip.load(), 4096
    NULL, SHAPE, cap = _hip.ERR_NULL, _hip.ERR_SHAPE, _hip.CHAIN_DIAG_MAX_DRAWS

    def diag(X=p, ldx=8, n_chains=2, n_draws=4, P=8):
        return lib.rbnn_chain_diag(X, ldx, n_chains, n_draws, P, p, p, p, p, p, p, p, None)
    assert diag(X=None) == NULL
    bad_counts = (dict(n_chains=0), dict(n_chains=-1), dict(n_draws=3), dict(n_draws=0), dict(n_draws=cap + 1), dict(P=0), dict(P=-5),
                  dict(n_chains=2 ** 31 // 4, n_draws=4), dict(n_chains=2 ** 31 - 1, n_draws=cap))          # C N >= 2^31
    for bad in bad_counts + (dict(ldx=7), dict(ldx=0), dict(ldx=2 ** 62), dict(P=2 ** 40, ldx=2 ** 40)):
        assert diag(**bad) == SHAPE, bad
    for bad in bad_counts:
        bad = {"n_chains": 2, "n_draws": 4, "P": 8, **bad}
        assert lib.rbnn_chain_diag_query(bad["n_chains"], bad["n_draws"], bad["P"], None, None) == SHAPE, bad
    # with every output null there is nothing to launch
    assert lib.rbnn_chain_diag(p, 8, 2, 4, 8, None, None, None, None, None, None, None, None) == 0


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was loaded before the refusal")
    monkeypatch.setattr(_hip, "load", refuse)


def test_refusals_fire_before_the_library_is_loaded(no_library):
    from robustbnns_amd import chain_diagnostics as D
    assert D.MAX_DRAWS == _hip.CHAIN_DIAG_MAX_DRAWS and D.MIN_DRAWS == 4
    # a device that is not the GPU, in flat_params.require_gpu_fc's wording
    with pytest.raises(NotImplementedError, match=r"runs on the MI355X kernels only \(device .*cpu.*\): there is no CPU compute path"):
        D.diagnose(torch.zeros(8, 5), 2)
    with pytest.raises(ValueError, match="2-D"):
        D.diagnose(torch.zeros(8), 2)
    # the dtype, the counts and the layout are refused before the device is looked at
    z = torch.zeros
    with pytest.raises(ValueError, match="float32 rows, not torch.float64"):
        D.diagnose(z(8, 5, dtype=torch.float64), 2)
    with pytest.raises(ValueError, match="9 draws, not a multiple of their 2 chains"):
        D.diagnose(z(9, 5), 2)
    with pytest.raises(ValueError, match="n_chains >= 1"):
        D.diagnose(z(8, 5), 0)
    with pytest.raises(ValueError, match=rf"4 <= draws per chain <= {D.MAX_DRAWS} .*, not 3"):
        D.diagnose(z(6, 5), 2)
    with pytest.raises(ValueError, match=rf"4 <= draws per chain <= {D.MAX_DRAWS} .*, not {D.MAX_DRAWS + 1}"):
        D.diagnose(z(2 * (D.MAX_DRAWS + 1), 5), 2)
    with pytest.raises(ValueError, match=r"stride\(1\) == 1"):
        D.diagnose(torch.zeros(5, 8).t(), 2)
    with pytest.raises(ValueError, match="row stride"):
        D.diagnose(torch.zeros(1, 5).expand(8, 5), 2)
    with pytest.raises(ValueError, match="positive byte budget"):
        D.diagnose(z(8, 5), 2, ws_bytes=0)


def test_drivers_refuse_a_net_without_a_stack(no_library):
    from robustbnns_amd import chain_diagnostics as D

    class Net:
        hmc_history = {"eps": [], "r_hat_U": 1.0}
    for fn in (D.weight_diagnostics, D.diagnostics_summary, D.print_summary):
        with pytest.raises(ValueError, match=r'num_chains=K.*no "stack"'):
            fn(Net())

    class Untrained:
        pass
    with pytest.raises(ValueError, match="num_chains"):
        D.weight_diagnostics(Untrained())


def test_slab_plan_tiles_the_columns_in_groups_of_64():
    from robustbnns_amd import chain_diagnostics as D
    assert D.slab_plan(669706, 400) == [(0, 669706)]
    for P, rows, budget in [(669706, 400, 64 << 20), (300, 256, 1), (300, 256, 3 * 64 * 256 * 4), (64, 8, 1 << 30), (1, 4, 1)]:
        plan = D.slab_plan(P, rows, budget)
        assert plan[0][0] == 0 and sum(w for _, w in plan) == P and all(a + w == b for (a, w), (b, _) in zip(plan, plan[1:]))
        assert all(e0 % D.SLAB == 0 for e0, _ in plan) and all(w % D.SLAB == 0 for _, w in plan[:-1]) and len({w for _, w in plan[:-1]}) <= 1
        w0 = -(-plan[0][1] // D.SLAB) * D.SLAB
        assert w0 * rows * 4 <= budget or w0 == D.SLAB                                   # within the budget, or the one group nothing is smaller than
        assert len(plan) == 1 or (w0 + D.SLAB) * rows * 4 > budget                       # and the budget is used
    assert D.slab_plan(300, 256, 1) == [(0, 64), (64, 64), (128, 64), (192, 64), (256, 44)]


def test_summary_line_skips_the_constant_weights():
    from robustbnns_amd import chain_diagnostics as D
    line = D.summary_line("w", [4.0, float("nan"), 1.0, 3.0, 2.0], [1.0, 1.0, 1.2, float("inf"), 1.05])
    assert line == {"site": "w", "size": 5, "n_eff_min": 1.0, "n_eff_median": 2.5, "r_hat_max": float("inf"), "r_hat_above_1_1": 0.4}
    line = D.summary_line("b", [float("nan")], [1.0])
    assert np.isnan(line["n_eff_min"]) and np.isnan(line["n_eff_median"]) and line["r_hat_max"] == 1.0 and line["r_hat_above_1_1"] == 0.0
    assert D.SUMMARY_COLUMNS == ["site", "size", "n_eff_min", "n_eff_median", "r_hat_max", "r_hat_above_1_1"]
    assert D.ChainDiagnostics._fields == ("mean", "std", "r_hat", "split_r_hat", "tau", "n_eff", "n_pairs")


def test_the_new_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    if not os.path.exists(KR.READELF):
        pytest.skip("llvm-readelf not in this image")
    res = KR.kernel_resources()
    new = {n: r for n, r in res.items() if re.search(r"::chain_diag_\w+_kernel", n)}
    # three tile widths, each with 16-byte and with scalar loads; the LDS is dynamic, the query's figure (held to 160 KiB above)
    assert sorted(re.search(r"chain_diag_(\w+)_kernel<(\d+), (\w+)>", n).groups() for n in new) == sorted(
        ("columns", str(T), v) for T in (16, 32, 64) for v in ("false", "true")), sorted(new)
    for n, r in new.items():
        assert r["scratch"] == 0 and r["spill_vgpr"] == 0 and r["lds"] <= LDS, (n, r)
    assert not [n for n in new if re.search("f64|fp64|wpca|cwg_|lockstep|svi_multi", n)]


@pytest.mark.parametrize("K,n", [(1, 4), (2, 9), (4, 64), (3, 33), (8, 250)])
def test_the_restatement_is_hmc_split_r_hat(K, n):
    """Definition 5 against the function it restates, on random [K, n] far from and near the origin, to 1e-12 relative; and its conventions
    for constant sequences."""
    from robustbnns_amd import hmc
    rng = np.random.default_rng(100 * K + n)
    for offset in (0.0, 50.0):
        v = offset + rng.standard_normal((K, n)) + 0.5 * rng.standard_normal((K, 1))
        ours = float(R.r_hat_of(R.split_halves(v[:, :, None].astype(R.LD)))[0])
        theirs = hmc.split_r_hat(v)
        assert abs(ours - theirs) <= 1e-12 * theirs, (ours, theirs)
    const = np.full((K, n, 1), 3.0)
    assert float(R.r_hat_of(R.split_halves(const))[0]) == hmc.split_r_hat(const[:, :, 0]) == 1.0
    steps = const + np.arange(K)[:, None, None] + (np.arange(n) >= n // 2)[None, :, None]            # constant halves at different levels
    assert float(R.r_hat_of(R.split_halves(steps))[0]) == hmc.split_r_hat(steps[:, :, 0]) == float("inf")


def test_the_restatement_agrees_with_its_exact_form_on_integer_draws():
    rng = np.random.default_rng(5)
    x = rng.integers(-8, 9, (2, 16, 6)).astype(np.float32)
    r = R.Restated(x)
    for e in range(6):
        n_pairs, tau = R.exact_tau(x[:, :, e].tolist())
        assert n_pairs == r.n_pairs[e] and abs(float(tau) - r.tau[e]) <= 64 * 16 * R.U
