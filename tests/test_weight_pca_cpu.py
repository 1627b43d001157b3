"""Host side of the weight-space PCA (no GPU): the five C-ABI additions and their argument checks, the workspace formula, the slab plan, what
weight_pca and multimodal refuse before the library is loaded, and the resources of the new kernels read from the built library.
Everything here fails on a tree without the feature: the modules, the include file and the C names do not exist there."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

from robustbnns_amd import _hip

pytestmark = pytest.mark.usefixtures("built_library")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"rbnn_wpca_workspace_query", "rbnn_wpca_normal_rows", "rbnn_wpca_col_mean", "rbnn_wpca_cross_gram", "rbnn_wpca_components"}
VP, I32, I64, U64, SZ = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_size_t


def test_header_declares_the_entry_points_and_the_abi_is_unchanged():
    import __graft_entry__ as G
    hdr = open(_hip.HEADER_PATH).read()
    declared = set(re.findall(r"\b(rbnn_\w+)\s*\(", hdr))
    assert NAMES <= declared and NAMES <= set(_hip.SIGNATURES)
    assert {n for n in declared if n.startswith("rbnn_wpca_")} == NAMES
    # the fences of the other host tests
    assert not [n for n in NAMES if "f64" in n or "fp64" in n or "svi_multi" in n or "lockstep" in n]
    assert "#define RBNN_ABI_VERSION 10" in hdr and _hip.ABI_VERSION == 10 and _hip.load().rbnn_abi_version() == 10
    assert len(G.SOURCES) == 12 and any(d.endswith("rbnn_wpca.inc") for d in G.DEPS)
    units = [s for s in G.SOURCES if '#include "rbnn_wpca.inc"' in open(s).read()]
    assert len(units) == 1                                                        # one translation unit holds it
    assert _hip.WPCA_CHUNK % 16 == 0 and _hip.WPCA_TENSOR == 0x57504341 and _hip.WPCA_MAX_COMPONENTS == 16
    assert _hip.SIGNATURES["rbnn_wpca_workspace_query"] == (I32, [I32, I32, I64, VP, VP])
    assert _hip.SIGNATURES["rbnn_wpca_normal_rows"] == (I32, [U64, I32, I32, I64, I64, VP, I64, VP])
    assert _hip.SIGNATURES["rbnn_wpca_col_mean"] == (I32, [VP, I64, I32, I64, VP, VP])
    assert _hip.SIGNATURES["rbnn_wpca_cross_gram"] == (I32, [VP, I64, I32, VP, I64, I32, VP, I64, VP, I64, VP, SZ, VP])
    assert _hip.SIGNATURES["rbnn_wpca_components"] == (I32, [VP, I32, VP, I64, I32, VP, I64, VP, I64, VP])


@pytest.mark.parametrize("m,n,P", [(1, 1, 1), (50, 50, 669706), (5, 17, 4099), (1000, 1000, 2048), (1000, 150, 2049)])
def test_workspace_query_follows_the_formula(m, n, P):
    """One chunk's partials of every 16 x 16 tile, 256 doubles each; the full size is one of them per chunk."""
    lo, hi = SZ(0), SZ(0)
    assert _hip.load().rbnn_wpca_workspace_query(m, n, P, C.byref(lo), C.byref(hi)) == 0
    tiles = ((m + 15) // 16) * ((n + 15) // 16)
    chunks = (P + _hip.WPCA_CHUNK - 1) // _hip.WPCA_CHUNK
    assert lo.value == tiles * 256 * 8 and hi.value == chunks * lo.value


def test_every_argument_error_returns_its_code_before_any_launch():
    """Fake pointers: a call that got past the checks would fault."""
    lib, p = _hip.load(), 4096
    NULL, SHAPE = _hip.ERR_NULL, _hip.ERR_SHAPE
    lo, hi = SZ(0), SZ(0)
    q = lib.rbnn_wpca_workspace_query
    assert q(4, 4, 8, None, C.byref(hi)) == NULL and q(4, 4, 8, C.byref(lo), None) == NULL
    assert q(0, 4, 8, C.byref(lo), C.byref(hi)) == SHAPE and q(4, 0, 8, C.byref(lo), C.byref(hi)) == SHAPE
    assert q(4, 4, 0, C.byref(lo), C.byref(hi)) == SHAPE
    assert q(2 ** 31 - 1, 2 ** 31 - 1, 8, C.byref(lo), C.byref(hi)) == SHAPE               # more tiles than a grid
    assert q(2 ** 19, 2 ** 19, 2 ** 62, C.byref(lo), C.byref(hi)) == SHAPE                 # the byte count overflows

    def rows(key=1, r0=0, n=4, e0=0, w=8, out=p, ld=8):
        return lib.rbnn_wpca_normal_rows(key, r0, n, e0, w, out, ld, None)
    assert rows(out=None) == NULL
    for bad in (dict(r0=-1), dict(n=0), dict(n=65536), dict(r0=2 ** 31 - 2, n=4), dict(e0=-4), dict(e0=2), dict(e0=5), dict(w=0), dict(ld=7),
                dict(e0=2 ** 34, w=8), dict(w=2 ** 35, ld=2 ** 35), dict(ld=2 ** 62)):
        assert rows(**bad) == SHAPE, bad

    def mean(X=p, ldx=8, n=4, P=8, mu=p):
        return lib.rbnn_wpca_col_mean(X, ldx, n, P, mu, None)
    assert mean(X=None) == NULL and mean(mu=None) == NULL
    for bad in (dict(n=0), dict(P=0), dict(ldx=7), dict(ldx=2 ** 62)):
        assert mean(**bad) == SHAPE, bad

    def gram(Y=p, ldy=8, m=4, X=p, ldx=8, n=4, mu=p, P=8, Cm=p, ldc=4, ws=p, ws_bytes=2048):
        return lib.rbnn_wpca_cross_gram(Y, ldy, m, X, ldx, n, mu, P, Cm, ldc, ws, ws_bytes, None)
    for k in ("Y", "X", "mu", "Cm", "ws"):
        assert gram(**{k: None}) == NULL, k
    for bad in (dict(m=0), dict(n=0), dict(P=0), dict(ldy=7), dict(ldx=7), dict(ldc=3), dict(ws_bytes=2047), dict(ldy=2 ** 62),
                dict(ldx=2 ** 62), dict(ldc=2 ** 62), dict(m=17, ws_bytes=2048), dict(P=2 ** 62, ldy=2 ** 62, ldx=2 ** 62)):
        assert gram(**bad) == SHAPE, bad

    def comps(A=p, k=2, X=p, ldx=8, n=4, mu=p, P=8, V=p, ldv=8):
        return lib.rbnn_wpca_components(A, k, X, ldx, n, mu, P, V, ldv, None)
    for k in ("A", "X", "mu", "V"):
        assert comps(**{k: None}) == NULL, k
    for bad in (dict(k=0), dict(k=17), dict(n=0), dict(P=0), dict(ldx=7), dict(ldv=7), dict(ldx=2 ** 62), dict(ldv=2 ** 62)):
        assert comps(**bad) == SHAPE, bad


def test_slab_plan_is_whole_chunks_within_the_budget():
    from robustbnns_amd import weight_pca as W
    CH = W.CHUNK
    assert CH == _hip.WPCA_CHUNK and CH % 4 == 0
    for P, budget, m, n, gen in [(669706, W.DEFAULT_WS_BYTES, 1000, 1000, 1000), (669706, W.DEFAULT_WS_BYTES, 50, 50, 0),
                                 (4099, 1, 40, 40, 40), (3 * CH + 5, 3 * W.chunk_bytes(4, 0) - 1, 17, 17, 0), (CH, 1 << 40, 3, 3, 3),
                                 (7, 1 << 20, 5, 17, 0), (5 * CH, 2 * W.chunk_bytes(W.tiles(5, 17), 5), 5, 17, 5)]:
        t = W.tiles(m, n)
        plan = W.slab_plan(P, budget, t, gen)
        per = W.chunk_bytes(t, gen)
        assert per == t * 2048 + gen * CH * 4
        # the slabs tile [0, P) in order; every border is a chunk border (a multiple of 4 with it); only the last slab is ragged
        assert plan[0][0] == 0 and sum(w for _, w in plan) == P
        assert all(a + w == b for (a, w), (b, _) in zip(plan, plan[1:]))
        assert all(e0 % CH == 0 and e0 % 4 == 0 for e0, _ in plan) and all(w % CH == 0 for _, w in plan[:-1])
        assert len({w for _, w in plan[:-1]}) <= 1 and 1 <= plan[-1][1] <= plan[0][1]
        # the budget holds every slab, or a slab is the one chunk nothing smaller than exists
        chunks = -(-plan[0][1] // CH)
        assert chunks * per <= budget or chunks == 1
        # and it is used: one more chunk per slab would not fit (unless one slab already covers P)
        assert len(plan) == 1 or (chunks + 1) * per > budget
    assert W.slab_plan(3 * CH + 5, 2 * W.chunk_bytes(4, 0), 4, 0) == [(0, 2 * CH), (2 * CH, CH + 5)]
    assert len(W.slab_plan(3 * CH + 5, 1, 4, 0)) == 4                                      # at least three rounds
    assert W.slab_plan(669706, 1, 0, 0) == [(0, 669706)]                                   # nothing to buffer per column: one slab


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was loaded before the refusal")
    monkeypatch.setattr(_hip, "load", refuse)


def test_refusals_fire_before_the_library_is_loaded(no_library):
    from robustbnns_amd import multimodal, weight_pca as W
    # a device that is not the GPU, in flat_params.require_gpu_fc's wording
    for make in (lambda: W.WeightPCA(2, device="cpu"), lambda: W.PriorRows(1, 5, 8, device="cpu"), lambda: W.MatrixRows(torch.zeros(5, 8))):
        with pytest.raises(NotImplementedError, match=r"runs on the MI355X kernels only \(device .*cpu.*\): there is no CPU compute path"):
            make()
    # dtype, layout
    with pytest.raises(ValueError, match="float32"):
        W.MatrixRows(torch.zeros(5, 8, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"stride\(1\) == 1"):
        W.MatrixRows(torch.zeros(8, 5).t())
    with pytest.raises(ValueError, match="row stride"):
        W.MatrixRows(torch.zeros(1, 8).expand(5, 8))
    with pytest.raises(ValueError, match="2-D"):
        W.MatrixRows(torch.zeros(8))
    # the counts (PriorRows on "cuda" touches no device until it draws)
    pca = W.WeightPCA(2, device="cuda")
    with pytest.raises(ValueError, match="at least 3 rows"):
        pca.fit(W.PriorRows(1, 2, 100))
    with pytest.raises(ValueError, match=r"n_components = 2 exceeds min\(n - 1, P\) = 1"):
        pca.fit(W.PriorRows(1, 5, 1))
    with pytest.raises(ValueError, match=r"n_components = 5 exceeds min\(n - 1, P\) = 4"):
        W.WeightPCA(5, device="cuda").fit(W.PriorRows(1, 5, 100))
    for k in (0, 17):
        with pytest.raises(ValueError, match="1 <= n_components <= 16"):
            W.WeightPCA(k, device="cuda")
    with pytest.raises(ValueError, match="not fitted"):
        pca.transform(W.PriorRows(1, 5, 100))
    with pytest.raises(ValueError, match="not fitted"):
        pca.components()
    # a transform whose P differs from the fit
    pca.rows_ = W.PriorRows(1, 5, 100)
    with pytest.raises(ValueError, match="P = 99 columns, the fit had 100"):
        pca.transform(W.PriorRows(1, 4, 99))

    class Net:
        hmc_history = {"eps": []}
        posterior = None
    with pytest.raises(ValueError, match='no "stack"'):
        multimodal.chains_pca(Net())
    with pytest.raises(ValueError, match="stored posterior samples"):
        multimodal.posterior_weights(Net())
    with pytest.raises(ValueError, match="at least one net"):
        multimodal.build_pca_df({}, 5)


def test_sign_rule_makes_the_largest_entry_of_every_column_positive():
    from robustbnns_amd import weight_pca as W
    u = torch.tensor([[0.1, -0.2], [-0.9, 0.3], [0.4, -0.95]], dtype=torch.float64)
    f = W.flip_signs(u)
    assert torch.equal(f, u * torch.tensor([-1.0, -1.0], dtype=torch.float64))
    assert torch.equal(W.flip_signs(f), f)


def test_the_new_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    if not os.path.exists(KR.READELF):
        pytest.skip("llvm-readelf not in this image")
    res = KR.kernel_resources()
    new = {n: r for n, r in res.items() if re.search(r"::wpca_\w+_kernel", n)}
    kinds = sorted(re.search(r"wpca_(\w+)_kernel", n).group(1) for n in new)
    # the Gram contraction with 16-byte and with scalar loads, one of each of the others
    assert kinds == ["chunk_sum", "col_mean", "components", "cross_gram", "cross_gram", "normal_rows"], sorted(new)
    for n, r in new.items():
        assert r["scratch"] == 0 and r["spill_vgpr"] == 0 and r["lds"] == 0, (n, r)
    assert not [n for n in new if "f64" in n or "fp64" in n]
