"""CPU tests (-m "not gpu") of the SVI guides in lockstep: the grouping and de-duplication of grid_search_halfMoons.lockstep_train, each
member's host RNG sequence (init and key as BNN.train's), the schedule against the moons loader, the additive C ABI (header, SIGNATURES,
host-side argument checks), the kernels' resources, and the marginal points of the GPU accuracy cases along their fp64 trajectories."""
import ctypes as C
import os
import random
import re
import sys

import pytest
import torch

import svi_lockstep_cases as Cs
import svi_restate as R
from robustbnns_amd import _hip, model_bnn, svi_train
from robustbnns_amd import grid_search_halfMoons as G

pytestmark = pytest.mark.usefixtures("built_library")

NAMES = {"rbnn_svi_multi_draw", "rbnn_svi_multi_gradient", "rbnn_svi_multi_adam_step", "rbnn_svi_multi_accuracy", "rbnn_svi_multi_finalize"}


def test_lockstep_train_groups_the_svi_models_by_net_shape(monkeypatch):
    calls = []

    def fake(nets, x_train, y_train, n_inputs, device, rel_path=None, batch_size=64):
        calls.append(([(n.basenet.hidden_size, n.basenet.activation, n.basenet.architecture, n.epochs, n.lr, n.name) for n in nets], list(n_inputs),
                      batch_size, rel_path))
    monkeypatch.setattr(model_bnn, "train_svi_lockstep", fake)
    x, y = R.two_moons(32, 0.1, 0)
    grid = ([16, 32], ["leaky"], ["fc", "fc2"], ["svi"], [2, 3], [0.01, 0.05], [None], [None], [16, 32], [1, 5, 10])
    out = G.lockstep_train(*grid, "out/", x_train=x, y_train=y, device="cuda:0")
    assert len(calls) == 4 and len(out) == 32                              # (hidden, architecture) groups of 2 x 2 x 2 models: posterior_samples folded
    seen = set()
    for members, n_inputs, batch, rel in calls:
        assert len(members) == 8 and len({m[:3] for m in members}) == 1 and batch == 64 and rel == "out/"
        assert [(m[3], m[4]) for m in members] == [(e, l) for e in (2, 3) for l in (0.01, 0.05) for _ in (16, 32)]      # the grid's order
        assert n_inputs == [16, 32] * 4
        names = [m[5] for m in members]
        assert len(set(names)) == 8 and not (set(names) & seen)
        seen |= set(names)
    assert seen == set(out) and all(v is not None for v in out.values())
    serial_names = [G.MoonsBNN(*c[:9], (1, 2, 1), 2).name for c in G._combinations(*grid)]
    assert list(out) == list(dict.fromkeys(serial_names))                  # serial_train's names, in its order
    # a ready loader, and the refusals
    routed = []
    monkeypatch.setattr(G, "_train", lambda *a, **kw: routed.append(a[3]) or G.MoonsBNN(*a[:9], (1, 2, 1), 2))
    calls.clear()
    G.lockstep_train([16], ["leaky"], ["fc"], ["svi"], [1], [0.01], [None], [None], [16], [1], "out/", train_loader=G.moons_loader(x, y, 64), device="cuda:0")
    assert routed == ["svi"] and not calls
    with pytest.raises(NotImplementedError, match="no CPU compute path"):
        G.lockstep_train([16], ["leaky"], ["fc"], ["svi"], [1], [0.01], [None], [None], [16], [1], "out/", x_train=x, y_train=y, device="cpu")
    with pytest.raises(NotImplementedError, match="conv"):
        G.lockstep_train([16], ["leaky"], ["conv"], ["svi"], [1], [0.01], [None], [None], [16], [1], "out/", x_train=x, y_train=y, device="cuda:0")
    assert not os.path.exists("out")


def test_every_member_takes_its_init_and_key_as_bnn_train_does(monkeypatch, tmp_path):
    x, y = R.two_moons(200, 0.1, 1)
    seen = {}

    class Fake:
        schedule = staticmethod(svi_train.LockstepSvi.schedule)

        def __init__(self, arch, activation, input_shape, n_classes, locs, raws, lrs, device, keys, batch_size):
            seen.update(locs=locs, raws=raws, lrs=lrs, keys=keys, batch=batch_size)

        def set_data(self, x, labels):
            seen["labels"] = labels

        def run(self, schedule):
            seen["schedule"] = schedule

        def epoch_totals(self):
            return [[(10.0 * (k + 1) + e, 7.0) for e in range(3)] for k in range(3)]

        def params(self, k):
            return seen["locs"][k], seen["raws"][k]
    monkeypatch.setattr(svi_train, "LockstepSvi", Fake)
    monkeypatch.setattr(model_bnn.BNN, "set_variational_params", lambda self, loc, raw, device: setattr(self, "svi_loc", loc) or setattr(self, "svi_scale", raw))
    nets = [G.MoonsBNN(32, "leaky", "fc2", "svi", ep, lr, None, None, n, (1, 2, 1), 2) for ep, lr, n in ((2, 0.05, 200), (3, 0.01, 100), (1, 0.05, 64))]
    held = {k: torch.full_like(v, 0.25) for k, v in nets[2].basenet.state_dict().items()}
    nets[2].svi_loc, nets[2].svi_scale = held, held                     # a net that holds parameters trains on from them
    model_bnn.train_svi_lockstep(nets, x, y, [200, 100, 64], "cuda:0", str(tmp_path) + "/")
    # what BNN.train draws before its first step: seeds, the loader iterator's base seed, the init, the key
    loader = G.moons_loader(x[:100], y[:100], 64)
    random.seed(0)
    model_bnn.set_rng_seed(0)
    iter(loader)
    loc, raw = svi_train.initial_params([(k, tuple(v.shape)) for k, v in nets[0].basenet.state_dict().items()])
    key = svi_train.draw_key()
    for k in (0, 1):
        assert seen["keys"][k] == key
        for name in loc:
            assert torch.equal(seen["locs"][k][name], loc[name]) and torch.equal(seen["raws"][k][name], raw[name]), (k, name)
    random.seed(0)
    model_bnn.set_rng_seed(0)
    iter(loader)
    assert seen["keys"][2] == svi_train.draw_key() and seen["locs"][2] is held          # no init drawn: the key comes first
    assert seen["lrs"] == [0.05, 0.01, 0.05] and seen["batch"] == 64
    assert torch.equal(seen["labels"], y.argmax(-1))
    assert nets[1].training_history == {"loss": [20.0, 21.0, 22.0], "accuracy": [7.0, 7.0, 7.0]}
    assert nets[0].training_history["loss"] == [10.0, 11.0] and nets[0].training_history["accuracy"] == [3.5, 3.5]
    for net in nets:
        assert os.path.exists(str(tmp_path / net.name / (net.name + "_weights.pt")))


def test_the_prologue_draws_what_bnn_train_itself_hands_its_trainer(monkeypatch, tmp_path, capsys):
    """BNN.train itself (seeding, its loop over a real moons loader, the trainer made at the first batch) with SviTrainer replaced by a recorder
    and the host->device copies by the identity: the init and the key it hands over are svi_lockstep_prologue's, for a fresh net and for one
    that holds parameters.  This is what pins the prologue's base-seed draw (an iterator over a DataLoader) to the loop it stands in for."""
    x, y = R.two_moons(100, 0.1, 1)
    got = {}

    class Recorder:
        def __init__(self, arch, activation, input_shape, n_classes, loc, raw, lr, device, key, batch_size):
            got.update(loc=loc, raw=raw, key=key, batch=batch_size)

        def step(self, x, labels):
            got["steps"] = got.get("steps", 0) + 1

        def epoch_totals(self):
            return 0.0, 0.0

        def begin_epoch(self):
            pass

        def params(self):
            return got["loc"], got["raw"]
    monkeypatch.setattr(svi_train, "SviTrainer", Recorder)
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **kw: self)
    monkeypatch.setattr(model_bnn.BNN, "set_variational_params", lambda self, loc, raw, device: setattr(self, "svi_loc", loc) or setattr(self, "svi_scale", raw))
    make = lambda: G.MoonsBNN(32, "leaky", "fc2", "svi", 2, 0.05, None, None, 100, (1, 2, 1), 2)
    held = {k: torch.full_like(v, 0.25) for k, v in make().basenet.state_dict().items()}
    for holds in (False, True):
        got.clear()
        trained, fresh = make(), make()
        if holds:
            trained.svi_loc, trained.svi_scale, fresh.svi_loc, fresh.svi_scale = held, held, held, held
        trained.train(train_loader=G.moons_loader(x, y, 64), device="cuda:0", rel_path=str(tmp_path) + "/")
        assert got["steps"] == 4 and got["batch"] == 64
        loc, raw, key = model_bnn.svi_lockstep_prologue(fresh)
        assert key == got["key"], holds
        for name in loc:
            assert torch.equal(loc[name], got["loc"][name]) and torch.equal(raw[name], got["raw"][name]), (holds, name)
        assert (loc is held) == holds
    capsys.readouterr()


def test_the_schedule_is_the_moons_loaders_batches():
    x, y = R.two_moons(300, 0.1, 2)
    ns, epochs = [300, 150, 64, 1], [2, 3, 1, 4]
    s = svi_train.LockstepSvi.schedule(ns, epochs, 64)
    assert s["count"].shape == (10, 4)
    for k, (n, ep) in enumerate(zip(ns, epochs)):
        batches = [int(xb.shape[0]) for _ in range(ep) for xb, _ in G.moons_loader(x[:n], y[:n], 64)]
        assert s["count"][:, k].tolist() == batches + [0] * (10 - len(batches))
        per = len(batches) // ep
        for t, c in enumerate(batches):
            i = t % per
            assert int(s["start"][t, k]) == 64 * i and int(s["last"][t, k]) == 64 * i + c - 1 < n
            assert int(s["slot"][t, k]) == (t // per if i == per - 1 else -1)
        assert s["slot"][len(batches):, k].tolist() == [-1] * (10 - len(batches))


def test_guards_without_a_gpu():
    loc = {k: torch.zeros(s) for k, s in R.shapes_of("fc", 2, 32, 2).items()}
    with pytest.raises(NotImplementedError, match="no CPU compute path"):
        svi_train.LockstepSvi("fc", "leaky", (1, 2, 1), 2, [loc], [loc], [0.01], "cpu", [1])
    with pytest.raises(NotImplementedError, match="conv"):
        svi_train.LockstepSvi("conv", "leaky", (1, 28, 28), 10, [loc], [loc], [0.01], "cuda:0", [1])
    with pytest.raises(ValueError, match="65535"):
        svi_train.LockstepSvi("fc", "leaky", (1, 2, 1), 2, [loc] * 6554, [loc] * 6554, 0.01, "cuda:0", [1] * 6554)
    other = {k: torch.zeros(s) for k, s in R.shapes_of("fc", 2, 64, 2).items()}
    with pytest.raises(ValueError, match="another net shape"):
        svi_train.LockstepSvi("fc", "leaky", (1, 2, 1), 2, [loc, other], [loc, other], [0.01, 0.01], "cuda:0", [1, 2])


def test_entry_points_are_additive_and_validate_without_a_gpu():
    assert NAMES <= set(_hip.SIGNATURES) and _hip.ABI_VERSION == 10
    hdr = open(_hip.HEADER_PATH).read()
    assert "#define RBNN_ABI_VERSION 10" in hdr and "#define RBNN_SVI_MULTI_ACC_SAMPLES 10" in hdr
    assert svi_train.ACC_SAMPLES == _hip.SVI_LOCKSTEP_ACC_SAMPLES == 10
    assert {n for n in re.findall(r"\b(rbnn_\w+)\s*\(", hdr) if "svi_multi" in n} == NAMES
    for struct, cls in (("rbnn_svi_multi", _hip.SviLockstep), ("rbnn_svi_multi_acc", _hip.SviLockstepAcc)):
        fields = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
        assert re.findall(r"\*?\b([a-zA-Z_0-9]+)\s*[,;]", fields) == [f[0] for f in cls._fields_], struct
    lib = _hip.load()
    net = _hip.NnTrainNet()
    net.arch, net.activation, net.in_features, net.hidden, net.n_classes, net.n_members = 1, 1, 2, 32, 2, 3
    n = 2 * 32 + 32 + 32 * 32 + 32 + 2 * 32 + 2
    net.member_stride = n
    g, acc, ws = _hip.SviLockstep(), _hip.SviLockstepAcc(), _hip.NnTrainWs()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)                                                    # non-NULL, never dereferenced: every call below is refused on the host

    def calls(net_p, g_p, counts, lr=p, acc_p=C.byref(acc)):
        return [lib.rbnn_svi_multi_draw(net_p, g_p, counts, 0, None),
                lib.rbnn_svi_multi_gradient(net_p, p, 2, 8, p, p, counts, 4, C.byref(ws), None),
                lib.rbnn_svi_multi_adam_step(net_p, g_p, counts, 0, 1, lr, 0.9, 0.999, 1e-8, None),
                lib.rbnn_svi_multi_accuracy(net_p, g_p, p, 2, 8, p, counts, 4, 0, 0, acc_p, None),
                lib.rbnn_svi_multi_finalize(net_p, g_p, p, None, p, 8, p, counts, 4, None, None, 0, None)]
    assert calls(C.byref(net), C.byref(g), p) == [-1] * 5                   # every pointer of the blocks NULL
    assert calls(None, C.byref(g), p) == [-1] * 5
    assert calls(C.byref(net), C.byref(g), None) == [-1] * 5
    for name, _ in _hip.SviLockstep._fields_[:10]:
        setattr(g, name, p)
    net.P = net.grad = p
    g.part_stride = 1
    assert [r for i, r in enumerate(calls(C.byref(net), None, p)) if i != 1] == [-1] * 4        # (the gradient takes no guide block)
    for members in (0, 6554, 65535):
        net.n_members = members
        assert calls(C.byref(net), C.byref(g), p) == [-2] * 5, members
    net.n_members = 3
    full = _hip.SviLockstepAcc()
    for name, _ in _hip.SviLockstepAcc._fields_:
        setattr(full, name, p)
    shape = [r for i, r in enumerate(calls(C.byref(net), C.byref(g), p, acc_p=C.byref(full))) if i != 1]
    assert shape == [-2] * 4                                                # part_stride 1 < the 2 KL partial sums of this net
    net.member_stride = n - 1
    assert lib.rbnn_svi_multi_draw(C.byref(net), C.byref(g), p, 0, None) == -2
    net.member_stride, g.part_stride = n, 2
    assert lib.rbnn_svi_multi_adam_step(C.byref(net), C.byref(g), p, 0, 0, p, 0.9, 0.999, 1e-8, None) == -2       # step numbers start at 1
    assert lib.rbnn_svi_multi_accuracy(C.byref(net), C.byref(g), p, 2, 8, p, p, 4, 0, 0, C.byref(acc), None) == -1  # its buffers are NULL
    assert lib.rbnn_svi_multi_finalize(C.byref(net), C.byref(g), p, p, None, 8, p, p, 4, None, None, 0, None) == -1 # Psum without labels
    assert lib.rbnn_svi_multi_finalize(C.byref(net), C.byref(g), p, None, p, 8, p, p, 4, p, None, 0, None) == -1    # epoch ends without a log
    one = _hip.SviTrainNet()
    one.arch, one.activation, one.in_features, one.hidden, one.n_classes = 1, 4, 2, 32, 2
    unsupported = lib.rbnn_svi_train_forward(C.byref(one), None, 2, 8, None, None, None)
    assert unsupported == -3
    net.activation = 4
    assert calls(C.byref(net), C.byref(g), p) == [unsupported] * 5
    net.activation, net.arch = 1, 2
    assert calls(C.byref(net), C.byref(g), p) == [unsupported] * 5


def test_the_new_kernels_use_no_scratch():
    """The kernels of csrc/rbnn_svi_lockstep.hip (its own and the guides' templates of rbnn_svi_step.hpp), the member-aware Adam kernel and the skipping GEMM / head kernels hold everything in registers (read from the code objects of
    the built library: no GPU)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources as KR
    if not os.path.exists(KR.READELF):
        pytest.skip("llvm-readelf not in this image")
    res = {n: r for n, r in KR.kernel_resources().items() if re.search(r"::(svils_\w+_kernel|adam_kernel<\(anonymous namespace\)::GuideMajor>|train_(gemm|head)_kernel<true, true>)", n)}
    # the accuracy head, the draw and the finalize in both of their instances (guide-major here, tensor-major for the conv guides), Adam + KL, GEMM, head
    assert len(res) == 1 + 2 + 2 + 1 + 1 + 1, sorted(res)
    bad = {n: (r["scratch"], r["spill_vgpr"]) for n, r in res.items() if r["scratch"] or r["spill_vgpr"]}
    assert not bad, bad


@pytest.mark.parametrize("name", list(Cs.ACC_CASES))
def test_marginal_points_of_the_accuracy_cases_are_within_one_percent(name):
    c, members = Cs.acc_members(name)
    counts = Cs.cpu_marginal_counts(name)
    print(f"[svi-lockstep marginal {name}] per member and epoch, n = {c['n']}: {counts}")
    assert len(counts) == 3 and all(m <= 0.01 * c["n"] for per in counts for m in per)
    assert len({m[0] for m in members}) == 3 and len({m[1] for m in members}) == 3
