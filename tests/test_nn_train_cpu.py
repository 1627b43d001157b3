"""Host tier of deterministic training (robustbnns_amd/nn_train.py, csrc/rbnn_nn_train.hip): the CPU half of Ensemble_NN.train against the
reference's recorded run, the fixtures against a plain torch restatement, the inputs of the GPU tier against their own caps, the guards, the
host-side argument checks of the new entry points and the new kernels' resources.  No HIP compute is called here."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

import nn_restate as NR
from robustbnns_amd import _hip, model_ensemble, model_nn

pytestmark = pytest.mark.usefixtures("built_library")


def _ensemble(meta):
    return model_ensemble.Ensemble_NN(meta["dataset"], meta["hidden"], meta["act"], meta["arch"], meta["epochs"], meta["lr"], tuple(meta["shape"]),
                                      meta["n_classes"], meta["M"])


@pytest.mark.parametrize("name", NR.ENS_CASES)
def test_ensemble_schedule_is_the_references_init_and_batches(name):
    """The members' initial weights bit for bit and every batch index of every member, from the generator state the fixture's run started at."""
    from robustbnns_amd.nn_train import ensemble_schedule
    meta, arr = NR.load(name)
    assert meta["N"] % 100 and meta["M"] == 3 and meta["epochs"] == 2
    torch.manual_seed(meta["seed0"])
    ens = _ensemble(meta)
    members, sched = ensemble_schedule(ens, meta["N"])
    assert len(members) == meta["M"] and tuple(sched.shape) == (meta["M"], meta["epochs"], meta["N"]) and sched.dtype == torch.int64
    for m, net in enumerate(members):
        want = NR.state_of(arr, f"init{m}:", meta["arch"])
        assert list(net.state_dict().keys()) == list(want.keys())
        for k, v in net.state_dict().items():
            assert torch.equal(v, want[k]), (m, k)
    assert torch.equal(sched, arr["rows"].to(torch.int64))
    assert all(sorted(sched[m, e].tolist()) == list(range(meta["N"])) for m in range(meta["M"]) for e in range(meta["epochs"]))


@pytest.mark.parametrize("name", NR.NN_CASES + NR.ENS_CASES)
def test_fixture_holds_together_under_a_plain_torch_restatement(name):
    """Autograd + torch.optim.Adam on the mean CE in fp32, from the recorded init over the recorded batches, lands on the reference's recorded
    parameters (per step where the fixture has steps), and the stored spread is the reference's distance from the same restatement in fp64.
    Bar of the fp32 comparison: two correct fp32 evaluations each sit within one spread of fp64, so they are within 2 spreads of each other."""
    meta, arr = NR.load(name)
    arch = meta["arch"]
    assert meta["torch"] and os.path.getsize(os.path.join(NR.GOLDEN, name + ".npz")) < 100 * 1024
    if meta["kind"] == "nn":
        r32, before = NR.run_nn_case(name, torch.float32)
        r64, _ = NR.run_nn_case(name, torch.float64)
        assert len(before) == meta["steps"] and meta["N"] % meta["batch"]
        final, scale = NR.state_of(arr, "final:", arch), NR.param_scale(r64.params())
        worst = max([NR.max_diff(NR.state_of(arr, f"step{i}:", arch), b) for i, b in enumerate(before)] + [NR.max_diff(final, r32.params())])
        spread = NR.max_diff(final, r64.params()) / scale
        runs = [(r32, r64, 0)]
    else:
        r32s, r64s = NR.run_ens_case(name, torch.float32), NR.run_ens_case(name, torch.float64)
        finals = [NR.state_of(arr, f"final{m}:", arch) for m in range(meta["M"])]
        scale = min(NR.param_scale(r.params()) for r in r64s)
        worst = max(NR.max_diff(f, r.params()) for f, r in zip(finals, r32s))
        spread = max(NR.max_diff(f, r.params()) / NR.param_scale(r.params()) for f, r in zip(finals, r64s))
        runs = [(a, b, m) for m, (a, b) in enumerate(zip(r32s, r64s))]
    print(f"[{name}] fp32 restatement vs the reference: max |diff| {worst:.2e} (bar {2 * meta['spread'] * scale:.2e}); spread {spread:.3e}, stored {meta['spread']:.3e}")
    assert worst <= 2 * meta["spread"] * scale
    assert abs(spread - meta["spread"]) <= 1e-3 * meta["spread"]
    # the epoch lines: loss = sum of the step means / N, accuracy from the training forward's own logits
    per = len(runs[0][0].losses) // meta["epochs"]
    n_marg = 0
    for r32, r64, m in runs:
        n_marg += sum(r64.n_marginal)
        for e in range(meta["epochs"]):
            loss_ref, acc_ref = meta["lines"][m * meta["epochs"] + e]
            assert abs(sum(r32.losses[e * per:(e + 1) * per]) / meta["N"] - loss_ref) <= 1e-8 + 1e-6 * loss_ref
            if sum(r64.n_marginal[e * per:(e + 1) * per]) == 0:
                assert f"{100 * sum(r64.correct[e * per:(e + 1) * per]) / meta['N']:.2f}" == f"{acc_ref:.2f}"
    assert n_marg <= 0.02 * meta["N"] * meta["epochs"] * len(runs)


@pytest.mark.parametrize("arch,act,shape,H,Cn,B,M", NR.GRAD_CASES)
def test_gpu_tier_inputs_stay_inside_their_caps(arch, act, shape, H, Cn, B, M):
    """What the GPU tier leaves out is decided by the fp64 evaluation alone: at most 1 % of the (member, pool point) evaluations within the kink
    margin (tests/test_hip_svi_train.py's cap per evaluated net; a pool point is dropped for every member when one member has it at a kink, and
    dropped points are never scored), at most 2 % of a case's scored points within the argmax margin; both CE branches are met where the
    case can meet them."""
    c = NR.grad_case(arch, act, shape, H, Cn, B, M)
    assert c["n_kink"] <= 0.01 * c["n_pool"] * M, c["n_kink"]
    refs = [NR.member_fp64(c, m, arch, act) for m in range(M)]
    n_marg = sum(r["n_marginal"] for r in refs)
    assert n_marg <= 0.02 * M * B, n_marg
    if Cn > 1 and B >= 65:
        assert all(0 < int(r["log1p"].sum()) < B for r in refs)
    assert tuple(c["rows"].shape) == (M, B) and int(c["rows"].max()) < len(c["lab"]) and int(c["rows"].min()) >= 0


def test_guards_raise_on_cpu_and_conv_with_nothing_launched(monkeypatch):
    from torch.utils.data import DataLoader, TensorDataset
    from robustbnns_amd import nn_train
    launched = []
    monkeypatch.setattr(_hip, "HipKernels", lambda: launched.append(1))
    x, y = torch.rand(8, 1, 28, 28), torch.eye(10)[torch.arange(8)]
    loader = DataLoader(TensorDataset(x, y), batch_size=4)
    net = model_nn.NN("mnist", (1, 28, 28), 10, 16, "leaky", "fc", 0.01, 1)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    conv = model_nn.NN("mnist", (1, 28, 28), 10, 16, "leaky", "conv", 0.01, 1)
    ens = model_ensemble.Ensemble_NN("mnist", 16, "leaky", "fc", 1, 0.01, (1, 28, 28), 10, 2)
    cens = model_ensemble.Ensemble_NN("mnist", 16, "leaky", "conv", 1, 0.01, (1, 28, 28), 10, 2)
    torch.manual_seed(5)
    rng = torch.get_rng_state()                           # a refused call seeds nothing and constructs no member
    with pytest.raises(NotImplementedError, match="no CPU compute path"):
        net.train(loader, "cpu")
    with pytest.raises(NotImplementedError, match="no CPU compute path"):
        net.train(train_loader=loader, device="cpu", seed=3, save=False)
    with pytest.raises(NotImplementedError, match="conv"):
        conv.train(loader, "cuda:0")
    with pytest.raises(NotImplementedError, match="no CPU compute path"):
        ens.train(x, y, "cpu")
    with pytest.raises(NotImplementedError, match="conv"):
        cens.train(x, y, "cuda:0")
    with pytest.raises(NotImplementedError, match="no CPU compute path"):
        nn_train.NnTrainer("fc", "leaky", (1, 28, 28), 10, [net.state_dict()], 0.01, "cpu")
    with pytest.raises(NotImplementedError, match="conv"):
        nn_train.NnTrainer("conv", "leaky", (1, 28, 28), 10, [conv.state_dict()], 0.01, "cuda:0")
    assert not launched and torch.equal(rng, torch.get_rng_state()) and ens.ensemble_models == {} and not hasattr(net, "device")
    assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())
    assert net.train(False) is net and net.training is False and ens.train(mode=True) is ens and ens.training is True


def test_ensemble_save_writes_the_files_load_reads(tmp_path):
    ens = model_ensemble.Ensemble_NN("half_moons", 16, "leaky", "fc2", 1, 0.01, (1, 2, 1), 2, 3)
    for seed in ens.random_seeds:
        ens.ensemble_models[str(seed)] = model_nn.NN("half_moons", (1, 2, 1), 2, 16, "leaky", "fc2", 0.01, 1)
    ens.save()
    member = ens.ensemble_models["0"].name
    files = sorted(os.listdir(os.path.join(model_nn.TESTS, ens.name, "weights")))
    assert files == [f"{member}_weights_{s}.pt" for s in range(3)]
    again = model_ensemble.Ensemble_NN("half_moons", 16, "leaky", "fc2", 1, 0.01, (1, 2, 1), 2, 3)
    again.load("cpu")
    for s in ("0", "1", "2"):
        for k, v in ens.ensemble_models[s].state_dict().items():
            assert torch.equal(v, again.ensemble_models[s].state_dict()[k]), (s, k)
    ens.save(seed=2)                                      # one member (the reference's `if seed:`)


def test_entry_points_validate_their_arguments_on_the_host():
    lib = _hip.load()
    net = _hip.NnTrainNet()
    net.arch, net.activation, net.in_features, net.hidden, net.n_classes, net.n_members = 1, 1, 17, 96, 10, 3
    n = 96 * 17 + 96 + 96 * 96 + 96 + 10 * 96 + 10
    assert lib.rbnn_nn_train_sizes(C.byref(net)) == n
    net.arch = 0
    assert lib.rbnn_nn_train_sizes(C.byref(net)) == 96 * 17 + 96 + 10 * 96 + 10
    assert lib.rbnn_nn_train_sizes(None) < 0
    for field, bad in (("n_classes", 17), ("n_classes", 0), ("hidden", 0), ("in_features", 0), ("n_members", 0), ("n_members", 65536), ("arch", 2),
                       ("activation", 4)):
        keep = getattr(net, field)
        setattr(net, field, bad)
        assert lib.rbnn_nn_train_sizes(C.byref(net)) < 0, (field, bad)
        setattr(net, field, keep)
    ws = _hip.NnTrainWs()
    assert lib.rbnn_nn_train_forward(C.byref(net), None, 17, 8, None, None, 4, C.byref(ws), None) != 0          # NULL pointers: nothing launched
    assert lib.rbnn_nn_weight_grads(C.byref(net), None, 17, 8, None, 4, C.byref(ws), None) != 0
    assert lib.rbnn_nn_adam_step(C.byref(net), 1, 0.01, 0.9, 0.999, 1e-8, None) != 0
    assert lib.rbnn_nn_train_finalize(C.byref(net), C.byref(ws), 4, None, None) != 0


def test_training_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources as KR
    if not os.path.exists(KR.READELF):
        pytest.skip("llvm-readelf not in this image")
    res = {n: r for n, r in KR.kernel_resources().items() if re.search(r"::(train_(gemm|head)_kernel<true, false>|nn_adam_kernel<true>|nn_finalize_kernel<true>)", n)}
    assert len(res) == 4, sorted(res)
    bad = {n: (r["scratch"], r["spill_vgpr"]) for n, r in res.items() if r["scratch"] or r["spill_vgpr"]}
    assert not bad, bad
