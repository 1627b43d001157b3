"""GPU tests (-m gpu) of SVI guides in lockstep (csrc/rbnn_svi_lockstep.hip, svi_train.LockstepSvi, model_bnn.train_svi_lockstep,
grid_search_halfMoons.lockstep_train): a member against an SviTrainer stepped alone on the same batches, bit for bit after every step; the
accuracy forward against fp64; what must not be read; no synchronisation; the public path against serial_train; the guards.

Marginal points (two largest fp64 mean probabilities within MARGIN = 2e-5) of the accuracy cases, measured on the CPU along each member's own
fp64 trajectory (tests/svi_lockstep_cases.py::cpu_marginal_counts, asserted by tests/test_svi_lockstep_cpu.py), per member and epoch:
    moons-fc2-32 (n = 300): [[0, 0], [0, 0], [0, 0]]        mnist-fc-16 (n = 150): [[0, 0], [0, 0], [0, 0]]
"""
import ctypes as C

import pytest
import torch

import svi_lockstep_cases as Cs
import svi_restate as R
from conftest import rel_err_points
from oracle import bnn_oracle as O
from test_hip_svi_train import _bits, _guide, accuracy_bounds

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("built_library")]
DEV = "cuda:0"
B = Cs.BATCH
STATE = ("loc", "raw", "sigma", "m_loc", "v_loc", "m_raw", "v_raw", "W", "grad")
_b64 = lambda t: t.detach().reshape(-1).clone().view(torch.int64).cpu()           # the bit patterns of fp64 values


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"


def _data(shape, Cn, n, seed):
    if shape == (1, 2, 1):
        x, y = R.two_moons(n, 0.1, seed)
    else:
        x, y = O.synthetic_inputs(n, shape, Cn, seed=seed)
    return x, y.argmax(-1)


def _exact_setup(name):
    arch, act, shape, H, Cn, members = Cs.EXACT_CASES[name]
    D = shape[0] * shape[1] * shape[2]
    guides = [_guide(arch, D, H, Cn, seed=100 + k, std=0.5 if D <= 16 else 0.05)[1:] for k in range(len(members))]
    keys = [0xA11CE0000 + 7919 * k for k in range(len(members))]
    x, lab = _data(shape, Cn, max(m[1] for m in members), seed=3)
    return arch, act, shape, H, Cn, members, guides, keys, x, lab


def _lockstep(arch, act, shape, Cn, members, guides, keys, x, lab, which=None):
    from robustbnns_amd.svi_train import LockstepSvi
    which = range(len(members)) if which is None else which
    ls = LockstepSvi(arch, act, shape, Cn, [guides[k][0] for k in which], [guides[k][1] for k in which], [members[k][0] for k in which], DEV,
                     [keys[k] for k in which], batch_size=B)
    ls.set_data(x, lab)
    sched = LockstepSvi.schedule([members[k][1] for k in which], [members[k][2] for k in which], B)
    return ls, sched


@pytest.mark.parametrize("accuracy", [False, True])
@pytest.mark.parametrize("name", list(Cs.EXACT_CASES))
def test_a_member_equals_the_trainer_alone_after_every_step(name, accuracy):
    from robustbnns_amd.svi_train import SviTrainer
    arch, act, shape, H, Cn, members, guides, keys, x, lab = _exact_setup(name)
    K = len(members)
    ls, sched = _lockstep(arch, act, shape, Cn, members, guides, keys, x, lab)
    alone = [SviTrainer(arch, act, shape, Cn, guides[k][0], guides[k][1], members[k][0], DEV, keys[k], batch_size=B) for k in range(K)]
    xd, yd = x.to(DEV), lab.to(DEV)
    T = ls.load_schedule(sched)
    frozen, compared = {}, 0
    for t in range(T):
        ls.scheduled_step(t, accuracy)
        for k in range(K):
            c, s0, slot = int(sched["count"][t, k]), int(sched["start"][t, k]), int(sched["slot"][t, k])
            mine = {nm: _bits(getattr(ls, nm)[k]) for nm in STATE}
            if c == 0:                                     # finished: nothing of it is written any more
                for nm in STATE:
                    assert torch.equal(mine[nm], frozen[k][nm]), (name, t, k, nm)
                assert torch.equal(_b64(ls.stats[k]), frozen[k]["stats"]), (name, t, k)
                continue
            tr = alone[k]
            tr.step(xd[s0:s0 + c], yd[s0:s0 + c], accuracy=accuracy)
            for nm in STATE:
                assert torch.equal(mine[nm], _bits(getattr(tr, nm))), (name, t, k, nm)
            assert torch.equal(_bits(ls.ws_t["ce"].view(K, B)[k, :c]), _bits(tr.ws_t["ce"][:c])), (name, t, k, "ce")
            assert torch.equal(_b64(ls.stats[k, 0]), _b64(tr.stats[0])), (name, t, k, "step loss")
            running = ls.stats[k, 1] if slot < 0 else ls.epoch_log[k, slot, 0]
            assert torch.equal(_b64(running), _b64(tr.stats[1])), (name, t, k, "running loss")
            if slot >= 0:
                assert ls.stats[k, 1:].tolist() == [0.0, 0.0]
                tr.begin_epoch()
            mine["stats"] = _b64(ls.stats[k])
            frozen[k] = mine
            compared += 1
    assert compared == sum(-(-m[1] // B) * m[2] for m in members)
    print(f"[svi-lockstep exact {name} accuracy={accuracy}] K = {K}, {T} lockstep steps, {compared} member-steps: {len(STATE)} buffers, ce, step loss "
          f"and running loss bit-equal to SviTrainer alone; finished members untouched; excluded: nothing")


def _full_run(which):
    arch, act, shape, H, Cn, members, guides, keys, x, lab = _exact_setup("moons-fc2-32-K3")
    members, guides, keys = members + [(0.02, 200, 2)], guides + [guides[0]], keys + [0xFEED]
    ls, sched = _lockstep(arch, act, shape, Cn, members, guides, keys, x, lab, which)
    ls.run(sched)
    torch.cuda.synchronize()
    out = []
    for j in range(len(which)):
        res = {nm: _bits(getattr(ls, nm)[j]) for nm in STATE}
        res["stats"], res["log"], res["Psum"] = _b64(ls.stats[j]), _b64(ls.epoch_log[j]), _bits(ls.Psum[j, :, :Cn])
        out.append(res)
    return out


def test_a_member_does_not_depend_on_k_and_two_runs_are_bit_identical():
    four, again = _full_run([0, 1, 2, 3]), _full_run([0, 1, 2, 3])
    for k in range(4):
        one = _full_run([k])[0]
        for nm in one:
            a, b = four[k][nm], one[nm]
            if nm == "log":                               # the K = 1 log has this member's epochs only (2 values per epoch)
                a = a[:b.shape[0]]
            assert torch.equal(a, b), (k, nm)
            assert torch.equal(four[k][nm], again[k][nm]), (k, nm)
    print(f"[svi-lockstep K-independence] members 0..3 of a K = 4 run equal their K = 1 runs in {len(four[0])} results (Psum and the epoch log "
          f"included); two K = 4 runs bit-identical; excluded: nothing")


@pytest.mark.parametrize("name", list(Cs.ACC_CASES))
def test_accuracy_forward_of_every_member_against_fp64(name):
    from robustbnns_amd.svi_train import ACC_KEY, LockstepSvi, SviTrainer
    c, members = Cs.acc_members(name)
    arch, act, n, Cn, K = c["arch"], c["act"], c["n"], c["Cn"], len(members)
    ls = LockstepSvi(arch, act, c["shape"], Cn, [c["loc"]] * K, [c["raw"]] * K, [m[1] for m in members], DEV, [m[0] for m in members], batch_size=B)
    ls.set_data(c["x"], c["lab"])
    sched = LockstepSvi.schedule([n] * K, [c["epochs"]] * K, B)
    T = ls.load_schedule(sched)
    probe = SviTrainer(arch, act, c["shape"], Cn, c["loc"], c["raw"], 0.01, DEV, 1, batch_size=B)      # its acc_post redraws at the members' parameters
    worst, correct_before = 0.0, [0.0] * K
    marginal = [[0] * c["epochs"] for _ in range(K)]
    for t in range(T):
        ls.scheduled_step(t, True)
        for k in range(K):
            cnt, s0, slot = int(sched["count"][t, k]), int(sched["start"][t, k]), int(sched["slot"][t, k])
            x, lab = c["x"][s0:s0 + cnt], c["lab"][s0:s0 + cnt]
            loc1, raw1 = ({kk: v.cpu().double() for kk, v in d.items()} for d in ls.params(k))
            psum64, pred, gap = R.accuracy_forward(loc1, raw1, arch, act, x, members[k][0], t)
            e = float(rel_err_points(ls.Psum[k, :cnt, :Cn].cpu().double(), psum64).max())
            assert e <= 1e-5, (name, t, k, e)
            worst = max(worst, e)
            c_safe, n_marg = accuracy_bounds(psum64, pred, gap, lab)
            total = float(ls.stats[k, 2]) if slot < 0 else float(ls.epoch_log[k, slot, 1])
            got = total - correct_before[k]
            assert c_safe <= got <= c_safe + n_marg and got == int(got), (name, t, k, got, c_safe, n_marg)
            correct_before[k] = 0.0 if slot >= 0 else total
            marginal[k][t // (-(-n // B))] += n_marg
            # the drawn weight sets: the trainer's own accuracy stack at the same parameters, key and draw id
            probe.loc.copy_(ls.loc[k]); probe.sigma.copy_(ls.sigma[k])
            probe.acc_post.redraw(members[k][0] ^ ACC_KEY, t)
            mine = ls.unflat(ls.acc_t["W"].view(K, 10, -1)[k])
            H, D = probe.H, probe.D
            ref = [probe.acc_post.W1[:, :H, :D], probe.acc_post.b1[:, :H]]
            if arch == "fc2":
                ref += [probe.acc_post.Wm[:, :H, :H], probe.acc_post.bm[:, :H]]
            ref += [probe.acc_post.W2[:, :, :H], probe.acc_post.b2]
            for key_, r in zip(ls.state_keys, ref):
                assert torch.equal(_bits(mine[key_].reshape(r.shape)), _bits(r)), (name, t, k, key_)
    for k in range(K):
        for ep, m in enumerate(marginal[k]):
            assert m <= 0.01 * n, (name, k, ep, m)
    print(f"[svi-lockstep accuracy {name}] K = {K}, {T} steps: Psum worst {worst / 1e-5:.3f} x 1e-5; marginal points per member and epoch "
          f"{marginal} of n = {n}; counts within [c_safe, c_safe + marginal]; the 10 drawn weight sets bit-equal to SviTrainer.acc_post's")


def _poisoned(poison, accuracy):
    from robustbnns_amd.svi_train import LockstepSvi
    arch, act, shape, H, Cn, K = "fc2", "leaky", (1, 17, 1), 32, 3, 3
    counts, starts, n = [37, 5, 0], [10, 50, 0], 80
    guides = [_guide(arch, 17, H, Cn, seed=40 + k, std=0.5)[1:] for k in range(K)]
    x, lab = _data(shape, Cn, n, seed=9)
    ls = LockstepSvi(arch, act, shape, Cn, [g[0] for g in guides], [g[1] for g in guides], [0.01, 0.05, 0.02], DEV, [11, 22, 33], batch_size=B)
    ls.set_data(4 * x - 2, lab)
    rows = torch.zeros(K, B, dtype=torch.int32)
    for k in range(K):
        rows[k] = torch.clamp(starts[k] + torch.arange(B), max=starts[k] + max(counts[k], 1) - 1)
    before = {nm: _bits(getattr(ls, nm)[2]) for nm in STATE}
    if poison:
        nan = float("nan")
        used = torch.zeros(n, dtype=torch.bool)
        for k in range(2):
            used[starts[k]:starts[k] + counts[k]] = True
        ls.X[~used.to(DEV)] = nan
        ls.labels[~used.to(DEV)] = Cn
        for k in range(K):
            for v in list(ls.ws_t.values()) + [ls.Psum]:
                v.view(K, B, -1)[k, counts[k]:] = Cn if v.dtype == torch.int32 else nan
            for nm in ("hid1", "hid2", "dact"):
                ls.acc_t[nm].view(K, 10, B, H)[k, :, counts[k]:] = nan
        ls.acc_t["W"].view(K, 10, -1)[2] = nan
    ls.step(rows.to(DEV), torch.tensor(counts, dtype=torch.int32).to(DEV), accuracy=accuracy)
    torch.cuda.synchronize()
    res = {}
    for k in range(2):
        for nm in STATE:
            res[f"{nm}[{k}]"] = _bits(getattr(ls, nm)[k])
        res[f"ce[{k}]"] = _bits(ls.ws_t["ce"].view(K, B)[k, :counts[k]])
        res[f"dZ[{k}]"] = _bits(ls.ws_t["dZ"].view(K, B, -1)[k, :counts[k], :Cn])
        res[f"stats[{k}]"] = _b64(ls.stats[k])
        assert bool(torch.isfinite(ls.stats[k]).all())
        if accuracy:
            res[f"Psum[{k}]"] = _bits(ls.Psum[k, :counts[k], :Cn])
    for nm, v in res.items():
        if not nm.startswith("stats"):
            assert bool(torch.isfinite(v.view(torch.float32)).all()), f"{nm} is not finite ({'poisoned' if poison else 'clean'} run)"
    for nm in STATE:                                       # the finished member: not one bit of its state is written
        assert torch.equal(_bits(getattr(ls, nm)[2]), before[nm]), nm
    assert ls.stats[2].tolist() == [0.0, 0.0, 0.0]
    return res


@pytest.mark.parametrize("accuracy", [False, True])
def test_nothing_behind_the_bounds_is_read(accuracy):
    clean, dirty = _poisoned(False, accuracy), _poisoned(True, accuracy)
    for nm in clean:
        assert torch.equal(clean[nm], dirty[nm]), f"{nm} depends on memory behind the bounds"
    print(f"[svi-lockstep bounds accuracy={accuracy}] K = 3, counts 37 / 5 / 0 of {B}: {len(clean)} results bit-identical and finite with NaN in the "
          f"workspace rows behind every count, in the data rows no member indexes, in the finished member's workspaces, Psum and weight sets, and "
          f"labels = C on unused rows; the finished member's state untouched; excluded: nothing")


def test_fifty_lockstep_steps_make_no_device_to_host_sync():
    from robustbnns_amd.svi_train import LockstepSvi
    arch, act, shape, H, Cn = "fc2", "leaky", (1, 2, 1), 32, 2
    ns, epochs = [17 * 64, 200, 64], [3, 12, 51]            # 51 steps; member 1 ends 12 epochs and finishes at step 48, member 2 ends one every step
    guides = [_guide(arch, 2, H, Cn, seed=60 + k, std=0.5)[1:] for k in range(3)]
    x, lab = _data(shape, Cn, max(ns), seed=2)
    ls = LockstepSvi(arch, act, shape, Cn, [g[0] for g in guides], [g[1] for g in guides], [0.01, 0.02, 0.05], DEV, [1, 2, 3], batch_size=B)
    ls.set_data(x, lab)
    T = ls.load_schedule(LockstepSvi.schedule(ns, epochs, B))
    assert T == 51
    ls.scheduled_step(0)
    torch.cuda.synchronize()
    launches = ls.launches
    torch.cuda.set_sync_debug_mode("error")
    try:
        for t in range(1, T):
            ls.scheduled_step(t)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    totals = ls.epoch_totals()
    assert (ls.launches - launches) == 50 * 14 and ls.t == 51          # fc2 with accuracy: 8 + 4 + the 2 torch launches, whatever K
    for k in range(3):
        for e in range(epochs[k]):
            loss, correct = totals[k][e]
            assert loss == loss and loss > 0 and 0 <= correct <= ns[k] and correct == int(correct), (k, e, loss, correct)


def test_lockstep_train_saves_what_serial_train_saves(tmp_path, capsys, monkeypatch):
    from robustbnns_amd import grid_search_halfMoons as G
    from robustbnns_amd import svi_train
    x, y = R.two_moons(300, 0.1, seed=4)
    grid = ([32], ["leaky"], ["fc2"], ["svi"], [2, 3], [0.01, 0.05], [None], [None], [100, 300], [5])
    made = []
    init = svi_train.LockstepSvi.__init__

    def spy(self, *a, **kw):
        made.append(len(a[4]))
        return init(self, *a, **kw)
    monkeypatch.setattr(svi_train.LockstepSvi, "__init__", spy)
    rel_s, rel_l = str(tmp_path / "serial") + "/", str(tmp_path / "lockstep") + "/"
    serial = G.serial_train(*grid, rel_s, x_train=x, y_train=y, device=DEV)
    lock = G.lockstep_train(*grid, rel_l, x_train=x, y_train=y, device=DEV)
    out = capsys.readouterr().out
    assert made == [8], made                                           # one sampler for the eight models
    assert list(serial) == list(lock) and len(lock) == 8
    worst = 0
    for name, a in serial.items():
        b = lock[name]
        pa = torch.load(rel_s + name + "/" + name + "_weights.pt", weights_only=False)["params"]
        pb = torch.load(rel_l + name + "/" + name + "_weights.pt", weights_only=False)["params"]
        assert pa.keys() == pb.keys() and len(pa) == 12
        for k in pa:
            assert torch.equal(pa[k], pb[k]), (name, k)
        for k in a.svi_loc:
            assert torch.equal(a.svi_loc[k], b.svi_loc[k]) and torch.equal(a.svi_scale[k], b.svi_scale[k]), (name, k)
        assert a.training_history["loss"] == b.training_history["loss"], name
        n = int([m for m in (100, 300) if G.MoonsBNN(32, "leaky", "fc2", "svi", a.epochs, a.lr, None, None, m, (1, 2, 1), 2).name == name][0])
        for e, (u, v) in enumerate(zip(a.training_history["accuracy"], b.training_history["accuracy"])):
            d = round((v - u) * n / 100)
            print(f"   {name} epoch {e + 1}: correct serial {round(u * n / 100)}  lockstep {round(v * n / 100)}  delta {d:+d}")
            assert abs(d) <= 0.01 * n, (name, e, u, v)
            worst = max(worst, abs(d))
            assert f"[Epoch {e + 1}]\t loss: {b.training_history['loss'][e] / n:.2f} \t accuracy: {v:.2f}" in out
    print(f"[svi-lockstep public path] 8 models: names, 12 saved tensors each and the epoch losses equal serial_train's; worst |delta correct| {worst}; "
          f"one LockstepSvi of 8 members")
    # a ready train_loader still goes through _train, one model at a time
    calls = []
    keep = G._train
    monkeypatch.setattr(G, "_train", lambda *a, **kw: calls.append(a[:9]) or keep(*a, **kw))
    made.clear()
    loader = G.moons_loader(x[:64], y[:64], 64)
    one = ([32], ["leaky"], ["fc2"], ["svi"], [1], [0.01], [None], [None], [64], [5])
    res = G.lockstep_train(*one, str(tmp_path / "loader") + "/", train_loader=loader, device=DEV)
    assert len(calls) == 1 and made == [] and len(res) == 1


def test_the_default_device_name_trains_like_cuda_0(tmp_path, capsys):
    """device="cuda", the default of lockstep_train and serial_train, names the current card while the buffers report cuda:0: the trainer
    must take its own rows and counts, and train what it trains under "cuda:0"."""
    from robustbnns_amd import grid_search_halfMoons as G
    from robustbnns_amd.svi_train import LockstepSvi
    x, y = R.two_moons(100, 0.1, seed=4)
    grid = ([32], ["leaky"], ["fc2"], ["svi"], [1, 2], [0.05], [None], [None], [100], [5])
    named = G.lockstep_train(*grid, str(tmp_path / "named") + "/", x_train=x, y_train=y, device=DEV)
    default = G.lockstep_train(*grid, str(tmp_path / "default") + "/", x_train=x, y_train=y)
    capsys.readouterr()
    assert list(named) == list(default) and len(default) == 2
    for name, a in named.items():
        b = default[name]
        for k in a.svi_loc:
            assert torch.equal(a.svi_loc[k], b.svi_loc[k]) and torch.equal(a.svi_scale[k], b.svi_scale[k]), (name, k)
        assert a.training_history == b.training_history, name
    _, loc, raw = _guide("fc", 2, 32, 2, seed=1, std=0.5)
    ls = LockstepSvi("fc", "leaky", (1, 2, 1), 2, [loc], [raw], [0.01], "cuda", [1], batch_size=8)
    ls.set_data(x, y.argmax(-1))
    assert ls.device == ls.W.device == ls.X.device
    ls.step(torch.arange(8, dtype=torch.int32, device="cuda")[None].contiguous(), torch.tensor([8], dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    assert ls.t == 1 and bool(torch.isfinite(ls.stats).all()) and float(ls.stats[0, 0]) > 0


def test_guards_and_c_abi():
    from robustbnns_amd import _hip
    from robustbnns_amd.model_bnn import BNN, train_svi_lockstep
    from robustbnns_amd.svi_train import LockstepSvi
    _, loc, raw = _guide("fc", 2, 32, 2, seed=1, std=0.5)
    _, loc2, raw2 = _guide("fc", 2, 64, 2, seed=1, std=0.5)
    with pytest.raises(NotImplementedError, match="no CPU compute path"):
        LockstepSvi("fc", "leaky", (1, 2, 1), 2, [loc], [raw], [0.01], "cpu", [1])
    with pytest.raises(NotImplementedError, match="conv"):
        LockstepSvi("conv", "leaky", (1, 28, 28), 10, [loc], [raw], [0.01], DEV, [1])
    with pytest.raises(ValueError, match="another net shape"):
        LockstepSvi("fc", "leaky", (1, 2, 1), 2, [loc, loc2], [raw, raw2], [0.01, 0.01], DEV, [1, 2])
    with pytest.raises(ValueError, match="65535"):
        LockstepSvi("fc", "leaky", (1, 2, 1), 2, [loc] * 6554, [raw] * 6554, 0.01, DEV, [1] * 6554)
    _, loc96, raw96 = _guide("fc", 784, 96, 10, seed=1, std=0.05)
    ls = LockstepSvi("fc", "leaky", (1, 28, 28), 10, [loc96], [raw96], [0.01], DEV, [1], batch_size=8)
    x8, y8 = O.synthetic_inputs(8, (1, 28, 28), 10, seed=2)
    ls.set_data(x8, y8.argmax(-1))
    before = (ls.loc.clone(), ls.raw.clone(), ls.stats.clone())
    rows, counts = torch.arange(8, dtype=torch.int32, device=DEV)[None].contiguous(), torch.tensor([8], dtype=torch.int32).to(DEV)
    with pytest.raises(NotImplementedError, match="no accuracy forward"):
        ls.step(rows, counts)
    assert ls.t == 0 and all(torch.equal(a, b) for a, b in zip(before, (ls.loc, ls.raw, ls.stats)))
    ls.step(rows, counts, accuracy=False)                                 # the step without it runs
    x, y = R.two_moons(64, 0.1, 0)
    nets = [BNN("half_moons", 32, "leaky", "fc2", "svi", 1, 0.01, None, None, (1, 2, 1), 2), BNN("half_moons", 64, "leaky", "fc2", "svi", 1, 0.01, None, None, (1, 2, 1), 2)]
    with pytest.raises(ValueError, match="one net shape"):
        train_svi_lockstep(nets, x, y, [64, 64], DEV, "out/")
    with pytest.raises(NotImplementedError, match="no CPU compute path"):
        train_svi_lockstep(nets[:1], x, y, [64], "cpu", "out/")
    conv = BNN("mnist", 32, "leaky", "conv", "svi", 1, 0.01, None, None, (1, 28, 28), 10)
    with pytest.raises(NotImplementedError, match="conv"):
        train_svi_lockstep([conv], x, y, [64], DEV, "out/")
    # the C ABI, with real device buffers
    lib = _hip.load()
    ls = LockstepSvi("fc", "leaky", (1, 2, 1), 2, [loc, loc], [raw, raw], [0.01, 0.02], DEV, [1, 2], batch_size=8)
    ls.set_data(x, y.argmax(-1))
    rows = torch.arange(8, dtype=torch.int32, device=DEV).repeat(2, 1).contiguous()
    counts = torch.tensor([8, 8], dtype=torch.int32).to(DEV)
    net, g, st = C.byref(ls.net), C.byref(ls.guides), _hip.stream_of(ls.W)
    grad = lambda: lib.rbnn_svi_multi_gradient(net, _hip.ptr(ls.X), ls.D, 64, _hip.ptr(ls.labels), _hip.ptr(rows), _hip.ptr(counts), 8, C.byref(ls.ws), st)
    draw = lambda: lib.rbnn_svi_multi_draw(net, g, _hip.ptr(counts), 0, st)
    adam = lambda: lib.rbnn_svi_multi_adam_step(net, g, _hip.ptr(counts), 0, 1, _hip.ptr(ls.lr_t), 0.9, 0.999, 1e-8, st)
    acc = lambda: lib.rbnn_svi_multi_accuracy(net, g, _hip.ptr(ls.X), ls.D, 64, _hip.ptr(rows), _hip.ptr(counts), 8, 0, 0, C.byref(ls.acc), st)
    fin = lambda: lib.rbnn_svi_multi_finalize(net, g, _hip.ptr(ls.ws_t["ce"]), None, _hip.ptr(ls.labels), 64, _hip.ptr(rows), _hip.ptr(counts), 8, None, None, 0, st)
    every = (draw, grad, adam, acc, fin)
    assert [f() for f in every] == [0] * 5
    assert lib.rbnn_svi_multi_draw(net, g, None, 0, st) == -1 and lib.rbnn_svi_multi_draw(None, g, _hip.ptr(counts), 0, st) == -1
    assert lib.rbnn_svi_multi_gradient(net, _hip.ptr(ls.X), ls.D, 64, _hip.ptr(ls.labels), None, _hip.ptr(counts), 8, C.byref(ls.ws), st) == -1
    assert lib.rbnn_svi_multi_adam_step(net, g, _hip.ptr(counts), 0, 1, None, 0.9, 0.999, 1e-8, st) == -1
    assert lib.rbnn_svi_multi_accuracy(net, g, _hip.ptr(ls.X), ls.D, 64, _hip.ptr(rows), _hip.ptr(counts), 8, 0, 0, None, st) == -1
    assert lib.rbnn_svi_multi_finalize(net, g, None, None, None, 64, _hip.ptr(rows), _hip.ptr(counts), 8, None, None, 0, st) == -1
    for members in (0, 6554):
        ls.net.n_members = members
        assert [f() for f in every] == [-2] * 5, members
    ls.net.n_members = 2
    one = _hip.SviTrainNet()
    one.arch, one.activation, one.in_features, one.hidden, one.n_classes = 0, 4, 2, 32, 2
    unsupported = lib.rbnn_svi_train_forward(C.byref(one), None, 2, 8, None, None, None)
    assert unsupported == -3
    ls.net.activation = 4
    assert [f() for f in every] == [unsupported] * 5
    ls.net.activation, ls.net.arch = 1, 2
    assert [f() for f in every] == [unsupported] * 5
    torch.cuda.synchronize()
