"""GPU tests (-m gpu) of conv SVI guides in lockstep (the rbnn_conv_svi_guides_* entry points of csrc/rbnn_conv_train.hip,
robustbnns_amd/conv_svi_train.ConvLockstepSvi, model_bnn.train_conv_svi_lockstep).  The reference is the single guide: guide k of a lockstep
run against a ConvSviTrainer stepped alone on data[rows[k]], as int32 words, 0 differing elements — parameters, moments, drawn weights,
gradients, per-point CE, the accuracy stack, Psum, the counters and the epoch log; then the gradients against fp64 autograd with the
single-guide tests' bars, finished guides, isolation, reproducibility, no device->host sync, canaries, train_conv_svi_lockstep end to end
against BNN.train_conv, and the guards.  Every check prints one line with its worst figure and what it excluded."""
import re

import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

import conv_restate as CR
import conv_svi_restate as V

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("built_library")]
DEV = "cuda:0"
CN, N_DATA = 10, 40
FLAT = ("loc", "raw", "sigma", "m_loc", "v_loc", "m_raw", "v_raw", "W", "grad")
SEEDS, KEYS3, LRS = (11, 12, 13), (0x1111222233334444, 0xFEDCBA9876543210, 0x0BADC0FFEE), (0.01, 0.02, 0.005)
# (Hc, activation, B): one tile; past the 64-row tile with several dK1 / dK2 slices; a ragged 64-channel tile and three dP1 slices; several
# slices of several units with ragged last ones in all three GEMMs
CASES = [(16, "leaky", 5), (16, "tanh", 65), (48, "leaky", 65), (144, "tanh", 129)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32).cpu() if t.dtype == torch.float32 else t.cpu().clone()


def _data(seed=3, n=N_DATA):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 1, 28, 28, generator=g), torch.randint(0, CN, (n,), generator=g)


def _rows(B, steps, seed=5, K=3):
    """Per step int32 [K, B] out of order from the N_DATA resident points, one index twice inside guide 0, one row shared by guides 1 and 2."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(steps):
        r = torch.stack([torch.randperm(N_DATA, generator=g)[torch.arange(B) % N_DATA] for _ in range(K)]).to(torch.int32)
        r[0, B - 1] = r[0, 0]
        r[2, B // 2] = r[1, 0]
        out.append(r.contiguous())
    return out


def _lockstep(Hc, act, B, guides, keys=KEYS3, lrs=LRS):
    from robustbnns_amd.conv_svi_train import ConvLockstepSvi
    tr = ConvLockstepSvi(act, (1, 28, 28), CN, [g[0] for g in guides], [g[1] for g in guides], list(lrs), DEV, list(keys), batch_size=B)
    tr.set_data(*_data())
    return tr


def _single(Hc, act, B, guide, key, lr):
    from robustbnns_amd.conv_svi_train import ConvSviTrainer
    return ConvSviTrainer(act, (1, 28, 28), CN, guide[0], guide[1], lr, DEV, key, batch_size=B)


def _guide_state(tr, k, B):
    """Guide k's bit patterns out of a lockstep trainer, named as _single_state names a single trainer's."""
    out = {name: torch.cat([_bits(v).reshape(-1) for v in tr.unflat(getattr(tr, name), k).values()]) for name in FLAT}
    out["ce"] = _bits(tr.ws_t["ce"][k * B:(k + 1) * B])
    out["Psum"] = _bits(tr.Psum[k * B * 16:(k + 1) * B * 16])
    out["kl_part"] = _bits(tr.kl_part[k * tr.n_partials:(k + 1) * tr.n_partials])
    out["stats"] = tr.stats[k].cpu().clone()
    return out


def _single_state(s, B):
    out = {name: _bits(getattr(s, name)) for name in FLAT}
    out["ce"], out["Psum"], out["kl_part"], out["stats"] = _bits(s.ws_t["ce"][:B]), _bits(s.Psum[:B]).reshape(-1), _bits(s.kl_part), s.stats.cpu().clone()
    return out


STACKS = {"model.0.weight": "K1w", "model.0.bias": "K1b", "model.3.weight": "K2w", "model.3.bias": "K2b", "model.7.weight": "Fw", "model.7.bias": "Fb"}


def _stack_differing(tr, k, post):
    """Differing int32 words between guide k's 10 weight sets of the lockstep accuracy stack (rows k * 10 .. k * 10 + 9 of every tensor-major
    block) and the stacks [10, ...] of a single trainer's resident ConvStackedPosterior; acc_sample(k, s) must be a view of the same rows."""
    S, d, off = V.ACC_SAMPLES, 0, 0
    for key, size in zip(tr.keys, tr.blocks):
        mine = tr.acc_W[off + k * S * size:off + (k + 1) * S * size]
        ref = getattr(post, STACKS[key]).reshape(-1)
        assert mine.numel() == ref.numel() and tr.acc_sample(k, S - 1)[key].data_ptr() == mine[(S - 1) * size:].data_ptr(), key
        d += int((mine.view(torch.int32) != ref.view(torch.int32)).sum())
        off += tr.K * S * size
    return d


def _differing(a, b):
    return {name: int((a[name] != b[name]).sum()) for name in a}


@pytest.mark.parametrize("Hc,act,B", CASES)
def test_guide_k_equals_the_guide_trained_alone_bit_for_bit(Hc, act, B):
    """K = 3 guides with different inits, keys and learning rates, 4 steps with the accuracy forward; after EVERY step guide k's loc, raw,
    sigma, both moment pairs, W, grad, per-point CE, Psum, KL partials and stats row equal, as int32 words, those of a ConvSviTrainer stepped
    alone on data[rows[k]] (bar: 0 differing elements), and so do the K * 10 weight sets of the accuracy stack (ConvSviTrainer.acc_post's)."""
    if (Hc, B) == (144, 129):
        assert CR.slice_plan(129, 144) == {"dP1": (2, 5), "dK2": (9, 15), "dK1": (2, 65)}
    steps = 4
    guides = [V.guide(Hc, CN, s) for s in SEEDS]
    tr = _lockstep(Hc, act, B, guides)
    singles = [_single(Hc, act, B, guides[k], KEYS3[k], LRS[k]) for k in range(3)]
    x, lab = (t.to(DEV) for t in _data())
    worst, worst_stack, correct = 0, 0, []
    for rows in _rows(B, steps):
        tr.step(rows.to(DEV), accuracy=True)
        for k, s in enumerate(singles):
            idx = rows[k].long().to(DEV)
            s.step(x[idx], lab[idx])
        torch.cuda.synchronize()
        for k, s in enumerate(singles):
            diff = _differing(_guide_state(tr, k, B), _single_state(s, B))
            worst = max(worst, max(diff.values()))
            assert not any(diff.values()), (k, tr.t, diff)
            d = _stack_differing(tr, k, s.acc_post)
            worst_stack = max(worst_stack, d)
            assert d == 0, (k, tr.t, d)
        correct.append(tr.stats[:, 2].tolist())
    assert all(float(s.stats[1]) > 0 for s in singles) and bool(torch.isfinite(tr.loc).all())
    print(f"[conv-svi lockstep Hc={Hc} {act} B={B}] 3 guides x {steps} steps x {len(FLAT) + 4} buffers against single trainers: worst {worst} differing "
          f"elements (bar 0); launches per step {tr.launches // steps}; excluded: nothing")
    print(f"[conv-svi lockstep accuracy Hc={Hc} {act} B={B}] {3 * V.ACC_SAMPLES} weight sets x {steps} steps against ConvSviTrainer.acc_post: worst "
          f"{worst_stack} differing elements (bar 0); Psum and the correct-prediction counts {correct[-1]} bit-equal (above); excluded: nothing")


def test_gradients_of_guide_1_of_3_match_fp64_autograd():
    """conv_svi_restate.GRAD_CASES[4] as it stands in the middle of three guides: against fp64 autograd of the summed CE at the GPU's OWN W, per
    tensor within 1e-5 max |fp64 gradient|, the per-point CE within 1e-5 relative (tests/test_hip_conv_svi_train.py's bars)."""
    Hc, act, B, Cn = V.GRAD_CASES[4]
    assert Cn == CN
    c = V.grad_case(Hc, act, B, Cn)
    from robustbnns_amd.conv_svi_train import ConvLockstepSvi
    guides = [V.guide(Hc, Cn, 21), (c["loc"], c["raw"]), V.guide(Hc, Cn, 22)]
    tr = ConvLockstepSvi(act, (1, 28, 28), Cn, [g[0] for g in guides], [g[1] for g in guides], 0.01, DEV, [7, V.GRAD_KEY, 9], batch_size=max(1, B // 2))
    tr.set_data(c["x"], c["lab"])
    tr.t = V.GRAD_DRAW
    rows = torch.stack([torch.arange(B).flip(0), torch.arange(B), (torch.arange(B) + 1) % B]).to(torch.int32).contiguous().to(DEV)
    tr.gradients(rows)
    torch.cuda.synchronize()
    W, G = tr.unflat(tr.W, 1), tr.unflat(tr.grad, 1)
    ce64, g64 = V.ce_grads(c["x"], c["lab"], {k: W[k].cpu().double() for k in V.KEYS}, act)
    worst = 0.0
    for k in V.KEYS:
        gmax = float(g64[k].abs().max())
        err = float((G[k].cpu().double() - g64[k]).abs().max())
        assert gmax > 0 and err <= 1e-5 * gmax, k
        worst = max(worst, err / (1e-5 * gmax))
    e_ce = float(((tr.ws_t["ce"][B:2 * B].cpu().double() - ce64).abs() / (1e-5 * ce64)).max())
    print(f"[conv-svi lockstep grad Hc={Hc} {act} B={B} C={Cn}] guide 1 of 3: worst gradient error {worst:.3f} x (1e-5 max|fp64 gradient|); per-point CE "
          f"{e_ce:.3f} x (1e-5 CE); excluded: {c['n_drop']} of {c['n_pool']} pool points")
    assert e_ce <= 1.0


# ------------------------------------------------------------------ finished guides, with canaries behind every buffer
CANARY = {torch.float32: float("nan"), torch.float64: float("nan"), torch.uint8: 255, torch.int32: 0x7FFFFFFF, torch.int64: -1}
PAD = 64


def _padded(t):
    big = torch.full((t.numel() + PAD,), CANARY[t.dtype], dtype=t.dtype, device=t.device)
    big[:t.numel()].copy_(t.reshape(-1))
    return big[:t.numel()].view(t.shape), big[t.numel():]


def _log_rows(tr, k):
    return tr.epoch_log[k].cpu().clone()


def test_finished_guides_are_left_alone_and_every_canary_is_intact():
    """Epochs (1, 3, 2) over 20 points at B = 8 (a ragged last batch of 4), accuracy on.  Each guide's final loc, raw, sigma, moments and epoch
    log equal a ConvSviTrainer run for its own epochs, bit for bit; guide 0's buffers (W, stats and the accuracy stack too) right after its last
    step equal its buffers at the end of the run; canaries behind every buffer of the trainer are intact."""
    from robustbnns_amd import _hip
    from robustbnns_amd.conv_svi_train import ConvLockstepSvi
    Hc, act, B, n, epochs = 16, "leaky", 8, 20, (1, 3, 2)
    guides = [V.guide(Hc, CN, s) for s in SEEDS]
    x, lab = _data(8, n)
    tr = ConvLockstepSvi(act, (1, 28, 28), CN, [g[0] for g in guides], [g[1] for g in guides], list(LRS), DEV, list(KEYS3), batch_size=B)
    tr.set_data(x, lab)
    T = tr.load_schedule(ConvLockstepSvi.schedule(n, epochs, B))
    assert T == 9 and tr.sched_B == [8, 8, 4] * 3
    tails = {}
    for name in FLAT + ("kl_part", "stats", "acc_W", "keys_t", "lr_t", "epoch_log", "X", "labels", "all_active"):
        view, tails[name] = _padded(getattr(tr, name))
        setattr(tr, name, view)
    for k in list(tr.ws_t):
        tr.ws_t[k], tails["ws_" + k] = (tr.acc_W, tails["acc_W"]) if k == "acc_W" else _padded(tr.ws_t[k])
    for k in list(tr.sched):
        tr.sched[k], tails["sched_" + k] = _padded(tr.sched[k])
    _hip.fill(tr.net, {**vars(tr), "keys": tr.keys_t})
    tr.ws = _hip.fill(_hip.ConvSviLockstepWs, tr.ws_t)
    tr.Psum = tr.ws_t["Psum"]
    kept = ("loc", "raw", "sigma", "m_loc", "v_loc", "m_raw", "v_raw", "W")
    snap = lambda k: {**{name: torch.cat([_bits(v).reshape(-1) for v in tr.unflat(getattr(tr, name), k).values()]) for name in kept},
                      "stats": tr.stats[k].cpu().clone(), "log": _log_rows(tr, k),
                      "stack": torch.cat([_bits(v).reshape(-1) for s in range(V.ACC_SAMPLES) for v in tr.acc_sample(k, s).values()])}
    after_last = {}
    for t in range(T):
        tr.scheduled_step(t)
        for k, e in enumerate(epochs):
            if t == 3 * e - 1:
                torch.cuda.synchronize()
                after_last[k] = snap(k)
    torch.cuda.synchronize()
    assert tr.t == 9 and sorted(after_last) == [0, 1, 2]
    moved = {(k, name): int((after_last[k][name] != v).sum()) for k in (0, 2) for name, v in snap(k).items()}
    assert not any(moved.values()), moved
    totals = tr.epoch_totals()
    xd, ld = x.to(DEV), lab.to(DEV)
    worst = 0
    for k, e in enumerate(epochs):
        s = _single(Hc, act, B, guides[k], KEYS3[k], LRS[k])
        ref = []
        for _ in range(e):
            s.begin_epoch()
            for i in range(0, n, B):
                s.step(xd[i:i + B], ld[i:i + B])
            ref.append(s.epoch_totals())
        assert totals[k][:e] == ref and totals[k][e:] == [(0.0, 0.0)] * (3 - e), (k, totals[k], ref)
        mine = _guide_state(tr, k, 4)
        theirs = _single_state(s, 4)
        diff = {name: int((mine[name] != theirs[name]).sum()) for name in kept[:-1] + ("kl_part",)}
        worst = max(worst, max(diff.values()))
        assert not any(diff.values()), (k, diff)
        assert float(tr.stats[k, 0]) == float(s.stats[0]) and tr.stats[k, 1:].tolist() == [0.0, 0.0]
    for name, tail in tails.items():
        intact = torch.isnan(tail).all() if tail.dtype.is_floating_point else (tail == CANARY[tail.dtype]).all()
        assert bool(intact) and tail.numel() == PAD, f"the run wrote behind {name}"
    print(f"[conv-svi lockstep finished guides] epochs {epochs}, 9 steps of 8, 8, 4 points: final state and epoch logs against single trainers: worst "
          f"{worst} differing elements (bar 0); guides 0 and 2 unmoved after their last steps in {len(after_last[0])} buffers; {len(tails)} canaries intact; "
          f"excluded: nothing")


def _three_steps(guides, keys, rows_seed, swap_rows_of=None):
    Hc, act, B = CASES[0]
    tr = _lockstep(Hc, act, B, guides, keys)
    rows = _rows(B, 3, rows_seed)
    if swap_rows_of is not None:
        for r, other in zip(rows, _rows(B, 3, rows_seed + 100)):
            r[swap_rows_of] = other[swap_rows_of]
    for r in rows:
        tr.step(r.to(DEV))
    torch.cuda.synchronize()
    per_guide = [_guide_state(tr, k, B) for k in range(3)]
    everything = {name: _bits(getattr(tr, name)) for name in FLAT + ("kl_part", "stats", "acc_W")}
    everything.update({"ws_" + k: _bits(v) for k, v in tr.ws_t.items()})
    return per_guide, everything


def test_guides_0_and_1_do_not_move_when_guide_2_changes():
    guides = [V.guide(16, CN, s) for s in SEEDS]
    a, _ = _three_steps(guides, KEYS3, 5)
    b, _ = _three_steps(guides[:2] + [V.guide(16, CN, 99)], KEYS3[:2] + (0x77,), 5, swap_rows_of=2)
    worst = 0
    for k in (0, 1):
        diff = _differing(a[k], b[k])
        worst = max(worst, max(diff.values()))
        assert not any(diff.values()), (k, diff)
    assert any(_differing(a[2], b[2]).values())
    print(f"[conv-svi lockstep isolation] guide 2's parameters, key and rows changed: guides 0 and 1 differ in {worst} elements of {len(a[0])} buffers "
          f"(bar 0), guide 2 differs; excluded: nothing")


def test_two_identical_runs_are_bit_identical():
    guides = [V.guide(16, CN, s) for s in SEEDS]
    (_, a), (_, b) = _three_steps(guides, KEYS3, 5), _three_steps(guides, KEYS3, 5)
    for name in a:
        assert torch.equal(a[name], b[name]), f"two identical runs differ in {name}"
    print(f"[conv-svi lockstep repeat Hc={CASES[0][0]} {CASES[0][1]} B={CASES[0][2]}] {len(a)} buffers bit-identical between two runs of 3 steps; excluded: nothing")


def test_run_makes_no_device_to_host_sync():
    from robustbnns_amd.conv_svi_train import ConvLockstepSvi
    Hc, act, B = CASES[0]
    tr = _lockstep(Hc, act, B, [V.guide(Hc, CN, s) for s in SEEDS])
    sch = ConvLockstepSvi.schedule(12, (1, 3, 2), B)
    tr.run(sch)                                                                # the first launches of every kernel
    torch.cuda.synchronize()
    T = tr.load_schedule(sch)
    before = tr.launches
    torch.cuda.set_sync_debug_mode("error")
    try:
        for t in range(T):
            tr.scheduled_step(t)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    totals = tr.epoch_totals()
    assert tr.launches - before == T * 22 and [len([r for r in g if r != (0.0, 0.0)]) for g in totals] == [1, 3, 2]
    assert all(r[0] == r[0] and 0 <= r[1] <= 12 for g in totals for r in g)
    print(f"[conv-svi lockstep no sync] {T} scheduled steps of 20 + 2 launches each between the schedule's upload and epoch_totals() with "
          f"torch's sync debug mode on 'error'; excluded: nothing")


# ------------------------------------------------------------------ train_conv_svi_lockstep against BNN.train_conv
def _epoch_lines(out):
    return re.findall(r"\[Epoch \d+\]\t loss: \S+ \t accuracy: \S+", out)


def test_train_conv_svi_lockstep_end_to_end(tmp_path, capsys):
    """Three BNN("conv", "svi") nets of Hc = 16 — (lr 0.01, 2 epochs), (lr 0.02, 1 epoch), one holding preset svi_loc / svi_scale — whole and
    with group=2, each against the same net trained by BNN.train_conv on an unshuffled DataLoader of the same data and batch size: the saved
    parameter files hold equal tensors, training_history is equal exactly, the epoch lines are the same text."""
    from robustbnns_amd.model_bnn import BNN, read_param_store, train_conv_svi_lockstep
    n, B = 19, 8
    x, lab = _data(41, n)
    y = torch.eye(CN)[lab]
    preset = V.guide(16, CN, 42)

    def nets():
        out = [BNN("mnist", 16, "leaky", "conv", "svi", e, lr, None, None, (1, 28, 28), CN) for e, lr in ((2, 0.01), (1, 0.02), (2, 0.005))]
        out[2].set_variational_params(preset[0], preset[1], DEV)
        return out

    ref, ref_dir = nets(), str(tmp_path / "single") + "/"
    capsys.readouterr()
    for net in ref:
        net.train_conv(DataLoader(TensorDataset(x, y), batch_size=B, shuffle=False), DEV, ref_dir)
    ref_lines = _epoch_lines(capsys.readouterr().out)
    assert len(ref_lines) == 5
    for tag, group in (("whole", None), ("group2", 2)):
        mine, rel = nets(), str(tmp_path / tag) + "/"
        train_conv_svi_lockstep(mine, x, y, DEV, rel_path=rel, batch_size=B, group=group)
        lines = _epoch_lines(capsys.readouterr().out)
        assert lines == ref_lines, (tag, lines, ref_lines)
        for a, b in zip(mine, ref):
            assert a.training_history == b.training_history and len(a.training_history["loss"]) == a.epochs, (tag, a.name)
            pa, pb = (read_param_store(d + a.name + "/" + a.name + "_weights.pt") for d in (rel, ref_dir))
            assert sorted(pa) == sorted(pb) and len(pa) == 12
            for key in pa:
                assert torch.equal(pa[key], pb[key]), (tag, a.name, key)
            assert not torch.equal(a.svi_loc["model.7.weight"].cpu(), preset[0]["model.7.weight"])
    print(f"[conv-svi lockstep end to end] 3 nets whole and in groups of 2 against BNN.train_conv: 12 saved tensors per net equal, training_history "
          f"equal, {len(ref_lines)} epoch lines the same text; excluded: nothing")


def test_guards_refuse_before_anything_is_launched():
    from robustbnns_amd.conv_svi_train import ConvLockstepSvi
    Hc, act, B = CASES[0]
    guides = [V.guide(Hc, CN, s) for s in SEEDS]
    args = lambda gs: (act, (1, 28, 28), CN, [g[0] for g in gs], [g[1] for g in gs], 0.01, DEV, list(range(len(gs))))
    tr = ConvLockstepSvi(*args(guides), batch_size=B)
    good = torch.zeros(3, B, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="set_data"):
        tr.step(good)
    tr.set_data(*_data())
    for bad in (torch.zeros(2, B, dtype=torch.int32, device=DEV), torch.zeros(3 * B, dtype=torch.int32, device=DEV),
                torch.zeros(3, B, dtype=torch.int64, device=DEV), torch.zeros(3, B, dtype=torch.int32), torch.zeros(3, 0, dtype=torch.int32, device=DEV),
                torch.zeros(B, 3, dtype=torch.int32, device=DEV).T, [[0] * B] * 3):
        with pytest.raises(ValueError, match="rows must be"):
            tr.step(bad)
    with pytest.raises(ValueError, match="active must be"):
        tr.step(good, active=torch.ones(2, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="epoch_slot"):
        tr.step(good, epoch_slot=torch.zeros(3, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="another net shape"):
        ConvLockstepSvi(*args(guides[:2] + [V.guide(32, CN, 1)]), batch_size=B)
    with pytest.raises(NotImplementedError, match="1x28x28"):
        ConvLockstepSvi(act, (3, 32, 32), *args(guides)[2:], batch_size=B)
    torch.cuda.synchronize()
    assert tr.launches == 0 and tr.t == 0 and float(tr.W.abs().max()) == 0.0 and float(tr.stats.abs().max()) == 0.0
    tr.step(good)
    torch.cuda.synchronize()
    assert tr.launches == 20 and tr.t == 1 and float(tr.W.abs().max()) > 0
    print("[conv-svi lockstep guards] 12 refusals before any launch (W and stats still zero, the launch counter at 0), then one step of 20 launches; "
          "excluded: nothing")
