"""GPU tests (-m gpu) of deep ensembles of conv nets trained in lockstep (model_ensemble.py:69-83 for the conv architecture; the rbnn_conv_ens_*
entry points of csrc/rbnn_conv_train.hip, robustbnns_amd/conv_train.ConvEnsembleTrainer, Ensemble_NN.train_conv): member k against that net
trained alone by ConvNnTrainer bit for bit, the gradients of a member other than 0 against fp64 autograd, isolation of the members from each
other and from data rows nobody names, two runs against each other, Ensemble_NN.train_conv end to end (whole and in member groups of 2), no
device->host sync inside a step, and the guards.  Every check prints one line with its worst figure.

Mutations these tests are written to catch: a member reading another member's weights or batch (any per-member base offset), rows not clamped
or taken from member 0, slice counts that depend on M (another summation order), dZ scaled by 1 / (M B), stats of the wrong member, a
per-member offset of the partial sums formed from the wrong slice count (visible only where a GEMM has several slices of several units)."""
import os

import pytest
import torch

import conv_restate as CR
import nn_restate as NR

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("built_library")]
DEV = "cuda:0"
NAMES = ("P", "m", "v", "grad", "stats")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu() if t.dtype == torch.float32 else t.detach().cpu().clone()


def _single(params, act, Cn, B, lr=0.01):
    from robustbnns_amd.conv_train import ConvNnTrainer
    return ConvNnTrainer(act, CR.SHAPE, Cn, params, lr, DEV, batch_size=B)


def _ens(params_list, act, Cn, B, lr=0.01):
    from robustbnns_amd.conv_train import ConvEnsembleTrainer
    return ConvEnsembleTrainer(act, CR.SHAPE, Cn, params_list, lr, DEV, batch_size=B)


def _member_state(tr, k):
    """P, m, v, grad of member k in state_dict order, and its stats row: the bits."""
    st = {name: _bits(torch.cat([v.reshape(-1) for v in tr.unflat(getattr(tr, name), k).values()])) for name in NAMES[:4]}
    st["stats"] = _bits(tr.stats[k])
    return st


def _single_state(tr):
    return {name: _bits(getattr(tr, name)) for name in NAMES}


_DATA = {}


def _data(Cn, n=40):
    """n resident points and labels (computed once, shared, never modified)."""
    if (Cn, n) not in _DATA:
        g = torch.Generator().manual_seed(4000 + 10 * n + Cn)
        _DATA[Cn, n] = (torch.rand(n, *CR.SHAPE, generator=g), torch.randint(0, Cn, (n,), generator=g))
    return _DATA[Cn, n]


def _rows(M, B, n, steps, seed):
    """[steps][M, B] row indices: different per member, out of order, one index twice inside member 0, one row shared by members 1 and 2."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(steps):
        r = torch.randint(0, n, (M, B), generator=g, dtype=torch.int32)
        r[0, 1] = r[0, 0]
        r[1, 0] = r[2, 0]
        out.append(r)
    return out


@pytest.mark.parametrize("Hc,act,B", [(16, "leaky", 5), (16, "leaky", 65), (16, "tanh", 5), (48, "leaky", 65), (144, "tanh", 129)])
def test_member_equals_the_net_trained_alone_bit_for_bit(Hc, act, B):
    """Four steps of M = 3 members on their own rows of 40 resident points; then P, m, v, grad and stats of member k, as int32, are those of a
    ConvNnTrainer stepped alone on data[rows[k]].  B = 65 crosses the 64-row tile of the GEMMs and gives dK1 and dK2 more than one slice;
    Hc = 48 leaves a ragged 64-channel tile and gives dP1 three slices.  (144, tanh, 129) is conv_restate.REGIME_CASES[0]'s plan: the
    per-member offsets of the partial sums (sP nP, s2 Hc N2, s1 C1 N1) carry 5 slices of 2 groups (the last of 1), 15 slices of 9 points (the
    last of 3) and 65 slices of 2 points (the last of 1), with a fold inside the slices of dP1, dK2 and dK1."""
    if (Hc, B) == (144, 129):
        assert CR.slice_plan(B, Hc) == {"dP1": (2, 5), "dK2": (9, 15), "dK1": (2, 65)}
    Cn, M, steps = 10, 3, 4
    x, lab = _data(Cn)
    params = [CR.fresh_params(act, Hc, Cn, 50 + k) for k in range(M)]
    rows = _rows(M, B, len(x), steps, 900 + Hc + B)
    tr = _ens(params, act, Cn, B)
    tr.set_data(x, lab)
    for r in rows:
        tr.step(rows=r.to(DEV))
    torch.cuda.synchronize()
    assert tr.t == steps and tuple(tr.stats.shape) == (M, 3)
    n_diff = 0
    for k in range(M):
        one = _single(params[k], act, Cn, B)
        for r in rows:
            idx = r[k].long()
            one.step(x[idx].to(DEV), lab[idx].to(DEV))
        torch.cuda.synchronize()
        a, b = _member_state(tr, k), _single_state(one)
        for name in NAMES:
            d = int((a[name] != b[name]).sum())
            n_diff += d
            assert d == 0, f"member {k}: {name} differs from the net trained alone in {d} of {a[name].numel()} elements"
        assert float(one.stats[1]) > 0 and bool(torch.isfinite(one.P).all())
    print(f"[conv-ensemble member Hc={Hc} {act} B={B}] {n_diff} differing elements over P, m, v, grad, stats of {M} members after {steps} steps "
          f"(bar 0); excluded: nothing")


def test_gradients_of_member_one_match_fp64_autograd():
    """tests/test_hip_conv_train.py::test_gradients_loss_and_count_match_fp64_autograd's bars, unchanged, on member 1 of 3: per tensor
    max |dW - fp64| <= 1e-5 max |fp64 dW|, per-point CE 1e-5 max(1, CE), step loss 1e-5 relative, correct count within the case's n_marginal
    (the caps on what the case excludes: tests/test_conv_train_cpu.py)."""
    Hc, act, B, Cn = 16, "relu", 5, 3
    c = CR.grad_case(Hc, act, B, Cn)
    ref = c["ref"]
    g = torch.Generator().manual_seed(31)
    extra, extra_lab = torch.rand(7, *CR.SHAPE, generator=g), torch.randint(0, Cn, (7,), generator=g)
    x, lab = torch.cat([extra, c["x"]]), torch.cat([extra_lab, c["lab"]])
    rows = torch.tensor([[3, 0, 6, 0, 9], [7, 8, 9, 10, 11], [11, 2, 1, 5, 4]], dtype=torch.int32)
    tr = _ens([CR.fresh_params(act, Hc, Cn, 11), c["params"], CR.fresh_params(act, Hc, Cn, 12)], act, Cn, 2)      # smaller than B: the workspaces grow
    tr.set_data(x, lab)
    tr.gradients(rows=rows.to(DEV))
    torch.cuda.synchronize()
    G = tr.unflat(tr.grad, 1)
    assert list(G) == CR.KEYS
    errs = {}
    for k, g64 in ref["grad"].items():
        gmax, err = float(g64.abs().max()), float((G[k].cpu().double() - g64).abs().max())
        errs[k] = err / (1e-5 * gmax)
    print(f"[conv-ensemble grad member 1 of 3, Hc={Hc} {act} B={B} C={Cn}] gradient error per tensor in units of 1e-5 max|fp64 gradient|: "
          + ", ".join(f"{k[6:]} {v:.3f}" for k, v in errs.items()))
    e = (tr.ws_t["ce"][B:2 * B].cpu().double() - ref["ce"]).abs() / (1e-5 * ref["ce"].clamp_min(1.0))
    assert max(errs.values()) <= 1.0, errs
    assert float(e.max()) <= 1.0, float(e.max())
    tr.step(rows=rows.to(DEV))
    stats = tr.stats[1].tolist()
    w_loss = abs(stats[0] - ref["loss"]) / (1e-5 * abs(ref["loss"]))
    assert w_loss <= 1.0, (stats[0], ref["loss"])
    assert stats[1] == stats[0] and stats[0] == float(torch.tensor(stats[0], dtype=torch.float32))
    assert ref["c_safe"] <= stats[2] <= ref["c_safe"] + ref["n_marginal"] and stats[2] == int(stats[2]), (stats[2], ref["c_safe"])
    print(f"[conv-ensemble grad member 1 of 3] worst gradient error {max(errs.values()):.3f} x (1e-5 max|fp64 gradient|); per-point CE {float(e.max()):.3f} x bar; "
          f"step loss {w_loss:.3f} x 1e-5; excluded: {c['n_drop']} of {c['n_pool']} pool points at a kink or a pooling tie, {ref['n_marginal']} of {B} points "
          f"within the argmax margin")


def _three_steps(params, x, lab, rows, act, Cn, B):
    tr = _ens(params, act, Cn, B)
    tr.set_data(x, lab)
    for r in rows:
        tr.step(rows=r.to(DEV))
    torch.cuda.synchronize()
    return [_member_state(tr, k) for k in range(len(params))]


def test_members_are_isolated_from_each_other_and_from_rows_nobody_names():
    """Member 1's parameters NaN and every data row outside all rows NaN: members 0 and 2 keep the bits of the clean run (NaN in, NaN out for
    member 1 is data, not a fault)."""
    Hc, act, B, Cn, M = 16, "leaky", 5, 10, 3
    x, lab = _data(Cn)
    params = [CR.fresh_params(act, Hc, Cn, 70 + k) for k in range(M)]
    rows = _rows(M, B, len(x), 3, 77)
    clean = _three_steps(params, x, lab, rows, act, Cn, B)
    named = torch.zeros(len(x), dtype=torch.bool)
    named[torch.cat(rows).reshape(-1).long()] = True
    assert 0 < int(named.sum()) < len(x)
    xd = x.clone()
    xd[~named] = float("nan")
    pd = [params[0], {k: torch.full_like(v, float("nan")) for k, v in params[1].items()}, params[2]]
    dirty = _three_steps(pd, xd, lab, rows, act, Cn, B)
    for k in (0, 2):
        for name in NAMES:
            assert torch.equal(clean[k][name], dirty[k][name]), f"member {k}: {name} depends on member 1 or on a row nobody names"
            if name != "stats":
                assert bool(torch.isfinite(clean[k][name].view(torch.float32)).all()), name
    assert bool(torch.isnan(dirty[1]["P"].view(torch.float32)).all())
    print(f"[conv-ensemble isolation Hc={Hc} {act} B={B}] members 0 and 2: P, m, v, grad, stats bit-identical and finite with member 1 NaN and "
          f"{int((~named).sum())} of {len(x)} unnamed data rows NaN; excluded: nothing")


def test_two_identical_runs_are_bit_identical():
    Hc, act, Cn, M = 16, "leaky", 10, 3
    x, lab = _data(Cn)
    params = [CR.fresh_params(act, Hc, Cn, 80 + k) for k in range(M)]
    rows = [r[:, :b].contiguous() for r, b in zip(_rows(M, 8, len(x), 3, 78), (8, 8, 5))]
    a, b = _three_steps(params, x, lab, rows, act, Cn, 8), _three_steps(params, x, lab, rows, act, Cn, 8)
    for k in range(M):
        for name in NAMES:
            assert torch.equal(a[k][name], b[k][name]), f"two identical runs differ in {name} of member {k}"
        assert float(a[k]["stats"][1]) > 0
    print(f"[conv-ensemble repeat Hc={Hc} {act}] P, m, v, grad, stats of {M} members bit-identical between two runs of 3 steps (B = 8, 8, 5); excluded: nothing")


def _ensemble(M=3):
    from robustbnns_amd.model_ensemble import Ensemble_NN
    return Ensemble_NN("mnist", 16, "leaky", "conv", 2, 0.01, CR.SHAPE, 10, M)


@pytest.mark.parametrize("group", [None, 2])
def test_train_conv_end_to_end_equals_every_member_trained_alone(group, capsys, tmp_path, monkeypatch):
    """ensemble_size 3, Hc 16, 2 epochs of 130 points (one full batch of 100 and a ragged one of 30): every member's state_dict is the bits of
    that member trained alone through ConvNnTrainer on ensemble_schedule's weights and batches; the epoch lines come member by member; the
    files load back; forward runs.  group = 2: the members in groups of 2 and 1, the same bits."""
    from robustbnns_amd import conv_train
    from robustbnns_amd.nn_train import ENSEMBLE_BATCH, ensemble_schedule, epoch_line
    from robustbnns_amd.savedir import TESTS
    monkeypatch.chdir(tmp_path)
    n, M = 130, 3
    g = torch.Generator().manual_seed(5)
    x, lab = torch.rand(n, *CR.SHAPE, generator=g), torch.randint(0, 10, (n,), generator=g)
    y = torch.eye(10)[lab]
    # every member alone, on the schedule the same generator state gives
    torch.manual_seed(21)
    probe = _ensemble()
    members, schedule = ensemble_schedule(probe, n)
    assert tuple(schedule.shape) == (M, 2, n)
    alone, expected = [], ""
    for k, net in enumerate(members):
        one = _single(net.state_dict(), "leaky", 10, ENSEMBLE_BATCH)
        expected += "\n == NN training ==\n"
        for epoch in range(2):
            one.begin_epoch()
            for i in range(0, n, ENSEMBLE_BATCH):
                idx = schedule[k, epoch, i:i + ENSEMBLE_BATCH]
                one.step(x[idx].to(DEV), lab[idx].to(DEV))
            expected += epoch_line(epoch, *one.epoch_totals(), n) + "\t"
        alone.append({key: v.cpu() for key, v in one.params().items()})
    torch.manual_seed(21)
    ens = _ensemble()
    capsys.readouterr()
    if group is None:
        tr = ens.train_conv(x, y, DEV)
    else:
        tr = conv_train.train_conv_ensemble(ens, x, y, DEV, group=group)
    out = capsys.readouterr().out
    assert list(ens.ensemble_models) == ["0", "1", "2"] and ens.device == DEV and ens._ens_engine is None
    assert tr.M == (M if group is None else 1) and tr.t == 4
    n_diff = 0
    for k in range(M):
        sd = ens.ensemble_models[str(k)].state_dict()
        assert list(sd) == CR.KEYS
        for key, v in sd.items():
            d = int((_bits(v) != _bits(alone[k][key])).sum())
            n_diff += d
            assert d == 0, f"member {k}: {key} differs from the member trained alone in {d} elements"
    assert expected in out, (expected, out)
    assert len(NR.parse_epoch_lines(out)) == 2 * M
    files = sorted(os.listdir(os.path.join(TESTS, ens.name, "weights")))
    assert files == [f"{ens.ensemble_models['0'].name}_weights_{s}.pt" for s in range(M)]
    fresh = _ensemble()
    fresh.load(DEV)
    for k in range(M):
        for key, v in fresh.ensemble_models[str(k)].state_dict().items():
            assert torch.equal(v.cpu(), alone[k][key]), (k, key)
    z = ens.forward(x[:8], n_samples=3)
    assert tuple(z.shape) == (8, 10) and bool(torch.isfinite(z).all()) and torch.equal(z, fresh.forward(x[:8], n_samples=3))
    print(f"[conv-ensemble train_conv group={group}] {n_diff} differing elements over the state_dicts of {M} members after 2 epochs of {n} points "
          f"(bar 0); {2 * M} epoch lines member by member; excluded: nothing")


def test_twenty_steps_make_no_device_to_host_sync():
    Hc, act, Cn, M = 16, "leaky", 10, 3
    x, lab = _data(Cn)
    tr = _ens([CR.fresh_params(act, Hc, Cn, 90 + k) for k in range(M)], act, Cn, 8)
    tr.set_data(x, lab)
    rows = [r.to(DEV) for r in _rows(M, 8, len(x), 21, 79)]
    short = [r[:, :8 - i % 3].contiguous() for i, r in enumerate(rows)]
    tr.step(rows=rows[0])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for i in range(20):
            tr.step(rows=short[i + 1])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    totals = tr.epoch_totals()
    assert tr.t == 21 and len(totals) == M and all(loss == loss and 0 <= correct <= 21 * 8 for loss, correct in totals)


def test_guards_raise_with_no_state_changed():
    from robustbnns_amd.conv_train import ConvEnsembleTrainer
    from robustbnns_amd.model_ensemble import Ensemble_NN
    x, y = torch.rand(8, *CR.SHAPE), torch.eye(10)[torch.arange(8)]
    fc = Ensemble_NN("mnist", 16, "leaky", "fc", 1, 0.01, CR.SHAPE, 10, 2)
    with pytest.raises(ValueError, match="train"):
        fc.train_conv(x, y, DEV)
    conv = Ensemble_NN("mnist", 16, "leaky", "conv", 1, 0.01, CR.SHAPE, 10, 2)
    with pytest.raises(NotImplementedError, match="no CPU compute path"):
        conv.train_conv(x, y, "cpu")
    conv.input_shape = (3, 32, 32)
    with pytest.raises(NotImplementedError, match="1x28x28"):
        conv.train_conv(x, y, DEV)
    conv.input_shape = CR.SHAPE
    with pytest.raises(NotImplementedError, match="conv"):
        conv.train(x, y, DEV)                                              # Ensemble_NN.train keeps refusing conv, and names train_conv
    with pytest.raises(NotImplementedError, match="train_conv"):
        conv.train(x, y, DEV)
    assert fc.ensemble_models == {} and conv.ensemble_models == {} and not hasattr(conv, "device") and not hasattr(fc, "device")
    params = [CR.fresh_params("leaky", 16, 10, 1), CR.fresh_params("leaky", 16, 10, 2)]
    with pytest.raises(NotImplementedError, match="no CPU compute path"):
        ConvEnsembleTrainer("leaky", CR.SHAPE, 10, params, 0.01, "cpu")
    with pytest.raises(NotImplementedError, match="1x28x28"):
        ConvEnsembleTrainer("leaky", (3, 32, 32), 10, params, 0.01, DEV)
    # a trainer refuses rows it cannot use before anything is launched: no half-applied step
    tr = _ens(params, "leaky", 10, 4)
    keep = [_member_state(tr, k) for k in range(2)]
    with pytest.raises(ValueError):
        tr.step(rows=torch.zeros(2, 4, dtype=torch.int32, device=DEV))      # no resident data
    tr.set_data(x, y.argmax(-1))
    for bad in (torch.zeros(3, 4, dtype=torch.int32, device=DEV), torch.zeros(8, dtype=torch.int32, device=DEV),
                torch.zeros(2, 4, dtype=torch.int64, device=DEV), torch.zeros(2, 4, dtype=torch.int32)):
        with pytest.raises(ValueError):
            tr.step(rows=bad)
        with pytest.raises(ValueError):
            tr.gradients(rows=bad)
    now = [_member_state(tr, k) for k in range(2)]
    assert tr.t == 0 and all(torch.equal(keep[k][name], now[k][name]) for k in range(2) for name in NAMES)
