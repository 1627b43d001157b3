"""tools/steps.py, tools/ab.py, tools/pmc.py on the CPU: command lines are built by pure functions and the process starter is a fake, so nothing
here starts a compiler, a profiler or the benchmark."""
import os
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tools"), ROOT]
import __graft_entry__ as G                                   # noqa: E402
import ab                                                     # noqa: E402
import pmc                                                    # noqa: E402
import steps                                                  # noqa: E402

FAULT = "HIP error: an illegal memory access was encountered"
BENCH_JSON = open(os.path.join(ROOT, "profiles", "r06z", "bench.json")).read().strip().splitlines()[-1]


class Fake:
    """In place of steps.start: records every command; answers[n] = (status, output) of the n-th GPU step (1-based), compile_fails: the
    numbers of the compile commands that fail.  A GPU step prints a bench line unless told otherwise."""
    def __init__(self, answers=None, compile_fails=()):
        self.answers, self.compile_fails, self.gpu, self.host, self.compiles = answers or {}, compile_fails, [], [], 0

    def __call__(self, cmd, cwd=None, env=None, stdout=None, stderr=None, **kw):
        if cmd[0] == "timeout":
            self.gpu.append((cmd, env))
            status, out = self.answers.get(len(self.gpu), (0, BENCH_JSON))
            stdout.write(out + "\n")
            stdout.flush()
            return types.SimpleNamespace(returncode=status)
        self.host.append(cmd)
        if "-c" in cmd and cmd[0] == G.HIPCC:
            self.compiles += 1
            if self.compiles in self.compile_fails:
                return types.SimpleNamespace(returncode=1, stdout="error: no such macro")
        return types.SimpleNamespace(returncode=0, stdout="")


@pytest.fixture
def fake(monkeypatch, tmp_path):
    f = Fake()
    monkeypatch.setattr(steps, "start", f)
    f.runner = steps.Runner("t", root=str(tmp_path))
    f.lines = []
    return f


def five_steps(runner):
    for i in range(1, 6):
        runner.gpu("bench", f"step{i}", ["prog", str(i)])


@pytest.mark.parametrize("unit", [os.path.basename(s) for s in G.SOURCES])
def test_flags_links_one_object_per_unit_of_the_build(unit):
    compile_cmd, link_cmd = ab.variant_commands(unit, "-DRBNN_ALLOW_ABLATION -DRBNN_X3_L1_ABL_SMALL")
    assert len(G.SOURCES) == 12
    assert [w for w in link_cmd if w.endswith(".o")] == [s[:-4] + ".o" for s in G.SOURCES]
    assert link_cmd[link_cmd.index("-o") + 1] == G.LIB and all(f in link_cmd for f in G.LDFLAGS)
    assert compile_cmd[:1 + len(G.CFLAGS)] == [G.HIPCC] + G.CFLAGS and G.CFLAGS == ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]
    assert compile_cmd[1 + len(G.CFLAGS):] == ["-DRBNN_ALLOW_ABLATION", "-DRBNN_X3_L1_ABL_SMALL", "-c", os.path.join(G.CSRC, unit), "-o", os.path.join(G.CSRC, unit[:-4] + ".o")]


def test_flags_refuses_a_file_that_is_no_unit():
    with pytest.raises(SystemExit):
        ab.variant_commands("rbnn_common.hpp", "")


@pytest.mark.parametrize("answer", [(134, ""), (139, ""), (124, ""), (137, ""), (-6, ""), (-11, ""), (-9, ""), (0, FAULT), (1, "")])
def test_nothing_is_started_after_a_failed_step(fake, answer):
    fake.answers = {2: answer}
    with pytest.raises(steps.Stop) as e:
        five_steps(fake.runner)
    assert [c[-1] for c, _ in fake.gpu] == ["1", "2"]                      # steps 3 to 5 never started, none started twice
    assert e.value.code not in (0, None) and "02_step2.log" in str(e.value.code)      # SystemExit with a message: status 1, the log's path shown
    log = open(os.path.join(fake.runner.out, "02_step2.log")).read()
    assert "prog 2" in log and "status %d" % answer[0] in log and answer[1] in log


@pytest.mark.parametrize("answer", [(134, ""), (139, ""), (124, ""), (137, ""), (-6, ""), (-11, ""), (-9, ""), (0, FAULT), (1, "")])
def test_flags_restores_the_library_after_a_stop(fake, answer):
    fake.answers, before = {2: answer}, dict(os.environ)
    with pytest.raises(steps.Stop):
        ab.run_flags(fake.runner, fake.lines.append, "rbnn_triple.hip", None, ["--workload", "c2"], ["", "-DA", "-DB", "-DC", "-DD"])
    assert len(fake.gpu) == 2 and fake.host[-1] == ab.RESTORE and "build(force=True)" in ab.RESTORE[-1]
    assert all(env.get("RBNN_ALLOW_ABLATION") == "1" for _, env in fake.gpu) and dict(os.environ) == before           # for its children only
    assert not any("-DC" in c for c in fake.host)                         # nor is anything built for the flag sets that will not run


def test_a_flag_set_that_does_not_compile_is_reported_and_skipped(fake):
    fake.compile_fails = (2,)
    ab.run_flags(fake.runner, fake.lines.append, "rbnn_triple.hip", None, ["--workload", "c2"], ["-DONE", "-DTWO", "-DTHREE"])
    assert len(fake.gpu) == 2 and fake.host[-1] == ab.RESTORE
    text = "\n".join(fake.lines)
    assert "error: no such macro" in text and text.count("7.009 {'fc_forward'") == 2 and "library rebuilt" in text
    assert [c for c in fake.host if "-shared" in c and c[0] == G.HIPCC] == [ab.variant_commands("rbnn_triple.hip", "")[1]] * 2


def test_every_gpu_command_runs_under_its_limit(fake, monkeypatch, tmp_path):
    ab.run_ab(fake.runner, fake.lines.append, ab.env_configs("c2", ["", "RBNN_FUSED_TAIL=0"], []), 2)
    ab.run_ab(fake.runner, fake.lines.append, ab.RECIPES["collectives"], 1)
    ab.run_ab(fake.runner, fake.lines.append, ab.tree_configs("r05", ["--workload", "c2"]), 1)
    ab.run_flags(fake.runner, fake.lines.append, "rbnn_conv_x3.hip", "tools/dense_stamps.py", ["--workload", "c5"], ["-DRBNN_ALLOW_ABLATION -DRBNN_DENSE_STAMPS=1"])
    monkeypatch.setattr(steps, "compile_all", lambda cmds: [steps.host(c) for c in cmds])
    ab.run_harness(fake.runner, fake.lines.append, "ablate", ["-DRBNN_ABL=0", "-DRBNN_ABL=1"])
    pmc.run(fake.runner, "c1", steps.bench_command(["--workload", "c1"]), ["sq", "lds"])
    kinds = ["bench"] * 6 + ["bench_other"] * 2 + ["bench"] * 2 + ["bench_other"] + ["harness"] * 2 + ["pmc"] * 2      # c1 / c2 lean runs: the measured limit
    assert len(fake.gpu) == len(kinds)
    for (cmd, _), kind in zip(fake.gpu, kinds):
        assert cmd[:4] == ["timeout", "-k", "10", str(steps.LIMITS[kind])]
    assert steps.LIMITS["tests"] == 1100 and steps.LIMITS["harness"] == 120
    logs = sorted(os.listdir(fake.runner.out))
    assert len([f for f in logs if f.endswith(".log")]) == len(kinds)       # one log per step, under <OUT>/<tag>/
    assert fake.runner.out == os.path.join(str(tmp_path), "t")
    env_cmds = [c for c, _ in fake.gpu[:4]]
    assert all(c[4:] == [steps.PY, steps.BENCH, "--workload", "c2", "--steps", "5", "--warmup", "1", "--cpu-seconds", "0", "--no-other-mode"] for c in env_cmds)
    assert [e.get("RBNN_FUSED_TAIL") for _, e in fake.gpu[:4]] == [None, "0", None, "0"]          # alternating
    assert [c[5] for c, _ in fake.gpu[8:10]] == [os.path.join(ROOT, "abtree", "r05", "bench.py"), steps.BENCH]
    assert fake.gpu[10][0][5] == os.path.join(ROOT, "tools", "dense_stamps.py")
    harness = [c for c in fake.host if c[-1].endswith("ablate.hip")]
    assert [c[1:6] for c in harness] == [["--offload-arch=gfx950", "-O3", "-std=c++17", "-DRBNN_ALLOW_ABLATION", "-DRBNN_FAST_BUILD"]] * 2
    for (cmd, _), s in zip(fake.gpu[13:], ("sq", "lds")):                   # counters in a run of their own, the program after `--`
        assert cmd[4:7] == ["rocprofv3", "--kernel-trace", "--pmc"] and cmd[7:7 + len(pmc.SETS[s])] == pmc.SETS[s]
        assert cmd[cmd.index("--") + 1:] == steps.bench_command(["--workload", "c1"])
        assert not any(w.endswith("-trace") and w != "--kernel-trace" for w in cmd) and "--stats" not in cmd


def test_counter_sets():
    assert pmc.SETS == {"sq": ["SQ_VALU_MFMA_BUSY_CYCLES", "SQ_BUSY_CYCLES", "SQ_WAVE_CYCLES", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY", "SQ_INSTS_VALU", "GRBM_GUI_ACTIVE"],
                        "lds": ["SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE", "SQ_INSTS_LDS", "GRBM_GUI_ACTIVE"], "fetch": ["FETCH_SIZE"], "write": ["WRITE_SIZE"]}


def test_bench_line():
    line = steps.bench_line("c2", "noise before\n" + BENCH_JSON + "\n")
    assert line == "c2 1.4268e+08 7.009 {'fc_forward': 3.213, 'fc_input_grad': 3.36}"


def test_counter_summary(tmp_path):
    rows = ["Kernel_Name,Counter_Name,Counter_Value"]
    per_launch = {"void (anonymous namespace)::fc_forward_x3_kernel<2, true>(Args)": [
                      {"GRBM_GUI_ACTIVE": 8000, "SQ_VALU_MFMA_BUSY_CYCLES": 512000, "SQ_WAVE_CYCLES": 4000, "SQ_WAIT_INST_ANY": 1000, "SQ_LDS_IDX_ACTIVE": 64000, "SQ_LDS_BANK_CONFLICT": 16000},
                      {"GRBM_GUI_ACTIVE": 24000, "SQ_VALU_MFMA_BUSY_CYCLES": 1536000, "SQ_WAVE_CYCLES": 12000, "SQ_WAIT_INST_ANY": 3000, "SQ_LDS_IDX_ACTIVE": 192000, "SQ_LDS_BANK_CONFLICT": 48000}],
                  "(anonymous namespace)::fc_grad_x3_kernel(GradPieceArgs)": [
                      {"GRBM_GUI_ACTIVE": 800, "SQ_VALU_MFMA_BUSY_CYCLES": 10240, "SQ_WAVE_CYCLES": 1000, "SQ_WAIT_INST_ANY": 500, "SQ_LDS_IDX_ACTIVE": 2560, "SQ_LDS_BANK_CONFLICT": 0},
                      {"GRBM_GUI_ACTIVE": 800, "SQ_VALU_MFMA_BUSY_CYCLES": 10240, "SQ_WAVE_CYCLES": 1000, "SQ_WAIT_INST_ANY": 500, "SQ_LDS_IDX_ACTIVE": 2560, "SQ_LDS_BANK_CONFLICT": 0}]}
    for name, launches in per_launch.items():
        rows += [f'"{name}",{c},{v}' for d in launches for c, v in d.items()]
    os.makedirs(tmp_path / "sq" / "host" / "1")
    (tmp_path / "sq" / "host" / "1" / "run_counter_collection.csv").write_text("\n".join(rows) + "\n")
    acc = pmc.read(str(tmp_path / "sq"))
    assert sorted(acc) == ["fc_forward_x3_kernel", "fc_grad_x3_kernel"] and len(acc["fc_forward_x3_kernel"]["GRBM_GUI_ACTIVE"]) == 2
    mean = lambda k: {c: sum(v) / len(v) for c, v in acc[k].items()}
    # mean per launch of the forward kernel: GRBM 16000 -> 2000 wall cycles; busy 1024000 / (1024 x 2000); lds 128000 / (256 x 2000); 32000 / 128000; 2000 / 8000
    assert pmc.derive(mean("fc_forward_x3_kernel")) == pytest.approx(
        {"wall_cycles": 2000, "mfma_busy_frac": 0.5, "lds_active_frac": 0.25, "wait_frac_of_wave_cycles": 0.25, "conflict/active": 0.25}, rel=1e-9)
    assert pmc.derive(mean("fc_grad_x3_kernel")) == pytest.approx(
        {"wall_cycles": 100, "mfma_busy_frac": 0.1, "lds_active_frac": 0.1, "wait_frac_of_wave_cycles": 0.5, "conflict/active": 0.0}, rel=1e-9, abs=1e-12)
    lines = pmc.summary(acc)
    assert lines[0].startswith("fc_forward_x3_kernel") and "launches=  2" in lines[0] and "wall_cycles=2000 mfma_busy_frac=0.500 lds_active_frac=0.250" in lines[0]
    assert "wait_frac_of_wave_cycles=0.250 conflict/active=0.250" in lines[0]
    assert [ln.split()[0] for ln in pmc.summary(acc, keep=("fc_grad",))] == ["fc_grad_x3_kernel"]        # the harness's gradient group: a name filter


def test_recipes():
    c2 = ["--steps", "30", "--warmup", "5"]
    assert [(e, t, a) for _, e, t, a in ab.RECIPES["collectives"]] == [
        ({}, False, c2), ({"RBNN_FUSED_TAIL": "0"}, False, c2),
        ({"RBNN_FORCE_COLLECTIVES": "1", "RBNN_FAKE_COLLECTIVES": "1"}, True, c2), ({"RBNN_FORCE_COLLECTIVES": "1"}, True, c2)]
    cmd = steps.bench_command(c2, 29512)
    assert cmd[1:] == ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1", "--master-port", "29512", steps.BENCH,
                       "--gpus", "1", "--steps", "30", "--warmup", "5", "--cpu-seconds", "0", "--no-other-mode"]
    groups = ["0 0", "3 0", "6 0", "13 0", "16 0", "25 0", "50 0", "0 5", "0 10", "0 20", "0 50", "6 10", "16 20"]
    assert [f'{e["RBNN_FC2_GROUP_FWD"]} {e["RBNN_FC2_GROUP_BWD"]}' for _, e, _, _ in ab.RECIPES["fc2_groups"]] == groups
    assert all(t is False and a == ["--workload", "fc2", "--steps", "10", "--warmup", "2", "--posterior", "stored"] and len(e) == 2 for _, e, t, a in ab.RECIPES["fc2_groups"])
    assert ab.env_configs("collectives", [], []) is ab.RECIPES["collectives"]


# ---------------------------------------------------------------------------------------------- the nine tools/*_timing.py programs
import importlib                                              # noqa: E402
import statistics                                             # noqa: E402

import torch                                                  # noqa: E402

import timing                                                 # noqa: E402
import torch_baselines as TB                                  # noqa: E402

ANSWERS = [(134, ""), (139, ""), (124, ""), (137, ""), (-6, ""), (-11, ""), (-9, ""), (0, FAULT), (1, "")]
NINE = ["hmc_timing", "nn_train_timing", "svi_train_timing", "conv_hmc_timing", "conv_svi_train_timing", "conv_train_timing", "chain_diag_timing",
        "uncertainty_timing", "weight_pca_timing"]
# (tool, options, kind, tag, the arguments that tell each case's child from the others)
PARENTS = [
    ("hmc_timing", [], "hmc_timing", "hmc_timing", [["--shape", s] for s in ("2,32,2,1024", "2,128,2,1024", "2,512,2,1024", "784,512,10,5000")]),
    ("hmc_timing", ["--chains", "8"], "hmc_timing", "hmc_timing", [["--shape", s, "--chains", "8"] for s in ("2,32,2,1024", "2,512,2,1024")]),
    ("nn_train_timing", [], "nn_train_timing", "nn_train_timing", [["--nets", H, "--members", "1,10,100", "--steps", "100"] for H in ("512", "1024")]),
    ("svi_train_timing", [], "svi_train_timing", "svi_train_timing", [["--nets", H, "--steps-per-epoch", "0", "--warmup", "20"] for H in ("512", "1024")]),
    ("svi_train_timing", ["--members", "1,8,32"], "svi_train_timing", "svi_train_timing",
     [["--nets", H, "--members", K, "--steps", "40"] for H in ("32", "512") for K in ("1", "8", "32")]),
    ("conv_hmc_timing", [], "timing", "conv_hmc_timing", [["--nets", H, "--torch", "1", "--n", "2", "--batch", "5000"] for H in ("512", "1024")]),
    ("conv_hmc_timing", ["--chains", "1,8"], "timing", "conv_hmc_timing", [["--nets", H, "--chains", K, "--n", "2"] for H in ("512", "1024") for K in ("1", "8")]),
    ("conv_svi_train_timing", [], "timing", "conv_svi_timing", [["--nets", H, "--steps", "40"] for H in ("512", "1024")]),
    ("conv_svi_train_timing", ["--members", "1,8,32"], "timing", "conv_svi_lockstep_timing",
     [["--nets", H, "--members", K, "--accuracy", acc, "--steps", "40"] for H in ("512", "1024") for K in ("1", "8", "32") for acc in ("1", "0")]),
    ("conv_train_timing", [], "timing", "conv_train_timing", [["--nets", H, "--steps", "40"] for H in ("512", "1024")]),
    ("conv_train_timing", ["--members", "1,8,32"], "timing", "conv_ensemble_timing",
     [["--nets", H, "--members", M, "--steps", "40"] for H in ("512", "1024") for M in ("1", "8", "32")]),
    ("chain_diag_timing", [], "timing", "chain_diag_timing", [["--cases", c, "--reps", "7", "--torch-reps", "3"] for c in ("8x50", "8x250")]),
    ("uncertainty_timing", [], "timing", "uncertainty_timing", [["--cases", c, "--reps", "7"] for c in ("fc512", "conv512", "parity_fc", "parity_conv")]),
    ("weight_pca_timing", [], "timing", "weight_pca_timing", [["--cases", c, "--reps", "7", "--host-reps", "3"] for c in ("posterior50", "same150", "prior1000")]),
]


@pytest.fixture
def fake_out(monkeypatch, tmp_path):
    f = Fake()
    monkeypatch.setattr(steps, "start", f)
    monkeypatch.setattr(steps, "OUT", str(tmp_path))
    f.root = str(tmp_path)
    return f


def holds(cmd, words):
    return any(cmd[i:i + len(words)] == words for i in range(len(cmd)))


@pytest.mark.parametrize("tool, options, kind, tag, cases", PARENTS, ids=[p[0] + "".join(p[1][:1]) for p in PARENTS])
def test_timing_tool_starts_one_checked_child_per_case(fake_out, capsys, tool, options, kind, tag, cases):
    assert sorted({p[0] for p in PARENTS}) == sorted(NINE)
    importlib.import_module(tool).main(options)
    assert len(fake_out.gpu) == len(cases)
    script = os.path.join(ROOT, "tools", tool + ".py")
    for (cmd, _), words in zip(fake_out.gpu, cases):
        assert cmd[:7] == ["timeout", "-k", "10", str(steps.LIMITS[kind]), steps.PY, script, "--child"]
        assert holds(cmd, words[:2]) and all(holds(cmd, words[i:i + 2]) for i in range(0, len(words), 2))
    assert len([f for f in os.listdir(os.path.join(fake_out.root, tag)) if f.endswith(".log")]) == len(cases)       # one log per case under <OUT>/<tag>/
    assert capsys.readouterr().out.count('"metric"') == len(cases)               # each child's last JSON line is printed (here: the fake's bench line)


@pytest.mark.parametrize("answer", ANSWERS)
@pytest.mark.parametrize("tool", NINE)
def test_timing_tool_starts_nothing_after_a_failed_case(fake_out, tool, answer):
    fake_out.answers = {2: answer}
    with pytest.raises(steps.Stop):
        importlib.import_module(tool).main([])
    assert len(fake_out.gpu) == 2 and fake_out.gpu[0][0] != fake_out.gpu[1][0]          # the third case never started, none started twice


@pytest.mark.parametrize("n", [1, 2, 7, 8])
def test_timing_summary(n):
    ms = sorted(3.0 + ((5 * i) % 7) * 0.25 for i in range(n))
    s = timing.summary(ms)
    assert s["median"] == statistics.median(ms) and s["spread"] == (ms[-1] - ms[0]) / statistics.median(ms)
    assert (s["min"], s["max"], s["blocks"]) == (ms[0], ms[-1], n)
    assert timing.summary(ms, 4)["median"] == statistics.median(ms) / 4 and timing.summary(ms, 4)["spread"] == s["spread"]
    assert timing.stats(ms) == {"median_ms": s["median"], "min_ms": ms[0], "max_ms": ms[-1], "runs": n}


def test_timing_tools_fill_their_figures_from_the_summary():
    ms, tool = [1.0, 2.0, 4.0, 5.0, 9.0], importlib.import_module
    assert timing.summary(ms)["blocks"] == 5 and timing.stats(ms)["runs"] == 5 and "runs" not in timing.stats(ms, runs=False)
    assert tool("conv_hmc_timing").figures(ms, 2) == {"ms_per_transition": 2.0, "ms_per_leapfrog_step": 0.2, "chain_transitions_per_s": 500.0, "spread": 2.0}
    assert tool("conv_svi_train_timing").figure(ms, 4, 2) == {"ms_per_step": 1.0, "spread": 2.0, "guide_steps_per_s": 2000.0}
    assert tool("conv_train_timing").figure(ms, 4) == {"ms_per_step": 1.0, "spread": 2.0}
    assert tool("nn_train_timing").figure(ms, 8, "a", "a_spread") == {"a": 0.5, "a_spread": 2.0}
    wall = timing.wall(lambda: None, 5, sync=lambda: None)                       # the host clock gives as many times as it was asked for, sorted
    assert len(wall) == 5 and wall == sorted(wall) and timing.stats(wall)["runs"] == 5


def small_nets():
    """(arch, the package's base net, inputs, labels) at fc2 D = 2, H = 32, C = 2, N = 4 and conv 1x28x28, hidden 16, C = 10, N = 2."""
    from robustbnns_amd.model_nn import NN
    torch.manual_seed(3)
    return [("fc2", NN("half_moons", (1, 2, 1), 2, 32, "leaky", "fc2", 0.01, 1), torch.rand(4, 1, 2, 1), torch.tensor([0, 1, 1, 0])),
            ("conv", NN("mnist", (1, 28, 28), 10, 16, "leaky", "conv", 0.01, 1), torch.rand(2, 1, 28, 28), torch.tensor([3, 7]))]


def test_baseline_logits_are_the_base_nets_forward():
    for arch, net, x, _ in small_nets():
        W = dict(net.state_dict())
        assert list(W) == TB.KEYS[arch] and [tuple(v.shape) for v in W.values()] == [s for _, s in (TB.fc2_shapes(2, 32, 2) if arch == "fc2" else TB.conv_shapes(16, 10))]
        with torch.no_grad():
            assert torch.allclose(TB.logits(arch, W, x), net.model(x))


def test_baseline_hmc_transition():
    for arch, net, x, y in small_nets():
        q0, grad = {k: v.clone() for k, v in net.state_dict().items()}, TB.potential_grad(arch, x, y)
        q, u, g, dH = TB.hmc_transition(grad, (q0, None), torch.Generator().manual_seed(5), 3, 0.0)
        assert all(torch.equal(q[k], q0[k]) for k in q0) and float(dH) == 0.0              # a step of size 0 goes nowhere, bit for bit
        assert torch.equal(u, grad(q0)[0]) and all(torch.equal(g[k], grad(q0)[1][k]) for k in q0)
        runs = [TB.hmc_transition(grad, TB.hmc_transition(grad, (q0, None), gen, 3, 1e-3), gen, 3, 1e-3) for gen in
                (torch.Generator().manual_seed(5), torch.Generator().manual_seed(5))]
        assert all(torch.equal(runs[0][0][k], runs[1][0][k]) for k in q0) and torch.equal(runs[0][3], runs[1][3])
        assert any(not torch.equal(runs[0][0][k], q0[k]) for k in q0) or float(runs[0][3]) > 0    # it moved, or the move was refused


def test_baseline_svi_and_adam_steps_move_every_parameter():
    for arch, net, x, y in small_nets():
        forward = lambda W, x: TB.logits(arch, W, x)
        loc0 = {k: v.clone() for k, v in net.state_dict().items()}
        raw0 = {k: torch.full_like(v, -3.0) for k, v in loc0.items()}
        loc, raw, opt = TB.svi_parameters(loc0, raw0, 0.01, "cpu")
        hits = TB.svi_step(forward, loc, raw, opt, x, y, accuracy=True)
        assert 0 <= int(hits) <= len(y) and TB.svi_step(forward, loc, raw, opt, x, y) is None
        for new, old in ((loc, loc0), (raw, raw0)):
            assert all(bool(torch.isfinite(new[k]).all()) and not torch.equal(new[k].detach(), old[k]) for k in old)
        W = {k: v.clone().requires_grad_(True) for k, v in loc0.items()}
        TB.adam_member_step(forward, W, torch.optim.Adam(list(W.values()), lr=0.01), x, y)
        assert all(bool(torch.isfinite(W[k]).all()) and not torch.equal(W[k].detach(), loc0[k]) for k in loc0)
