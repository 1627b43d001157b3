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
