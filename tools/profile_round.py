#!/usr/bin/env python3
"""A round's record on the GPU machine: python tools/profile_round.py <tag> <stage>  -> <OUT>/<tag>/  (OUT: tools/steps.py; copy what should be judged into
profiles/<tag>/).  One stage per visit; every GPU step runs under tools/steps.py (its own time limit; the first failure ends the stage).

    tests : the GPU test tier (-s: statistics printed), then smoke()
    bench : every bench workload (JSON lines) + the 1-rank forced-collectives run
    prof  : rocprofv3 --kernel-trace --stats and four separate --pmc passes (fetch, write, sq, lds) of the workloads in WLS (default "c2 c5 conv"; QUICK=1: c2;
            also c3 c4 fc2 fc2_1024 conv1024 eval): five bench runs per workload, so three or four workloads per visit
    trace : the --kernel-trace --stats pass and the summary alone"""
import glob
import json
import os
import shutil
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pmc                                                    # noqa: E402
import steps                                                  # noqa: E402

FULL = [steps.PY, steps.BENCH, "--full"]
FORCED = steps.bench_command(["--steps", "10", "--warmup", "2"], torchrun_port=29511)
# stage bench: (file name, command, environment)
BENCHES = [("bench", FULL + ["--steps", "20", "--warmup", "5"], {}),
           ("bench_c3", FULL + ["--workload", "c3", "--steps", "2", "--warmup", "1", "--cpu-seconds", "10"], {}),
           ("bench_c4", FULL + ["--workload", "c4", "--steps", "5", "--warmup", "1"], {}),
           ("bench_c5_n1024_t10", FULL + ["--workload", "c5", "--points", "1024", "--iters", "10", "--steps", "1", "--warmup", "1", "--cpu-seconds", "10"], {}),
           ("bench_conv", FULL + ["--workload", "conv", "--steps", "5", "--warmup", "1"], {}),
           ("bench_fc2", FULL + ["--workload", "fc2", "--steps", "5", "--warmup", "1"], {}),
           ("bench_fc2_1024", FULL + ["--workload", "fc2_1024", "--steps", "3", "--warmup", "1", "--cpu-seconds", "10"], {}),
           ("bench_conv1024", FULL + ["--workload", "conv1024", "--steps", "3", "--warmup", "1", "--cpu-seconds", "10"], {}),
           ("bench_c1", FULL + ["--workload", "c1", "--steps", "200", "--warmup", "20", "--cpu-seconds", "5"], {}),
           ("bench_eval", FULL + ["--workload", "eval", "--steps", "10", "--warmup", "2", "--cpu-seconds", "10"], {}),
           ("bench_c2_torchrun_1rank_forced_collectives", FORCED, {"RBNN_FORCE_COLLECTIVES": "1"})]
# stage prof: workload -> (points, samples per GPU that the command runs at, bench arguments)
PROF = {"c2": (10000, 100, ["--steps", "5", "--warmup", "2"]),
        "c3": (10000, 500, ["--iters", "2", "--steps", "1", "--warmup", "1", "--no-other-mode"]),
        "c4": (10000, 250, ["--steps", "2", "--warmup", "1", "--no-other-mode"]),
        "fc2": (10000, 100, ["--steps", "3", "--warmup", "1", "--no-other-mode"]),
        "fc2_1024": (10000, 100, ["--steps", "3", "--warmup", "1", "--no-other-mode"]),
        "c5": (512, 62, ["--points", "512", "--iters", "3", "--steps", "1", "--warmup", "1", "--no-other-mode"]),
        "conv": (2048, 16, ["--steps", "3", "--warmup", "1"]),
        "conv1024": (1024, 16, ["--steps", "3", "--warmup", "1", "--no-other-mode"]),
        "eval": (10000, 100, ["--steps", "3", "--warmup", "1", "--no-other-mode"])}


# stage prof's counter sets: the sq / lds sets every committed profiles/*/summary.txt was taken with (tools/pmc.py's own sq / lds sets differ)
SETS = {**pmc.SETS, "sq": ["SQ_INSTS_VALU_MFMA_MOPS_F32", "SQ_VALU_MFMA_BUSY_CYCLES", "SQ_BUSY_CYCLES", "SQ_WAVE_CYCLES", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY"],
        "lds": ["SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE", "GRBM_GUI_ACTIVE"]}


def tests(r):
    print("\n".join(r.gpu("tests", "pytest_gpu", [steps.PY, "-m", "pytest", "tests", "-m", "gpu", "-q", "-s"]).splitlines()[-2:]))
    print(r.gpu("smoke", "smoke", [steps.PY, "-c", "import __graft_entry__ as g; g.smoke()"]).splitlines()[-1])


def bench(r):
    for name, cmd, env in BENCHES:
        d = steps.last_json(r.gpu("bench_full", name, cmd, env=env))
        json.dump(d, open(os.path.join(r.out, name + ".json"), "w"))
        print(name, d["precision_mode"], "%.4g" % d["value"], "%.4g ms" % d["ms_per_step"], flush=True)


def prof(r, passes):
    for wl in ("c2" if os.environ.get("QUICK") else os.environ.get("WLS", "c2 c5 conv")).split():
        points, samples, args = PROF[wl]
        out = os.path.join(r.out, wl)
        program = FULL + ["--workload", wl, "--cpu-seconds", "0"] + args
        for p in passes:
            what, d = (["--stats"], "trace") if p == "trace" else (["--pmc"] + SETS[p], "pmc_" + p)
            pmc.rocprof(r, "bench_full", f"{wl}_{p}", what, os.path.join(out, d), program)
        status, text = steps.host([steps.PY, os.path.join(steps.ROOT, "tools", "summarize_profile.py"), out, wl, str(points), str(samples)])
        open(os.path.join(out, "summary.txt"), "w").write(text)
        if status != 0:
            sys.exit(f"summarize_profile.py failed (status {status}): {out}/summary.txt holds its output")
        for f in glob.glob(os.path.join(out, "trace", "**", "run_kernel_stats.csv"), recursive=True):
            shutil.copy(f, os.path.join(out, "kernel_stats.csv"))
        for f in glob.glob(os.path.join(out, "*", "**", "run_kernel_trace.csv"), recursive=True):       # bulky; the summary keeps the per-kernel numbers
            os.remove(f)
        print("\n".join(text.splitlines()[:30]), flush=True)
    merged = {}
    for f in sorted(glob.glob(os.path.join(r.out, "*", "pmc_traffic.json"))):
        d = json.load(open(f))
        merged.setdefault("source", []).append(d.pop("source", None))
        merged.update(d)
    json.dump(merged, open(os.path.join(r.out, "pmc_traffic.json"), "w"), indent=1)
    print(sorted(k for k in merged if k != "source"))


def main():
    if len(sys.argv) != 3 or sys.argv[2] not in ("tests", "bench", "prof", "trace"):
        sys.exit(__doc__)
    {"tests": tests, "bench": bench, "prof": lambda r: prof(r, ["trace", "fetch", "write", "sq", "lds"]), "trace": lambda r: prof(r, ["trace"])}[sys.argv[2]](steps.Runner(sys.argv[1]))


if __name__ == "__main__":
    main()
