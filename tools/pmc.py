#!/usr/bin/env python3
"""rocprofv3 counter passes of a bench workload or of a stand-alone program, each set a run of its own, and the one summariser of their CSV.

    python tools/pmc.py <tag> <workload> [--sets sq lds] [--filter NAME ...] [bench args...]     -> <OUT>/<tag>/pmc_<workload>.txt (OUT: tools/steps.py)
    python tools/pmc.py <tag> --exe <program> [--sets sq lds] [--filter fc_forward fc_grad]       (a program that tools/ab.py harness built)

Per kernel, mean per launch: wall cycles = GRBM_GUI_ACTIVE / 8 (XCDs), the matrix pipe's busy fraction of 1024 SIMDs, the waiting fraction of the
wave cycles, the LDS's active fraction of 256 CUs, its bank conflicts per active cycle.  --filter keeps the kernels whose name holds a fragment."""
import argparse
import collections
import csv
import glob
import os
import re
import shutil
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import steps                                                  # noqa: E402

SETS = {"sq": ["SQ_VALU_MFMA_BUSY_CYCLES", "SQ_BUSY_CYCLES", "SQ_WAVE_CYCLES", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY", "SQ_INSTS_VALU", "GRBM_GUI_ACTIVE"],
        "lds": ["SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE", "SQ_INSTS_LDS", "GRBM_GUI_ACTIVE"],
        "fetch": ["FETCH_SIZE"], "write": ["WRITE_SIZE"]}


def rocprof(runner, kind, name, what, outdir, program, env=None):
    """One rocprofv3 run of `program` (after `--`) as a step of the runner; what: ["--stats"] or ["--pmc", counters...]."""
    tmp = tempfile.gettempdir()
    cmd = ["rocprofv3", "--kernel-trace"] + what + ["--output-format", "csv", "-d", outdir, "-o", "run", "--"] + list(program)
    return runner.gpu(kind, name, cmd, env={**(env or {}), "TMPDIR": tmp}, cwd=tmp)


def kernel_name(name):
    m = re.search(r"(\w+_kernel)", name)
    return (m.group(1) if m else name[:40]) + ("<3,32>" if "Geo<3, 32>" in name else "")


def read(root, name_of=kernel_name):
    """{kernel: {counter: [value per launch]}} of every *counter_collection.csv under root."""
    acc = collections.defaultdict(lambda: collections.defaultdict(list))
    for f in glob.glob(os.path.join(root, "**", "*counter_collection.csv"), recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                acc[name_of(r["Kernel_Name"])][r["Counter_Name"]].append(float(r["Counter_Value"]))
    return acc


def derive(m):
    """The derived quantities of one kernel's mean counters (only those whose counters were collected)."""
    out = {}
    if "GRBM_GUI_ACTIVE" in m:
        cyc = out["wall_cycles"] = m["GRBM_GUI_ACTIVE"] / 8
        if "SQ_VALU_MFMA_BUSY_CYCLES" in m:
            out["mfma_busy_frac"] = m["SQ_VALU_MFMA_BUSY_CYCLES"] / (1024 * cyc + 1e-9)
        if "SQ_LDS_IDX_ACTIVE" in m:
            out["lds_active_frac"] = m["SQ_LDS_IDX_ACTIVE"] / (256 * cyc + 1e-9)
    if "SQ_WAIT_INST_ANY" in m and "SQ_WAVE_CYCLES" in m:
        out["wait_frac_of_wave_cycles"] = m["SQ_WAIT_INST_ANY"] / (m["SQ_WAVE_CYCLES"] + 1e-9)
    if "SQ_LDS_IDX_ACTIVE" in m:
        out["conflict/active"] = m.get("SQ_LDS_BANK_CONFLICT", 0) / (m["SQ_LDS_IDX_ACTIVE"] + 1e-9)
    return out


def summary(acc, keep=()):
    """One line per kernel, longest first: launches, derived quantities, mean counters."""
    lines = []
    for n, d in sorted(acc.items(), key=lambda kv: -sum(kv[1].get("GRBM_GUI_ACTIVE", [0]))):
        if keep and not any(k in n for k in keep):
            continue
        m = {c: sum(v) / len(v) for c, v in d.items()}
        q = derive(m)
        lines.append(f"{n:36s} launches={max(len(v) for v in d.values()):3d} " + " ".join(f"{k}={v:.4g}" if k == "wall_cycles" else f"{k}={v:.3f}" for k, v in q.items())
                     + " | " + " ".join(f"{c}={v:.4g}" for c, v in sorted(m.items())))
    return lines


def run(runner, what, program, sets, keep=()):
    """One pass per set under the runner; -> the summary lines (also in <out>/pmc_<what>.txt).  The bulky CSV trees are removed."""
    lines = []
    for s in sets:
        d = os.path.join(runner.out, f"pmc_{s}_{what}")
        rocprof(runner, "pmc", f"pmc_{s}_{what}", ["--pmc"] + SETS[s], d, program)
        lines += [f"{s:5s} {ln}" for ln in summary(read(d), keep)]
        shutil.rmtree(d, ignore_errors=True)
        with open(os.path.join(runner.out, f"pmc_{what}.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    return lines


def main():
    ap = argparse.ArgumentParser(usage=__doc__)
    ap.add_argument("tag")
    ap.add_argument("workload", nargs="?")
    ap.add_argument("--exe")
    ap.add_argument("--sets", nargs="+", default=["sq", "lds"], choices=list(SETS))
    ap.add_argument("--filter", nargs="+", default=[])
    a, bench_args = ap.parse_known_args()
    what, program = (os.path.basename(a.exe), [a.exe]) if a.exe else (a.workload, steps.bench_command(["--workload", a.workload] + bench_args))
    print("\n".join(run(steps.Runner(a.tag), what, program, a.sets, a.filter)))


if __name__ == "__main__":
    main()
