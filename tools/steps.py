"""The one place in tools/ that starts a child process which may use the GPU.

Runner.gpu() runs a command as `timeout -k 10 <LIMITS[kind]> ...` in a fresh child process, stdout and stderr in a log under OUT/<tag>/, then
applies the stop rule of shared GPU machines: after a fault (HIP's illegal-memory-access text, even at status 0), an abort, a segmentation fault, a
time limit or any other non-zero status it raises Stop and the caller starts nothing more on the GPU.  Nothing is retried.  host() runs host-only
work (hipcc, the restore build).  `start` is a module attribute so that a CPU test can put a fake in its place."""
import json
from concurrent.futures import ThreadPoolExecutor
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PY = sys.executable
BENCH = os.path.join(ROOT, "bench.py")
# which directory comes back from a GPU visit is the machine's business: the environment names it, the code does not
OUT = os.path.abspath(os.environ.get("RBNN_TOOLS_OUT") or os.path.join(ROOT, "tools_out"))

# seconds per kind of GPU step; profiles/tools_runner/README.txt says where each comes from.  tests, harness: the earlier scripts'.  bench (a lean
# c1 / c2 run), pmc (the same under rocprofv3 --pmc): 3 x the measured wall time + 90 s.  smoke, bench_full (profile_round's --full runs),
# bench_other (a lean run of another workload or under torch.distributed.run): NOT MEASURED; under seven minutes, so that no step but the test
# tier, whose output streams into its log, can keep a visit silent for longer than that.  timing (one net of conv_svi_train_timing.py, its
# torch-autograd side included): 3 x the measured wall time (12.0 s for conv-512, 10.1 s for conv-1024) + 90 s.
# hmc_timing, nn_train_timing, svi_train_timing (one shape or net of those tools): NOT MEASURED per case; the provisional 400 s of unmeasured kinds
# until profiles/timing_tools/README.txt has the wall times.
LIMITS = {"tests": 1100, "smoke": 300, "harness": 120, "bench": 102, "pmc": 102, "bench_full": 400, "bench_other": 400, "timing": 126,
          "hmc_timing": 400, "nn_train_timing": 400, "svi_train_timing": 400}
STOP_STATUSES = (134, 139, 124, 137, -6, -11, -9)            # abort, segmentation fault, time limit, kill: as a shell and as a Python parent see them
FAULT_TEXT = "an illegal memory access was encountered"

start = subprocess.run                                       # (cmd, cwd=, env=, stdout=, stderr=) -> an object with .returncode


class Stop(SystemExit):
    """A GPU step failed: nothing more may be started on the GPU in this invocation.  Uncaught, it ends the tool with its message and status 1."""


class Runner:
    def __init__(self, tag, root=None):
        self.out = os.path.join(root or OUT, tag)
        os.makedirs(self.out, exist_ok=True)
        self.n = 0

    def gpu(self, kind, name, cmd, env=None, cwd=ROOT):
        """Run one GPU step under its time limit -> its output (stdout + stderr, also in <out>/<nn>_<name>.log); raises Stop when it failed."""
        self.n += 1
        log = os.path.join(self.out, "%02d_%s.log" % (self.n, name))
        full = ["timeout", "-k", "10", str(LIMITS[kind])] + list(cmd)
        t0 = time.time()
        with open(log, "w") as f:
            f.write("$ %s %s\n" % (" ".join("%s=%s" % kv for kv in (env or {}).items()), " ".join(full)))
            f.flush()
            status = start(full, cwd=cwd, env={**os.environ, **(env or {})}, stdout=f, stderr=subprocess.STDOUT).returncode
        text = open(log).read().split("\n", 1)[1]               # the child's output, without the command line above it
        with open(log, "a") as f:
            f.write("[steps] status %d after %.1f s (limit %d s)\n" % (status, time.time() - t0, LIMITS[kind]))
        if status in STOP_STATUSES or FAULT_TEXT in text:
            raise Stop("GPU fault, abort or time limit (status %d) in step %s: nothing more is started; log: %s" % (status, name, log))
        if status != 0:
            raise Stop("step %s ended with status %d; log: %s" % (name, status, log))
        return text


def bench_command(args, torchrun_port=None, bench=BENCH):
    """A lean bench.py run (no CPU leg, one precision mode); torchrun_port: as one rank under torch.distributed.run; bench: another tree's
    bench.py, or a tools script that takes bench.py's arguments."""
    launch = [PY, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1", "--master-port",
              str(torchrun_port), bench, "--gpus", "1"] if torchrun_port else [PY, bench]
    return launch + list(args) + ["--cpu-seconds", "0", "--no-other-mode"]


def bench_kind(args, torchrun=False):
    wl = args[args.index("--workload") + 1] if "--workload" in args else "c2"
    return "bench" if wl in ("c1", "c2") and not torchrun else "bench_other"


def last_json(text):
    """The result line of a bench.py run: the last line of its output that is a JSON object."""
    return json.loads([ln for ln in text.splitlines() if ln.startswith("{")][-1])


def bench_line(label, d):
    """label, value, ms per step and {kernel: avg ms} of a bench.py result (a dict or the text that holds its JSON line)."""
    d = d if isinstance(d, dict) else last_json(d)
    return "%s %.5g %s %s" % (label, d["value"], round(d["ms_per_step"], 3), {k: round(v["avg_ms"], 3) for k, v in d["roofline"]["kernels"].items()})


def host(cmd, cwd=ROOT):
    """Host-only work (a compiler, the restore build) -> (status, output); starts nothing on the GPU."""
    r = start(cmd, cwd=cwd, env=dict(os.environ), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, errors="replace")
    return r.returncode, getattr(r, "stdout", None) or ""


def compile_all(cmds):
    """Run the compile commands, at most 16 at a time -> [(status, output)] in order."""
    with ThreadPoolExecutor(16) as pool:
        return list(pool.map(host, cmds))
