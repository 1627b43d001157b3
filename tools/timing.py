"""The measurement core of the tools/*_timing.py programs: the two clocks, the one summary of a list of times, and the two sides of a tool.

A tool's parent side (cases) starts one child per case through steps.Runner: one time limit each, the log kept, nothing started after a
failure.  Its --child side (child) is the measuring program itself: what to put behind `rocprofv3 --kernel-trace --stats --`."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as G                        # noqa: E402
import steps as S                                  # noqa: E402

BLOCKS = 7                                         # timed blocks or repetitions of a figure, where a tool's options do not say


def blocks(run_block, n_blocks=BLOCKS, warmup=None):
    """Device events: ms of each of n_blocks calls of run_block after one warm-up block (or one call of `warmup`), sorted."""
    (warmup or run_block)()
    torch.cuda.synchronize()
    out = []
    for _ in range(n_blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run_block()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return sorted(out)


def wall(fn, reps, warmup=True, sync=torch.cuda.synchronize):
    """The host clock: ms of each of `reps` whole calls of fn after one warm-up call, the device synchronised before and after, sorted."""
    if warmup:
        fn()
    out = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        out.append(1e3 * (time.perf_counter() - t0))
    return sorted(out)


def summary(ms, per=1):
    """Of a sorted list of times, each divided by `per` (the steps or transitions of a block): median, min, max, the spread
    (max - min) / median, and how many there were."""
    med = statistics.median(ms)
    return {"median": med / per, "min": ms[0] / per, "max": ms[-1] / per, "spread": (ms[-1] - ms[0]) / med, "blocks": len(ms)}


def stats(ms, per=1, runs=True):
    """The summary under the key names of the analysis tools' and hmc_timing.py's records."""
    s = summary(ms, per)
    return {"median_ms": s["median"], "min_ms": s["min"], "max_ms": s["max"], **({"runs": s["blocks"]} if runs else {})}


def cases(tag, script, todo, kind="timing"):
    """The parent side of a tool: every (name, child arguments) of `todo` as `script --child <arguments>` in a child of its own under
    steps.LIMITS[kind], its log under <OUT>/<tag>/; prints each child's last JSON line.  steps.Stop propagates: nothing more is started."""
    runner = S.Runner(tag)
    for name, args in todo:
        text = runner.gpu(kind, name, [S.PY, os.path.abspath(script), "--child"] + [str(v) for v in args])
        print(json.dumps(S.last_json(text)), flush=True)


def child(measure):
    """The child side of a tool: the library is built (a no-op where it is up to date), then measure() -> the case's JSON line."""
    G.build()
    print(json.dumps(measure()), flush=True)


def opts(a, *names):
    """['--name', value, ...] of the parsed options `a`: what a parent hands on to its children."""
    return [w for n in names for w in ("--" + n.replace("_", "-"), getattr(a, n))]
