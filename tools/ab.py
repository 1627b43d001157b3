#!/usr/bin/env python3
"""Same-box A/B runs of bench.py and of the stand-alone harnesses on the GPU machine; every GPU step goes through tools/steps.py (tools/README.md).

    python tools/ab.py env <workload> "<ENV=val ...>" ... [-- bench args]    environments alternating, twice; --steps 5 --warmup 1 by default
    python tools/ab.py env collectives | fc2_groups                           the recipes (RECIPES below)
    python tools/ab.py trees <tag> <rounds> <bench args...>                   abtree/<tag> (`git archive <rev> | tar -x -C abtree/<tag>`, built) against this tree
    python tools/ab.py flags <unit.hip> [--run <tools script>] <bench args...> -- "<flags>" ...   one unit of the library rebuilt per flag set ("" = none)
    python tools/ab.py harness <ablate|ablate_split|ablate_triple> "<flags>" ...   one stand-alone program per flag set (tools/<name>.hip)

Lines go to the terminal and to <OUT>/ab/<subcommand>.txt.  Only numbers of one invocation compare.  A flag set with an ablation switch must also
carry -DRBNN_ALLOW_ABLATION (csrc/rbnn_common.hpp); only the children of `flags` may load such a library, and the product library is rebuilt at its end."""
import os
import shlex
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import __graft_entry__ as G                                   # noqa: E402
import steps                                                  # noqa: E402

STEPS = ["--steps", "5", "--warmup", "1"]
HARNESS_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-DRBNN_ALLOW_ABLATION", "-DRBNN_FAST_BUILD"]
RESTORE = [steps.PY, "-c", "import __graft_entry__ as g; g.build(force=True)"]

# (label, environment, as one rank under torch.distributed.run, bench arguments)
_C2 = ["--steps", "30", "--warmup", "5"]
_FC2 = ["--workload", "fc2", "--steps", "10", "--warmup", "2", "--posterior", "stored"]
RECIPES = {
    # why the 1-rank C2 step with the collectives forced on costs more than the plain step: (b) is what the launch SEQUENCE costs (separate
    # reduce / loss / dZ / slab-sum kernels, G materialised), (c) adds the 1-rank RCCL all-reduces, (d) is the plain step without the fused tail
    "collectives": [("(a) plain, fused tail", {}, False, _C2),
                    ("(d) plain, separate tail kernels", {"RBNN_FUSED_TAIL": "0"}, False, _C2),
                    ("(b) sharded sequence, no-op comm", {"RBNN_FORCE_COLLECTIVES": "1", "RBNN_FAKE_COLLECTIVES": "1"}, True, _C2),
                    ("(c) sharded sequence, 1-rank RCCL", {"RBNN_FORCE_COLLECTIVES": "1"}, True, _C2)],
    # fc2-512, S = 100, N = 10000, stored posterior: samples per reused hidden image, forward / backward (0 = all 100 at once)
    "fc2_groups": [(f"fwd_group={f} bwd_group={b}", {"RBNN_FC2_GROUP_FWD": str(f), "RBNN_FC2_GROUP_BWD": str(b)}, False, _FC2)
                   for f, b in ((0, 0), (3, 0), (6, 0), (13, 0), (16, 0), (25, 0), (50, 0), (0, 5), (0, 10), (0, 20), (0, 50), (6, 10), (16, 20))],
}


def report(path):
    """-> say(line): to the terminal and, as it comes, to the file."""
    def say(line):
        print(line, flush=True)
        with open(path, "a") as f:
            f.write(line + "\n")
    return say


def split_dashes(words):
    i = words.index("--") if "--" in words else len(words)
    return words[:i], words[i + 1:]


def env_configs(workload, envs, bench_args):
    if workload in RECIPES:
        return RECIPES[workload]
    args = ["--workload", workload] + (bench_args or STEPS)
    return [(e, dict(kv.split("=", 1) for kv in e.split()), False, args) for e in envs]


def tree_configs(tag, args):
    return [(tag, {}, False, args, os.path.join(ROOT, "abtree", tag)), ("now", {}, False, args, ROOT)]


def run_ab(runner, say, configs, reps):
    """Every configuration in turn, reps times over: (label, environment, torchrun, bench arguments[, tree to run in])."""
    for rep in range(1, reps + 1):
        for i, (label, env, torchrun, args, *tree) in enumerate(configs):
            port = 29510 + (rep - 1) * len(configs) + i if torchrun else None
            cmd = steps.bench_command(args, port, os.path.join(*tree, "bench.py") if tree else steps.BENCH)
            text = runner.gpu(steps.bench_kind(args, torchrun), f"rep{rep}_{i}", cmd, env=env, cwd=tree[0] if tree else ROOT)
            say(steps.bench_line(f"rep{rep} [{label}]", text))


def variant_commands(unit, flags):
    """(compile, link) of the library with `unit` built with the extra flags: build()'s flags, one object per unit of build()'s list."""
    src = os.path.join(G.CSRC, unit)
    if src not in G.SOURCES:
        raise SystemExit(f"{unit} is not a unit of the library: {[os.path.basename(s) for s in G.SOURCES]}")
    objs = [s[:-4] + ".o" for s in G.SOURCES]
    return [G.HIPCC] + G.CFLAGS + shlex.split(flags) + ["-c", src, "-o", src[:-4] + ".o"], [G.HIPCC] + G.LDFLAGS + ["-o", G.LIB] + objs


def run_flags(runner, say, unit, script, bench_args, flag_sets):
    if "--steps" not in bench_args:
        bench_args = bench_args + STEPS
    cmd = steps.bench_command(bench_args, bench=os.path.join(ROOT, script) if script else steps.BENCH)
    try:
        if not all(os.path.exists(s[:-4] + ".o") for s in G.SOURCES):          # objects may not have travelled with the tree
            status, out = steps.host(RESTORE)
            if status != 0:
                raise SystemExit(f"the library does not build:\n{out}")
        for i, flags in enumerate(flag_sets):
            say(f"== {unit} {flags}")
            for c in variant_commands(unit, flags):
                status, out = steps.host(c)
                if status != 0:
                    say(f"build failed (status {status}), flag set skipped:\n{out}")
                    break
            else:
                text = runner.gpu(steps.bench_kind(bench_args), f"flags{i}", cmd, env={"RBNN_ALLOW_ABLATION": "1"})
                say("\n".join(ln for ln in text.splitlines() if ln.startswith(("wave", "   "))) if script else steps.bench_line(unit, text))
    finally:
        status, out = steps.host(RESTORE)
        say("library rebuilt without variant flags" if status == 0 else f"RESTORE FAILED: run `python __graft_entry__.py --force`\n{out}")


def run_harness(runner, say, name, flag_sets):
    bindir = os.path.join(tempfile.gettempdir(), "rbnn_harness")
    os.makedirs(bindir, exist_ok=True)
    exes = [os.path.join(bindir, f"{name}_{i}") for i in range(len(flag_sets))]
    src = os.path.join(ROOT, "tools", name + ".hip")
    built = steps.compile_all([[G.HIPCC] + HARNESS_FLAGS + shlex.split(f) + ["-o", e, src] for f, e in zip(flag_sets, exes)])
    for i, (flags, exe, (status, out)) in enumerate(zip(flag_sets, exes, built)):
        say(f"== {flags}   ({exe})")
        say(runner.gpu("harness", f"{name}_{i}", [exe]) if status == 0 else f"build failed (status {status}), skipped:\n{out}")


def main():
    a = sys.argv[1:]
    if len(a) < 2 or a[0] not in ("env", "trees", "flags", "harness"):
        sys.exit(__doc__)
    runner = steps.Runner("ab")
    say = report(os.path.join(runner.out, a[0] + ".txt"))
    if a[0] == "env":
        envs, bench_args = split_dashes(a[2:])
        run_ab(runner, say, env_configs(a[1], envs, bench_args), 2)
    elif a[0] == "trees":
        run_ab(runner, say, tree_configs(a[1], a[3:]), int(a[2]))
    elif a[0] == "flags":
        bench_args, flag_sets = split_dashes(a[2:])
        script = bench_args.pop(bench_args.index("--run") + 1) if "--run" in bench_args else None
        run_flags(runner, say, a[1], script, [w for w in bench_args if w != "--run"], flag_sets)
    else:
        run_harness(runner, say, a[1], a[2:])


if __name__ == "__main__":
    main()
