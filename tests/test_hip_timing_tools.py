"""The measuring functions of the nine tools/*_timing.py programs on the GPU, each called in this process at the smallest size it accepts
with 2 timed blocks: the JSON line has the keys its records have (profiles/*/timing*, profiles/timing_tools/README.txt), every time is finite
and positive, the block count is the one asked for, and lockstep chains are bit-identical to single ones where the tool says so.  No time
is compared."""
import importlib
import json
import math
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tools")]

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("built_library")]

STATS3 = ["median_ms", "min_ms", "max_ms"]
STATS = STATS3 + ["runs"]
STEP = ["ms_per_step", "spread"]
HMC = ["ms_per_transition", "ms_per_leapfrog_step", "chain_transitions_per_s", "spread"]
SVI = ["ms_per_step", "ms_per_epoch_469", "spread"]
LOCK = ["lockstep_member_steps_per_s", "lockstep_spread", "serial_member_steps_per_s", "serial_spread", "lockstep_over_serial"]
NN_M = ["lockstep_ms_per_step", "lockstep_spread", "lockstep_ms_per_member_step", "sequential_ms_per_step", "sequential_spread",
        "sequential_ms_per_member_step", "gain"]
FLOATS = ["entropy", "expected_entropy", "mutual_information", "confidence", "agreement", "variance", "nll", "brier"]
MODE = {"max_abs_diff": FLOATS, "max_abs_diff_same_prediction": FLOATS, "prediction_mismatches": 0, "correct_mismatches": 0}


def nest(flat, **nested):
    return {**{k: 0 for k in flat}, **nested}


# (tool, its measuring function, arguments, the keys of its line: a dict's keys nest, a list is a dict of leaves)
CASES = [
    ("hmc_timing", "measure", (2, 32, 2, 64, 2, 1), {}, nest(["shape", "n_params", "speedup_median"], hip=STATS3, torch_autograd=STATS3)),
    ("hmc_timing", "measure_chains", (2, 32, 2, 64, 2, 2, 1), {},
     nest(["shape", "chains", "serial_chain_transitions_per_s", "lockstep_chain_transitions_per_s", "ratio", "chains_bit_identical"], serial=STATS3, lockstep=STATS3)),
    ("nn_train_timing", "measure", (32, [1, 2], 2, 1, 2), dict(shape=(1, 2, 1), C=2, N=256, B=64, blocks=2),
     nest(["net", "lr", "batch", "steps", "blocks", "nn_train_batch64_ms_per_step", "nn_train_batch64_spread", "torch_autograd_ms_per_member_step",
           "torch_autograd_spread"], **{"M=1": NN_M, "M=2": NN_M})),
    ("svi_train_timing", "measure", (32, 2, 1, 2), dict(shape=(1, 2, 1), C=2, N=256, B=64, blocks=2),
     nest(["net", "lr", "batch", "steps", "blocks", "speedup_no_accuracy"], with_accuracy=SVI, no_accuracy=SVI, torch_autograd_no_accuracy=SVI)),
    ("svi_train_timing", "measure_members", (32, 2, 2), dict(blocks=2),
     nest(["net", "batch", "members", "steps_per_block", "blocks"], with_accuracy=LOCK, no_accuracy=LOCK)),
    ("conv_hmc_timing", "measure", (16, 8, 1, 1), dict(blocks=2),
     nest(["net", "batch", "L", "n_params", "transitions_per_block", "blocks", "launches_per_transition", "torch_over_this"], this=HMC, torch_autograd=HMC)),
    ("conv_hmc_timing", "measure_chains", (16, 2, 8, 1), dict(blocks=2),
     nest(["net", "batch", "L", "n_params", "chains_asked", "chains", "transitions_per_block", "blocks", "launches_per_transition", "lockstep_over_apart"],
          lockstep=HMC, one_after_the_other=HMC)),
    ("conv_svi_train_timing", "measure", (16, 2, 1), dict(B=8, blocks=2),
     nest(["net", "batch", "steps_per_block", "blocks", "torch_over_this_with_accuracy", "torch_over_this_no_accuracy"], with_accuracy=STEP, no_accuracy=STEP,
          torch_autograd_with_accuracy=STEP, torch_autograd_no_accuracy=STEP)),
    ("conv_svi_train_timing", "measure_members", (16, 2, True, 2, 1), dict(B=8, N=64, blocks=2),
     nest(["net", "guides", "batch", "accuracy", "steps_per_block", "blocks", "launches_per_step", "lockstep_over_sequential"],
          lockstep=STEP + ["guide_steps_per_s"], one_after_the_other=STEP + ["guide_steps_per_s"])),
    ("conv_train_timing", "measure", (16, 2, 1), dict(B=8, blocks=2),
     nest(["net", "batch", "steps_per_block", "blocks", "ms_per_step", "spread", "torch_over_this"], torch_autograd=STEP,
          ms_per_entry_point=["forward_and_head", "weight_grads", "adam", "finalize"])),
    ("conv_train_timing", "measure_members", (16, 2, 2, 1), dict(B=8, N=64, blocks=2),
     nest(["net", "members", "batch", "steps_per_block", "blocks", "lockstep_over_sequential"], lockstep=STEP + ["member_steps_per_s"],
          one_after_the_other=STEP + ["member_steps_per_s"])),
    ("chain_diag_timing", "measure", (2, 8, 2, 2), dict(P=37),
     nest(["case", "P", "chains", "draws", "input_bytes", "max_rel_diff_tau_vs_torch", "n_eff_median"], diagnose=STATS, device_copy=STATS, torch_float64=STATS)),
    ("weight_pca_timing", "measure", ("posterior50", 2, 2), dict(rows=3, P=7),
     nest(["case", "P", "host_method", "rows"], fit=STATS, transform_50_rows=STATS, components=STATS, host_fit=STATS, host_transform_50_rows=STATS)),
    ("weight_pca_timing", "measure", ("same150", 2, 2), dict(rows=17, P=4099, prior_rows=8),
     nest(["case", "P", "host_method", "rows"], fit=STATS, transform_50_rows=STATS, components=STATS, transform_prior_1000_rows_with_draw=STATS, host_fit=STATS,
          host_transform_50_rows=STATS)),
    ("weight_pca_timing", "measure", ("prior1000", 2, 2), dict(P=1031, prior_rows=8), nest(["case", "P", "host_method"], fit_with_draw=STATS, host_fit=STATS)),
    ("uncertainty_timing", "time_case", ("fc", 32, 16, 37, 2), {},
     nest(["arch", "hidden", "S", "N", "C", "precision", "P_bytes", "prediction_mismatches_vs_torch"], forward=STATS, uncertainty=STATS,
          uncertainty_8_prefixes=STATS, stats_kernel=STATS, device_copy=STATS, torch_float64=STATS, max_diff_vs_torch=FLOATS)),
    ("uncertainty_timing", "time_case", ("conv", 16, 16, 20, 2), {},
     nest(["arch", "hidden", "S", "N", "C", "precision", "P_bytes", "prediction_mismatches_vs_torch"], forward=STATS, uncertainty=STATS,
          uncertainty_8_prefixes=STATS, stats_kernel=STATS, device_copy=STATS, torch_float64=STATS, max_diff_vs_torch=FLOATS)),
    ("uncertainty_timing", "parity_case", ("fc", 128, 5, 37), {}, nest(["arch", "hidden", "S", "N", "C"], modes={m: MODE for m in ("exact", "triple", "split")})),
]
TIMES = ("ms_per_", "speedup", "ratio", "gain", "_over_")            # with the endings _ms and _per_s: a time, a rate or a ratio of two times


def paths(d, prefix=""):
    """The key paths of a line, nested keys included."""
    if isinstance(d, (list, tuple)):
        d = dict.fromkeys(d)
    out = set()
    for k, v in d.items():
        out |= paths(v, prefix + k + "/") if isinstance(v, (dict, list, tuple)) else {prefix + k}
    return out


@pytest.mark.parametrize("tool, fn, args, kw, keys", CASES, ids=[f"{c[0]}.{c[1]}-{c[2][0]}" for c in CASES])
def test_measuring_function_at_its_smallest_size(tool, fn, args, kw, keys):
    res = json.loads(json.dumps(getattr(importlib.import_module(tool), fn)(*args, **kw)))       # what the child prints
    print(json.dumps(res))
    assert paths(res) == paths(keys)
    flat = {}

    def walk(d, prefix=""):
        for k, v in d.items():
            walk(v, prefix + k + "/") if isinstance(v, dict) else flat.__setitem__(prefix + k, v)
    walk(res)
    times = {k: v for k, v in flat.items() if k.endswith(("_ms", "_per_s")) or any(t in k for t in TIMES)}
    assert (times or fn == "parity_case") and all(isinstance(v, float) and math.isfinite(v) and v > 0 for v in times.values()), times
    assert all(isinstance(v, float) and math.isfinite(v) and v >= 0 for k, v in flat.items() if k.endswith("spread"))
    counts = [v for k, v in flat.items() if k.split("/")[-1] in ("blocks", "runs")]
    assert all(c == 2 for c in counts) and (counts or tool == "hmc_timing" or fn == "parity_case")       # hmc_timing.py's lines name no count
    if "chains_bit_identical" in res:
        assert res["chains_bit_identical"] is True
