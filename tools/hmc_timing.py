"""Per-transition time of HMC on the GPU (robustbnns_amd.hmc.HmcSampler, csrc/rbnn_hmc.hip) against a torch-autograd HMC transition on the
same GPU, at the shapes of the reference's half-moons grid (fc2, hidden 32 / 128 / 512, B = 1024, D = 2) and of saved model_1 (fc2-512,
B = 5000, D = 784).  Both run L = 10 leapfrog steps at a fixed step size with unit mass (the sampling phase: no adaptation, no host reads).
Each figure: median and min..max over --reps blocks of --n transitions, timed with device events after a warm-up transition.  One JSON line
per shape.

    python tools/hmc_timing.py [--reps 7] [--n 20]

--chains K: instead, K chains in lockstep (hmc.LockstepHmc: every launch covers all K) against K consecutive HmcSampler transitions in the
same process, on half-moons fc2-32 and fc2-512 at B = 1024: chain-transitions per second of both and their ratio, one JSON line per shape.

    python tools/hmc_timing.py --chains 8

Every shape is measured in a child process of its own through timing.cases (its log under <OUT>/hmc_timing/).  --child --shape D,H,C,B: the
measuring program itself (what to put behind `rocprofv3 --kernel-trace --stats --`, with --reps 1 --n 1)."""
import argparse

import torch

import timing as T
import torch_baselines as TB

SHAPES = ["2,32,2,1024", "2,128,2,1024", "2,512,2,1024", "784,512,10,5000"]           # D,H,C,B of an fc2 net and its batch
CHAIN_SHAPES = ["2,32,2,1024", "2,512,2,1024"]
L, EPS = 10, 1e-4
DEV = "cuda:0"


def timed(fn, reps, n):
    def block():
        for _ in range(n):
            fn()
    return T.stats(T.blocks(block, reps, warmup=fn), n, runs=False)


def start(D, H, C, B, K):
    """K start positions, then the batch, from one generator."""
    g = torch.Generator().manual_seed(0)
    q0s = [TB.normal_weights(TB.fc2_shapes(D, H, C), 0.1, g) for _ in range(K)]
    return q0s, torch.rand(B, D, generator=g).to(DEV), torch.randint(0, C, (B,), generator=g).to(DEV)


def measure(D, H, C, B, reps, n):
    from robustbnns_amd.hmc import HmcSampler
    (q0,), x, lab = start(D, H, C, B, 1)
    s = HmcSampler("fc2", "leaky", (1, D, 1), C, q0, EPS, L, DEV, 1, adapt_step_size=False, batch_size=B)
    s.stage(x, lab)
    state = {"i": 0}

    def hip_step():
        s.transition(state["i"], L)
        state["i"] += 1

    hip = timed(hip_step, reps, n)
    gen, grad = torch.Generator(device=DEV).manual_seed(0), TB.potential_grad("fc2", x, lab)
    cur = {"s": ({k: v.to(DEV) for k, v in q0.items()}, None)}

    def torch_step():
        cur["s"] = TB.hmc_transition(grad, cur["s"], gen, L, EPS)

    ref = timed(torch_step, reps, n)
    return {"shape": f"fc2 {D}->{H}->{H}->{C} B={B} L={L}", "n_params": s.n_params, "hip": hip, "torch_autograd": ref,
            "speedup_median": ref["median_ms"] / hip["median_ms"]}


def measure_chains(D, H, C, B, K, reps, n):
    """K chains in lockstep against K single chains one after the other: the same L, step size, batch and start positions on both sides."""
    from robustbnns_amd.hmc import HmcSampler, LockstepHmc
    q0s, x, lab = start(D, H, C, B, K)
    singles = [HmcSampler("fc2", "leaky", (1, D, 1), C, q0s[k], EPS, L, DEV, 1 + k, adapt_step_size=False, batch_size=B) for k in range(K)]
    for s in singles:
        s.stage(x, lab)
    ls = LockstepHmc("fc2", "leaky", (1, D, 1), C, q0s, EPS, L, DEV, list(range(1, 1 + K)), adapt_step_size=False, batch_size=B)
    ls.set_data(x, lab)
    ls.stage()
    state = {"i": 0, "j": 0}

    def serial_step():
        for s in singles:
            s.transition(state["i"], L)
        state["i"] += 1

    def lockstep_step():
        ls.transition(state["j"], L)
        state["j"] += 1

    serial, lock = timed(serial_step, reps, n), timed(lockstep_step, reps, n)
    same = all(torch.equal(ls.q_cur[k], singles[k].q_cur) for k in range(K))       # both sides ran the same number of transitions
    tps = lambda t: 1e3 * K / t["median_ms"]
    return {"shape": f"fc2 {D}->{H}->{H}->{C} B={B} L={L}", "chains": K, "serial": serial, "lockstep": lock,
            "serial_chain_transitions_per_s": tps(serial), "lockstep_chain_transitions_per_s": tps(lock),
            "ratio": serial["median_ms"] / lock["median_ms"], "chains_bit_identical": same}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=T.BLOCKS)
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--chains", type=int, default=0, help="K > 0: K chains in lockstep against K consecutive single chains")
    ap.add_argument("--shape", default="", help="D,H,C,B: this shape alone")
    ap.add_argument("--child", action="store_true", help="measure --shape in this process (what the runner starts)")
    a = ap.parse_args(argv)
    if a.child:
        shape = [int(v) for v in a.shape.split(",")]
        return T.child(lambda: measure_chains(*shape, a.chains, a.reps, a.n) if a.chains > 0 else measure(*shape, a.reps, a.n))
    shapes = [a.shape] if a.shape else CHAIN_SHAPES if a.chains > 0 else SHAPES
    T.cases("hmc_timing", __file__, [(("k%d_" % a.chains if a.chains > 0 else "") + s.replace(",", "_"),
                                      ["--shape", s] + T.opts(a, "chains", "reps", "n")) for s in shapes], "hmc_timing")


if __name__ == "__main__":
    main()
