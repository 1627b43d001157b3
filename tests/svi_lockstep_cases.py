"""Set-ups shared by tests/test_hip_svi_lockstep.py (GPU) and tests/test_svi_lockstep_cpu.py (host): the members of the lockstep runs, and the
fp64 restatement of a member's run that counts its marginal points (no GPU)."""
import torch

import svi_restate as R

MARGIN = 2e-5        # as tests/test_hip_svi_train.py: two largest fp64 mean probabilities this close -> the point may be scored either way
BATCH = 64

# test 1: (arch, act, shape, H, C, [(lr, n, epochs)])
EXACT_CASES = {
    "moons-fc2-32-K3": ("fc2", "leaky", (1, 2, 1), 32, 2, [(0.05, 300, 2), (0.01, 150, 3), (0.05, 64, 1)]),      # last batches 44 / 22, member 2 ends first
    "mnist-fc-128-K2": ("fc", "tanh", (1, 28, 28), 128, 10, [(0.01, 5 * 64 + 17, 1), (0.02, 64 + 1, 2)]),
    "ragged-fc-16-K2": ("fc", "leaky", (1, 17, 1), 16, 3, [(0.01, 100, 1), (0.03, 37, 2)]),                        # ragged N and K; accuracy stack padded to 32
}

# test 2: members 1 and 2 of an epoch_case set-up: the key and lr that replace member 0's
ACC_CASES = {"moons-fc2-32": [(0xC0FFEE1234567 + 1, 0.02), (0x5EED5EED5EED, 0.1)],
             "mnist-fc-16": [(0xC0FFEE1234567 + 1, 0.02), (0x5EED5EED5EED, 0.005)]}


def acc_members(name):
    """The epoch_case set-up `name` as member 0 and the two members derived from it: [(key, lr)]."""
    from test_hip_svi_train import epoch_case
    c = epoch_case(name)
    return c, [(c["key"], c["lr"])] + ACC_CASES[name]


def cpu_marginal_counts(name):
    """Per member and epoch the marginal points of the accuracy forward along the member's own fp64 trajectory (tests/svi_restate.py)."""
    c, members = acc_members(name)
    n, out = c["n"], []
    for key, lr in members:
        r = R.Restatement(c["loc"], c["raw"], c["arch"], c["act"], lr, key, torch.float64)
        per_epoch, t = [], 0
        for _ in range(c["epochs"]):
            m = 0
            for i in range(0, n, BATCH):
                x, lab = c["x"][i:i + BATCH], c["lab"][i:i + BATCH]
                r.step(x, lab)
                _, _, gap = R.accuracy_forward(r.loc, r.raw, c["arch"], c["act"], x, key, t)
                m += int((gap < MARGIN).sum())
                t += 1
            per_epoch.append(m)
        out.append(per_epoch)
    return out
