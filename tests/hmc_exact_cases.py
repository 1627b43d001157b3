"""Inputs and closed forms of the exact-property HMC tests (tests/test_hip_hmc_exact.py on the GPU, their CPU tier in tests/test_hmc_cpu.py).
Nothing here is taken from tests/hmc_restate.py: the closed forms are numpy fp64 written from the mathematics, so a mistake shared by the
restatement and the kernels is not shared by them.

The one-class net.  A net with ONE class has CE = logsumexp(z) - z_0 = 0 for every q and every point: the head's label-class gradient is
-sum_{k != y} e_k / den = -0, so dCE/dW is exactly zero, U(q) = 1/2 |q|^2 and the posterior is exactly N(0, I).  With a diagonal inverse mass
m a leapfrog step is then linear and separate in every coordinate, a harmonic oscillator with omega^2 = m_i:
    (q, r) -> Kick . Drift . Kick (q, r),   Kick = [[1, 0], [-eps/2, 1]],   Drift = [[1, eps m_i], [0, 1]],
and L steps are the L-th power of that 2 x 2 matrix (stable while eps sqrt(m_i) < 2)."""
import numpy as np
import torch

import svi_restate as R

H, EPS = 16, 0.25                        # eps sqrt(max m_inv) = 0.5: well inside the stability limit 2
M_VALUES = (0.25, 1.0, 4.0)


def one_class_case(arch, seed=0):
    """arch 2 -> 16 (-> 16) -> 1, tanh (fc: 65 parameters, fc2: 337), 8 points with label 0, a position ~ N(0, I), the hand-set inverse mass
    (0.25, 1, 4, 0.25, ... over the flat parameter vector) and a momentum r = N(0, 1) / sqrt(m_inv) — all fp32 values."""
    g = torch.Generator().manual_seed(seed)
    shapes = R.shapes_of(arch, 2, H, 1)
    q0 = {k: torch.randn(*s, generator=g) for k, s in shapes.items()}
    n = sum(int(np.prod(s)) for s in shapes.values())
    m_inv = torch.tensor(M_VALUES).repeat(-(-n // 3))[:n].clone()
    return {"shapes": shapes, "q0": q0, "n": n, "x": torch.randn(8, 2, generator=g), "lab": torch.zeros(8, dtype=torch.long), "m_inv": m_inv,
            "r0": torch.randn(n, generator=g) / m_inv.sqrt()}


def leapfrog_closed_form(q, r, m_inv, eps, L):
    """(q', r', K', 1/2 sum q'^2) after L leapfrog steps of U = 1/2 |q|^2 under the diagonal inverse mass m_inv, in numpy fp64."""
    q, r, m = (np.asarray(v, dtype=np.float64) for v in (q, r, m_inv))
    kick = np.array([[1.0, 0.0], [-0.5 * eps, 1.0]])
    step = np.empty((m.size, 2, 2))
    for i, mi in enumerate(m):
        step[i] = kick @ np.array([[1.0, eps * mi], [0.0, 1.0]]) @ kick
    out = np.einsum("nij,nj->ni", np.linalg.matrix_power(step, L), np.stack([q, r], 1))
    q1, r1 = out[:, 0], out[:, 1]
    return q1, r1, 0.5 * float(np.sum(m * r1 * r1)), 0.5 * float(np.sum(q1 * q1))


def stationary_starts(K=16, seed=1):
    """K exact N(0, I) draws over the fc one-class net's parameters from a seeded CPU generator: the chain's stationary law."""
    g = torch.Generator().manual_seed(seed)
    shapes = R.shapes_of("fc", 2, H, 1)
    return [{k: torch.randn(*s, generator=g) for k, s in shapes.items()} for _ in range(K)]


STATIONARY_KEYS = tuple(range(700, 716))

# Adaptation on the one-class net: 16 chains from Uniform(-2, 2), keys 900 ... 915, step size 0.1, num_steps 10, 150 warmup transitions
# (windows [0, 75) start, [75, 100) middle, [100, 150) end), 200 samples.
ADAPT = {"step_size": 0.1, "num_steps": 10, "warmup": 150, "samples": 200, "keys": tuple(range(900, 916)), "accept": (0.7, 0.98), "q2": 0.05}


def adapt_starts(K=16):
    """Chain k's start: Uniform(-2, 2) key by key in state_dict order from torch's CPU generator seeded with its key (as initial_position)."""
    shapes = R.shapes_of("fc", 2, H, 1)
    out = []
    for key in ADAPT["keys"][:K]:
        g = torch.Generator().manual_seed(key)
        out.append({k: (torch.rand(*s, generator=g) * 2 - 1) * 2.0 for k, s in shapes.items()})
    return out


def welford_rows(n_rows=300, n=65, seed=5):
    """Rows q_t = 1000 + 0.01 N(0, 1) in fp32: the mean is 1e5 standard deviations from zero, where an fp32 sum of squares loses everything."""
    g = torch.Generator().manual_seed(seed)
    return (1000.0 + 0.01 * torch.randn(n_rows, n, generator=g, dtype=torch.float64)).float()


def welford_reference(rows):
    """fp64 two-pass mean and M2 of the (fp32) rows and the window end's m_inv = (n / (n + 5)) M2 / (n - 1) + 1e-3 * 5 / (n + 5)."""
    v = rows.double().numpy()
    n = v.shape[0]
    mean = v.mean(0)
    m2 = ((v - mean) ** 2).sum(0)
    return mean, m2, (n / (n + 5.0)) * m2 / (n - 1.0) + 1e-3 * 5.0 / (n + 5.0)
