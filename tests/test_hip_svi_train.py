"""GPU tests (-m gpu) of SVI training (model_bnn.py:105-136, :303-365; csrc/rbnn_train.hip, robustbnns_amd/svi_train.py): the weight
gradients and the step loss against fp64 autograd on the oracle's draw, the Adam kernel against torch.optim.Adam, 20-step trajectories
against the CPU restatement (tests/svi_restate.py), BNN.train end to end, reproducibility, the param-store round trip, no device->host
sync inside a step, and the guards; whole epochs with a short last batch (the loss, the accuracy forward's Psum and the counters after EVERY
step against fp64 at the GPU's own parameters), BNN.train's history and printed line against a hand-driven trainer, and what the training
entry points must not read (NaN behind every bound).  Every new check prints one line: worst error in units of its bar, what was excluded."""
import ctypes as C
import random

import pytest
import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader, TensorDataset

import svi_restate as R
from conftest import rel_err_points
from oracle import bnn_oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("built_library")]
DEV = "cuda:0"
KINK = 2e-6          # points with a hidden pre-activation this close to 0 are excluded: act' jumps there (oracle.kink_margin)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"


def _guide(arch, D, H, Cn, seed, std):
    g = torch.Generator().manual_seed(seed)
    shapes = R.shapes_of(arch, D, H, Cn)
    loc = {k: std * torch.randn(*s, generator=g) for k, s in shapes.items()}
    raw = {k: -3.0 + 0.5 * torch.randn(*s, generator=g) for k, s in shapes.items()}
    return shapes, loc, raw


GRAD_CASES = [("fc", "leaky", (1, 28, 28), 128, 10, 128), ("fc", "relu", (1, 28, 28), 512, 10, 128), ("fc", "leaky", (1, 28, 28), 16, 10, 128),
              ("fc2", "tanh", (1, 28, 28), 256, 10, 128), ("fc2", "sigm", (1, 2, 1), 32, 2, 128), ("fc2", "leaky", (1, 28, 28), 128, 10, 37),
              # the edges of train_gemm_kernel / train_head_kernel: a partial 64-tile beside a full one (H = 96, 160), H = 1024, D % 16 != 0 (10, 17),
              # D = 3072, C = 1 and C = 16 (the ABI's limits), B = 1, 3 (one partly filled head block), 65, 300 (K loop of the weight gradients longer
              # than 16 stages), the ones column in a tile of its own (N + 1 = 65, 1025), fc + sigm, fc2 + relu
              ("fc", "sigm", (1, 28, 28), 96, 10, 65), ("fc2", "relu", (1, 28, 28), 160, 10, 300), ("fc", "leaky", (1, 28, 28), 1024, 10, 128),
              ("fc2", "tanh", (1, 28, 28), 1024, 10, 65), ("fc", "leaky", (1, 5, 2), 96, 2, 65), ("fc2", "tanh", (1, 5, 2), 32, 3, 128),
              ("fc", "tanh", (1, 17, 1), 160, 10, 3), ("fc2", "leaky", (1, 17, 1), 96, 10, 65),            # the latter: H % 64, D % 16, B % 64 all != 0
              ("fc", "relu", (3, 32, 32), 128, 10, 65), ("fc2", "sigm", (3, 32, 32), 96, 10, 37),
              ("fc", "leaky", (1, 28, 28), 32, 1, 65), ("fc", "tanh", (1, 28, 28), 64, 16, 65), ("fc2", "leaky", (1, 28, 28), 128, 16, 300),
              ("fc2", "sigm", (1, 28, 28), 64, 10, 1), ("fc", "leaky", (1, 28, 28), 128, 10, 1), ("fc2", "relu", (1, 17, 1), 32, 10, 3),
              ("fc", "leaky", (1, 5, 2), 96, 2, 300)]
# what a case changes of the defaults.  std: of the guide's loc (default 0.05, 0.5 at D <= 16); fit: the labels of three points in four are the
# fp64 prediction at the draw.  The last case: fitted labels and weights scaled so that a third of the points are confidently classified (CE < 1e-3:
# log1pf(rest) against the cancellation of logf(den) - 0).  There CE = e^-gap, so its RELATIVE error is the ABSOLUTE error of the logit gap, about
# 1e-7 |z| per fp32 dot product in front of it: a 784 -> 128 -> 10 net that classifies this confidently has |z| up to 50 and leaves torch's own fp32
# evaluation beyond 1e-5 of CE (measured on the CPU), so the case is a 10 -> 96 -> 2 net (|z| <= 18, gap >= 7 suffices with two classes).
GRAD_OPTS = {("fc", "leaky", (1, 5, 2), 96, 2, 300): {"std": 0.35, "fit": True}}
CONFIDENT = 1e-3


def grad_case(arch, act, shape, H, Cn, B):
    """The inputs of one GRAD_CASES case, from the oracle alone (no GPU): the guide, the batch, the draw's fp64 weights and logits, the points
    outside the kink margin, and which of them take the head kernel's log1pf branch (label = argmax of the logits)."""
    opt = GRAD_OPTS.get((arch, act, shape, H, Cn, B), {})
    D = shape[0] * shape[1] * shape[2]
    shapes, loc, raw = _guide(arch, D, H, Cn, seed=H + B, std=opt.get("std", 0.05 if D > 16 else 0.5))
    x, y = O.synthetic_inputs(B, shape, Cn, seed=B)
    if D <= 16:
        x = 4 * x - 2
    lab = y.argmax(-1)
    eps = R.draw_eps(shapes, arch, GRAD_KEY, GRAD_DRAW)
    W64 = {k: loc[k].double() + F.softplus(raw[k].double()) * eps[k][0] for k in shapes}
    stacked = {k: v[None] for k, v in W64.items()}
    ok = O.kink_margin(x.double(), stacked, arch, act, 1) > KINK
    z = O.nn_logits(x.double(), stacked, arch, act)[0]
    if opt.get("fit"):
        lab = torch.where(torch.arange(B) % 4 != 0, z.argmax(-1), lab)
    ce = torch.logsumexp(z, -1) - z.gather(1, lab[:, None])[:, 0]
    on_log1p = z.gather(1, lab[:, None])[:, 0] == z.max(-1)[0]
    return {"D": D, "shapes": shapes, "loc": loc, "raw": raw, "x": x, "lab": lab, "W64": W64, "ok": ok, "ce": ce[ok], "log1p": on_log1p[ok],
            "confident": bool(opt.get("fit"))}


GRAD_KEY, GRAD_DRAW = 0x0123456789ABCDEF, 5


@pytest.mark.parametrize("arch,act,shape,H,Cn,B", GRAD_CASES)
def test_weight_gradients_and_step_loss_match_fp64_autograd(arch, act, shape, H, Cn, B):
    """Also the per-point CE (ws_t["ce"]) against fp64 logsumexp(z) - z_y: absolute error <= 1e-5 max(1, CE), so that both branches of the head
    kernel's CE are held on their own; in the confident case the points on the log1pf branch are held to 1e-5 RELATIVE to their CE."""
    from robustbnns_amd.svi_train import SviTrainer
    c = grad_case(arch, act, shape, H, Cn, B)
    D, shapes, loc, raw, W64, ok = c["D"], c["shapes"], c["loc"], c["raw"], c["W64"], c["ok"]
    key, draw = GRAD_KEY, GRAD_DRAW
    print(f"[{arch} {D}->{H}->{Cn} {act} B={B}] points within the kink margin: {int((~ok).sum())}")
    assert int((~ok).sum()) <= 0.01 * B
    x, lab = c["x"][ok], c["lab"][ok]
    n = int(x.shape[0])
    Wg = {k: v.clone().requires_grad_(True) for k, v in W64.items()}
    ce64, _ = R.ce_grads(x.reshape(x.shape[0], -1).double(), lab, Wg, arch, act)
    ce64.backward()
    tr = SviTrainer(arch, act, shape, Cn, loc, raw, 0.01, DEV, key, batch_size=64)       # smaller than B: the workspaces grow
    tr.t = draw
    tr.gradients(x.to(DEV), lab.to(DEV))
    torch.cuda.synchronize()
    W, G = tr.unflat(tr.W), tr.unflat(tr.grad)
    worst = 0.0
    for k in shapes:
        ew = float((W[k].cpu().double() - W64[k]).abs().max() / (W64[k].abs().max()))
        g64 = Wg[k].grad
        gmax = float(g64.abs().max())
        err = float((G[k].cpu().double() - g64).abs().max())
        print(f"   {k}: draw rel err {ew:.1e}  max|dW - fp64| = {err:.2e} = {err / max(gmax, 1e-300):.1e} max|dW|")
        assert ew < 2e-6, k
        assert err <= 1e-5 * gmax, k                  # C = 1: the gradient is exactly zero, and so must the kernel's be
        worst = max(worst, err / (1e-5 * gmax) if gmax else 0.0)
    # the per-point CE, each branch on its own
    ce_gpu = tr.ws_t["ce"][:n].cpu().double()
    e_ce = (ce_gpu - c["ce"]).abs()
    bar = 1e-5 * c["ce"].clamp_min(1.0)
    n_log1p, n_conf = int(c["log1p"].sum()), int((c["log1p"] & (c["ce"] < CONFIDENT)).sum())
    if c["confident"]:
        bar = torch.where(c["log1p"], 1e-5 * c["ce"], bar)
        assert n_conf >= n // 4, (n_conf, n)
    w = {name: float((e_ce / bar)[m].max()) if bool(m.any()) else 0.0 for name, m in (("log1p", c["log1p"]), ("log", ~c["log1p"]))}
    print(f"   per-point CE: worst {w['log1p']:.3f} x bar on the log1pf branch ({n_log1p} points, {n_conf} with CE < {CONFIDENT:g}"
          f"{', bar 1e-5 x CE' if c['confident'] else ''}), {w['log']:.3f} x bar on the logf branch ({n - n_log1p} points)")
    assert bool((e_ce <= bar).all()), f"per-point CE: worst {max(w.values()):.2f} x its bar"
    if Cn > 1 and B >= 65:
        assert 0 < n_log1p < n, "both branches of the head kernel's CE must be met"
    # the reported step loss: sum CE + KL of the pre-update guide, same draw
    tr.t = draw
    tr.step(x.to(DEV), lab.to(DEV), accuracy=False)
    loss = float(tr.stats[0])
    ref = float(ce64.detach()) + float(R.kl({k: v.double() for k, v in loc.items()}, {k: v.double() for k, v in raw.items()}))
    print(f"   step loss {loss:.8e}  fp64 {ref:.8e}  rel {abs(loss - ref) / abs(ref):.1e}")
    assert abs(loss - ref) <= 1e-5 * abs(ref)
    print(f"[svi-train grad {arch} {D}->{H}->{Cn} {act} B={B}] worst gradient error {worst:.3f} x (1e-5 max|fp64 gradient|); per-point CE "
          f"{max(w.values()):.3f} x bar; step loss {abs(loss - ref) / abs(ref) / 1e-5:.3f} x 1e-5; excluded: kink {int((~ok).sum())} of {B} points")


# The far-end inputs' seeds.  m_raw's scale |g_raw| + |m_raw| does not bound the OPERANDS of g_raw = (grad eps + sigma - 1/sigma) sigmoid(raw): at an
# element where grad eps cancels 1/sigma - sigma and m_raw is small too, the 2^-21 of the regenerated eps is no longer small against it.  The
# ratio operands / scale is at most 180 over the elements of the t = 1, 2, 10 inputs; seed 100 + t gives 649 at t = 1000 and 1654 at t = 10^7
# (there the fp64 comparison itself is ill-posed at that one element: 7.1e-6 x scale measured), so the far-end seeds are the first after 100 + t
# that keep the ratio under 300 (270, 228, 138), which the test asserts of its inputs.
ADAM_SEED = {1000: 1101, 100000: 100100, 10 ** 7: 10 ** 7 + 101}


@pytest.mark.parametrize("t", [1, 2, 10, 1000, 100000, 10 ** 7])
def test_adam_step_kernel_matches_torch_optim_adam(t):
    """Tolerance: every output is a chain of at most ~10 fp32 operations (2^-24 relative rounding each) on operands bounded by the scale
    named below, and the regenerated eps carries the hardware log / sin (about 2^-21 relative): 2e-6 x scale bounds each result.
    t >= 1000 (the far end: beta1^t and then beta2^t vanish from the bias corrections) also carries, in the first 1800 elements, raw in
    [15, 25] (both sides of softplus's threshold 20), raw in [-12, -6], and dead elements with grad = m = v = loc = 0 (eps_adam alone in the
    denominator of loc's update: the update is exactly 0; a scale of 0 admits no error at all).
    The KL sum: every element's term is >= 0 and is a chain of ~4 fp32 operations on operands bounded by M = |log sigma| + (sigma^2 + loc^2) / 2
    + 1/2, and the block's tree sum adds 8 levels + 3 of the thread's own: at most ~16 x 2^-24 sum M ~ 1e-6 sum M.  sum M <= 10 KL is
    asserted of the inputs (the wide raw range: ~1.0, the terms are dominated by sigma^2 / 2 and -log sigma), so 1e-5 |KL| bounds the sum."""
    from robustbnns_amd import _hip
    from robustbnns_amd.svi_train import ADAM_EPS, BETAS, SviTrainer
    arch, D, H, Cn, lr, key, draw = "fc2", 20, 64, 5, 0.01, 0xFEEDFACE12345678, 17
    shapes, loc, raw = _guide(arch, D, H, Cn, seed=t, std=0.3)
    tr = SviTrainer(arch, "leaky", (1, D, 1), Cn, loc, raw, lr, DEV, key, batch_size=8)
    g = torch.Generator().manual_seed(ADAM_SEED.get(t, 100 + t))
    n = tr.n_params
    raw_f = torch.randn(n, generator=g) - 1.0
    vals = {"loc": torch.randn(n, generator=g), "raw": raw_f, "grad": torch.randn(n, generator=g) * 3}
    for p in ("loc", "raw"):
        m = 0.2 * torch.randn(n, generator=g)
        vals["m_" + p], vals["v_" + p] = m, (m.abs() + torch.rand(n, generator=g)) ** 2
    if t >= 1000:
        raw_f[:600] = 15.0 + 10.0 * torch.rand(600, generator=g)
        raw_f[600:1200] = -12.0 + 6.0 * torch.rand(600, generator=g)
        raw_f[0], raw_f[1], raw_f[2], raw_f[600] = 20.0, 19.999998, 20.000002, -12.0
        for v in vals.values():
            if v is not raw_f:
                v[1200:1800] = 0.0
    for name, v in vals.items():
        getattr(tr, name).copy_(v)
    tr.sigma.copy_(F.softplus(raw_f.to(DEV)))
    sig32 = tr.sigma.cpu().double()
    _hip.check(tr.k.lib.rbnn_svi_adam_step(C.byref(tr.net), C.c_uint64(key), C.c_uint32(draw), t, lr, BETAS[0], BETAS[1], ADAM_EPS,
                                           _hip.ptr(tr.kl_part), _hip.stream_of(tr.loc)), "rbnn_svi_adam_step")
    torch.cuda.synchronize()
    eps = torch.cat([v[0].reshape(-1) for v in R.draw_eps(shapes, arch, key, draw).values()])
    d = {k: v.double() for k, v in vals.items()}
    sig = F.softplus(d["raw"])
    g_loc = d["grad"] + d["loc"]
    g_raw = (d["grad"] * eps + sig - 1 / sig) * torch.sigmoid(d["raw"])
    if t >= 1000:
        operands = ((d["grad"] * eps).abs() + sig + 1 / sig) * torch.sigmoid(d["raw"])
        assert float((operands / (g_raw.abs() + d["m_raw"].abs())).max()) <= 300
    out = {}
    for p, gr in (("loc", g_loc), ("raw", g_raw)):
        w = d[p].clone().requires_grad_(True)
        opt = torch.optim.Adam([w], lr=lr)
        opt.state[w] = {"step": torch.tensor(float(t - 1)), "exp_avg": d["m_" + p].clone(), "exp_avg_sq": d["v_" + p].clone()}
        w.grad = gr.clone()
        opt.step()
        out[p], out["m_" + p], out["v_" + p] = w.detach(), opt.state[w]["exp_avg"], opt.state[w]["exp_avg_sq"]
        gs = gr.abs() + d["m_" + p].abs()
        step_size = lr / (1 - BETAS[0] ** t)
        scale = {p: d[p].abs() + step_size * (1 + out["m_" + p].abs() / (out["v_" + p].sqrt() / (1 - BETAS[1] ** t) ** 0.5 + ADAM_EPS)),
                 "m_" + p: gs, "v_" + p: d["v_" + p] + gr * gr}
        for name, sc in scale.items():
            got = getattr(tr, name).cpu().double()
            assert bool(torch.isfinite(got).all()), name
            diff = (got - out[name]).abs()
            err = torch.where(sc > 0, diff / sc.clamp_min(1e-300), torch.where(diff == 0, 0.0, float("inf"))).max()
            print(f"t={t} {name}: max |err| / scale = {float(err):.2e}")
            assert float(err) <= 2e-6, name
    sig_new = F.softplus(out["raw"])
    err = ((tr.sigma.cpu().double() - sig_new).abs() / (sig_new + torch.sigmoid(out["raw"]) * (out["raw"].abs() + lr))).max()
    print(f"t={t} sigma: max |err| / scale = {float(err):.2e}")
    assert float(err) <= 2e-6
    kl = float(((-torch.log(sig32) + 0.5 * (sig32 ** 2 + d["loc"] ** 2)) - 0.5).sum())
    mag = float((torch.log(sig32).abs() + 0.5 * (sig32 ** 2 + d["loc"] ** 2) + 0.5).sum())
    e_kl = abs(float(tr.kl_part.double().sum()) - kl)
    print(f"[svi-train adam t={t}] KL partial sums: {e_kl / (1e-5 * abs(kl)):.3f} x (1e-5 |KL|); sum of operand magnitudes {mag / kl:.2f} KL; excluded: nothing")
    assert mag <= 10 * kl
    assert e_kl <= 1e-5 * abs(kl)


# max |theta_fp32 - theta_fp64| of loc / raw after these 20 steps of the CPU restatement itself (tests/svi_restate.py, measured on the CPU
# with this exact setup: fp32 and fp64 runs from the same init and the same eps)
TRAJ_CASES = [("moons", "fc2", "leaky", (1, 2, 1), 32, 2, 32, 1.07e-6), ("mnist", "fc", "tanh", (1, 28, 28), 128, 10, 64, 1.44e-4)]


@pytest.mark.parametrize("name,arch,act,shape,H,Cn,B,spread", TRAJ_CASES)
def test_twenty_steps_follow_the_fp64_restatement(name, arch, act, shape, H, Cn, B, spread):
    from robustbnns_amd.model_bnn import set_rng_seed
    from robustbnns_amd.svi_train import SviTrainer, initial_params
    D = shape[0] * shape[1] * shape[2]
    if name == "moons":
        x, y = R.two_moons(20 * B, 0.1, seed=5)
    else:
        x, y = O.synthetic_inputs(20 * B, shape, Cn, seed=11)
    set_rng_seed(0)
    loc, raw = initial_params(list(R.shapes_of(arch, D, H, Cn).items()))
    key, lr = 0x5EED, 0.01
    r64 = R.Restatement(loc, raw, arch, act, lr, key, torch.float64)
    tr = SviTrainer(arch, act, shape, Cn, loc, raw, lr, DEV, key, batch_size=B)
    xd, yd = x.to(DEV), y.argmax(-1).to(DEV)
    for i in range(20):
        r64.step(x[i * B:(i + 1) * B], y[i * B:(i + 1) * B].argmax(-1))
        tr.step(xd[i * B:(i + 1) * B], yd[i * B:(i + 1) * B])
    gl, gr = tr.params()
    dl = max(float((gl[k].cpu().double() - r64.loc[k]).abs().max()) for k in r64.loc)
    dr = max(float((gr[k].cpu().double() - r64.raw[k]).abs().max()) for k in r64.loc)
    print(f"[{name}] after 20 steps: max |loc - fp64| {dl:.2e}  max |raw - fp64| {dr:.2e}  (fp32-vs-fp64 spread of the restatement {spread:.2e})")
    assert dl <= 10 * spread and dr <= 10 * spread


def _moons_bnn(epochs, lr=0.05):
    from robustbnns_amd.model_bnn import BNN
    return BNN("half_moons", 32, "leaky", "fc2", "svi", epochs, lr, None, None, (1, 2, 1), 2)


def _moons_loader(n, seed, batch=64):
    x, y = R.two_moons(n, 0.1, seed)
    return DataLoader(TensorDataset(x, y), batch_size=batch, shuffle=False)


# ------------------------------------------------------------------ whole epochs, with a short last batch
MARGIN = 2e-5        # a point whose two largest fp64 mean probabilities are this close may be scored either way (each moves by the 1e-5 forward bar)
EPOCH_CASES = ["moons-fc2-32", "mnist-fc-128", "mnist-fc-16"]


def epoch_case(name):
    """Data, guide and settings of one EPOCH_CASES set-up (no GPU): n points in batches of 64 with a short last batch."""
    if name == "moons-fc2-32":
        arch, act, shape, H, Cn, n, lr, std = "fc2", "leaky", (1, 2, 1), 32, 2, 300, 0.05, 0.5          # last batch 44
        x, y = R.two_moons(n, 0.1, seed=7)
    else:
        arch, act, shape, Cn, lr, std = "fc", "tanh" if name == "mnist-fc-128" else "leaky", (1, 28, 28), 10, 0.01, 0.05
        H, n = (128, 5 * 64 + 17) if name == "mnist-fc-128" else (16, 2 * 64 + 22)       # H = 16: the accuracy stack is padded to 32 hidden units
        x, y = O.synthetic_inputs(n, shape, Cn, seed=21)
    D = shape[0] * shape[1] * shape[2]
    _, loc, raw = _guide(arch, D, H, Cn, seed=n + H, std=std)
    return {"arch": arch, "act": act, "shape": shape, "H": H, "Cn": Cn, "n": n, "lr": lr, "x": x, "lab": y.argmax(-1), "loc": loc, "raw": raw,
            "key": 0xC0FFEE1234567, "batch": 64, "epochs": 2}


def accuracy_bounds(psum, pred, gap, lab):
    """(c_safe, n_marginal) of one accuracy forward in fp64: the correct points among those that are not marginal, and the marginal ones."""
    marginal = gap < MARGIN
    return int(((pred == lab) & ~marginal).sum()), int(marginal.sum())


@pytest.mark.parametrize("name", EPOCH_CASES)
def test_every_step_of_two_epochs_with_a_short_last_batch(name):
    """After EVERY step, at the parameters read back from the GPU: Psum[:B] against the fp64 accuracy forward of the updated guide (1e-5 per
    point), the increment of stats[2] within [c_safe, c_safe + n_marginal], stats[0] against the fp64 loss at the GPU's own pre-update
    parameters (1e-5 relative: no trajectory drift in the comparison), stats[1] = the running sum of the stats[0] read back, and begin_epoch()."""
    from robustbnns_amd.svi_train import SviTrainer
    c = epoch_case(name)
    arch, act, n, bs = c["arch"], c["act"], c["n"], c["batch"]
    tr = SviTrainer(arch, act, c["shape"], c["Cn"], c["loc"], c["raw"], c["lr"], DEV, c["key"], batch_size=bs)
    xd, yd = c["x"].to(DEV), c["lab"].to(DEV)
    read = lambda: tuple({k: v.cpu().double() for k, v in d.items()} for d in tr.params())
    w_psum = w_loss = 0.0
    marginal_total, steps = 0, 0
    for epoch in range(c["epochs"]):
        tr.begin_epoch()
        running, correct_before, marginal_epoch = 0.0, 0.0, 0
        for i in range(0, n, bs):
            x, lab = c["x"][i:i + bs], c["lab"][i:i + bs]
            B, t = int(x.shape[0]), tr.t
            loc0, raw0 = read()
            tr.step(xd[i:i + bs], yd[i:i + bs])
            loc1, raw1 = read()
            stats, psum = tr.stats.tolist(), tr.Psum[:B, :c["Cn"]].cpu().double()
            # the loss of the step: CE at the draw of step t + KL, both of the PRE-update guide
            eps = {k: v[0] for k, v in R.draw_eps(tr.shapes, arch, c["key"], t).items()}
            loss64 = float(R.step_gradients(loc0, raw0, eps, x.reshape(B, -1).double(), lab, arch, act)[0])
            e_loss = abs(stats[0] - loss64) / abs(loss64)
            assert e_loss <= 1e-5, (epoch, i, stats[0], loss64)
            running += stats[0]
            assert abs(stats[1] - running) <= 2.0 ** -50 * abs(running), (epoch, i, stats[1], running)
            # the accuracy forward of the UPDATED guide
            psum64, pred, gap = R.accuracy_forward(loc1, raw1, arch, act, x, c["key"], t)
            e_psum = float(rel_err_points(psum, psum64).max())
            assert e_psum <= 1e-5, (epoch, i, e_psum)
            c_safe, n_marg = accuracy_bounds(psum64, pred, gap, lab)
            got = stats[2] - correct_before
            assert c_safe <= got <= c_safe + n_marg and got == int(got), (epoch, i, got, c_safe, n_marg)
            correct_before = stats[2]
            marginal_epoch += n_marg
            w_psum, w_loss, steps = max(w_psum, e_psum / 1e-5), max(w_loss, e_loss / 1e-5), steps + 1
        assert marginal_epoch <= 0.01 * n, marginal_epoch
        marginal_total += marginal_epoch
        last = tr.stats.tolist()
        assert tr.epoch_totals() == (last[1], last[2]) and last[2] == correct_before
        tr.begin_epoch()
        assert tr.stats.tolist() == [last[0], 0.0, 0.0]
    print(f"[svi-train epochs {name}] {steps} steps, last batch of {n % bs}: Psum worst {w_psum:.3f} x 1e-5, step loss worst {w_loss:.3f} x 1e-5, stats[1] = "
          f"the running sum; excluded from the exact count: {marginal_total} marginal points of {c['epochs'] * n}")


# relative |fp32 - fp64| of the epoch losses of the CPU restatement itself on this run (tests/svi_restate.py, same init and eps; measured on the
# CPU by tests/test_svi_train_cpu.py::test_history_case_spread_is_the_measured_one): the GPU's epoch losses are allowed 10x that
HISTORY_CASE = {"n": 300, "seed": 6, "batch": 64, "epochs": 2, "lr": 0.05, "spread": 2.63e-8}


def history_restatements(dtypes):
    """The run of test_bnn_train_history_... on the CPU: BNN.train's seed, init and key, the restatement in every dtype asked for.  Returns the
    epoch losses per dtype."""
    from robustbnns_amd.model_bnn import set_rng_seed
    from robustbnns_amd.svi_train import draw_key, initial_params
    h = HISTORY_CASE
    train = _moons_loader(h["n"], h["seed"], h["batch"])
    random.seed(0)
    set_rng_seed(0)
    iter(train)                                   # see test_bnn_train_end_to_end_matches_the_cpu_restatement
    loc, raw = initial_params(list(R.shapes_of("fc2", 2, 32, 2).items()))
    key = draw_key()
    out = {}
    for dt in dtypes:
        r = R.Restatement(loc, raw, "fc2", "leaky", h["lr"], key, dt, record=True)
        for _ in range(h["epochs"]):
            for xb, yb in train:
                r.step(xb, yb.argmax(-1))
        per = len(train)
        out[dt] = [sum(r.losses[e * per:(e + 1) * per]) for e in range(h["epochs"])]
    return out


def test_bnn_train_history_and_epoch_line_are_the_trainers_counters(tmp_path, capsys):
    """training_history and the printed line against a second, hand-driven SviTrainer from the same seed / init / key (bit-equal: the same kernels
    in the same order), with n = len(dataset) = 300, not 5 batches x 64; the epoch losses against the fp64 restatement at the measured bar."""
    from robustbnns_amd.model_bnn import set_rng_seed
    from robustbnns_amd.svi_train import SviTrainer, draw_key, initial_params
    h = HISTORY_CASE
    n, epochs = h["n"], h["epochs"]
    train = _moons_loader(n, h["seed"], h["batch"])
    assert n % h["batch"] and len(train) * h["batch"] != n
    bnn = _moons_bnn(epochs, h["lr"])
    bnn.train(train, DEV, str(tmp_path) + "/")
    out = capsys.readouterr().out
    random.seed(0)
    set_rng_seed(0)
    iter(train)
    loc, raw = initial_params([(k, tuple(v.shape)) for k, v in bnn.basenet.state_dict().items()])
    tr = SviTrainer("fc2", "leaky", (1, 2, 1), 2, loc, raw, h["lr"], DEV, draw_key(), batch_size=h["batch"])
    losses = []
    for e in range(epochs):
        tr.begin_epoch()
        for xb, yb in train:
            tr.step(xb.to(DEV), yb.to(DEV).argmax(-1))
        loss, correct = tr.epoch_totals()
        assert correct == int(correct) and 0 <= correct <= n
        assert bnn.training_history["loss"][e] == loss
        assert bnn.training_history["accuracy"][e] == 100 * correct / n
        line = f"[Epoch {e + 1}]\t loss: {loss / n:.2f} \t accuracy: {100 * correct / n:.2f}"
        assert line in out, (line, out)
        losses.append(loss)
    assert len(bnn.training_history["loss"]) == len(bnn.training_history["accuracy"]) == epochs
    gl, gr = tr.params()
    for k in gl:
        assert torch.equal(gl[k], bnn.svi_loc[k].to(DEV)) and torch.equal(gr[k], bnn.svi_scale[k].to(DEV)), k
    ref = history_restatements([torch.float64])[torch.float64]
    worst = max(abs(a - b) / abs(b) for a, b in zip(losses, ref))
    print(f"[svi-train history] epoch losses GPU {losses}  fp64 restatement {ref}: worst relative difference {worst:.2e} = "
          f"{worst / (10 * h['spread']):.3f} x (10 x the restatement's own fp32-vs-fp64 spread {h['spread']:.2e}); excluded: nothing")
    assert worst <= 10 * h["spread"]


# ------------------------------------------------------------------ what must not be read
def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _poisoned_step(arch, D, Cn, B, poison, accuracy):
    """One step of a fresh trainer on B < Bmax points; poison: NaN in everything the entry points have no business reading (rows >= B of every
    workspace, of X and of Psum; columns [D, Dp) of X[:B] unless the accuracy forward runs: rbnn_fc_forward is documented to read zero columns
    there), labels[B:] = a class >= C.  Returns the bit patterns of every result."""
    from robustbnns_amd.svi_train import SviTrainer
    shape, H = (1, D, 1), 32
    shapes, loc, raw = _guide(arch, D, H, Cn, seed=D + B, std=0.5)
    x, y = O.synthetic_inputs(B, shape, Cn, seed=D)
    tr = SviTrainer(arch, "leaky", shape, Cn, loc, raw, 0.01, DEV, 0xBADC0DE, batch_size=64)
    assert B < tr.Bmax and B % 4 and tr.Dp > D
    if poison:
        nan = float("nan")
        for v in tr.ws_t.values():
            v[B:] = nan
        tr.X[B:] = nan
        tr.Psum[B:] = nan
        if not accuracy:
            tr.X[:B, D:] = nan
        tr.labels[B:] = Cn
    tr.step((4 * x - 2).to(DEV), y.argmax(-1).to(DEV), accuracy=accuracy)
    torch.cuda.synchronize()
    res = {name: _bits(getattr(tr, name)) for name in ("W", "grad", "loc", "raw", "sigma", "m_loc", "v_loc", "m_raw", "v_raw")}
    res["ce"], res["dZ"], res["stats"] = _bits(tr.ws_t["ce"][:B]), _bits(tr.ws_t["dZ"][:B, :Cn]), _bits(tr.stats)
    if accuracy:
        res["Psum"] = _bits(tr.Psum[:B, :Cn])
    for name in res:
        src = tr.stats if name == "stats" else None
        finite = torch.isfinite(src).all() if src is not None else torch.isfinite(res[name].view(torch.float32)).all()
        assert bool(finite), f"{name} is not finite ({'poisoned' if poison else 'clean'} run)"
    return res


@pytest.mark.parametrize("accuracy", [False, True])
@pytest.mark.parametrize("arch,D,Cn,B", [("fc", 2, 2, 37), ("fc", 10, 3, 5), ("fc", 17, 10, 61), ("fc2", 2, 2, 3), ("fc2", 10, 10, 37), ("fc2", 17, 3, 1)])
def test_nothing_behind_the_bounds_is_read(arch, D, Cn, B, accuracy):
    """NaN is data: every index stays inside its allocation, and a NaN that leaked into a sum would stay there."""
    clean, dirty = _poisoned_step(arch, D, Cn, B, False, accuracy), _poisoned_step(arch, D, Cn, B, True, accuracy)
    for name in clean:
        assert torch.equal(clean[name], dirty[name]), f"{name} depends on memory behind the bounds"
    print(f"[svi-train bounds {arch} D={D} C={Cn} B={B} accuracy={accuracy}] {len(clean)} results bit-identical with NaN in rows >= {B}"
          f"{'' if accuracy else f' and columns [{D}, Dp)'} and labels[{B}:] = {Cn}; excluded: nothing")


def test_two_trainers_from_the_same_arguments_are_bit_identical():
    from robustbnns_amd.svi_train import SviTrainer
    shapes, loc, raw = _guide("fc2", 784, 256, 10, seed=4, std=0.05)
    x, y = O.synthetic_inputs(3 * 100, (1, 28, 28), 10, seed=8)
    runs = []
    for _ in range(2):
        tr = SviTrainer("fc2", "leaky", (1, 28, 28), 10, loc, raw, 0.01, DEV, 0x5EED5EED, batch_size=100)
        for i in range(3):
            tr.step(x[100 * i:100 * (i + 1)].to(DEV), y[100 * i:100 * (i + 1)].argmax(-1).to(DEV))
        torch.cuda.synchronize()
        runs.append({name: _bits(getattr(tr, name)) for name in ("grad", "W", "loc", "raw", "sigma", "m_loc", "v_loc", "m_raw", "v_raw", "stats")})
    for name in runs[0]:
        assert torch.equal(runs[0][name], runs[1][name]), name
    print(f"[svi-train bit-identical fc2 784->256->10 B=100] {len(runs[0])} buffers equal after 3 steps; excluded: nothing")


def test_bnn_train_end_to_end_matches_the_cpu_restatement(tmp_path, capsys):
    import random
    from robustbnns_amd.model_bnn import set_rng_seed
    from robustbnns_amd.svi_train import draw_key, initial_params
    epochs, lr = 6, 0.05
    train, test = _moons_loader(512, 1), _moons_loader(1000, 2, batch=500)
    bnn = _moons_bnn(epochs, lr)
    bnn.train(train, DEV, str(tmp_path) + "/")
    out = capsys.readouterr().out
    for e in range(1, epochs + 1):
        assert f"[Epoch {e}]\t loss: " in out
    assert len(bnn.training_history["loss"]) == len(bnn.training_history["accuracy"]) == epochs
    acc = bnn.evaluate(test, DEV, n_samples=10)
    # the same run on the CPU in fp64: same seed, same init, same key, same batches
    random.seed(0)
    set_rng_seed(0)
    iter(train)                                   # creating the loader's iterator draws its base seed from the CPU generator, before the init
    loc, raw = initial_params([(k, tuple(v.shape)) for k, v in bnn.basenet.state_dict().items()])
    r64 = R.Restatement(loc, raw, "fc2", "leaky", lr, draw_key(), torch.float64)
    for _ in range(epochs):
        for xb, yb in train:
            r64.step(xb, yb.argmax(-1))
    xt, yt = test.dataset.tensors
    acc64 = 100.0 * float((R.predict(r64.loc, r64.raw, xt, "fc2", "leaky", range(10)).argmax(-1) == yt.argmax(-1)).double().mean())
    print(f"held-out accuracy (10 samples): GPU {acc:.2f}  CPU fp64 restatement {acc64:.2f};  history {bnn.training_history}")
    assert abs(acc - acc64) <= 3.0


def test_two_runs_from_the_same_seed_write_bit_identical_param_files(tmp_path):
    train = _moons_loader(256, 3)
    stores = []
    for run in ("a", "b"):
        bnn = _moons_bnn(2)
        bnn.train(train, DEV, str(tmp_path / run) + "/")
        stores.append(torch.load(str(tmp_path / run / bnn.name / (bnn.name + "_weights.pt")), weights_only=False)["params"])
    assert stores[0].keys() == stores[1].keys() and len(stores[0]) == 12
    for k in stores[0]:
        assert torch.equal(stores[0][k], stores[1][k]), k


def test_trained_net_round_trips_through_the_param_file(tmp_path):
    from robustbnns_amd.adversarialAttacks import fgsm_attack
    from robustbnns_amd.model_bnn import set_rng_seed
    train = _moons_loader(256, 4)
    x, y = R.two_moons(64, 0.1, 9)
    rel_a, rel_b = str(tmp_path / "a") + "/", str(tmp_path / "b") + "/"
    bnn = _moons_bnn(2)
    bnn.train(train, DEV, rel_a)
    again = _moons_bnn(2)
    again.load(DEV, rel_a)
    for k in bnn.svi_loc:
        assert torch.equal(again.svi_loc[k], bnn.svi_loc[k]) and torch.equal(again.svi_scale[k], bnn.svi_scale[k]), k
    assert torch.equal(again.forward(x, n_samples=5, seeds=[1, 2, 3, 4, 5]), bnn.forward(x, n_samples=5, seeds=[1, 2, 3, 4, 5]))

    def fgsm(net):
        set_rng_seed(3)
        return fgsm_attack(net, x.clone().to(DEV), y.to(DEV), {"epsilon": 0.2}, n_samples=5).detach().cpu()
    assert torch.equal(fgsm(bnn), fgsm(again))
    # a loaded net that has already drawn (cached guide, slots, seeded draw) trains on from ITS parameters; afterwards its forwards and
    # attacks are those of the trained parameters (the caches of the old guide are dropped)
    before = {k: v.clone() for k, v in again.svi_loc.items()}
    again.forward(x, n_samples=5)
    again.forward(x, n_samples=5, seeds=[1, 2, 3, 4, 5])
    again.epochs = 1
    again.train(train, DEV, rel_b)
    steps = len(train)
    moved = max(float((again.svi_loc[k] - before[k]).abs().max()) for k in before)
    print(f"continued training: max |loc - loaded loc| {moved:.3e} after {steps} steps of lr {again.lr}")
    assert 0 < moved <= 4 * again.lr * steps
    fresh = _moons_bnn(2)                          # same name as `again` (the name carries the constructor's epochs)
    fresh.load(DEV, rel_b)
    assert torch.equal(fgsm(again), fgsm(fresh))
    assert torch.equal(again.forward(x, n_samples=5, seeds=[1, 2, 3, 4, 5]), fresh.forward(x, n_samples=5, seeds=[1, 2, 3, 4, 5]))


def test_fifty_steps_make_no_device_to_host_sync():
    from robustbnns_amd.svi_train import SviTrainer
    shapes, loc, raw = _guide("fc2", 784, 256, 10, seed=1, std=0.05)
    tr = SviTrainer("fc2", "leaky", (1, 28, 28), 10, loc, raw, 0.01, DEV, 0xABC, batch_size=128)
    x = torch.rand(51, 128, 1, 28, 28, device=DEV)
    lab = torch.randint(0, 10, (51, 128), device=DEV)
    tr.step(x[0], lab[0])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for i in range(1, 51):
            tr.step(x[i], lab[i])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    loss, correct = tr.epoch_totals()
    assert loss == loss and 0 <= correct <= 51 * 128 and tr.t == 51


def test_guards_raise_not_implemented(tmp_path):
    from robustbnns_amd.model_bnn import BNN
    loader = _moons_loader(64, 5)
    with pytest.raises(NotImplementedError):
        _moons_bnn(1).train(loader, "cpu", str(tmp_path) + "/")
    conv = BNN("mnist", 32, "leaky", "conv", "svi", 1, 0.01, None, None, (1, 28, 28), 10)
    with pytest.raises(NotImplementedError):
        conv.train(loader, DEV, str(tmp_path) + "/")
    hmc = BNN("half_moons", 32, "leaky", "fc2", "hmc", None, None, 5, 2, (1, 2, 1), 2)
    with pytest.raises(NotImplementedError):
        hmc.train(loader, DEV, str(tmp_path) + "/")
    assert hmc.train(False) is hmc and hmc.training is False                     # nn.Module.train(mode) still passes through
    # a hidden size outside what rbnn_svi_draw covers (16, or a multiple of 32): refused at construction, nothing is trained
    from robustbnns_amd.svi_train import SviTrainer
    for arch in ("fc", "fc2"):
        _, loc, raw = _guide(arch, 784, 48, 10, seed=1, std=0.05)
        with pytest.raises(NotImplementedError):
            SviTrainer(arch, "leaky", (1, 28, 28), 10, loc, raw, 0.01, DEV, 1, batch_size=8)
    # a hidden size the training kernels take and the accuracy forward (rbnn_fc_forward: 32, 64, k * 128) does not: gradients and steps without
    # the accuracy run (GRAD_CASES); a step WITH it is refused before anything is launched (BNN itself takes powers of two only)
    _, loc, raw = _guide("fc", 784, 96, 10, seed=1, std=0.05)
    tr = SviTrainer("fc", "leaky", (1, 28, 28), 10, loc, raw, 0.01, DEV, 1, batch_size=8)
    before = (tr.loc.clone(), tr.raw.clone(), tr.stats.clone())
    x8, y8 = O.synthetic_inputs(8, (1, 28, 28), 10, seed=2)
    with pytest.raises(NotImplementedError):
        tr.step(x8.to(DEV), y8.argmax(-1).to(DEV))
    assert tr.t == 0 and all(torch.equal(a, b) for a, b in zip(before, (tr.loc, tr.raw, tr.stats)))
