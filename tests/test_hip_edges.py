"""GPU tests (-m gpu) of the default kernels off the 28x28 path: input widths, point / sample counts, loss modes and input strides
that the other modules never reach.

  A  triple fc / fc2 (what `auto` picks) against fp64 across input widths: D % 32 == 0, D % 4 != 0, fewer than / exactly 9 gradient
     column tiles, N at the 16-point group and 256-point image edges, S in {1, 8, 9, 17}, C in {2, 10}; inputs in [-2, 3]
  B  triple PGD step by step on the kernel's own iterates, through both step entry points (attack_step_triple carrying the next
     iterate's image; attack_step + image rebuild when D % 4 != 0)
  C  the autograd hook (RBNN_LOSS_UPSTREAM / _LOGIT) against an fp64 vector-Jacobian product: fc, fc2, conv, triple and exact;
     NaN in the padding classes of G_up must not reach the result
  D  conv MEAN_LOGIT (deterministic nets, ensembles) against the decision-pinned fp64 oracle, FGSM on it
  E  conv input row strides and alignment: padded ldx is bit-identical to the dense one; an unaligned view costs a copy, not an error
Every case prints one line: its worst error against fp64 in units of 1e-5 and what each exclusion removed (kink / cancellation /
marginal pixel).  Everything goes through the C-ABI (robustbnns_amd._hip); the oracle is the checker only.
"""
import ctypes as _C

import numpy as np
import pytest
import torch

from conftest import cancellation_condition, rel_err_points
from oracle import bnn_oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("built_library")]
TOL, TAU, KINK, DEV = 1e-5, 1e-3, 2e-6, "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from robustbnns_amd import _hip
    _hip.load()


def _line(tag, worst, kink, canc, marg, N, extra=""):
    """kink / cancellation: points; marginal-pixel: pixels (the most any one compared image set of the case left out)."""
    print(f"[edges {tag}] {extra}worst {worst / TOL:.3f} x 1e-5; excluded: kink {kink} / cancellation {canc} / marginal-pixel {marg} of {N} "
          f"(points / points / pixels)")


def _safe_pixels(ref, rows):
    """Pixels compared in an adversarial image: |g| > TAU * max|g| of the point, on the points in `rows`."""
    N = ref.shape[0]
    g = ref.reshape(N, -1).abs()
    safe = (g > TAU * g.max(1, keepdim=True)[0]) & rows.reshape(N, 1)
    return safe, int((~safe)[rows].sum())


def _check_attack(adv, x, eps_step, ref, rows, what):
    """adv == clamp(x + eps_step * sign(ref), 0, 1) at the safe pixels (fp32, the reference's order); returns the marginal-pixel count."""
    safe, marg = _safe_pixels(ref, rows)
    want = torch.clamp(x + eps_step * ref.sign().float(), 0, 1)
    bad = ((adv.cpu().reshape(len(x), -1) - want.reshape(len(x), -1)).abs() > 1e-6) & safe
    assert not bad.any(), f"{what}: {int(bad.sum())} non-marginal pixels differ"
    return marg


# ------------------------------------------------------------------ A. triple fc / fc2 against fp64 across input widths
# std: every pre-activation is ~N(0, sigma^2) with sigma ~ std * sqrt(D / 3) ~ 0.5-1, so P(|a| < 2e-6) per unit is ~3e-6 and a point
# has a kink within the margin with probability ~S * H * 3e-6 < 2 %: far more than 40 % of the points clear it (asserted per case)
A_CASES = [  # arch, act, shape, H, C, S, N, std
    ("fc", "leaky", (1, 17, 1), 128, 2, 9, 257, 0.2), ("fc", "relu", (1, 10, 10), 256, 10, 8, 16, 0.1),
    ("fc", "tanh", (1, 12, 12), 384, 5, 17, 15, 0.08), ("fc", "leaky", (1, 14, 14), 128, 10, 1, 1, 0.1),
    ("fc", "sigm", (1, 5, 50), 256, 3, 3, 255, 0.1), ("fc", "leaky", (1, 32, 32), 512, 10, 5, 300, 0.05),
    ("fc", "relu", (3, 32, 32), 512, 10, 9, 129, 0.03), ("fc", "leaky", (3, 32, 32), 1024, 10, 2, 17, 0.03),
    ("fc", "leaky", (1, 28, 28), 640, 10, 3, 40, 0.05),
    ("fc2", "relu", (1, 17, 1), 128, 2, 3, 256, 0.2), ("fc2", "tanh", (1, 10, 10), 384, 7, 9, 33, 0.1),
    ("fc2", "sigm", (1, 32, 32), 128, 10, 8, 1, 0.05), ("fc2", "leaky", (3, 32, 32), 256, 10, 4, 130, 0.03),
    ("fc2", "leaky", (1, 28, 28), 384, 10, 2, 70, 0.05),
]


def _geometry(eng):
    p = eng.post
    return f"ld_rows={p.triple_images().ld_rows} Dp/16={p.Dp // 16} D%4={p.D % 4} "


def test_auto_precision_boundary_between_lowdim_and_triple():
    """in_features 16 resolves to the one-launch lowdim kernels, 17 to the triple kernels (both with hidden % 128 == 0, <= 10 classes)."""
    from robustbnns_amd import AttackEngine, StackedPosterior
    for D, want in ((16, "lowdim"), (17, "triple")):
        post = O.synthetic_posterior("fc", D, 128, 2, 2, 0.2)
        eng = AttackEngine(StackedPosterior("fc", "leaky", (1, D, 1), 2, 128, post, DEV))
        print(f"[edges boundary] D={D}: precision == {eng.precision}")
        assert eng.precision == want


def _fp64_checks(eng, arch, act, x, y, post, S, tag, attack=True):
    """Forward (probabilities, logits), PER_SAMPLE, MEAN_PROB and MEAN_LOGIT gradients, FGSM on both means, a repeated-index seeds call."""
    from robustbnns_amd import _hip
    N, D = x.shape[0], eng.post.D
    lab = y.argmax(-1)
    p64 = O.cast(post, torch.float64)
    xd = x.double()
    worst = float(rel_err_points(eng.forward(x, S).cpu(), O.bnn_forward(xd, p64, arch, act, S)).max())
    worst = max(worst, float(rel_err_points(eng.forward(x, S, logits=True).cpu(), O.ensemble_forward(xd, p64, arch, act, S)).max()))
    assert worst < TOL, f"{tag}: forward {worst / TOL:.3f} x 1e-5"
    ok = O.kink_margin(xd, p64, arch, act, S) > KINK
    kinks = int((~ok).sum())
    assert kinks <= max(3, N // 20) and int(ok.sum()) >= 0.4 * N
    e = rel_err_points(eng.loss_gradients(x, y, S).cpu(), O.loss_gradients(xd, y, p64, arch, act, S))[ok]
    worst = max(worst, float(e.max()) if e.numel() else 0.0)
    assert not bool((e >= TOL).any()), f"{tag}: loss_gradients {float(e.max()) / TOL:.3f} x 1e-5"
    canc = marg = 0
    labd = lab.int().to(DEV)
    for mode, kind in ((_hip.LOSS_MEAN_PROB, "bnn"), (_hip.LOSS_MEAN_LOGIT, "ensemble")):
        G = eng.gradient(eng.pad_inputs(x), labd, None, S, mode)[:, :D].cpu().reshape(x.shape)
        ref = O.meanprob_gradients(xd, lab, p64, arch, act, S, kind=kind)
        bound = torch.clamp(2.0 ** -23 * cancellation_condition(x, lab, post, arch, act, S, kind), min=TOL)
        e = rel_err_points(G, ref)
        assert not bool((e > bound)[ok].any()), (tag, kind, float((e / bound)[ok].max()), int((e / bound)[ok].argmax()))
        n_c = int((bound > TOL)[ok].sum())
        assert n_c <= max(1, N // 100)
        canc = max(canc, n_c)
        plain = ok & (bound <= TOL)
        if plain.any():
            worst = max(worst, float(e[plain].max()))
        if attack:
            adv = eng.fgsm(x, y, S, 0.1, mode=mode)
            marg = max(marg, _check_attack(adv, x, 0.1, ref, plain, f"{tag} fgsm {kind}"))
    idx = [S - 1, 0, 0, 1 if S > 1 else 0]
    p_idx = O.bnn_forward(xd, p64, arch, act, len(idx), seeds=idx)
    e_f = float(rel_err_points(eng.forward(x, len(idx), seeds=idx).cpu(), p_idx).max())
    g_idx = O._input_grad(xd, lab, O.select(p64, idx), arch, act, "per_sample")
    e_g = rel_err_points(eng.loss_gradients(x, y, len(idx), seeds=idx).cpu(), g_idx)[ok]
    assert e_f < TOL and not bool((e_g >= TOL).any()), f"{tag}: seeds {idx}: forward {e_f / TOL:.3f}, gradients {float(e_g.max()) / TOL:.3f} x 1e-5"
    worst = max(worst, e_f, float(e_g.max()) if e_g.numel() else 0.0)
    return worst, kinks, canc, marg


@pytest.mark.parametrize("arch,act,shape,H,C,S,N,std", A_CASES)
def test_triple_default_against_fp64_across_input_widths(arch, act, shape, H, C, S, N, std):
    from robustbnns_amd import AttackEngine, StackedPosterior
    D = int(np.prod(shape))
    post = O.synthetic_posterior(arch, D, H, C, S, std)
    x, y = O.synthetic_inputs(N, shape, C, seed=D + H + N)
    eng = AttackEngine(StackedPosterior(arch, act, shape, C, H, post, DEV))          # no precision argument: what a caller gets
    assert eng.precision == "triple"
    tag = f"A {arch} {act} {shape} H={H} C={C} S={S} N={N}"
    worst, kinks, canc, marg = _fp64_checks(eng, arch, act, x, y, post, S, tag)
    _line(tag, worst, kinks, canc, marg, N, f"precision == {eng.precision} {_geometry(eng)}")
    assert worst < TOL


@pytest.mark.parametrize("arch,H", [("fc", 512), ("fc2", 256)])
def test_triple_default_with_standardised_inputs(arch, H):
    """Inputs in [-2, 3], as standardised CIFAR pixels are: the X image's scale is taken from max |x| away from [0, 1]."""
    from robustbnns_amd import AttackEngine, StackedPosterior
    shape, C, S, N = (3, 32, 32), 10, 3, 64
    D = int(np.prod(shape))
    post = O.synthetic_posterior(arch, D, H, C, S, 0.015)
    x, y = O.synthetic_inputs(N, shape, C, seed=91)
    x = x * 5.0 - 2.0
    eng = AttackEngine(StackedPosterior(arch, "leaky", shape, C, H, post, DEV))
    assert eng.precision == "triple"
    tag = f"A {arch} leaky {shape} H={H} inputs in [-2, 3] S={S} N={N}"
    worst, kinks, canc, marg = _fp64_checks(eng, arch, "leaky", x, y, post, S, tag, attack=False)
    _line(tag, worst, kinks, canc, marg, N, f"precision == {eng.precision} {_geometry(eng)}")


# ------------------------------------------------------------------ B. triple PGD step by step on the kernel's own iterates
B_CASES = [  # arch, act, shape, H, C, S, N, std, loss, step path
    ("fc", "sigm", (1, 5, 50), 256, 3, 3, 64, 0.1, "mean_prob", "rebuild"),
    ("fc2", "relu", (1, 17, 1), 128, 2, 3, 64, 0.2, "mean_prob", "rebuild"),
    ("fc", "relu", (3, 32, 32), 512, 10, 3, 40, 0.03, "mean_prob", "carry"),
    ("fc2", "tanh", (1, 10, 10), 384, 7, 3, 40, 0.1, "mean_prob", "carry"),
    ("fc", "leaky", (1, 32, 32), 512, 10, 3, 50, 0.05, "mean_logit", "carry"),
]


@pytest.mark.parametrize("arch,act,shape,H,C,S,N,std,loss,path", B_CASES)
def test_triple_pgd_steps_along_the_kernels_iterates(arch, act, shape, H, C, S, N, std, loss, path):
    """x_k = pgd(x, iters=k), k = 1..4: every x_{k+1} is one reference step (oracle.pgd_step's fp32 order, fp64 gradient) from the
    kernel's own x_k, alpha = 2 / max(x_0) per image; the entry point that ran is counted."""
    from robustbnns_amd import AttackEngine, StackedPosterior, _hip
    D = int(np.prod(shape))
    post = O.synthetic_posterior(arch, D, H, C, S, std)
    x, y = O.synthetic_inputs(N, shape, C, seed=D + 5)
    lab = y.argmax(-1)
    p64 = O.cast(post, torch.float64)
    eng = AttackEngine(StackedPosterior(arch, act, shape, C, H, post, DEV))
    assert eng.precision == "triple"
    eng.post.triple_images()
    calls = {"attack_step": 0, "attack_step_triple": 0, "triple_rows": 0}
    for fn in calls:
        real = getattr(eng.k, fn)
        setattr(eng.k, fn, (lambda real, fn: lambda *a, **kw: (calls.__setitem__(fn, calls[fn] + 1), real(*a, **kw))[1])(real, fn))
    mode, kind = (_hip.LOSS_MEAN_PROB, "bnn") if loss == "mean_prob" else (_hip.LOSS_MEAN_LOGIT, "ensemble")
    eps = 0.1
    alpha = (2 / x.reshape(N, -1).max(1)[0]).reshape((N,) + (1,) * len(shape))
    iters = [x]
    for k in range(1, 5):
        for fn in calls:
            calls[fn] = 0
        iters.append(eng.pgd(x, y, S, eps, alpha=None, iters=k, mode=mode).cpu())
        if path == "carry":
            assert calls["attack_step_triple"] == k and calls["attack_step"] == 0 and calls["triple_rows"] == 1, calls
        else:
            assert calls["attack_step"] == k and calls["attack_step_triple"] == 0 and calls["triple_rows"] == k, calls
    assert torch.equal(eng.pgd(x, y, S, eps, alpha=None, iters=4, mode=mode).cpu(), iters[4])        # bit-deterministic
    kinks = marg = 0
    for k in range(4):
        xk = iters[k]
        g = O.meanprob_gradients(xk.double(), lab, p64, arch, act, S, kind)
        ok = O.kink_margin(xk.double(), p64, arch, act, S) > KINK
        kinks = max(kinks, int((~ok).sum()))
        assert int((~ok).sum()) <= max(3, N // 20)
        want = torch.clamp(x + torch.clamp(xk + alpha * g.sign().float() - x, min=-eps, max=eps), min=0, max=1)
        safe, m = _safe_pixels(g, ok)
        marg = max(marg, m)
        bad = ((iters[k + 1] - want).abs().reshape(N, -1) > 1e-6) & safe
        assert not bad.any(), f"step {k} -> {k + 1}: {int(bad.sum())} non-marginal pixels differ"
    entry = "attack_step_triple" if path == "carry" else "attack_step + rebuild"
    _line(f"B {arch} {act} {shape} H={H} C={C} S={S} N={N} {loss}", 0.0, kinks, 0, marg, N,
          f"step entry point: {entry} D%4={D % 4}; pixels of 4 steps equal at the safe pixels; ")


# ------------------------------------------------------------------ C. the autograd hook against an fp64 vector-Jacobian product
def _upstream_condition(x, gup, post, arch, act, S, logits):
    """cancellation_condition for the vector-Jacobian product: sum_s max_d |c_s| / max_d |sum_s c_s| over the per-sample contributions."""
    p64 = O.cast(post, torch.float64)
    xd = x.double().clone().requires_grad_(True)
    N = x.shape[0]
    outs = [O.nn_logits(xd, O.select(p64, [s]), arch, act)[0] for s in range(S)]
    if not logits:
        outs = [torch.softmax(o, -1) for o in outs]
    c = [torch.autograd.grad((o * gup.double()).sum() / S, xd, retain_graph=True)[0].reshape(N, -1) for o in outs]
    return sum(v.abs().max(1)[0] for v in c) / sum(c).abs().max(1)[0].clamp_min(1e-300)


def _upstream_ref(x, gup, post, arch, act, S, logits, seeds=None):
    p64 = O.cast(post, torch.float64)
    if seeds is not None:
        p64, S = O.select(p64, seeds), len(seeds)
    xd = x.double().clone().requires_grad_(True)
    out = O.ensemble_forward(xd, p64, arch, act, S) if logits else O.bnn_forward(xd, p64, arch, act, S)
    (out * gup.double()).sum().backward()
    return xd.grad.detach()


C_CASES = [  # arch, act, shape, H, C, S, N, std, precision
    ("fc", "leaky", (1, 28, 28), 512, 10, 3, 40, 0.05, "triple"), ("fc", "leaky", (3, 32, 32), 512, 10, 2, 24, 0.03, "triple"),
    ("fc2", "leaky", (1, 28, 28), 256, 10, 3, 40, 0.05, "triple"), ("fc", "leaky", (1, 28, 28), 64, 10, 4, 20, 0.05, "exact"),
    ("conv", "sigm", (1, 28, 28), 64, 10, 2, 12, 0.05, "triple"), ("conv", "tanh", (3, 32, 32), 32, 10, 2, 8, 0.05, "triple"),
    ("conv", "leaky", (1, 28, 28), 512, 10, 2, 16, 0.03, "triple"), ("conv", "leaky", (3, 32, 32), 64, 10, 2, 12, 0.04, "triple"),
    ("conv", "tanh", (1, 28, 28), 64, 10, 2, 12, 0.05, "exact"),
]


def _engine(arch, act, shape, H, C, post, precision=None):
    from robustbnns_amd import AttackEngine, StackedPosterior
    from robustbnns_amd.conv import ConvEngine, ConvStackedPosterior
    if arch == "conv":
        return ConvEngine(ConvStackedPosterior(act, shape, C, H, post, DEV), precision=precision)
    return AttackEngine(StackedPosterior(arch, act, shape, C, H, post, DEV), precision=precision)


def _conv_post(shape, H, C, S, std):
    q2 = ((shape[1] - 4) // 2) - 5
    return O.synthetic_posterior("conv", int(np.prod(shape)), H, C, S, std, in_ch=shape[0], head=q2 * q2 * H)


@pytest.mark.parametrize("arch,act,shape,H,C,S,N,std,precision", C_CASES)
def test_autograd_hook_against_fp64_vjp(arch, act, shape, H, C, S, N, std, precision):
    """forward(x.requires_grad_()) -> backward(gup) (the caller's surface: BNN.forward for probabilities, the engine's forward with
    logits=True as NN / Ensemble_NN call it) and eng.gradient(LOSS_UPSTREAM[_LOGIT], G_up) against fp64 autograd of <gup, forward>;
    gup has mixed signs and a one-hot row; NaN in G_up's padding classes C..15 leaves the result bit-identical."""
    D = int(np.prod(shape))
    post = _conv_post(shape, H, C, S, std) if arch == "conv" else O.synthetic_posterior(arch, D, H, C, S, std)
    hook_checks(arch, act, shape, H, C, S, N, post, precision)


def hook_checks(arch, act, shape, H, C, S, N, post, precision):
    """The checks of test_autograd_hook_against_fp64_vjp on a given posterior (also run by test_hip_rescale at 13 and 16 classes)."""
    import test_hip_round2 as R2
    from robustbnns_amd import _hip
    from robustbnns_amd.model_bnn import BNN
    D = int(np.prod(shape))
    x, y = O.synthetic_inputs(N, shape, C, seed=D + H + 3)
    # conv's default is triple: the exact conv kernels are asked for by name (fc at H = 64 resolves to exact by itself)
    eng = _engine(arch, act, shape, H, C, post, precision="exact" if (arch == "conv" and precision == "exact") else None)
    assert eng.precision == precision
    p64 = O.cast(post, torch.float64)
    gup = torch.randn(N, C, generator=torch.Generator().manual_seed(N + C))
    gup[0] = 0.0
    gup[0, 1] = 1.0                                                              # a one-hot row
    ok = O.kink_margin(x.double(), p64, arch, act, S) > KINK if arch != "conv" else torch.ones(N, dtype=torch.bool)
    kinks = int((~ok).sum())
    assert kinks <= max(3, N // 20)
    worst, canc = 0.0, 0
    for logits, mode in ((False, _hip.LOSS_UPSTREAM), (True, _hip.LOSS_UPSTREAM_LOGIT)):
        # the caller's surface
        xr = x.clone().requires_grad_(True)
        if not logits and arch != "conv" and shape == (1, 28, 28):
            bnn = BNN("mnist", H, act, arch, "hmc", None, None, S, 0, shape, C)
            bnn.set_posterior_samples(post, DEV)
            assert bnn._engine.precision == precision
            out = bnn.forward(xr, n_samples=S)
        else:
            out = eng.forward(xr, S, logits=logits)
        out.backward(gup.to(out.device))
        G_auto = xr.grad.detach().cpu().reshape(N, -1)
        # the C-ABI: G_up [N, 16] with NaN in the padding classes
        gz = torch.zeros(N, _hip.CPAD)
        gz[:, :C] = gup
        gn = torch.full((N, _hip.CPAD), float("nan"))
        gn[:, :C] = gup
        G_zero = eng.gradient(eng.pad_inputs(x), None, None, S, mode, G_up=gz.to(DEV))[:, :D].cpu().clone()
        G_nan = eng.gradient(eng.pad_inputs(x), None, None, S, mode, G_up=gn.to(DEV))[:, :D].cpu().clone()
        assert torch.equal(G_nan, G_zero), "the padding classes of G_up reached the result"
        ref = _upstream_ref(x, gup, post, arch, act, S, logits).reshape(N, -1)
        bound = torch.clamp(2.0 ** -23 * _upstream_condition(x, gup, post, arch, act, S, logits), min=TOL)
        n_c = int((bound > TOL)[ok].sum())
        assert n_c <= max(1, N // 100)
        canc = max(canc, n_c)
        if arch == "conv":
            st1, st2 = R2.conv_stashes(eng, N, S, H)
            pinned, far, n_diff = R2.conv_pinned_oracle(x, None, post, act, S, st1, st2, "upstream_logit" if logits else "upstream", gup)
            assert far < R2.KINK_CONV
            pinned = pinned.reshape(N, -1)
            for G in (G_auto, G_zero):
                e = rel_err_points(G, pinned)
                assert not bool((e > bound).any()), f"conv {'logits' if logits else 'probs'}: {float((e / bound).max()):.3f} x the bound (pinned oracle)"
                worst = max(worst, float(e[bound <= TOL].max()))
                unexplained = (rel_err_points(G, ref) >= bound) & (n_diff == 0)
                assert not unexplained.any(), f"{int(unexplained.sum())} points differ from plain fp64 without a flipped decision"
            kinks = max(kinks, int((n_diff > 0).sum()))          # conv: points with a decision pinned away from fp64's own
            continue
        for G in (G_auto, G_zero):
            e = rel_err_points(G, ref)
            assert not bool((e > bound)[ok].any()), ("logits" if logits else "probs", float((e / bound)[ok].max()))
            worst = max(worst, float(e[ok & (bound <= TOL)].max()))
    if arch != "conv":
        # a seeds subset through the hook
        idx = [S - 1, 0, 0]
        xr = x.clone().requires_grad_(True)
        eng.forward(xr, len(idx), seeds=idx).backward(gup.to(DEV))
        e = rel_err_points(xr.grad.reshape(N, -1), _upstream_ref(x, gup, post, arch, act, S, False, seeds=idx).reshape(N, -1))[ok]
        assert float(e.max()) < TOL, f"seeds {idx}: {float(e.max()) / TOL:.3f} x 1e-5"
        worst = max(worst, float(e.max()))
    _line(f"C {arch} {act} {shape} H={H} C={C} S={S} N={N}", worst, kinks, canc, 0, N,
          f"precision == {eng.precision}; UPSTREAM and UPSTREAM_LOGIT, autograd and C-ABI, NaN padding inert; ")


# ------------------------------------------------------------------ D. conv MEAN_LOGIT against the decision-pinned fp64 oracle
def _d_cases():
    import test_hip_round2 as R2
    cases = [c for c in R2.CONV_CASES if c[-1] in ("exact", "triple")]
    cases += [("leaky", (1, 28, 28), 10, 48, 2, 20, 0.05, "triple"), ("relu", (3, 32, 32), 10, 48, 2, 15, 0.05, "triple"),
              ("leaky", (3, 32, 32), 10, 48, 2, 15, 0.05, "exact")]
    return cases


@pytest.mark.parametrize("act,shape,Cn,Hc,S,N,std,precision", _d_cases())
def test_conv_mean_logit_with_pinned_decisions(act, shape, Cn, Hc, S, N, std, precision):
    """RBNN_LOSS_MEAN_LOGIT on conv (a deterministic NN / an Ensemble_NN under fgsm / pgd): max < 1e-5 and median < MEDIAN_BAR against the
    fp64 oracle with the kernels' own pooling / sign decisions; every point further than 1e-5 from the plain oracle has a flipped decision;
    FGSM on the mean logits equal at the safe pixels."""
    import test_hip_round2 as R2
    from robustbnns_amd import _hip
    from robustbnns_amd.conv import ConvEngine, ConvStackedPosterior
    post = _conv_post(shape, Hc, Cn, S, std)
    x, y = O.synthetic_inputs(N, shape, Cn, seed=Hc + N + 1)
    lab = y.argmax(-1)
    p64 = O.cast(post, torch.float64)
    eng = ConvEngine(ConvStackedPosterior(act, shape, Cn, Hc, post, DEV), precision=precision)
    assert eng.precision == precision
    G = eng.gradient(eng.pad_inputs(x), lab.int().to(DEV), None, S, _hip.LOSS_MEAN_LOGIT).cpu().reshape(N, -1).clone()
    st1, st2 = R2.conv_stashes(eng, N, S, Hc)
    pinned, far, n_diff = R2.conv_pinned_oracle(x, lab, post, act, S, st1, st2, "mean_logit")
    bound = torch.clamp(2.0 ** -23 * cancellation_condition(x, lab, post, "conv", act, S, "ensemble"), min=TOL)
    canc = int((bound > TOL).sum())
    assert canc <= max(1, N // 100)
    err = R2.per_point_err(G, pinned)
    assert not bool((err > bound).any()), f"pinned: {float((err / bound).max()):.3f} x the bound"
    assert float(err[bound <= TOL].max()) < TOL and float(err.median()) < R2.MEDIAN_BAR
    assert far < R2.KINK_CONV
    plain = O.meanprob_gradients(x.double(), lab, p64, "conv", act, S, kind="ensemble")
    err_plain = R2.per_point_err(G, plain)
    unexplained = (err_plain >= bound) & (n_diff == 0)
    assert not unexplained.any(), f"{int(unexplained.sum())} points differ from the plain fp64 oracle without a flipped decision"
    clean = (err_plain < TOL)
    adv = eng.fgsm(x, y, S, 0.1, mode=_hip.LOSS_MEAN_LOGIT)
    marg = _check_attack(adv, x, 0.1, plain, clean, "fgsm mean_logit")
    _line(f"D conv {act} {shape} Hc={Hc} C={Cn} S={S} N={N} {precision} mean_logit", float(err[bound <= TOL].max()), int((n_diff > 0).sum()),
          canc, marg, N, f"precision == {eng.precision}; pinned median {float(err.median()) / TOL:.3f} x 1e-5; farthest flipped decision from a tie {far:.1e}; ")


# ------------------------------------------------------------------ E. conv input row strides and alignment
@pytest.mark.parametrize("shape,precision", [((1, 28, 28), "exact"), ((1, 28, 28), "triple"), ((3, 32, 32), "exact"), ((3, 32, 32), "triple")])
def test_conv_forward_padded_row_stride_is_bit_identical(shape, precision):
    """The conv forwards at the C-ABI with ldx = Cin*W*W + 4 and + 36 (NaN in the pad columns) leave P bit-identical to ldx = Cin*W*W;
    rbnn_attack_step on conv-sized rows with a padded ldx gives the same pixels and leaves the pad columns alone."""
    from robustbnns_amd import _hip
    from robustbnns_amd.conv import ConvEngine, ConvStackedPosterior
    Hc, C, S, N = 32, 10, 2, 9
    D = int(np.prod(shape))
    post = _conv_post(shape, Hc, C, S, 0.05)
    x, y = O.synthetic_inputs(N, shape, C, seed=13)
    eng = ConvEngine(ConvStackedPosterior("leaky", shape, C, Hc, post, DEV), precision=precision)
    assert eng.precision == precision
    k = eng.k
    ws = eng.workspace(N, S)
    Xd = x.reshape(N, D).to(DEV).contiguous()
    ds = eng._input_scales(Xd, iterates=False)

    # straight to the C-ABI: the tensor façade (robustbnns_amd._hip) accepts contiguous tensors only, the library any ldx it validates
    lib, net, w, st = k.lib, eng.post.descriptor(), k._conv_ws(ws), _hip.stream_of(Xd)
    ptr = _hip.ptr

    def fwd(X):
        if precision == "triple":
            rows, k2_exp = eng.post.triple_images()[:2]
            _hip.check(lib.rbnn_conv_forward_triple(_C.byref(net), ptr(rows), k2_exp, 0, ptr(ds[4:]), ptr(X), X.stride(0), N, None, S,
                                                    _hip.OUT_PROBS, _C.byref(w), st), "rbnn_conv_forward_triple")
        else:
            _hip.check(lib.rbnn_conv_forward(_C.byref(net), ptr(X), X.stride(0), N, None, S, _hip.OUT_PROBS, _C.byref(w), st), "rbnn_conv_forward")
        return ws["P"][:S * N * _hip.CPAD].cpu().clone()

    def step(X, X0, G, project):
        _hip.check(lib.rbnn_attack_step(ptr(X), ptr(X0), X.stride(0), ptr(G), 1, 0, D, None, 0.05, 0.03, int(project), N, D, st),
                   "rbnn_attack_step")

    def padded(t, ldx):
        buf = torch.full((N, ldx), float("nan"), device=DEV)
        buf[:, :D] = t
        return buf, buf[:, :D]

    P0 = fwd(Xd)
    assert torch.isfinite(P0).all()
    G = torch.randn(N, D, generator=torch.Generator().manual_seed(2)).to(DEV)
    G[:, ::7] = 0.0
    ref = {}
    for project in (False, True):
        X = Xd.clone()
        step(X, Xd if project else None, G, project)
        ref[project] = X.cpu()
    for extra in (4, 36):
        buf, X = padded(Xd, D + extra)
        assert X.stride(0) == D + extra and X.data_ptr() % 16 == 0
        assert torch.equal(fwd(X), P0), f"ldx = D + {extra}: P differs"
        for project in (False, True):
            b, Xs = padded(Xd, D + extra)
            b0, X0s = padded(Xd, D + extra)
            step(Xs, X0s if project else None, G, project)
            assert torch.equal(Xs.cpu(), ref[project]) and torch.isnan(b[:, D:]).all(), f"attack_step, ldx = D + {extra}, project={project}"
    print(f"[edges E conv {shape} {precision}] ldx = D, D + 4, D + 36: P and attack_step bit-identical, pad columns untouched")


@pytest.mark.parametrize("kind", ["conv-exact", "conv-triple", "fc-exact", "fc-triple"])
def test_unaligned_input_view_costs_a_copy_not_an_error(kind):
    """An input built as buf[1:1 + N*D].view(N, *shape) (4 bytes past a 16-byte boundary) gives forward, gradient and fgsm results
    bit-identical to the aligned tensor: pad_inputs copies it (the kernels refuse an unaligned X with RBNN_ERR_ALIGN)."""
    from robustbnns_amd import _hip
    arch, precision = kind.split("-")
    shape, H, C, S, N = (1, 28, 28), (32 if arch == "conv" else 128), 10, 2, 20
    D = int(np.prod(shape))
    post = _conv_post(shape, H, C, S, 0.05) if arch == "conv" else O.synthetic_posterior(arch, D, H, C, S, 0.05)
    eng = _engine(arch, "leaky", shape, H, C, post, precision=precision)
    assert eng.precision == precision
    x, y = O.synthetic_inputs(N, shape, C, seed=17)
    xa = x.to(DEV)
    buf = torch.empty(N * D + 4, device=DEV)
    xu = buf[1:1 + N * D].view(N, *shape)
    xu.copy_(xa)
    assert xu.data_ptr() % 16 == 4 and xa.data_ptr() % 16 == 0
    lab = y.argmax(-1).int().to(DEV)
    out = {}
    for tag, xin in (("aligned", xa), ("unaligned", xu)):
        Xp = eng.pad_inputs(xin)
        assert Xp.data_ptr() % 16 == 0
        out[tag] = (eng.forward(xin, S).cpu(), eng.gradient(Xp, lab, None, S, _hip.LOSS_MEAN_PROB)[:, :D].cpu().clone(),
                    eng.fgsm(xin, y, S, 0.1).cpu())
    assert torch.equal(xu, xa)                                                       # the caller's tensor is not written
    for a, b, what in zip(out["aligned"], out["unaligned"], ("forward", "gradient", "fgsm")):
        assert torch.equal(a, b), what
    print(f"[edges E {kind}] a 4-byte-offset input view: forward, gradient, fgsm bit-identical to the aligned tensor")
