"""Host tests (no GPU) of the dynamic-range guard of the weight images that share one power-of-two scale.

The triple and split images (rbnn_triple_rows, rbnn_split_rows, the conv images) carry each weight as fp16 pieces at ONE scale per tensor, taken
from the tensor's largest magnitude (conv1's triple kernel: one per sample).  A weight 2^-a below that maximum loses bits once a > ~15: pieces 2
and 3 fall into fp16 subnormals.  Rescaling a block of units by 2^a and the next layer's matching weights by 2^-a computes the same function
(relu / leaky: act(c v) = c act(v) for c > 0; max pooling commutes with it), keeps every tensor's max / mean inside posterior.narrow_range, and
leaves the rest of the tensor 2^a below its scale.  posterior.slices_in_range is the guard that sends such posteriors to the fp32 kernels.

  - the fp64 oracle is invariant under every rescaling (the construction itself, shared with tests/test_hip_rescale.py)
  - emulated_image (numpy fp16, round to nearest even, the kernels' piece split and scale_exp) is the documented reason for the 2^12 threshold:
    every rescaled posterior whose emulated images miss 1e-5 against fp64 is refused, for stored posteriors and SVI guides alike
  - the guard accepts every trained fixture, the posteriors bench.py builds and the i.i.d. synthetic posteriors the GPU suite asserts triple on
"""
import glob
import os

import numpy as np
import pytest
import torch

from conftest import rel_err_points
from oracle import bnn_oracle as O

TOL, KINK = 1e-5, 2e-6
ALPHAS = [2.0 ** 8, 2.0 ** 16, 2.0 ** 20, 2.0 ** 24, 2.0 ** 30]
KEYS = {"fc": dict(W1="model.1.weight", b1="model.1.bias", W2="model.3.weight"),
        "fc2": dict(W1="model.1.weight", b1="model.1.bias", Wm="model.3.weight", bm="model.3.bias", W2="model.5.weight"),
        "conv": dict(K1w="model.0.weight", K1b="model.0.bias", K2w="model.3.weight", K2b="model.3.bias", Fw="model.7.weight")}
RESCALINGS = {"fc": ("units", "sample"), "fc2": ("layer1", "layer2"), "conv": ("conv1", "conv2")}


def rescale(post, arch, how, alpha, s=0, units=slice(3, 19)):
    """A copy of the stacked posterior computing the same function, sample s rescaled by the power of two alpha (exact in fp32):
      units  (fc)   W1 rows and b1 of `units` x alpha, the matching W2 columns / alpha
      sample (fc)   W1[s], b1[s] x alpha, W2[s] / alpha
      layer1 (fc2)  W1 rows and b1 of `units` x alpha, the matching Wm columns / alpha
      layer2 (fc2)  Wm rows and bm of `units` x alpha, the matching W2 columns / alpha
      conv1         conv1 channel `units` (an int): K1w row and K1b x alpha, that input channel of K2w / alpha
      conv2         conv2 channel `units` (an int): K2w row and K2b x alpha, that channel's head columns of Fw / alpha"""
    p = {k: v.clone() for k, v in post.items()}
    k, a = KEYS[arch], float(alpha)
    if how == "sample":
        p[k["W1"]][s] *= a
        p[k["b1"]][s] *= a
        p[k["W2"]][s] /= a
    elif how in ("units", "layer1"):
        p[k["W1"]][s, units] *= a
        p[k["b1"]][s, units] *= a
        p[k["W2" if arch == "fc" else "Wm"]][s, :, units] /= a
    elif how == "layer2":
        p[k["Wm"]][s, units] *= a
        p[k["bm"]][s, units] *= a
        p[k["W2"]][s, :, units] /= a
    elif how == "conv1":
        p[k["K1w"]][s, units] *= a
        p[k["K1b"]][s, units] *= a
        p[k["K2w"]][s, :, units] /= a
    elif how == "conv2":
        np2 = p[k["Fw"]].shape[-1] // p[k["K2w"]].shape[1]          # the head reads the conv2 output flattened channel-major
        p[k["K2w"]][s, units] *= a
        p[k["K2b"]][s, units] *= a
        p[k["Fw"]][s, :, units * np2:(units + 1) * np2] /= a
    else:
        raise ValueError(how)
    return p


def rescale_guide(loc, scl, arch, alpha, units=slice(3, 19)):
    """An SVI guide whose loc and sigma = softplus(raw scale) are rescaled block-wise as `rescale` does for one sample (fc: hidden units,
    conv: conv2 channel `units`, an int); the raw scale is softplus^-1 of the new sigma (fp64)."""
    sig = {k: torch.nn.functional.softplus(v.double()) for k, v in scl.items()}
    loc = {k: v.double().clone() for k, v in loc.items()}
    a = float(alpha)
    if arch == "conv":
        np2 = loc["model.7.weight"].shape[-1] // loc["model.3.weight"].shape[0]
        for d in (loc, sig):
            d["model.3.weight"][units] *= a
            d["model.3.bias"][units] *= a
            d["model.7.weight"][:, units * np2:(units + 1) * np2] /= a
    else:
        for d in (loc, sig):
            d["model.1.weight"][units] *= a
            d["model.1.bias"][units] *= a
            d[KEYS[arch]["W2" if arch == "fc" else "Wm"]][:, units] /= a
    raw = {k: torch.where(v > 20, v, torch.log(torch.expm1(v))).float() for k, v in sig.items()}
    return {k: v.float() for k, v in loc.items()}, raw


def pieces(v, n):
    """The n fp16 pieces of fp32 values v (already scaled), as the kernels split them (rbnn_common.hpp split3_plain_pair: p0 = f16(v),
    p1 = f16(v - p0), p2 = f16(v - p0 - p1), round to nearest even, the remainders exact in fp32), summed in fp64."""
    r = v.astype(np.float32)
    out = np.zeros(v.shape, np.float64)
    for _ in range(n):
        p = r.astype(np.float16).astype(np.float32)
        out += p
        r = r - p
    return out


def emulated_image(post, arch, n=3):
    """The weights as the images carry them: every weight tensor at one scale 2^scale_exp(max |tensor|) (conv1: one per sample), n fp16
    pieces each, reconstructed in fp64.  Biases and the conv head stay fp32 (the kernels read them so)."""
    from robustbnns_amd.posterior import scale_exp
    k = KEYS[arch]
    imaged = [k["K2w"]] if arch == "conv" else [k["W1"], k["W2"]] + ([k["Wm"]] if arch == "fc2" else [])
    out = {key: v.double() for key, v in post.items()}
    for key in imaged:
        e = scale_exp(float(post[key].abs().max()))
        out[key] = torch.from_numpy(pieces(post[key].numpy() * 2.0 ** e, n) * 2.0 ** -e)
    if arch == "conv":
        w = post[k["K1w"]]
        for s in range(w.shape[0]):
            e = scale_exp(float(w[s].abs().max()))
            out[k["K1w"]][s] = torch.from_numpy(pieces(w[s].numpy() * 2.0 ** e, n) * 2.0 ** -e)
    return out


def stacked(post, device="cpu", act="leaky"):
    """StackedPosterior / ConvStackedPosterior of a stacked state dict, its geometry read off the weights."""
    from robustbnns_amd.conv import ConvStackedPosterior
    from robustbnns_amd.posterior import StackedPosterior
    if "model.0.weight" in post:
        cin, H, C = post["model.0.weight"].shape[2], post["model.3.weight"].shape[1], post["model.7.weight"].shape[1]
        return ConvStackedPosterior(act, (1, 28, 28) if cin == 1 else (3, 32, 32), C, H, post, device)
    arch = "fc2" if "model.5.weight" in post else "fc"
    W1, W2 = post["model.1.weight"], post[KEYS[arch]["W2"]]
    D = int(np.prod(W1.shape[2:]))
    return StackedPosterior(arch, act, (1, D, 1), W2.shape[1], W1.shape[1], post, device)


SMALL = {  # arch: (D or shape, H, C, S, N, std)
    "fc": ((1, 28, 28), 256, 10, 2, 24, 0.05), "fc2": ((1, 28, 28), 256, 10, 2, 24, 0.05), "conv": ((1, 28, 28), 16, 10, 2, 4, 0.05)}


def small_problem(arch):
    shape, H, C, S, N, std = SMALL[arch]
    D = int(np.prod(shape))
    post = (O.synthetic_posterior("conv", D, H, C, S, std, in_ch=shape[0], head=((shape[1] - 4) // 2 - 5) ** 2 * H) if arch == "conv"
            else O.synthetic_posterior(arch, D, H, C, S, std))
    x, y = O.synthetic_inputs(N, shape, C, seed=D + H)
    return post, x, y, S


def units_of(arch):
    return 5 if arch == "conv" else slice(3, 19)


@pytest.mark.parametrize("arch,how", [(a, h) for a in RESCALINGS for h in RESCALINGS[a]])
def test_fp64_oracle_is_invariant_under_the_rescalings(arch, how):
    post, x, y, S = small_problem(arch)
    p64 = O.cast(post, torch.float64)
    lab = y.argmax(-1)
    f0, g0 = O.bnn_forward(x.double(), p64, arch, "leaky", S), O.meanprob_gradients(x.double(), lab, p64, arch, "leaky", S)
    for act in ("leaky", "relu"):
        f0 = O.bnn_forward(x.double(), p64, arch, act, S)
        for alpha in ALPHAS:
            q = O.cast(rescale(post, arch, how, alpha, units=units_of(arch)), torch.float64)
            assert float(rel_err_points(O.bnn_forward(x.double(), q, arch, act, S), f0).max()) < 1e-12, (act, alpha)
            assert float(rel_err_points(O.ensemble_forward(x.double(), q, arch, act, S),
                                        O.ensemble_forward(x.double(), p64, arch, act, S)).max()) < 1e-12, (act, alpha)
    for alpha in (ALPHAS[0], ALPHAS[-1]):
        q = O.cast(rescale(post, arch, how, alpha, units=units_of(arch)), torch.float64)
        assert float(rel_err_points(O.meanprob_gradients(x.double(), lab, q, arch, "leaky", S), g0).max()) < 1e-12


@pytest.mark.parametrize("arch,how", [(a, h) for a in RESCALINGS for h in RESCALINGS[a]])
def test_guard_refuses_every_rescaling_whose_emulated_images_miss_the_bar(arch, how):
    """Per alpha: the error of the emulated triple (3 pieces) and split (2 pieces) images against fp64 of the unscaled posterior (fc / fc2:
    the MEAN_PROB gradient off the kinks; conv: the forward probabilities) — every alpha at which it reaches 1e-5 is refused; 2^8 (the slices
    stay within 2^12 of the scale) is accepted, everything from 2^16 on is refused."""
    post, x, y, S = small_problem(arch)
    p64 = O.cast(post, torch.float64)
    lab = y.argmax(-1)
    xd = x.double()
    if arch == "conv":
        ref = O.bnn_forward(xd, p64, arch, "leaky", S)
        err_of = lambda q: float(rel_err_points(O.bnn_forward(xd, q, arch, "leaky", S), ref).max())
    else:
        ok = O.kink_margin(xd, p64, arch, "leaky", S) > KINK
        ref = O.meanprob_gradients(xd, lab, p64, arch, "leaky", S)
        err_of = lambda q: float(rel_err_points(O.meanprob_gradients(xd, lab, q, arch, "leaky", S), ref)[ok].max())
    assert stacked(post).range_ok()
    missed = []
    for alpha in ALPHAS:
        q = rescale(post, arch, how, alpha, units=units_of(arch))
        accepted = stacked(q).range_ok()
        errs = {n: err_of(emulated_image(q, arch, n)) for n in (3, 2)}
        print(f"[rescale guard {arch} {how}] alpha 2^{int(np.log2(alpha))}: emulated triple {errs[3] / TOL:.3g} / split {errs[2] / TOL:.3g} "
              f"x 1e-5; guard {'accepts' if accepted else 'refuses'}")
        if max(errs.values()) >= TOL:
            missed.append(alpha)
            assert not accepted, f"alpha {alpha}: the emulated images miss 1e-5 and the guard accepts"
        assert accepted == (alpha < 2.0 ** 12)
    assert missed and max(ALPHAS) in missed                  # the emulation does see the loss it guards against


@pytest.mark.parametrize("arch", ["fc", "fc2", "conv"])
def test_guard_on_rescaled_svi_guides(arch):
    """SviGuide / ConvSviGuide decide range_ok on the bounds |loc| + EPS_MAX softplus(scale) in their one load-time sync: a block-wise
    rescaled guide is refused from 2^16 on and accepted at 2^8."""
    from robustbnns_amd.conv import ConvSviGuide
    from robustbnns_amd.posterior import SviGuide
    post, _, _, _ = small_problem(arch)
    loc = {k: v[0] for k, v in post.items()}
    scl = {k: torch.full_like(v, -3.0) for k, v in loc.items()}
    make = (lambda lc, sc: ConvSviGuide(lc, sc, "cpu")) if arch == "conv" else (lambda lc, sc: SviGuide(lc, sc, arch, "cpu"))
    assert make(loc, scl).range_ok
    for alpha in ALPHAS:
        g = make(*rescale_guide(loc, scl, arch, alpha, units=units_of(arch)))
        assert g.range_ok == (alpha < 2.0 ** 12), alpha


def test_guard_accepts_the_trained_fixtures_bench_posteriors_and_the_suites_synthetic_ones(golden):
    """What must keep its mode: every tests/golden/trained_* posterior, the posteriors and guides bench.py builds for each workload (stored
    posteriors capped at 100 samples here), and the i.i.d. synthetic posteriors the GPU tier asserts triple / split on (including
    test_hip_triple's and test_hip_parity's 0.1 % outliers at 100x)."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from robustbnns_amd.conv import ConvSviGuide
    from robustbnns_amd.posterior import SviGuide
    import test_hip_edges as E
    names = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trained_*.npz")))
    assert len(names) >= 5
    for name in names:
        assert stacked(golden(name).posterior()).range_ok(), name
    for wname, w in bench.WORKLOADS.items():
        w = dict(w, S=min(w["S"], 100))
        _, _, post = bench.make_problem(w, 0, "cpu")
        assert stacked(post).range_ok(), wname
        loc, scale = bench.make_guide(w, 0)
        g = ConvSviGuide(loc, scale, "cpu") if w["arch"] == "conv" else SviGuide(loc, scale, w["arch"], "cpu")
        assert g.range_ok, wname
    for arch, act, shape, H, C, S, N, std in E.A_CASES:
        assert stacked(O.synthetic_posterior(arch, int(np.prod(shape)), H, C, S, std)).range_ok(), (arch, shape, H, C, S)
    import test_hip_round2 as R2
    for act, shape, C, Hc, S, N, std, precision in R2.CONV_CASES + E._d_cases():
        if precision != "exact":
            assert stacked(E._conv_post(shape, Hc, C, S, std)).range_ok(), (shape, Hc, C, S)
    post = O.synthetic_posterior("fc", 784, 256, 10, 5, 0.03)
    g = torch.Generator().manual_seed(17)
    for k in ("model.1.weight", "model.3.weight"):
        m = torch.rand(post[k].shape, generator=g) < 1e-3
        post[k] = torch.where(m, post[k] * 100.0, post[k])
    assert stacked(post).range_ok()
