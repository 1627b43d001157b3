"""GPU parity tests (-m gpu): the HIP path, called through the C-ABI, against
  (1) the golden vectors produced by the reference's own functions (tests/golden/*.npz),
  (2) the fp64 oracle on seeded inputs at sizes it finishes in seconds (ragged N, every H config),
  (3) size-independent properties at BASELINE.json's full size (N=10 000, S=100).
Tolerance: 1e-5 relative to each point's largest component (north star).  Both precision modes of the two GEMMs
are held to it: "exact" (fp32 MFMA) and "split" (error-compensated half pairs on the f16 MFMA pipe, what "fast"
picks for fc / relu|leaky / hidden % 128 == 0 / classes <= 10) — every case the split kernels cover runs in both.
Adversarial images: equal except where |g| < tau * max|g| (a sign flip there is within fp32 noise)."""
import os

import numpy as np
import pytest
import torch

from conftest import cancellation_condition, pgd_whole_attack_statistic, rel_err, rel_err_points
from oracle import bnn_oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("built_library")]
TOL = 1e-5
TAU = 1e-3
KINK = 2e-6      # points with a hidden pre-activation this close to 0 are excluded: act' jumps there (oracle.kink_margin)
DEV = "cuda:0"
FC_CASES = ["halfmoons_fc_h64_s10_n100", "mnist_fc_h32_s8_n8_leaky", "mnist_fc_h32_s8_n8_relu", "mnist_fc_h16_s4_n6_sigm",
            "mnist_fc_h16_s4_n6_tanh", "mnist_fc_h512_s8_n8_leaky", "mnist_fc_h512_s8_n8_relu",
            "mnist_fc2_h32_s4_n6_leaky", "halfmoons_fc2_h32_s6_n40"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from robustbnns_amd import _hip
    _hip.load()


def split_covers(arch, act, H, C):
    return arch in ("fc", "fc2") and max(32, H) % 128 == 0 and C <= 10


def exact_covers(H):
    H = max(32, H)
    return H in (32, 64) or H % 128 == 0                               # include/robustbnns_hip.h: 32, 64 or k*128


def modes_for(arch, act, H, C):
    return ["fast", "exact"] if split_covers(arch, act, H, C) and exact_covers(H) else ["fast"]


# every fixture also in "auto" — what a caller of the package gets: `lowdim_kernel` / the lowdim fc2 launches on the half-moons fixtures (the
# kernels BASELINE config 1 is benchmarked on meet the reference's own forward_probs / loss_gradients / meanprob_grad arrays here), triple on the
# h512 ones, the fp32 MFMA elsewhere
GOLDEN_MODES = [(n, m) for n in FC_CASES for m in (["auto", "fast", "exact"] if "_fc_h512_" in n else ["auto", "fast"])]


def expected_precision(name, precision):
    if precision == "auto":
        return "lowdim" if name.startswith("halfmoons_") else ("triple" if "_fc_h512_" in name else "exact")
    return "split" if precision == "fast" and "_fc_h512_" in name else "exact"


def make_bnn(g):
    from robustbnns_amd.model_bnn import BNN
    m = g.meta
    bnn = BNN(m["dataset"], m["hidden"], m["act"], m["arch"], "hmc", None, None, m["S"], 0, tuple(m["shape"]), m["n_classes"])
    bnn.set_posterior_samples(g.posterior(), DEV)
    return bnn


def adv_equal(adv, ref, grad):
    adv, ref, grad = (torch.as_tensor(v).cpu().reshape(len(ref), -1) for v in (adv, ref, grad))
    safe = grad.abs() > TAU * grad.abs().max(dim=1, keepdim=True)[0]
    bad = ((adv - ref).abs() > 1e-6) & safe
    assert not bad.any(), f"{int(bad.sum())} non-marginal pixels differ"


# ------------------------------------------------------------------ (1) golden vectors, through the reference's call surface
@pytest.mark.parametrize("name,precision", GOLDEN_MODES)
def test_golden_forward_and_gradients(golden, name, precision, monkeypatch):
    from robustbnns_amd import lossGradients
    monkeypatch.setenv("RBNN_PRECISION", precision)
    g = golden(name); m = g.meta; bnn = make_bnn(g); x, y = g.t("x"), g.t("y")
    assert bnn._engine.precision == expected_precision(name, precision)
    assert rel_err(bnn.forward(x.to(DEV), n_samples=m["S"]).cpu(), g.t("forward_probs")) < TOL
    seeds = [int(s) for s in g.arr["forward_seeds"]]
    assert rel_err(bnn.forward(x.to(DEV), n_samples=len(seeds), seeds=seeds).cpu(), g.t("forward_probs_seeds")) < TOL
    assert rel_err(bnn.forward(x.to(DEV), n_samples=1).cpu(), g.t("forward_probs_s1")) < TOL
    with pytest.raises(ValueError):
        bnn.forward(x.to(DEV), n_samples=2, seeds=[0])
    with pytest.raises(IndexError):
        bnn.forward(x.to(DEV), n_samples=1, seeds=[m["S"]])
    eng = bnn._engine
    assert rel_err(eng.loss_gradients(x, y, m["S"]).cpu(), g.t("loss_gradients")) < TOL
    assert rel_err(eng.loss_gradients(x, y, m["S_half"]).cpu(), g.t("loss_gradients_half")) < TOL
    lg = lossGradients.loss_gradient(bnn, x[1].to(DEV), y[1].to(DEV), n_samples=m["S"])
    assert lg.shape == x[1].shape and rel_err(lg.cpu()[None], g.t("loss_gradients")[1:2]) < TOL
    from robustbnns_amd import _hip
    G = eng.gradient(eng.pad_inputs(x), y.argmax(-1).int().to(DEV), None, m["S"], _hip.LOSS_MEAN_PROB)
    assert rel_err(G[:, :eng.post.D].cpu().reshape(x.shape), g.t("meanprob_grad")) < TOL


@pytest.mark.parametrize("name,precision", GOLDEN_MODES)
def test_golden_attacks_and_evaluation(golden, name, precision, monkeypatch):
    from robustbnns_amd import adversarialAttacks as A
    monkeypatch.setenv("RBNN_PRECISION", precision)
    g = golden(name); m = g.meta; bnn = make_bnn(g); x, y = g.t("x"), g.t("y")
    assert bnn._engine.precision == expected_precision(name, precision)
    lab = y.argmax(-1)
    hyper = {"epsilon": m["eps"]}
    ref_g = g.t("meanprob_grad")
    adv = A.fgsm_attack(bnn, x.to(DEV), lab.to(DEV), hyper, n_samples=m["S"])
    assert adv.shape == x.shape
    adv_equal(adv, g.t("fgsm"), ref_g)
    adv_equal(A.fgsm_attack(bnn, x.to(DEV), lab.to(DEV), None, n_samples=m["S"]), g.t("fgsm_default_eps"), ref_g)
    one = A.fgsm_attack(bnn, x[2:3].clone(), lab[2:3], hyper, n_samples=m["S"])            # the reference's batch-1 call shape
    adv_equal(one, g.t("fgsm")[2:3], ref_g[2:3])
    idx = torch.from_numpy(g.arr["pgd_idx"])
    pg = A.pgd_attack(bnn, x[idx].to(DEV), lab[idx].to(DEV), hyper, n_samples=m["S"]).cpu()
    assert float((pg - g.t("pgd")).abs().max()) <= 2 * m["eps"] + 1e-6
    # 40 compounding sign steps: the EXACT statement is tests/test_hip_round3.py::test_pgd_single_steps_along_the_reference_trajectory (one
    # step at a time along the reference's own iterates, zero non-marginal pixels); the whole-attack difference is a reported statistic
    pgd_whole_attack_statistic(name + " [" + precision + "]", pg, g.t("pgd"))
    if "pgd_default" in g.arr:
        pg = A.pgd_attack(bnn, x[idx].to(DEV), lab[idx].to(DEV), None, n_samples=m["S"]).cpu()
        pgd_whole_attack_statistic(name + " default hyperparameters", pg, g.t("pgd_default"))
    oa, aa, rob = A.attack_evaluation(bnn, x, g.t("fgsm"), y, DEV, n_samples=m["S"])
    assert (oa, aa) == (float(g.arr["eval_orig_acc"]), float(g.arr["eval_adv_acc"]))
    assert float((rob.cpu() - g.t("eval_softmax_rob")).abs().max()) < 1e-6
    rob2 = A.softmax_robustness(bnn.forward(x.to(DEV), m["S"]), bnn.forward(g.t("fgsm").to(DEV), m["S"]))
    assert float((rob2.cpu() - g.t("eval_softmax_rob")).abs().max()) < 1e-6


def test_golden_deterministic_and_ensemble(golden):
    from robustbnns_amd import adversarialAttacks as A
    from robustbnns_amd.model_ensemble import Ensemble_NN
    from robustbnns_amd.model_nn import NN
    g = golden("mnist_det_ens_fc_h32_m4_n6"); m = g.meta; post = g.posterior()
    x, y = g.t("x"), g.t("y"); lab = y.argmax(-1); M = m["M"]; hyper = {"epsilon": m["eps"]}
    ens = Ensemble_NN("mnist", m["hidden"], m["act"], m["arch"], 1, 0.01, tuple(m["shape"]), m["n_classes"], M)
    ens.device = DEV
    for i in range(M):
        net = NN("mnist", tuple(m["shape"]), m["n_classes"], m["hidden"], m["act"], m["arch"], 0.01, 1)
        net.load_state_dict({k: v[i] for k, v in post.items()})
        net.device = DEV
        ens.ensemble_models[str(i)] = net
    nn0 = ens.ensemble_models["0"]
    assert rel_err(nn0.forward(x.to(DEV)).cpu(), g.t("nn0_logits")) < TOL
    assert rel_err(ens.forward(x.to(DEV), n_samples=M).cpu(), g.t("ens_logits")) < TOL
    assert rel_err(ens.forward(x.to(DEV), n_samples=2).cpu(), g.t("ens_logits_2")) < TOL
    with pytest.raises(ValueError):
        ens.forward(x.to(DEV), n_samples=M + 1)
    ge = O.meanprob_gradients(x, lab, post, m["arch"], m["act"], M, kind="ensemble")
    g1 = O.meanprob_gradients(x, lab, post, m["arch"], m["act"], 1, kind="ensemble")
    adv_equal(A.fgsm_attack(ens, x.to(DEV), lab.to(DEV), hyper, n_samples=M), g.t("ens_fgsm"), ge)
    adv_equal(A.fgsm_attack(nn0, x.to(DEV), lab.to(DEV), hyper, n_samples=None), g.t("nn0_fgsm"), g1)
    # PGD through the call surface: the step itself is pinned one iteration at a time along the reference's own ensemble / deterministic-NN
    # iterates (tests/test_hip_round3.py::test_pgd_single_steps_along_the_reference_trajectory, fixture pgd_traj_det_ens_fc_h32_m4_n6: the
    # same nets); here the whole 40-step attacks of all points, held to the whole-attack gate (and printed)
    pgd_whole_attack_statistic("mnist_det_ens ensemble", A.pgd_attack(ens, x.to(DEV), lab.to(DEV), hyper, n_samples=M), g.t("ens_pgd"))
    pgd_whole_attack_statistic("mnist_det_ens deterministic NN", A.pgd_attack(nn0, x.to(DEV), lab.to(DEV), hyper, n_samples=None), g.t("nn0_pgd"))
    oa, aa, rob = A.attack_evaluation(ens, x, g.t("ens_fgsm"), y, DEV, n_samples=M)
    assert (oa, aa) == (float(g.arr["ens_eval_orig_acc"]), float(g.arr["ens_eval_adv_acc"]))
    assert float((rob.cpu() - g.t("ens_eval_softmax_rob")).abs().max()) < 1e-6
    oa, aa, rob = A.attack_evaluation(nn0, x, g.t("nn0_fgsm"), y, DEV, n_samples=None)
    assert (oa, aa) == (float(g.arr["nn0_eval_orig_acc"]), float(g.arr["nn0_eval_adv_acc"]))
    assert float((rob.cpu() - g.t("nn0_eval_softmax_rob")).abs().max()) < 1e-6


def test_baseline_attacks_driver(golden, tmp_path, monkeypatch):
    """plot_baseline_attacks.build_baseline_attacks_df: NN / BNN / ensemble sections, the reference's schema and CSV path;
    every cell equals the (golden-pinned) attack + attack_evaluation calls it is made of."""
    from robustbnns_amd import adversarialAttacks as A, plot_baseline_attacks as PB, savedir
    from robustbnns_amd.model_ensemble import Ensemble_NN
    from robustbnns_amd.model_nn import NN
    g = golden("mnist_det_ens_fc_h32_m4_n6"); m = g.meta; post = g.posterior(); M = m["M"]
    x, y = g.t("x"), g.t("y")
    ens = Ensemble_NN("mnist", m["hidden"], m["act"], m["arch"], 1, 0.01, tuple(m["shape"]), m["n_classes"], M)
    ens.device = DEV
    for i in range(M):
        net = NN("mnist", tuple(m["shape"]), m["n_classes"], m["hidden"], m["act"], m["arch"], 0.01, 1)
        net.load_state_dict({k: v[i] for k, v in post.items()})
        net.device = DEV
        ens.ensemble_models[str(i)] = net
    nn0 = ens.ensemble_models["0"]
    gb = golden("mnist_fc_h32_s8_n8_leaky"); bnn = make_bnn(gb)
    monkeypatch.chdir(tmp_path)
    df = PB.build_baseline_attacks_df(nn0, bnn, ens, "mnist", DEV, "fgsm", x, y, bayesian_attack_samples=(1, 4),
                                      bayesian_defence_samples=(1, 8), n_samples_list=(1, M))
    N = len(x)
    assert list(df.columns) == ["attack_method", "epsilon", "test_acc", "adv_acc", "softmax_rob", "attack_samples",
                                "defence_samples", "model_type"]
    assert len(df) == N * (1 + 2 * 2 + 2) and set(df["attack_method"]) == {"fgsm"} and set(df["epsilon"]) == {0.3}
    assert list(df["model_type"].unique()) == ["nn", "bnn", "ensemble"]
    nn_rows = df[df["model_type"] == "nn"]
    assert float(nn_rows["test_acc"].iloc[0]) == float(g.arr["nn0_eval_orig_acc"])       # the reference's own numbers (eps 0.3 default)
    cell = df[(df["model_type"] == "bnn") & (df["attack_samples"] == 4) & (df["defence_samples"] == 8)]
    adv = A.attack(net=bnn, x_test=x, y_test=y, dataset_name="mnist", device=DEV, method="fgsm", filename=bnn.name, n_samples=4)
    oa, aa, rob = A.attack_evaluation(net=bnn, x_test=x, x_attack=adv, y_test=y, device=DEV, n_samples=8)
    assert (float(cell["test_acc"].iloc[0]), float(cell["adv_acc"].iloc[0])) == (oa, aa)
    assert np.abs(cell["softmax_rob"].to_numpy() - rob.cpu().numpy()).max() < 1e-6
    e_rows = df[(df["model_type"] == "ensemble") & (df["attack_samples"] == M)]
    assert float(e_rows["test_acc"].iloc[0]) == float(g.arr["ens_eval_orig_acc"]) and (e_rows["defence_samples"] == M).all()
    back = PB.load_baseline_attacks_df("mnist", "fgsm", "")
    assert len(back) == len(df) and list(back.columns) == list(df.columns)
    assert os.path.exists(savedir.TESTS + "/mnist_baseline_attacks_fgsm.csv")


def test_half_moons_grid_driver(tmp_path, monkeypatch):
    """grid_search_halfMoons.serial_compute_grads / grid_attack over a 2 x 2 model grid stored in the reference's on-disk HMC
    format (<name>/<name>_weights_<i>.pt): every cell equals the direct loss_gradients / attack call and the fp64 oracle."""
    from robustbnns_amd import adversarialAttacks as A, grid_search_halfMoons as GS, savedir
    monkeypatch.chdir(tmp_path)
    shape, C, S = (1, 2, 1), 2, 6
    x, y = O.synthetic_inputs(40, shape, C, seed=3)
    rel = str(tmp_path) + "/models/"
    posts = {}
    for arch, hid in (("fc2", 32), ("fc2", 128)):
        for n_inp in (100, 200):
            bnn = GS.MoonsBNN(hid, "leaky", arch, "hmc", None, None, S, 10, n_inp, shape, C)
            assert bnn.name == f"half_moons_bnn_hmc_hid={hid}_act=leaky_arch={arch}_inp={n_inp}_samp={S}_warm=10_stepsize=0.001_numsteps=10"
            post = O.synthetic_posterior(arch, 2, hid, C, S, 1.5 / hid ** 0.5)     # O(1) pre-activations: fp32 itself stays well inside the bar
            post = {k: v + 0.01 * n_inp / 100 for k, v in post.items()}            # different weights per grid cell
            bnn.set_posterior_samples(post, "cpu")
            bnn.save(rel_path=rel)
            posts[bnn.name] = post
    grid = dict(hidden_size=[32, 128], activation=["leaky"], architecture=["fc2"], inference=["hmc"], epochs=[None], lr=[None],
                n_samples=[S], warmup=[10], n_inputs=[100, 200])
    grads = GS.serial_compute_grads(**grid, posterior_samples=[S], rel_path=rel, x_test=x, y_test=y, device=DEV)
    assert len(grads) == 4
    for (name, s_), g in grads.items():
        arch, hid = "fc2", int(name.split("hid=")[1].split("_")[0])
        p64 = O.cast(posts[name], torch.float64)
        ref = O.loss_gradients(x.double(), y, p64, arch, "leaky", s_)
        ok = O.kink_margin(x.double(), p64, arch, "leaky", s_) > KINK
        assert g.shape == (40, 2) and int(ok.sum()) >= 36 and rel_err(torch.from_numpy(g).reshape(ref.shape)[ok], ref[ok]) < TOL
        assert os.path.exists(savedir.DATA + name + "/" + name + "_samp=" + str(s_) + "_lossGrads.pkl")
    advs = GS.grid_attack("fgsm", **grid, posterior_samples=[2, S], x_test=x, y_test=y, device=DEV, rel_path=rel)
    assert len(advs) == 8
    for (name, s_), adv in advs.items():
        hid = int(name.split("hid=")[1].split("_")[0])
        p64 = O.cast(posts[name], torch.float64)
        gm = O.meanprob_gradients(x.double(), y.argmax(-1), p64, "fc2", "leaky", s_)
        ok = O.kink_margin(x.double(), p64, "fc2", "leaky", s_) > KINK
        adv_equal(adv[ok], torch.clamp(x + 0.3 * gm.sign().float(), 0, 1)[ok], gm[ok])
        assert torch.equal(A.load_attack("fgsm", name, n_samples=s_).cpu(), adv.cpu())


# ------------------------------------------------------------------ (2) fp64 oracle, every tile configuration, ragged sizes
ORACLE_CASES = [  # arch, act, shape, C, H, S, N, std
    ("fc", "leaky", (1, 28, 28), 10, 512, 7, 333, 0.05), ("fc", "relu", (1, 28, 28), 10, 512, 5, 257, 0.05),
    ("fc", "leaky", (1, 28, 28), 10, 1024, 2, 65, 0.05), ("fc", "leaky", (1, 28, 28), 10, 256, 3, 129, 0.05),
    ("fc", "tanh", (1, 28, 28), 10, 128, 3, 70, 0.05), ("fc", "sigm", (1, 28, 28), 10, 64, 3, 40, 0.05),
    ("fc", "leaky", (1, 28, 28), 10, 32, 9, 1, 0.05), ("fc", "leaky", (1, 2, 1), 2, 16, 4, 300, 0.5),
    ("fc", "leaky", (3, 8, 8), 16, 64, 3, 50, 0.1), ("fc", "relu", (1, 5, 5), 3, 128, 2, 17, 0.2),
    ("fc2", "leaky", (1, 28, 28), 10, 512, 3, 200, 0.05), ("fc2", "relu", (1, 28, 28), 10, 64, 3, 33, 0.08),
    ("fc2", "tanh", (1, 2, 1), 2, 32, 6, 40, 0.4), ("fc2", "sigm", (1, 28, 28), 10, 128, 2, 20, 0.08),
]


ORACLE_CASES += [  # split-mode shapes: 4-column-tile grouping with a partial group, 2 and 10 classes, big / tiny weights and inputs
    ("fc", "leaky", (1, 10, 10), 2, 128, 3, 300, 0.1), ("fc", "relu", (3, 8, 8), 7, 384, 2, 77, 0.1),
    ("fc", "leaky", (1, 28, 28), 10, 640, 2, 513, 0.02), ("fc", "leaky", (1, 28, 28), 10, 128, 17, 30, 0.05),
]
ORACLE_CASES += [  # point-tile boundaries of the 256-point blocks and single-sample / single-point jobs in the split kernels
    ("fc", "leaky", (1, 28, 28), 10, 256, 1, 1, 0.05), ("fc", "relu", (1, 28, 28), 10, 128, 2, 255, 0.05),
    ("fc", "leaky", (1, 28, 28), 10, 128, 9, 256, 0.05), ("fc", "leaky", (1, 14, 14), 4, 256, 11, 257, 0.08),
]
ORACLE_CASES += [("fc2", "leaky", (1, 28, 28), 10, 256, 5, 300, 0.05), ("fc2", "relu", (1, 14, 14), 4, 128, 9, 257, 0.1),
                 ("fc2", "leaky", (1, 2, 1), 2, 128, 6, 70, 0.15)]
ORACLE_CASES += [("fc2", "leaky", (1, 28, 28), 10, 1024, 2, 70, 0.03)]       # the reference's saved model_3 / model_7 shape
ORACLE_CASES += [("fc", "sigm", (1, 28, 28), 10, 256, 3, 140, 0.05), ("fc", "tanh", (1, 14, 14), 5, 128, 4, 90, 0.1),
                 ("fc2", "tanh", (1, 28, 28), 10, 256, 3, 130, 0.05), ("fc2", "sigm", (1, 8, 8), 3, 128, 2, 50, 0.2)]
ORACLE_MODES = [c + (m,) for c in ORACLE_CASES for m in modes_for(c[0], c[1], c[4], c[3])
                if m != "exact" or max(32, c[4]) % 512 == 0 or max(32, c[4]) & (max(32, c[4]) - 1) == 0]
# exact at the hidden sizes k*128 that are neither a power of two nor k*512 (640): appended, so that every case above keeps its id
ORACLE_MODES += [c + ("exact",) for c in ORACLE_CASES if "exact" in modes_for(c[0], c[1], c[4], c[3]) and c + ("exact",) not in ORACLE_MODES]


@pytest.mark.parametrize("arch,act,shape,C,H,S,N,std,precision", ORACLE_MODES)
def test_against_fp64_oracle(arch, act, shape, C, H, S, N, std, precision):
    from robustbnns_amd import AttackEngine, StackedPosterior, _hip
    D = int(np.prod(shape))
    post = O.synthetic_posterior(arch, D, H, C, S, std)
    x, y = O.synthetic_inputs(N, shape, C, seed=H + N)
    lab = y.argmax(-1)
    p64 = O.cast(post, torch.float64)
    eng = AttackEngine(StackedPosterior(arch, act, shape, C, H, post, DEV), precision=precision)
    assert eng.precision == ("split" if precision == "fast" and split_covers(arch, act, H, C) else "exact")
    assert rel_err(eng.forward(x, S).cpu(), O.bnn_forward(x.double(), p64, arch, act, S)) < TOL
    assert rel_err(eng.forward(x, S, logits=True).cpu(), O.ensemble_forward(x.double(), p64, arch, act, S)) < TOL
    ok = O.kink_margin(x.double(), p64, arch, act, S) > KINK                  # gradients: away from activation kinks
    assert int((~ok).sum()) <= max(3, N // 20)
    assert rel_err(eng.loss_gradients(x, y, S).cpu()[ok], O.loss_gradients(x.double(), y, p64, arch, act, S)[ok]) < TOL
    labd = lab.int().to(DEV)
    for mode, kind in ((_hip.LOSS_MEAN_PROB, "bnn"), (_hip.LOSS_MEAN_LOGIT, "ensemble")):
        G = eng.gradient(eng.pad_inputs(x), labd, None, S, mode)[:, :D].cpu().reshape(x.shape)
        ref = O.meanprob_gradients(x.double(), lab, p64, arch, act, S, kind=kind)
        # 1e-5 per point — except where the samples' contributions to the expected gradient cancel k : 1 with k 2^-23 > 1e-5: there one rounding
        # of the shared loss gradient moves the sum by more than the bar in ANY fp32 evaluation (conftest.cancellation_condition; the half-moons-sized
        # case has one such point of 300, at 777 : 1, where torch's own fp32 evaluation of the oracle sits 1.9e-5 from fp64)
        bound = torch.clamp(2.0 ** -23 * cancellation_condition(x, lab, post, arch, act, S, kind), min=TOL)
        e = rel_err_points(G, ref)
        assert not bool((e > bound)[ok].any()), (kind, float((e / bound)[ok].max()), int((e / bound)[ok].argmax()))
        assert int((bound > TOL)[ok].sum()) <= max(1, N // 100)
        adv = eng.fgsm(x, y, S, 0.1, mode=mode).cpu()
        adv_equal(adv[ok], torch.clamp(x + 0.1 * ref.sign().float(), 0, 1)[ok], ref[ok])
    # a seeds subset in shuffled order == the same samples gathered on the host
    if S >= 3:
        sub = [S - 1, 0, 1]
        assert rel_err(eng.forward(x, 3, seeds=sub).cpu(), O.bnn_forward(x.double(), p64, arch, act, 3, seeds=sub)) < TOL


@pytest.mark.parametrize("k", [-9, 7])
def test_split_mode_operand_scales(k):
    """Split precision carries every operand with a power-of-two scale taken from its largest magnitude: weights
    2^k larger and inputs 2^k smaller (same products) must give the same parity, and so must vanishing gradients
    (confident predictions: |dZ| down to 1e-12 — lossGradients.compute_vanishing_norms_idxs lives on those)."""
    from robustbnns_amd import AttackEngine, StackedPosterior, _hip
    D, H, C, S, N = 784, 256, 10, 4, 150
    post = O.synthetic_posterior("fc", D, H, C, 1, 0.05)
    g = torch.Generator().manual_seed(9)                            # a tight posterior (samples agree) with a sharp output layer:
    post = {k_: v.repeat(S, *([1] * (v.dim() - 1))) + 1e-3 * torch.randn((S,) + tuple(v.shape[1:]), generator=g) for k_, v in post.items()}
    post["model.3.weight"] = post["model.3.weight"] * 40.0          # confident on ~half of the points: gradients from 1e-10 to 1
    post["model.1.weight"] = post["model.1.weight"] * 2.0 ** k
    x, y = O.synthetic_inputs(N, (1, 28, 28), C, seed=5)
    x = x * 2.0 ** (-k)
    p64 = O.cast(post, torch.float64)
    eng = AttackEngine(StackedPosterior("fc", "leaky", (1, 28, 28), C, H, post, DEV), precision="split")
    ref_p = O.bnn_forward(x.double(), p64, "fc", "leaky", S)
    assert rel_err(eng.forward(x, S).cpu(), ref_p) < TOL
    # use the predicted class as the label: p - y is then tiny wherever the net is confident (no fp32 cancellation noise in it)
    lab = ref_p.argmax(-1)
    ok = O.kink_margin(x.double(), p64, "fc", "leaky", S) > KINK * 2.0 ** 0
    G = eng.gradient(eng.pad_inputs(x), lab.int().to(DEV), None, S, _hip.LOSS_MEAN_PROB)[:, :D].cpu().reshape(x.shape)
    ref = O.meanprob_gradients(x.double(), lab, p64, "fc", "leaky", S)
    mags = ref.reshape(N, -1).abs().max(1)[0]
    assert float(mags.min()) < 1e-3 * float(mags.max())           # the batch does span vanishing and ordinary gradients
    # fp32 softmax: p - y carries ~6e-8 absolute noise, so points are compared where that is below the tolerance
    cond = (1.0 - ref_p.max(-1)[0]) > 1e-2
    assert int((ok & cond).sum()) >= 20
    exact = AttackEngine(StackedPosterior("fc", "leaky", (1, 28, 28), C, H, post, DEV), precision="exact")
    Ge = exact.gradient(exact.pad_inputs(x), lab.int().to(DEV), None, S, _hip.LOSS_MEAN_PROB)[:, :D].cpu().reshape(x.shape)
    e_split = (G - ref).reshape(N, -1).abs().max(1)[0] / mags
    e_exact = (Ge - ref).reshape(N, -1).abs().max(1)[0] / mags
    # the sharp output layer (logits up to ~30) puts fp32 itself at the edge of the bar here: hold the split mode to the
    # bar or to the exact fp32 kernels' own error, whichever is larger ...
    assert float(e_split[ok & cond].max()) < max(TOL, 1.5 * float(e_exact[ok & cond].max()))
    # ... and on the saturated points, where the fp32 dZ noise feeds both modes alike, to the same error as the exact mode
    assert float(e_split[ok].max()) <= 2.0 * float(e_exact[ok].max()) + 1e-6
    print(f"k={k}: cond points split {float(e_split[ok & cond].max()):.2e} exact {float(e_exact[ok & cond].max()):.2e}; "
          f"all points split {float(e_split[ok].max()):.2e} exact {float(e_exact[ok].max()):.2e}")


@pytest.mark.parametrize("arch,shape,C,H,S,N,precision", [("fc", (1, 28, 28), 10, 512, 6, 300, "split"), ("fc", (1, 28, 28), 10, 512, 6, 300, "exact"),
                                                          ("fc", (1, 28, 28), 10, 512, 6, 300, "triple"), ("fc2", (1, 28, 28), 10, 256, 3, 300, "triple"),
                                                          ("fc", (1, 2, 1), 2, 64, 10, 100, "exact"), ("fc2", (1, 28, 28), 10, 64, 3, 70, "exact")])
def test_pgd_hip_graph_replay_is_bit_identical(arch, shape, C, H, S, N, precision, monkeypatch):
    """PGD runs iteration 1 eagerly and replays a captured HIP graph for the rest: same launches, same bits as the eager loop."""
    from robustbnns_amd import AttackEngine, StackedPosterior
    D = int(np.prod(shape))
    post = O.synthetic_posterior(arch, D, H, C, S, 0.05 if D > 16 else 0.5)
    x, y = O.synthetic_inputs(N, shape, C, seed=21)
    eng = AttackEngine(StackedPosterior(arch, "leaky", shape, C, H, post, DEV), precision=precision)
    monkeypatch.setenv("RBNN_HIPGRAPH", "0")
    eager = eng.pgd(x, y, S, 0.2, iters=6).cpu()
    monkeypatch.setenv("RBNN_HIPGRAPH", "1")
    captured = []
    orig = eng._capture
    eng._capture = lambda fn: captured.append(orig(fn)) or captured[-1]
    graphed = eng.pgd(x, y, S, 0.2, iters=6).cpu()
    assert captured and captured[0] is not None, "the iteration was not captured"
    assert torch.equal(eager, graphed)
    again = eng.pgd(x, y, S, 0.2, alpha=2 / 225, iters=4).cpu()          # scalar step size, fresh capture
    monkeypatch.setenv("RBNN_HIPGRAPH", "0")
    assert torch.equal(again, eng.pgd(x, y, S, 0.2, alpha=2 / 225, iters=4).cpu())


def test_split_mode_heavy_tails_and_sparse_inputs():
    """Split precision takes ONE power-of-two scale per tensor from its largest magnitude: outlier weights (x100), MNIST-like
    inputs (80 % exact zeros, saturated ones) and a few all-zero images must still meet the bar against the fp64 oracle."""
    from robustbnns_amd import AttackEngine, StackedPosterior, _hip
    D, H, C, S, N = 784, 256, 10, 5, 200
    post = O.synthetic_posterior("fc", D, H, C, S, 0.03)
    g = torch.Generator().manual_seed(17)
    for k in ("model.1.weight", "model.3.weight"):                  # 0.1 % outliers, 100x the bulk
        m = torch.rand(post[k].shape, generator=g) < 1e-3
        post[k] = torch.where(m, post[k] * 100.0, post[k])
    x, y = O.synthetic_inputs(N, (1, 28, 28), C, seed=8)
    x = torch.where(torch.rand(x.shape, generator=g) < 0.8, torch.zeros_like(x), x)
    x = torch.where(torch.rand(x.shape, generator=g) < 0.05, torch.ones_like(x), x)
    x[:3] = 0.0
    p64 = O.cast(post, torch.float64)
    eng = AttackEngine(StackedPosterior("fc", "leaky", (1, 28, 28), C, H, post, DEV), precision="split")
    assert rel_err(eng.forward(x, S).cpu(), O.bnn_forward(x.double(), p64, "fc", "leaky", S)) < TOL
    ok = O.kink_margin(x.double(), p64, "fc", "leaky", S) > KINK
    ok[:3] = True                                                    # all-zero images: pre-activation = bias, no kink issue expected
    ok &= O.kink_margin(x.double(), p64, "fc", "leaky", S) > KINK
    assert int(ok.sum()) >= N - max(3, N // 20) - 3
    lab = y.argmax(-1)
    G = eng.gradient(eng.pad_inputs(x), lab.int().to(DEV), None, S, _hip.LOSS_MEAN_PROB)[:, :D].cpu().reshape(x.shape)
    ref = O.meanprob_gradients(x.double(), lab, p64, "fc", "leaky", S)
    exact = AttackEngine(StackedPosterior("fc", "leaky", (1, 28, 28), C, H, post, DEV), precision="exact")
    Ge = exact.gradient(exact.pad_inputs(x), lab.int().to(DEV), None, S, _hip.LOSS_MEAN_PROB)[:, :D].cpu().reshape(x.shape)
    e_split, e_exact = rel_err(G[ok], ref[ok]), rel_err(Ge[ok], ref[ok])
    print(f"heavy tails: split {e_split:.2e}  exact fp32 {e_exact:.2e}")
    assert e_split < max(TOL, 1.5 * e_exact)                         # outlier weights make the logits large: fp32 itself is the yardstick
    assert rel_err(eng.loss_gradients(x, y, S).cpu()[ok], O.loss_gradients(x.double(), y, p64, "fc", "leaky", S)[ok]) < max(TOL, 1.5 * e_exact)
    adv = eng.fgsm(x, y, S, 0.1).cpu()
    adv_equal(adv[ok], torch.clamp(x + 0.1 * ref.sign().float(), 0, 1)[ok], ref[ok])


@pytest.mark.parametrize("precision,blocks", [("split", 2), ("exact", 3), ("split", 1)])
def test_sharded_step_with_real_kernels_and_rccl(precision, blocks, monkeypatch):
    """AttackEngine._step_sharded (async all-reduces, point-block pipeline) on the GPU kernels over a 1-rank RCCL group with the
    collectives forced on: same adversarial images as the plain single-GPU step (slab partitioning differs per block, so
    pixels with a vanishing gradient component are excluded as everywhere else)."""
    import socket
    import torch.distributed as dist
    from robustbnns_amd import AttackEngine, StackedPosterior, _hip
    D, H, C, S, N = 784, 256, 10, 6, 1100
    post = O.synthetic_posterior("fc", D, H, C, S, 0.05)
    x, y = O.synthetic_inputs(N, (1, 28, 28), C, seed=13)
    sp = StackedPosterior("fc", "leaky", (1, 28, 28), C, H, post, DEV)
    plain = AttackEngine(sp, precision=precision)
    ref_f = plain.fgsm(x, y, S, 0.25).cpu()
    ref_p = plain.pgd(x, y, S, 0.25, iters=3).cpu()
    G = plain.gradient(plain.pad_inputs(x), y.argmax(-1).int().to(DEV), None, S, _hip.LOSS_MEAN_PROB)[:, :D].cpu()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1"); monkeypatch.setenv("MASTER_PORT", str(port))
    monkeypatch.setenv("RBNN_FORCE_COLLECTIVES", "1"); monkeypatch.setenv("RBNN_COMM_BLOCKS", str(blocks))
    monkeypatch.setenv("RBNN_COMM_MIN_POINTS", "256")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        eng = AttackEngine(sp, group=dist.group.WORLD, total_samples=S, precision=precision)
        assert eng.world == 2 and eng._comm_blocks(N) == blocks          # world forced to 2: every exchange runs
        adv_equal(eng.fgsm(x, y, S, 0.25).cpu(), ref_f, G)
        pg = eng.pgd(x, y, S, 0.25, iters=3).cpu()
        assert float(((pg - ref_p).abs() > 1e-6).double().mean()) < 0.01
        assert rel_err(eng.forward(x, S).cpu(), plain.forward(x, S).cpu()) < 1e-6
        # what bench.py's `comm` record is made of (engine.CommStats): every all-reduce of a step counted with its bytes, and an event pair on the
        # launch stream around every point where that stream waits for one — two per point block here (sum_s p_s [n, 16]; the gradients [n, D_pad])
        from robustbnns_amd.engine import CommStats
        cs = CommStats(lambda: torch.cuda.Event(enable_timing=True))
        eng.comm_stats = cs
        cs.on = True
        adv_equal(eng.fgsm(x, y, S, 0.25).cpu(), ref_f, G)
        cs.on = False
        torch.cuda.synchronize()
        assert cs.calls == 2 * blocks and cs.bytes == 4 * N * (16 + sp.Dp) and len(cs.exposed) == 2 * blocks
        waits = [a.elapsed_time(b) for a, b in cs.exposed]
        assert all(0.0 <= w < 50.0 for w in waits), waits
    finally:
        dist.destroy_process_group()


def test_upstream_gradient_mode_matches_autograd():
    """RBNN_LOSS_UPSTREAM: vector-Jacobian product of the mean-probability forward for an arbitrary dL/dp."""
    from robustbnns_amd import AttackEngine, StackedPosterior, _hip
    D, H, C, S, N = 784, 64, 10, 4, 20
    post = O.synthetic_posterior("fc", D, H, C, S, 0.05)
    x, _ = O.synthetic_inputs(N, (1, 28, 28), C, seed=3)
    eng = AttackEngine(StackedPosterior("fc", "leaky", (1, 28, 28), C, H, post, DEV))
    gup = torch.randn(N, 16, generator=torch.Generator().manual_seed(1))
    G = eng.gradient(eng.pad_inputs(x), None, None, S, _hip.LOSS_UPSTREAM, G_up=gup.to(DEV))[:, :D].cpu()
    xr = x.double().requires_grad_(True)
    p = O.bnn_forward(xr, O.cast(post, torch.float64), "fc", "leaky", S)
    (p * gup[:, :C].double()).sum().backward()
    assert rel_err(G, xr.grad.reshape(N, -1)) < TOL


# ------------------------------------------------------------------ (3) properties at BASELINE.json's full size
@pytest.fixture(scope="module", params=["fast", "exact"])
def full_size(request):
    from robustbnns_amd import AttackEngine, StackedPosterior
    D, H, C, S, N = 784, 512, 10, 100, 10000
    g = torch.Generator().manual_seed(7)
    post = {"model.1.weight": torch.randn(S, H, D, generator=g) * 0.05, "model.1.bias": torch.randn(S, H, generator=g) * 0.05,
            "model.3.weight": torch.randn(S, C, H, generator=g) * 0.05, "model.3.bias": torch.randn(S, C, generator=g) * 0.05}
    x, y = O.synthetic_inputs(N, (1, 28, 28), C, seed=11)
    eng = AttackEngine(StackedPosterior("fc", "leaky", (1, 28, 28), C, H, post, DEV), precision=request.param)
    assert eng.precision == ("split" if request.param == "fast" else "exact")
    return eng, post, x, y


def test_full_size_properties(full_size):
    from robustbnns_amd import _hip
    eng, post, x, y = full_size
    S, N, D = 100, 10000, 784
    lab = y.argmax(-1).int().to(DEV)
    X = eng.pad_inputs(x)
    p = eng.forward(x, S)
    assert float((p.sum(-1) - 1).abs().max()) < 1e-5 and float(p.min()) >= 0                    # probabilities
    G = eng.gradient(X, lab, None, S, _hip.LOSS_MEAN_PROB).clone()
    # (a) a subset of rows run alone gives the same rows (tile / grid independence), and matches the fp64 oracle
    rows = torch.tensor([0, 1, 63, 64, 255, 256, 4999, 9983, 9984, 9999])
    Gs = eng.gradient(eng.pad_inputs(x[rows]), lab[rows.to(DEV)], None, S, _hip.LOSS_MEAN_PROB).clone()
    assert rel_err(Gs.cpu(), G[rows.to(DEV)].cpu()) < 2e-6
    ref = O.meanprob_gradients(x[rows].double(), y[rows].argmax(-1), O.cast(post, torch.float64), "fc", "leaky", S)
    ok = O.kink_margin(x[rows].double(), O.cast(post, torch.float64), "fc", "leaky", S) > KINK
    assert int(ok.sum()) >= len(rows) - 2
    assert rel_err(G[rows.to(DEV)].cpu()[ok], ref.reshape(len(rows), -1)[ok]) < TOL
    # (b) slab chunking is only a summation-order choice
    for chunk in (1, 8):
        ws, n_slabs, _ = eng.gradient_slabs(X, lab, None, S, _hip.LOSS_MEAN_PROB, chunk=chunk)
        Gc = torch.empty_like(G)
        eng.k.sum_slabs(ws["slabs"], n_slabs, N, D, 1.0, Gc)
        assert rel_err(Gc.cpu(), G.cpu()) < 5e-6          # fp32 reordering noise at K = chunk*512 (measured 2.3e-6)
    # (c) the expected gradient is additive over disjoint sample sets (what the sample-sharded all-reduce relies on)
    lg = eng.loss_gradients(x[:512], y[:512], S)
    a = eng.gradient(eng.pad_inputs(x[:512]), lab[:512], torch.arange(0, 50, dtype=torch.int32, device=DEV), 50, _hip.LOSS_PER_SAMPLE).clone()
    b = eng.gradient(eng.pad_inputs(x[:512]), lab[:512], torch.arange(50, 100, dtype=torch.int32, device=DEV), 50, _hip.LOSS_PER_SAMPLE).clone()
    assert rel_err(((a + b) / 2).cpu(), lg.reshape(512, -1).cpu()) < 5e-6
    # (d) FGSM output is exactly x +- eps (or x where g == 0), clamped; PGD stays in the eps-ball and in [0,1]
    adv = eng.fgsm(x, y, S, 0.3).cpu()
    step = (adv - x).reshape(N, -1)
    expect = torch.clamp(x.reshape(N, -1) + 0.3 * G.cpu().sign(), 0, 1) - x.reshape(N, -1)
    assert float((step - expect).abs().max()) == 0.0
    pg = eng.pgd(x[:256], y[:256], S, 0.2, iters=3).cpu()
    assert float((pg - x[:256]).abs().max()) <= 0.2 + 1e-6 and float(pg.min()) >= 0 and float(pg.max()) <= 1
    # (e) determinism: same inputs, same bits
    G2 = eng.gradient(X, lab, None, S, _hip.LOSS_MEAN_PROB)
    assert torch.equal(G2, G)
    # (f) evaluation counts agree with a host argmax of the same outputs
    oa, aa, rob, o, a_ = eng.evaluate(x, adv, y, S)
    assert oa == 100 * float((o.argmax(-1).cpu() == y.argmax(-1)).sum()) / N
    assert aa == 100 * float((a_.argmax(-1).cpu() == y.argmax(-1)).sum()) / N
    assert float(rob.min()) >= 0 and float(rob.max()) <= 1


def test_svi_materialize_and_forward():
    """Seeded SVI forwards, both RNG modes (parity unpinned vs pyro; pinned here against the oracle restatements): "device" = the in-place
    draw kernel rbnn_svi_draw with the seed as the sample's Philox key (oracle: svi_draw_philox); "host" = a CPU restatement of the
    guide's draw order -> rbnn_svi_materialize (oracle: svi_materialize on the same eps)."""
    from robustbnns_amd.model_bnn import BNN
    C, H, S, N = 10, 32, 5, 16
    bnn = BNN("mnist", H, "leaky", "fc", "svi", 1, 0.01, None, None, (1, 28, 28), C)
    g = torch.Generator().manual_seed(3)
    loc = {k: torch.randn(v.shape, generator=g) * 0.05 for k, v in bnn.basenet.state_dict().items()}
    scale = {k: torch.full(v.shape, -3.0) for k, v in bnn.basenet.state_dict().items()}
    scale["model.1.bias"][:4] = 25.0                                       # softplus threshold branch
    bnn.set_variational_params(loc, scale, DEV)
    x, _ = O.synthetic_inputs(N, (1, 28, 28), C, seed=2)
    seeds = [3, 0, 4, 1, 2]
    assert bnn.svi_rng == "device"
    out = bnn.forward(x.to(DEV), n_samples=S, seeds=seeds).cpu()
    role = lambda d: {"W1": d["model.1.weight"].reshape(H, -1), "b1": d["model.1.bias"], "W2": d["model.3.weight"], "b2": d["model.3.bias"]}
    W, _ = O.svi_draw_philox(role(loc), role(scale), None, 0, S, sample_keys=seeds)
    post = {"model.1.weight": W["W1"], "model.1.bias": W["b1"], "model.3.weight": W["W2"], "model.3.bias": W["b2"]}
    assert rel_err(out, O.bnn_forward(x.double(), post, "fc", "leaky", S)) < TOL
    out2 = bnn.forward(x.to(DEV), n_samples=S, seeds=seeds).cpu()
    assert torch.equal(out, out2)                                          # same seeds, same draws
    avg = bnn.forward(x.to(DEV), n_samples=S, avg_posterior=True).cpu()    # logits of the mean weights (model_bnn.py:206-216)
    assert rel_err(avg, O.nn_logits(x, {k: v[None] for k, v in loc.items()}, "fc", "leaky")[0]) < TOL
    # host RNG mode: eps from torch's CPU generator in the guide's order, materialised by rbnn_svi_materialize
    bnn.svi_rng = "host"
    bnn.set_variational_params(loc, scale, DEV)
    out = bnn.forward(x.to(DEV), n_samples=S, seeds=seeds).cpu()
    eps = bnn._svi_eps(S, seeds).cpu()
    keys = list(loc); off = 0; epsd = {}
    for k in keys:
        n = loc[k].numel(); epsd[k] = eps[:, off:off + n].reshape((S,) + tuple(loc[k].shape)); off += n
    post = O.svi_materialize(loc, scale, epsd)
    assert rel_err(out, O.bnn_forward(x, post, "fc", "leaky", S)) < TOL
    assert torch.equal(out, bnn.forward(x.to(DEV), n_samples=S, seeds=seeds).cpu())


def test_autograd_through_forward(golden):
    """The reference's own fgsm recipe, run by the caller: requires_grad + CrossEntropyLoss + backward + sign."""
    g = golden("mnist_fc_h512_s8_n8_leaky"); m = g.meta; bnn = make_bnn(g)
    x = g.t("x").to(DEV).requires_grad_(True)
    out = bnn.forward(x, n_samples=m["S"])
    loss = torch.nn.CrossEntropyLoss(reduction="sum")(out, g.t("y").argmax(-1).to(DEV))
    loss.backward()
    assert rel_err(x.grad.cpu(), g.t("meanprob_grad")) < TOL
    adv = torch.clamp(x.detach() + m["eps"] * x.grad.sign(), 0, 1)
    adv_equal(adv, g.t("fgsm"), g.t("meanprob_grad"))


# ------------------------------------------------------------------ conv architecture (model_nn.py:93-106)
KINK_CONV = 3e-7   # conv nets have 50k-100k activations + pooling windows per (point, sample); fp32 noise of a pre-activation ~1e-7


def test_conv_golden(golden):
    """The reference-generated conv fixture through the reference's call surface."""
    from robustbnns_amd import adversarialAttacks as A, lossGradients, _hip
    g = golden("mnist_conv_h16_s2_n4_leaky"); m = g.meta; bnn = make_bnn(g); x, y = g.t("x"), g.t("y")
    assert type(bnn._engine).__name__ == "ConvEngine"
    assert rel_err(bnn.forward(x.to(DEV), n_samples=m["S"]).cpu(), g.t("forward_probs")) < TOL
    assert rel_err(bnn.forward(x.to(DEV), n_samples=1).cpu(), g.t("forward_probs_s1")) < TOL
    eng = bnn._engine
    assert rel_err(eng.loss_gradients(x, y, m["S"]).cpu(), g.t("loss_gradients")) < TOL
    G = eng.gradient(eng.pad_inputs(x), y.argmax(-1).int().to(DEV), None, m["S"], _hip.LOSS_MEAN_PROB)
    assert rel_err(G.cpu().reshape(x.shape), g.t("meanprob_grad")) < TOL
    lab = y.argmax(-1); hyper = {"epsilon": m["eps"]}
    adv_equal(A.fgsm_attack(bnn, x.to(DEV), lab.to(DEV), hyper, n_samples=m["S"]), g.t("fgsm"), g.t("meanprob_grad"))
    idx = torch.from_numpy(g.arr["pgd_idx"])
    pg = A.pgd_attack(bnn, x[idx].to(DEV), lab[idx].to(DEV), hyper, n_samples=m["S"]).cpu()
    assert float(((pg - g.t("pgd")).abs() > 1e-6).double().mean()) < 0.02
    oa, aa, rob = A.attack_evaluation(bnn, x, g.t("fgsm"), y, DEV, n_samples=m["S"])
    assert (oa, aa) == (float(g.arr["eval_orig_acc"]), float(g.arr["eval_adv_acc"]))
    assert float((rob.cpu() - g.t("eval_softmax_rob")).abs().max()) < 1e-6
    sd = bnn.posterior.state_dict(1)
    assert all(torch.equal(sd[k], g.posterior()[k][1]) for k in sd)


@pytest.mark.parametrize("precision", ["fast", "exact"])
@pytest.mark.parametrize("act,C,Hc,S,N", [("leaky", 10, 16, 2, 5), ("relu", 10, 32, 2, 19), ("leaky", 10, 64, 3, 33),
                                          ("leaky", 10, 512, 2, 12), ("leaky", 3, 272, 1, 5), ("leaky", 10, 1024, 1, 40)])
def test_conv_against_fp64_oracle(act, C, Hc, S, N, precision):
    from robustbnns_amd import _hip
    from robustbnns_amd.conv import ConvEngine, ConvStackedPosterior
    post = O.synthetic_posterior("conv", 784, Hc, C, S, 0.05 if Hc < 512 else (0.03 if Hc < 1024 else 0.02))
    x, y = O.synthetic_inputs(N, (1, 28, 28), C, seed=Hc + N)
    lab = y.argmax(-1); p64 = O.cast(post, torch.float64)
    eng = ConvEngine(ConvStackedPosterior(act, (1, 28, 28), C, Hc, post, DEV), precision=precision)
    assert eng.precision == ("split" if precision == "fast" else "exact")       # split: conv2 forward on the f16 pipe (hi/lo pairs)
    assert rel_err(eng.forward(x, S).cpu(), O.bnn_forward(x.double(), p64, "conv", act, S)) < TOL
    assert rel_err(eng.forward(x, S, logits=True).cpu(), O.ensemble_forward(x.double(), p64, "conv", act, S)) < TOL
    ok = O.kink_margin(x.double(), p64, "conv", act, S) > KINK_CONV
    assert int(ok.sum()) >= 2          # at Hc=512 only ~1 point in 4 is this far from every kink
    ref = O.loss_gradients(x.double(), y, p64, "conv", act, S)
    assert rel_err(eng.loss_gradients(x, y, S).cpu()[ok], ref[ok]) < TOL
    ref = O.meanprob_gradients(x.double(), lab, p64, "conv", act, S)
    G = eng.gradient(eng.pad_inputs(x), lab.int().to(DEV), None, S, _hip.LOSS_MEAN_PROB).cpu().reshape(x.shape)
    assert rel_err(G[ok], ref[ok]) < TOL
    # every point, kinks included: a flipped pooling maximum / activation sign moves the gradient by one element's worth
    assert rel_err(G, ref) < 5e-2
    adv = eng.fgsm(x, y, S, 0.1).cpu()
    adv_equal(adv[ok], torch.clamp(x + 0.1 * ref.sign().float(), 0, 1)[ok], ref[ok])
    pg = eng.pgd(x[:3], y[:3], S, 0.2, iters=3).cpu()
    assert float((pg - x[:3]).abs().max()) <= 0.2 + 1e-6 and float(pg.min()) >= 0 and float(pg.max()) <= 1
