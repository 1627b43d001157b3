"""GPU tests (-m gpu) of SVI training (model_bnn.py:105-136, :303-365; csrc/rbnn_train.hip, robustbnns_amd/svi_train.py): the weight
gradients and the step loss against fp64 autograd on the oracle's draw, the Adam kernel against torch.optim.Adam, 20-step trajectories
against the CPU restatement (tests/svi_restate.py), BNN.train end to end, reproducibility, the param-store round trip, no device->host
sync inside a step, and the guards."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader, TensorDataset

import svi_restate as R
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
              ("fc2", "tanh", (1, 28, 28), 256, 10, 128), ("fc2", "sigm", (1, 2, 1), 32, 2, 128), ("fc2", "leaky", (1, 28, 28), 128, 10, 37)]


@pytest.mark.parametrize("arch,act,shape,H,Cn,B", GRAD_CASES)
def test_weight_gradients_and_step_loss_match_fp64_autograd(arch, act, shape, H, Cn, B):
    from robustbnns_amd.svi_train import SviTrainer
    D = shape[0] * shape[1] * shape[2]
    shapes, loc, raw = _guide(arch, D, H, Cn, seed=H + B, std=0.05 if D > 16 else 0.5)
    x, y = O.synthetic_inputs(B, shape, Cn, seed=B)
    if D <= 16:
        x = 4 * x - 2
    lab = y.argmax(-1)
    key, draw = 0x0123456789ABCDEF, 5
    eps = R.draw_eps(shapes, arch, key, draw)
    W64 = {k: loc[k].double() + F.softplus(raw[k].double()) * eps[k][0] for k in shapes}
    ok = O.kink_margin(x.double(), {k: v[None] for k, v in W64.items()}, arch, act, 1) > KINK
    print(f"[{arch} {D}->{H}->{Cn} {act} B={B}] points within the kink margin: {int((~ok).sum())}")
    assert int((~ok).sum()) <= 0.01 * B
    x, lab = x[ok], lab[ok]
    Wg = {k: v.clone().requires_grad_(True) for k, v in W64.items()}
    ce64, _ = R.ce_grads(x.reshape(x.shape[0], -1).double(), lab, Wg, arch, act)
    ce64.backward()
    tr = SviTrainer(arch, act, shape, Cn, loc, raw, 0.01, DEV, key, batch_size=64)       # smaller than B: the workspaces grow
    tr.t = draw
    tr.gradients(x.to(DEV), lab.to(DEV))
    torch.cuda.synchronize()
    W, G = tr.unflat(tr.W), tr.unflat(tr.grad)
    for k in shapes:
        ew = float((W[k].cpu().double() - W64[k]).abs().max() / (W64[k].abs().max()))
        g64 = Wg[k].grad
        err = float((G[k].cpu().double() - g64).abs().max())
        print(f"   {k}: draw rel err {ew:.1e}  max|dW - fp64| = {err:.2e} = {err / float(g64.abs().max()):.1e} max|dW|")
        assert ew < 2e-6, k
        assert err <= 1e-5 * float(g64.abs().max()), k
    # the reported step loss: sum CE + KL of the pre-update guide, same draw
    tr.t = draw
    tr.step(x.to(DEV), lab.to(DEV), accuracy=False)
    loss = float(tr.stats[0])
    ref = float(ce64.detach()) + float(R.kl({k: v.double() for k, v in loc.items()}, {k: v.double() for k, v in raw.items()}))
    print(f"   step loss {loss:.8e}  fp64 {ref:.8e}  rel {abs(loss - ref) / abs(ref):.1e}")
    assert abs(loss - ref) <= 1e-5 * abs(ref)


@pytest.mark.parametrize("t", [1, 2, 10])
def test_adam_step_kernel_matches_torch_optim_adam(t):
    """Tolerance: every output is a chain of at most ~10 fp32 operations (2^-24 relative rounding each) on operands bounded by the scale
    named below, and the regenerated eps carries the hardware log / sin (about 2^-21 relative): 2e-6 x scale bounds each result."""
    from robustbnns_amd import _hip
    from robustbnns_amd.svi_train import ADAM_EPS, BETAS, SviTrainer
    arch, D, H, Cn, lr, key, draw = "fc2", 20, 64, 5, 0.01, 0xFEEDFACE12345678, 17
    shapes, loc, raw = _guide(arch, D, H, Cn, seed=t, std=0.3)
    tr = SviTrainer(arch, "leaky", (1, D, 1), Cn, loc, raw, lr, DEV, key, batch_size=8)
    g = torch.Generator().manual_seed(100 + t)
    n = tr.n_params
    raw_f = torch.randn(n, generator=g) - 1.0
    vals = {"loc": torch.randn(n, generator=g), "raw": raw_f, "grad": torch.randn(n, generator=g) * 3}
    for p in ("loc", "raw"):
        m = 0.2 * torch.randn(n, generator=g)
        vals["m_" + p], vals["v_" + p] = m, (m.abs() + torch.rand(n, generator=g)) ** 2
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
            err = ((got - out[name]).abs() / sc).max()
            print(f"t={t} {name}: max |err| / scale = {float(err):.2e}")
            assert float(err) <= 2e-6, name
    sig_new = F.softplus(out["raw"])
    err = ((tr.sigma.cpu().double() - sig_new).abs() / (sig_new + torch.sigmoid(out["raw"]) * (out["raw"].abs() + lr))).max()
    print(f"t={t} sigma: max |err| / scale = {float(err):.2e}")
    assert float(err) <= 2e-6
    kl = float(((-torch.log(sig32) + 0.5 * (sig32 ** 2 + d["loc"] ** 2)) - 0.5).sum())
    assert abs(float(tr.kl_part.double().sum()) - kl) <= 1e-5 * abs(kl)


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
