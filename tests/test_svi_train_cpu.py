"""CPU tests of SVI training (model_bnn.py:105-136, :303-365): the restatement in tests/svi_restate.py is the reference's semantics (the loss
torch.distributions computes, the gradients autograd gives, torch.optim.Adam's update), the guide's initialisation order, and the argument
checks of the training entry points of the C-ABI (no GPU touched); the restated accuracy forward against a plain loop over samples, and —
with the reference alone — that every case of the GPU module's gradient and epoch tests keeps its exclusions under its cap."""
import ctypes as C

import pytest
import torch
from torch.distributions import Categorical, Normal, kl_divergence

import svi_restate as R
from robustbnns_amd import _hip
from robustbnns_amd.model_bnn import set_rng_seed
from robustbnns_amd.svi_train import initial_params, state_keys


def _guide(arch, D, H, Cn, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = R.shapes_of(arch, D, H, Cn)
    loc = {k: 0.3 * torch.randn(*s, generator=g, dtype=torch.float64) for k, s in shapes.items()}
    raw = {k: torch.randn(*s, generator=g, dtype=torch.float64) - 1.0 for k, s in shapes.items()}
    x = torch.rand(13, D, generator=g, dtype=torch.float64)
    y = torch.randint(0, Cn, (13,), generator=g)
    return shapes, loc, raw, x, y


@pytest.mark.parametrize("arch,act", [("fc", "leaky"), ("fc", "tanh"), ("fc2", "sigm"), ("fc2", "relu")])
def test_restatement_is_the_torch_distributions_loss_and_its_autograd_gradients(arch, act):
    shapes, loc, raw, x, y = _guide(arch, 6, 8, 3, seed=len(arch) + len(act))
    eps = {k: v[0] for k, v in R.draw_eps(shapes, arch, 0x1234, 3).items()}
    loss, g_loc, g_raw, _, _ = R.step_gradients(loc, raw, eps, x, y, arch, act)
    # the reference's loss: -Categorical(logits=log_softmax(z)).log_prob(y).sum() + sum KL(Normal(loc, softplus(raw)) || Normal(0, 1))
    L = {k: v.clone().requires_grad_(True) for k, v in loc.items()}
    Rw = {k: v.clone().requires_grad_(True) for k, v in raw.items()}
    W = {k: L[k] + torch.nn.functional.softplus(Rw[k]) * eps[k] for k in shapes}
    h = x
    ks = R.layer_keys(arch)
    for i, k in enumerate(ks):
        h = h @ W[k + ".weight"].T + W[k + ".bias"]
        if i + 1 < len(ks):
            h = {"relu": torch.relu, "leaky": torch.nn.functional.leaky_relu, "sigm": torch.sigmoid, "tanh": torch.tanh}[act](h)
    ref = -Categorical(logits=torch.log_softmax(h, -1)).log_prob(y).sum()
    for k in shapes:
        ref = ref + kl_divergence(Normal(L[k], torch.nn.functional.softplus(Rw[k])), Normal(torch.zeros_like(L[k]), torch.ones_like(L[k]))).sum()
    ref.backward()
    assert abs(float(loss) - float(ref.detach())) <= 1e-12 * abs(float(ref.detach()))
    for k in shapes:
        assert torch.allclose(g_loc[k], L[k].grad, rtol=1e-10, atol=1e-12), k
        assert torch.allclose(g_raw[k], Rw[k].grad, rtol=1e-10, atol=1e-12), k


def test_restated_update_is_torch_optim_adam_over_several_steps():
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(40, generator=g, dtype=torch.float64)
    grads = [torch.randn(40, generator=g, dtype=torch.float64) * 10.0 ** (i % 3 - 1) for i in range(7)]
    p = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=0.02)
    q, m, v = p0.clone(), torch.zeros(40, dtype=torch.float64), torch.zeros(40, dtype=torch.float64)
    for t, gr in enumerate(grads, 1):
        p.grad = gr.clone()
        opt.step()
        R.adam_update(q, gr, m, v, t, 0.02)
        assert torch.allclose(q, p.detach(), rtol=0, atol=1e-15), t


def test_guide_init_draws_loc_then_scale_per_key_in_state_dict_order():
    shapes = list(R.shapes_of("fc2", 5, 16, 3).items())
    set_rng_seed(0)
    loc, raw = initial_params(shapes)
    set_rng_seed(0)
    for k, s in shapes:
        assert torch.equal(loc[k], torch.randn(s)) and torch.equal(raw[k], torch.randn(s)), k
    assert list(loc) == state_keys("fc2") == [k for k, _ in shapes]


def test_accuracy_forward_is_a_plain_loop_over_the_ten_samples():
    from robustbnns_amd import svi_train
    assert (R.ACC_KEY, R.ACC_SAMPLES) == (svi_train.ACC_KEY, svi_train.ACC_SAMPLES)
    for arch, act in (("fc", "tanh"), ("fc2", "leaky")):
        shapes, loc, raw, x, y = _guide(arch, 6, 8, 3, seed=11)
        key, t = 0xABCDEF0123456789, 4
        psum, pred, gap = R.accuracy_forward(loc, raw, arch, act, x.reshape(13, 1, 6, 1), key, t)
        eps = R.draw_eps(shapes, arch, key ^ R.ACC_KEY, t, n_samples=10)
        acts = {"leaky": torch.nn.functional.leaky_relu, "tanh": torch.tanh}
        total = torch.zeros(13, 3, dtype=torch.float64)
        for s in range(10):
            W = {k: loc[k] + torch.nn.functional.softplus(raw[k]) * eps[k][s] for k in shapes}
            h, ks = x, R.layer_keys(arch)
            for i, k in enumerate(ks):
                h = h @ W[k + ".weight"].T + W[k + ".bias"]
                if i + 1 < len(ks):
                    h = acts[act](h)
            total += torch.softmax(h, -1)
        assert torch.allclose(psum, total, rtol=1e-13, atol=0)
        assert torch.equal(pred, torch.argmax(total, -1))
        top = (total / 10).sort(-1, descending=True)[0]
        assert torch.allclose(gap, top[:, 0] - top[:, 1], rtol=0, atol=1e-15)
        # another step, another key: other draws
        assert not torch.equal(R.accuracy_forward(loc, raw, arch, act, x.reshape(13, 1, 6, 1), key, t + 1)[0], psum)
        assert not torch.equal(R.accuracy_forward(loc, raw, arch, act, x.reshape(13, 1, 6, 1), key + 1, t)[0], psum)


def test_first_maximum_wins_an_exact_tie():
    p = torch.tensor([[0.25, 0.5, 0.5], [0.5, 0.5, 0.25], [0.125, 0.25, 0.75], [1.0, 1.0, 1.0], [0.3, 0.2, 0.3]], dtype=torch.float64)
    assert R.first_argmax(p).tolist() == [1, 0, 2, 0, 0]
    assert R.top2_gap(p).tolist() == [0.0, 0.0, 0.5, 0.0, 0.0]
    assert R.first_argmax(p[:, :1]).tolist() == [0] * 5 and bool(torch.isinf(R.top2_gap(p[:, :1])).all())       # one class: never marginal


def test_restatement_records_the_loss_of_every_step():
    shapes, loc, raw, x, y = _guide("fc", 6, 8, 3, seed=2)
    r, plain = R.Restatement(loc, raw, "fc", "leaky", 0.01, 7, record=True), R.Restatement(loc, raw, "fc", "leaky", 0.01, 7)
    got = [r.step(x, y) for _ in range(4)]
    assert r.losses == got and len(set(got)) == 4 and plain.losses is None
    assert [plain.step(x, y) for _ in range(4)] == got
    # the recorded loss of step t is the ELBO of the guide BEFORE that step's update, at the draw of step t
    again = R.Restatement(loc, raw, "fc", "leaky", 0.01, 7)
    for t in range(3):
        again.step(x, y)
    assert got[3] == float(R.step_gradients(again.loc, again.raw, again.eps(3), x, y, "fc", "leaky")[0])


def _gpu_cases():
    import test_hip_svi_train as T
    return T


@pytest.mark.parametrize("case", _gpu_cases().GRAD_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2][0] * c[2][1] * c[2][2]}-{c[3]}-{c[4]}-{c[5]}")
def test_gradient_cases_keep_their_exclusions_under_the_cap(case):
    """With the oracle alone: at most 1 % of a case's points lie within the kink margin (none at B <= 3), a case with C > 1 and B >= 65 has
    points on both branches of the head kernel's CE, and the confident case has at least a quarter of its points at CE < 1e-3."""
    T = _gpu_cases()
    c, B = T.grad_case(*case), case[5]
    n = int(c["ok"].sum())
    assert B - n <= 0.01 * B
    if case[4] > 1 and B >= 65:
        assert 0 < int(c["log1p"].sum()) < n
    if c["confident"]:
        assert int((c["log1p"] & (c["ce"] < T.CONFIDENT)).sum()) >= n // 4


def test_gradient_cases_cover_the_edges():
    T = _gpu_cases()
    D = lambda c: c[2][0] * c[2][1] * c[2][2]
    cases = T.GRAD_CASES
    assert {96, 160, 1024} <= {c[3] for c in cases} and {1, 16} <= {c[4] for c in cases} and {1, 3, 65, 300} <= {c[5] for c in cases}
    for arch in ("fc", "fc2"):
        assert {10, 17, 3072} <= {D(c) for c in cases if c[0] == arch}
    assert ("fc2", "relu") in {c[:2] for c in cases} and ("fc", "sigm") in {c[:2] for c in cases}
    assert any(c[3] % 64 and D(c) % 16 and c[5] % 64 for c in cases)
    assert len(set(cases)) == len(cases) and sum(1 for c in cases if T.grad_case(*c)["confident"]) == 1


@pytest.mark.parametrize("name", _gpu_cases().EPOCH_CASES)
def test_epoch_cases_keep_the_marginal_points_under_the_cap(name):
    """The fp64 restatement's own trajectory of every epoch set-up: points whose two largest mean probabilities are closer than the margin are
    at most 1 % of each epoch's points (expected: none), and every epoch ends on a short batch."""
    T = _gpu_cases()
    c = T.epoch_case(name)
    n, bs = c["n"], c["batch"]
    assert 0 < n % bs < bs
    r = R.Restatement(c["loc"], c["raw"], c["arch"], c["act"], c["lr"], c["key"], torch.float64)
    for epoch in range(c["epochs"]):
        marginal = 0
        for i in range(0, n, bs):
            x, lab = c["x"][i:i + bs], c["lab"][i:i + bs]
            t = r.t
            r.step(x, lab)
            psum, pred, gap = R.accuracy_forward(r.loc, r.raw, c["arch"], c["act"], x, c["key"], t)
            marginal += T.accuracy_bounds(psum, pred, gap, lab)[1]
        assert marginal <= 0.01 * n, (epoch, marginal)
        assert marginal == 0, (epoch, marginal)


def test_history_case_spread_is_the_measured_one():
    """The bar of the GPU module's history test is 10 x the relative fp32-vs-fp64 spread of the restatement's own epoch losses: measured here."""
    T = _gpu_cases()
    out = T.history_restatements([torch.float32, torch.float64])
    spread = max(abs(a - b) / abs(b) for a, b in zip(out[torch.float32], out[torch.float64]))
    print(f"epoch losses fp32 {out[torch.float32]}  fp64 {out[torch.float64]}  relative spread {spread:.3e} (recorded {T.HISTORY_CASE['spread']:.3e})")
    assert T.HISTORY_CASE["spread"] / 4 <= spread <= 4 * T.HISTORY_CASE["spread"]


@pytest.mark.usefixtures("built_library")
def test_training_entry_points_reject_bad_arguments_without_launching():
    lib = _hip.load()
    net = _hip.SviTrainNet()
    net.arch, net.activation, net.in_features, net.hidden, net.n_classes = 1, 1, 784, 512, 10
    n_part = C.c_int64(0)
    assert lib.rbnn_svi_train_sizes(C.byref(net), C.byref(n_part)) == 512 * 784 + 512 + 512 * 512 + 512 + 10 * 512 + 10
    assert n_part.value == (512 * 196 + 128 + 512 * 128 + 128 + 10 * 128 + 3 + 255) // 256
    assert lib.rbnn_svi_train_sizes(None, None) == -1
    fake = 0x10000                                          # never dereferenced: every call below returns before a launch
    ws = _hip.SviTrainWs(*([fake] * len(_hip.SVI_TRAIN_WS_KEYS)))
    assert lib.rbnn_svi_train_draw(C.byref(net), 1, 0, None) == -1                            # loc / sigma / W not set
    assert lib.rbnn_svi_train_forward(C.byref(net), None, 784, 8, fake, C.byref(ws), None) == -1
    for name in ("loc", "raw", "sigma", "m_loc", "v_loc", "m_raw", "v_raw", "W", "grad"):
        setattr(net, name, fake)
    assert lib.rbnn_svi_train_forward(C.byref(net), fake, 784, 8, None, C.byref(ws), None) == -1
    assert lib.rbnn_svi_train_forward(C.byref(net), fake, 784, 8, fake, None, None) == -1
    assert lib.rbnn_svi_train_forward(C.byref(net), fake, 784, 0, fake, C.byref(ws), None) == -2      # B <= 0
    assert lib.rbnn_svi_train_forward(C.byref(net), fake, 784, -3, fake, C.byref(ws), None) == -2
    assert lib.rbnn_svi_train_forward(C.byref(net), fake, 700, 8, fake, C.byref(ws), None) == -2      # ldx < D
    assert lib.rbnn_svi_weight_grads(C.byref(net), fake, 784, 0, C.byref(ws), None) == -2
    assert lib.rbnn_svi_weight_grads(C.byref(net), None, 784, 8, C.byref(ws), None) == -1
    assert lib.rbnn_svi_adam_step(C.byref(net), 1, 0, 0, 0.01, 0.9, 0.999, 1e-8, fake, None) == -2       # step < 1
    assert lib.rbnn_svi_adam_step(C.byref(net), 1, 0, 1, 0.01, 0.9, 0.999, 1e-8, None, None) == -1
    assert lib.rbnn_svi_train_finalize(fake, 0, fake, 8, None, 16, None, 10, fake, None) == -2
    assert lib.rbnn_svi_train_finalize(fake, 4, fake, 0, None, 16, None, 10, fake, None) == -2
    assert lib.rbnn_svi_train_finalize(fake, 4, fake, 8, fake, 16, None, 10, fake, None) == -1            # Psum without labels
    assert lib.rbnn_svi_train_finalize(None, 4, fake, 8, None, 16, None, 10, fake, None) == -1
    for field, bad, rc in (("hidden", 0, -2), ("n_classes", 17, -2), ("in_features", 0, -2), ("arch", 2, -3), ("activation", 4, -3)):
        good = getattr(net, field)
        setattr(net, field, bad)
        assert lib.rbnn_svi_train_draw(C.byref(net), 1, 0, None) == rc, field
        assert lib.rbnn_svi_train_forward(C.byref(net), fake, 784, 8, fake, C.byref(ws), None) == rc, field
        setattr(net, field, good)
    net.arch = 1
    ws.hid2 = None
    assert lib.rbnn_svi_train_forward(C.byref(net), fake, 784, 8, fake, C.byref(ws), None) == -1        # fc2 needs the second layer's buffers
