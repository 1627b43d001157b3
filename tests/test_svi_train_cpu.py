"""CPU tests of SVI training (model_bnn.py:105-136, :303-365): the restatement in tests/svi_restate.py is the reference's semantics (the loss
torch.distributions computes, the gradients autograd gives, torch.optim.Adam's update), the guide's initialisation order, and the argument
checks of the training entry points of the C-ABI (no GPU touched)."""
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
