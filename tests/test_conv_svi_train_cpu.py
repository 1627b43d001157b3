"""Host tier of SVI training of conv guides (robustbnns_amd/conv_svi_train.py, BNN.train_conv, csrc/rbnn_conv_train.hip): the new entry points in
the header, in _hip.SIGNATURES and in the library under the unchanged ABI number, their host-side argument checks, the restatement
(tests/conv_svi_restate.py) against full torch autograd of the ELBO, the inputs of the GPU tier against their own caps, the condition and
the spread of the trajectory case, every refusal with nothing loaded, and the resources of the kernels a step launches.  No HIP compute here."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

import conv_restate as CR
import conv_svi_restate as V
from robustbnns_amd import _hip
from robustbnns_amd.conv_train import CONV_KEYS
from robustbnns_amd.svi_train import ACC_KEY

pytestmark = pytest.mark.usefixtures("built_library")
NAMES = ["rbnn_conv_svi_train_sizes", "rbnn_conv_svi_train_draw", "rbnn_conv_svi_train_forward", "rbnn_conv_svi_weight_grads",
         "rbnn_conv_svi_adam_step"]
OK, ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED, ERR_ALIGN = 0, -1, -2, -3, -5
BUFFERS = ("loc", "raw", "sigma", "m_loc", "v_loc", "m_raw", "v_raw", "W", "grad")


def test_new_entry_points_are_additive_under_abi_10():
    lib = _hip.load()
    header = open(_hip.HEADER_PATH).read()
    declared = set(re.findall(r"\b(rbnn_\w+)\s*\(", header))
    assert re.search(r"#define RBNN_ABI_VERSION 10\b", header) and _hip.ABI_VERSION == 10 and lib.rbnn_abi_version() == 10
    for name in NAMES:
        assert name in declared and name in _hip.SIGNATURES and hasattr(lib, name), name
    assert declared == set(_hip.SIGNATURES)
    assert tuple(n for n, _ in _hip.ConvSviTrainNet._fields_)[6:] == BUFFERS == _hip.ConvSviTrainNet._pointers_


def _net(hidden=32, n_classes=10):
    net = _hip.ConvSviTrainNet()
    net.activation, net.in_channels, net.in_width, net.hidden, net.n_classes = 1, 1, 28, hidden, n_classes
    return net


def test_sizes_follow_the_flat_layout_and_the_deterministic_trainers_workspace():
    lib, out, det, n_part = _hip.load(), _hip.ConvTrainBytes(), _hip.ConvTrainBytes(), C.c_int64(0)
    for Hc, Cn, B in ((16, 3, 1), (48, 10, 65), (1024, 10, 128)):
        assert lib.rbnn_conv_svi_train_sizes(C.byref(_net(Hc, Cn)), B, C.byref(n_part), C.byref(out)) == OK
        shapes = V.shapes_of(Hc, Cn)
        numels = [int(torch.Size(s).numel()) for s in shapes.values()]
        assert list(shapes) == V.KEYS == CONV_KEYS
        assert out.n_params == sum(numels) == 832 + 801 * Hc + 49 * Hc * Cn + Cn
        assert n_part.value == -(-sum(-(-n // 4) for n in numels) // 256)               # one thread per quad of a tensor, 256 a block
        d = _hip.ConvTrainNet()
        d.activation, d.in_channels, d.in_width, d.hidden, d.n_classes = 1, 1, 28, Hc, Cn
        assert lib.rbnn_conv_train_sizes(C.byref(d), B, C.byref(det)) == OK
        assert all(getattr(out, k) == getattr(det, k) for k, _ in _hip.ConvTrainBytes._fields_)
    assert lib.rbnn_conv_svi_train_sizes(C.byref(_net()), 4, None, C.byref(out)) == OK          # n_partials is nullable


def test_entry_points_validate_their_arguments_on_the_host():
    """Every refusal comes back as its status code before anything is launched (there is no device here to launch on)."""
    lib, out = _hip.load(), _hip.ConvTrainBytes()
    buf = (C.c_float * 4096)()
    base = C.addressof(buf)
    base += (-base) % 16
    ws = _hip.ConvTrainWs()
    for k in _hip.CONV_TRAIN_WS_KEYS:
        setattr(ws, k, base)

    def full(**kw):
        net = _net(**kw)
        for name in BUFFERS:
            setattr(net, name, base)
        return net
    calls = {"sizes": lambda n: lib.rbnn_conv_svi_train_sizes(C.byref(n), 8, None, C.byref(out)),
             "draw": lambda n: lib.rbnn_conv_svi_train_draw(C.byref(n), 1, 0, None),
             "forward": lambda n: lib.rbnn_conv_svi_train_forward(C.byref(n), base, 784, base, 4, C.byref(ws), None),
             "grads": lambda n: lib.rbnn_conv_svi_weight_grads(C.byref(n), base, 784, 4, C.byref(ws), None),
             "adam": lambda n: lib.rbnn_conv_svi_adam_step(C.byref(n), 1, 0, 1, 0.01, 0.9, 0.999, 1e-8, base, None)}
    for field, bad, rc in (("hidden", 8, ERR_SHAPE), ("hidden", 0, ERR_SHAPE), ("hidden", 40, ERR_SHAPE), ("hidden", 4112, ERR_SHAPE),
                           ("n_classes", 0, ERR_SHAPE), ("n_classes", 17, ERR_SHAPE), ("activation", 4, ERR_UNSUPPORTED),
                           ("activation", -1, ERR_UNSUPPORTED), ("in_channels", 3, ERR_UNSUPPORTED), ("in_width", 32, ERR_UNSUPPORTED)):
        net = full()
        setattr(net, field, bad)
        for name, call in calls.items():
            assert call(net) == rc, (name, field, bad)
    assert lib.rbnn_conv_svi_train_sizes(None, 8, None, C.byref(out)) == ERR_NULL and lib.rbnn_conv_svi_train_draw(None, 1, 0, None) == ERR_NULL
    assert lib.rbnn_conv_svi_train_sizes(C.byref(_net()), 8, None, None) == ERR_NULL
    assert lib.rbnn_conv_svi_train_sizes(C.byref(_net()), 0, None, C.byref(out)) == ERR_SHAPE
    for name in ("draw", "forward", "grads", "adam"):                      # every buffer NULL
        assert calls[name](_net()) == ERR_NULL, name
    for missing, names in (("loc", ("draw", "adam")), ("sigma", ("draw", "adam")), ("W", ("draw", "forward", "grads")), ("grad", ("grads", "adam")),
                           ("raw", ("adam",)), ("m_loc", ("adam",)), ("v_raw", ("adam",))):
        net = full()
        setattr(net, missing, None)
        for name in names:
            assert calls[name](net) == ERR_NULL, (name, missing)
    net = full()
    fwd = lambda X, ldx, lab, B, w: lib.rbnn_conv_svi_train_forward(C.byref(net), X, ldx, lab, B, w, None)
    wg = lambda X, ldx, B, w: lib.rbnn_conv_svi_weight_grads(C.byref(net), X, ldx, B, w, None)
    assert fwd(None, 784, base, 4, C.byref(ws)) == ERR_NULL and fwd(base, 784, None, 4, C.byref(ws)) == ERR_NULL and fwd(base, 784, base, 4, None) == ERR_NULL
    assert wg(None, 784, 4, C.byref(ws)) == ERR_NULL and wg(base, 784, 4, None) == ERR_NULL
    assert fwd(base, 784, base, 4, C.byref(_hip.ConvTrainWs())) == ERR_NULL and wg(base, 784, 4, C.byref(_hip.ConvTrainWs())) == ERR_NULL
    for call in (lambda X, ldx, B: fwd(X, ldx, base, B, C.byref(ws)), lambda X, ldx, B: wg(X, ldx, B, C.byref(ws))):
        assert call(base, 784, 0) == ERR_SHAPE and call(base, 784, -3) == ERR_SHAPE and call(base, 784, 65537) == ERR_SHAPE
        assert call(base, 780, 4) == ERR_SHAPE and call(base, 786, 4) == ERR_SHAPE                                   # below 784; not a multiple of 4
        assert call(base + 4, 784, 4) == ERR_ALIGN
    net.W = base + 4
    assert fwd(base, 784, base, 4, C.byref(ws)) == ERR_ALIGN                                                         # the drawn weights are the forward's operand
    net.W = base
    assert lib.rbnn_conv_svi_adam_step(C.byref(net), 1, 0, 0, 0.01, 0.9, 0.999, 1e-8, base, None) == ERR_SHAPE
    assert lib.rbnn_conv_svi_adam_step(C.byref(net), 1, 0, 1, 0.01, 0.9, 0.999, 1e-8, None, None) == ERR_NULL


@pytest.mark.parametrize("Hc,act,B,Cn", V.GRAD_CASES)
def test_restatement_matches_full_autograd_of_the_elbo_and_the_pool_keeps_its_cap(Hc, act, B, Cn):
    """g_loc / g_raw (the analytic KL gradient and the chain rule through the reparameterised draw, on autograd's dCE/dW) against torch
    autograd of the whole ELBO in fp64: 1e-10 relative to each tensor's largest gradient.  The pool: at most a third dropped by the fp64
    evaluation at the drawn weights, B points remain, none of them discontinuous."""
    c = V.grad_case(Hc, act, B, Cn)
    assert c["n_pool"] == 3 * B + 8 and 3 * c["n_drop"] <= c["n_pool"] and len(c["lab"]) == B == len(c["x"])
    assert not bool(CR.discontinuous(c["x"], c["W64"], act).any())
    assert int(c["lab"].max()) < Cn and int(c["lab"].min()) >= 0
    d = lambda t: {k: v.double() for k, v in t.items()}
    loss, gl, gr, dW, W = V.step_gradients(d(c["loc"]), d(c["raw"]), c["eps"], c["x"], c["lab"], act)
    loss_a, al, ar = V.elbo_autograd(d(c["loc"]), d(c["raw"]), c["eps"], c["x"], c["lab"], act)
    assert all(torch.equal(W[k], c["W64"][k]) for k in V.KEYS)
    worst = 0.0
    for got, ref in ((gl, al), (gr, ar)):
        for k in V.KEYS:
            gmax = float(ref[k].abs().max())
            assert gmax > 0 and float(dW[k].abs().max()) > 0, k
            worst = max(worst, float((got[k] - ref[k]).abs().max()) / gmax)
    print(f"[conv-svi-restate Hc={Hc} {act} B={B} C={Cn}] g_loc / g_raw vs autograd of the ELBO: worst {worst:.2e} relative; loss {float(loss):.10e} vs "
          f"{loss_a:.10e}; dropped {c['n_drop']} of {c['n_pool']} pool points")
    assert worst <= 1e-10 and abs(float(loss) - loss_a) <= 1e-12 * abs(loss_a)


def test_draw_restatement_is_the_flat_draws_counter_layout():
    """eps of tensor i: one row of n_elem columns under tensor id i — element e is component e % 4 of the block with counter (e / 4, i, s, draw)."""
    from oracle import bnn_oracle as O
    from robustbnns_amd.conv import ConvSviGuide
    assert V.TENSOR_IDS == ConvSviGuide.TENSOR_IDS and V.ACC_KEY == ACC_KEY
    shapes = V.shapes_of(16, 3)
    eps = V.draw_eps(shapes, 0xABCDEF0123456789, 7, 2)
    for k, shp in shapes.items():
        n = int(torch.Size(shp).numel())
        for s in range(2):
            ref = torch.from_numpy(O.philox_normals(0xABCDEF0123456789, 7, V.TENSOR_IDS[k], s, 1, n)[0])
            assert torch.equal(eps[k][s].reshape(-1), ref), (k, s)
    assert not torch.equal(eps["model.0.bias"][0], eps["model.0.bias"][1])


def test_trajectory_case_meets_no_discontinuity_and_its_spread_is_the_recorded_one():
    """The condition of the 20-step GPU test on the fp64 run: every step's pool keeps the cap and no batch point of any step is discontinuous at
    that step's drawn weights.  The fp32-vs-fp64 spread of the restatement over the trajectory is measured HERE (torch on the CPU, never the
    code under test) and must be the constant the GPU test multiplies: conv_svi_restate.TRAJ_SPREAD."""
    ref = V.traj_reference()
    assert len(ref["batches"]) == V.TRAJ["steps"] == 20 and V.TRAJ["act"] == "tanh" and V.TRAJ["hidden"] == 16 and V.TRAJ["batch"] == 8
    assert ref["n_bad"] == 0
    assert all(3 * d <= n == 3 * 8 + 8 for d, n in ref["drops"]), ref["drops"]
    assert all(len(lb) == 8 for _, lb in ref["batches"])
    spread = V.traj_spread()
    print(f"[conv-svi-restate trajectory seed {V.TRAJ_SEED}] 20 steps; dropped per step {[d for d, _ in ref['drops']]} of 32; fp32-vs-fp64 spread loc "
          f"{spread['loc']:.3e} raw {spread['raw']:.3e} (recorded {V.TRAJ_SPREAD}); losses {ref['r64'].losses[0]:.6e} .. {ref['r64'].losses[-1]:.6e}")
    for name in ("loc", "raw"):
        assert 0.5 * V.TRAJ_SPREAD[name] <= spread[name] <= 1.01 * V.TRAJ_SPREAD[name], (name, spread[name])


def test_guards_fire_with_nothing_loaded_and_no_state_changed(monkeypatch, tmp_path):
    from torch.utils.data import DataLoader, TensorDataset
    from robustbnns_amd import conv_svi_train
    from robustbnns_amd.model_bnn import BNN
    launched = []
    monkeypatch.setattr(_hip, "HipKernels", lambda: launched.append(1))
    monkeypatch.setattr(_hip, "load", lambda: launched.append(2))
    x, y = torch.rand(8, 1, 28, 28), torch.eye(10)[torch.arange(8)]
    loader = DataLoader(TensorDataset(x, y), batch_size=4)
    bnn = lambda arch, inf="svi", shape=(1, 28, 28): BNN("mnist", 16, "leaky", arch, inf, 1 if inf == "svi" else None, 0.01 if inf == "svi" else None,
                                                         None if inf == "svi" else 5, None if inf == "svi" else 2, shape, 10)
    conv, fc, fc2, hmc, cifar = bnn("conv"), bnn("fc"), bnn("fc2"), bnn("conv", "hmc"), bnn("conv", shape=(3, 32, 32))
    loc, raw = V.guide(16, 10, 1)
    torch.manual_seed(5)
    rng = torch.get_rng_state()
    rel = str(tmp_path) + "/"
    with pytest.raises(NotImplementedError, match="no CPU compute path"):
        conv.train_conv(loader, "cpu", rel)
    with pytest.raises(NotImplementedError, match="1x28x28"):
        cifar.train_conv(loader, "cuda:0", rel)
    for net in (fc, fc2):
        with pytest.raises(ValueError, match=r"\btrain\b"):
            net.train_conv(loader, "cuda:0", rel)
    with pytest.raises(NotImplementedError, match="train_hmc"):
        hmc.train_conv(loader, "cuda:0", rel)
    with pytest.raises(NotImplementedError, match="conv"):
        conv.train(loader, "cuda:0", rel)                                    # BNN.train keeps refusing conv ...
    with pytest.raises(NotImplementedError, match="train_conv"):
        conv.train(loader, "cuda:0", rel)                                    # ... and now names the method that trains it
    with pytest.raises(NotImplementedError, match="no CPU compute path"):
        conv_svi_train.ConvSviTrainer("leaky", (1, 28, 28), 10, loc, raw, 0.01, "cpu", 1)
    with pytest.raises(NotImplementedError, match="1x28x28"):
        conv_svi_train.ConvSviTrainer("leaky", (3, 32, 32), 10, loc, raw, 0.01, "cuda:0", 1)
    assert not launched and torch.equal(rng, torch.get_rng_state())
    for net in (conv, fc, fc2, hmc, cifar):
        assert not hasattr(net, "device") and not hasattr(net, "training_history") and net.svi_loc is None and net.posterior is None
    assert not os.listdir(tmp_path)


def test_kernels_of_a_conv_svi_step_use_no_scratch():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources as KR
    if not os.path.exists(KR.READELF):
        pytest.skip("llvm-readelf not in this image")
    step = (r"svi_draw_flat_kernel\(|conv1_pool_kernel<\d, rbnn_conv_shared::Geo<1, 28>, 0>|conv2_pool_kernel<\d, rbnn_conv_shared::Geo<1, 28> >|::conv_fc_kernel\(|::conv_(head|reduce)_kernel\(|"
            r"::conv_(do2|wgrad_gemm|route1)_kernel<\d, false>|::train_gemm_kernel<false, false>|svi::\(anonymous namespace\)::adam_kernel<svi::\(anonymous namespace\)::Single>|"
            r"\)::reduce_samples_kernel\(|\(anonymous namespace\)::finalize_kernel\(")
    res = {n: r for n, r in KR.kernel_resources().items() if re.search(step, n)}
    # the draw, conv1 / conv2 x 4 activations, the Linear, the head, the strided GEMM (dFw), do2 and route1 x 4, the conv GEMM in 3 modes, the
    # partial sums' reduction, Adam + KL over the conv layout, the sum over the accuracy samples, the step's sums
    assert len(res) == 1 + 8 + 1 + 1 + 1 + 8 + 3 + 1 + 1 + 1 + 1, sorted(res)
    bad = {n: (r["scratch"], r["spill_vgpr"]) for n, r in res.items() if r["scratch"] or r["spill_vgpr"]}
    assert not bad, bad
