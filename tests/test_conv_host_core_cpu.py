"""Host tier of what the six conv trainers and samplers share (robustbnns_amd/conv_train.py: tensor_major / views / flat_of, conv_group on
conv.conv_ws_budget): the tensor-major layout against its offsets written out by hand, and one RBNN_CONV_WS_GB read behind the three group
functions and ConvEngine's point block.  No HIP compute is called here."""
import types

import pytest
import torch

from fake_kernels import FakeKernels
from robustbnns_amd.conv_train import CONV_KEYS, flat_of, tensor_major, views

SHAPES = lambda Hc, Cn: dict(zip(CONV_KEYS, ((32, 1, 5, 5), (32,), (Hc, 32, 5, 5), (Hc,), (Cn, 49 * Hc), (Cn,))))


def test_tensor_major_round_trip_and_view_offsets():
    """(Hc 16, C 3, K 3): flat [K, n] -> tensor_major -> flat_of(k) is flat[k]; views(buf, i, n)[key] is a view of buf — no copy — at element
    sum(blocks before key) * n + i * size, in the tensor's shape, for n = K and for the accuracy stack's n = K * 10 with i = k * 10 + s."""
    K, S, shapes = 3, 10, SHAPES(16, 3)
    blocks = [int(torch.Size(s).numel()) for s in shapes.values()]
    nets = types.SimpleNamespace(state_keys=list(CONV_KEYS), shapes=shapes, blocks=blocks)
    n = sum(blocks)
    assert blocks == [800, 32, 800 * 16, 16, 49 * 16 * 3, 3] and n == 832 + 801 * 16 + 49 * 16 * 3 + 3
    flat = torch.arange(K * n, dtype=torch.float32).reshape(K, n)
    tm = tensor_major(flat, blocks)
    assert tuple(tm.shape) == (K * n,) and torch.equal(tm.sort().values, flat.reshape(-1))
    assert torch.equal(tensor_major(flat[:1], blocks), flat[0])               # one net: the single net's flat buffer
    for k in range(K):
        assert torch.equal(flat_of(tm, k, blocks, K), flat[k])
        v = views(tm, k, K, nets)
        assert list(v) == list(CONV_KEYS)
        for t, key in enumerate(CONV_KEYS):
            first = sum(blocks[:t])
            assert tuple(v[key].shape) == shapes[key]
            assert v[key].data_ptr() == tm.data_ptr() + 4 * (first * K + k * blocks[t]), (key, k)
            assert torch.equal(v[key].reshape(-1), flat[k, first:first + blocks[t]]), (key, k)
    acc = torch.arange(K * S * n, dtype=torch.float32)
    for k, s in ((0, 0), (1, 7), (2, 9)):
        i = k * S + s
        v = views(acc, i, K * S, nets)
        for t, key in enumerate(CONV_KEYS):
            start = sum(blocks[:t]) * K * S + i * blocks[t]
            assert v[key].data_ptr() == acc.data_ptr() + 4 * start and tuple(v[key].shape) == shapes[key], (key, k, s)
            assert torch.equal(v[key].reshape(-1), acc[start:start + blocks[t]]), (key, k, s)
    v = views(tm, 1, K, nets)["model.3.bias"]
    v.fill_(-1.0)                                                              # a view: writing it writes the buffer
    assert torch.equal(flat_of(tm, 1, blocks, K)[832 + 800 * 16:832 + 801 * 16], torch.full((16,), -1.0))


@pytest.mark.usefixtures("built_library")
def test_groups_and_point_block_follow_one_budget_read(monkeypatch):
    """RBNN_CONV_WS_GB = 0.001 (1 MB): every group function answers 1 and ConvEngine.point_block 16, through conv.conv_ws_budget — the one
    place the variable is read; an explicit budget_gb goes the same way and wins over the variable."""
    from robustbnns_amd import conv
    from robustbnns_amd.conv_hmc import conv_hmc_chains_group
    from robustbnns_amd.conv_svi_train import conv_svi_lockstep_group
    from robustbnns_amd.conv_train import conv_ensemble_group, conv_group
    groups = (conv_ensemble_group, conv_svi_lockstep_group, conv_hmc_chains_group)
    p1w, p2w = conv.conv_geometry((1, 28, 28))
    post = types.SimpleNamespace(arch="conv", P1W=p1w, NP2=p2w * p2w, H=32, S=3, C=10, D=784, Dp=784, device=torch.device("cpu"))
    eng = conv.ConvEngine(post, kernels=FakeKernels())
    monkeypatch.setenv("RBNN_CONV_WS_GB", "0.001")
    assert conv.conv_ws_budget() == 0.001 * 2 ** 30 and conv.conv_ws_budget(2) == 2 * 2 ** 30
    assert [g("leaky", 1024, 10, 100, 100) for g in groups] == [1, 1, 1]
    assert eng.point_block(3) == 16
    assert [g("leaky", 16, 10, 7, 8, budget_gb=48) for g in groups] == [7, 7, 7]
    assert conv_group(100000, 50, None) == int(0.001 * 2 ** 30 // 100000) == 10 and conv_group(100000, 50, None, 9, 4) == 4
    assert conv_group(2 ** 40, 50, None) == 1 and conv_group(100000, 7, None) == 7
    monkeypatch.setenv("RBNN_CONV_WS_GB", "48")
    assert [g("leaky", 16, 10, 7, 8) for g in groups] == [7, 7, 7] and eng.point_block(3) > 16
