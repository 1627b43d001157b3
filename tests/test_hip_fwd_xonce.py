"""GPU tests of the triple forward's two-chunk form (-m gpu): with an even number of 256-unit chunks fc_forward_x3_kernel keeps two chunks'
accumulators and streams the X tile once per item (RBNN_X3_FWD_XONCE, default on; 0 = one chunk at a time, the form every other H uses).

  bytes    every accumulator receives the same MFMAs in the same order in both forms, so everything the forward writes — P, the 1-bit stashes,
           the act' streams, fc2's hidden image — must be equal BYTE FOR BYTE between the switch at 0 and at 1, in one process
  fp64     equality of the two forms says nothing if both are wrong: one case is also held to the fp64 oracle, with the bound
           tests/test_hip_triple.py applies to the same quantities
Everything goes through the C-ABI (robustbnns_amd._hip) and the engine's own workspace.
"""
import pytest
import torch

from conftest import rel_err
from oracle import bnn_oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("built_library")]
TOL, KINK, DEV = 1e-5, 2e-6, "cuda:0"          # tests/test_hip_triple.py's
SWITCH = "RBNN_X3_FWD_XONCE"
OUTPUTS = ("P", "mask1", "mask2", "dact1", "dact2")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from robustbnns_amd import _hip
    _hip.load()


def _engine(arch, act, D, H, C, S):
    from robustbnns_amd import AttackEngine, StackedPosterior
    post = O.synthetic_posterior(arch, D, H, C, S, 0.05)
    sp = StackedPosterior(arch, act, (1, D, 1), C, H, post, DEV)
    assert sp.triple_supported()
    eng = AttackEngine(sp, precision="triple")
    assert eng.precision == "triple"
    return eng, post


def _forward_bytes(eng, Xp, sidx, S, switch, monkeypatch):
    """One forward with the switch set -> {buffer: int32 copy of everything the forward kernels can write}.  The buffers are refilled with a
    pattern first (the hidden image with zeros: its rows past N are read as operands), so a store one form misses shows."""
    monkeypatch.setenv(SWITCH, switch)
    ws = eng.workspace(Xp.shape[0], S)
    bufs = {k: ws[k] for k in OUTPUTS if k in ws}
    for t in bufs.values():
        t.view(torch.int32).fill_(0x5A5A5A5A)
    if "hid_triple" in ws["triple"]:
        bufs["hid_triple"] = ws["triple"]["hid_triple"]
        bufs["hid_triple"].zero_()
    eng.forward_padded(Xp, sidx, S)
    torch.cuda.synchronize()
    return {k: t.view(torch.int32).clone() for k, t in bufs.items()}


# arch, act, D, H, N, seeds (S = 3 samples stored; None: the first two), buffers the case must have written
CASES = [
    ("fc", "leaky", 784, 512, 130, [2, 0, 1], ("P", "mask1")),          # one pair, odd KT, ragged second tile, permuted samples
    ("fc", "relu", 32, 512, 16, None, ("P", "mask1")),                  # one K stage: the first stage is the last one
    ("fc", "sigm", 64, 512, 130, None, ("P", "dact1")),                 # two K stages; act' as an fp32 stream
    ("fc", "leaky", 784, 1024, 130, [1, 2, 0], ("P", "mask1")),         # two pairs, odd KT: the X ring's parity runs across the hand-off
    ("fc", "relu", 64, 1024, 16, None, ("P", "mask1")),                 # two pairs, even KT
    ("fc", "leaky", 32, 1024, 130, None, ("P", "mask1")),               # two pairs of one K stage each
    ("fc", "relu", 784, 768, 130, None, ("P", "mask1")),                # three chunks: falls back to one chunk at a time
    ("fc", "leaky", 64, 256, 16, None, ("P", "mask1")),                 # one chunk: falls back
    ("fc", "relu", 784, 384, 130, None, ("P", "mask1")),                # the 4-wave form
    ("fc2", "leaky", 784, 512, 130, [2, 0, 1], ("P", "mask1", "mask2", "hid_triple")),   # layer 1 (hidden image) and the XF32 layer 2
    ("fc2", "relu", 32, 512, 16, None, ("P", "mask1", "mask2", "hid_triple")),
    ("fc2", "sigm", 64, 512, 130, None, ("P", "dact1", "dact2", "hid_triple")),
    ("fc2", "leaky", 64, 1024, 130, None, ("P", "mask1", "mask2", "hid_triple")),        # two pairs in both layers (layer 2: KT = 32)
]


@pytest.mark.parametrize("arch,act,D,H,N,seeds,written", CASES)
def test_two_chunk_forward_equals_the_one_chunk_forward_byte_for_byte(arch, act, D, H, N, seeds, written, monkeypatch):
    C, S = 10, (3 if seeds else 2)
    eng, _ = _engine(arch, act, D, H, C, 3)
    x, _ = O.synthetic_inputs(N, (1, D, 1), C, seed=7)
    Xp = eng.pad_inputs(x)
    sidx, S = eng.sample_index(S, seeds)
    assert (sidx is not None) == bool(seeds)
    off = _forward_bytes(eng, Xp, sidx, S, "0", monkeypatch)
    on = _forward_bytes(eng, Xp, sidx, S, "1", monkeypatch)
    assert set(written) <= set(on), sorted(on)
    for k in on:
        assert torch.equal(off[k], on[k]), f"{k}: {int((off[k] != on[k]).sum())} of {on[k].numel()} words differ between the two forms"
    for k in written:                                           # the comparison is of results, not of two untouched patterns
        fresh = 0 if k == "hid_triple" else 0x5A5A5A5A
        assert int((on[k] != fresh).sum()) > 0, k


def test_two_chunk_forward_against_the_fp64_oracle(monkeypatch):
    """D = 784, H = 512, N = 130 with the switch on: mean probabilities and loss_gradients vs the fp64 oracle, test_hip_triple.py's bound (gradients
    on the points whose pre-activations stay clear of the kink, as there)."""
    monkeypatch.setenv(SWITCH, "1")
    arch, act, D, H, C, S, N = "fc", "leaky", 784, 512, 10, 3, 130
    eng, post = _engine(arch, act, D, H, C, S)
    x, y = O.synthetic_inputs(N, (1, D, 1), C, seed=7)
    p64 = O.bnn_forward(x.double(), O.cast(post, torch.float64), arch, act, S)
    assert rel_err(eng.forward(x, S).cpu(), p64) < TOL
    ok = O.kink_margin(x.double(), O.cast(post, torch.float64), arch, act, S) > KINK
    assert int(ok.sum()) >= 0.4 * N
    g64 = O.loss_gradients(x.double(), y, O.cast(post, torch.float64), arch, act, S)
    assert rel_err(eng.loss_gradients(x, y, S).cpu()[ok], g64[ok]) < TOL
