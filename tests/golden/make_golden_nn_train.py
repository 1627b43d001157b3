#!/usr/bin/env python3
"""Golden vectors of deterministic TRAINING: the reference's own NN.train (model_nn.py:175-219) and Ensemble_NN.train
(model_ensemble.py:69-83) on small data, run on the CPU.

    python tests/golden/make_golden_nn_train.py

Both functions are imported unmodified from the reference checkout (ROBUSTBNNS_REFERENCE) behind the inert keras / pyro stubs of
make_golden.py and run as they are:

  * NN.train gets an observing wrapper around its (unshuffled) loader that records the net's state_dict whenever a batch is fetched, i.e.
    the parameters BEFORE every step;
  * Ensemble_NN.train builds its own DataLoader(..., batch_size=100, shuffle=True) per member: the name `DataLoader` in its module is bound
    to a subclass that records the batches it yields, and the row indices are recovered from the (unique) rows of x.

Only arrays and the printed epoch lines are stored; no reference source is copied.  Every fixture carries `spread`: the largest distance of
the reference's fp32 result from the fp64 restatement (tests/nn_restate.py) of the same run, relative to the largest parameter — what two
correct implementations in different precisions differ by on this run.
"""
import contextlib
import copy
import io
import os
import shutil
import sys
import tempfile

import numpy as np
import torch
from torch.utils.data import DataLoader

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as MG                                             # noqa: E402  (stubs)


@contextlib.contextmanager
def captured():
    """The reference prints its epoch lines and writes weight files under relative directories: a scratch cwd, stdout kept."""
    cwd, tmp, buf = os.getcwd(), tempfile.mkdtemp(), io.StringIO()
    os.chdir(tmp)
    try:
        with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(io.StringIO()):
            yield buf
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp, ignore_errors=True)


class ObservedLoader:
    def __init__(self, loader, net):
        self.loader, self.net, self.dataset, self.states = loader, net, loader.dataset, []

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for batch in self.loader:
            self.states.append(copy.deepcopy(self.net.state_dict()))
            yield batch


def data_of(kind, n, seed):
    import nn_restate  # noqa: F401  (path check)
    import svi_restate as R
    from oracle import bnn_oracle as O
    if kind == "moons":
        x, y = R.two_moons(n, 0.1, seed)
        return x, y, (1, 2, 1), 2
    x, y = O.synthetic_inputs(n, (1, 4, 4), 10, seed)
    return x, y, (1, 4, 4), 10


def write(name, out, meta):
    out["meta"] = np.array(repr(meta))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)  spread {meta['spread']:.3e}")


def run_nn(name, kind, arch, act, hidden, lr, n=150, batch=64, epochs=2, seed0=11, seed=0):
    import model_nn
    import nn_restate as NR
    x, y, shape, C = data_of(kind, n, seed0)
    torch.manual_seed(seed0)
    net = model_nn.NN(dataset_name="half_moons" if kind == "moons" else "mnist", input_shape=shape, output_size=C, hidden_size=hidden,
                      activation=act, architecture=arch, lr=lr, epochs=epochs)
    init = copy.deepcopy(net.state_dict())
    obs = ObservedLoader(DataLoader(dataset=list(zip(x, y)), batch_size=batch, shuffle=False), net)
    with captured() as buf:
        net.train(obs, "cpu", seed=seed, save=False)
    lines = NR.parse_epoch_lines(buf.getvalue())
    assert len(lines) == epochs and len(obs.states) == epochs * len(obs) and n % batch
    out = {"x": x.numpy(), "y": y.numpy()}
    out.update({"init:" + k: v.numpy() for k, v in init.items()})
    for i, st in enumerate(obs.states):
        out.update({f"step{i}:" + k: v.numpy() for k, v in st.items()})
    final = {k: v.detach().clone() for k, v in net.state_dict().items()}
    out.update({"final:" + k: v.numpy() for k, v in final.items()})
    meta = dict(kind="nn", dataset=net.dataset_name, shape=list(shape), n_classes=C, hidden=hidden, act=act, arch=arch, lr=lr, epochs=epochs,
                N=n, batch=batch, seed0=seed0, seed=seed, steps=len(obs.states), lines=lines, torch=torch.__version__)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out, meta=np.array(repr(dict(meta, spread=0.0))))
    r64, _ = NR.run_nn_case(name, torch.float64)
    meta["spread"] = NR.max_diff(final, r64.params()) / NR.param_scale(r64.params())
    write(name, out, meta)


class RecordingLoader(DataLoader):
    seen = []

    def __iter__(self):
        epoch = []
        RecordingLoader.seen.append(epoch)
        for xb, yb in super().__iter__():
            epoch.append(xb.clone())
            yield xb, yb


def run_ens(name, kind, arch, act, hidden, lr, M=3, n=250, epochs=2, seed0=23):
    import model_ensemble
    import nn_restate as NR
    x, y, shape, C = data_of(kind, n, seed0)
    assert len({r.numpy().tobytes() for r in x}) == n, "the rows of x must be unique: the batches are recovered from them"
    index = {r.numpy().tobytes(): i for i, r in enumerate(x)}
    torch.manual_seed(seed0)
    ens = model_ensemble.Ensemble_NN(dataset_name="half_moons" if kind == "moons" else "mnist", hidden_size=hidden, activation=act,
                                     architecture=arch, epochs=epochs, lr=lr, input_shape=shape, output_size=C, ensemble_size=M)
    inits = []
    real_nn = model_ensemble.NN

    def observed_nn(*a, **k):                                        # the member as constructed: its initial parameters
        net = real_nn(*a, **k)
        inits.append(copy.deepcopy(net.state_dict()))
        return net
    RecordingLoader.seen = []
    model_ensemble.DataLoader, model_ensemble.NN = RecordingLoader, observed_nn
    try:
        with captured() as buf:
            ens.train(x_train=x, y_train=y, device="cpu")
    finally:
        model_ensemble.DataLoader, model_ensemble.NN = DataLoader, real_nn
    lines = NR.parse_epoch_lines(buf.getvalue())
    assert len(inits) == M and len(RecordingLoader.seen) == M * epochs and len(lines) == M * epochs and n % 100
    rows = np.zeros((M, epochs, n), dtype=np.int32)
    for j, ep in enumerate(RecordingLoader.seen):
        got = [index[r.numpy().tobytes()] for b in ep for r in b]
        assert sorted(got) == list(range(n))
        rows[j // epochs, j % epochs] = got
    out = {"x": x.numpy(), "y": y.numpy(), "rows": rows}
    finals = []
    for m in range(M):
        out.update({f"init{m}:" + k: v.numpy() for k, v in inits[m].items()})
        finals.append({k: v.detach().clone() for k, v in ens.ensemble_models[str(m)].state_dict().items()})
        out.update({f"final{m}:" + k: v.numpy() for k, v in finals[m].items()})
    meta = dict(kind="ens", dataset=ens.dataset_name, shape=list(shape), n_classes=C, hidden=hidden, act=act, arch=arch, lr=lr, epochs=epochs,
                N=n, M=M, batch=100, seed0=seed0, lines=lines, torch=torch.__version__)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out, meta=np.array(repr(dict(meta, spread=0.0))))
    r64 = NR.run_ens_case(name, torch.float64)
    meta["spread"] = max(NR.max_diff(finals[m], r64[m].params()) / NR.param_scale(r64[m].params()) for m in range(M))
    write(name, out, meta)


def main():
    MG._install_stubs()
    sys.path.insert(0, MG.REF)
    torch.set_num_threads(1)
    run_nn("nn_train_nn_moons_fc2_h32", "moons", "fc2", "leaky", 32, 0.02)
    run_nn("nn_train_nn_small_fc_h16", "small", "fc", "tanh", 16, 0.01)
    run_ens("nn_train_ens_moons_fc_h32", "moons", "fc", "leaky", 32, 0.02)
    run_ens("nn_train_ens_small_fc2_h16", "small", "fc2", "sigm", 16, 0.01)


if __name__ == "__main__":
    main()
