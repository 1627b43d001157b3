"""Half-moons model grid: expected loss gradients and attacks for every stored BNN of a hyper-parameter grid — the call
surface of the reference's grid_search_halfMoons.py (MoonsBNN :18-25, _train / serial_train :30-50, serial_compute_grads :94-102,
grid_attack :133-153).

The reference trains the grid (`_train`: here HMC through BNN.train_hmc and SVI through BNN.train, fc / fc2 on the GPU; conv training is
out of scope: DESIGN.md section 7), then for every combination loads the HMC posterior from disk and runs `loss_gradients` / `attack` — on CPU through 10 joblib processes (:58-59, :91-92, :129-131).
Here every model is one resident posterior on the GPU and every (model, n_samples) cell one batched run over all test
points; the grid itself is a plain loop (the work per cell is milliseconds).  Dataset loading is out of scope as well,
so the caller passes the test tensors (`x_test [N,1,2,1]`, `y_test [N,2]` one-hot, as utils.load_dataset returns them).

`lockstep_train` is the counterpart of the reference's parallel_train (:52-59: 10 joblib processes, one model each): the HMC models of the
grid that differ only in their training-set size run as chains of ONE lockstep sampler (hmc.LockstepHmc: every kernel launch covers all of
them), and what it saves equals serial_train's bit for bit; the SVI models of one net shape run as members of ONE svi_train.LockstepSvi.
"""
import itertools

import torch

from torch.utils.data import DataLoader

from .adversarialAttacks import attack
from .flat_params import require_gpu_fc
from .lossGradients import loss_gradients
from .model_bnn import BNN
from .savedir import TESTS


class MoonsBNN(BNN):
    """grid_search_halfMoons.py:18-25: a BNN on half_moons whose name carries the training-set size."""

    def __init__(self, hidden_size, activation, architecture, inference, epochs, lr, n_samples, warmup, n_inputs,
                 input_shape, output_size):
        super(MoonsBNN, self).__init__("half_moons", hidden_size, activation, architecture, inference, epochs, lr, n_samples,
                                       warmup, input_shape, output_size, step_size=0.001)
        self.name = self.get_name(n_inputs)


def _combinations(*axes):
    return list(itertools.product(*axes))


def moons_loader(x_train, y_train, batch_size):
    """The reference's half-moons train loader (data_loaders(..., shuffle=False)) over tensors the caller passes."""
    return DataLoader(dataset=list(zip(x_train, y_train)), batch_size=batch_size, shuffle=False)


def _train(hidden_size, activation, architecture, inference, epochs, lr, n_samples, warmup, n_inputs, posterior_samples, rel_path, device,
           x_train=None, y_train=None, train_loader=None):
    """:30-41: one model of the grid.  Batch 64 for svi (BNN.train), 1024 for hmc (BNN.train_hmc); the data are x_train / y_train (the first
    n_inputs points) or a ready train_loader.  Returns the trained net."""
    require_gpu_fc("grid training", architecture)
    batch_size = 64 if inference == "svi" else 1024
    if train_loader is None:
        if x_train is None or y_train is None:
            raise ValueError("_train needs x_train / y_train or a train_loader: dataset loading is out of scope")
        train_loader = moons_loader(x_train[:n_inputs], y_train[:n_inputs], batch_size)
    x0, y0 = train_loader.dataset[0]
    bnn = MoonsBNN(hidden_size, activation, architecture, inference, epochs, lr, n_samples, warmup, n_inputs, tuple(x0.shape), int(y0.shape[-1]))
    if inference == "hmc":
        bnn.train_hmc(train_loader=train_loader, device=device, rel_path=rel_path)
    else:
        bnn.train(train_loader=train_loader, device=device, rel_path=rel_path)
    return bnn


def serial_train(hidden_size, activation, architecture, inference, epochs, lr, n_samples, warmup, n_inputs, posterior_samples, rel_path,
                 x_train=None, y_train=None, train_loader=None, device="cuda"):
    """:43-50: _train over the grid, one model after the other.  Returns {bnn.name: bnn}."""
    out = {}
    for init in _combinations(hidden_size, activation, architecture, inference, epochs, lr, n_samples, warmup, n_inputs, posterior_samples):
        bnn = _train(*init, rel_path, device, x_train=x_train, y_train=y_train, train_loader=train_loader)
        out[bnn.name] = bnn
    return out


def lockstep_train(hidden_size, activation, architecture, inference, epochs, lr, n_samples, warmup, n_inputs, posterior_samples, rel_path,
                   x_train=None, y_train=None, train_loader=None, device="cuda"):
    """serial_train with the HMC models of the grid sampled in lockstep.  The combinations that differ only in n_inputs and
    posterior_samples (and share the number of samples their last batch gets) form a group: one hmc.LockstepHmc whose chains have the same
    net shape, warmup and sample count and differ in their data, which are rows / counts into the resident x_train.  Every train_hmc reseeds
    with 0 and the moons loader does not shuffle, so each chain gets the start position and key it has in serial_train; before a chain's
    resample indices are drawn, the CPU generator is put back to the state it had after that chain's key was drawn.  Returns {bnn.name: bnn};
    names and saved tensors equal serial_train's.  The svi models that share (hidden, activation, architecture) form a group too: one
    svi_train.LockstepSvi through model_bnn.train_svi_lockstep, whatever their epochs, lr and n_inputs; saved parameters and epoch losses
    equal serial_train's, the epoch accuracies up to marginal points.  A ready train_loader goes through _train one by one."""
    from .hmc import LockstepHmc
    from .model_bnn import lockstep_history, train_svi_lockstep
    combos = _combinations(hidden_size, activation, architecture, inference, epochs, lr, n_samples, warmup, n_inputs, posterior_samples)
    out, groups, svi_groups = {}, {}, {}
    for init in combos:
        h, act, arch, inf, ep, lr_, ns, wu, ninp, _ = init
        if inf == "svi" and train_loader is None:
            require_gpu_fc("grid training", arch)
            require_gpu_fc("SVI training", device=device)
            if x_train is None or y_train is None:
                raise ValueError("lockstep_train needs x_train / y_train or a train_loader: dataset loading is out of scope")
            # one member per (epochs, lr, n_samples, warmup, n_inputs) of a net shape, in the grid's order: posterior_samples repeats the model
            svi_groups.setdefault((h, act, arch), {}).setdefault((ep, lr_, ns, wu, ninp), None)
            out[MoonsBNN(h, act, arch, inf, ep, lr_, ns, wu, ninp, tuple(x_train[0].shape), int(y_train.shape[-1])).name] = None
            continue
        if inf != "hmc" or train_loader is not None:
            bnn = _train(*init, rel_path, device, x_train=x_train, y_train=y_train, train_loader=train_loader)
            out[bnn.name] = bnn
            continue
        require_gpu_fc("grid training", arch)
        require_gpu_fc("HMC", device=device)
        if x_train is None or y_train is None:
            raise ValueError("lockstep_train needs x_train / y_train or a train_loader: dataset loading is out of scope")
        members = groups.setdefault((h, act, arch, ep, lr_, ns, wu), {})
        members.setdefault(ninp, None)                                   # one chain per training-set size, in the grid's order
        out[MoonsBNN(h, act, arch, inf, ep, lr_, ns, wu, ninp, tuple(x_train[0].shape), int(y_train.shape[-1])).name] = None
    for (h, act, arch), members in svi_groups.items():
        nets = [MoonsBNN(h, act, arch, "svi", ep, lr_, ns, wu, ninp, tuple(x_train[0].shape), int(y_train.shape[-1]))
                for (ep, lr_, ns, wu, ninp) in members]
        train_svi_lockstep(nets, x_train, y_train, [m[4] for m in members], device, rel_path=rel_path, batch_size=64)
        for bnn in nets:
            out[bnn.name] = bnn
    labels = None if y_train is None else y_train.argmax(-1)
    for (h, act, arch, ep, lr_, ns, wu), members in groups.items():
        chains = {}                                                      # batch_samples -> [(bnn, first row, count, q0, key, generator state)]
        for ninp in members:
            loader = moons_loader(x_train[:ninp], y_train[:ninp], 1024)
            x0, y0 = loader.dataset[0]
            bnn = MoonsBNN(h, act, arch, "hmc", ep, lr_, ns, wu, ninp, tuple(x0.shape), int(y0.shape[-1]))
            x_batch, _, batch_samples, q0, key = bnn._hmc_prologue(loader, device)
            n = len(loader.dataset)
            chains.setdefault(batch_samples, []).append((bnn, n - int(x_batch.shape[0]), int(x_batch.shape[0]), q0, key, torch.get_rng_state()))
        for batch_samples, cs in chains.items():
            B = max(c[2] for c in cs)
            rows = torch.zeros(len(cs), B, dtype=torch.int32)
            for k, c in enumerate(cs):
                rows[k, :c[2]] = torch.arange(c[1], c[1] + c[2], dtype=torch.int32)
            b = cs[0][0].basenet
            sampler = LockstepHmc(b.architecture, b.activation, b.input_shape, b.output_size, [c[3] for c in cs], cs[0][0].step_size,
                                  cs[0][0].num_steps, device, [c[4] for c in cs], batch_size=B)
            sampler.set_data(x_train, labels)
            stacks = sampler.run(rows=rows, counts=[c[2] for c in cs], num_samples=batch_samples, warmup=wu)
            for k, (bnn, _, _, _, _, rng) in enumerate(cs):
                torch.set_rng_state(rng)
                idx = torch.randint(0, batch_samples, (bnn.n_samples,)).to(device)
                bnn.hmc_history = lockstep_history(sampler, k, idx)
                bnn.set_posterior_samples({key_: v.index_select(0, idx).contiguous() for key_, v in stacks[k].items()}, device)
                bnn.save(rel_path=rel_path, filename=None)
                out[bnn.name] = bnn
    return out


def serial_compute_grads(hidden_size, activation, architecture, inference, epochs, lr, n_samples, warmup, n_inputs,
                         posterior_samples, rel_path, x_test, y_test, device="cuda"):
    """:94-102 (+ _compute_grads :66-78): loss_gradients of every model x posterior_samples; pickles land where the
    reference puts them (DATA + <bnn.name>/ + <bnn.name>_samp=<S>_lossGrads.pkl).  Returns {(bnn.name, S): ndarray}."""
    input_shape, output_size = tuple(x_test.shape[1:]), int(y_test.shape[-1])
    loader = DataLoader(dataset=list(zip(x_test, y_test)), batch_size=32, shuffle=False)
    out = {}
    for (h, act, arch, inf, ep, lr_, ns, wu, ninp, psamp) in _combinations(hidden_size, activation, architecture, inference, epochs,
                                                                       lr, n_samples, warmup, n_inputs, posterior_samples):
        bnn = MoonsBNN(h, act, arch, inf, ep, lr_, ns, wu, ninp, input_shape, output_size)
        bnn.load(device=device, rel_path=rel_path)
        out[(bnn.name, psamp)] = loss_gradients(net=bnn, n_samples=psamp, savedir=bnn.name + "/", data_loader=loader,
                                                device=device, filename=bnn.name)
    return out


def grid_attack(method, hidden_size, activation, architecture, inference, epochs, lr, n_samples, warmup, n_inputs,
                posterior_samples, x_test, y_test, device="cuda", rel_path=TESTS):
    """:133-153: every model is loaded once and attacked with each number of posterior samples.  Returns
    {(bnn.name, S): x_attack}; the attack pickles / PNGs are written by `attack` as in the reference."""
    input_shape, output_size = tuple(x_test.shape[1:]), int(y_test.shape[-1])
    out = {}
    for init in _combinations(hidden_size, activation, architecture, inference, epochs, lr, n_samples, warmup, n_inputs):
        bnn = MoonsBNN(*init, input_shape, output_size)
        bnn.load(device=device, rel_path=rel_path)
        for p_samp in posterior_samples:
            out[(bnn.name, p_samp)] = attack(net=bnn, x_test=x_test, y_test=y_test, dataset_name="half_moons", device=device,
                                             method=method, filename=bnn.name, n_samples=p_samp)
    return out
