"""Bayesian network — the call surface of the reference's model_bnn.BNN (model_bnn.py:69-391).

`forward(inputs, n_samples, avg_posterior, seeds)` is the Monte-Carlo posterior predictive of
model_bnn.py:198-258, computed for the whole batch and all samples by the HIP kernels:

  hmc  the stored chain is one StackedPosterior; `seeds` index it (model_bnn.py:246-252);
  svi  weights are drawn as loc + softplus(scale) * eps (model_bnn.py:124-130).  On the GPU ONE kernel (fc / fc2:
       rbnn_svi_draw, writing the fp32 stack AND the packed / triple images; conv: rbnn_svi_draw_flat + the image
       builders; Philox eps in registers) redraws all S samples IN PLACE, so the posterior, its engine and its workspaces
       are reused draw after draw and a redraw contains no device->host sync.  RBNN_SVI_RNG=host: eps from torch's CPU
       generator in the guide's order -> rbnn_svi_materialize -> a new stacked posterior per draw.
       PARITY UNPINNED for the draw itself (pyro-ppl 1.3.0 is not available to check RNG order against); everything
       downstream of explicit weights is pinned.

Training: `train(train_loader, device, rel_path, filename)` runs the reference's SVI training (model_bnn.py:303-365) for fc / fc2 on the GPU
(svi_train.SviTrainer: one weight draw, the training forward, the weight gradients and one Adam step per batch — csrc/rbnn_train.hip) and
saves the param store.  `train_conv(train_loader, device, rel_path, filename)` runs the same algorithm for a conv net of the 1x28x28 geometry
(conv_svi_train.ConvSviTrainer around the conv training forward and weight gradients, csrc/rbnn_conv_train.hip); `train()` itself keeps
refusing conv.  `train_conv_svi_lockstep(nets, x_train, y_train, device)` is train_conv for several conv nets of one shape at once
(conv_svi_train.ConvLockstepSvi: every launch covers all of them; each net's files and history are train_conv's bit for bit).  CPU devices
and the 3x32x32 geometry raise NotImplementedError.  `train()`
refuses an HMC net too and names `train_hmc(train_loader, device, rel_path, filename, num_chains=1)`, which samples the chain of an fc / fc2
net on the GPU (hmc.HmcSampler, csrc/rbnn_hmc.hip; num_chains = K > 1: K chains in lockstep, hmc.LockstepHmc, pooled and judged by their
split-R-hat) and writes the per-sample files `load()` reads.  `train_hmc_conv(train_loader, device, rel_path, filename, num_chains=1,
group=None)` is train_hmc for a conv net of the 1x28x28 geometry (conv_hmc.ConvHmcSampler: the same chain kernels around the conv training
forward and weight gradients; num_chains = K > 1: conv_hmc.ConvLockstepHmc, K chains behind every launch in groups that fit the conv
workspace budget, pooled and judged by their split-R-hat); `train_hmc()` itself keeps refusing conv.
"""
import os
import random

import numpy as np
import torch
from torch import nn

from . import _hip
from .factory import make_engine, posterior_from_stacked, posterior_from_state_dicts
from .flat_params import require_gpu_fc, state_shapes
from .model_nn import NN
from .savedir import TESTS

saved_BNNs = {"model_0": ["mnist", {"hidden_size": 512, "activation": "leaky", "architecture": "conv", "inference": "svi", "epochs": 5, "lr": 0.01, "n_samples": None, "warmup": None}],
              "model_1": ["mnist", {"hidden_size": 512, "activation": "leaky", "architecture": "fc2", "inference": "hmc", "epochs": None, "lr": None, "n_samples": 100, "warmup": 50}],
              "model_2": ["fashion_mnist", {"hidden_size": 1024, "activation": "leaky", "architecture": "conv", "inference": "svi", "epochs": 10, "lr": 0.001, "n_samples": None, "warmup": None}],
              "model_3": ["fashion_mnist", {"hidden_size": 1024, "activation": "leaky", "architecture": "fc2", "inference": "hmc", "epochs": None, "lr": None, "n_samples": 100, "warmup": 50}],
              "model_4": ["fashion_mnist", {"hidden_size": 1024, "activation": "leaky", "architecture": "conv", "inference": "svi", "epochs": 5, "lr": 0.01, "n_samples": None, "warmup": None}],
              "model_5": ["mnist", {"hidden_size": 512, "activation": "leaky", "architecture": "fc2", "inference": "svi", "epochs": 10, "lr": 0.01, "n_samples": None, "warmup": None}],
              "model_6": ["mnist", {"hidden_size": 256, "activation": "leaky", "architecture": "conv", "inference": "svi", "epochs": 10, "lr": 0.05, "n_samples": None, "warmup": None}],
              "model_7": ["mnist", {"hidden_size": 1024, "activation": "leaky", "architecture": "fc2", "inference": "svi", "epochs": 5, "lr": 0.02, "n_samples": None, "warmup": None}],
              "model_8": ["mnist", {"hidden_size": 1024, "activation": "leaky", "architecture": "conv", "inference": "svi", "epochs": 10, "lr": 0.02, "n_samples": None, "warmup": None}],
              "model_9": ["fashion_mnist", {"hidden_size": 512, "activation": "leaky", "architecture": "fc", "inference": "hmc", "epochs": None, "lr": None, "n_samples": 100, "warmup": 100}]}


def set_rng_seed(seed):
    """What pyro.set_rng_seed does (torch + random + numpy) — model_bnn.py:224,358,374."""
    torch.manual_seed(seed)
    random.seed(seed)
    np.random.seed(seed)


def param_store_state(loc, scale):
    """The dict pyro 1.3.0's ParamStoreDict.save() pickles (pyro/params/param_store.py get_state(), [recalled]; the reference
    writes it at model_bnn.py:148-155): {"params": {name: UNCONSTRAINED value, a leaf tensor with requires_grad},
    "constraints": {name: torch.distributions constraint}}.  The guide's params `<key>_loc` / `<key>_scale` (:125-126) are
    registered without a constraint, i.e. constraints.real, for which unconstrained == constrained."""
    from torch.distributions import constraints
    params = {}
    for k, v in loc.items():
        params[k + "_loc"] = v.detach().cpu().clone().requires_grad_(True)
    for k, v in scale.items():
        params[k + "_scale"] = v.detach().cpu().clone().requires_grad_(True)
    return {"params": params, "constraints": {name: constraints.real for name in params}}


def read_param_store(path):
    """name -> CONSTRAINED fp32 tensor from a pyro param-store file (what pyro.get_param_store().load() + iteration yields,
    model_bnn.py:177-181).  Unconstrained values go through transform_to(constraint), the identity for constraints.real.
    Also accepts a bare {name: tensor} dict.  weights_only=False: the file pickles constraint objects."""
    from torch.distributions import constraints, transform_to
    store = torch.load(path, map_location="cpu", weights_only=False)
    if not isinstance(store, dict):
        raise TypeError(f"{path}: malformed ParamStore state ({type(store).__name__})")
    if "params" not in store:
        return {k: v.detach().to(torch.float32) for k, v in store.items()}
    if set(store.keys()) != {"params", "constraints"}:
        raise KeyError(f"{path}: malformed ParamStore keys {sorted(store.keys())}")
    out = {}
    for name, value in store["params"].items():
        c = store["constraints"].get(name, constraints.real)
        c = constraints.real if isinstance(c, type(constraints.real)) else c       # pyro's own unpickling workaround
        value = value.detach()
        out[name] = (value if c is constraints.real else transform_to(c)(value)).to(torch.float32)
    return out


def lockstep_history(sampler, k=None, idx=None):
    """One chain's logs in the layout of BNN.hmc_history: chain k of a lockstep sampler (hmc.LockstepHmc, conv_hmc.ConvLockstepHmc: its logs
    are lists with one entry per chain), or with k None the chain of a single sampler (its logs are the attributes themselves)."""
    of = (lambda v: v) if k is None else (lambda v: v[k])
    h = {"eps": of(sampler.eps_log), "L": of(sampler.L_log), "dH": of(sampler.dH_log), "accept_prob": of(sampler.accept_prob_log),
         "accepted": of(sampler.accepted_log), "m_inv": of(sampler.m_inv).cpu(), "key": sampler.key if k is None else sampler.chain_keys[k]}
    if idx is not None:
        h["resampled"] = idx.cpu()
    return h


def lockstep_r_hat(log, warmup):
    """Split-R-hat of the chains' potential (the logged U_new of log [K, transitions, columns]) over the sampling phase; nan with fewer than
    4 samples or one chain."""
    from .hmc import LOG_COLUMNS, split_r_hat
    U = log[:, warmup:, LOG_COLUMNS.index("U_new")]
    return split_r_hat(U) if U.shape[1] >= 4 else float("nan")


def require_one_shape(nets):
    """The lockstep SVI drivers' refusal of nets that differ in shape from the first."""
    shape_of = lambda b: (b.architecture, b.activation, tuple(b.input_shape), int(b.output_size), int(b.hidden_size))
    for net in nets[1:]:
        if shape_of(net.basenet) != shape_of(nets[0].basenet):
            raise ValueError(f"lockstep SVI nets share one net shape: {shape_of(net.basenet)} is not {shape_of(nets[0].basenet)}")


def svi_lockstep_prologue(net):
    """What BNN.train draws from the host generators before its first step, in its order: the seeding, the base seed a DataLoader's iterator
    takes from the CPU generator when the first epoch's loop creates it, the guide's initial parameters (unless the net holds some) and the
    key.  -> (loc, raw, key)."""
    from torch.utils.data import DataLoader
    from .svi_train import draw_key, initial_params
    random.seed(0)
    set_rng_seed(0)
    iter(DataLoader([0], batch_size=1))
    if net.svi_loc is None:
        loc, raw = initial_params(state_shapes(net.basenet))
    else:
        loc, raw = net.svi_loc, net.svi_scale
    return loc, raw, draw_key()


def svi_lockstep_prologues(nets, device):
    """svi_lockstep_prologue of every net in order, each put on `device` first -> (locs, raws, keys)."""
    locs, raws, keys = [], [], []
    for net in nets:
        net.device = device
        net.basenet.device = device
        loc, raw, key = svi_lockstep_prologue(net)
        locs.append(loc); raws.append(raw); keys.append(key)
    return locs, raws, keys


def record_svi_lockstep(trainer, nets, n_points, device, rel_path):
    """The end of a lockstep run, net by net as BNN.train prints and saves: the epoch lines from the trainer's epoch_totals() (net k saw
    n_points[k] points an epoch), training_history, set_variational_params from trainer.params(k), and save()."""
    totals = trainer.epoch_totals()
    for k, net in enumerate(nets):
        print("\n == SVI training ==")
        n, loss_list, accuracy_list = n_points[k], [], []
        for epoch in range(net.epochs):
            loss, correct = totals[k][epoch]
            print(f"\n[Epoch {epoch + 1}]\t loss: {loss / n:.2f} \t accuracy: {100 * correct / n:.2f}", end="\t")
            loss_list.append(loss)
            accuracy_list.append(100 * correct / n)
        net.training_history = {"loss": loss_list, "accuracy": accuracy_list}
        loc, raw = trainer.params(k)
        net.set_variational_params(loc, raw, device)
        net.save(rel_path=rel_path, filename=None)


def train_svi_lockstep(nets, x_train, y_train, n_inputs, device, rel_path=TESTS, batch_size=64):
    """BNN.train for several SVI nets of ONE net shape at once (svi_train.LockstepSvi: every kernel launch covers all of them).  The nets may
    differ in epochs, lr and training-set size: member k trains on x_train[:n_inputs[k]] in order, unshuffled, in batches of batch_size (what
    grid_search_halfMoons.moons_loader yields).  Each member takes its init and key exactly as BNN.train would, prints its epoch lines, and gets
    training_history, set_variational_params and save(): parameters and epoch losses equal BNN.train's bit for bit; the epoch accuracies may
    differ at points whose two largest mean probabilities lie within the forward kernels' error of each other (another GEMM tile plan).
    Shuffled or arbitrary loaders stay with BNN.train."""
    nets = list(nets)
    if not nets or len(n_inputs) != len(nets):
        raise ValueError(f"train_svi_lockstep needs one n_inputs per net, not {len(n_inputs)} for {len(nets)} nets")
    for net in nets:
        if net.inference != "svi":
            raise NotImplementedError("train() runs SVI only: sample an HMC posterior with BNN.train_hmc(train_loader, device) (fc / fc2) or "
                                      "BNN.train_hmc_conv(train_loader, device) (conv, 1x28x28)")
        require_gpu_fc("SVI training", net.basenet.architecture)
    require_gpu_fc("SVI training", device=device)
    b0 = nets[0].basenet
    require_one_shape(nets)
    n_inputs =[min(int(n), int(x_train.shape[0])) for n in n_inputs]
    if min(n_inputs) < 1:
        raise ValueError("every member needs at least one training point")
    from .svi_train import LockstepSvi
    locs, raws, keys = svi_lockstep_prologues(nets, device)
    trainer = LockstepSvi(b0.architecture, b0.activation, b0.input_shape, b0.output_size, locs, raws, [net.lr for net in nets], device, keys,
                          batch_size=int(batch_size))
    trainer.set_data(x_train, y_train.argmax(-1))
    trainer.run(LockstepSvi.schedule(n_inputs, [net.epochs for net in nets], int(batch_size)))
    record_svi_lockstep(trainer, nets, n_inputs, device, rel_path)
    return trainer


def train_conv_svi_lockstep(nets, x_train, y_train, device, rel_path=TESTS, batch_size=128, group=None):
    """BNN.train_conv for several SVI conv nets of ONE net shape (1x28x28) at once, the counterpart of train_svi_lockstep
    (conv_svi_train.ConvLockstepSvi: every kernel launch covers all of a group's nets).  The nets may differ in epochs and lr; every net
    trains on all of x_train in order, unshuffled, in batches of batch_size with a short last batch.  Each net takes its initialisation and
    key exactly as BNN.train_conv would (svi_lockstep_prologue) unless it already holds parameters, prints its epoch lines and gets
    training_history, set_variational_params and save(): parameters, losses and accuracies are BNN.train_conv's on an unshuffled DataLoader of
    the same data and batch size, bit for bit.  group: nets trained at a time — None: all of them when their workspaces fit the
    RBNN_CONV_WS_GB budget, else the largest group that does (conv_svi_lockstep_group); the groups follow one another and no net's bits depend
    on the grouping.  Every refusal comes before any state is changed, a generator touched or the library loaded."""
    nets = list(nets)
    if not nets:
        raise ValueError("train_conv_svi_lockstep needs at least one net")
    for net in nets:
        if net.inference == "hmc":
            raise NotImplementedError("train_conv_svi_lockstep() runs SVI only: an HMC posterior is sampled with BNN.train_hmc(train_loader, device) for "
                                      "fc / fc2 and with BNN.train_hmc_conv(train_loader, device) for a conv net of the 1x28x28 geometry")
        if net.basenet.architecture != "conv":
            raise ValueError(f"train_conv_svi_lockstep trains the conv architecture; a {net.basenet.architecture!r} net trains through "
                             "train_svi_lockstep")
    from .conv_train import check_conv_trainable
    for net in nets:
        check_conv_trainable(net.basenet.input_shape, device)
    b0 = nets[0].basenet
    require_one_shape(nets)
    names =[net.name for net in nets]
    for name in names:
        if names.count(name) > 1:
            raise ValueError(f"two nets are named {name!r}: their saved files would overwrite each other (give them different epochs or lr, or "
                             "train them in separate calls under different rel_path)")
    n = int(x_train.shape[0])
    if n < 1 or int(batch_size) < 1 or (group is not None and int(group) < 1):
        raise ValueError(f"train_conv_svi_lockstep needs at least one training point, batch_size >= 1 and group >= 1 (got {n}, {batch_size}, {group})")
    from .conv_svi_train import ConvLockstepSvi, conv_svi_lockstep_group
    B = min(int(batch_size), n)
    if group is None:
        group = conv_svi_lockstep_group(b0.activation, b0.hidden_size, b0.output_size, len(nets), B)
    x_dev, lab_dev = x_train.to(device), y_train.argmax(-1).to(device)
    for first in range(0, len(nets), int(group)):
        members = nets[first:first + int(group)]
        locs, raws, keys = svi_lockstep_prologues(members, device)
        trainer = ConvLockstepSvi(b0.activation, b0.input_shape, b0.output_size, locs, raws, [net.lr for net in members], device, keys, batch_size=B)
        trainer.set_data(x_dev, lab_dev)
        trainer.run(ConvLockstepSvi.schedule(n, [net.epochs for net in members], B))
        record_svi_lockstep(trainer, members, [n] * len(members), device, rel_path)
        del trainer


class BNN(nn.Module):

    def __init__(self, dataset_name, hidden_size, activation, architecture, inference, epochs, lr, n_samples, warmup,
                 input_shape, output_size, step_size=0.005, num_steps=10):
        super(BNN, self).__init__()
        self.dataset_name = dataset_name
        self.inference = inference
        self.architecture = architecture
        self.epochs = epochs
        self.lr = lr
        self.n_samples = n_samples
        self.warmup = warmup
        self.step_size = step_size
        self.num_steps = num_steps
        self.basenet = NN(dataset_name=dataset_name, input_shape=input_shape, output_size=output_size,
                          hidden_size=hidden_size, activation=activation, architecture=architecture, epochs=epochs, lr=lr)
        self.name = self.get_name()
        self.posterior = None                 # hmc: StackedPosterior of the chain
        self.svi_loc = self.svi_scale = None  # svi: dict key -> tensor (raw scale, softplus applied at draw)
        # SVI draws.  "device" (default): eps comes from the GPU generator — fresh from the live generator without seeds (the
        # reference draws from the live global RNG too), one generator re-seeded per seed otherwise (same seed -> same weights,
        # whatever the other seeds are).  "host": a CPU restatement of the guide's draw order (2 discarded tensors per key, then
        # one per parameter) — same-seed parity with pyro is unpinned either way, and at MNIST fc-512 the
        # host loop costs 3.7 s per 100 draws against 2.4 ms for the whole forward.
        self.svi_rng = os.environ.get("RBNN_SVI_RNG", "device")
        self._engine = None
        self._drawn = None                    # svi: (key, engine) of the last SEEDED draw (same seeds -> same weights: reused, not redrawn)
        self._guide = None                    # svi, fc / fc2: posterior.SviGuide of the current parameters (bounds fixed once per guide)
        self._slots = {}                      # svi: n_samples -> (StackedPosterior.for_guide, engine) redrawn in place by unseeded calls
        self._draws = 0                       # number of in-place redraws so far

    def get_name(self, n_inputs=None):
        """model_bnn.py:90-103"""
        name = str(self.dataset_name) + "_bnn_" + str(self.inference) + "_hid=" + str(self.basenet.hidden_size) + \
               "_act=" + str(self.basenet.activation) + "_arch=" + str(self.basenet.architecture)
        if n_inputs:
            name = name + "_inp=" + str(n_inputs)
        if self.inference == "svi":
            return name + "_ep=" + str(self.epochs) + "_lr=" + str(self.lr)
        elif self.inference == "hmc":
            return name + "_samp=" + str(self.n_samples) + "_warm=" + str(self.warmup) + \
                   "_stepsize=" + str(self.step_size) + "_numsteps=" + str(self.num_steps)

    # ------------------------------------------------------------------ posterior in
    def _make_posterior(self, stacked, device):
        b = self.basenet
        return posterior_from_stacked(b.architecture, b.activation, b.input_shape, b.output_size, b.hidden_size, stacked, device)

    def set_posterior_samples(self, samples, device):
        """hmc: `samples` = list of NN.state_dict()s (what load() reads from disk), or a dict key -> [S,...]."""
        self.device = device
        self.basenet.device = device
        if isinstance(samples, dict):
            self.posterior = self._make_posterior(samples, device)
        else:
            b = self.basenet
            self.posterior = posterior_from_state_dicts(samples, b.architecture, b.activation, b.input_shape,
                                                        b.output_size, b.hidden_size, device)
        self._engine = make_engine(self.posterior)

    def set_variational_params(self, loc, scale, device):
        """svi: dicts state_dict-key -> tensor, the `<key>_loc` / `<key>_scale` params of model_bnn.py:125-126."""
        self.device = device
        self.basenet.device = device
        self.svi_loc = {k: v.detach().to(device, torch.float32).contiguous() for k, v in loc.items()}
        self.svi_scale = {k: v.detach().to(device, torch.float32).contiguous() for k, v in scale.items()}
        self._engine = None
        self._drawn, self._guide, self._slots = None, None, {}     # nothing drawn from the previous guide may be served for this one

    @property
    def posterior_predictive(self):
        """dict idx -> NN carrying sample idx (the reference's attribute, model_bnn.py:186-190); built on demand."""
        import copy
        out = {}
        for i in range(self.posterior.S):
            net = copy.deepcopy(self.basenet)
            net.load_state_dict(self.posterior.state_dict(i))
            out[i] = net
        return out

    def save(self, rel_path=TESTS, filename=None):
        """hmc branch of model_bnn.py:138-165: one state_dict file per stored sample."""
        if filename is None:
            filename = self.name + "_weights"
        path = rel_path + self.name + "/"
        os.makedirs(os.path.dirname(path), exist_ok=True)
        if self.inference == "hmc":
            for key, value in self.posterior_predictive.items():
                torch.save(value.state_dict(), path + filename + "_" + str(key) + ".pt")
        else:
            torch.save(param_store_state(self.svi_loc, self.svi_scale), path + filename + ".pt")

    def load(self, device, rel_path=TESTS, filename=None):
        """model_bnn.py:167-196"""
        if filename is None:
            filename = self.name + "_weights"
        path = rel_path + self.name + "/"
        if self.inference == "svi":
            params = read_param_store(path + filename + ".pt")
            keys = list(self.basenet.state_dict().keys())
            missing = [k + sfx for k in keys for sfx in ("_loc", "_scale") if k + sfx not in params]
            if missing:
                raise KeyError(f"param store {path + filename}.pt lacks {missing[:4]}{'...' if len(missing) > 4 else ''} "
                               f"(has {sorted(params)[:4]}...): not written by this architecture's guide (model_bnn.py:124-126)")
            self.set_variational_params({k: params[k + "_loc"] for k in keys}, {k: params[k + "_scale"] for k in keys}, device)
            print("\nLoading ", path + filename + ".pt\n")
        elif self.inference == "hmc":
            sds = [torch.load(path + filename + "_" + str(i) + ".pt", map_location="cpu") for i in range(self.n_samples)]
            if len(sds) != self.n_samples:
                raise AttributeError("wrong number of posterior models")
            self.set_posterior_samples(sds, device)

    # ------------------------------------------------------------------ svi draws
    def _svi_eps(self, n_samples, seeds):
        """eps per draw in the order the guide consumes the RNG ([recalled]): for every
        state_dict key two discarded randn_like (the eagerly evaluated pyro.param initialisers,
        model_bnn.py:125-126), then one standard normal per parameter in named_parameters() order."""
        shapes = state_shapes(self.basenet)
        total = sum(int(np.prod(s)) for _, s in shapes)
        if self.svi_rng == "device" and torch.device(self.device).type == "cuda":
            if not seeds:
                return torch.randn(n_samples, total, device=self.device, dtype=torch.float32)
            eps = torch.empty(n_samples, total, device=self.device, dtype=torch.float32)
            gen = torch.Generator(device=self.device)
            for i in range(n_samples):
                gen.manual_seed(int(seeds[i]))
                torch.randn(total, generator=gen, device=self.device, dtype=torch.float32, out=eps[i])
            return eps
        eps = torch.empty(n_samples, total, dtype=torch.float32)
        for i in range(n_samples):
            if seeds:
                set_rng_seed(seeds[i])
            for _, shp in shapes:
                torch.randn(shp)
                torch.randn(shp)
            off = 0
            for _, shp in shapes:
                n = int(np.prod(shp))
                eps[i, off:off + n] = torch.randn(shp).reshape(-1)
                off += n
        return eps.to(self.device)

    def draw_posterior(self, n_samples, seeds=None):
        """n_samples weight draws as a StackedPosterior (model_bnn.py:124-130, :222-232)."""
        keys = list(self.basenet.state_dict().keys())
        loc = torch.cat([self.svi_loc[k].reshape(-1) for k in keys])
        scale = torch.cat([self.svi_scale[k].reshape(-1) for k in keys])
        eps = self._svi_eps(n_samples, seeds).contiguous()
        out = torch.empty_like(eps)
        _hip.HipKernels().svi_materialize(loc, scale, eps, out)
        stacked, off = {}, 0
        for k in keys:
            shp = tuple(self.svi_loc[k].shape)
            n = int(np.prod(shp))
            stacked[k] = out[:, off:off + n].reshape((n_samples,) + shp)
            off += n
        return self._make_posterior(stacked, self.device)

    # ------------------------------------------------------------------ svi: in-place redraw (fc / fc2 on the GPU)
    def _in_place(self):
        ok = (self.inference == "svi" and self.basenet.architecture in ("fc", "fc2", "conv") and self.svi_rng == "device"
              and torch.device(self.device).type == "cuda")
        if ok and self.basenet.architecture != "conv":
            # rbnn_svi_draw stages W2 [C, H] in LDS (160 KB: hidden <= 4096 at 10 classes); a wider net keeps the older path
            # (draw_posterior: rbnn_svi_materialize into a new stack), which has no such limit
            b = self.basenet
            ok = int(b.output_size) * max(32, int(b.hidden_size)) * 4 <= 160 * 1024
        return ok

    def _new_slot(self, n_samples):
        b = self.basenet
        if b.architecture == "conv":
            from .conv import ConvStackedPosterior, ConvSviGuide
            if self._guide is None:
                self._guide = ConvSviGuide(self.svi_loc, self.svi_scale, self.device)
            post = ConvStackedPosterior.for_guide(self._guide, b.activation, b.input_shape, b.output_size, b.hidden_size, n_samples)
        else:
            from .posterior import StackedPosterior, SviGuide
            if self._guide is None:
                self._guide = SviGuide(self.svi_loc, self.svi_scale, b.architecture, self.device)
            post = StackedPosterior.for_guide(self._guide, b.activation, b.input_shape, b.output_size, n_samples)
        eng = make_engine(post)
        if eng.precision == "triple":
            post.triple_images()                          # allocated once; every redraw writes them in the draw kernel itself
        elif eng.precision == "split":
            post.split_images()
        return post, eng

    def _fresh_key(self):
        """64 bits from torch's global CPU generator — the stream the reference's draws advance (model_bnn.py:230-232 under
        pyro.set_rng_seed): set_rng_seed(k) makes the following unseeded draws reproducible.  Host arithmetic only."""
        return int(torch.randint(-(2 ** 63), 2 ** 63 - 1, (1,), dtype=torch.int64).item())

    def redraw(self, n_samples):
        """Fresh weights for the `n_samples` samples of the resident SVI stack (what every un-seeded forward of the reference does,
        model_bnn.py:230-232): one kernel launch, nothing allocated, no device->host sync.  Returns the (unchanged) engine."""
        slot = self._slots.get(n_samples)
        if slot is None:
            if len(self._slots) >= 2:                         # e.g. an attack with S samples scored with S' defence samples
                self._slots.pop(next(iter(self._slots)))
            slot = self._slots[n_samples] = self._new_slot(n_samples)
        self._draws += 1
        # the key alone identifies the draw: reproducible under set_rng_seed.  lowdim engines (half-moons): the draw is left pending and generated
        # inside the next rbnn_lowdim_run launch (posterior.StackedPosterior.lazy_capable); anything else that reads the stack materialises it
        if getattr(slot[1], "precision", None) in ("lowdim", "triple") and hasattr(slot[0], "lazy_capable"):
            slot[0].redraw(self._fresh_key(), 0, lazy=True)
        else:
            slot[0].redraw(self._fresh_key(), 0)
        return slot[1]

    # ------------------------------------------------------------------ hot path handles
    def hot_path(self, n_samples, avg_posterior=False, seeds=None):
        """(engine, n_samples, seeds, logits) to run `n_samples` posterior samples through the kernels."""
        if seeds:
            if len(seeds) != n_samples:
                raise ValueError("Number of seeds should match number of samples.")     # model_bnn.py:200-202
        if self.inference == "hmc":
            return self._engine, n_samples, seeds, False
        if avg_posterior is True:                         # model_bnn.py:206-216: logits of the mean weights
            stacked = {k: v.unsqueeze(0) for k, v in self.svi_loc.items()}
            return make_engine(self._make_posterior(stacked, self.device)), 1, None, True
        # (identity, version) of every variational tensor: an in-place edit bumps _version, a REPLACED tensor (net.svi_loc[k] = new, version 0
        # again) changes data_ptr — either way the guide's bounds (hard bounds of the fp16 piece scaling), stacks and seeded draws are stale
        ver = tuple((t.data_ptr(), t._version) for t in list(self.svi_loc.values()) + list(self.svi_scale.values()))
        if ver != getattr(self, "_guide_ver", None):
            self._guide_ver, self._drawn, self._guide, self._slots = ver, None, None, {}
        if not seeds:                                     # the reference draws from the live RNG: fresh weights on every call
            if self._in_place():
                return self.redraw(n_samples), n_samples, None, False
            return make_engine(self.draw_posterior(n_samples, seeds)), n_samples, None, False
        # seeded draws are a pure function of (seeds, loc, scale): evaluate(), attack_evaluation() and the drivers call forward() batch
        # after batch with the same seeds — keep the last drawn posterior (weights, packed images, workspaces) instead of re-materialising
        # it per call.  set_variational_params() drops it, so a reloaded guide can never be served an older guide's draw.
        key = (int(n_samples), tuple(int(v) for v in seeds), self.svi_rng)
        if self._drawn is None or self._drawn[0] != key:
            if self._in_place():
                post, eng = self._new_slot(n_samples)
                keys = torch.tensor([int(v) for v in seeds], dtype=torch.int64).to(self.device)      # seed i -> Philox key i: the draw for a
                post.redraw(0, 0, sample_keys=keys)                                                  # seed does not depend on its position
                self._drawn = (key, eng)
            else:
                self._drawn = (key, make_engine(self.draw_posterior(n_samples, seeds)))
        return self._drawn[1], n_samples, None, False

    def forward(self, inputs, n_samples=10, avg_posterior=False, seeds=None):
        """model_bnn.py:198-258 -> mean probabilities [B, C] (raw logits if avg_posterior, :216)."""
        eng, S, sd, logits = self.hot_path(n_samples, avg_posterior, seeds)
        return eng.forward(inputs.to(self.device), S, seeds=sd, logits=logits)

    def train(self, *args, **kwargs):
        """model_bnn.py:350-365 (SVI, fc / fc2, on the GPU); train(mode) is nn.Module's pass-through (:333-334)."""
        if args and isinstance(args[0], bool) or "mode" in kwargs:
            return super().train(*args, **kwargs)
        return self._train_svi(*args, **kwargs)

    def _train_svi(self, train_loader, device, rel_path=TESTS, filename=None):
        """model_bnn.py:303-348 + :350-360: seed, epochs of SviTrainer steps, the per-epoch line, save().  The guide's parameters are
        initialised at the first step (after the loader's iterator has made its first batch: a shuffled loader draws its permutation seed
        from the CPU generator first, as the reference's does — RandomSampler's order of draws recalled, not checked) unless the net
        already holds some (load() or an earlier train(): pyro's param store persists), which are then trained further."""
        if self.inference == "hmc":
            raise NotImplementedError("train() runs SVI only: sample an HMC posterior with BNN.train_hmc(train_loader, device) (fc / fc2) or "
                                      "BNN.train_hmc_conv(train_loader, device) (conv, 1x28x28)")
        require_gpu_fc("SVI training", self.basenet.architecture)
        require_gpu_fc("SVI training", device=device)
        from .svi_train import SviTrainer
        b = self.basenet
        self._svi_epochs(train_loader, device, rel_path, filename, lambda loc, raw, key, B: SviTrainer(
            b.architecture, b.activation, b.input_shape, b.output_size, loc, raw, self.lr, device, key, batch_size=B))

    def train_conv(self, train_loader, device, rel_path=TESTS, filename=None):
        """_train_svi for the conv architecture of the 1x28x28 geometry (conv_svi_train.ConvSviTrainer, csrc/rbnn_conv_train.hip): the same
        seeding, initialisation at the first batch, key, epoch lines, training_history, set_variational_params and save().  Every refusal
        comes before any state is changed, a generator touched or the library loaded."""
        if self.inference == "hmc":
            raise NotImplementedError("train_conv() runs SVI only: an HMC posterior is sampled with BNN.train_hmc(train_loader, device) for fc / "
                                      "fc2 and with BNN.train_hmc_conv(train_loader, device) for a conv net of the 1x28x28 geometry")
        if self.basenet.architecture != "conv":
            raise ValueError(f"train_conv trains the conv architecture; a {self.basenet.architecture!r} net trains through train")
        from .conv_train import check_conv_trainable
        check_conv_trainable(self.basenet.input_shape, device)
        from .conv_svi_train import ConvSviTrainer
        b = self.basenet
        self._svi_epochs(train_loader, device, rel_path, filename, lambda loc, raw, key, B: ConvSviTrainer(
            b.activation, b.input_shape, b.output_size, loc, raw, self.lr, device, key, batch_size=B))

    def _svi_epochs(self, train_loader, device, rel_path, filename, make_trainer):
        """The epoch loop of _train_svi and train_conv behind their guards; make_trainer(loc, raw, key, batch_size) constructs the trainer at
        the first batch."""
        from .svi_train import draw_key, initial_params
        self.device = device
        self.basenet.device = device
        random.seed(0)
        set_rng_seed(0)
        print("\n == SVI training ==")
        b, trainer = self.basenet, None
        loss_list, accuracy_list = [], []
        n = len(train_loader.dataset)
        for epoch in range(self.epochs):
            for x_batch, y_batch in train_loader:
                if trainer is None:
                    if self.svi_loc is None:
                        loc, raw = initial_params(state_shapes(b))
                    else:
                        loc, raw = self.svi_loc, self.svi_scale
                    trainer = make_trainer(loc, raw, draw_key(), int(x_batch.shape[0]))
                trainer.step(x_batch.to(device), y_batch.to(device).argmax(-1))
            loss, correct = trainer.epoch_totals() if trainer is not None else (0.0, 0.0)
            if trainer is not None:
                trainer.begin_epoch()
            total_loss, accuracy = loss / n, 100 * correct / n
            print(f"\n[Epoch {epoch + 1}]\t loss: {total_loss:.2f} \t accuracy: {accuracy:.2f}", end="\t")
            loss_list.append(loss)                        # the reference's loss_list holds the epoch's sum (model_bnn.py:342)
            accuracy_list.append(accuracy)
        self.training_history = {"loss": loss_list, "accuracy": accuracy_list}
        if trainer is not None:
            loc, raw = trainer.params()
            self.set_variational_params(loc, raw, device)   # drops the guide, slots and seeded draws of the previous parameters
        self.save(rel_path=rel_path, filename=filename)

    def train_hmc(self, train_loader, device, rel_path=TESTS, filename=None, num_chains=1):
        """The hmc half of model_bnn.py:350-365 + _train_hmc (:260-301), fc / fc2 on the GPU: seed, the chain (hmc.HmcSampler with self.step_size,
        self.num_steps, self.warmup), the resampling of get_samples(n_samples), save().

        The reference calls mcmc.run once per batch; every call is a FRESH chain (warmup + batch_samples = int(n_samples / num_batches) + 1 samples)
        that replaces the samples of the one before, and get_samples(n_samples) then draws n_samples indices with replacement from the last run.
        The earlier runs reach the result only through pyro's RNG stream, which is unpinned.  So the loader is iterated (its shuffle draws
        happen), the chain runs on the LAST batch only, and the stack is resampled with torch.randint(0, batch_samples, (n_samples,)) from the
        CPU generator.  A dataset smaller than one batch (num_batches = 0, where the reference divides by zero) counts as one batch.
        self.hmc_history keeps the chain's logs.

        num_chains = K > 1: K chains in lockstep on the GPU (hmc.LockstepHmc; every launch covers all chains).  Chain 0 takes its start
        position and key exactly where the single chain does (it IS the num_chains = 1 chain, bit for bit); chains 1..K-1 draw theirs
        afterwards.  All run batch_samples samples on the last batch; the pooled stack is chain-major [K * batch_samples, ...]
        (hmc_history["stack"]) and is resampled with torch.randint(0, K * batch_samples, (n_samples,)).  hmc_history's logs are chain 0's,
        "chains" holds every chain's, "r_hat_U" the split-R-hat of the chains' potential over the sampling phase (hmc.split_r_hat)."""
        if self.inference != "hmc":
            raise ValueError(f"train_hmc() samples an HMC posterior; this net's inference is {self.inference!r} (use train())")
        if int(num_chains) < 1:
            raise ValueError(f"train_hmc() needs num_chains >= 1, not {num_chains}")
        require_gpu_fc("HMC", self.basenet.architecture)
        require_gpu_fc("HMC", device=device)
        from .hmc import HmcSampler, LockstepHmc
        b, K = self.basenet, int(num_chains)
        net = (b.architecture, b.activation, b.input_shape, b.output_size)
        self._sample_hmc(train_loader, device, rel_path, filename, K, lambda B: K,
                         lambda q0, key, B: HmcSampler(*net, q0, self.step_size, self.num_steps, device, key, batch_size=B),
                         lambda q0s, keys, B: LockstepHmc(*net, q0s, self.step_size, self.num_steps, device, keys, batch_size=B))

    def train_hmc_conv(self, train_loader, device, rel_path=TESTS, filename=None, num_chains=1, group=None):
        """train_hmc for the conv architecture of the 1x28x28 geometry (conv_hmc.ConvHmcSampler: the chain's kernels of csrc/rbnn_hmc.hip
        around the conv training forward and weight gradients of csrc/rbnn_conv_train.hip): the same prologue, the chain on the last batch,
        the resampling with torch.randint(0, batch_samples, (n_samples,)), set_posterior_samples, hmc_history and save().

        num_chains = K > 1: K chains with every launch covering all of them (conv_hmc.ConvLockstepHmc), exactly as train_hmc runs K fc
        chains.  Chain 0 takes its start position and key where the single chain does (it IS the num_chains = 1 chain, bit for bit); chains
        1..K-1 draw theirs afterwards, all before any chain runs.  All run batch_samples samples on the last batch; the pooled stack is
        chain-major [K * batch_samples, ...] (hmc_history["stack"]) and is resampled with torch.randint(0, K * batch_samples, (n_samples,)).
        hmc_history's logs are chain 0's, "chains" holds every chain's, "r_hat_U" the split-R-hat of the chains' potential over the sampling
        phase.  The chains run in consecutive groups of `group` (None: as many as fit the RBNN_CONV_WS_GB budget,
        conv_hmc.conv_hmc_chains_group; else an int in [1, K]), one group after the other; the chains are independent and every host draw is
        made before the first group, so the grouping changes no bit.
        Every refusal comes before any state is changed, a generator touched or the library loaded."""
        if self.inference != "hmc":
            raise ValueError(f"train_hmc_conv() samples an HMC posterior; this net's inference is {self.inference!r} (use train_conv())")
        if self.basenet.architecture != "conv":
            raise ValueError(f"train_hmc_conv samples the conv architecture; a {self.basenet.architecture!r} net samples through train_hmc")
        K = int(num_chains)
        if K < 1:
            raise ValueError(f"train_hmc_conv() needs num_chains >= 1, not {num_chains}")
        if group is not None and not 1 <= int(group) <= K:
            raise ValueError(f"train_hmc_conv() runs its chains in groups of 1 .. num_chains = {K}, not group = {group}")
        from .conv_train import check_conv_trainable
        check_conv_trainable(self.basenet.input_shape, device)
        from .conv_hmc import ConvHmcSampler, ConvLockstepHmc, conv_hmc_chains_group
        b = self.basenet
        net = (b.activation, b.input_shape, b.output_size)
        self._sample_hmc(train_loader, device, rel_path, filename, K,
                         lambda B: conv_hmc_chains_group(b.activation, b.hidden_size, b.output_size, K, B) if group is None else int(group),
                         lambda q0, key, B: ConvHmcSampler(*net, q0, self.step_size, self.num_steps, device, key, batch_size=B),
                         lambda q0s, keys, B: ConvLockstepHmc(*net, q0s, self.step_size, self.num_steps, device, keys, batch_size=B))

    def _sample_hmc(self, train_loader, device, rel_path, filename, K, group_of, one_chain, lockstep_chains):
        """train_hmc and train_hmc_conv behind their guards: the prologue, the draws of chains 1..K-1 (every host draw before the first chain
        runs), the chains on the last batch — one_chain(q0, key, B) for K = 1, else lockstep_chains(q0s, keys, B) for consecutive groups of
        group_of(B) chains (fc / fc2: one group of K) —, the chain-major stack, the resampling, hmc_history, set_posterior_samples and save()."""
        x_batch, y_batch, batch_samples, q0, key = self._hmc_prologue(train_loader, device)
        x, labels, B = x_batch.to(device), y_batch.to(device).argmax(-1), int(x_batch.shape[0])
        if K == 1:
            sampler = one_chain(q0, key, B)
            stack = sampler.run(x, labels, batch_samples, self.warmup)
            chains = [lockstep_history(sampler)]
        else:
            from .hmc import initial_position
            from .svi_train import draw_key
            q0s, keys = [q0], [key]
            for _ in range(1, K):
                q0s.append(initial_position(state_shapes(self.basenet)))
                keys.append(draw_key())
            group = group_of(B)
            stacks, chains, logs = [], [], []
            for a in range(0, K, group):
                sampler = lockstep_chains(q0s[a:a + group], keys[a:a + group], B)
                stacks += [{k: v.clone() for k, v in s.items()} for s in sampler.run(x, labels, batch_samples, self.warmup)]
                chains += [lockstep_history(sampler, k) for k in range(sampler.K)]
                logs.append(sampler.log)
                del sampler                                                               # the next group's workspaces take its place
            stack = {k: torch.cat([s[k] for s in stacks], 0) for k in stacks[0]}          # chain-major [K * batch_samples, ...]
        idx = torch.randint(0, K * batch_samples, (self.n_samples,)).to(device)
        self.hmc_history = {**chains[0], "resampled": idx.cpu()}
        if K > 1:
            self.hmc_history.update({"stack": stack, "chains": chains, "r_hat_U": lockstep_r_hat(torch.cat(logs, 0), self.warmup)})
        self.set_posterior_samples({k: v.index_select(0, idx).contiguous() for k, v in stack.items()}, device)
        self.save(rel_path=rel_path, filename=filename)

    def _hmc_prologue(self, train_loader, device):
        """train_hmc up to the chain: the seeding, the pass over the loader, the start position and the key, in the order their draws leave
        the CPU generator.  -> (x_batch, y_batch of the LAST batch, batch_samples, q0, key)."""
        from .hmc import initial_position
        from .svi_train import draw_key
        self.device = device
        self.basenet.device = device
        random.seed(0)
        set_rng_seed(0)
        print("\n == HMC training ==")
        num_batches = int(len(train_loader.dataset) / train_loader.batch_size)
        batch_samples = int(self.n_samples / max(1, num_batches)) + 1
        print("\nn_batches=", num_batches, "\tbatch_samples =", batch_samples)
        x_batch = y_batch = None
        for x_batch, y_batch in train_loader:            # every batch but the last reaches the result through the RNG stream only
            pass
        if x_batch is None:
            raise ValueError("train_hmc() needs a loader with at least one batch")
        q0 = initial_position(state_shapes(self.basenet))
        return x_batch, y_batch, batch_samples, q0, draw_key()

    def evaluate(self, test_loader, device, n_samples=10, seeds_list=None):
        """model_bnn.py:367-391"""
        random.seed(0)
        set_rng_seed(0)
        bnn_seeds = list(range(n_samples)) if seeds_list is None else seeds_list
        correct = 0.0
        for x_batch, y_batch in test_loader:
            outputs = self.forward(x_batch.to(device), n_samples=n_samples, seeds=bnn_seeds)
            correct += float((outputs.argmax(-1) == y_batch.to(device).argmax(-1)).sum())
        accuracy = 100 * correct / len(test_loader.dataset)
        print("Accuracy: %.2f%%" % (accuracy))
        return accuracy
