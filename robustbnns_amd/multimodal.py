"""Posterior samples in weight space — the numerical core of the reference's test_multimodal.py.

The script samples HMC posteriors of fc2-512 nets on 1 000, 10 000 and 60 000 training points, flattens every posterior sample into one vector
of P = 669 706 weights (test_multimodal.py:87-98), projects the 50 samples of each posterior and 1 000 draws of the N(0, I) prior onto two
principal components (:100-161) and draws one density per set (:166-194).  `posterior_weights` is the flattening, `build_pca_df` the
projections with the script's DataFrame (columns n_samples, n_training_points, x, y; the prior's rows first), both on the GPU through
weight_pca.WeightPCA; the prior's rows come from weight_pca.PriorRows (a Philox key instead of 1000 calls of Normal.rsample: seed-for-seed
parity with torch's generator is unpinned, like the SVI draw) and its 1000 x P matrix is never stored.  `chains_pca` is the same picture for
the chains of one train_hmc(num_chains=K) run: where the chains sit in weight space, beside hmc_history["r_hat_U"].
Plotting (:166-194) needs seaborn and is out of scope.
"""
import pandas
import torch

from .weight_pca import MatrixRows, PriorRows, WeightPCA

COLUMNS = ["n_samples", "n_training_points", "x", "y"]
PRIOR_KEY = 0x6D756C74696D6F64          # the default Philox key of the prior's rows


def _flatten(stack, keys):
    """dict key -> [S, ...] => fp32 [S, P], the tensors of `keys` side by side."""
    return torch.cat([stack[k].reshape(stack[k].shape[0], -1).to(torch.float32) for k in keys], 1).contiguous()


def posterior_weights(net):
    """fp32 [S, P] on the GPU: sample s of net.posterior flattened in parameters() order — weight, bias per layer, the order of the
    state_dict (test_multimodal.py:87-98).  fc, fc2 and conv posteriors."""
    if getattr(net, "posterior", None) is None:
        raise ValueError("posterior_weights() needs a net with stored posterior samples (an HMC posterior: load() or train_hmc())")
    post = net.posterior
    keys = [k for k, _ in net.basenet.named_parameters()]
    rows = [torch.cat([sd[k].reshape(-1) for k in keys]) for sd in (post.state_dict(s) for s in range(post.S))]
    return torch.stack(rows).to(post.device, torch.float32).contiguous()


def _rows(n_samples, n_training_points, xy):
    return [{"n_samples": n_samples, "n_training_points": n_training_points, "x": float(x), "y": float(y)} for x, y in xy.tolist()]


def build_pca_df(nets, n_samples, same_pca=False, key=PRIOR_KEY, n_prior=1000):
    """test_multimodal.py:100-161.  nets: an ordered mapping n_training_points -> BNN with stored posterior samples, of which the first
    n_samples are taken.  same_pca=False: every set, the prior included, is fitted on itself (:122-124, :155-157); same_pca=True: one fit on
    the concatenation of all posterior sets, the prior and each set are transformed (:102-107, :120-121, :152-153).
    -> DataFrame n_samples, n_training_points, x, y: the prior's n_prior rows (n_training_points = 0) first, then each net's in order."""
    sets = {n_inputs: posterior_weights(net)[:int(n_samples)] for n_inputs, net in nets.items()}
    if not sets:
        raise ValueError("build_pca_df() needs at least one net")
    first = next(iter(sets.values()))
    device, P = first.device, int(first.shape[1])
    if any(int(w.shape[1]) != P for w in sets.values()):
        raise ValueError("build_pca_df() projects nets of one shape: their weight counts differ")
    new = lambda: WeightPCA(2, device=device)
    prior = PriorRows(key, n_prior, P, device=device)
    if same_pca:
        pca = new().fit(MatrixRows(torch.cat(list(sets.values()))))
        project = pca.transform
    else:
        project = lambda rows: new().fit_transform(rows)
    out = _rows(int(n_prior), 0, project(prior))
    for n_inputs, w in sets.items():
        out += _rows(int(n_samples), n_inputs, project(MatrixRows(w)))
    return pandas.DataFrame(out, columns=COLUMNS)


def chains_pca(net):
    """One fit on the pooled chains of a train_hmc(num_chains=K) / train_hmc_conv(num_chains=K) run — hmc_history["stack"], chain-major
    [K * draws, ...] — -> DataFrame chain, draw, x, y (row c * draws + d is draw d of chain c)."""
    hist = getattr(net, "hmc_history", None) or {}
    if "stack" not in hist:
        raise ValueError("chains_pca() needs the pooled chains of a train_hmc(num_chains=K) or train_hmc_conv(num_chains=K) run with K > 1: "
                         "this net's hmc_history has no \"stack\"")
    stack = hist["stack"]
    K = len(hist["chains"])
    W = _flatten(stack, [k for k, _ in net.basenet.named_parameters()])
    if W.shape[0] % K:
        raise ValueError(f"the stack holds {W.shape[0]} draws, not a multiple of its {K} chains")
    draws = W.shape[0] // K
    xy = WeightPCA(2, device=W.device).fit_transform(MatrixRows(W)).tolist()
    return pandas.DataFrame([{"chain": i // draws, "draw": i % draws, "x": x, "y": y} for i, (x, y) in enumerate(xy)],
                            columns=["chain", "draw", "x", "y"])
