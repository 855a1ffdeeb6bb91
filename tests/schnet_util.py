"""Shared builders of the SchNet tests: the layer restated from its formula in numpy (nothing from models.py), a seeded model, and the
few-line call of the stage entry ``gnnb_aggregate_cfconv`` (it has no Python method: ``CompiledModel``'s stage methods are a closed list)."""
import copy

import numpy as np
import torch

import gnnbuilder_amd as gnnb
import ref64 as R
from gnnbuilder_amd import runtime
from helpers import ACTS, batch_vector

LN2 = np.log(2.0)


def ssp(v):
    return np.logaddexp(v, v.dtype.type(0)) - v.dtype.type(LN2)


def filters(dist, w1, b1, w2, b2, cutoff, dtype=np.float64):
    """``w_ij = (W2 ssp(W1 rbf + b1) + b2) C(d_ij)`` per edge, [E, F]; ``G = 1``: the one centre is 0, ``coeff = -0.5 / cutoff^2``."""
    d, G = np.asarray(dist, dtype).reshape(-1), np.asarray(w1).shape[1]
    mu = np.linspace(0.0, cutoff, G).astype(dtype)
    coeff = dtype(-0.5 / float(mu[1] - mu[0]) ** 2 if G > 1 else -0.5 / cutoff ** 2)
    rbf = np.exp(coeff * (d[:, None] - mu) ** 2)
    h = ssp(rbf @ np.asarray(w1, dtype).T + np.asarray(b1, dtype))
    c = dtype(0.5) * (np.cos(d * dtype(np.pi / cutoff)) + dtype(1))
    return ((h @ np.asarray(w2, dtype).T + np.asarray(b2, dtype)) * c[:, None]).astype(dtype)


def aggregate_ref(x1, coo, dist, w1, b1, w2, b2, cutoff, dtype=np.float64):
    """``sum_{j -> i} x1_j * w_ij``, edges in COO order (``np.add.at`` is sequential); a row without in-edges is 0."""
    x1 = np.asarray(x1, dtype)
    out = np.zeros_like(x1)
    if len(coo):
        np.add.at(out, coo[:, 1], x1[coo[:, 0]] * filters(dist, w1, b1, w2, b2, cutoff, dtype))
    return out


def operands(num_nodes, num_edges, w, g, cutoff, seed):
    """x1, dist, w1, b1, w2, b2: distances uniform in [0.3, 1.1 cutoff], the others in [-1, 1], weights scaled by their fan-in."""
    rng = np.random.default_rng(seed)
    u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)  # noqa: E731
    return (u(num_nodes, w), rng.uniform(0.3, 1.1 * cutoff, num_edges).astype(np.float32), u(w, g) / np.float32(g), u(w), u(w, w) / np.float32(w),
            u(w))


def cfconv(cm, x1, dist, w1, b1, w2, b2, cutoff, out=None):
    """``gnnb_aggregate_cfconv`` on ``cm``'s prepared batch; device tensors, ``x1`` / ``out`` [N, w] contiguous."""
    w, g = int(w1.shape[0]), int(w1.shape[1])
    out = torch.empty_like(x1) if out is None else out
    p = lambda a: a.data_ptr() if a.numel() else None  # noqa: E731
    runtime._check(cm.lib.gnnb_aggregate_cfconv(cm._ws, p(x1), w, w, p(dist), p(w1), g, p(b1), p(w2), w, p(b2), g, float(cutoff), p(out), w,
                                                None))
    return out


def make_model(in_dim=9, hidden=12, layers=3, gaussians=50, cutoff=5.0, act="relu", pools=("add", "mean", "max"), seed=0):
    """Skip on (SchNet's residual); every bias seeded non-zero, so that a bias in the wrong place shows."""
    torch.manual_seed(seed)
    model = gnnb.GNNModel(in_dim, 1, hidden, layers, hidden, gnnb.SchNetConv_GNNB, ACTS[act], True, gnnb.GlobalPooling(list(pools)),
                          gnnb.MLP(len(pools) * hidden, 19, 64, 1), None, gnn_gaussians=gaussians, gnn_cutoff=cutoff)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("bias"):
                p.uniform_(-0.5, 0.5)
    return model.eval()


def run(model, batch, x, dist):
    """The whole model as it stands (its own dtype): numpy [B, out]."""
    dtype = next(model.parameters()).dtype
    with torch.no_grad():
        return model(R._t(x, dtype), R.edge_index(batch.coo), torch.from_numpy(batch_vector(batch)), R._t(dist, dtype)).numpy()


def forward64(model, batch, x, dist):
    return run(copy.deepcopy(model).double(), batch, x, dist)
