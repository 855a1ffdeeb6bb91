"""Shared builders of the EdgeConv tests: the layer restated from its formula in numpy (nothing from models.py), a seeded model, and the
call of the stage entry ``gnnb_aggregate_edgeconv`` (it has no Python method: ``CompiledModel``'s stage methods are a closed list)."""
import numpy as np
import torch

import gnnbuilder_amd as gnnb
from gnnbuilder_amd import runtime
from helpers import ACTS


def _max(n, coo, pre, w2, b2):
    """``max_{j -> i} W2 relu(pre_ij) + b2`` from -inf over the edges ``(j, i)``, rows of ``coo``; a row without in-edges is 0."""
    out = np.full((n, len(w2)), -np.inf, pre.dtype)
    np.maximum.at(out, coo[:, 1], np.maximum(pre, 0) @ w2.T + b2)
    return np.where(np.isneginf(out), pre.dtype.type(0), out)


def layer_ref(x, coo, w1, b1, w2, b2, dtype=np.float64):
    """The layer's formula: ``pre_ij = W1 [x_i | x_j - x_i] + b1``."""
    x, w1, b1, w2, b2 = (np.asarray(a, dtype) for a in (x, w1, b1, w2, b2))
    return _max(len(x), coo, np.concatenate([x[coo[:, 1]], x[coo[:, 0]] - x[coo[:, 1]]], 1) @ w1.T + b1, w2, b2)


def stage_ref(ab, coo, w2, b2, dtype=np.float64):
    """The stage entry's formula on the GEMM result ``[a | b]``: ``pre_ij = a_i + b_j``."""
    ab, w2, b2 = (np.asarray(a, dtype) for a in (ab, w2, b2))
    h = w2.shape[1]
    return _max(len(ab), coo, ab[coo[:, 1], :h] + ab[coo[:, 0], h:2 * h], w2, b2)


def operands(num_nodes, w, seed):
    """ab [N, 2 w], w2 [w, w], b2 [w]: uniform, the weights scaled by their fan-in, b2 offset to -0.5 so that many maxima are negative."""
    rng = np.random.default_rng(seed)
    u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)  # noqa: E731
    return u(num_nodes, 2 * w), u(w, w) / np.float32(w ** 0.5), u(w) * np.float32(0.25) - np.float32(0.5)


def edgeconv(cm, ab, w2, b2, out):
    """``gnnb_aggregate_edgeconv`` (no skip, no activation) on ``cm``'s prepared batch; contiguous device tensors, ``ab`` [N, 2 h]."""
    w, h = int(w2.shape[0]), int(w2.shape[1])
    p = lambda a: a.data_ptr() if a.numel() else None  # noqa: E731
    runtime._check(cm.lib.gnnb_aggregate_edgeconv(cm._ws, p(ab), 2 * h, h, p(w2), h, p(b2), w, None, runtime.ACT["none"], p(out), w, None))
    return out


def make_model(in_dim=7, hidden=32, layers=3, seed=0, act="relu", pools=("add", "mean", "max")):
    """Skip on; nn.2's bias seeded around -0.5, so that a max seeded with 0 or a bias on an empty row shows."""
    torch.manual_seed(seed)
    model = gnnb.GNNModel(in_dim, None, hidden, layers, hidden, gnnb.EdgeConv_GNNB, ACTS[act], True, gnnb.GlobalPooling(list(pools)),
                          gnnb.MLP(len(pools) * hidden, 19, 64, 1), None, gnn_aggr="max")
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("nn.2.bias"):
                p.uniform_(-0.75, -0.25)
    return model.eval()
