"""Shared builders of the GENConv tests: the aggregate restated from its formula in numpy (nothing from models.py), a seeded model."""
import copy

import numpy as np
import torch

import gnnbuilder_amd as gnnb
import ref64 as R
from helpers import ACTS, batch_vector

EPS = 1e-7


def messages(s, coo, e=None, we=None, be=None, dtype=np.float64):
    """``m_ij = relu(s_j + W_e e_ij + b_e) + eps`` per edge, [E, width] (``e`` None: no edge term)."""
    m = np.asarray(s, dtype)[coo[:, 0]]
    if e is not None:
        m = m + (np.asarray(e, dtype) @ np.asarray(we, dtype).T + np.asarray(be, dtype))
    return np.maximum(m, dtype(0)) + dtype(EPS)


def aggregate_ref(s, coo, r=None, e=None, we=None, be=None, t=1.0, dtype=np.float64):
    """``sum_j softmax_j(t m_ij)[c] m_ij[c] + r_i[c]``, two passes: the segment max by ``np.maximum.at``, then both sums by
    ``np.add.at``, edges in COO order; a row without in-edges is ``r_i`` (0 with ``r`` None)."""
    m = messages(s, coo, e, we, be, dtype)
    n, w = len(s), m.shape[1]
    z = dtype(t) * m
    zmax = np.full((n, w), -np.inf, dtype)
    np.maximum.at(zmax, coo[:, 1], z)
    wgt = np.exp(z - zmax[coo[:, 1]])
    den, num = np.zeros((n, w), dtype), np.zeros((n, w), dtype)
    np.add.at(den, coo[:, 1], wgt)
    np.add.at(num, coo[:, 1], wgt * m)
    agg = np.where(den > 0, num / np.where(den > 0, den, dtype(1)), dtype(0)).astype(dtype)
    return agg if r is None else agg + np.asarray(r, dtype)


def make_model(in_dim=9, hidden=12, layers=3, edge_dim=4, t=1.0, act="relu", skip=True, pools=("add", "mean", "max"), seed=0, out_dim=None):
    """``edge_dim = 0``: ``GENConv_GNNB``.  The layers' temperatures are spread round ``t`` and every bias is seeded non-zero, so that
    a temperature or a bias in the wrong place shows."""
    torch.manual_seed(seed)
    out_dim = hidden if out_dim is None else out_dim
    conv = gnnb.GENEConv_GNNB if edge_dim else gnnb.GENConv_GNNB
    model = gnnb.GNNModel(in_dim, edge_dim or None, hidden, layers, out_dim, conv, ACTS[act], skip, gnnb.GlobalPooling(list(pools)),
                          gnnb.MLP(len(pools) * out_dim, 19, 64, 1), None, gnn_softmax_t=t)
    with torch.no_grad():
        for l, c in enumerate(model.gnn_convs):
            c.conv.t.fill_(t * (1.0 - 0.125 * l))
            for name, p in c.conv.named_parameters():
                if name.endswith("bias"):
                    p.uniform_(-0.5, 0.5)
    return model.eval()


def run(model, batch, x, edge_attr=None):
    """The whole model as it stands (its own dtype): numpy [B, out]."""
    dtype = next(model.parameters()).dtype
    with torch.no_grad():
        return model(R._t(x, dtype), R.edge_index(batch.coo), torch.from_numpy(batch_vector(batch)),
                     None if edge_attr is None else R._t(edge_attr, dtype)).numpy()


def forward64(model, batch, x, edge_attr=None):
    return run(copy.deepcopy(model).double(), batch, x, edge_attr)
