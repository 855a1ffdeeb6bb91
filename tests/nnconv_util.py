"""Shared builders of the NNConv tests: the float64 restatement through the explicit ``[E, in, out]`` tensor (numpy, nothing taken
from models.py), the coefficient aggregate ``A`` by its definition, the weight fold, a seeded ``GNNModel`` and its ``.double()`` run."""
import copy

import numpy as np
import torch

import gnnbuilder_amd as gnnb
import ref64 as R
from helpers import ACTS, batch_vector


def coefs(e, w1, b1, dtype):
    """The per-edge coefficient vectors ``[E, K' + 1]``: ``[e ; 1]`` or ``[relu(w1 e + b1) ; 1]``."""
    e = np.asarray(e, dtype)
    c = e if w1 is None else np.maximum(e @ np.asarray(w1, dtype).T + np.asarray(b1, dtype), 0)
    return np.concatenate([c, np.ones((len(e), 1), dtype)], 1)


def aggregate_ref(x, coo, e, w1=None, b1=None, aggr="add", dtype=np.float64):
    """``A[i, k in + col] = aggr_{j -> i} c_ijk x_j[col]`` -> [N, (K' + 1) in], edges added in COO order per destination."""
    x, c = np.asarray(x, dtype), coefs(e, w1, b1, dtype)
    a = np.zeros((len(x), c.shape[1], x.shape[1]), dtype)
    np.add.at(a, coo[:, 1], c[:, :, None] * x[coo[:, 0]][:, None, :])
    if aggr == "mean":
        a /= np.maximum(np.bincount(coo[:, 1], minlength=len(x)), 1).astype(dtype)[:, None, None]
    return a.reshape(len(x), c.shape[1] * x.shape[1])


def aggregate_ref_blocks(x, coo, e, w1=None, b1=None, aggr="add", dtype=np.float64):
    """``aggregate_ref`` one coefficient block at a time, for batches of tens of thousands of nodes: the ``[E, K' + 1, in]``
    tensor is never built.  The edges are put in destination order once (a stable sort: COO order per destination stays) and the
    rows in the order of falling in-degree; round ``t`` then adds the ``t``-th message of every row that has one, which is a
    leading slice of the rows.  Every row starts from 0 and takes its messages in COO order, each product rounded before it is
    added: the bits of ``aggregate_ref`` in either dtype (tests/test_nnconv_model_torch.py)."""
    x, c = np.asarray(x, dtype), coefs(e, w1, b1, dtype)
    n, w = x.shape
    deg = np.bincount(coo[:, 1], minlength=n)[:n]
    order = np.argsort(coo[:, 1], kind="stable")
    src, c = coo[order, 0], c[order]
    rows = np.argsort(-deg, kind="stable")  # the rows by falling in-degree
    start, left = (np.cumsum(deg) - deg)[rows], deg[rows]
    a = np.zeros((c.shape[1], n, w), dtype)  # block-major, rows in that order, until the end
    for t in range(int(deg.max()) if n else 0):
        cnt = int(np.searchsorted(-left, -t, "left"))  # the rows with more than t in-edges
        at = start[:cnt] + t
        xe = x[src[at]]
        if cnt * w <= 1 << 16:  # (the long tail of a few hubs: all blocks in one statement)
            a[:, :cnt] += c[at].T[:, :, None] * xe[None]
            continue
        for k in range(c.shape[1]):
            a[k, :cnt] += c[at, k:k + 1] * xe
    if aggr == "mean":
        a /= np.maximum(left, 1).astype(dtype)[None, :, None]
    out = np.empty((n, c.shape[1], w), dtype)
    out[rows] = a.transpose(1, 0, 2)
    return out.reshape(n, c.shape[1] * w)


def theta_sum(x, coo, e, w2, b2, fo, w1=None, b1=None, dtype=np.float64):
    """``sum_{j -> i} x_j Theta(e_ij)`` through the explicit ``[E, in, out]`` tensor, ``Theta = nn(e).view(in, out)``."""
    x = np.asarray(x, dtype)
    theta = (coefs(e, w1, b1, dtype)[:, :-1] @ np.asarray(w2, dtype).T + np.asarray(b2, dtype)).reshape(len(coo), x.shape[1], fo)
    out = np.zeros((len(x), fo), dtype)
    np.add.at(out, coo[:, 1], np.einsum("ei,eio->eo", x[coo[:, 0]], theta))
    return out


def fold(w2, b2, fi, fo):
    """``W_fold[k in + col, o] = W2[col out + o, k]``, block ``K'`` from ``b2``: [(K' + 1) in, out]."""
    w = np.concatenate([np.asarray(w2), np.asarray(b2)[:, None]], 1).reshape(fi, fo, -1)  # [col, o, k]
    return np.ascontiguousarray(w.transpose(2, 0, 1)).reshape(-1, fo)


def make_model(in_dim=9, hidden=12, layers=3, edge_dim=4, edge_hidden=0, aggr="add", act="relu", skip=True, pools=("add", "mean", "max"), seed=0,
               out_dim=None):
    torch.manual_seed(seed)
    out_dim = hidden if out_dim is None else out_dim
    model = gnnb.GNNModel(in_dim, edge_dim, hidden, layers, out_dim, gnnb.NNConv_GNNB, ACTS[act], skip, gnnb.GlobalPooling(list(pools)),
                          gnnb.MLP(len(pools) * out_dim, 19, 64, 1), None, gnn_edge_hidden=edge_hidden, gnn_aggr=aggr)
    with torch.no_grad():  # (PyG initialises the bias with zeros: a seeded one, so that a bias in the wrong place shows)
        for conv in model.gnn_convs:
            conv.conv.bias.uniform_(-0.5, 0.5)
    return model.eval()


def run(model, batch, x, edge_attr):
    """The whole model as it stands (its own dtype): numpy [B, out]."""
    dtype = next(model.parameters()).dtype
    with torch.no_grad():
        return model(R._t(x, dtype), R.edge_index(batch.coo), torch.from_numpy(batch_vector(batch)), R._t(edge_attr, dtype)).numpy()


def forward64(model, batch, x, edge_attr):
    return run(copy.deepcopy(model).double(), batch, x, edge_attr)


def forward_by_graphs(model, batch, x, edge_attr, graphs=32, double=True):
    """``forward64`` (``double=False``: the model as it stands) of a batch whose ``[E, in, out]`` tensor does not fit: the same
    definition on ``graphs`` graphs at a time (``helpers.sub_batch``), the rows put together.  No sum of the model crosses a
    graph and the edges of a graph keep their order, so this is the one-piece run up to the blocking torch's GEMMs choose for
    another row count: a few ulps of the output's scale (tests/test_nnconv_model_torch.py)."""
    import dataclasses

    import gine_util
    from helpers import sub_batch, sub_edge_rows
    m = copy.deepcopy(model).double() if double else model
    whole, outs = dataclasses.replace(batch, x=np.ascontiguousarray(x)), []
    for g0 in range(0, batch.num_graphs, graphs):
        gids = np.arange(g0, min(g0 + graphs, batch.num_graphs))
        sub, _ = sub_batch(whole, gids)
        outs.append(gine_util.run(m, sub, sub.x, edge_attr[sub_edge_rows(batch, gids)]))
    return np.concatenate(outs)
