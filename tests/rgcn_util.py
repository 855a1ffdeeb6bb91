"""Shared builders of the RGCNConv tests: a seeded ``GNNModel`` of ``RGCNConv_GNNB`` layers, seeded edge types, the float64
restatement of one layer behind its GEMM (``rgcn_ref``: numpy, nothing taken from models.py), the slot records as numpy gives
them, and the whole model on its own ``.double()`` copy."""
import copy

import numpy as np
import torch

import gnnbuilder_amd as gnnb
import ref64 as R
from helpers import ACTS, batch_vector

FAULTS = ("sum_not_mean", "mean_over_all", "block_shift", "bias_per_edge", "types_in_input_order")
RELATIONS = (1, 3, 8)
UNUSED_AT_8 = 5  # the relation no edge has at R = 8


def make_rgcn_model(in_dim=9, hidden=32, layers=3, out_dim=None, relations=4, act="relu", skip=True, pools=("add", "mean", "max"),
                    mlp_hidden=64, mlp_layers=2, task_out=19, out_act=None, seed=0):
    torch.manual_seed(seed)
    out_dim = hidden if out_dim is None else out_dim
    model = gnnb.GNNModel(in_dim, None, hidden, layers, out_dim, gnnb.RGCNConv_GNNB, ACTS[act], skip,
                          gnnb.GlobalPooling(list(pools)), gnnb.MLP(len(pools) * out_dim, task_out, mlp_hidden, mlp_layers), out_act,
                          gnn_relations=relations)
    # (PyG initialises the bias with zeros: a seeded one, so that a bias in the wrong place shows)
    with torch.no_grad():
        for conv in model.gnn_convs:
            conv.conv.bias.uniform_(-0.5, 0.5)
    return model.eval()


def edge_types(batch, relations, seed):
    """Seeded uniform types in ``[0, relations)``, int32 [E], one per ``batch.coo`` row; at ``relations == 8`` relation
    ``UNUSED_AT_8`` is left without an edge (its edges get relation 0)."""
    t = np.random.default_rng(seed).integers(0, relations, batch.num_edges).astype(np.int32)
    if relations == 8:
        t[t == UNUSED_AT_8] = 0
    return t


def _act(v, act):
    if act == "none":
        return v
    if act == "relu":
        return np.maximum(v, v.dtype.type(0))
    t = torch.from_numpy(np.ascontiguousarray(v))
    return {"gelu": torch.nn.functional.gelu, "sigmoid": torch.sigmoid, "tanh": torch.tanh}[act](t).numpy()


def relation_counts(coo, types, relations, num_nodes):
    """``|N_r(i)|`` as int64 [N, relations]: duplicate edges and ``(v, v)`` edges counted as they occur."""
    coo = np.asarray(coo).reshape(-1, 2)
    cnt = np.zeros((num_nodes, relations), np.int64)
    np.add.at(cnt, (coo[:, 1], np.asarray(types, np.int64)), 1)
    return cnt


def fault_bias(width, dtype):
    """The bias of the ``bias_per_edge`` fault: what a fold that left ``bias`` in the relation blocks would add per edge."""
    return (0.125 * (np.arange(width) % 3 + 1)).astype(dtype)


def rgcn_ref(p, root, skip, act, coo, types, relations, dtype=np.float64, fault=None):
    """One RGCNConv layer behind its GEMM, [N, width] in ``dtype``: ``p`` [N, relations * width] in relation blocks; per relation
    the sum of the in-edges' rows of its block, divided by their count, the relations added in turn, then ``root`` [N, width] or
    None, then ``skip`` [N, width] or None, then ``act`` -- PyG's order.  ``dtype=np.float32`` is ``base``.  ``fault``: one of
    ``FAULTS``, a wrong kernel restated -- no division, division by the whole in-degree, relation ``r`` reading block
    ``r + 1 mod relations``, a bias added to every gathered row, the types taken in another edge order than ``coo``'s."""
    coo = np.asarray(coo).reshape(-1, 2)
    src, dst = coo[:, 0].astype(np.int64), coo[:, 1].astype(np.int64)
    p = np.asarray(p, dtype)
    n, w = p.shape[0], p.shape[1] // relations
    t = np.asarray(types, np.int64)
    if fault == "types_in_input_order":  # (the types did not follow their edges through the ingest's sort)
        t = t[np.random.default_rng(99).permutation(t.size)]
    deg = np.bincount(dst, minlength=n).astype(dtype)
    out = np.zeros((n, w), dtype)
    for r in range(relations):
        m = t == r
        blk = (r + 1) % relations if fault == "block_shift" else r
        s = np.zeros((n, w), dtype)
        np.add.at(s, dst[m], p[src[m], blk * w:(blk + 1) * w])
        cnt = np.bincount(dst[m], minlength=n).astype(dtype)
        if fault == "bias_per_edge":
            s = (s + cnt[:, None] * fault_bias(w, dtype)[None, :]).astype(dtype)
        if fault == "sum_not_mean":
            term = s
        elif fault == "mean_over_all":
            term = s / np.maximum(deg, dtype(1))[:, None]
        else:
            term = s / np.maximum(cnt, dtype(1))[:, None]
        out = (out + term).astype(dtype)
    if root is not None:
        out = out + np.asarray(root, dtype)
    if skip is not None:
        out = out + np.asarray(skip, dtype)
    return _act(out.astype(dtype), act)


def slot_records(types, coo, row_ptr, in_deg, eid, relations):
    """The records numpy gives for the CSR slots of the tables (``tables_to_host``, ``edge_index_table_to_host``): int32 [E, 2],
    (relation, bits of ``np.float32(1) / np.float32(count)``); a type outside ``[0, relations)`` gives (0, bits of 0.0) and takes
    no part in a count.  Slots no row owns stay (0, 0)."""
    types = np.asarray(types, np.int64)
    coo = np.asarray(coo).reshape(-1, 2)
    n = len(in_deg)
    ok = (types >= 0) & (types < relations)
    cnt = np.zeros((n, relations), np.int64)
    np.add.at(cnt, (coo[ok, 1], types[ok]), 1)
    rec = np.zeros((len(types), 2), np.int32)
    for i in np.flatnonzero(np.asarray(in_deg) > 0):
        s = np.arange(row_ptr[i], row_ptr[i] + in_deg[i])
        t = types[eid[s]]
        good = (t >= 0) & (t < relations)
        tt = np.where(good, t, 0)
        w = np.where(good, np.float32(1) / np.maximum(cnt[i, tt], 1).astype(np.float32), np.float32(0)).astype(np.float32)
        rec[s, 0] = tt
        rec[s, 1] = w.view(np.int32)
    return rec


def run(model, batch, x, types):
    """The whole RGCNConv model as it stands (its own dtype): ``edge_type`` handed to every layer."""
    dtype = next(model.parameters()).dtype
    ei = R.edge_index(batch.coo)
    h = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)
    et = torch.from_numpy(np.asarray(types, np.int64))
    with torch.no_grad():
        for i, (conv, act) in enumerate(zip(model.gnn_convs, model.gnn_activations)):
            h_in = h
            h = conv(h, ei, et)
            if model.gnn_skip_connection and i != 0 and i != model.gnn_num_layers - 1:
                h = h + h_in
            h = act(h)
        # (the number of graphs given: a trailing graph without a node has its row)
        pooled = model.global_pooling(h, torch.from_numpy(batch_vector(batch)), batch.num_graphs)
        out = model.mlp_head(pooled)
        if model.output_activation_module is not None:
            out = model.output_activation_module(out)
    return out.numpy()


def forward64(model, batch, x, types):
    """The float64 reference: the model's own definition on a ``.double()`` copy."""
    return run(copy.deepcopy(model).double(), batch, x, types)
