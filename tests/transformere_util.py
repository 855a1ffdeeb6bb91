"""Shared builders of the tests of TransformerConv with edge features: a seeded ``GNNModel`` of ``TransformerEConv_GNNB`` layers,
the float64 restatements -- of the whole layer from ``x`` and its weights (``transformere_layer``: ``p_ij`` formed explicitly, an
explicit two-pass softmax per destination; ``folded=True``: the score through ``qe = W_e^T q`` and the value through ``W_e`` applied
to the weighted attribute sum, the algebra the accelerated path relies on) and of the stage behind its GEMM (``transformere_ref``:
``qe`` and ``w_edge`` as the separate operands they are there) --, nothing taken from models.py, and the stage's operands on dyadic
grids on which every score is exact in fp32."""
import numpy as np
import torch

import gnnbuilder_amd as gnnb
from helpers import ACTS
from transformer_util import _act, _grid, stage_case

EDGE_DIMS = (1, 3, 4, 16)


def make_transformere_model(in_dim=9, edge_dim=4, hidden=32, layers=3, out_dim=None, heads=4, act="relu", skip=True,
                            pools=("add", "mean", "max"), mlp_hidden=64, mlp_layers=2, task_out=19, out_act=None, seed=0):
    torch.manual_seed(seed)
    out_dim = hidden if out_dim is None else out_dim
    model = gnnb.GNNModel(in_dim, edge_dim, hidden, layers, out_dim, gnnb.TransformerEConv_GNNB, ACTS[act], skip,
                          gnnb.GlobalPooling(list(pools)), gnnb.MLP(len(pools) * out_dim, task_out, mlp_hidden, mlp_layers), out_act,
                          gnn_heads=heads)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("bias"):
                p.uniform_(-0.1, 0.1)
    return model.eval()


def _softmax_weights(s, dst, n, dtype):
    """PyG's softmax per destination and head in two explicit passes: the maximum, then exp(s - max) / (sum + 1e-16)."""
    heads = s.shape[1]
    smax = np.full((n, heads), -np.inf, dtype)
    np.maximum.at(smax, dst, s)
    e = np.exp(s - smax[dst]).astype(dtype)
    den = np.zeros((n, heads), dtype)
    np.add.at(den, dst, e)
    return (e / (den[dst] + dtype(1e-16))).astype(dtype)


def transformere_layer(x, coo, edge_attr, weights, heads, folded=False):
    """One layer from its input, in float64.  ``weights``: dict of ``key``, ``query``, ``value``, ``skip`` -> (W [H C, in], b [H C])
    and ``edge`` -> W_e [H C, d].  Direct (``folded=False``): ``p_ij = W_e e_ij`` per edge, added to the key row and to the value
    row.  ``folded=True``: ``s = q_i . k_j + (W_e[h]^T q_i[h]) . e_ij`` and ``out = sum a v_j + W_e[h] (sum a e_ij)`` -- no ``p_ij``."""
    f8 = np.float64
    x, ea = np.asarray(x, f8), np.asarray(edge_attr, f8)
    coo = np.asarray(coo).reshape(-1, 2)
    src, dst = coo[:, 0], coo[:, 1]
    n = x.shape[0]
    lin = lambda name: x @ np.asarray(weights[name][0], f8).T + np.asarray(weights[name][1], f8)  # noqa: E731
    we = np.asarray(weights["edge"], f8)
    w, d = we.shape
    c = w // heads
    ea = ea.reshape(len(coo), d)
    q, k, v = (lin(name).reshape(n, heads, c) for name in ("query", "key", "value"))
    we3 = we.reshape(heads, c, d)
    if not folded:
        p = np.einsum("hcd,ed->ehc", we3, ea)
        s = ((k[src] + p) * q[dst]).sum(-1) / np.sqrt(f8(c))
        a = _softmax_weights(s, dst, n, f8)
        out = np.zeros((n, heads, c), f8)
        np.add.at(out, dst, a[:, :, None] * (v[src] + p))
    else:
        qe = np.einsum("hcd,nhc->nhd", we3, q)
        s = ((k[src] * q[dst]).sum(-1) + (qe[dst] * ea[:, None, :]).sum(-1)) / np.sqrt(f8(c))
        a = _softmax_weights(s, dst, n, f8)
        out, aacc = np.zeros((n, heads, c), f8), np.zeros((n, heads, d), f8)
        np.add.at(out, dst, a[:, :, None] * v[src])
        np.add.at(aacc, dst, a[:, :, None] * ea[:, None, :])
        out = out + np.einsum("hcd,nhd->nhc", we3, aacc)
    return out.reshape(n, w) + lin("skip")


def layer_weights(conv):
    """``transformere_layer``'s ``weights`` of a ``_TransformerEConv``."""
    g = lambda m: (m.weight.detach().numpy(), m.bias.detach().numpy())  # noqa: E731
    return dict(key=g(conv.lin_key), query=g(conv.lin_query), value=g(conv.lin_value), skip=g(conv.lin_skip),
                edge=conv.lin_edge.weight.detach().numpy())


# ---- the stage
def transformere_scores(q, k, qe, coo, edge_attr, heads, scale, dtype=np.float64):
    """(src, dst, s [E, heads]) in ``dtype``: ``s = (sum_c q_dst[h, c] k_src[h, c] + sum_d qe_dst[h, d] e[d]) * scale`` (dot, then
    edge dot, then scale) over ``coo`` as given, explicit (v, v) rows included."""
    coo = np.asarray(coo).reshape(-1, 2)
    n, w = q.shape
    c = w // heads
    src, dst = coo[:, 0], coo[:, 1]
    q3, k3 = np.asarray(q, dtype).reshape(n, heads, c), np.asarray(k, dtype).reshape(n, heads, c)
    qe3 = np.asarray(qe, dtype).reshape(n, heads, -1)
    ea = np.asarray(edge_attr, dtype).reshape(len(coo), -1)
    s = (q3[dst] * k3[src]).sum(-1, dtype=dtype) + (qe3[dst] * ea[:, None, :]).sum(-1, dtype=dtype)
    return src, dst, (s * dtype(scale)).astype(dtype)


def transformere_ref(q, k, v, qe, root, skip, act, coo, edge_attr, w_edge, heads, scale, dtype=np.float64, return_weights=False):
    """``act((sum_j a_ij (v_j + w_edge e_ij) + root_i) + skip_i)`` [N, width] in ``dtype``: the projected term ``w_edge e_ij`` formed
    explicitly per edge (attribute index increasing), PyG's softmax in two explicit passes over ``transformere_scores``.
    ``dtype=np.float32`` is ``base``.  A row without in-edges is ``act(root_i + skip_i)``."""
    n, w = q.shape
    c = w // heads
    src, dst, s = transformere_scores(q, k, qe, coo, edge_attr, heads, scale, dtype)
    a = _softmax_weights(s, dst, n, dtype)
    ea, we = np.asarray(edge_attr, dtype).reshape(len(src), -1), np.asarray(w_edge, dtype)
    p = np.zeros((len(src), w), dtype)
    for t in range(we.shape[1]):
        p = (p + ea[:, t:t + 1] * we[None, :, t]).astype(dtype)
    out = np.zeros((n, heads, c), dtype)
    np.add.at(out, dst, a[:, :, None] * (np.asarray(v, dtype).reshape(n, heads, c)[src] + p.reshape(-1, heads, c)))
    out = out.reshape(n, w)
    if root is not None:
        out = out + np.asarray(root, dtype)
    if skip is not None:
        out = out + np.asarray(skip, dtype)
    out = _act(out.astype(dtype), act)
    return (out, a, dst, s) if return_weights else out


# ---- the stage's operands on dyadic grids: transformer_util.stage_case's (q, k, v multiples of 1/4 in [-1, 1], root and skip of
# 1/16, a power-of-two scale) plus qe, edge_attr and w_edge on multiples of 1/4 in [-1, 1].  A dot q . k is a multiple of 1/16 of
# magnitude <= C <= 256, the edge dot a multiple of 1/16 of magnitude <= d <= 16: their sum has at most 13 significant bits, exact
# in fp32 and float64 in any summation order, and the scale changes the exponent only -- every fp32 score IS the float64 score.
def edge_case(coo, num_nodes, width, heads, edge_dim, kind):
    """``stage_case``'s dict plus ``qe`` [N, heads * edge_dim], ``edge_attr`` [E, edge_dim] and ``w_edge`` [width, edge_dim]."""
    coo = np.asarray(coo).reshape(-1, 2)
    rng = np.random.default_rng(100000 * edge_dim + 1000 * width + heads)
    c = dict(stage_case(num_nodes, width, heads, kind))
    c["qe"] = _grid(rng, (num_nodes, heads * edge_dim), 0.25, 1.0)
    c["edge_attr"] = _grid(rng, (len(coo), edge_dim), 0.25, 1.0)
    c["w_edge"] = _grid(rng, (width, edge_dim), 0.25, 1.0)
    return c


def assert_exact_scores(c, coo, heads):
    """The exactness claim above, on the reference alone (fp32 against float64 on the CPU); returns the float64 (dst, s)."""
    args = (c["q"], c["k"], c["qe"], coo, c["edge_attr"], heads, c["scale"])
    _, dst, s64 = transformere_scores(*args, np.float64)
    _, _, s32 = transformere_scores(*args, np.float32)
    for name in ("q", "k", "qe", "edge_attr"):
        assert np.array_equal(c[name] * 4, np.round(c[name] * 4)) and np.abs(c[name]).max() <= 1.0
    assert np.log2(c["scale"]) == np.round(np.log2(c["scale"]))
    d16 = s64 / c["scale"] * 16
    assert np.array_equal(d16, np.round(d16)) and np.abs(d16).max() <= 16 * (256 + 16)
    assert s32.dtype == np.float32 and np.array_equal(s32.astype(np.float64), s64)  # every score is exact in fp32
    return dst, s64
