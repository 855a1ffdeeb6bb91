"""Shared builders of the tests of ResGatedGraphConv with edge features: a seeded ``GNNModel`` of ``ResGatedGraphEConv_GNNB``
layers, the float64 restatements -- of the whole layer from ``x`` and its weights, edge by edge (``resgatede_layer``: the
concatenation formed explicitly per edge) and of the stage behind its GEMM (``resgatede_ref``: ``w_gate`` and ``w_value`` as the
separate operands they are there) --, nothing taken from models.py, and the stage's operands on dyadic grids on which every gate
argument AND every gated value is exact in fp32."""
import numpy as np
import torch

import gnnbuilder_amd as gnnb
from helpers import ACTS
from resgated_util import _act, _grid, gates, stage_case

# (width, edge_dim): both row forms, several strides, both attribute forms (edge_dim % 4 == 0 or not), the caps, width 1
SHAPES = [(32, 4), (9, 3), (130, 16), (24, 1), (256, 16), (1, 4)]


def make_resgatede_model(in_dim=9, edge_dim=4, hidden=32, layers=3, out_dim=None, act="relu", skip=True, pools=("add", "mean", "max"),
                         mlp_hidden=64, mlp_layers=2, task_out=19, out_act=None, seed=0):
    torch.manual_seed(seed)
    out_dim = hidden if out_dim is None else out_dim
    model = gnnb.GNNModel(in_dim, edge_dim, hidden, layers, out_dim, gnnb.ResGatedGraphEConv_GNNB, ACTS[act], skip,
                          gnnb.GlobalPooling(list(pools)), gnnb.MLP(len(pools) * out_dim, task_out, mlp_hidden, mlp_layers), out_act)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("bias"):  # (the conv's own zero-initialised bias among them)
                p.uniform_(-0.1, 0.1)
    return model.eval()


def resgatede_layer(x, coo, edge_attr, weights):
    """One layer from its input, in float64, one edge at a time.  ``weights``: dict of ``key``, ``query``, ``value`` -> (W
    [out, in + d], b [out]), ``skip`` -> W [out, in], ``bias`` -> [out]."""
    f8 = np.float64
    x, ea = np.asarray(x, f8), np.asarray(edge_attr, f8)
    coo = np.asarray(coo).reshape(-1, 2)
    wk, bk = (np.asarray(a, f8) for a in weights["key"])
    wq, bq = (np.asarray(a, f8) for a in weights["query"])
    wv, bv = (np.asarray(a, f8) for a in weights["value"])
    out = x @ np.asarray(weights["skip"], f8).T + np.asarray(weights["bias"], f8)
    ea = ea.reshape(len(coo), -1)
    for e, (j, i) in enumerate(coo):
        zi, zj = np.concatenate([x[i], ea[e]]), np.concatenate([x[j], ea[e]])
        s = (wk @ zi + bk) + (wq @ zj + bq)
        out[i] += (1.0 / (1.0 + np.exp(-s))) * (wv @ zj + bv)
    return out


def layer_weights(conv):
    """``resgatede_layer``'s ``weights`` of a ``_ResGatedGraphEConv``."""
    g = lambda m: (m.weight.detach().numpy(), m.bias.detach().numpy())  # noqa: E731
    return dict(key=g(conv.lin_key), query=g(conv.lin_query), value=g(conv.lin_value), skip=conv.lin_skip.weight.detach().numpy(),
                bias=conv.bias.detach().numpy())


# ---- the stage
def edge_terms(k, q, v, coo, edge_attr, w_gate, w_value, dtype=np.float64):
    """(src, dst, s [E, width], u [E, width]) in ``dtype``: ``s = (k_dst + q_src) + sum_d w_gate[:, d] e[d]`` and ``u = v_src +
    sum_d w_value[:, d] e[d]``, the attribute index increasing, over ``coo`` as given.  ``w_gate`` / ``w_value`` None: that term
    removed."""
    coo = np.asarray(coo).reshape(-1, 2)
    src, dst = coo[:, 0], coo[:, 1]
    ea = np.asarray(edge_attr, dtype).reshape(len(coo), -1)
    s = (np.asarray(k, dtype)[dst] + np.asarray(q, dtype)[src]).astype(dtype)
    u = np.asarray(v, dtype)[src].astype(dtype)
    for t in range(ea.shape[1]):
        if w_gate is not None:
            s = (s + np.asarray(w_gate, dtype)[None, :, t] * ea[:, t:t + 1]).astype(dtype)
        if w_value is not None:
            u = (u + np.asarray(w_value, dtype)[None, :, t] * ea[:, t:t + 1]).astype(dtype)
    return src, dst, s, u


def resgatede_ref(k, q, v, root, skip, act, coo, edge_attr, w_gate, w_value, dtype=np.float64):
    """``act((sum_j sigmoid(s_ij) * u_ij + root_i) + skip_i)`` [N, width] in ``dtype`` with ``edge_terms``' s and u: the neighbours
    added with ``np.add.at`` in COO order per destination, ``root`` and ``skip`` last.  ``dtype=np.float32`` is ``base``.  A row
    without in-edges is ``act(root_i + skip_i)``."""
    _, dst, s, u = edge_terms(k, q, v, coo, edge_attr, w_gate, w_value, dtype)
    out = np.zeros(np.asarray(k).shape, dtype)
    np.add.at(out, dst, (gates(s) * u).astype(dtype))
    if root is not None:
        out = out + np.asarray(root, dtype)
    if skip is not None:
        out = out + np.asarray(skip, dtype)
    return _act(out.astype(dtype), act)


# ---- the stage's operands on dyadic grids: resgated_util.stage_case's (k and q multiples of 1/4 in [-2, 2], times 64 for "steep";
# v, root and skip multiples of 1/16 in [-1, 1]) plus w_gate in {-1/4, 0, 1/4} and edge_attr and w_value on multiples of 1/4 in
# [-1, 1].  A product w e is a multiple of 1/16; the gate's edge term has magnitude <= d / 4 <= 4, so "flat" arguments are
# multiples of 1/16 with |s| <= 8 and "steep" ones reach +-260; the value's edge term has magnitude <= d <= 16, u a multiple of
# 1/16 with |u| <= 17.  Every partial sum has at most 13 significant bits: s and u are exact in fp32 in any order.
def edge_case(coo, num_nodes, width, edge_dim, kind):
    """``stage_case``'s dict plus ``edge_attr`` [E, edge_dim], ``w_gate`` and ``w_value`` [width, edge_dim]."""
    coo = np.asarray(coo).reshape(-1, 2)
    rng = np.random.default_rng(100000 * edge_dim + 1000 * width + 3)
    c = dict(stage_case(num_nodes, width, kind))
    c["edge_attr"] = _grid(rng, (len(coo), edge_dim), 0.25, 1.0)
    c["w_gate"] = (rng.integers(-1, 2, (width, edge_dim)) * 0.25).astype(np.float32) + np.float32(0)
    c["w_value"] = _grid(rng, (width, edge_dim), 0.25, 1.0)
    return c


def assert_exact_terms(c, coo):
    """The exactness claim above, on the reference alone (fp32 against float64 on the CPU); returns the fp32 (dst, s, u)."""
    args = (c["k"], c["q"], c["v"], coo, c["edge_attr"], c["w_gate"], c["w_value"])
    _, dst, s64, u64 = edge_terms(*args, np.float64)
    _, _, s32, u32 = edge_terms(*args, np.float32)
    assert set(np.unique(c["w_gate"])) <= {-0.25, 0.0, 0.25}
    for name in ("edge_attr", "w_value"):
        assert np.array_equal(c[name] * 4, np.round(c[name] * 4)) and np.abs(c[name]).max() <= 1.0
    assert s32.dtype == np.float32 and np.array_equal(s32.astype(np.float64), s64)  # every gate argument is exact in fp32
    assert u32.dtype == np.float32 and np.array_equal(u32.astype(np.float64), u64)  # ... and so is every gated value
    return dst, s32, u32
