"""Shared builders of the tests of GAT (v1) with edge features: a seeded ``GNNModel`` of ``GATv1EConv_GNNB`` layers, the float64
restatement of one attention layer behind its GEMM (``gate_ref``: an explicit per-destination attribute MEAN for the self loops,
projected afterwards -- PyG's order, not the kernel's --, an explicit two-pass softmax per destination, nothing taken from
models.py), and the stage's operands on dyadic grids."""
import numpy as np
import torch

import gat_util
import gnnbuilder_amd as gnnb
from gatv2_util import SLOPE, _act, _grid  # noqa: F401  (SLOPE: the stage tests' negative_slope, 1/4)
from gatv2e_util import attended_edges
from helpers import ACTS


def make_gate_model(in_dim=9, edge_dim=4, hidden=32, layers=3, out_dim=None, heads=4, act="relu", skip=True, pools=("add", "mean", "max"),
                    mlp_hidden=64, mlp_layers=2, task_out=19, out_act=None, seed=0):
    torch.manual_seed(seed)
    out_dim = hidden if out_dim is None else out_dim
    model = gnnb.GNNModel(in_dim, edge_dim, hidden, layers, out_dim, gnnb.GATv1EConv_GNNB, ACTS[act], skip,
                          gnnb.GlobalPooling(list(pools)), gnnb.MLP(len(pools) * out_dim, task_out, mlp_hidden, mlp_layers), out_act,
                          gnn_heads=heads)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("bias"):
                p.uniform_(-0.1, 0.1)
    return model.eval()


def fold_edge(w_edge, att_edge, heads, dtype=np.float64):
    """``a_edge`` [heads, d] in ``dtype``: row h = sum_c att_edge[h, c] * w_edge[h C + c, :], c increasing."""
    w_edge = np.asarray(w_edge, dtype)
    c = w_edge.shape[0] // heads
    att = np.asarray(att_edge, dtype).reshape(heads, c)
    out = np.zeros((heads, w_edge.shape[1]), dtype)
    for k in range(c):
        out = (out + att[:, k:k + 1] * w_edge[np.arange(heads) * c + k]).astype(dtype)
    return out


def gate_scores(s_src, s_dst, a_edge, coo, edge_attr, slope, dtype=np.float64, fill="mean"):
    """(src, dst, s [E' + N, heads], num_kept): ``s = leaky_relu((s_src[src] + s_dst[dst]) + a_edge . attr)`` (attribute index
    increasing) in ``dtype`` over ``coo`` without its explicit (v, v) rows, then one self loop per node whose attribute is the MEAN
    of the node's remaining in-edges' attributes (``fill=0``: zeros, NOT the layer); the last N rows are the self loops'."""
    n = np.asarray(s_src).shape[0]
    if np.asarray(coo).size == 0:  # (a batch without edges: the self loops alone, their attribute 0 -- the width from a_edge)
        loops = np.arange(n)
        src, dst, attr, kept = loops, loops, np.zeros((n, np.asarray(a_edge).shape[1]), dtype), 0
    else:
        src, dst, attr, kept = attended_edges(coo, edge_attr, n, dtype, fill)
    ae = np.asarray(a_edge, dtype)
    t = np.zeros((len(src), ae.shape[0]), dtype)
    for k in range(ae.shape[1]):
        t = (t + attr[:, k:k + 1] * ae[None, :, k]).astype(dtype)
    z = (np.asarray(s_src, dtype)[src] + np.asarray(s_dst, dtype)[dst]) + t
    return src, dst, np.where(z > 0, z, z * dtype(slope)).astype(dtype), kept


def gate_ref(xl, s_src, s_dst, a_edge, bias, skip, act, coo, edge_attr, heads, slope, dtype=np.float64, fill="mean"):
    """``act(sum_j a_ij xl_j + bias + skip_i)`` [N, width] in ``dtype``: PyG's softmax in two explicit passes per destination and
    head over the scores of ``gate_scores``; the message is ``xl_j`` alone.  ``dtype=np.float32`` is ``base``."""
    n, w = xl.shape
    c = w // heads
    src, dst, s, _ = gate_scores(s_src, s_dst, a_edge, coo, edge_attr, slope, dtype, fill)
    smax = np.full((n, heads), -np.inf, dtype)
    np.maximum.at(smax, dst, s)
    e = np.exp(s - smax[dst]).astype(dtype)
    den = np.zeros((n, heads), dtype)
    np.add.at(den, dst, e)
    a = (e / (den[dst] + dtype(1e-16))).astype(dtype)
    out = np.zeros((n, heads, c), dtype)
    np.add.at(out, dst, a[:, :, None] * np.asarray(xl, dtype).reshape(n, heads, c)[src])
    out = out.reshape(n, w)
    if bias is not None:
        out = out + np.asarray(bias, dtype)
    if skip is not None:
        out = out + np.asarray(skip, dtype)
    return _act(out.astype(dtype), act)


# ---- the stage's operands on dyadic grids (negative_slope SLOPE = 1/4).  xl, bias, skip, s_src, s_dst: gat_util.stage_case's.
# "flat": s_src, s_dst multiples of 1/8 in [-1, 1]; a_edge and edge_attr multiples of 1/4 in [-1, 1]: t = a_edge . e is a multiple of
#   1/16 with |t| <= d <= 16, z = (s_src + s_dst) + t a multiple of 1/16 with |z| <= 18, leaky_relu(z) a multiple of 1/64: at most 11
#   significant bits -- every NON-SELF score is exact in fp32 and float64.  The self score is not: its attribute is a mean,
#   sum / deg, which rounds.  That is intended: it is the layer's new arithmetic.
# "steep": s_src, s_dst the integers of [-256, 256]; a_edge and edge_attr multiples of 1/2 in [-1, 1] and the attribute rows CONSTANT
#   PER DESTINATION: t is a multiple of 1/4 with |t| <= 16; k t is exact for every k <= 1200 (a multiple of 1/4 below 2^15), so the
#   kernel's (k t) / k = t, and the mean of k equal rows r is (k r) / k = r exactly: EVERY score, the self score included, is exact
#   in fp32 -- z an integer multiple of 1/4 with |z| <= 528, its leaky_relu a multiple of 1/16.
def edge_case(coo, num_nodes, width, heads, edge_dim, kind, seed=None):
    """``gat_util.stage_case``'s dict plus ``edge_attr`` [E, edge_dim] and ``a_edge`` [heads, edge_dim] for operand set ``kind``."""
    coo = np.asarray(coo).reshape(-1, 2)
    rng = np.random.default_rng(100000 * edge_dim + 1000 * width + heads if seed is None else seed)
    c = gat_util.stage_case(num_nodes, width, heads, kind, seed=seed)
    if kind == "flat":
        c["edge_attr"] = _grid(rng, (len(coo), edge_dim), 0.25, 1.0)
        c["a_edge"] = _grid(rng, (heads, edge_dim), 0.25, 1.0)
    else:
        c["edge_attr"] = _grid(rng, (num_nodes, edge_dim), 0.5, 1.0)[coo[:, 1]]
        c["a_edge"] = _grid(rng, (heads, edge_dim), 0.5, 1.0)
    return c


def assert_exact_scores(c, coo, kind):
    """The exactness claims above, on the reference alone (fp32 against float64 on the CPU); returns the float64 scores'
    (dst, s, num_kept)."""
    args = (c["s_src"], c["s_dst"], c["a_edge"], coo, c["edge_attr"], SLOPE)
    _, dst, s64, kept = gate_scores(*args, np.float64)
    _, _, s32, _ = gate_scores(*args, np.float32)
    assert s32.dtype == np.float32
    assert np.array_equal(s32[:kept].astype(np.float64), s64[:kept])  # every non-self score is exact in fp32
    if kind == "steep":
        assert np.array_equal(s32.astype(np.float64), s64)  # ... and the self scores too: the mean of equal rows is the row
    return dst, s64, kept
