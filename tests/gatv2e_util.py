"""Shared builders of the tests of GATv2 with edge features: a seeded ``GNNModel`` of ``GATv2EConv_GNNB`` layers, the float64
restatement of one attention layer behind its GEMM (``gatv2e_ref``: an explicit per-destination attribute mean for the self loops,
an explicit two-pass softmax per destination, nothing taken from models.py), and the stage's operands on dyadic grids."""
import numpy as np
import torch

import gnnbuilder_amd as gnnb
from gatv2_util import SLOPE, _act, _grid, stage_case  # noqa: F401  (SLOPE: the stage tests' negative_slope, 1/4)
from helpers import ACTS


def make_gatv2e_model(in_dim=9, edge_dim=4, hidden=32, layers=3, out_dim=None, heads=4, act="relu", skip=True, pools=("add", "mean", "max"),
                      mlp_hidden=64, mlp_layers=2, task_out=19, out_act=None, seed=0):
    torch.manual_seed(seed)
    out_dim = hidden if out_dim is None else out_dim
    model = gnnb.GNNModel(in_dim, edge_dim, hidden, layers, out_dim, gnnb.GATv2EConv_GNNB, ACTS[act], skip,
                          gnnb.GlobalPooling(list(pools)), gnnb.MLP(len(pools) * out_dim, task_out, mlp_hidden, mlp_layers), out_act,
                          gnn_heads=heads)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("bias"):
                p.uniform_(-0.1, 0.1)
    return model.eval()


def attended_edges(coo, edge_attr, num_nodes, dtype=np.float64, fill="mean"):
    """(src, dst, attr [E' + N, d], num_kept) of the edges the layer attends over, in ``dtype``: ``coo`` without its explicit
    (v, v) rows -- their attribute rows are dropped with them, whatever they hold --, then one self loop per node whose attribute
    is the mean of the attributes of the node's remaining in-edges (0 without any); ``fill=0``: zeros instead (NOT the layer: the
    variant a kernel that ignores the mean would compute)."""
    coo = np.asarray(coo).reshape(-1, 2)
    keep = coo[:, 0] != coo[:, 1]
    coo, ea = coo[keep], np.asarray(edge_attr).reshape(len(keep), -1)[keep].astype(dtype)
    d = ea.shape[1]
    loop_attr = np.zeros((num_nodes, d), dtype)
    if fill == "mean":
        deg = np.bincount(coo[:, 1], minlength=num_nodes)
        np.add.at(loop_attr, coo[:, 1], ea)  # (in COO order = CSR slot order per destination: graph prep's fill is stable)
        loop_attr = (loop_attr / np.maximum(deg, 1).astype(dtype)[:, None]).astype(dtype)
    else:
        assert fill == 0
    loops = np.arange(num_nodes)
    return np.concatenate([coo[:, 0], loops]), np.concatenate([coo[:, 1], loops]), np.concatenate([ea, loop_attr]), len(coo)


def gatv2e_scores(xl, xr, att, coo, edge_attr, w_edge, heads, slope, dtype=np.float64, fill="mean"):
    """(src, dst, s [E' + N, heads], num_kept): ``s = sum_c att[h, c] * leaky_relu((xl_src[h, c] + xr_dst[h, c]) + p[h, c])`` with
    ``p = w_edge @ attr`` (attribute index increasing) in ``dtype``; the last N rows are the self loops'."""
    n, w = xl.shape
    c = w // heads
    src, dst, attr, kept = attended_edges(coo, edge_attr, n, dtype, fill)
    we = np.asarray(w_edge, dtype)
    p = np.zeros((len(src), w), dtype)
    for k in range(we.shape[1]):
        p = (p + attr[:, k:k + 1] * we[None, :, k]).astype(dtype)
    xl3, xr3 = np.asarray(xl, dtype).reshape(n, heads, c), np.asarray(xr, dtype).reshape(n, heads, c)
    z = (xl3[src] + xr3[dst]) + p.reshape(-1, heads, c)
    z = np.where(z > 0, z, z * dtype(slope))
    return src, dst, (z * np.asarray(att, dtype).reshape(1, heads, c)).sum(-1, dtype=dtype), kept


def gatv2e_ref(xl, xr, att, bias, skip, act, coo, edge_attr, w_edge, heads, slope, dtype=np.float64, fill="mean"):
    """``act(sum_j a_ij xl_j + bias + skip_i)`` [N, width] in ``dtype``: PyG's softmax in two explicit passes per destination and
    head over the scores of ``gatv2e_scores``; the message is ``xl_j`` alone.  ``dtype=np.float32`` is ``base``."""
    n, w = xl.shape
    c = w // heads
    src, dst, s, _ = gatv2e_scores(xl, xr, att, coo, edge_attr, w_edge, heads, slope, dtype, fill)
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


# ---- the stage's operands on dyadic grids (negative_slope SLOPE = 1/4).
# "flat": gatv2_util.stage_case's grids (xl, xr multiples of 1/4 in [-1, 1]; att multiples of span / 4, span = 2^-ceil(log2 C)) plus
#   edge_attr and W_e on multiples of 1/4 in [-1, 1]: p is a multiple of 1/16 with |p| <= d <= 16, z = xl + xr + p a multiple of 1/16
#   with |z| <= 18, leaky_relu(z) a multiple of 1/64, a term a multiple of span / 256 and |s| <= 18 C span <= 36: at most
#   14 + log2(C) <= 22 significant bits -- every NON-SELF score is exact in fp32 and float64 in any summation order.  The self
#   score is not: its attribute is a mean, sum / deg, which rounds.  That is intended: it is the layer's new arithmetic.
# "steep": att on the integers of [-A, A], A = min(256, 2^(15 - ceil(log2 C))); W_e and edge_attr on multiples of 1/2 in [-1, 1] and
#   the attribute rows CONSTANT PER DESTINATION: p is a multiple of 1/4 with |p| <= 16, z a multiple of 1/4, leaky_relu(z) of 1/16,
#   |s| <= 18 A C <= 18 * 2^15 at a resolution of 1/16: below 2^24 steps.  The mean of k equal rows r is (k r) / k = r exactly (k r
#   is exact: a multiple of 1/2 below 2^11), so EVERY score, the self score included, is exact in fp32.
def edge_case(coo, num_nodes, width, heads, edge_dim, kind, seed=None):
    """``stage_case``'s dict plus ``edge_attr`` [E, edge_dim] and ``w_edge`` [width, edge_dim] for operand set ``kind``."""
    coo = np.asarray(coo).reshape(-1, 2)
    rng = np.random.default_rng(100000 * edge_dim + 1000 * width + heads if seed is None else seed)
    c = stage_case(num_nodes, width, heads, kind, seed=seed)
    C = width // heads
    if kind == "flat":
        c["edge_attr"] = _grid(rng, (len(coo), edge_dim), 0.25, 1.0)
        c["w_edge"] = _grid(rng, (width, edge_dim), 0.25, 1.0)
    else:
        A = min(256.0, 2.0 ** (15 - int(np.ceil(np.log2(C)))))
        c["att"] = _grid(rng, (width,), 1.0, A)
        c["edge_attr"] = _grid(rng, (num_nodes, edge_dim), 0.5, 1.0)[coo[:, 1]]
        c["w_edge"] = _grid(rng, (width, edge_dim), 0.5, 1.0)
    return c


def assert_exact_scores(c, coo, heads, kind):
    """The exactness claims above, on the reference alone (fp32 against float64 on the CPU); returns the float64 scores'
    (dst, s, num_kept)."""
    args = (c["xl"], c["xr"], c["att"], coo, c["edge_attr"], c["w_edge"], heads, SLOPE)
    _, dst, s64, kept = gatv2e_scores(*args, np.float64)
    _, _, s32, _ = gatv2e_scores(*args, np.float32)
    assert s32.dtype == np.float32
    assert np.array_equal(s32[:kept].astype(np.float64), s64[:kept])  # every non-self score is exact in fp32
    if kind == "steep":
        assert np.array_equal(s32.astype(np.float64), s64)  # ... and the self scores too: the mean of equal rows is the row
    return dst, s64, kept
