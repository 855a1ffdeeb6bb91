"""Shared builders of the GAT (v1) tests: a seeded ``GNNModel`` of ``GATv1Conv_GNNB`` layers, the float64 restatement of one
attention layer behind its GEMM (``gat_ref``: an explicit two-pass softmax per destination, nothing taken from models.py), and the
stage's operands on dyadic grids on which every score is exact in fp32."""
import numpy as np
import torch

import gatv2_util
import gnnbuilder_amd as gnnb
from gatv2_util import SLOPE, _act, _grid  # noqa: F401  (SLOPE = 1/4: a power of two, so that leaky_relu stays on the grid)
from helpers import ACTS


def make_gat_model(in_dim=9, hidden=32, layers=3, out_dim=None, heads=4, act="relu", skip=True, pools=("add", "mean", "max"),
                   mlp_hidden=64, mlp_layers=2, task_out=19, out_act=None, seed=0):
    torch.manual_seed(seed)
    out_dim = hidden if out_dim is None else out_dim
    model = gnnb.GNNModel(in_dim, None, hidden, layers, out_dim, gnnb.GATv1Conv_GNNB, ACTS[act], skip,
                          gnnb.GlobalPooling(list(pools)), gnnb.MLP(len(pools) * out_dim, task_out, mlp_hidden, mlp_layers), out_act,
                          gnn_heads=heads)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("bias"):
                p.uniform_(-0.1, 0.1)
    return model.eval()


def gat_scores(s_src, s_dst, coo, slope, dtype=np.float64):
    """(src, dst, s [E', heads]) of the edges the layer attends over -- ``coo`` without its explicit (v, v) rows, then one self
    loop per node -- in ``dtype``: ``s = leaky_relu(s_src[src] + s_dst[dst])``."""
    coo = np.asarray(coo).reshape(-1, 2)
    coo = coo[coo[:, 0] != coo[:, 1]]
    loops = np.arange(s_src.shape[0])
    src, dst = np.concatenate([coo[:, 0], loops]), np.concatenate([coo[:, 1], loops])
    z = np.asarray(s_src, dtype)[src] + np.asarray(s_dst, dtype)[dst]
    return src, dst, np.where(z > 0, z, z * dtype(slope)).astype(dtype)


def gat_ref(xl, s_src, s_dst, bias, skip, act, coo, heads, slope, dtype=np.float64, return_weights=False):
    """``act(sum_j a_ij xl_j + bias + skip_i)`` [N, width] in ``dtype`` with PyG's softmax in two explicit passes per destination
    and head: the maximum of the scores, then ``exp(s - max) / (sum exp(s - max) + 1e-16)``.  ``dtype=np.float32`` is ``base``."""
    n, w = xl.shape
    c = w // heads
    src, dst, s = gat_scores(s_src, s_dst, coo, slope, dtype)
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
    out = _act(out.astype(dtype), act)
    return (out, a, dst) if return_weights else out


def stage_case(num_nodes, width, heads, kind, seed=None):
    """dict of xl [N, width], s_src, s_dst [N, heads], bias [width], skip [N, width] (fp32) for operand set ``kind``.  xl, bias and
    skip are ``gatv2_util.stage_case``'s (multiples of 1/4 and 1/16 in [-1, 1]).  The scores come from
    ``default_rng(1000 * width + heads)``, s_src drawn before s_dst -- "flat": multiples of 1/8 in [-1, 1], so z = s_src + s_dst is
    a multiple of 1/8 in [-2, 2] and leaky_relu of it (slope 1/4) a multiple of 1/32; "steep": the integers of [-256, 256], z an
    integer in [-512, 512], its leaky_relu a multiple of 1/4.  Either way a score is exact in fp32 and in float64."""
    base = gatv2_util.stage_case(num_nodes, width, heads, "flat", seed)
    rng = np.random.default_rng(1000 * width + heads if seed is None else seed)
    step, span = (1 / 8, 1.0) if kind == "flat" else (1.0, 256.0)
    s_src = _grid(rng, (num_nodes, heads), step, span)
    s_dst = _grid(rng, (num_nodes, heads), step, span)
    return dict(xl=base["xl"], s_src=s_src, s_dst=s_dst, bias=base["bias"], skip=base["skip"])
