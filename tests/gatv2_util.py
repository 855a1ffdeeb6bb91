"""Shared builders of the GATv2 tests: a seeded ``GNNModel`` of ``GATv2Conv_GNNB`` layers, the float64 restatement of one
attention layer behind its GEMM (``gatv2_ref``: an explicit two-pass softmax per destination, nothing taken from models.py), and
the stage's operands on dyadic grids on which every score is exact in fp32."""
import numpy as np
import torch

import gnnbuilder_amd as gnnb
from helpers import ACTS

SLOPE = 0.25  # the stage tests' negative_slope: a power of two, so that leaky_relu stays on the grid


def make_gatv2_model(in_dim=9, hidden=32, layers=3, out_dim=None, heads=4, act="relu", skip=True, pools=("add", "mean", "max"),
                     mlp_hidden=64, mlp_layers=2, task_out=19, out_act=None, seed=0):
    torch.manual_seed(seed)
    out_dim = hidden if out_dim is None else out_dim
    model = gnnb.GNNModel(in_dim, None, hidden, layers, out_dim, gnnb.GATv2Conv_GNNB, ACTS[act], skip,
                          gnnb.GlobalPooling(list(pools)), gnnb.MLP(len(pools) * out_dim, task_out, mlp_hidden, mlp_layers), out_act,
                          gnn_heads=heads)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("bias"):
                p.uniform_(-0.1, 0.1)
    return model.eval()


def _act(v, act):
    if act == "none":
        return v
    if act == "relu":
        return np.maximum(v, v.dtype.type(0))
    t = torch.from_numpy(np.ascontiguousarray(v))
    return {"gelu": torch.nn.functional.gelu, "sigmoid": torch.sigmoid, "tanh": torch.tanh}[act](t).numpy()


def gatv2_scores(xl, xr, att, coo, heads, slope, dtype=np.float64):
    """(src, dst, s [E', heads]) of the edges the layer attends over -- ``coo`` without its explicit (v, v) rows, then one self
    loop per node -- in ``dtype``: ``s = sum_c att[h, c] * leaky_relu(xl_src[h, c] + xr_dst[h, c])``."""
    coo = np.asarray(coo).reshape(-1, 2)
    coo = coo[coo[:, 0] != coo[:, 1]]
    n, w = xl.shape
    c = w // heads
    loops = np.arange(n)
    src, dst = np.concatenate([coo[:, 0], loops]), np.concatenate([coo[:, 1], loops])
    xl3, xr3 = np.asarray(xl, dtype).reshape(n, heads, c), np.asarray(xr, dtype).reshape(n, heads, c)
    z = xl3[src] + xr3[dst]
    z = np.where(z > 0, z, z * dtype(slope))
    return src, dst, (z * np.asarray(att, dtype).reshape(1, heads, c)).sum(-1, dtype=dtype)


def gatv2_ref(xl, xr, att, bias, skip, act, coo, heads, slope, dtype=np.float64, return_weights=False):
    """``act(sum_j a_ij xl_j + bias + skip_i)`` [N, width] in ``dtype`` with PyG's softmax in two explicit passes per destination
    and head: the maximum of the scores, then ``exp(s - max) / (sum exp(s - max) + 1e-16)``.  ``dtype=np.float32`` is ``base``."""
    n, w = xl.shape
    c = w // heads
    src, dst, s = gatv2_scores(xl, xr, att, coo, heads, slope, dtype)
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


# ---- the stage's operands on dyadic grids.  xl and xr are multiples of 1/4 in [-1, 1], so xl_j + xr_i is a multiple of 1/4 in
# [-2, 2] and leaky_relu of it (slope 1/4) a multiple of 1/16.  "flat": att on multiples of span / 4 with span = 2^-ceil(log2 C):
# |s| <= 2 C span <= 2 and every term a multiple of span / 64 -- at most 9 + log2(C) <= 17 significant bits.  "steep": att on
# the integers of [-256, 256]: every term a multiple of 1/16 and |s| <= 512 C <= 2^17 -- 21 bits.  Either way a score is exact in
# fp32 and float64 in any summation order.
def _grid(rng, shape, step, span):
    return (np.round(rng.uniform(-span, span, shape) / step) * step).astype(np.float32)


def stage_case(num_nodes, width, heads, kind, seed=None):
    """dict of xl, xr [N, width], att [width], bias [width], skip [N, width] (fp32) for operand set ``kind`` ("flat" / "steep")."""
    rng = np.random.default_rng(1000 * width + heads if seed is None else seed)
    c = width // heads
    span = 2.0 ** -int(np.ceil(np.log2(c))) if kind == "flat" else 256.0
    step = span / 4 if kind == "flat" else 1.0
    return dict(xl=_grid(rng, (num_nodes, width), 0.25, 1.0), xr=_grid(rng, (num_nodes, width), 0.25, 1.0), att=_grid(rng, (width,), step, span),
                bias=_grid(rng, (width,), 1 / 16, 1.0), skip=_grid(rng, (num_nodes, width), 1 / 16, 1.0))
