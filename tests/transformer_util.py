"""Shared builders of the TransformerConv tests: a seeded ``GNNModel`` of ``TransformerConv_GNNB`` layers, the float64 restatement
of one attention layer behind its GEMM (``transformer_ref``: an explicit two-pass softmax per destination, nothing taken from
models.py), and the stage's operands on dyadic grids on which every score is exact in fp32."""
import numpy as np
import torch

import gnnbuilder_amd as gnnb
from helpers import ACTS

SHAPES = [(32, 1), (32, 4), (9, 3), (130, 2), (24, 2), (256, 8)]  # (width, heads): both forms, one and four strides, odd C


def make_transformer_model(in_dim=9, hidden=32, layers=3, out_dim=None, heads=4, act="relu", skip=True, pools=("add", "mean", "max"),
                           mlp_hidden=64, mlp_layers=2, task_out=19, out_act=None, seed=0):
    torch.manual_seed(seed)
    out_dim = hidden if out_dim is None else out_dim
    model = gnnb.GNNModel(in_dim, None, hidden, layers, out_dim, gnnb.TransformerConv_GNNB, ACTS[act], skip,
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


def transformer_scores(q, k, coo, heads, scale, dtype=np.float64):
    """(src, dst, s [E, heads]) of the edges the layer attends over -- ``coo`` as given, explicit (v, v) rows included, no self
    loop added -- in ``dtype``: ``s = (sum_c q_dst[h, c] * k_src[h, c]) * scale`` (dot, then scale)."""
    coo = np.asarray(coo).reshape(-1, 2)
    n, w = q.shape
    c = w // heads
    src, dst = coo[:, 0], coo[:, 1]
    q3, k3 = np.asarray(q, dtype).reshape(n, heads, c), np.asarray(k, dtype).reshape(n, heads, c)
    return src, dst, ((q3[dst] * k3[src]).sum(-1, dtype=dtype) * dtype(scale)).astype(dtype)


def transformer_ref(q, k, v, root, skip, act, coo, heads, scale, dtype=np.float64, return_weights=False):
    """``act((sum_j a_ij v_j + root_i) + skip_i)`` [N, width] in ``dtype`` with PyG's softmax in two explicit passes per
    destination and head: the maximum of the scores, then ``exp(s - max) / (sum exp(s - max) + 1e-16)``.  ``dtype=np.float32`` is
    ``base``.  A row without in-edges is ``act(root_i + skip_i)``."""
    n, w = q.shape
    c = w // heads
    src, dst, s = transformer_scores(q, k, coo, heads, scale, dtype)
    smax = np.full((n, heads), -np.inf, dtype)
    np.maximum.at(smax, dst, s)
    e = np.exp(s - smax[dst]).astype(dtype)
    den = np.zeros((n, heads), dtype)
    np.add.at(den, dst, e)
    a = (e / (den[dst] + dtype(1e-16))).astype(dtype)
    out = np.zeros((n, heads, c), dtype)
    np.add.at(out, dst, a[:, :, None] * np.asarray(v, dtype).reshape(n, heads, c)[src])
    out = out.reshape(n, w)
    if root is not None:
        out = out + np.asarray(root, dtype)
    if skip is not None:
        out = out + np.asarray(skip, dtype)
    out = _act(out.astype(dtype), act)
    return (out, a, dst, s) if return_weights else out


# ---- the stage's operands on dyadic grids.  q and k are multiples of 1/4 in [-1, 1]: a product is a multiple of 1/16 in [-1, 1]
# and a dot product over C <= 256 columns a multiple of 1/16 of magnitude <= 256 -- at most 13 significant bits, exact in fp32 and
# float64 in any summation order.  The scale is a power of two ("flat": 2^-ceil(log2 C), so |s| <= 1; "steep": 256, so scores
# hundreds apart and the softmax one-hot), which changes the exponent only: every fp32 score IS the float64 score.
def _grid(rng, shape, step, span):
    return (np.round(rng.uniform(-span, span, shape) / step) * step).astype(np.float32)


def stage_scale(width, heads, kind):
    c = width // heads
    return 2.0 ** -int(np.ceil(np.log2(c))) if kind == "flat" else 256.0


def stage_case(num_nodes, width, heads, kind):
    """dict of q, k, v, root, skip [N, width] (fp32) and ``scale`` for operand set ``kind`` ("flat" / "steep"); the operands do not
    depend on ``kind``, the scale does."""
    rng = np.random.default_rng(1000 * width + heads)
    return dict(q=_grid(rng, (num_nodes, width), 0.25, 1.0), k=_grid(rng, (num_nodes, width), 0.25, 1.0),
                v=_grid(rng, (num_nodes, width), 0.25, 1.0), root=_grid(rng, (num_nodes, width), 1 / 16, 1.0),
                skip=_grid(rng, (num_nodes, width), 1 / 16, 1.0), scale=stage_scale(width, heads, kind))
