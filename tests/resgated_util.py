"""Shared builders of the ResGatedGraphConv tests: a seeded ``GNNModel`` of ``ResGatedGraphConv_GNNB`` layers, the float64
restatement of one gated layer behind its GEMM (``resgated_ref``: nothing taken from models.py), and the stage's operands on
dyadic grids on which every gate argument ``k_i + q_j`` is exact in fp32."""
import numpy as np
import torch

import gnnbuilder_amd as gnnb
from helpers import ACTS

WIDTHS = [32, 9, 130, 24, 256, 1]  # both forms, one and several strides, an odd width, the cap, and width 1


def make_resgated_model(in_dim=9, hidden=32, layers=3, out_dim=None, act="relu", skip=True, pools=("add", "mean", "max"),
                        mlp_hidden=64, mlp_layers=2, task_out=19, out_act=None, seed=0):
    torch.manual_seed(seed)
    out_dim = hidden if out_dim is None else out_dim
    model = gnnb.GNNModel(in_dim, None, hidden, layers, out_dim, gnnb.ResGatedGraphConv_GNNB, ACTS[act], skip,
                          gnnb.GlobalPooling(list(pools)), gnnb.MLP(len(pools) * out_dim, task_out, mlp_hidden, mlp_layers), out_act)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("bias"):  # (the conv's own zero-initialised bias among them)
                p.uniform_(-0.1, 0.1)
    return model.eval()


def _act(v, act):
    if act == "none":
        return v
    if act == "relu":
        return np.maximum(v, v.dtype.type(0))
    t = torch.from_numpy(np.ascontiguousarray(v))
    return {"gelu": torch.nn.functional.gelu, "sigmoid": torch.sigmoid, "tanh": torch.tanh}[act](t).numpy()


def gate_arguments(k, q, coo, dtype=np.float64):
    """(src, dst, s [E, width]) with ``s = k_dst + q_src`` in ``dtype``: the destination's key meets the source's query."""
    coo = np.asarray(coo).reshape(-1, 2)
    src, dst = coo[:, 0], coo[:, 1]
    return src, dst, (np.asarray(k, dtype)[dst] + np.asarray(q, dtype)[src]).astype(dtype)


def gates(s):
    """``1 / (1 + exp(-s))`` in ``s``'s dtype; ``exp`` overflows to inf without a warning and the gate is then exactly 0."""
    with np.errstate(over="ignore"):
        return (s.dtype.type(1) / (s.dtype.type(1) + np.exp(-s))).astype(s.dtype)


def resgated_ref(k, q, v, root, skip, act, coo, dtype=np.float64):
    """``act((sum_j sigmoid(k_i + q_j) * v_j + root_i) + skip_i)`` [N, width] in ``dtype``: the neighbours added with
    ``np.add.at`` in COO order per destination (sequential), ``root`` and ``skip`` last.  ``dtype=np.float32`` is ``base``.  A
    row without in-edges is ``act(root_i + skip_i)``."""
    src, dst, s = gate_arguments(k, q, coo, dtype)
    out = np.zeros(np.asarray(k).shape, dtype)
    np.add.at(out, dst, (gates(s) * np.asarray(v, dtype)[src]).astype(dtype))
    if root is not None:
        out = out + np.asarray(root, dtype)
    if skip is not None:
        out = out + np.asarray(skip, dtype)
    return _act(out.astype(dtype), act)


# ---- the stage's operands on dyadic grids.  k and q are multiples of 1/4 in [-2, 2]: k_i + q_j is a multiple of 1/4 in [-4, 4],
# exact in fp32 and float64, and the gates lie in [0.01799, 0.98201] ("flat").  "steep": k and q times 64 -- still exact, arguments up
# to +-256 --, so exp overflows and the gates reach exactly 0 and exactly 1 in fp32.  v, root and skip are multiples of 1/16 in
# [-1, 1].  (+ 0.0: no -0 among the operands, so that 0 + root is root to the bit.)
def _grid(rng, shape, step, span):
    return (np.round(rng.uniform(-span, span, shape) / step) * step).astype(np.float32) + np.float32(0)


def stage_case(num_nodes, width, kind):
    """dict of k, q, v, root, skip [N, width] (fp32) for operand set ``kind`` ("flat" / "steep")."""
    rng = np.random.default_rng(1000 * width + 7)
    scale = np.float32(1.0 if kind == "flat" else 64.0)
    return dict(k=_grid(rng, (num_nodes, width), 0.25, 2.0) * scale, q=_grid(rng, (num_nodes, width), 0.25, 2.0) * scale,
                v=_grid(rng, (num_nodes, width), 1 / 16, 1.0), root=_grid(rng, (num_nodes, width), 1 / 16, 1.0),
                skip=_grid(rng, (num_nodes, width), 1 / 16, 1.0))
