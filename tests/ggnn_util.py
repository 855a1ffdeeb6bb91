"""Shared builders of the GatedGraphConv tests: a seeded ``GNNModel`` of ``GatedGraphConv_GNNB`` layers, the float64 restatement
of one step behind its GEMM (``ggnn_ref``: numpy, nothing taken from models.py), and the stage's operands on dyadic grids on
which every sum of ``p_j`` and every r and z argument is exact in fp32."""
import numpy as np
import torch

import gnnbuilder_amd as gnnb
from helpers import ACTS

WIDTHS = [32, 9, 130, 24, 256, 1]  # both forms, one and several strides, an odd width, the cap, and width 1
FAULTS = ("bias_per_edge", "swap_rz", "h_shift", "r_on_gi")


def make_ggnn_model(in_dim=9, hidden=32, layers=3, out_dim=None, steps=1, act="relu", skip=True, pools=("add", "mean", "max"),
                    mlp_hidden=64, mlp_layers=2, task_out=19, out_act=None, seed=0):
    torch.manual_seed(seed)
    out_dim = hidden if out_dim is None else out_dim
    model = gnnb.GNNModel(in_dim, None, hidden, layers, out_dim, gnnb.GatedGraphConv_GNNB, ACTS[act], skip,
                          gnnb.GlobalPooling(list(pools)), gnnb.MLP(len(pools) * out_dim, task_out, mlp_hidden, mlp_layers), out_act,
                          gnn_steps=steps)
    return model.eval()


def _act(v, act):
    if act == "none":
        return v
    if act == "relu":
        return np.maximum(v, v.dtype.type(0))
    t = torch.from_numpy(np.ascontiguousarray(v))
    return {"gelu": torch.nn.functional.gelu, "sigmoid": torch.sigmoid, "tanh": torch.tanh}[act](t).numpy()


def sigmoid(s):
    """``1 / (1 + exp(-s))`` in ``s``'s dtype; ``exp`` overflows to inf without a warning and the gate is then exactly 0."""
    with np.errstate(over="ignore"):
        return (s.dtype.type(1) / (s.dtype.type(1) + np.exp(-s))).astype(s.dtype)


def pad_h(h, width, dtype):
    """``h`` [N, h_width] with zero columns up to ``width``."""
    h = np.asarray(h, dtype)
    return np.concatenate([h, np.zeros((h.shape[0], width - h.shape[1]), dtype)], 1)


def neighbour_sums(p, coo, dtype=np.float64):
    """``sum_{j in N(i)} p_j`` [N, 3 width] in ``dtype``: ``np.add.at`` in COO order per destination (sequential)."""
    coo = np.asarray(coo).reshape(-1, 2)
    acc = np.zeros(np.asarray(p).shape, dtype)
    np.add.at(acc, coo[:, 1], np.asarray(p, dtype)[coo[:, 0]])
    return acc


def gate_arguments(p, gh, b_ih, coo, dtype=np.float64):
    """(r argument, z argument) [N, width] each in ``dtype``: ``(acc_g + b_ih[g]) + gh_g``."""
    w = np.asarray(p).shape[1] // 3
    gi = neighbour_sums(p, coo, dtype)
    if b_ih is not None:
        gi = gi + np.asarray(b_ih, dtype)[None, :]
    gh = np.asarray(gh, dtype)
    return (gi[:, :w] + gh[:, :w]).astype(dtype), (gi[:, w:2 * w] + gh[:, w:2 * w]).astype(dtype)


def ggnn_ref(p, gh, h, b_ih, skip, act, coo, dtype=np.float64, fault=None):
    """One GatedGraphConv step behind its GEMM, [N, width] in ``dtype``: ``gi = sum_j p_j + b_ih``, ``r = sigmoid(gi_r + gh_r)``,
    ``z = sigmoid(gi_z + gh_z)``, ``n = tanh(gi_n + r * gh_n)``, ``act(n + z * (h - n) + skip)``; ``h`` [N, h_width] is padded
    with zero columns.  ``dtype=np.float32`` is ``base``.  ``fault``: one of ``FAULTS``, a wrong kernel restated -- ``bias_ih``
    added once per edge, r and z swapped, ``h`` laid out at the full width without its padding (its columns shifted), ``r``
    applied to ``gi_n`` instead of ``gh_n``."""
    coo = np.asarray(coo).reshape(-1, 2)
    p = np.asarray(p, dtype)
    n_rows, w = p.shape[0], p.shape[1] // 3
    gi = neighbour_sums(p, coo, dtype)
    if b_ih is not None:
        b = np.asarray(b_ih, dtype)[None, :]
        if fault == "bias_per_edge":
            gi = (gi + np.bincount(coo[:, 1], minlength=n_rows).astype(dtype)[:, None] * b).astype(dtype)
        else:
            gi = gi + b
    gh = np.asarray(gh, dtype)
    hp = pad_h(h, w, dtype)
    if fault == "h_shift":  # (rows of h_width floats read at stride width, nothing padded: the columns land elsewhere)
        flat = np.concatenate([np.asarray(h, dtype).ravel(), np.zeros(n_rows * w, dtype)])
        hp = flat[:n_rows * w].reshape(n_rows, w)
    blocks = (1, 0, 2) if fault == "swap_rz" else (0, 1, 2)
    ir, iz, inn = (slice(b * w, (b + 1) * w) for b in blocks)
    r = sigmoid((gi[:, ir] + gh[:, ir]).astype(dtype))
    z = sigmoid((gi[:, iz] + gh[:, iz]).astype(dtype))
    arg = r * gi[:, inn] + gh[:, inn] if fault == "r_on_gi" else gi[:, inn] + r * gh[:, inn]
    n = np.tanh(arg.astype(dtype))
    out = n + z * (hp - n)
    if skip is not None:
        out = out + np.asarray(skip, dtype)
    return _act(out.astype(dtype), act)


# ---- the stage's operands on dyadic grids.  p, b_ih, h and skip are multiples of 1/16 in [-1, 1], gh multiples of 1/4 in
# [-2, 2]: a sum of up to 2^19 rows of p is exact in fp32, and so is every r and z argument (acc + b_ih) + gh ("flat").  "steep":
# p_r, p_z, gh_r, gh_z and the terms of the tanh argument (p_n, b_ih_n, gh_n) times 64 -- still exact --, so the gates reach
# exactly 0 and exactly 1 and the tanh exactly +-1 in fp32.  (+ 0.0: no -0 among the operands.)
def _grid(rng, shape, step, span):
    return (np.round(rng.uniform(-span, span, shape) / step) * step).astype(np.float32) + np.float32(0)


def stage_case(num_nodes, width, h_width, kind):
    """dict of p, gh [N, 3 width], h [N, h_width], b_ih [3 width], skip [N, width] (fp32) for operand set ``kind`` ("flat" /
    "steep")."""
    rng = np.random.default_rng(1000 * width + 10 * h_width + 7)
    scale = np.float32(1.0 if kind == "flat" else 64.0)
    b_ih = _grid(rng, (3 * width,), 1 / 16, 1.0)
    b_ih[2 * width:] *= scale
    return dict(p=_grid(rng, (num_nodes, 3 * width), 1 / 16, 1.0) * scale, gh=_grid(rng, (num_nodes, 3 * width), 0.25, 2.0) * scale,
                h=_grid(rng, (num_nodes, h_width), 1 / 16, 1.0), b_ih=b_ih, skip=_grid(rng, (num_nodes, width), 1 / 16, 1.0))


def arguments_are_exact(c, coo):
    """Asserts -- on the reference alone -- that every neighbour sum and every r and z argument of case ``c`` is exact in fp32;
    returns the fp32 (r argument, z argument)."""
    a32, a64 = neighbour_sums(c["p"], coo, np.float32), neighbour_sums(c["p"], coo, np.float64)
    assert a32.dtype == np.float32 and np.array_equal(a32.astype(np.float64), a64)
    r32, z32 = gate_arguments(c["p"], c["gh"], c["b_ih"], coo, np.float32)
    r64, z64 = gate_arguments(c["p"], c["gh"], c["b_ih"], coo, np.float64)
    assert r32.dtype == np.float32 and np.array_equal(r32.astype(np.float64), r64) and np.array_equal(z32.astype(np.float64), z64)
    return r32, z32
