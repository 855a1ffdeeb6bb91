"""Shared builders of the PNA-with-edge-features tests: a seeded ``GNNModel`` of ``PNAEConv_GNNB`` layers, grids on which every
message of the stage kernel is exact in fp32, the stage's float64 restatement, and an independent per-edge restatement of the
whole conv.  The layer walk of a whole model (``run`` / ``forward64``) is ``gine_util``'s: it hands ``edge_attr`` to every conv."""
import numpy as np
import torch

import gnnbuilder_amd as gnnb
import ref64 as R
from helpers import ACTS


def make_pnae_model(in_dim=9, edge_dim=3, hidden=32, layers=3, out_dim=None, act="relu", skip=True, pools=("add", "mean", "max"),
                    mlp_hidden=64, mlp_layers=2, task_out=19, out_act=None, seed=0):
    torch.manual_seed(seed)
    out_dim = hidden if out_dim is None else out_dim
    model = gnnb.GNNModel(in_dim, edge_dim, hidden, layers, out_dim, gnnb.PNAEConv_GNNB, ACTS[act], skip,
                          gnnb.GlobalPooling(list(pools)), gnnb.MLP(len(pools) * out_dim, task_out, mlp_hidden, mlp_layers), out_act)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("bias"):
                p.uniform_(-0.1, 0.1)
    return model.eval()


def pnae_conv64(x, coo, edge_attr, w, delta):
    """One ``PNAEConv_GNNB`` layer restated edge by edge in float64 numpy, with nothing taken from models.py: explicit concat,
    pre-NN, the four statistics per destination in a Python loop, PyG's std, the three scalers, post-NN, ``lin``.
    ``w``: dict of the layer's ``state_dict`` arrays (keys without the ``conv.`` prefix)."""
    w = {k: np.asarray(v, np.float64) for k, v in w.items()}
    x, ea = np.asarray(x, np.float64), np.asarray(edge_attr, np.float64)
    coo = np.asarray(coo).reshape(-1, 2)
    n, f = x.shape
    msgs = [[] for _ in range(n)]
    for (s, d), e in zip(coo, ea):
        enc = w["edge_encoder.weight"] @ e + w["edge_encoder.bias"]
        msgs[d].append(w["pre_nns.0.0.weight"] @ np.concatenate([x[d], x[s], enc]) + w["pre_nns.0.0.bias"])  # destination first
    out = np.zeros((n, w["lin.weight"].shape[0]))
    for i in range(n):
        agg = np.zeros(4 * f)
        deg = len(msgs[i])
        if deg:
            h = np.stack(msgs[i])
            mean = h.sum(0) / deg
            var = (h * h).sum(0) / deg - mean * mean
            std = np.sqrt(np.maximum(var, 1e-5))
            std[std <= np.sqrt(1e-5)] = 0.0
            agg = np.concatenate([h.max(0), h.min(0), mean, std])
        logd = np.log(max(deg, 1) + 1.0)
        cat = np.concatenate([x[i], agg, agg * (logd / delta), agg * (delta / logd)])
        out[i] = w["lin.weight"] @ (w["post_nns.0.0.weight"] @ cat + w["post_nns.0.0.bias"]) + w["lin.bias"]
    return out


# ---- the stage kernel's operands on grids: x and edge_attr on multiples of 1/4 in [-1, 1], W_b and W_e on multiples of 1/16 in
# [-1/2, 1/2], b_e and q on multiples of 1/16 in [-1, 1].  p_j = W_b x_j is then a multiple of 1/64 below 2^9 and every message
# q_i + p_j + W_e e + b_e a multiple of 1/64 below 2^10: 16 significant bits, exact in fp32 and float64 in any summation order.
def _grid(rng, shape, step, span):
    return (np.round(rng.uniform(-span, span, shape) / step) * step).astype(np.float32)


def stage_case(batch, width, edge_dim):
    """Grid operands for ``batch``, drawn from ``default_rng(width)``: dict of x [N, width], wb [width, width], p = x wb^T (exact),
    q [N, width], ea [E, edge_dim], we [width, edge_dim], be [width]."""
    rng = np.random.default_rng(width)
    x = _grid(rng, (batch.num_nodes, width), 0.25, 1.0)
    wb = _grid(rng, (width, width), 1 / 16, 0.5)
    c = dict(x=x, wb=wb, p=(x.astype(np.float64) @ wb.astype(np.float64).T).astype(np.float32),
             q=_grid(rng, (batch.num_nodes, width), 1 / 16, 1.0), ea=_grid(rng, (batch.num_edges, edge_dim), 0.25, 1.0),
             we=_grid(rng, (width, edge_dim), 1 / 16, 0.5), be=_grid(rng, (width,), 1 / 16, 1.0))
    assert np.array_equal(c["p"].astype(np.float64), x.astype(np.float64) @ wb.astype(np.float64).T)
    return c


def stage_messages(coo, c, q, dtype):
    """h_ij [E, width] in ``dtype``, in the kernel's order of operations: (W_e e + b_e + p_j) + q_i."""
    src, dst = np.asarray(coo).reshape(-1, 2).T
    t = c["ea"].astype(dtype) @ c["we"].astype(dtype).T + c["be"].astype(dtype)
    h = t + c["p"].astype(dtype)[src]
    return h + q.astype(dtype)[dst] if q is not None else h


def stage_ref(coo, num_nodes, h):
    """max | min | mean | std of the messages ``h`` [E, width] per destination, in ``h``'s dtype: ``ref64.pna_agg64``'s formulas on
    per-edge messages (sums in COO order per destination = CSR slot order).  Returns (out [N, 4 width], var [N, width], deg)."""
    dtype = h.dtype.type
    dst = np.asarray(coo).reshape(-1, 2)[:, 1]
    n, w = num_nodes, h.shape[1]
    deg = np.bincount(dst, minlength=n)[:n]
    s1, s2 = np.zeros((n, w), dtype), np.zeros((n, w), dtype)
    np.add.at(s1, dst, h)
    np.add.at(s2, dst, h * h)
    mx, mn = np.full((n, w), -np.inf, dtype), np.full((n, w), np.inf, dtype)
    np.maximum.at(mx, dst, h)
    np.minimum.at(mn, dst, h)
    has = (deg > 0)[:, None]
    d = np.maximum(deg, 1).astype(dtype)[:, None]
    mean = s1 / d
    var = s2 / d - mean * mean
    sd = np.sqrt(np.maximum(var, dtype(R.PNA_STD_EPS)))
    sd = np.where(sd <= np.sqrt(dtype(R.PNA_STD_EPS)), dtype(0), sd)
    z = dtype(0)
    out = np.concatenate([np.where(has, mx, z), np.where(has, mn, z), np.where(has, mean, z), np.where(has, sd, z)], 1).astype(dtype)
    return out, np.where(has, var, z), deg


def layer_variances(model, batch, x, edge_attr):
    """Per layer of a float64 copy of ``model``: (var [N, F] of the messages per (node, column), max_j h_ij^2 [N, F]) on the rows
    that have in-edges -- what decides which side of PyG's 1e-5 threshold a std falls."""
    import copy
    m = copy.deepcopy(model).double()
    ei = R.edge_index(batch.coo)
    h = torch.from_numpy(np.ascontiguousarray(x)).double()
    ea = torch.from_numpy(np.ascontiguousarray(edge_attr)).double()
    dst = ei[1].numpy()
    out = []
    with torch.no_grad():
        for i, (conv, act) in enumerate(zip(m.gnn_convs, m.gnn_activations)):
            msg = conv.conv.message(h, ei, ea).numpy()
            n, w = h.shape[0], msg.shape[1]
            deg = np.bincount(dst, minlength=n)[:n]
            s1, s2, hi = np.zeros((n, w)), np.zeros((n, w)), np.zeros((n, w))
            np.add.at(s1, dst, msg)
            np.add.at(s2, dst, msg * msg)
            np.maximum.at(hi, dst, msg * msg)
            has = deg > 0
            d = np.maximum(deg, 1)[:, None]
            out.append(((s2 / d - (s1 / d) ** 2)[has], hi[has]))
            h_in = h
            h = conv(h, ei, ea)
            if m.gnn_skip_connection and i != 0 and i != m.gnn_num_layers - 1:
                h = h + h_in
            h = act(h)
    return out
