"""A float64 reference of every forward route, and the acceptance rule the precision tests apply with it.

``forward64`` evaluates the package's own PyTorch model (``models.py`` is plain torch and runs in any dtype) on a float64
copy; ``layer64`` / ``pool64`` are its stage entry points.  GINE / Simple / LGConv have no ``GNNModel`` form: ``gine64``,
``simple64`` and ``lg64`` restate the oracle's formulas in float64 numpy.

The stage entry points (``gnnb_aggregate``, ``gnnb_linear``, ...) have float64 restatements of their own: ``gcn_agg64``,
``sum_agg64``, ``mean_agg64``, ``pna_agg64``, ``simple64``, ``lg64`` (``gnnb_hip.h`` ``gnnb_agg``) and ``linear64``.  Each takes
a ``dtype``: float32 gives the fp32 evaluation the budget measures against -- neighbours summed in CSR order (COO order per
destination: ``np.add.at`` is sequential), the self term last, as the kernels do.  ``workspace_edges`` applies the documented
self-loop rule (``gnnb_hip.h``, ``gnnb_graph_prep``): the tables of a GCN workspace hold no explicit ``(v, v)`` edge.
``agg_rows64`` and ``linear64(rows=...)`` give chosen rows only, for batches of millions of nodes.

``budget(got, ref, base)`` asks a result to be as accurate as a plain fp32 evaluation of the same model: with
``s = max|ref|``, ``e = max|got - ref| / s`` and ``e32 = max|base - ref| / s`` (``base``: the fp32 oracle's output for the
same inputs) it accepts ``e <= K * e32 + F``.  K and F are calibrated on the MI355X.
"""
import copy

import numpy as np
import torch

from helpers import batch_vector

K = 4.0
F = 2.0 ** -22


def _t(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def edge_index(coo):
    """[E, 2] (src, dst) rows -> PyG int64 [2, E]."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(coo).reshape(-1, 2).T).astype(np.int64))


def run(model, batch, x, coo=None):
    """The whole model as it stands (its own dtype, no copy): conv stack, pooling of every graph of the batch (trailing
    empty graphs included), MLP head, output activation.  ``coo`` replaces the batch's edges (fault tests)."""
    dtype = next(model.parameters()).dtype
    ei = edge_index(batch.coo if coo is None else coo)
    h = _t(x, dtype)
    with torch.no_grad():
        for i, (conv, act) in enumerate(zip(model.gnn_convs, model.gnn_activations)):
            h_in = h
            h = conv(h, ei)
            if model.gnn_skip_connection and i != 0 and i != model.gnn_num_layers - 1:
                h = h + h_in
            h = act(h)
        pooled = model.global_pooling(h, torch.from_numpy(batch_vector(batch)), batch.num_graphs)
        out = model.mlp_head(pooled)
        if model.output_activation_module is not None:
            out = model.output_activation_module(out)
    return out.numpy()


def forward64(model, batch, x, coo=None):
    """``model`` (a ``GNNModel``) evaluated in float64 on ``x`` and the batch's graphs; numpy [B, out]."""
    return run(copy.deepcopy(model).double(), batch, x, coo)


def layer64(conv, x, coo):
    """One conv module (``GCNConv_GNNB`` ...) in float64 on ``x`` [N, F]; numpy [N, out]."""
    with torch.no_grad():
        return copy.deepcopy(conv).double()(_t(x), edge_index(coo)).numpy()


def pool64(h, batch, pools):
    """Global pooling (``add`` / ``mean`` / ``max`` concatenated) of node rows ``h`` in float64; numpy [B, k*d]."""
    from gnnbuilder_amd import GlobalPooling
    with torch.no_grad():
        return GlobalPooling(list(pools))(_t(h), torch.from_numpy(batch_vector(batch)), batch.num_graphs).numpy()


def _csr_sums(x, coo, n, scale=None):
    src, dst = np.asarray(coo).reshape(-1, 2).T
    out = np.zeros((n, x.shape[1]), x.dtype)
    msg = x[src] if scale is None else x[src] * scale[:, None]
    np.add.at(out, dst, msg)
    return out


def workspace_edges(coo, gcn_workspace):
    """The edges a workspace's tables hold: a GCN workspace drops every explicit self loop (``gnnb_graph_prep``)."""
    coo = np.asarray(coo).reshape(-1, 2)
    return coo[coo[:, 0] != coo[:, 1]] if gcn_workspace else coo


def _in_deg(coo, n):
    return np.bincount(np.asarray(coo).reshape(-1, 2)[:, 1], minlength=n)[:n]


def simple64(x, coo, dtype=np.float64):
    """SimpleConv (sum aggregation): ``sum_j x_j``."""
    x = np.asarray(x, dtype)
    return _csr_sums(x, coo, x.shape[0])


def lg64(x, coo, dtype=np.float64):
    """LGConv: ``sum_j x_j / sqrt(d_i d_j)`` with d = in-degree (every edge, self loops included), no self term."""
    x = np.asarray(x, dtype)
    src, dst = np.asarray(coo).reshape(-1, 2).T
    deg = _in_deg(coo, x.shape[0]).astype(dtype)
    prod = deg[dst] * deg[src]
    s = np.where(prod > 0, dtype(1) / np.sqrt(np.maximum(prod, dtype(1))), dtype(0)).astype(dtype)
    return _csr_sums(x, coo, x.shape[0], s)


def gcn_agg64(x, coo, dtype=np.float64, deg=None):
    """PyG ``gcn_norm`` aggregate with exactly one self loop per node: ``sum_j x_j / sqrt(d_i d_j) + x_i / d_i``,
    d = 1 + in-degree over ``coo`` (pass ``workspace_edges(coo, True)`` for a GCN workspace: its explicit self loops are
    replaced, not counted; on any other workspace they are ordinary edges).  ``deg``: the in-degrees, where ``coo`` holds only
    part of the edges (``agg_rows64``)."""
    x = np.asarray(x, dtype)
    src, dst = np.asarray(coo).reshape(-1, 2).T
    deg = _in_deg(coo, x.shape[0]) if deg is None else deg
    dinv = (dtype(1) / np.sqrt(deg.astype(dtype) + dtype(1))).astype(dtype)
    out = _csr_sums(x, coo, x.shape[0], (dinv[dst] * dinv[src]).astype(dtype))
    return out + x * (dinv * dinv)[:, None]


def sum_agg64(x, coo, eps=0.0, dtype=np.float64):
    """GIN's aggregate: ``sum_j x_j + (1 + eps) x_i`` (``1 + eps`` formed in fp32, as the kernels take ``eps``)."""
    x = np.asarray(x, dtype)
    return _csr_sums(x, coo, x.shape[0]) + x * dtype(np.float32(1) + np.float32(eps))


def mean_agg64(x, coo, dtype=np.float64, deg=None):
    """SAGE's aggregate: ``mean_j x_j``, 0 without a neighbour."""
    x = np.asarray(x, dtype)
    deg = (_in_deg(coo, x.shape[0]) if deg is None else deg).astype(dtype)
    return _csr_sums(x, coo, x.shape[0]) / np.maximum(deg, dtype(1))[:, None]


def gine_agg64(x, coo, edge_term, eps=0.0, dtype=np.float64):
    """GINE's aggregate (``gnnb_aggregate_edges``): ``(1 + eps) x_i + sum_j relu(x_j + edge_term[e])``, ``edge_term`` [E, w]
    in COO order."""
    x = np.asarray(x, dtype)
    src, dst = np.asarray(coo).reshape(-1, 2).T
    out = np.zeros_like(x)
    np.add.at(out, dst, np.maximum(x[src] + np.asarray(edge_term, dtype), dtype(0)))
    return out + x * dtype(np.float32(1) + np.float32(eps))


def agg_rows64(kind, coo, num_nodes, rows, fetch, eps=0.0, dtype=np.float64):
    """Rows ``rows`` (unique node ids) of ``gcn_agg64`` / ``sum_agg64`` / ``mean_agg64`` / ``simple64`` (``kind`` gcn / sum /
    mean / simple) over a graph of ``num_nodes`` nodes, reading only the features they need: ``fetch(ids)`` returns the rows
    ``ids`` (increasing) of x.  The same operations in the same order as the full form -- the rows' in-edges in COO order,
    in-degrees over every edge -- so the values are identical to the full form's at those rows."""
    rows = np.asarray(rows, np.int64)
    src, dst = np.asarray(coo).reshape(-1, 2).T
    pos = np.full(num_nodes, -1, np.int64)
    pos[rows] = np.arange(len(rows))
    assert len(np.unique(rows)) == len(rows)
    sel = pos[dst] >= 0
    need = np.unique(np.concatenate([rows, src[sel]]))
    loc = lambda ids: np.searchsorted(need, ids)  # noqa: E731
    lcoo = np.stack([loc(src[sel]), loc(dst[sel])], 1)
    x = np.asarray(fetch(need))
    assert x.shape[0] == len(need)
    if kind == "gcn":
        out = gcn_agg64(x, lcoo, dtype, deg=_in_deg(coo, num_nodes)[need])
    elif kind == "mean":
        out = mean_agg64(x, lcoo, dtype)
    elif kind == "sum":
        out = sum_agg64(x, lcoo, eps, dtype)
    else:
        assert kind == "simple", kind
        out = simple64(x, lcoo, dtype)
    return out[loc(rows)]


PNA_STD_EPS = 1e-5


def pna_agg64(x, coo, q=None, dtype=np.float64, clamp=True):
    """PNA's aggregate ``[max | min | mean | std]_j (q_i + x_j)`` ([N, 4w]); ``q`` None: no destination term.  PyG's std:
    ``sqrt(max(E[h^2] - E[h]^2, 1e-5))``, 0 where that is <= ``sqrt(1e-5)``; in-degree 0 gives 0 everywhere.
    ``clamp=False`` is the fault the tests inject (the plain ``sqrt(max(var, 0))``)."""
    x = np.asarray(x, dtype)
    n, w = x.shape
    src, dst = np.asarray(coo).reshape(-1, 2).T
    h = x[src] + (np.asarray(q, dtype)[dst] if q is not None else dtype(0))
    deg = _in_deg(coo, n)
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
    if clamp:
        sd = np.sqrt(np.maximum(var, dtype(PNA_STD_EPS)))
        sd = np.where(sd <= np.sqrt(dtype(PNA_STD_EPS)), dtype(0), sd)
    else:
        sd = np.sqrt(np.maximum(var, dtype(0)))
    z = dtype(0)
    return np.concatenate([np.where(has, mx, z), np.where(has, mn, z), np.where(has, mean, z), np.where(has, sd, z)], 1).astype(dtype)


ACTS64 = {"none": lambda v: v, "relu": lambda v: torch.relu(v), "tanh": torch.tanh, "sigmoid": torch.sigmoid,
          "gelu": lambda v: torch.nn.functional.gelu(v)}


def linear64(segments, weight, bias=None, skip=None, act="none", dtype=torch.float64, rows=None):
    """``gnnb_linear``: ``act(sum_s (rowscale_s * A_s) . W[:, koff_s : koff_s + K_s]^T + bias + skip)``.  ``segments``:
    (A [M, K_s], rowscale [M] or None) tensors or arrays, any strides; float32 ``dtype`` is the torch CPU fp32 product, its
    4-column chunks summed in K order (one BLAS call over the whole K would sum more accurately than any GPU kernel, and
    differently on every CPU).  ``rows``: only those rows of the result (A, rowscale and skip are indexed first: a device
    tensor of any size gives up just those rows)."""
    if rows is not None:
        r = torch.as_tensor(np.asarray(rows, np.int64))
        pick = lambda a: None if a is None else (a[r.to(a.device)].cpu() if torch.is_tensor(a) else np.asarray(a)[np.asarray(rows)])  # noqa: E731
        segments = [(pick(a), pick(rs)) for a, rs in segments]
        skip = pick(skip)
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)  # noqa: E731
    w = t(weight)
    acc, koff = None, 0
    for a, rs in segments:
        a = t(a)
        if rs is not None:
            a = a * t(rs)[:, None]
        for c in range(0, a.shape[1], 4):  # (fp32: 4-column chunks accumulated in order, as the kernels' MFMA K steps)
            p = a[:, c:c + 4] @ w[:, koff + c:koff + min(c + 4, a.shape[1])].T
            acc = p if acc is None else acc + p
        koff += a.shape[1]
    if bias is not None:
        acc = acc + t(bias)
    if skip is not None:
        acc = acc + t(skip)
    return ACTS64[act](acc).numpy()


def gine64(x, coo, edge_attr, weights, eps=0.0):
    """GINEConv: ``W1 relu(W0 ((1 + eps) x_i + sum_j relu(x_j + We e_ij + be)) + b0) + b1``; ``weights`` =
    [We, be, W0, b0, W1, b1] as the oracle takes them."""
    we, be, w0, b0, w1, b1 = (np.asarray(w, np.float64) for w in weights)
    x = np.asarray(x, np.float64)
    src, dst = np.asarray(coo).reshape(-1, 2).T
    msg = np.maximum(x[src] + np.asarray(edge_attr, np.float64) @ we.T + be, 0.0)
    agg = np.zeros_like(x)
    np.add.at(agg, dst, msg)
    z = (1.0 + np.float64(np.float32(eps))) * x + agg
    return np.maximum(z @ w0.T + b0, 0.0) @ w1.T + b1


def errors(got, ref, base):
    """(e, e32, index of the worst element of ``got``) relative to ``s = max|ref|`` (1 for an all-zero reference)."""
    got, ref, base = (np.asarray(a, np.float64) for a in (got, ref, base))
    assert got.shape == ref.shape == base.shape, (got.shape, ref.shape, base.shape)
    if ref.size == 0:
        return 0.0, 0.0, ()
    s = float(np.abs(ref).max()) or 1.0
    d = np.abs(got - ref)
    d = np.where(np.isnan(d), np.inf, d)
    worst = np.unravel_index(int(np.argmax(d)), d.shape)
    return float(d[worst]) / s, float(np.abs(base - ref).max()) / s, tuple(int(i) for i in worst)


def budget(got, ref, base, k=K, f=F, what=""):
    """Assert ``e <= k * e32 + f`` (module docstring); returns ``(e, e32)``."""
    e, e32, worst = errors(got, ref, base)
    limit = k * e32 + f
    assert e <= limit, (f"{what + ': ' if what else ''}e = {e:.3e} > {k:g} * e32 + {f:.2e} = {limit:.3e} "
                        f"(e32 = {e32:.3e}, e/e32 = {e / max(e32, 1e-300):.2f}; worst element {worst}: "
                        f"got {np.asarray(got)[worst]!r}, float64 {np.asarray(ref)[worst]!r})")
    return e, e32


def ratio(e, e32):
    """``e / e32`` with the same floor the budget has (``F / K``), for reporting."""
    return e / max(e32, F / K)


def round_bits(a, bits):
    """``a`` (float64 tensor or array) rounded to ``bits`` significant bits (round to nearest)."""
    m, ex = np.frexp(np.asarray(a, np.float64))
    return np.ldexp(np.round(m * 2.0 ** bits) / 2.0 ** bits, ex)
