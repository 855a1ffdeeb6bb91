"""A float64 reference of every forward route, and the acceptance rule the precision tests apply with it.

``forward64`` evaluates the package's own PyTorch model (``models.py`` is plain torch and runs in any dtype) on a float64
copy; ``layer64`` / ``pool64`` are its stage entry points.  GINE / Simple / LGConv have no ``GNNModel`` form: ``gine64``,
``simple64`` and ``lg64`` restate the oracle's formulas in float64 numpy.

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
    out = np.zeros((n, x.shape[1]), np.float64)
    msg = x[src] if scale is None else x[src] * scale[:, None]
    np.add.at(out, dst, msg)
    return out


def simple64(x, coo):
    """SimpleConv (sum aggregation): ``sum_j x_j``."""
    x = np.asarray(x, np.float64)
    return _csr_sums(x, coo, x.shape[0])


def lg64(x, coo):
    """LGConv: ``sum_j x_j / sqrt(d_i d_j)`` with d = in-degree (every edge, self loops included), no self term."""
    x = np.asarray(x, np.float64)
    src, dst = np.asarray(coo).reshape(-1, 2).T
    deg = np.bincount(dst, minlength=x.shape[0]).astype(np.float64)
    prod = deg[dst] * deg[src]
    s = np.where(prod > 0, 1.0 / np.sqrt(np.maximum(prod, 1.0)), 0.0)
    return _csr_sums(x, coo, x.shape[0], s)


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
