"""Model API of the MI355X backend -- counterpart of the reference's ``gnnbuilder/models.py``.

Same classes, constructor arguments, attribute names and ``state_dict`` parameter names as the
reference, so a user script (or a checkpoint) written against ``gnnbuilder.models`` keeps working.
The reference builds its conv layers on ``torch_geometric``; this package has no such dependency:
each conv is written here directly in PyTorch tensor ops (``index_add_`` / ``scatter_reduce``)
with the module layout PyG uses, so parameter names match
(``conv.lin.weight``, ``mlp.linear_0.weight``, ``conv.lin_l.weight``, ``conv.pre_nns.0.0.weight`` ...).

Role split (same as the reference): ``GNNModel.forward`` is the *model definition* in PyTorch --
what a user trains, and what ``Project.gen_testbench_data`` records as the golden output
(reference ``code_gen.py:279-285``).  The accelerated path is ``Project`` / ``runtime.CompiledModel``
(hand-written HIP behind the C ABI); it never dispatches back to this file.

Semantics follow SURVEY.md Appendix A, each checked against the reference's PyG golden vectors
in ``tests/test_models_torch.py``.
"""
from __future__ import annotations

import math
from typing import Callable, List, Optional

import torch
import torch.nn as nn
from torch import Tensor

from .utils import layer_param_name_combiner

TorchModuleArg = Callable[..., torch.nn.Module]
TorchModuleArgOptional = Optional[Callable[..., torch.nn.Module]]


def _in_degree(edge_index: Tensor, num_nodes: int) -> Tensor:
    deg = torch.zeros(num_nodes, dtype=torch.long, device=edge_index.device)
    if edge_index.numel():
        deg.index_add_(0, edge_index[1], torch.ones_like(edge_index[1]))
    return deg


def _glorot(w: Tensor) -> None:
    a = math.sqrt(6.0 / (w.size(-2) + w.size(-1)))
    with torch.no_grad():
        w.uniform_(-a, a)


# --------------------------------------------------------------------------------------- GCN
class _GCNConv(nn.Module):
    """``D^-1/2 (A+I) D^-1/2 X W^T + b`` with ``d_i = 1 + indeg(i)`` (reference models.py:41;
    native restatement gnn_builder_lib.h:1213-1387).  Parameters: ``bias``, ``lin.weight``."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.lin = nn.Linear(in_channels, out_channels, bias=False)
        self.bias = nn.Parameter(torch.zeros(out_channels))
        _glorot(self.lin.weight)

    def forward(self, x: Tensor, edge_index: Tensor) -> Tensor:
        n = x.size(0)
        # PyG gcn_norm -> add_remaining_self_loops: the input's explicit self loops are REPLACED by exactly one
        # self loop per node, so an edge (v, v) neither adds a message nor raises the degree
        if edge_index.numel():
            edge_index = edge_index[:, edge_index[0] != edge_index[1]]
        src, dst = edge_index[0], edge_index[1]
        dinv = (_in_degree(edge_index, n).to(x.dtype) + 1.0).pow(-0.5)
        h = self.lin(x)
        out = h * (dinv * dinv).unsqueeze(-1)
        if src.numel():
            out = out.index_add(0, dst, h[src] * (dinv[src] * dinv[dst]).unsqueeze(-1))
        return out + self.bias


class GCNConv_GNNB(nn.Module):
    def __init__(self, in_channels: int, out_channels: int, p_in: int = 1, p_out: int = 1):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.p_in = p_in
        self.p_out = p_out
        self.conv = _GCNConv(in_channels, out_channels)

    def forward(self, x: Tensor, edge_index: Tensor) -> Tensor:
        return self.conv(x, edge_index)


# --------------------------------------------------------------------------------------- GIN
class GIN_MLP(nn.Module):
    """Linear -> ReLU -> Linear (reference models.py:47-67)."""

    def __init__(self, in_dim: int, out_dim: int, hidden_dim: Optional[int] = None):
        super().__init__()
        self.in_dim = in_dim
        self.out_dim = out_dim
        self.hidden_dim = out_dim if hidden_dim is None else hidden_dim
        self.linear_0 = nn.Linear(self.in_dim, self.hidden_dim)
        self.linear_1 = nn.Linear(self.hidden_dim, self.out_dim)
        self.relu = nn.ReLU()
        self.in_features = self.in_dim

    def forward(self, x: Tensor) -> Tensor:
        return self.linear_1(self.relu(self.linear_0(x)))


class _GINConv(nn.Module):
    """``nn((1+eps) x_i + sum_j x_j)`` with a fixed eps (reference models.py:91)."""

    def __init__(self, mlp: nn.Module, eps: float = 0.0):
        super().__init__()
        self.nn = mlp
        self.register_buffer("eps", torch.tensor([float(eps)]))

    def forward(self, x: Tensor, edge_index: Tensor) -> Tensor:
        src, dst = edge_index[0], edge_index[1]
        agg = torch.zeros_like(x)
        if src.numel():
            agg = agg.index_add(0, dst, x[src])
        return self.nn(agg + (1.0 + self.eps) * x)


class GINConv_GNNB(nn.Module):
    def __init__(self, in_channels: int, out_channels: int, hidden_dim: Optional[int] = None,
                 eps: float = 0.0, p_in: int = 1, p_out: int = 1):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        # The reference stores the argument but always builds the MLP with hidden = out_channels
        # (models.py:84,90; SURVEY finding 6).  The emitter here reads ``mlp.hidden_dim``.
        self.hidden_dim = hidden_dim
        self.eps = eps
        self.p_in = p_in
        self.p_out = p_out
        self.mlp = GIN_MLP(in_channels, out_channels, None)
        self.conv = _GINConv(self.mlp, eps=eps)

    def forward(self, x: Tensor, edge_index: Tensor) -> Tensor:
        return self.conv(x, edge_index)


# --------------------------------------------------------------------------------------- SAGE
class _SAGEConv(nn.Module):
    """``W_l mean_j x_j + b_l + W_r x_i`` (reference models.py:259; lib:2161-2341)."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.lin_l = nn.Linear(in_channels, out_channels, bias=True)
        self.lin_r = nn.Linear(in_channels, out_channels, bias=False)

    def forward(self, x: Tensor, edge_index: Tensor) -> Tensor:
        n = x.size(0)
        src, dst = edge_index[0], edge_index[1]
        agg = torch.zeros_like(x)
        if src.numel():
            agg = agg.index_add(0, dst, x[src])
        deg = _in_degree(edge_index, n).clamp(min=1).to(x.dtype)
        return self.lin_l(agg / deg.unsqueeze(-1)) + self.lin_r(x)


class SAGEConv_GNNB(nn.Module):
    def __init__(self, in_channels: int, out_channels: int, p_in: int = 1, p_out: int = 1):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.p_in = p_in
        self.p_out = p_out
        self.conv = _SAGEConv(in_channels, out_channels)

    def forward(self, x: Tensor, edge_index: Tensor) -> Tensor:
        return self.conv(x, edge_index)


# --------------------------------------------------------------------------------------- PNA
class _DegreeScalerAggregation(nn.Module):
    def __init__(self, avg_deg_log: float):
        super().__init__()
        self.avg_deg_log = torch.Tensor([avg_deg_log])


class _PNAConv(nn.Module):
    """PNA with aggregators [max, min, mean, std] x scalers [identity, amplification,
    attenuation], towers=1, one pre and one post layer (reference models.py:227-234).
    ``std`` is PyG's: ``sqrt(clamp(E[h^2]-E[h]^2, 1e-5))`` zeroed where ``<= sqrt(1e-5)``
    (SURVEY finding 5, pinned by ``tb_pna_output.bin``)."""

    def __init__(self, in_channels: int, out_channels: int, avg_deg_log: float, pre_blocks: int = 2):
        super().__init__()
        self.aggr_module = _DegreeScalerAggregation(avg_deg_log)
        self.pre_nns = nn.ModuleList([nn.Sequential(nn.Linear(pre_blocks * in_channels, in_channels))])
        self.post_nns = nn.ModuleList([nn.Sequential(nn.Linear(13 * in_channels, out_channels))])
        self.lin = nn.Linear(out_channels, out_channels)

    def forward(self, x: Tensor, edge_index: Tensor) -> Tensor:
        src, dst = edge_index[0], edge_index[1]
        h = self.pre_nns[0](torch.cat([x[dst], x[src]], dim=-1))  # destination first
        return self.reduce(x, edge_index, h)

    def reduce(self, x: Tensor, edge_index: Tensor, h: Tensor) -> Tensor:
        """Everything behind the messages ``h`` [E, in]: the four aggregators, the scalers, post-NN and ``lin``."""
        n, f = x.size(0), x.size(1)
        src, dst = edge_index[0], edge_index[1]
        idx = dst.unsqueeze(-1).expand(-1, f)
        zeros = x.new_zeros(n, f)
        deg = _in_degree(edge_index, n)
        cnt = deg.clamp(min=1).to(x.dtype).unsqueeze(-1)
        if src.numel():
            mx = zeros.scatter_reduce(0, idx, h, "amax", include_self=False)
            mn = zeros.scatter_reduce(0, idx, h, "amin", include_self=False)
            s1 = zeros.index_add(0, dst, h)
            s2 = zeros.index_add(0, dst, h * h)
        else:
            mx = mn = s1 = s2 = zeros
        mean = s1 / cnt
        var = s2 / cnt - mean * mean
        std = var.clamp(min=1e-5).sqrt()
        std = std.masked_fill(std <= math.sqrt(1e-5), 0.0)
        has = (deg > 0).unsqueeze(-1)
        std = torch.where(has, std, zeros)
        agg = torch.cat([mx, mn, mean, std], dim=-1)
        delta = self.aggr_module.avg_deg_log.to(x.device, x.dtype)
        logd = torch.log(deg.clamp(min=1).to(x.dtype) + 1.0).unsqueeze(-1)
        out = torch.cat([x, agg, agg * (logd / delta), agg * (delta / logd)], dim=-1)
        return self.lin(self.post_nns[0](out))


class PNAConv_GNNB(nn.Module):
    def __init__(self, in_channels: int, out_channels: int, delta: float = 1.0, p_in: int = 1,
                 p_out: int = 1):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.delta = delta
        self.p_in = p_in
        self.p_out = p_out
        self.aggregators = ["max", "min", "mean", "std"]
        self.scalers = ["identity", "amplification", "attenuation"]
        # `delta` is used verbatim as avg_deg_log (reference models.py:236-237)
        self.conv = _PNAConv(in_channels, out_channels, float(delta))
        self.delta_scaler = self.conv.aggr_module.avg_deg_log.item()

    def forward(self, x: Tensor, edge_index: Tensor) -> Tensor:
        return self.conv(x, edge_index)


class _PNAEConv(_PNAConv):
    """``_PNAConv`` with edge features: PyG's ``PNAConv(..., edge_dim=d, towers=1, pre_layers=1, post_layers=1,
    divide_input=False)``.  The message is ``pre_nn(cat[x_i, x_j, edge_encoder(e_ij)])``, destination first; aggregators, the
    std clamp and mask, the scalers and ``delta`` are ``_PNAConv``'s.  Parameters: ``edge_encoder.weight`` [in, edge_dim],
    ``edge_encoder.bias`` [in], ``pre_nns.0.0.weight`` [in, 3 in], and the rest as ``_PNAConv``."""

    def __init__(self, in_channels: int, out_channels: int, edge_dim: int, avg_deg_log: float):
        super().__init__(in_channels, out_channels, avg_deg_log, pre_blocks=3)
        self.edge_encoder = nn.Linear(edge_dim, in_channels)

    def message(self, x: Tensor, edge_index: Tensor, edge_attr: Tensor) -> Tensor:
        src, dst = edge_index[0], edge_index[1]
        return self.pre_nns[0](torch.cat([x[dst], x[src], self.edge_encoder(edge_attr)], dim=-1))  # destination first

    def forward(self, x: Tensor, edge_index: Tensor, edge_attr: Tensor) -> Tensor:
        return self.reduce(x, edge_index, self.message(x, edge_index, edge_attr))


class PNAEConv_GNNB(nn.Module):
    """PNA with edge features (no class of the reference: its ``PNAConv_GNNB`` stores ``graph_input_edge_dim`` and drops it).
    ``GNNModel(..., graph_input_edge_dim=d, gnn_conv=PNAEConv_GNNB, ...)`` builds every layer with ``edge_dim=d`` (1 .. 16) and
    ``forward(x, edge_index, batch, edge_attr)`` hands the same ``edge_attr`` [E, d] to each.  The accelerated path is
    ``runtime.CompiledModel.from_model`` with ``forward_edges`` / ``forward_pyg_edges`` (C ABI ``include/gnnb_pna_edge.h``: the
    pre-NN is linear, so the edge term ``(W_c W_enc) e_ij + W_c b_enc`` is formed inside the aggregate kernel,
    csrc/k_pna_edge.hip).  ``Project`` does not generate such designs."""

    def __init__(self, in_channels: int, out_channels: int, edge_dim: int, delta: float = 1.0, p_in: int = 1,
                 p_out: int = 1):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.edge_dim = edge_dim
        self.delta = delta
        self.p_in = p_in
        self.p_out = p_out
        self.aggregators = ["max", "min", "mean", "std"]
        self.scalers = ["identity", "amplification", "attenuation"]
        self.conv = _PNAEConv(in_channels, out_channels, edge_dim, float(delta))
        self.delta_scaler = self.conv.aggr_module.avg_deg_log.item()

    def forward(self, x: Tensor, edge_index: Tensor, edge_attr: Tensor) -> Tensor:
        return self.conv(x, edge_index, edge_attr)


# --------------------------------------------------------------------------------------- GINE
class _GINEConv(nn.Module):
    """``nn((1+eps) x_i + sum_j relu(x_j + lin(e_ij)))`` (PyG GINEConv with edge_dim; reference models.py:97-123,
    native gine_conv gnn_builder_lib.h:1555-1742).  Parameters: ``nn.*``, ``lin.weight`` [in, edge_dim], ``lin.bias``."""

    def __init__(self, mlp: nn.Module, in_channels: int, edge_dim: int, eps: float = 0.0):
        super().__init__()
        self.nn = mlp
        self.lin = nn.Linear(edge_dim, in_channels)
        self.register_buffer("eps", torch.tensor([float(eps)]))

    def forward(self, x: Tensor, edge_index: Tensor, edge_attr: Tensor) -> Tensor:
        src, dst = edge_index[0], edge_index[1]
        agg = torch.zeros_like(x)
        if src.numel():
            agg = agg.index_add(0, dst, torch.relu(x[src] + self.lin(edge_attr)))
        return self.nn(agg + (1.0 + self.eps) * x)


class GINEConv_GNNB(nn.Module):
    """Reference models.py:97-123.  Not in SUPPORTED_GNN_CONVS there (the emitter has a TODO for it,
    templates/model.cpp.jinja:143-144); here ``GNNModel`` stacks it: ``GNNModel(..., graph_input_edge_dim=d, gnn_conv=
    GINEConv_GNNB, ...)`` builds every layer with ``edge_dim=d`` (1 .. 16) and ``forward(x, edge_index, batch, edge_attr)`` hands
    the same ``edge_attr`` [E, d] to each.  The accelerated path is ``runtime.CompiledModel.from_model`` with
    ``forward_edges`` / ``forward_pyg_edges`` (C ABI ``include/gnnb_edge.h``: the edge projection runs inside the aggregate kernel,
    csrc/k_gine.hip).  One layer as separate stage calls stays reachable through ``runtime.CompiledModel.gine_conv``
    (``gnnb_aggregate_edges`` + ``gnnb_linear``).  ``Project`` does not generate GINE designs."""

    def __init__(self, in_channels: int, out_channels: int, edge_dim: int, hidden_dim: Optional[int] = None,
                 eps: float = 0.0, p_in: int = 1, p_out: int = 1):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.edge_dim = edge_dim
        self.hidden_dim = hidden_dim
        self.eps = eps
        self.p_in = p_in
        self.p_out = p_out
        self.mlp = GIN_MLP(in_channels, out_channels, hidden_dim)
        self.conv = _GINEConv(self.mlp, in_channels, edge_dim, eps=eps)

    def forward(self, x: Tensor, edge_index: Tensor, edge_attr: Tensor) -> Tensor:
        return self.conv(x, edge_index, edge_attr)


class GATConv_GNNB(nn.Module):
    """Listed by the reference's SUPPORTED_GNN_CONVS but it has no native kernel for it
    (gnn_builder_lib.h:2343 ``// TODO: GAT layer``; template TODO model.cpp.jinja:141-142);
    out of scope here as well.  Attention models run as ``GATv2Conv_GNNB`` below (``GATv2EConv_GNNB`` with edge features);
    PyG's ``GATConv`` itself runs as ``GATv1Conv_GNNB`` (``GATv1EConv_GNNB`` with ``edge_dim``).  This stub keeps the reference's behaviour."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        raise NotImplementedError(
            "GATConv_GNNB has no native path in the reference (gnn_builder_lib.h:2343) and none here")


# --------------------------------------------------------------------------------------- GATv2
MAX_GAT_HEADS = 8  # of a GATv2 model (include/gnnb_gat.h)


class _GATv2Conv(nn.Module):
    """PyG's ``GATv2Conv(in_channels, out_channels, heads, concat=True, negative_slope, add_self_loops=True, bias=True,
    share_weights=False, edge_dim=None, dropout=0)`` with ``out_channels`` PER HEAD, as PyG counts it::

        xl = lin_l(x) [N, H, C]      xr = lin_r(x) [N, H, C]
        s_ij[h] = sum_c att[h, c] * leaky_relu(xl_j[h, c] + xr_i[h, c])     for j in N(i) u {i}
        a_ij[h] = exp(s_ij[h] - max_j s_ij[h]) / (sum_j exp(s_ij[h] - max_j s_ij[h]) + 1e-16)
        out_i[h, :] = sum_j a_ij[h] * xl_j[h, :]  + bias

    Self loops are PyG's (``remove_self_loops`` + ``add_self_loops``): explicit ``(v, v)`` edges of the input are removed and
    exactly one is added per node -- the rule ``_GCNConv`` applies.  Parameters: ``lin_l.weight`` [H C, in], ``lin_l.bias``,
    ``lin_r.weight``, ``lin_r.bias``, ``att`` [1, H, C], ``bias`` [H C]; weights and ``att`` glorot, biases zero.  ``edge_dim=d``
    is ``_GATv2EConv`` below."""

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1, negative_slope: float = 0.2):
        super().__init__()
        self.heads = heads
        self.out_channels = out_channels
        self.negative_slope = negative_slope
        self.lin_l = nn.Linear(in_channels, heads * out_channels)
        self.lin_r = nn.Linear(in_channels, heads * out_channels)
        self.att = nn.Parameter(torch.empty(1, heads, out_channels))
        self.bias = nn.Parameter(torch.zeros(heads * out_channels))
        _glorot(self.lin_l.weight)
        _glorot(self.lin_r.weight)
        _glorot(self.att)
        with torch.no_grad():
            self.lin_l.bias.zero_()
            self.lin_r.bias.zero_()

    def forward(self, x: Tensor, edge_index: Tensor) -> Tensor:
        n, H, C = x.size(0), self.heads, self.out_channels
        if edge_index.numel():
            edge_index = edge_index[:, edge_index[0] != edge_index[1]]
        loops = torch.arange(n, dtype=torch.long, device=x.device)
        src = torch.cat([edge_index[0].long(), loops]) if edge_index.numel() else loops
        dst = torch.cat([edge_index[1].long(), loops]) if edge_index.numel() else loops
        xl = self.lin_l(x).view(n, H, C)
        xr = self.lin_r(x).view(n, H, C)
        s = (nn.functional.leaky_relu(xl[src] + xr[dst], self.negative_slope) * self.att).sum(dim=-1)  # [E + N, H]
        idx = dst.unsqueeze(-1).expand(-1, H)
        smax = s.new_full((n, H), float("-inf")).scatter_reduce(0, idx, s, reduce="amax", include_self=True)
        e = (s - smax[dst]).exp()
        a = e / (s.new_zeros(n, H).index_add(0, dst, e)[dst] + 1e-16)
        out = x.new_zeros(n, H, C).index_add(0, dst, a.unsqueeze(-1) * xl[src])
        return out.reshape(n, H * C) + self.bias


class GATv2Conv_GNNB(nn.Module):
    """GATv2 (no class of the reference, whose ``GATConv_GNNB`` is a stub): ``out_channels`` is the layer's WHOLE output width,
    split over ``heads`` (1 .. 8, dividing it) and concatenated -- PyG's ``GATv2Conv(in_channels, out_channels // heads,
    heads=heads)``.  ``GNNModel(..., gnn_conv=GATv2Conv_GNNB, gnn_heads=H)`` stacks it; ``forward(x, edge_index)``.  The
    accelerated path is ``runtime.CompiledModel.from_model`` with the ordinary ``forward`` / ``forward_pyg`` (C ABI
    ``include/gnnb_gat.h``: one GEMM and one launch of csrc/k_gatv2.hip per layer, the softmax online inside the aggregate).
    This class ignores ``graph_input_edge_dim`` and ``edge_attr``; scores that see the bond features are ``GATv2EConv_GNNB``'s.
    ``Project`` does not generate such designs."""

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1, negative_slope: float = 0.2, p_in: int = 1,
                 p_out: int = 1):
        super().__init__()
        if not isinstance(heads, int) or isinstance(heads, bool) or not 1 <= heads <= MAX_GAT_HEADS:
            raise ValueError(f"heads must be an int in 1 .. {MAX_GAT_HEADS} (got {heads!r})")
        if out_channels % heads != 0:
            raise ValueError(f"out_channels ({out_channels}) must be divisible by heads ({heads})")
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.heads = heads
        self.negative_slope = float(negative_slope)
        self.p_in = p_in
        self.p_out = p_out
        self.conv = _GATv2Conv(in_channels, out_channels // heads, heads, self.negative_slope)

    def forward(self, x: Tensor, edge_index: Tensor) -> Tensor:
        return self.conv(x, edge_index)


# --------------------------------------------------------------------------------------- GAT (v1)
class _GATConv(nn.Module):
    """PyG's ``GATConv(in_channels, out_channels, heads, concat=True, negative_slope, add_self_loops=True, bias=True,
    edge_dim=None, dropout=0, residual=False)`` with ``out_channels`` PER HEAD, as PyG counts it::

        x' = lin(x) [N, H, C]
        s_ij[h] = leaky_relu(sum_c att_src[h, c] * x'_j[h, c] + sum_c att_dst[h, c] * x'_i[h, c])     for j in N(i) u {i}
        a_ij[h] = exp(s_ij[h] - max_j s_ij[h]) / (sum_j exp(s_ij[h] - max_j s_ij[h]) + 1e-16)
        out_i[h, :] = sum_j a_ij[h] * x'_j[h, :]  + bias

    Self loops are PyG's, as ``_GATv2Conv`` has them: explicit ``(v, v)`` edges are removed, then one is added per node.
    Parameters: ``lin.weight`` [H C, in] (no bias), ``att_src`` [1, H, C], ``att_dst`` [1, H, C], ``bias`` [H C]; the weight and
    both ``att`` glorot, the bias zero."""

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1, negative_slope: float = 0.2):
        super().__init__()
        self.heads = heads
        self.out_channels = out_channels
        self.negative_slope = negative_slope
        self.lin = nn.Linear(in_channels, heads * out_channels, bias=False)
        self.att_src = nn.Parameter(torch.empty(1, heads, out_channels))
        self.att_dst = nn.Parameter(torch.empty(1, heads, out_channels))
        self.bias = nn.Parameter(torch.zeros(heads * out_channels))
        _glorot(self.lin.weight)
        _glorot(self.att_src)
        _glorot(self.att_dst)

    def forward(self, x: Tensor, edge_index: Tensor) -> Tensor:
        n, H, C = x.size(0), self.heads, self.out_channels
        if edge_index.numel():
            edge_index = edge_index[:, edge_index[0] != edge_index[1]]
        loops = torch.arange(n, dtype=torch.long, device=x.device)
        src = torch.cat([edge_index[0].long(), loops]) if edge_index.numel() else loops
        dst = torch.cat([edge_index[1].long(), loops]) if edge_index.numel() else loops
        xl = self.lin(x).view(n, H, C)
        s_src = (xl * self.att_src).sum(dim=-1)  # [N, H]
        s_dst = (xl * self.att_dst).sum(dim=-1)
        s = nn.functional.leaky_relu(s_src[src] + s_dst[dst], self.negative_slope)  # [E + N, H]
        idx = dst.unsqueeze(-1).expand(-1, H)
        smax = s.new_full((n, H), float("-inf")).scatter_reduce(0, idx, s, reduce="amax", include_self=True)
        e = (s - smax[dst]).exp()
        a = e / (s.new_zeros(n, H).index_add(0, dst, e)[dst] + 1e-16)
        out = x.new_zeros(n, H, C).index_add(0, dst, a.unsqueeze(-1) * xl[src])
        return out.reshape(n, H * C) + self.bias


class GATv1Conv_GNNB(nn.Module):
    """GAT as PyG's ``GATConv`` computes it (the reference's ``GATConv_GNNB`` is a stub and stays one): ``out_channels`` is the
    layer's WHOLE output width, split over ``heads`` (1 .. 8, dividing it) and concatenated -- PyG's ``GATConv(in_channels,
    out_channels // heads, heads=heads)``.  ``GNNModel(..., gnn_conv=GATv1Conv_GNNB, gnn_heads=H)`` stacks it;
    ``forward(x, edge_index)``.  The accelerated path is ``runtime.CompiledModel.from_model`` with the ordinary ``forward`` /
    ``forward_pyg`` (C ABI ``include/gnnb_gatconv.h``: one GEMM, which also gives both per-node scores, and one launch of
    csrc/k_gat.hip per layer).  This class ignores ``graph_input_edge_dim`` and ``edge_attr``.  ``Project`` does not generate such
    designs."""

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1, negative_slope: float = 0.2, p_in: int = 1,
                 p_out: int = 1):
        super().__init__()
        if not isinstance(heads, int) or isinstance(heads, bool) or not 1 <= heads <= MAX_GAT_HEADS:
            raise ValueError(f"heads must be an int in 1 .. {MAX_GAT_HEADS} (got {heads!r})")
        if out_channels % heads != 0:
            raise ValueError(f"out_channels ({out_channels}) must be divisible by heads ({heads})")
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.heads = heads
        self.negative_slope = float(negative_slope)
        self.p_in = p_in
        self.p_out = p_out
        self.conv = _GATConv(in_channels, out_channels // heads, heads, self.negative_slope)

    def forward(self, x: Tensor, edge_index: Tensor) -> Tensor:
        return self.conv(x, edge_index)


class _GATEConv(_GATConv):
    """``_GATConv`` with edge features: PyG's ``GATConv(..., edge_dim=d, fill_value='mean')``.  The edge term enters the score
    only, as one scalar per head; the message stays ``x'_j``::

        p_ij = lin_edge(e_ij) [H, C]                     lin_edge: Linear(d, H C, bias=False)
        s_ij[h] = leaky_relu(att_src[h] . x'_j[h] + att_dst[h] . x'_i[h] + att_edge[h] . p_ij[h])     for j in N(i) u {i}

    Self loops: explicit ``(v, v)`` rows of the input are removed TOGETHER WITH their attribute rows, one self loop is added per
    node and its attribute is the mean of the attributes of the node's remaining in-edges (taken after the removal; 0 for a node
    without in-edges).  Parameters: ``_GATConv``'s, then ``att_edge`` [1, H, C] and ``lin_edge.weight`` [H C, d], both glorot."""

    def __init__(self, in_channels: int, out_channels: int, edge_dim: int, heads: int = 1, negative_slope: float = 0.2):
        super().__init__(in_channels, out_channels, heads, negative_slope)
        self.att_edge = nn.Parameter(torch.empty(1, heads, out_channels))
        self.lin_edge = nn.Linear(edge_dim, heads * out_channels, bias=False)
        _glorot(self.att_edge)
        _glorot(self.lin_edge.weight)

    def forward(self, x: Tensor, edge_index: Tensor, edge_attr: Tensor) -> Tensor:
        n, H, C = x.size(0), self.heads, self.out_channels
        d = self.lin_edge.in_features
        edge_attr = edge_attr.reshape(-1, d)
        if edge_index.numel():
            keep = edge_index[0] != edge_index[1]
            edge_index, edge_attr = edge_index[:, keep], edge_attr[keep]
        loops = torch.arange(n, dtype=torch.long, device=x.device)
        esrc = edge_index[0].long() if edge_index.numel() else loops[:0]
        edst = edge_index[1].long() if edge_index.numel() else loops[:0]
        # fill_value='mean': the self loop's attribute is the mean over the remaining in-edges (count clamped to 1: 0 without any)
        deg = x.new_zeros(n).index_add(0, edst, x.new_ones(edst.numel()))
        loop_attr = x.new_zeros(n, d).index_add(0, edst, edge_attr) / deg.clamp(min=1).unsqueeze(-1)
        src, dst = torch.cat([esrc, loops]), torch.cat([edst, loops])
        p = self.lin_edge(torch.cat([edge_attr, loop_attr])).view(-1, H, C)
        xl = self.lin(x).view(n, H, C)
        s_src = (xl * self.att_src).sum(dim=-1)  # [N, H]
        s_dst = (xl * self.att_dst).sum(dim=-1)
        s_edge = (p * self.att_edge).sum(dim=-1)  # [E + N, H]
        s = nn.functional.leaky_relu(s_src[src] + s_dst[dst] + s_edge, self.negative_slope)
        idx = dst.unsqueeze(-1).expand(-1, H)
        smax = s.new_full((n, H), float("-inf")).scatter_reduce(0, idx, s, reduce="amax", include_self=True)
        e = (s - smax[dst]).exp()
        a = e / (s.new_zeros(n, H).index_add(0, dst, e)[dst] + 1e-16)
        out = x.new_zeros(n, H, C).index_add(0, dst, a.unsqueeze(-1) * xl[src])
        return out.reshape(n, H * C) + self.bias


class GATv1EConv_GNNB(nn.Module):
    """GAT (v1) with edge features: ``GATv1Conv_GNNB`` whose scores see ``edge_attr`` -- PyG's ``GATConv(in_channels,
    out_channels // heads, heads=heads, edge_dim=d)``.  ``GNNModel(..., graph_input_edge_dim=d, gnn_conv=GATv1EConv_GNNB,
    gnn_heads=H)`` builds every layer with ``edge_dim=d`` (1 .. 16) and ``forward(x, edge_index, batch, edge_attr)`` hands the same
    ``edge_attr`` [E, d] to each.  The accelerated path is ``runtime.CompiledModel.from_model`` with ``forward_edges`` /
    ``forward_pyg_edges`` (C ABI ``include/gnnb_gatconv_edge.h``: ``att_edge`` is folded into ``lin_edge`` at upload, the edge term
    is ``d`` FMAs per edge and head inside the aggregate kernel, csrc/k_gat_edge.hip).  ``Project`` does not generate such designs."""

    def __init__(self, in_channels: int, out_channels: int, edge_dim: int, heads: int = 1, negative_slope: float = 0.2,
                 p_in: int = 1, p_out: int = 1):
        super().__init__()
        if not isinstance(heads, int) or isinstance(heads, bool) or not 1 <= heads <= MAX_GAT_HEADS:
            raise ValueError(f"heads must be an int in 1 .. {MAX_GAT_HEADS} (got {heads!r})")
        if out_channels % heads != 0:
            raise ValueError(f"out_channels ({out_channels}) must be divisible by heads ({heads})")
        if not isinstance(edge_dim, int) or isinstance(edge_dim, bool) or not 1 <= edge_dim <= 16:
            raise ValueError(f"edge_dim must be an int in 1 .. 16 (got {edge_dim!r})")
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.edge_dim = edge_dim
        self.heads = heads
        self.negative_slope = float(negative_slope)
        self.p_in = p_in
        self.p_out = p_out
        self.conv = _GATEConv(in_channels, out_channels // heads, edge_dim, heads, self.negative_slope)

    def forward(self, x: Tensor, edge_index: Tensor, edge_attr: Tensor) -> Tensor:
        return self.conv(x, edge_index, edge_attr)


class _GATv2EConv(_GATv2Conv):
    """``_GATv2Conv`` with edge features: PyG's ``GATv2Conv(..., edge_dim=d, fill_value='mean')``.  The edge term enters the score
    only, the message stays ``xl_j``::

        p_ij = lin_edge(e_ij) [H, C]                     lin_edge: Linear(d, H C, bias=False)
        s_ij[h] = sum_c att[h, c] * leaky_relu(xl_j[h, c] + xr_i[h, c] + p_ij[h, c])     for j in N(i) u {i}

    Self loops: explicit ``(v, v)`` rows of the input are removed TOGETHER WITH their attribute rows, one self loop is added per
    node and its attribute is the mean of the attributes of the node's remaining in-edges (taken after the removal; 0 for a node
    without in-edges).  Parameters: ``_GATv2Conv``'s, then ``lin_edge.weight`` [H C, d], glorot."""

    def __init__(self, in_channels: int, out_channels: int, edge_dim: int, heads: int = 1, negative_slope: float = 0.2):
        super().__init__(in_channels, out_channels, heads, negative_slope)
        self.lin_edge = nn.Linear(edge_dim, heads * out_channels, bias=False)
        _glorot(self.lin_edge.weight)

    def forward(self, x: Tensor, edge_index: Tensor, edge_attr: Tensor) -> Tensor:
        n, H, C = x.size(0), self.heads, self.out_channels
        d = self.lin_edge.in_features
        edge_attr = edge_attr.reshape(-1, d)
        if edge_index.numel():
            keep = edge_index[0] != edge_index[1]
            edge_index, edge_attr = edge_index[:, keep], edge_attr[keep]
        loops = torch.arange(n, dtype=torch.long, device=x.device)
        esrc = edge_index[0].long() if edge_index.numel() else loops[:0]
        edst = edge_index[1].long() if edge_index.numel() else loops[:0]
        # fill_value='mean': the self loop's attribute is the mean over the remaining in-edges (count clamped to 1: 0 without any)
        deg = x.new_zeros(n).index_add(0, edst, x.new_ones(edst.numel()))
        loop_attr = x.new_zeros(n, d).index_add(0, edst, edge_attr) / deg.clamp(min=1).unsqueeze(-1)
        src, dst = torch.cat([esrc, loops]), torch.cat([edst, loops])
        p = self.lin_edge(torch.cat([edge_attr, loop_attr])).view(-1, H, C)
        xl = self.lin_l(x).view(n, H, C)
        xr = self.lin_r(x).view(n, H, C)
        s = (nn.functional.leaky_relu(xl[src] + xr[dst] + p, self.negative_slope) * self.att).sum(dim=-1)  # [E + N, H]
        idx = dst.unsqueeze(-1).expand(-1, H)
        smax = s.new_full((n, H), float("-inf")).scatter_reduce(0, idx, s, reduce="amax", include_self=True)
        e = (s - smax[dst]).exp()
        a = e / (s.new_zeros(n, H).index_add(0, dst, e)[dst] + 1e-16)
        out = x.new_zeros(n, H, C).index_add(0, dst, a.unsqueeze(-1) * xl[src])
        return out.reshape(n, H * C) + self.bias


class GATv2EConv_GNNB(nn.Module):
    """GATv2 with edge features: ``GATv2Conv_GNNB`` whose scores see ``edge_attr`` -- PyG's ``GATv2Conv(in_channels,
    out_channels // heads, heads=heads, edge_dim=d)``.  ``GNNModel(..., graph_input_edge_dim=d, gnn_conv=GATv2EConv_GNNB,
    gnn_heads=H)`` builds every layer with ``edge_dim=d`` (1 .. 16) and ``forward(x, edge_index, batch, edge_attr)`` hands the same
    ``edge_attr`` [E, d] to each.  The accelerated path is ``runtime.CompiledModel.from_model`` with ``forward_edges`` /
    ``forward_pyg_edges`` (C ABI ``include/gnnb_gat_edge.h``: the edge projection and the scores are formed inside the aggregate
    kernel, csrc/k_gatv2_edge.hip).  ``Project`` does not generate such designs."""

    def __init__(self, in_channels: int, out_channels: int, edge_dim: int, heads: int = 1, negative_slope: float = 0.2,
                 p_in: int = 1, p_out: int = 1):
        super().__init__()
        if not isinstance(heads, int) or isinstance(heads, bool) or not 1 <= heads <= MAX_GAT_HEADS:
            raise ValueError(f"heads must be an int in 1 .. {MAX_GAT_HEADS} (got {heads!r})")
        if out_channels % heads != 0:
            raise ValueError(f"out_channels ({out_channels}) must be divisible by heads ({heads})")
        if not isinstance(edge_dim, int) or isinstance(edge_dim, bool) or not 1 <= edge_dim <= 16:
            raise ValueError(f"edge_dim must be an int in 1 .. 16 (got {edge_dim!r})")
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.edge_dim = edge_dim
        self.heads = heads
        self.negative_slope = float(negative_slope)
        self.p_in = p_in
        self.p_out = p_out
        self.conv = _GATv2EConv(in_channels, out_channels // heads, edge_dim, heads, self.negative_slope)

    def forward(self, x: Tensor, edge_index: Tensor, edge_attr: Tensor) -> Tensor:
        return self.conv(x, edge_index, edge_attr)


# --------------------------------------------------------------------------------------- TransformerConv
class _TransformerConv(nn.Module):
    """PyG's ``TransformerConv(in_channels, out_channels, heads, concat=True, beta=False, dropout=0, edge_dim=None, bias=True,
    root_weight=True)`` -- the Graph Transformer layer -- with ``out_channels`` PER HEAD, as PyG counts it::

        q = lin_query(x) [N, H, C]   k = lin_key(x) [N, H, C]   v = lin_value(x) [N, H, C]   r = lin_skip(x) [N, H C]
        s_ij[h] = (q_i[h, :] . k_j[h, :]) / sqrt(C)                        for j in N(i) -- the input's edges as they are
        a_ij[h] = exp(s_ij[h] - max_j s_ij[h]) / (sum_j exp(s_ij[h] - max_j s_ij[h]) + 1e-16)
        out_i   = concat_h( sum_j a_ij[h] * v_j[h, :] ) + r_i

    No self loop is added and none is removed: an explicit ``(v, v)`` edge is an ordinary edge, a node without in-edges gets
    ``lin_skip(x)`` alone.  Modules in PyG's order ``lin_key``, ``lin_query``, ``lin_value``, ``lin_skip``, each
    ``nn.Linear(in, H C, bias=True)`` with torch's default initialisation (what PyG's ``Linear`` uses); the conv has no
    parameter of its own.  ``edge_dim`` is ``_TransformerEConv``'s.  Out of scope: ``beta=True``, ``concat=False``,
    ``root_weight=False``, dropout."""

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1):
        super().__init__()
        self.heads = heads
        self.out_channels = out_channels
        self.lin_key = nn.Linear(in_channels, heads * out_channels)
        self.lin_query = nn.Linear(in_channels, heads * out_channels)
        self.lin_value = nn.Linear(in_channels, heads * out_channels)
        self.lin_skip = nn.Linear(in_channels, heads * out_channels)

    def forward(self, x: Tensor, edge_index: Tensor) -> Tensor:
        n, H, C = x.size(0), self.heads, self.out_channels
        src, dst = edge_index[0].long(), edge_index[1].long()
        q = self.lin_query(x).view(n, H, C)
        k = self.lin_key(x).view(n, H, C)
        v = self.lin_value(x).view(n, H, C)
        s = (q[dst] * k[src]).sum(dim=-1) / math.sqrt(C)  # [E, H]
        idx = dst.unsqueeze(-1).expand(-1, H)
        smax = s.new_full((n, H), float("-inf")).scatter_reduce(0, idx, s, reduce="amax", include_self=True)
        e = (s - smax[dst]).exp()
        a = e / (s.new_zeros(n, H).index_add(0, dst, e)[dst] + 1e-16)
        out = x.new_zeros(n, H, C).index_add(0, dst, a.unsqueeze(-1) * v[src])
        return out.reshape(n, H * C) + self.lin_skip(x)


class TransformerConv_GNNB(nn.Module):
    """The Graph Transformer layer (no class of the reference): ``out_channels`` is the layer's WHOLE output width, split over
    ``heads`` (1 .. 8, dividing it) and concatenated, as ``GATv2Conv_GNNB`` counts it -- PyG's ``TransformerConv(in_channels,
    out_channels // heads, heads=heads)``.  ``GNNModel(..., gnn_conv=TransformerConv_GNNB, gnn_heads=H)`` stacks it;
    ``forward(x, edge_index)``.  The accelerated path is ``runtime.CompiledModel.from_model`` with the ordinary ``forward`` /
    ``forward_pyg`` (C ABI ``include/gnnb_transformer.h``: one GEMM ``x -> [q | k | v | r]`` and one launch of
    csrc/k_transformer.hip per layer, the softmax online inside the aggregate).  This class ignores ``graph_input_edge_dim`` and
    ``edge_attr``; attention that sees the bond features is ``TransformerEConv_GNNB``'s.  Out of scope: ``beta=True``,
    ``concat=False``, ``root_weight=False`` and dropout.  ``Project`` does not generate such designs."""

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1, p_in: int = 1, p_out: int = 1):
        super().__init__()
        if not isinstance(heads, int) or isinstance(heads, bool) or not 1 <= heads <= MAX_GAT_HEADS:
            raise ValueError(f"heads must be an int in 1 .. {MAX_GAT_HEADS} (got {heads!r})")
        if out_channels % heads != 0:
            raise ValueError(f"out_channels ({out_channels}) must be divisible by heads ({heads})")
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.heads = heads
        self.p_in = p_in
        self.p_out = p_out
        self.conv = _TransformerConv(in_channels, out_channels // heads, heads)

    def forward(self, x: Tensor, edge_index: Tensor) -> Tensor:
        return self.conv(x, edge_index)


class _TransformerEConv(_TransformerConv):
    """``_TransformerConv`` with edge features: PyG's ``TransformerConv(..., edge_dim=d)``.  The projected edge attributes are added
    to the key AND to the value::

        p_ij    = lin_edge(e_ij) [H, C]                                    lin_edge: Linear(d, H C, bias=False)
        s_ij[h] = (q_i[h, :] . (k_j[h, :] + p_ij[h, :])) / sqrt(C)         for j in N(i) -- the input's edges as they are
        a_ij[h] = exp(s_ij[h] - max_j s_ij[h]) / (sum_j exp(s_ij[h] - max_j s_ij[h]) + 1e-16)
        out_i   = concat_h( sum_j a_ij[h] * (v_j[h, :] + p_ij[h, :]) ) + r_i

    No self loop is added and none is removed: an explicit ``(v, v)`` edge is an ordinary edge and so is its attribute row; a node
    without in-edges gets ``lin_skip(x)`` alone.  Parameters: ``_TransformerConv``'s, then ``lin_edge.weight`` [H C, d] with
    torch's default ``Linear`` initialisation (what PyG uses there).  This is the layer as it is defined: project, add to key and
    value.  (The accelerated path evaluates the same sums with the projection moved out of the per-edge work; that is its
    business, include/gnnb_transformer_edge.h.)"""

    def __init__(self, in_channels: int, out_channels: int, edge_dim: int, heads: int = 1):
        super().__init__(in_channels, out_channels, heads)
        self.lin_edge = nn.Linear(edge_dim, heads * out_channels, bias=False)

    def forward(self, x: Tensor, edge_index: Tensor, edge_attr: Tensor) -> Tensor:
        n, H, C = x.size(0), self.heads, self.out_channels
        src, dst = edge_index[0].long(), edge_index[1].long()
        p = self.lin_edge(edge_attr.reshape(-1, self.lin_edge.in_features)).view(-1, H, C)
        q = self.lin_query(x).view(n, H, C)
        k = self.lin_key(x).view(n, H, C)[src] + p
        v = self.lin_value(x).view(n, H, C)[src] + p
        s = (q[dst] * k).sum(dim=-1) / math.sqrt(C)  # [E, H]
        idx = dst.unsqueeze(-1).expand(-1, H)
        smax = s.new_full((n, H), float("-inf")).scatter_reduce(0, idx, s, reduce="amax", include_self=True)
        e = (s - smax[dst]).exp()
        a = e / (s.new_zeros(n, H).index_add(0, dst, e)[dst] + 1e-16)
        out = x.new_zeros(n, H, C).index_add(0, dst, a.unsqueeze(-1) * v)
        return out.reshape(n, H * C) + self.lin_skip(x)


class TransformerEConv_GNNB(nn.Module):
    """The Graph Transformer layer with edge features: ``TransformerConv_GNNB`` whose keys and values see ``edge_attr`` -- PyG's
    ``TransformerConv(in_channels, out_channels // heads, heads=heads, edge_dim=d)``.  ``GNNModel(..., graph_input_edge_dim=d,
    gnn_conv=TransformerEConv_GNNB, gnn_heads=H)`` builds every layer with ``edge_dim=d`` (1 .. 16) and
    ``forward(x, edge_index, batch, edge_attr)`` hands the same ``edge_attr`` [E, d] to each.  The accelerated path is
    ``runtime.CompiledModel.from_model`` with ``forward_edges`` / ``forward_pyg_edges`` (C ABI
    ``include/gnnb_transformer_edge.h``: one GEMM ``x -> [q | k | v | r | qe]`` and one launch of csrc/k_transformer_edge.hip per
    layer).  Out of scope: ``beta=True``, ``concat=False``, ``root_weight=False`` and dropout.  ``Project`` does not generate such
    designs."""

    def __init__(self, in_channels: int, out_channels: int, edge_dim: int, heads: int = 1, p_in: int = 1, p_out: int = 1):
        super().__init__()
        if not isinstance(heads, int) or isinstance(heads, bool) or not 1 <= heads <= MAX_GAT_HEADS:
            raise ValueError(f"heads must be an int in 1 .. {MAX_GAT_HEADS} (got {heads!r})")
        if out_channels % heads != 0:
            raise ValueError(f"out_channels ({out_channels}) must be divisible by heads ({heads})")
        if not isinstance(edge_dim, int) or isinstance(edge_dim, bool) or not 1 <= edge_dim <= 16:
            raise ValueError(f"edge_dim must be an int in 1 .. 16 (got {edge_dim!r})")
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.edge_dim = edge_dim
        self.heads = heads
        self.p_in = p_in
        self.p_out = p_out
        self.conv = _TransformerEConv(in_channels, out_channels // heads, edge_dim, heads)

    def forward(self, x: Tensor, edge_index: Tensor, edge_attr: Tensor) -> Tensor:
        return self.conv(x, edge_index, edge_attr)


# --------------------------------------------------------------------------------------- ResGatedGraphConv
class _ResGatedGraphConv(nn.Module):
    """PyG's ``ResGatedGraphConv(in_channels, out_channels, act=Sigmoid(), edge_dim=None, root_weight=True, bias=True)`` -- the
    Residual Gated Graph ConvNet of Bresson & Laurent, the "GatedGCN" of *Benchmarking GNNs* without its edge stream::

        k = lin_key(x) [N, out]   q = lin_query(x) [N, out]   v = lin_value(x) [N, out]   r = lin_skip(x) [N, out]
        g_ij  = sigmoid(k_i + q_j)                     [out] -- a gate per column; for j in N(i), the input's edges as they are
        out_i = sum_j g_ij * v_j + r_i + bias          elementwise

    The DESTINATION's key meets the SOURCE's query (PyG's ``message(k_i, q_j, v_j)``).  No self loop is added and none is
    removed: an explicit ``(v, v)`` edge is an ordinary edge, duplicate edges count as often as they occur, a node without
    in-edges gets ``lin_skip(x_i) + bias`` alone.  Modules in PyG's order ``lin_key``, ``lin_query``, ``lin_value`` -- each
    ``nn.Linear(in, out, bias=True)`` --, ``lin_skip`` -- ``nn.Linear(in, out, bias=False)`` --, all with torch's default
    initialisation (what PyG's ``Linear`` uses), and the conv's own ``bias`` [out], zero-initialised.  Out of scope:
    ``edge_dim``, ``root_weight=False``, ``bias=False``, gates other than the sigmoid."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.out_channels = out_channels
        self.lin_key = nn.Linear(in_channels, out_channels)
        self.lin_query = nn.Linear(in_channels, out_channels)
        self.lin_value = nn.Linear(in_channels, out_channels)
        self.lin_skip = nn.Linear(in_channels, out_channels, bias=False)
        self.bias = nn.Parameter(torch.zeros(out_channels))

    def forward(self, x: Tensor, edge_index: Tensor) -> Tensor:
        src, dst = edge_index[0].long(), edge_index[1].long()
        k, q, v = self.lin_key(x), self.lin_query(x), self.lin_value(x)
        out = torch.zeros_like(v).index_add(0, dst, torch.sigmoid(k[dst] + q[src]) * v[src])
        return out + self.lin_skip(x) + self.bias


class ResGatedGraphConv_GNNB(nn.Module):
    """The residual gated graph conv (no class of the reference): PyG's ``ResGatedGraphConv(in_channels, out_channels)``.
    ``GNNModel(..., gnn_conv=ResGatedGraphConv_GNNB)`` stacks it (``gnn_heads`` stays 1); ``forward(x, edge_index)``.  The
    accelerated path is ``runtime.CompiledModel.from_model`` with the ordinary ``forward`` / ``forward_pyg`` (C ABI
    ``include/gnnb_resgated.h``: one GEMM ``x -> [k | q | v | r]`` and one launch of csrc/k_resgated.hip per layer, the gate formed
    inside the aggregate).  This class ignores ``graph_input_edge_dim`` and ``edge_attr``: PyG's ``edge_dim`` form, which
    concatenates ``e_ij`` to the inputs of key, query and value, is a model kind of its own -- ``ResGatedGraphEConv_GNNB``
    below.  Out of scope: ``root_weight=False``, ``bias=False`` and other gates.  ``Project`` does not generate such designs."""

    def __init__(self, in_channels: int, out_channels: int, p_in: int = 1, p_out: int = 1):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.p_in = p_in
        self.p_out = p_out
        self.conv = _ResGatedGraphConv(in_channels, out_channels)

    def forward(self, x: Tensor, edge_index: Tensor) -> Tensor:
        return self.conv(x, edge_index)


class _ResGatedGraphEConv(nn.Module):
    """PyG's ``ResGatedGraphConv(in_channels, out_channels, act=Sigmoid(), edge_dim=d, root_weight=True, bias=True)``: the gated
    graph conv whose key, query and value see the edge's attributes, concatenated behind the node's features per edge::

        k_ij = lin_key([x_i | e_ij])   q_ij = lin_query([x_j | e_ij])   v_ij = lin_value([x_j | e_ij])     [out] each
        out_i = sum_j sigmoid(k_ij + q_ij) * v_ij + lin_skip(x_i) + bias      for j in N(i), the input's edges as they are

    Modules in PyG's order and with PyG's shapes, so that a PyG ``state_dict`` loads: ``lin_key``, ``lin_query``, ``lin_value``
    -- each ``nn.Linear(in + d, out, bias=True)`` --, ``lin_skip`` -- ``nn.Linear(in, out, bias=False)`` --, and the conv's own
    ``bias`` [out], zero-initialised.  No self loop is added and none is removed; an explicit ``(v, v)`` edge is an ordinary edge
    with its own attribute row; a node without in-edges gets ``lin_skip(x_i) + bias`` alone.  Out of scope:
    ``root_weight=False``, ``bias=False``, gates other than the sigmoid."""

    def __init__(self, in_channels: int, out_channels: int, edge_dim: int):
        super().__init__()
        self.out_channels = out_channels
        self.edge_dim = edge_dim
        self.lin_key = nn.Linear(in_channels + edge_dim, out_channels)
        self.lin_query = nn.Linear(in_channels + edge_dim, out_channels)
        self.lin_value = nn.Linear(in_channels + edge_dim, out_channels)
        self.lin_skip = nn.Linear(in_channels, out_channels, bias=False)
        self.bias = nn.Parameter(torch.zeros(out_channels))

    def forward(self, x: Tensor, edge_index: Tensor, edge_attr: Tensor) -> Tensor:
        src, dst = edge_index[0].long(), edge_index[1].long()
        e = edge_attr.to(x.dtype).reshape(src.numel(), self.edge_dim)
        k = self.lin_key(torch.cat([x[dst], e], dim=-1))
        q = self.lin_query(torch.cat([x[src], e], dim=-1))
        v = self.lin_value(torch.cat([x[src], e], dim=-1))
        out = x.new_zeros(x.shape[0], self.out_channels).index_add(0, dst, torch.sigmoid(k + q) * v)
        return out + self.lin_skip(x) + self.bias


class ResGatedGraphEConv_GNNB(nn.Module):
    """The residual gated graph conv with edge features: PyG's ``ResGatedGraphConv(in_channels, out_channels, edge_dim=d)``.
    ``GNNModel(..., graph_input_edge_dim=d, gnn_conv=ResGatedGraphEConv_GNNB)`` builds every layer with ``edge_dim=d`` (1 .. 16)
    and ``forward(x, edge_index, batch, edge_attr)`` hands the same ``edge_attr`` [E, d] to each (``gnn_heads`` stays 1).  The
    accelerated path is ``runtime.CompiledModel.from_model`` with ``forward_edges`` / ``forward_pyg_edges`` (C ABI
    ``include/gnnb_resgated_edge.h``: one GEMM ``x -> [k | q | v | r]`` and one launch of csrc/k_resgated_edge.hip per layer).
    Out of scope: ``root_weight=False``, ``bias=False`` and other gates.  ``Project`` does not generate such designs."""

    def __init__(self, in_channels: int, out_channels: int, edge_dim: int, p_in: int = 1, p_out: int = 1):
        super().__init__()
        if not isinstance(edge_dim, int) or isinstance(edge_dim, bool) or not 1 <= edge_dim <= 16:
            raise ValueError(f"edge_dim must be an int in 1 .. 16 (got {edge_dim!r})")
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.edge_dim = edge_dim
        self.p_in = p_in
        self.p_out = p_out
        self.conv = _ResGatedGraphEConv(in_channels, out_channels, edge_dim)

    def forward(self, x: Tensor, edge_index: Tensor, edge_attr: Tensor) -> Tensor:
        return self.conv(x, edge_index, edge_attr)


# --------------------------------------------------------------------------------------- GatedGraphConv
class _GatedGraphConv(nn.Module):
    """PyG's ``GatedGraphConv(out_channels, num_layers, aggr='add', bias=True)`` -- the Gated Graph Neural Network of Li et al.,
    the update function of Gilmer's MPNN family; the one layer whose update is recurrent::

        h = [x | 0]                              x [N, in] padded with zero columns to out; in > out: ValueError
        for t in 0 .. num_layers - 1:
            m_i = sum_j (h_j @ weight[t])        weight [num_layers, out, out], a plain matmul; j in N(i), the input's edges
            h   = rnn(m, h)                      ONE torch.nn.GRUCell(out, out), shared by all steps

    No self loop is added and none is removed: an explicit ``(v, v)`` edge is an ordinary edge, duplicate edges count as often
    as they occur, a node without in-edges gets ``rnn(0, h_i)``.  Parameters with PyG's ``state_dict`` names and shapes --
    ``weight``, ``rnn.weight_ih``, ``rnn.weight_hh`` [3 out, out], ``rnn.bias_ih``, ``rnn.bias_hh`` [3 out] --, initialised as
    PyG does (``weight`` uniform in +- 1 / sqrt(out), the cell torch's default).  Out of scope: ``aggr`` other than add,
    ``bias=False``, ``edge_weight``."""

    def __init__(self, in_channels: int, out_channels: int, num_layers: int):
        super().__init__()
        if in_channels > out_channels:
            raise ValueError(f"GatedGraphConv pads its input with zero columns up to out_channels: in_channels ({in_channels}) must not "
                             f"exceed out_channels ({out_channels})")
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.num_layers = num_layers
        self.weight = nn.Parameter(torch.empty(num_layers, out_channels, out_channels))
        self.rnn = nn.GRUCell(out_channels, out_channels, bias=True)
        bound = 1.0 / math.sqrt(out_channels)
        nn.init.uniform_(self.weight, -bound, bound)

    def forward(self, x: Tensor, edge_index: Tensor) -> Tensor:
        if x.size(-1) > self.out_channels:
            raise ValueError("The number of input channels is not allowed to be larger than the number of output channels")
        src, dst = edge_index[0].long(), edge_index[1].long()
        h = x
        if h.size(-1) < self.out_channels:
            h = torch.cat([h, h.new_zeros(h.size(0), self.out_channels - h.size(-1))], dim=1)
        for t in range(self.num_layers):
            m = torch.matmul(h, self.weight[t])
            m = torch.zeros_like(m).index_add(0, dst, m[src])
            h = self.rnn(m, h)
        return h


class GatedGraphConv_GNNB(nn.Module):
    """The gated graph conv (no class of the reference): PyG's ``GatedGraphConv(out_channels, num_layers=steps)``.
    ``GNNModel(..., gnn_conv=GatedGraphConv_GNNB, gnn_steps=T)`` stacks it (``T`` in 1 .. 8 steps per layer, every layer's input
    at most as wide as its output); ``forward(x, edge_index)``.  The accelerated path is ``runtime.CompiledModel.from_model`` with
    the ordinary ``forward`` / ``forward_pyg`` (C ABI ``include/gnnb_ggnn.h``: per step one GEMM ``h -> [p | gh]`` on the message
    weight folded into the GRU's input weight and one launch of csrc/k_ggnn.hip, the whole GRU cell in the aggregate's epilogue).
    This class ignores ``graph_input_edge_dim`` and ``edge_attr``; ``aggr`` other than add, ``bias=False`` and ``edge_weight``
    are out of scope.  ``Project`` does not generate such designs."""

    def __init__(self, in_channels: int, out_channels: int, steps: int = 1, p_in: int = 1, p_out: int = 1):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.steps = steps
        self.p_in = p_in
        self.p_out = p_out
        self.conv = _GatedGraphConv(in_channels, out_channels, steps)

    def forward(self, x: Tensor, edge_index: Tensor) -> Tensor:
        return self.conv(x, edge_index)


# --------------------------------------------------------------------------------------- RGCNConv
class _RGCNConv(nn.Module):
    """PyG's ``RGCNConv(in_channels, out_channels, num_relations, aggr='mean', root_weight=True, bias=True)`` without basis or
    block decomposition -- the relational GCN of Schlichtkrull et al., for graphs whose edges carry an integer type::

        out_i = x_i @ root + bias + sum_{r < R} (1 / |N_r(i)|) * sum_{j in N_r(i)} x_j @ weight[r]

    ``N_r(i)``: the in-edges of ``i`` with type ``r``; duplicate edges count as often as they occur, an explicit ``(v, v)`` edge
    is an ordinary edge, no self loop is added or removed, a relation without an edge into ``i`` contributes 0.  Parameters with
    PyG's ``state_dict`` names and shapes -- ``weight`` [R, in, out], ``root`` [in, out] (both applied as ``x @ W``), ``bias``
    [out] --, initialised as PyG does (glorot, glorot, zeros).  Out of scope: ``num_bases``, ``num_blocks``, ``aggr`` other than
    mean, ``root_weight=False``, ``bias=False``."""

    def __init__(self, in_channels: int, out_channels: int, num_relations: int):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.num_relations = num_relations
        self.weight = nn.Parameter(torch.empty(num_relations, in_channels, out_channels))
        self.root = nn.Parameter(torch.empty(in_channels, out_channels))
        self.bias = nn.Parameter(torch.zeros(out_channels))
        for t in (self.weight, self.root):  # (PyG's glorot: uniform in +- sqrt(6 / (size(-2) + size(-1))))
            bound = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
            nn.init.uniform_(t, -bound, bound)

    def forward(self, x: Tensor, edge_index: Tensor, edge_type: Tensor) -> Tensor:
        src, dst = edge_index[0].long(), edge_index[1].long()
        edge_type = edge_type.reshape(-1).long()
        if edge_type.numel() != src.numel():
            raise ValueError(f"edge_type must hold one type per edge: {src.numel()} edges, {edge_type.numel()} types")
        if edge_type.numel() and (int(edge_type.min()) < 0 or int(edge_type.max()) >= self.num_relations):
            raise ValueError(f"edge_type must lie in [0, {self.num_relations}): got {int(edge_type.min())} .. {int(edge_type.max())}")
        out = x @ self.root + self.bias
        for r in range(self.num_relations):  # (per relation, as PyG evaluates it: the mean of the neighbours, then the transform)
            m = edge_type == r
            s, d = src[m], dst[m]
            cnt = x.new_zeros(x.size(0)).index_add(0, d, x.new_ones(d.numel()))
            h = torch.zeros_like(x).index_add(0, d, x[s]) / cnt.clamp(min=1).unsqueeze(-1)
            out = out + h @ self.weight[r]
        return out


class RGCNConv_GNNB(nn.Module):
    """The relational graph conv (no class of the reference): PyG's ``RGCNConv(in_channels, out_channels, num_relations=R)``.
    ``GNNModel(..., gnn_conv=RGCNConv_GNNB, gnn_relations=R)`` stacks it (``R`` in 1 .. 8); ``forward(x, edge_index, edge_type)``
    with ``edge_type`` int64 [E] in ``[0, R)``, the same for every layer.  The accelerated path is
    ``runtime.CompiledModel.from_model`` with ``forward_types`` / ``forward_pyg_types`` (C ABI ``include/gnnb_rgcn.h``: one GEMM
    ``x -> [p_0 | .. | p_{R-1} | root]`` and one launch of csrc/k_rgcn.hip per layer, one gathered row per edge).  This class
    ignores ``graph_input_edge_dim`` and ``edge_attr``.  ``Project`` does not generate such designs."""

    def __init__(self, in_channels: int, out_channels: int, relations: int = 1, p_in: int = 1, p_out: int = 1):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.relations = relations
        self.p_in = p_in
        self.p_out = p_out
        self.conv = _RGCNConv(in_channels, out_channels, relations)

    def forward(self, x: Tensor, edge_index: Tensor, edge_type: Tensor) -> Tensor:
        return self.conv(x, edge_index, edge_type)


# --------------------------------------------------------------------------------------- pooling / MLP
SUPPORTED_GLOBAL_POOLING_AGGRS = {"add": "SumAggregation", "max": "MaxAggregation", "mean": "MeanAggregation"}
SUPPORTED_GLOBAL_POOLING_MODE = ["cat"]


class GlobalPooling(nn.Module):
    """Concatenation of add / mean / max readouts in the order of ``aggrs``
    (reference models.py:326-359)."""

    def __init__(self, aggrs: List[str], mode: str = "cat"):
        super().__init__()
        self.aggrs = aggrs
        self.mode = mode
        if aggrs == []:
            raise ValueError("GlobalPooling needs at least one aggregation (add / mean / max)")
        for a in self.aggrs:
            if a not in SUPPORTED_GLOBAL_POOLING_AGGRS:
                raise NotImplementedError(
                    f"unknown pooling aggregation {a!r}; choose from {SUPPORTED_GLOBAL_POOLING_AGGRS}")
        if self.mode not in SUPPORTED_GLOBAL_POOLING_MODE:
            raise NotImplementedError(
                f"unknown pooling mode {self.mode!r}; choose from {SUPPORTED_GLOBAL_POOLING_MODE}")

    def forward(self, x: Tensor, index: Optional[Tensor] = None, dim_size: Optional[int] = None) -> Tensor:
        if index is None:  # one graph: [N, d] -> [1, k*d]
            index = torch.zeros(x.size(0), dtype=torch.long, device=x.device)
            dim_size = 1
        if dim_size is None:
            dim_size = int(index.max().item()) + 1 if index.numel() else 0
        d = x.size(1)
        idx = index.unsqueeze(-1).expand(-1, d)
        zeros = x.new_zeros(dim_size, d)
        outs = []
        for a in self.aggrs:
            if a == "add":
                outs.append(zeros.index_add(0, index, x))
            elif a == "mean":
                cnt = torch.zeros(dim_size, dtype=x.dtype, device=x.device).index_add(
                    0, index, torch.ones_like(index, dtype=x.dtype)).clamp(min=1)
                outs.append(zeros.index_add(0, index, x) / cnt.unsqueeze(-1))
            else:
                outs.append(zeros.scatter_reduce(0, idx, x, "amax", include_self=False))
        return torch.cat(outs, dim=-1)

    @property
    def num_of_aggrs(self) -> int:
        return len(self.aggrs)

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}({self.aggrs}, mode={self.mode})"


SUPPORTED_ACTIVATIONS = [nn.ReLU, nn.GELU, nn.Sigmoid, nn.Tanh]
_ACT_NAME = {nn.ReLU: "relu", nn.GELU: "gelu", nn.Sigmoid: "sigmoid", nn.Tanh: "tanh"}


class MLP(nn.Module):
    """Linear -> act, repeated ``hidden_layers`` times, then Linear (reference models.py:365-450)."""

    def __init__(self, in_dim: int, out_dim: int, hidden_dim: int = 64, hidden_layers: int = 2,
                 activation: TorchModuleArg = nn.ReLU, norm_layer: TorchModuleArgOptional = None,
                 p_in: int = 1, p_hidden: int = 1, p_out: int = 1):
        super().__init__()
        self.in_dim = in_dim
        self.out_dim = out_dim
        self.hidden_dim = hidden_dim
        self.hidden_layers = hidden_layers
        self.activation = activation
        self.norm_layer = norm_layer
        if self.activation not in SUPPORTED_ACTIVATIONS:
            raise ValueError(f"MLP activation must be one of {SUPPORTED_ACTIVATIONS}, got {activation}")
        if self.norm_layer is not None:
            raise NotImplementedError("MLP norm_layer: no normalisation layer has a native path (the reference has none either)")
        if hidden_layers < 0:
            raise ValueError(f"MLP hidden_layers cannot be negative (got {hidden_layers})")
        self.p_in = p_in
        self.p_hidden = p_hidden
        self.p_out = p_out

        self.linear_layers = nn.ModuleList()
        self.activations = nn.ModuleList()
        self.norm_layers = nn.ModuleList()
        dims = [in_dim] + [hidden_dim] * hidden_layers + [out_dim]
        for i in range(len(dims) - 1):
            self.linear_layers.append(nn.Linear(dims[i], dims[i + 1]))
            if i < len(dims) - 2:
                self.activations.append(self.activation())
        self.layer_list = []
        for i, lin in enumerate(self.linear_layers):
            self.layer_list.append(lin)
            if i < len(self.linear_layers) - 1:
                self.layer_list.append(self.activations[i])
        self.mlp = nn.Sequential(*self.layer_list)

    def forward(self, x: Tensor) -> Tensor:
        return self.mlp(x)

    @property
    def p_factors(self):
        if self.hidden_layers == 0:
            return [(self.p_in, self.p_out)]
        f = [(self.p_in if i == 0 else self.p_hidden, self.p_hidden) for i in range(self.hidden_layers)]
        f.append((self.p_hidden, self.p_out))
        return f

    @property
    def num_of_layers(self) -> int:
        return len(self.linear_layers)


SUPPORTED_GNN_CONVS = [GCNConv_GNNB, GINConv_GNNB, GATConv_GNNB, PNAConv_GNNB, SAGEConv_GNNB, GINEConv_GNNB, PNAEConv_GNNB,
                       GATv2Conv_GNNB, GATv2EConv_GNNB, TransformerConv_GNNB, TransformerEConv_GNNB, ResGatedGraphConv_GNNB,
                       ResGatedGraphEConv_GNNB, GATv1Conv_GNNB, GATv1EConv_GNNB, GatedGraphConv_GNNB, RGCNConv_GNNB]
_CONV_NAME = {GCNConv_GNNB: "gcn", GINConv_GNNB: "gin", SAGEConv_GNNB: "sage", PNAConv_GNNB: "pna", GINEConv_GNNB: "gine",
              PNAEConv_GNNB: "pnae", GATv2Conv_GNNB: "gatv2", GATv2EConv_GNNB: "gatv2e", TransformerConv_GNNB: "transformer",
              TransformerEConv_GNNB: "transformere", ResGatedGraphConv_GNNB: "resgated", ResGatedGraphEConv_GNNB: "resgatede",
              GATv1Conv_GNNB: "gat", GATv1EConv_GNNB: "gate", GatedGraphConv_GNNB: "ggnn", RGCNConv_GNNB: "rgcn"}
# convs that take edge_attr, and what the messages call them
_EDGE_CONVS = {GINEConv_GNNB: "GINE", PNAEConv_GNNB: "PNAE", GATv2EConv_GNNB: "GATv2E", TransformerEConv_GNNB: "TransformerE",
               ResGatedGraphEConv_GNNB: "ResGatedE", GATv1EConv_GNNB: "GATE"}
MAX_EDGE_DIM = 16  # of a GINE, PNAE, GATv2E, TransformerE, ResGatedE or GATE model (include/gnnb_edge.h, gnnb_pna_edge.h, gnnb_gat_edge.h, gnnb_transformer_edge.h, gnnb_resgated_edge.h, gnnb_gatconv_edge.h)
_GAT_CONVS = (GATv2Conv_GNNB, GATv2EConv_GNNB)  # the GATv2 convs (heads and negative_slope travel beside a GCN description)
_TF_CONVS = (TransformerConv_GNNB, TransformerEConv_GNNB)  # the TransformerConv convs (heads travel beside a GIN description)
_GAT1_CONVS = (GATv1Conv_GNNB, GATv1EConv_GNNB)  # PyG's GATConv (heads and negative_slope travel beside a GCN description: include/gnnb_gatconv.h, gnnb_gatconv_edge.h)
_HEAD_CONVS = _GAT_CONVS + _TF_CONVS + _GAT1_CONVS  # convs with attention heads: the ones that take gnn_heads
MAX_RGCN_RELATIONS = 8  # of an RGCNConv model (include/gnnb_rgcn.h): edge types in [0, relations), beside a GIN description
MAX_GGNN_STEPS = 8  # of a GatedGraphConv model (include/gnnb_ggnn.h): steps per layer, beside a GIN description


class GNNModel(nn.Module):
    """Conv stack (+skip on middle layers, activation after every conv) -> global pooling ->
    MLP head (reference models.py:462-575)."""

    def __init__(self, graph_input_feature_dim: int, graph_input_edge_dim: Optional[int],
                 gnn_hidden_dim: int, gnn_num_layers: int, gnn_output_dim: int,
                 gnn_conv: TorchModuleArg, gnn_activation: TorchModuleArg, gnn_skip_connection: bool,
                 global_pooling: GlobalPooling, mlp_head: MLP,
                 output_activation: TorchModuleArgOptional, gnn_p_in: int = 1, gnn_p_hidden: int = 1,
                 gnn_p_out: int = 1, gnn_heads: int = 1, gnn_steps: int = 1, gnn_relations: int = 1) -> None:
        super().__init__()
        self.graph_input_feature_dim = graph_input_feature_dim
        self.graph_input_edge_dim = graph_input_edge_dim
        self.gnn_hidden_dim = gnn_hidden_dim
        self.gnn_num_layers = gnn_num_layers
        self.gnn_output_dim = gnn_output_dim
        self.gnn_conv = gnn_conv
        if self.gnn_conv not in SUPPORTED_GNN_CONVS:
            raise ValueError(f"gnn_conv {gnn_conv} is not a *_GNNB conv class of this package: {SUPPORTED_GNN_CONVS}")
        self.gnn_activation = gnn_activation
        if self.gnn_activation not in SUPPORTED_ACTIVATIONS:
            raise ValueError(f"gnn_activation {gnn_activation} has no native kernel; choose from {SUPPORTED_ACTIVATIONS}")
        self.gnn_skip_connection = gnn_skip_connection
        conv_kwargs = {}
        if self.gnn_conv in _EDGE_CONVS:
            d = self.graph_input_edge_dim
            if not isinstance(d, int) or isinstance(d, bool) or not 1 <= d <= MAX_EDGE_DIM:
                raise ValueError(f"a {_EDGE_CONVS[self.gnn_conv]} model needs graph_input_edge_dim, an int in 1 .. {MAX_EDGE_DIM} (got {d!r})")
            conv_kwargs = {"edge_dim": d}
            if self.gnn_conv is GINEConv_GNNB:
                conv_kwargs["hidden_dim"] = None  # (the MLP's hidden width = out_channels, as for GIN)

        self.gnn_heads = gnn_heads
        if self.gnn_conv in _HEAD_CONVS:
            if not isinstance(gnn_heads, int) or isinstance(gnn_heads, bool) or not 1 <= gnn_heads <= MAX_GAT_HEADS:
                kind = "TransformerConv" if self.gnn_conv in _TF_CONVS else "GAT" if self.gnn_conv in _GAT1_CONVS else "GATv2"
                raise ValueError(f"a {kind} model needs gnn_heads, an int in 1 .. {MAX_GAT_HEADS} (got {gnn_heads!r})")
            widths = [gnn_output_dim] if gnn_num_layers <= 1 else [gnn_hidden_dim, gnn_output_dim]
            if gnn_num_layers >= 1 and any(w % gnn_heads for w in widths):
                raise ValueError(f"gnn_hidden_dim and gnn_output_dim ({gnn_hidden_dim}, {gnn_output_dim}) must be divisible by "
                                 f"gnn_heads ({gnn_heads})")
            conv_kwargs = {**conv_kwargs, "heads": gnn_heads}  # (GATv2E, TransformerE, GATE: edge_dim from above stays)
        elif gnn_heads != 1:
            raise ValueError(f"gnn_heads={gnn_heads!r}: only a GATv2 model (gnn_conv=GATv2Conv_GNNB) has attention heads")

        self.gnn_steps = gnn_steps
        if self.gnn_conv is GatedGraphConv_GNNB:
            if not isinstance(gnn_steps, int) or isinstance(gnn_steps, bool) or not 1 <= gnn_steps <= MAX_GGNN_STEPS:
                raise ValueError(f"a GatedGraphConv model needs gnn_steps, an int in 1 .. {MAX_GGNN_STEPS} (got {gnn_steps!r})")
            # (h_0 = [x | 0]: a layer pads its input with zero columns and cannot narrow it)
            chain = ([graph_input_feature_dim, gnn_output_dim] if gnn_num_layers == 1 else
                     [graph_input_feature_dim, gnn_hidden_dim, gnn_output_dim] if gnn_num_layers >= 2 else [])
            if any(a > b for a, b in zip(chain, chain[1:])):
                raise ValueError(f"a GatedGraphConv layer's input must not be wider than its output: graph_input_feature_dim <= "
                                 f"gnn_hidden_dim <= gnn_output_dim is needed (got {chain})")
            conv_kwargs = {**conv_kwargs, "steps": gnn_steps}
        elif gnn_steps != 1:
            raise ValueError(f"gnn_steps={gnn_steps!r}: only a GatedGraphConv model (gnn_conv=GatedGraphConv_GNNB) has steps")

        self.gnn_relations = gnn_relations
        if self.gnn_conv is RGCNConv_GNNB:
            if not isinstance(gnn_relations, int) or isinstance(gnn_relations, bool) or not 1 <= gnn_relations <= MAX_RGCN_RELATIONS:
                raise ValueError(f"an RGCNConv model needs gnn_relations, an int in 1 .. {MAX_RGCN_RELATIONS} (got {gnn_relations!r})")
            conv_kwargs = {**conv_kwargs, "relations": gnn_relations}
        elif gnn_relations != 1:
            raise ValueError(f"gnn_relations={gnn_relations!r}: only an RGCNConv model (gnn_conv=RGCNConv_GNNB) has relations")

        self.global_pooling = global_pooling
        self.mlp_head = mlp_head  # registered before gnn_convs: parameter order mlp_head_*, gnn_convs_*
        self.output_activation = output_activation
        self.output_activation_module = None
        if self.output_activation is not None:
            self.output_activation_module = self.output_activation(dim=-1)

        self.gnn_p_in = gnn_p_in
        self.gnn_p_hidden = gnn_p_hidden
        self.gnn_p_out = gnn_p_out

        self.gnn_convs = nn.ModuleList()
        self.gnn_activations = nn.ModuleList()
        L = self.gnn_num_layers
        if L == 0 and self.graph_input_feature_dim != self.gnn_output_dim:
            raise ValueError(
                f"a model without conv layers passes the node features straight to the pooling: gnn_output_dim "
                f"({self.gnn_output_dim}) must equal graph_input_feature_dim ({self.graph_input_feature_dim})")
        for i in range(L):
            if L == 1:
                dims = (self.graph_input_feature_dim, self.gnn_output_dim, self.gnn_p_in, self.gnn_p_out)
            elif i == 0:
                dims = (self.graph_input_feature_dim, self.gnn_hidden_dim, self.gnn_p_in, self.gnn_p_hidden)
            elif i == L - 1:
                dims = (self.gnn_hidden_dim, self.gnn_output_dim, self.gnn_p_hidden, self.gnn_p_out)
            else:
                dims = (self.gnn_hidden_dim, self.gnn_hidden_dim, self.gnn_p_hidden, self.gnn_p_hidden)
            self.gnn_convs.append(self.gnn_conv(dims[0], dims[1], p_in=dims[2], p_out=dims[3], **conv_kwargs))
            self.gnn_activations.append(self.gnn_activation())

    def forward(self, x: Tensor, edge_index: Tensor, batch: Optional[Tensor] = None, edge_attr: Optional[Tensor] = None,
                edge_type: Optional[Tensor] = None) -> Tensor:
        """``batch=None``: one graph -> ``[1, out]``, exactly the reference.  With ``batch``
        (node -> graph index, PyG ``Batch`` convention) every graph is pooled separately ->
        ``[num_graphs, out]``; the reference ignores ``batch`` and pools all nodes into one row
        (models.py:551-553,569; SURVEY finding 3), which has no meaning for independent graphs.
        ``edge_attr`` [E, graph_input_edge_dim]: a GINE, PNAE, GATv2E, TransformerE, ResGatedE or GATE model's edge features, the same for every layer (required
        there; the other convs ignore it).  ``edge_type`` int64 [E] in [0, gnn_relations): an RGCNConv model's edge types, the same
        for every layer (required there; the other convs ignore it)."""
        gine = self.gnn_conv in _EDGE_CONVS
        typed = self.gnn_conv is RGCNConv_GNNB
        if typed and edge_type is None:
            raise ValueError("an RGCNConv model needs edge_type [E], integers in [0, gnn_relations)")
        if gine and edge_attr is None:
            raise ValueError(f"a {_EDGE_CONVS[self.gnn_conv]} model needs edge_attr [E, graph_input_edge_dim]")
        h = x
        for i, (conv, act) in enumerate(zip(self.gnn_convs, self.gnn_activations)):
            h_in = h
            h = conv(h, edge_index, edge_attr) if gine else conv(h, edge_index, edge_type) if typed else conv(h, edge_index)
            if self.gnn_skip_connection and i != 0 and i != self.gnn_num_layers - 1:
                h = h + h_in
            h = act(h)
        pooled = self.global_pooling(h) if batch is None else self.global_pooling(h, batch)
        out = self.mlp_head(pooled)
        if self.output_activation_module is not None:
            out = self.output_activation_module(out)
        return out

    # ------------------------------------------------------------------ introspection (reference models.py:577-634)
    @property
    def input_node_features_dim(self):
        return self.graph_input_feature_dim

    @property
    def input_edge_features_dim(self):
        return self.graph_input_edge_dim

    @property
    def output_features_dim(self):
        return self.mlp_head.out_dim

    @property
    def gnn_layer_sizes(self):
        return [(c.in_channels, c.out_channels) for c in self.gnn_convs]

    @property
    def layers(self):
        return dict(self.named_children())

    @property
    def layer_names(self):
        return {k: f"{k}" for k in self.layers}

    @property
    def layer_parameters(self):
        return {k: list(v.named_parameters()) for k, v in self.layers.items()}

    @property
    def layer_parameters_flat(self):
        return [p for l in self.layer_parameters.values() for p in l]

    @property
    def layer_parameter_names(self):
        return {k: [layer_param_name_combiner(self.layer_names[k], p[0]) for p in v]
                for k, v in self.layer_parameters.items()}

    @property
    def layer_parameter_names_flat(self):
        return [p for l in self.layer_parameter_names.values() for p in l]

    @property
    def layer_parameter_shapes(self):
        return {k: [list(p[1].size()) for p in v] for k, v in self.layer_parameters.items()}

    @property
    def layer_parameter_shapes_flat(self):
        return [p for l in self.layer_parameter_shapes.values() for p in l]

    # ------------------------------------------------------------------ what the MI355X emitter consumes
    def spec(self) -> dict:
        """Plain description of the architecture = the fields of ``gnnb_model_desc``
        (include/gnnb_hip.h)."""
        if self.gnn_conv not in _CONV_NAME:
            raise NotImplementedError(f"{self.gnn_conv.__name__} has no native path")
        out_act = None
        if self.output_activation is not None:
            # the reference builds output_activation(dim=-1) (models.py:500-502): a softmax-like module
            out_act = {nn.Softmax: "softmax", nn.LogSoftmax: "log_softmax"}.get(self.output_activation)
            if out_act is None:
                raise NotImplementedError(f"output_activation {self.output_activation} has no native path "
                                          "(nn.Softmax and nn.LogSoftmax do)")
        conv0 = self.gnn_convs[0] if len(self.gnn_convs) else None
        gat = {}
        if self.gnn_conv in _GAT_CONVS + _GAT1_CONVS:  # (a GCN description on the C side; these two travel beside it: include/gnnb_gat.h, gnnb_gatconv.h)
            gat = {"heads": int(self.gnn_heads), "negative_slope": float(conv0.negative_slope) if conv0 is not None else 0.2}
        elif self.gnn_conv in _TF_CONVS:  # (a GIN description on the C side, heads beside it: include/gnnb_transformer.h, _edge.h)
            gat = {"heads": int(self.gnn_heads)}
        elif self.gnn_conv is GatedGraphConv_GNNB:  # (a GIN description on the C side, steps beside it: include/gnnb_ggnn.h)
            gat = {"steps": int(self.gnn_steps)}
        elif self.gnn_conv is RGCNConv_GNNB:  # (a GIN description on the C side, relations beside it: include/gnnb_rgcn.h)
            gat = {"relations": int(self.gnn_relations)}
        return {
            "conv": _CONV_NAME[self.gnn_conv],
            "num_layers": self.gnn_num_layers,
            "in_dim": self.graph_input_feature_dim,
            "hidden_dim": self.gnn_hidden_dim,
            "out_dim": self.gnn_output_dim,
            "activation": _ACT_NAME[self.gnn_activation],
            "skip": bool(self.gnn_skip_connection),
            "pools": list(self.global_pooling.aggrs),
            "mlp_hidden_layers": self.mlp_head.hidden_layers,
            "mlp_hidden": self.mlp_head.hidden_dim,
            "mlp_out": self.mlp_head.out_dim,
            "mlp_activation": _ACT_NAME[self.mlp_head.activation],
            "gin_eps": float(conv0.eps) if isinstance(conv0, (GINConv_GNNB, GINEConv_GNNB)) else 0.0,
            "edge_dim": int(self.graph_input_edge_dim) if self.gnn_conv in _EDGE_CONVS else 0,
            "pna_delta": float(conv0.delta_scaler) if isinstance(conv0, (PNAConv_GNNB, PNAEConv_GNNB)) else 1.0,
            "output_activation": out_act,
            **gat,
        }

    def canonical_param_names(self) -> List[str]:
        """Flat parameter names (``layer_parameter_names_flat`` style) in the order the C ABI's
        ``gnnb_model_create`` expects: conv layers first, then the head.  (The C side's statement of the same order, and of
        the member each tensor is read under: ``LayerSlots`` in csrc/gnnb_weights.h.)"""
        per_conv = {
            "gcn": ["conv_lin_weight", "conv_bias"],
            "gin": ["mlp_linear_0_weight", "mlp_linear_0_bias", "mlp_linear_1_weight", "mlp_linear_1_bias"],
            "sage": ["conv_lin_l_weight", "conv_lin_l_bias", "conv_lin_r_weight"],
            "pna": ["conv_pre_nns_0_0_weight", "conv_pre_nns_0_0_bias", "conv_post_nns_0_0_weight",
                    "conv_post_nns_0_0_bias", "conv_lin_weight", "conv_lin_bias"],
            "gine": ["mlp_linear_0_weight", "mlp_linear_0_bias", "mlp_linear_1_weight", "mlp_linear_1_bias",
                     "conv_lin_weight", "conv_lin_bias"],  # (conv.lin: the edge projection [in, edge_dim], [in])
        }
        # (PNA's six, then the edge encoder [in, edge_dim], [in]: the base conv's tensors first, the edge tensors behind)
        per_conv["pnae"] = per_conv["pna"] + ["conv_edge_encoder_weight", "conv_edge_encoder_bias"]
        per_conv["gatv2"] = ["conv_lin_l_weight", "conv_lin_l_bias", "conv_lin_r_weight", "conv_lin_r_bias", "conv_att", "conv_bias"]
        per_conv["gatv2e"] = per_conv["gatv2"] + ["conv_lin_edge_weight"]  # (GATv2's six, then lin_edge [out, edge_dim])
        # (PyG's registration order: key, query, value, skip -- the C side stacks them as [W_q ; W_k ; W_v ; W_skip])
        per_conv["transformer"] = [f"conv_lin_{n}_{t}" for n in ("key", "query", "value", "skip") for t in ("weight", "bias")]
        per_conv["transformere"] = per_conv["transformer"] + ["conv_lin_edge_weight"]  # (the eight, then lin_edge [out, edge_dim])
        # (key, query, value with their biases, lin_skip's weight -- it has no bias --, then the conv's own bias: include/gnnb_resgated.h)
        per_conv["resgated"] = [f"conv_lin_{n}_{t}" for n in ("key", "query", "value") for t in ("weight", "bias")] + [
            "conv_lin_skip_weight", "conv_bias"]
        per_conv["resgatede"] = per_conv["resgated"]  # (the same eight; key, query and value weights are [out, in + edge_dim])
        per_conv["gat"] = ["conv_lin_weight", "conv_att_src", "conv_att_dst", "conv_bias"]  # (include/gnnb_gatconv.h)
        # (GAT v1's four, then att_edge [1, heads, out / heads] and lin_edge [out, edge_dim]: include/gnnb_gatconv_edge.h)
        per_conv["gate"] = per_conv["gat"] + ["conv_att_edge", "conv_lin_edge_weight"]
        # (PyG's state_dict order: the per-step message weights [steps, out, out], then the one GRU cell: include/gnnb_ggnn.h)
        per_conv["ggnn"] = ["conv_weight", "conv_rnn_weight_ih", "conv_rnn_weight_hh", "conv_rnn_bias_ih", "conv_rnn_bias_hh"]
        per_conv["rgcn"] = ["conv_weight", "conv_root", "conv_bias"]  # (PyG's state_dict order: include/gnnb_rgcn.h)
        per_conv = per_conv[self.spec()["conv"]]
        names = [f"gnn_convs_{l}_{p}" for l in range(self.gnn_num_layers) for p in per_conv]
        for i in range(self.mlp_head.num_of_layers):
            names += [f"mlp_head_linear_layers_{i}_weight", f"mlp_head_linear_layers_{i}_bias"]
        return names

    def canonical_params(self) -> List[Tensor]:
        by_name = dict(zip(self.layer_parameter_names_flat, [p[1] for p in self.layer_parameters_flat]))
        return [by_name[n].detach() for n in self.canonical_param_names()]
