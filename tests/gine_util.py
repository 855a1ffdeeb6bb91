"""Shared builders of the GINE tests: a seeded ``GNNModel`` of ``GINEConv_GNNB`` layers (``helpers.make_model`` builds the
convs without edge features), seeded edge attributes, and the model's own PyTorch definition evaluated layer by layer the
way ``ref64.run`` does -- every graph of the batch pooled, trailing empty ones included."""
import copy

import numpy as np
import torch

import gnnbuilder_amd as gnnb
import ref64 as R
from helpers import ACTS, batch_vector


def make_gine_model(in_dim=9, edge_dim=3, hidden=32, layers=3, out_dim=None, act="relu", skip=True, pools=("add", "mean", "max"),
                    mlp_hidden=64, mlp_layers=2, task_out=19, out_act=None, seed=0):
    torch.manual_seed(seed)
    out_dim = hidden if out_dim is None else out_dim
    model = gnnb.GNNModel(in_dim, edge_dim, hidden, layers, out_dim, gnnb.GINEConv_GNNB, ACTS[act], skip,
                          gnnb.GlobalPooling(list(pools)), gnnb.MLP(len(pools) * out_dim, task_out, mlp_hidden, mlp_layers), out_act)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("bias"):
                p.uniform_(-0.1, 0.1)
    return model.eval()


def edge_attrs(num_edges, edge_dim, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (num_edges, edge_dim)).astype(np.float32)


def stage_weights(width, edge_dim, seed):
    """(w_edge [width, edge_dim], b_edge [width]) uniform(-0.5, 0.5), as ``test_hip_gine._stage_case`` draws them."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.5, 0.5, (width, edge_dim)).astype(np.float32), rng.uniform(-0.5, 0.5, width).astype(np.float32)


# The in-degrees at which k_gine_aggregate changes behaviour: <= GINE_R = 4 (every slot preloaded), <= GINE_CHUNK = 64 (one
# piece, plain slot order), above (pieces of 64 over the workgroup's lane groups)
DEGREE_CLASSES = (("deg<=4", 0, 4), ("deg5-64", 5, 64), ("deg>64", 65, None))


def degree_classes(coo, num_nodes):
    """{class name: boolean row mask} of the non-empty ``DEGREE_CLASSES`` over the in-degrees of ``coo``."""
    deg = np.bincount(np.asarray(coo).reshape(-1, 2)[:, 1], minlength=num_nodes)[:num_nodes]
    masks = {name: (deg >= lo) & (deg <= (deg.max() if hi is None else hi)) for name, lo, hi in DEGREE_CLASSES}
    return {name: m for name, m in masks.items() if m.any()}


def budget_by_degree(got, ref, base, coo, what=""):
    """``ref64.budget`` (K = 4, F = 2^-22) on the rows of every in-degree class -- each with its own ``max|ref|``, so that a
    hub's sum does not set the scale of a molecule's row -- and on the whole array.  Every figure is printed before the first
    assertion; returns {class or "all": e / e32}."""
    got, ref, base = (np.asarray(a) for a in (got, ref, base))
    parts = dict(degree_classes(coo, ref.shape[0]), all=np.ones(ref.shape[0], bool))
    out = {}
    for name, m in parts.items():
        e, e32, _ = R.errors(got[m], ref[m], base[m])
        out[name] = R.ratio(e, e32)
        print(f"{what}/{name}: rows {int(m.sum())}, s = {np.abs(ref[m]).max():.4g}, e = {e:.3e}, e32 = {e32:.3e}, e / e32 = {out[name]:.2f}")
    for name, m in parts.items():
        R.budget(got[m], ref[m], base[m], what=f"{what}/{name}")
    return out


def run(model, batch, x, edge_attr):
    """The whole GINE model as it stands (its own dtype): ``ref64.run`` with ``edge_attr`` handed to every layer."""
    dtype = next(model.parameters()).dtype
    ei = R.edge_index(batch.coo)
    h = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)
    ea = torch.from_numpy(np.ascontiguousarray(edge_attr)).to(dtype)
    with torch.no_grad():
        for i, (conv, act) in enumerate(zip(model.gnn_convs, model.gnn_activations)):
            h_in = h
            h = conv(h, ei, ea)
            if model.gnn_skip_connection and i != 0 and i != model.gnn_num_layers - 1:
                h = h + h_in
            h = act(h)
        pooled = model.global_pooling(h, torch.from_numpy(batch_vector(batch)), batch.num_graphs)
        out = model.mlp_head(pooled)
        if model.output_activation_module is not None:
            out = model.output_activation_module(out)
    return out.numpy()


def forward64(model, batch, x, edge_attr):
    """The float64 reference: the model's own definition on a ``.double()`` copy."""
    return run(copy.deepcopy(model).double(), batch, x, edge_attr)
