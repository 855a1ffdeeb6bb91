"""``GNNModel`` stacks ``GINEConv_GNNB`` (the model definition in PyTorch: what a user trains and what the accelerated path,
``runtime.CompiledModel.forward_edges``, is held against in tests/test_hip_gine.py).  No GPU."""
import numpy as np
import pytest
import torch

import gnnbuilder_amd as gnnb
import golden_util as G
from gine_util import edge_attrs, make_gine_model, run
from gnnbuilder_amd.batching import from_pyg_batch
from helpers import batch_vector, edge_batch, make_model


def test_three_layer_gine_model_runs_on_a_packed_batch():
    model = make_gine_model(in_dim=9, edge_dim=3, hidden=32, layers=3, skip=True)
    b = edge_batch(8, 9, seed=1)
    ea = edge_attrs(b.num_edges, 3, seed=2)
    ei = torch.from_numpy(np.ascontiguousarray(b.coo.T.astype(np.int64)))
    with torch.no_grad():
        out = model(torch.from_numpy(b.x), ei, torch.from_numpy(batch_vector(b)), torch.from_numpy(ea))
        kw = model(torch.from_numpy(b.x), ei, batch=torch.from_numpy(batch_vector(b)), edge_attr=torch.from_numpy(ea))
    # (a trailing one-node graph: index.max() + 1 graphs are pooled)
    assert out.shape == (b.num_graphs, 19) and torch.isfinite(out).all() and torch.equal(out, kw)
    assert np.array_equal(out.numpy(), run(model, b, b.x, ea))  # (the layer walk the GPU tests use as their reference)
    # every layer got the edge features: changing them changes the output, and each layer projects them on its own
    with torch.no_grad():
        other = model(torch.from_numpy(b.x), ei, torch.from_numpy(batch_vector(b)), torch.from_numpy(-ea))
    assert not torch.equal(out, other)
    assert [tuple(c.conv.lin.weight.shape) for c in model.gnn_convs] == [(9, 3), (32, 3), (32, 3)]
    assert [c.mlp.hidden_dim for c in model.gnn_convs] == [32, 32, 32]  # (hidden = out_channels, as for GIN)


def test_first_layer_reproduces_the_reference_golden():
    model = make_gine_model(in_dim=G.F, edge_dim=G.EDGE_DIM, hidden=G.F, layers=1, out_dim=G.F)
    layer = model.gnn_convs[0]
    w = G.gine_weights()
    with torch.no_grad():
        layer.conv.eps.fill_(G.conv_kwargs("gine")["eps"])
        for p, v in zip((layer.conv.lin.weight, layer.conv.lin.bias, layer.mlp.linear_0.weight, layer.mlp.linear_0.bias,
                         layer.mlp.linear_1.weight, layer.mlp.linear_1.bias), w):
            p.copy_(torch.from_numpy(v))
        x, coo = G.graph()
        got = layer(torch.from_numpy(x), torch.from_numpy(coo.T.astype(np.int64)), torch.from_numpy(G.edge_features())).numpy()
    assert np.abs(got - G.f32("tb_gine_output", (G.N, G.F))).max() < 1e-6  # (test_oracle_golden.py's bound)


def test_spec_and_parameter_names():
    model = make_gine_model(in_dim=9, edge_dim=3, hidden=32, layers=3)
    spec = model.spec()
    assert spec["conv"] == "gine" and spec["edge_dim"] == 3 and spec["num_layers"] == 3
    assert make_model("gcn", hidden=16).spec()["edge_dim"] == 0 and make_model("gin", hidden=16).spec()["edge_dim"] == 0
    names = model.canonical_param_names()
    per_layer = ["mlp_linear_0_weight", "mlp_linear_0_bias", "mlp_linear_1_weight", "mlp_linear_1_bias", "conv_lin_weight", "conv_lin_bias"]
    assert names[:18] == [f"gnn_convs_{l}_{p}" for l in range(3) for p in per_layer]
    assert names[18:] == [f"mlp_head_linear_layers_{i}_{p}" for i in range(3) for p in ("weight", "bias")]
    shapes = [tuple(p.shape) for p in model.canonical_params()]
    assert shapes[:6] == [(32, 9), (32,), (32, 32), (32,), (9, 3), (9,)]
    assert shapes[6:12] == [(32, 32), (32,), (32, 32), (32,), (32, 3), (32,)]
    assert gnnb.GINEConv_GNNB in gnnb.models.SUPPORTED_GNN_CONVS


def test_a_gine_model_needs_its_edge_features():
    model = make_gine_model()
    b = edge_batch(4, 9, seed=3, hub=False)
    ei = torch.from_numpy(np.ascontiguousarray(b.coo.T.astype(np.int64)))
    with pytest.raises(ValueError, match="edge_attr"):
        model(torch.from_numpy(b.x), ei, torch.from_numpy(batch_vector(b)))
    for bad in (None, 0, 17):
        with pytest.raises(ValueError, match="graph_input_edge_dim"):
            make_gine_model(edge_dim=bad)
    # the other convs ignore the new argument
    gcn = make_model("gcn", in_dim=9, hidden=16)
    with torch.no_grad():
        a = gcn(torch.from_numpy(b.x), ei, torch.from_numpy(batch_vector(b)))
        c = gcn(torch.from_numpy(b.x), ei, torch.from_numpy(batch_vector(b)), edge_attr=torch.zeros(b.num_edges, 3))
    assert torch.equal(a, c)


def test_project_does_not_generate_gine_designs(tmp_path):
    with pytest.raises(NotImplementedError, match="GINE"):
        gnnb.Project("gine", make_gine_model(), "regression", build_dir=tmp_path)


@pytest.mark.parametrize("form", ["batch", "ptr"])
def test_from_pyg_batch_reorders_edge_attributes_with_their_edges(form):
    b = edge_batch(8, 4, seed=5)
    E = b.num_edges
    perm = np.random.default_rng(6).permutation(E)
    ei = np.ascontiguousarray(b.coo.T.astype(np.int64))[:, perm]
    ea = edge_attrs(E, 4, seed=7)  # (row i belongs to shuffled edge i)
    kw = {"batch": batch_vector(b), "num_graphs": b.num_graphs} if form == "batch" else {"ptr": b.node_ptr.astype(np.int64)}
    plain = from_pyg_batch(b.x, ei, **kw)
    gb, ea_ord, order = from_pyg_batch(b.x, ei, edge_attr=ea, return_edge_order=True, **kw)
    gb2, ea_ord2 = from_pyg_batch(b.x, ei, edge_attr=ea, **kw)
    for a, c in ((plain, gb), (plain, gb2)):  # (the default call's result is unchanged)
        assert np.array_equal(a.coo, c.coo) and np.array_equal(a.node_ptr, c.node_ptr) and np.array_equal(a.edge_ptr, c.edge_ptr)
    assert isinstance(plain, type(b)) and np.array_equal(ea_ord, ea_ord2)
    # an independent reordering: every input edge's graph by a linear scan, positions by a stable bucket walk
    graph_of = np.array([int(np.flatnonzero(b.node_ptr[1:] > d)[0]) for d in ei[1]])
    want = [i for g in range(b.num_graphs) for i in range(E) if graph_of[i] == g]
    assert np.array_equal(order, want) and ea_ord.dtype == np.float32 and np.array_equal(ea_ord, ea[want])
    assert np.array_equal(gb.coo, ei.T[want].astype(np.int32))
    with pytest.raises(ValueError, match="edge_attr"):
        from_pyg_batch(b.x, ei, edge_attr=ea[:-1], **kw)
