"""``GATv1EConv_GNNB`` -- PyG's ``GATConv(edge_dim=d)`` in plain torch -- and ``GNNModel`` stacking it (the model definition: what a
user trains and what the accelerated path, ``runtime.CompiledModel.forward_edges``, is held against in tests/test_hip_gate.py).
No GPU."""
import numpy as np
import pytest
import torch

import gnnbuilder_amd as gnnb
from gat_util import make_gat_model
from gate_util import fold_edge, gate_ref, make_gate_model
from gnnbuilder_amd import synthetic
from gnnbuilder_amd.batching import pack_graphs
from helpers import looped_graph, make_model


def _conv_operands(conv, x):
    """(xl, s_src, s_dst, a_edge, bias) of ``conv`` (a ``GATv1EConv_GNNB`` in float64) on ``x``, as float64 arrays: plain products
    here, so that ``gate_ref`` restates everything behind them."""
    sd = {k: v.numpy().astype(np.float64) for k, v in conv.state_dict().items()}
    xl = np.asarray(x, np.float64) @ sd["conv.lin.weight"].T
    h = conv.heads
    x3 = xl.reshape(xl.shape[0], h, -1)
    return (xl, (x3 * sd["conv.att_src"]).sum(-1), (x3 * sd["conv.att_dst"]).sum(-1),
            fold_edge(sd["conv.lin_edge.weight"], sd["conv.att_edge"], h), sd["conv.bias"])


def _randomise_biases(conv, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in conv.named_parameters():
            if n.endswith("bias"):
                p.copy_(torch.rand(p.shape, generator=g, dtype=p.dtype) * 0.2 - 0.1)


def _apply(conv, x, coo, ea):
    dt = next(conv.parameters()).dtype
    with torch.no_grad():
        return conv(torch.from_numpy(np.asarray(x)).to(dt), torch.from_numpy(np.ascontiguousarray(np.asarray(coo).reshape(-1, 2).T.astype(np.int64))),
                    torch.from_numpy(np.asarray(ea)).to(dt)).numpy()


def _attrs(num_edges, d, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (num_edges, d))


def test_conv_on_a_hand_made_graph():
    """Five nodes: node 0 has no in-edge, node 3 has three (one of them twice from node 1), node 4 an explicit self loop."""
    torch.manual_seed(1)
    heads, fout, d, slope = 2, 8, 3, 0.2
    conv = gnnb.GATv1EConv_GNNB(5, fout, edge_dim=d, heads=heads, negative_slope=slope).double()
    _randomise_biases(conv, 2)
    coo = np.array([[0, 1], [1, 3], [2, 3], [1, 3], [4, 4], [0, 2], [3, 4]], np.int64)
    deg = np.bincount(coo[coo[:, 0] != coo[:, 1]][:, 1], minlength=5)
    assert deg[0] == 0 and deg[3] == 3
    x, ea = np.random.default_rng(3).uniform(-1, 1, (5, 5)), _attrs(len(coo), d, 4)
    xl, s_src, s_dst, a_edge, bias = _conv_operands(conv, x)
    got = _apply(conv, x, coo, ea)
    want = gate_ref(xl, s_src, s_dst, a_edge, bias, None, "none", coo, ea, heads, slope)
    assert got.shape == (5, fout) and np.abs(got - want).max() <= 1e-13
    assert np.abs(got[0] - (xl[0] + bias)).max() <= 1e-15  # in-degree 0: the self term alone
    # node 3 by hand: three in-edges and the self loop with the mean of their attributes
    rows = [1, 2, 3]
    mean = ea[rows].mean(0)
    for h in range(heads):
        z = np.array([s_src[coo[r, 0], h] + s_dst[3, h] + a_edge[h] @ ea[r] for r in rows] + [s_src[3, h] + s_dst[3, h] + a_edge[h] @ mean])
        s = np.where(z > 0, z, slope * z)
        a = np.exp(s - s.max())
        a /= a.sum() + 1e-16
        c = fout // heads
        cols = slice(h * c, (h + 1) * c)
        want3 = a[:3] @ xl[coo[rows, 0]][:, cols] + a[3] * xl[3, cols] + bias[cols]
        assert np.abs(got[3, cols] - want3).max() <= 1e-13
    # fill = 0 is another layer
    assert np.abs(gate_ref(xl, s_src, s_dst, a_edge, bias, None, "none", coo, ea, heads, slope, fill=0) - want).max() > 1e-4


@pytest.mark.parametrize("fin,fout,heads,d,slope", [(9, 16, 1, 4, 0.2), (11, 24, 4, 3, 0.2), (7, 9, 3, 16, 0.05)])
def test_conv_matches_the_two_pass_restatement_on_a_looped_graph(fin, fout, heads, d, slope):
    torch.manual_seed(fin)
    conv = gnnb.GATv1EConv_GNNB(fin, fout, edge_dim=d, heads=heads, negative_slope=slope).double()
    _randomise_biases(conv, fin)
    x, coo = looped_graph(40, fin, seed=fin)
    assert (coo[:, 0] == coo[:, 1]).sum() >= 10  # explicit self loops, one node with two
    ea = _attrs(len(coo), d, fin)
    xl, s_src, s_dst, a_edge, bias = _conv_operands(conv, x)
    want = gate_ref(xl, s_src, s_dst, a_edge, bias, None, "none", coo, ea, heads, slope)
    got = _apply(conv, x, coo, ea)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"GATv1EConv_GNNB ({fin}, {fout}, heads {heads}, edge_dim {d}) against the two-pass restatement: {err:.3e} relative")
    assert got.shape == (x.shape[0], fout) and err <= 1e-12


def test_explicit_self_loops_with_nan_attributes_change_nothing():
    torch.manual_seed(1)
    conv = gnnb.GATv1EConv_GNNB(9, 16, edge_dim=4, heads=2).double()
    x, coo = looped_graph(40, 9, seed=2)
    loops = coo[:, 0] == coo[:, 1]
    assert loops.sum() >= 10
    ea = _attrs(len(coo), 4, 3)
    poisoned = ea.copy()
    poisoned[loops] = np.nan
    got = _apply(conv, x, coo, poisoned)
    assert np.isfinite(got).all() and np.array_equal(got, _apply(conv, x, coo[~loops], ea[~loops]))


def test_without_edges_every_row_is_lin_plus_bias():
    torch.manual_seed(2)
    conv = gnnb.GATv1EConv_GNNB(9, 16, edge_dim=4, heads=4).double()
    _randomise_biases(conv, 3)
    x = np.random.default_rng(4).uniform(-1, 1, (7, 9))
    xl, _, _, _, bias = _conv_operands(conv, x)
    got = _apply(conv, x, np.zeros((0, 2), np.int64), np.zeros((0, 4)))
    assert np.abs(got - (xl + bias)).max() <= 1e-15  # (softmax over the self term alone: the weight is 1 / (1 + 1e-16))


def test_state_dict_names_shapes_and_initialisation():
    torch.manual_seed(0)
    conv = gnnb.GATv1EConv_GNNB(9, 32, edge_dim=5, heads=4)
    sd = {k: tuple(v.shape) for k, v in conv.state_dict().items()}
    assert sd == {"conv.att_src": (1, 4, 8), "conv.att_dst": (1, 4, 8), "conv.att_edge": (1, 4, 8), "conv.bias": (32,),
                  "conv.lin.weight": (32, 9), "conv.lin_edge.weight": (32, 5)}  # PyG's names
    assert not conv.state_dict()["conv.bias"].any()
    for name, bound in (("conv.lin_edge.weight", (6 / (32 + 5)) ** 0.5), ("conv.att_edge", (6 / (4 + 8)) ** 0.5)):
        v = conv.state_dict()[name]
        assert v.abs().max() <= bound and v.abs().max() > 0.5 * bound
    assert conv.heads == 4 and conv.negative_slope == 0.2 and conv.in_channels == 9 and conv.out_channels == 32 and conv.edge_dim == 5


def test_gnn_model_spec_and_parameter_names():
    model = make_gate_model(in_dim=9, edge_dim=4, hidden=32, layers=3, heads=4)
    spec = model.spec()
    assert spec["conv"] == "gate" and spec["heads"] == 4 and spec["negative_slope"] == 0.2 and spec["num_layers"] == 3
    assert spec["edge_dim"] == 4
    assert gnnb.GATv1EConv_GNNB in gnnb.models.SUPPORTED_GNN_CONVS and "GATv1EConv_GNNB" in gnnb.__all__
    assert gnnb.models._CONV_NAME[gnnb.GATv1EConv_GNNB] == "gate" and gnnb.GATv1EConv_GNNB in gnnb.models._HEAD_CONVS
    assert gnnb.GATv1EConv_GNNB in gnnb.models._EDGE_CONVS
    names = model.canonical_param_names()
    per_layer = ["conv_lin_weight", "conv_att_src", "conv_att_dst", "conv_bias", "conv_att_edge", "conv_lin_edge_weight"]
    assert names[:18] == [f"gnn_convs_{l}_{p}" for l in range(3) for p in per_layer]
    assert names[18:] == [f"mlp_head_linear_layers_{i}_{p}" for i in range(3) for p in ("weight", "bias")]
    shapes = [tuple(p.shape) for p in model.canonical_params()]
    assert shapes[:6] == [(32, 9), (1, 4, 8), (1, 4, 8), (32,), (1, 4, 8), (32, 4)]
    assert shapes[6:12] == [(32, 32), (1, 4, 8), (1, 4, 8), (32,), (1, 4, 8), (32, 4)]
    # every layer has its own lin_edge / att_edge, all fed the same edge_attr
    assert not torch.equal(model.gnn_convs[0].conv.att_edge, model.gnn_convs[1].conv.att_edge)
    b = synthetic.make_batch("qm9", 6, seed=5)
    rng = np.random.default_rng(5)
    b = pack_graphs([(rng.uniform(-1, 1, (b.graph(g)[0].shape[0], 9)).astype(np.float32), b.graph(g)[1]) for g in range(6)])
    x, ei = torch.from_numpy(b.x), torch.from_numpy(np.ascontiguousarray(b.coo.T.astype(np.int64)))
    batch = torch.from_numpy(np.repeat(np.arange(b.num_graphs), np.diff(b.node_ptr)).astype(np.int64))
    ea = torch.from_numpy(rng.uniform(-1, 1, (b.num_edges, 4)).astype(np.float32))
    with torch.no_grad():
        out = model(x, ei, batch, ea)
        assert out.shape == (b.num_graphs, 19) and torch.isfinite(out).all()
        assert not torch.allclose(model(x, ei, batch, torch.zeros_like(ea)), out, atol=1e-6)  # the attributes matter
        with pytest.raises(ValueError, match="needs edge_attr"):
            model(x, ei, batch)
        # the skip connection on the middle layer, restated: layer by layer with the convs themselves
        h0 = torch.relu(model.gnn_convs[0](x, ei, ea))
        h1 = torch.relu(model.gnn_convs[1](h0, ei, ea) + h0)
        h2 = torch.relu(model.gnn_convs[2](h1, ei, ea))
        assert torch.allclose(model(x, ei, None, ea), model.mlp_head(model.global_pooling(h2)), atol=1e-6)


def test_the_plain_gat_model_is_what_it_was():
    model = make_gat_model(in_dim=9, hidden=32, layers=2, heads=4)
    spec = model.spec()
    assert spec["conv"] == "gat" and spec["edge_dim"] == 0 and gnnb.GATv1Conv_GNNB not in gnnb.models._EDGE_CONVS
    assert model.canonical_param_names()[:4] == [f"gnn_convs_0_{p}" for p in ("conv_lin_weight", "conv_att_src", "conv_att_dst", "conv_bias")]
    assert set(model.gnn_convs[0].state_dict()) == {"conv.att_src", "conv.att_dst", "conv.bias", "conv.lin.weight"}
    # with zero att_edge the edge model is the plain one on the same tensors
    torch.manual_seed(3)
    e = gnnb.GATv1EConv_GNNB(9, 16, edge_dim=4, heads=2).double()
    p = gnnb.GATv1Conv_GNNB(9, 16, heads=2).double()
    with torch.no_grad():
        e.conv.att_edge.zero_()
    p.load_state_dict({k: v for k, v in e.state_dict().items() if "edge" not in k})
    x, coo = looped_graph(40, 9, seed=4)
    ei = torch.from_numpy(np.ascontiguousarray(coo.T.astype(np.int64)))
    with torch.no_grad():
        assert torch.allclose(p(torch.from_numpy(x).double(), ei), torch.from_numpy(_apply(e, x, coo, _attrs(len(coo), 4, 5))), atol=1e-13)


def test_value_errors():
    with pytest.raises(ValueError, match="divisible"):
        gnnb.GATv1EConv_GNNB(9, 30, edge_dim=4, heads=4)
    for bad in (0, 9, -1, 2.0, True):
        with pytest.raises(ValueError, match="heads"):
            gnnb.GATv1EConv_GNNB(9, 32, edge_dim=4, heads=bad)
    for bad in (0, 17, -1, 4.0, True, None):
        with pytest.raises(ValueError, match="edge_dim"):
            gnnb.GATv1EConv_GNNB(9, 32, edge_dim=bad, heads=4)
    for bad in (None, 0, 17):
        with pytest.raises(ValueError, match="a GATE model needs graph_input_edge_dim"):
            make_gate_model(edge_dim=bad)
    with pytest.raises(ValueError, match="divisible"):
        make_gate_model(hidden=30, out_dim=32, heads=4)
    with pytest.raises(ValueError, match="a GAT model needs gnn_heads"):
        make_gate_model(heads=9)
    for bad in (0, 2.0, True):
        with pytest.raises(ValueError, match="gnn_heads"):
            make_gate_model(heads=bad)
    assert make_gate_model(edge_dim=16, heads=8).spec()["edge_dim"] == 16
    # the reference's stub stays a stub
    with pytest.raises(NotImplementedError):
        gnnb.GATConv_GNNB(4, 4)
    assert "GATv1EConv_GNNB" in gnnb.GATConv_GNNB.__doc__
    assert make_model("gcn", hidden=16).spec()["edge_dim"] == 0  # (the other convs' specs are what they were)


def test_project_does_not_generate_such_designs(tmp_path):
    with pytest.raises(NotImplementedError, match="GAT designs with edge features"):
        gnnb.Project("gate", make_gate_model(), "regression", build_dir=tmp_path)


def test_equal_to_pyg_after_load_state_dict():
    pyg_nn = pytest.importorskip("torch_geometric.nn")
    torch.manual_seed(5)
    ours = gnnb.GATv1EConv_GNNB(9, 24, edge_dim=4, heads=3, negative_slope=0.2).double()
    _randomise_biases(ours, 6)
    theirs = pyg_nn.GATConv(9, 8, heads=3, concat=True, negative_slope=0.2, add_self_loops=True, bias=True, edge_dim=4,
                            fill_value="mean").double()
    theirs.load_state_dict({k[len("conv."):]: v for k, v in ours.state_dict().items()})
    x, coo = looped_graph(40, 9, seed=6)
    ea = _attrs(len(coo), 4, 7)
    ei = torch.from_numpy(np.ascontiguousarray(coo.T.astype(np.int64)))
    with torch.no_grad():
        want = theirs(torch.from_numpy(x).double(), ei, torch.from_numpy(ea)).numpy()
    assert np.abs(_apply(ours, x, coo, ea) - want).max() <= 1e-12
