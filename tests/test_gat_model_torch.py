"""``GATv1Conv_GNNB`` -- PyG's ``GATConv`` in plain torch -- and ``GNNModel`` stacking it (the model definition: what a user trains
and what the accelerated path, ``runtime.CompiledModel.forward``, is held against in tests/test_hip_gat.py).  No GPU."""
import numpy as np
import pytest
import torch

import gnnbuilder_amd as gnnb
from gat_util import gat_ref, make_gat_model
from gnnbuilder_amd import synthetic
from gnnbuilder_amd.batching import pack_graphs
from helpers import looped_graph, make_model


def _conv_operands(conv, x):
    """(xl, s_src, s_dst, bias) of ``conv`` (a ``GATv1Conv_GNNB`` in float64) on ``x``, as float64 arrays: the linear and both
    per-node scores are plain products here, so that ``gat_ref`` restates everything behind them."""
    sd = {k: v.numpy().astype(np.float64) for k, v in conv.state_dict().items()}
    xl = np.asarray(x, np.float64) @ sd["conv.lin.weight"].T
    h = conv.heads
    x3 = xl.reshape(xl.shape[0], h, -1)
    return xl, (x3 * sd["conv.att_src"]).sum(-1), (x3 * sd["conv.att_dst"]).sum(-1), sd["conv.bias"]


def _randomise_biases(conv, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in conv.named_parameters():
            if n.endswith("bias"):
                p.copy_(torch.rand(p.shape, generator=g, dtype=p.dtype) * 0.2 - 0.1)


def _qm9_like(fin, seed):
    b = synthetic.make_batch("qm9", 6, seed=seed)
    rng = np.random.default_rng(seed)
    return pack_graphs([(rng.uniform(-1, 1, (b.graph(g)[0].shape[0], fin)).astype(np.float32), b.graph(g)[1]) for g in range(6)])


def _apply(conv, x, coo):
    with torch.no_grad():
        return conv(torch.from_numpy(np.asarray(x)).to(next(conv.parameters()).dtype),
                    torch.from_numpy(np.ascontiguousarray(np.asarray(coo).reshape(-1, 2).T.astype(np.int64)))).numpy()


@pytest.mark.parametrize("fin,fout,heads,slope", [(9, 16, 1, 0.2), (11, 24, 4, 0.2), (7, 9, 3, 0.05)])
@pytest.mark.parametrize("graph", ["qm9", "looped"])
def test_conv_matches_the_two_pass_restatement_in_float64(fin, fout, heads, slope, graph):
    torch.manual_seed(fin)
    conv = gnnb.GATv1Conv_GNNB(fin, fout, heads=heads, negative_slope=slope).double()
    _randomise_biases(conv, fin)
    if graph == "qm9":
        b = _qm9_like(fin, seed=fin)
        x, coo = b.x, b.coo
    else:
        x, coo = looped_graph(40, fin, seed=fin)
        assert (coo[:, 0] == coo[:, 1]).sum() >= 10  # explicit self loops, one node with two
    got = _apply(conv, x, coo)
    xl, s_src, s_dst, bias = _conv_operands(conv, x)
    want = gat_ref(xl, s_src, s_dst, bias, None, "none", coo, heads, slope)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"GATv1Conv_GNNB ({fin}, {fout}, heads {heads}) on {graph} against the two-pass restatement: {err:.3e} relative")
    assert got.shape == (x.shape[0], fout) and err <= 1e-12


def test_conv_matches_a_dense_per_node_restatement():
    """Node by node with a dense adjacency: the closed neighbourhood's scores, their softmax and the weighted sum, in float64."""
    torch.manual_seed(4)
    heads, fout, slope = 3, 12, 0.2
    conv = gnnb.GATv1Conv_GNNB(9, fout, heads=heads, negative_slope=slope).double()
    _randomise_biases(conv, 5)
    x, coo = looped_graph(40, 9, seed=5)
    xl, s_src, s_dst, bias = _conv_operands(conv, x)
    n, c = x.shape[0], fout // heads
    mult = np.zeros((n, n))  # mult[i, j]: how often i attends j -- a repeated (j, i) edge as often as it occurs, i itself once
    e = coo[coo[:, 0] != coo[:, 1]]
    np.add.at(mult, (e[:, 1], e[:, 0]), 1.0)
    mult[np.arange(n), np.arange(n)] = 1.0
    want = np.zeros((n, fout))
    for i in range(n):
        for h in range(heads):
            z = s_src[:, h] + s_dst[i, h]
            s = np.where(z > 0, z, slope * z)
            w = mult[i] * np.exp(s - s[mult[i] > 0].max())
            a = w / (w.sum() + 1e-16)
            want[i, h * c:(h + 1) * c] = a @ xl[:, h * c:(h + 1) * c]
    want += bias
    assert np.abs(_apply(conv, x, coo) - want).max() <= 1e-12


def test_explicit_self_loops_change_nothing():
    torch.manual_seed(1)
    conv = gnnb.GATv1Conv_GNNB(9, 16, heads=2).double()
    x, coo = looped_graph(40, 9, seed=2)
    loops = coo[:, 0] == coo[:, 1]
    assert loops.sum() >= 10
    assert np.array_equal(_apply(conv, x, coo), _apply(conv, x, coo[~loops]))


def test_a_node_without_in_edges_gives_lin_plus_bias():
    torch.manual_seed(2)
    conv = gnnb.GATv1Conv_GNNB(9, 16, heads=4).double()
    _randomise_biases(conv, 3)
    x, coo = looped_graph(40, 9, seed=3)
    deg = np.bincount(coo[coo[:, 0] != coo[:, 1]][:, 1], minlength=40)
    lone = np.flatnonzero(deg == 0)
    assert len(lone) >= 3
    xl, _, _, bias = _conv_operands(conv, x)
    got = _apply(conv, x, coo)
    assert np.abs(got[lone] - (xl[lone] + bias)).max() <= 1e-15  # (softmax over the self term alone: the weight is 1 / (1 + 1e-16))


def test_with_zero_attention_the_layer_is_the_mean_over_the_closed_neighbourhood():
    torch.manual_seed(3)
    conv = gnnb.GATv1Conv_GNNB(9, 12, heads=3).double()
    _randomise_biases(conv, 4)
    with torch.no_grad():
        conv.conv.att_src.zero_()
        conv.conv.att_dst.zero_()
    x, coo = looped_graph(40, 9, seed=4)
    xl, _, _, bias = _conv_operands(conv, x)
    e = coo[coo[:, 0] != coo[:, 1]]
    want = xl.copy()
    np.add.at(want, e[:, 1], xl[e[:, 0]])
    want = want / (1.0 + np.bincount(e[:, 1], minlength=40))[:, None] + bias
    assert np.abs(_apply(conv, x, coo) - want).max() <= 1e-13


def test_state_dict_names_shapes_and_initialisation():
    torch.manual_seed(0)
    conv = gnnb.GATv1Conv_GNNB(9, 32, heads=4)
    sd = {k: tuple(v.shape) for k, v in conv.state_dict().items()}
    assert sd == {"conv.att_src": (1, 4, 8), "conv.att_dst": (1, 4, 8), "conv.bias": (32,), "conv.lin.weight": (32, 9)}  # PyG's names
    assert not conv.state_dict()["conv.bias"].any()  # PyG: the bias zero, the weight and both att glorot
    for name, bound in (("conv.lin.weight", (6 / (32 + 9)) ** 0.5), ("conv.att_src", (6 / (4 + 8)) ** 0.5), ("conv.att_dst", (6 / (4 + 8)) ** 0.5)):
        v = conv.state_dict()[name]
        assert v.abs().max() <= bound and v.abs().max() > 0.5 * bound
    assert not torch.equal(conv.state_dict()["conv.att_src"], conv.state_dict()["conv.att_dst"])
    assert conv.heads == 4 and conv.negative_slope == 0.2 and conv.in_channels == 9 and conv.out_channels == 32


def test_gnn_model_spec_and_parameter_names():
    model = make_gat_model(in_dim=9, hidden=32, layers=3, heads=4)
    spec = model.spec()
    assert spec["conv"] == "gat" and spec["heads"] == 4 and spec["negative_slope"] == 0.2 and spec["num_layers"] == 3
    assert spec["edge_dim"] == 0
    assert "heads" not in make_model("gcn", hidden=16).spec()  # (the other convs' specs are what they were)
    assert gnnb.GATv1Conv_GNNB in gnnb.models.SUPPORTED_GNN_CONVS and "GATv1Conv_GNNB" in gnnb.__all__
    assert gnnb.models._CONV_NAME[gnnb.GATv1Conv_GNNB] == "gat" and gnnb.GATv1Conv_GNNB in gnnb.models._HEAD_CONVS
    names = model.canonical_param_names()
    per_layer = ["conv_lin_weight", "conv_att_src", "conv_att_dst", "conv_bias"]
    assert names[:12] == [f"gnn_convs_{l}_{p}" for l in range(3) for p in per_layer]
    assert names[12:] == [f"mlp_head_linear_layers_{i}_{p}" for i in range(3) for p in ("weight", "bias")]
    shapes = [tuple(p.shape) for p in model.canonical_params()]
    assert shapes[:4] == [(32, 9), (1, 4, 8), (1, 4, 8), (32,)]
    assert shapes[4:8] == [(32, 32), (1, 4, 8), (1, 4, 8), (32,)]
    b = _qm9_like(9, seed=5)
    with torch.no_grad():
        out = model(torch.from_numpy(b.x), torch.from_numpy(np.ascontiguousarray(b.coo.T.astype(np.int64))),
                    torch.from_numpy(np.repeat(np.arange(b.num_graphs), np.diff(b.node_ptr)).astype(np.int64)))
    assert out.shape == (b.num_graphs, 19) and torch.isfinite(out).all()
    one = make_gat_model(heads=1)  # (gnn_heads defaults to 1)
    assert one.spec()["heads"] == 1 and tuple(one.gnn_convs[0].state_dict()["conv.att_src"].shape) == (1, 1, 32)
    # the skip connection on the middle layer, restated: layer by layer with the convs themselves
    skip, plain = make_gat_model(layers=3, heads=2, skip=True, seed=3), make_gat_model(layers=3, heads=2, skip=False, seed=3)
    x, ei = torch.from_numpy(b.x), torch.from_numpy(np.ascontiguousarray(b.coo.T.astype(np.int64)))
    with torch.no_grad():
        h0 = torch.relu(skip.gnn_convs[0](x, ei))
        h1 = torch.relu(skip.gnn_convs[1](h0, ei) + h0)
        h2 = torch.relu(skip.gnn_convs[2](h1, ei))
        want = skip.mlp_head(skip.global_pooling(h2))
        assert torch.allclose(skip(x, ei), want, atol=1e-6) and not torch.allclose(plain(x, ei), want, atol=1e-6)


def test_value_errors():
    with pytest.raises(ValueError, match="divisible"):
        gnnb.GATv1Conv_GNNB(9, 30, heads=4)
    for bad in (0, 9, -1, 2.0, True):
        with pytest.raises(ValueError, match="heads"):
            gnnb.GATv1Conv_GNNB(9, 32, heads=bad)
    with pytest.raises(ValueError, match="divisible"):
        make_gat_model(hidden=30, out_dim=32, heads=4)
    with pytest.raises(ValueError, match="divisible"):
        make_gat_model(hidden=32, out_dim=30, heads=4)
    with pytest.raises(ValueError, match="a GAT model needs gnn_heads"):
        make_gat_model(heads=9)
    for bad in (0, 2.0, True):
        with pytest.raises(ValueError, match="gnn_heads"):
            make_gat_model(heads=bad)
    # a one-layer model has no hidden width to divide
    assert make_gat_model(hidden=30, out_dim=32, layers=1, heads=4).spec()["out_dim"] == 32
    # the reference's stub stays a stub, names GATv2Conv_GNNB as before and now the new class too
    with pytest.raises(NotImplementedError):
        gnnb.GATConv_GNNB(4, 4)
    assert "GATv2Conv_GNNB" in gnnb.GATConv_GNNB.__doc__ and "GATv1Conv_GNNB" in gnnb.GATConv_GNNB.__doc__
    with pytest.raises(NotImplementedError):
        gnnb.GNNModel(9, None, 16, 2, 16, gnnb.GATConv_GNNB, torch.nn.ReLU, True, gnnb.GlobalPooling(["add"]), gnnb.MLP(16, 2), None)


def test_project_does_not_generate_gat_designs(tmp_path):
    with pytest.raises(NotImplementedError, match="GAT designs"):
        gnnb.Project("gat", make_gat_model(), "regression", build_dir=tmp_path)


def test_equal_to_pyg_after_load_state_dict():
    pyg_nn = pytest.importorskip("torch_geometric.nn")
    torch.manual_seed(5)
    ours = gnnb.GATv1Conv_GNNB(9, 24, heads=3, negative_slope=0.2).double()
    _randomise_biases(ours, 6)
    theirs = pyg_nn.GATConv(9, 8, heads=3, concat=True, negative_slope=0.2, add_self_loops=True, bias=True).double()
    theirs.load_state_dict({k[len("conv."):]: v for k, v in ours.state_dict().items()})
    x, coo = looped_graph(40, 9, seed=6)
    ei = torch.from_numpy(np.ascontiguousarray(coo.T.astype(np.int64)))
    with torch.no_grad():
        want = theirs(torch.from_numpy(x).double(), ei).numpy()
    assert np.abs(_apply(ours, x, coo) - want).max() <= 1e-12
