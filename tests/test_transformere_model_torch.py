"""``TransformerEConv_GNNB`` -- PyG's ``TransformerConv(edge_dim=d)`` in plain torch -- and ``GNNModel`` stacking it (the model
definition: what a user trains and what the accelerated path, ``runtime.CompiledModel.forward_edges``, is held against in
tests/test_hip_transformere.py).  ``torch_geometric`` is not required: the definition is pinned by the float64 numpy restatement
``transformere_util.transformere_layer`` (``p_ij`` formed explicitly, a two-pass softmax per destination), and the algebra the
accelerated path relies on by that restatement's ``folded=True`` variant.  No GPU."""
import numpy as np
import pytest
import torch

import gnnbuilder_amd as gnnb
from gnnbuilder_amd import synthetic
from gnnbuilder_amd.batching import pack_graphs
from helpers import looped_graph, make_model
from transformere_util import EDGE_DIMS, layer_weights, make_transformere_model, transformere_layer

NAMES = ("key", "query", "value", "skip")  # PyG's registration order; lin_edge behind them
CASES = [(9, 16, 1, 1), (11, 24, 4, 3), (7, 9, 3, 4), (9, 32, 4, 16), (5, 12, 3, 16), (6, 8, 1, 4)]  # (in, out, heads, edge_dim)


def _qm9_like(fin, seed):
    b = synthetic.make_batch("qm9", 6, seed=seed)
    rng = np.random.default_rng(seed)
    return pack_graphs([(rng.uniform(-1, 1, (b.graph(g)[0].shape[0], fin)).astype(np.float32), b.graph(g)[1]) for g in range(6)])


def _apply(conv, x, coo, ea):
    dtype = next(conv.parameters()).dtype
    with torch.no_grad():
        return conv(torch.from_numpy(np.asarray(x)).to(dtype),
                    torch.from_numpy(np.ascontiguousarray(np.asarray(coo).reshape(-1, 2).T.astype(np.int64))),
                    torch.from_numpy(np.asarray(ea)).to(dtype)).numpy()


def _graph(kind, fin, seed):
    if kind == "qm9":
        b = _qm9_like(fin, seed)
        return b.x, b.coo
    x, coo = looped_graph(40, fin, seed=seed)
    assert (coo[:, 0] == coo[:, 1]).sum() >= 10 and (np.bincount(coo[:, 1], minlength=40) == 0).sum() >= 3
    return x, coo


def test_the_cases_cover_the_heads_and_edge_dims():
    assert {c[2] for c in CASES} == {1, 3, 4} and {c[3] for c in CASES} == set(EDGE_DIMS)


@pytest.mark.parametrize("fin,fout,heads,d", CASES)
@pytest.mark.parametrize("graph", ["qm9", "looped"])
def test_conv_matches_the_two_pass_restatement_in_float64(fin, fout, heads, d, graph):
    torch.manual_seed(fin + d)
    conv = gnnb.TransformerEConv_GNNB(fin, fout, d, heads=heads).double()
    x, coo = _graph(graph, fin, seed=fin)
    ea = np.random.default_rng(d).uniform(-1, 1, (len(coo), d))
    got = _apply(conv, x, coo, ea)
    want = transformere_layer(x, coo, ea, layer_weights(conv.conv), heads)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"TransformerEConv_GNNB ({fin}, {fout}, heads {heads}, edge_dim {d}) on {graph} against the restatement: {err:.3e} relative")
    assert got.shape == (x.shape[0], fout) and err <= 1e-12


@pytest.mark.parametrize("fin,fout,heads,d", CASES)
def test_the_folded_form_is_the_direct_form_in_float64(fin, fout, heads, d):
    """q . (k + W_e e) = q . k + (W_e^T q) . e and sum a (v + W_e e) = sum a v + W_e sum a e: what the kernel relies on."""
    torch.manual_seed(100 + fin + d)
    conv = gnnb.TransformerEConv_GNNB(fin, fout, d, heads=heads).double()
    x, coo = _graph("looped", fin, seed=fin + 1)
    ea = np.random.default_rng(d + 1).uniform(-1, 1, (len(coo), d))
    w = layer_weights(conv.conv)
    direct, folded = transformere_layer(x, coo, ea, w, heads), transformere_layer(x, coo, ea, w, heads, folded=True)
    assert not np.array_equal(direct, transformere_layer(x, coo, np.zeros_like(ea), w, heads))  # (the edge term matters)
    assert np.abs(direct - folded).max() <= 1e-13 * np.abs(direct).max()


def test_an_explicit_self_loops_attributes_count():
    torch.manual_seed(1)
    conv = gnnb.TransformerEConv_GNNB(9, 16, 3, heads=2).double()
    x, coo = looped_graph(40, 9, seed=2)
    loops = coo[:, 0] == coo[:, 1]
    ea = np.random.default_rng(3).uniform(-1, 1, (len(coo), 3))
    with_loops, without = _apply(conv, x, coo, ea), _apply(conv, x, coo[~loops], ea[~loops])
    looped = np.unique(coo[loops][:, 1])
    others = np.setdiff1d(np.arange(40), looped)
    assert (np.abs(with_loops - without)[looped].max(1) > 1e-6).all()  # a (v, v) edge is an ordinary edge of v's softmax
    assert np.array_equal(with_loops[others], without[others])
    ea2 = ea.copy()
    ea2[loops] += 0.5  # ... and its attribute row an ordinary attribute row: only the looped rows move
    moved = _apply(conv, x, coo, ea2)
    assert (np.abs(moved - with_loops)[looped].max(1) > 1e-6).all() and np.array_equal(moved[others], with_loops[others])


def test_a_node_without_in_edges_gets_lin_skip():
    torch.manual_seed(2)
    conv = gnnb.TransformerEConv_GNNB(9, 16, 4, heads=4).double()
    x, coo = looped_graph(40, 9, seed=3)
    lone = np.flatnonzero(np.bincount(coo[:, 1], minlength=40) == 0)
    assert len(lone) >= 3
    sd = {k: v.numpy() for k, v in conv.state_dict().items()}
    r = x.astype(np.float64) @ sd["conv.lin_skip.weight"].T + sd["conv.lin_skip.bias"]
    assert np.abs(_apply(conv, x, coo, np.ones((len(coo), 4)))[lone] - r[lone]).max() <= 1e-15
    assert np.abs(_apply(conv, x, np.zeros((0, 2), np.int64), np.zeros((0, 4))) - r).max() <= 1e-15


def test_zero_attributes_give_the_layer_without_edge_features():
    torch.manual_seed(3)
    conv = gnnb.TransformerEConv_GNNB(9, 12, 4, heads=3).double()
    plain = gnnb.TransformerConv_GNNB(9, 12, heads=3).double()
    plain.load_state_dict({k: v for k, v in conv.state_dict().items() if "lin_edge" not in k})
    x, coo = looped_graph(40, 9, seed=4)
    ei = torch.from_numpy(np.ascontiguousarray(coo.T.astype(np.int64)))
    with torch.no_grad():
        want = plain(torch.from_numpy(x).double(), ei).numpy()
    assert np.abs(_apply(conv, x, coo, np.zeros((len(coo), 4))) - want).max() <= 1e-14


def test_state_dict_names_shapes_and_initialisation():
    torch.manual_seed(0)
    conv = gnnb.TransformerEConv_GNNB(9, 32, 4, heads=4)
    sd = {k: tuple(v.shape) for k, v in conv.state_dict().items()}
    assert list(sd) == [f"conv.lin_{n}.{t}" for n in NAMES for t in ("weight", "bias")] + ["conv.lin_edge.weight"]
    assert all(sd[f"conv.lin_{n}.weight"] == (32, 9) and sd[f"conv.lin_{n}.bias"] == (32,) for n in NAMES)
    assert sd["conv.lin_edge.weight"] == (32, 4) and conv.conv.lin_edge.bias is None
    assert isinstance(conv.conv, gnnb.models._TransformerConv) and isinstance(conv.conv.lin_edge, torch.nn.Linear)
    for name, t in conv.state_dict().items():  # torch's default nn.Linear initialisation: uniform(+-1 / sqrt(in))
        bound = 1.0 / (4 if "lin_edge" in name else 9) ** 0.5
        assert t.abs().max() <= bound and t.abs().max() > 0.5 * bound, name
    assert conv.heads == 4 and conv.edge_dim == 4 and conv.in_channels == 9 and conv.out_channels == 32 and conv.conv.out_channels == 8
    for word in ("edge_dim", "beta", "concat", "root_weight", "ropout", "edge_attr", "forward_edges"):
        assert word in gnnb.TransformerEConv_GNNB.__doc__, word
    assert "follow-up" not in gnnb.TransformerConv_GNNB.__doc__ and "TransformerEConv_GNNB" in gnnb.TransformerConv_GNNB.__doc__


def test_gnn_model_spec_and_parameter_names():
    model = make_transformere_model(in_dim=9, edge_dim=3, hidden=32, layers=3, heads=4)
    spec = model.spec()
    assert spec["conv"] == "transformere" and spec["heads"] == 4 and spec["edge_dim"] == 3 and "negative_slope" not in spec
    assert spec["num_layers"] == 3 and spec["gin_eps"] == 0.0
    assert "heads" not in make_model("gin", hidden=16).spec()  # (the other convs' specs are what they were)
    assert gnnb.TransformerEConv_GNNB in gnnb.models.SUPPORTED_GNN_CONVS and "TransformerEConv_GNNB" in gnnb.__all__
    assert gnnb.models._CONV_NAME[gnnb.TransformerEConv_GNNB] == "transformere"
    assert gnnb.models._EDGE_CONVS[gnnb.TransformerEConv_GNNB] == "TransformerE"
    assert gnnb.TransformerEConv_GNNB in gnnb.models._HEAD_CONVS
    names = model.canonical_param_names()
    per_layer = ["conv_lin_key_weight", "conv_lin_key_bias", "conv_lin_query_weight", "conv_lin_query_bias",
                 "conv_lin_value_weight", "conv_lin_value_bias", "conv_lin_skip_weight", "conv_lin_skip_bias", "conv_lin_edge_weight"]
    assert names[:27] == [f"gnn_convs_{l}_{p}" for l in range(3) for p in per_layer]
    assert names[27:] == [f"mlp_head_linear_layers_{i}_{p}" for i in range(3) for p in ("weight", "bias")]
    shapes = [tuple(p.shape) for p in model.canonical_params()]
    assert shapes[:9] == [(32, 9), (32,)] * 4 + [(32, 3)] and shapes[9:18] == [(32, 32), (32,)] * 4 + [(32, 3)]
    params = model.canonical_params()
    assert torch.equal(params[8], model.gnn_convs[0].conv.lin_edge.weight)
    assert params[17] is not params[8] and not torch.equal(params[17], params[8])  # each layer has its own lin_edge
    # a plain TransformerConv model is what it was
    from transformer_util import make_transformer_model
    plain = make_transformer_model(in_dim=9, hidden=32, layers=3, heads=4)
    assert plain.spec()["conv"] == "transformer" and plain.spec()["edge_dim"] == 0 and len(plain.canonical_param_names()) == 30


@pytest.mark.parametrize("layers", [1, 2, 3])
def test_gnn_model_stacks_layers_with_skip(layers):
    """The stack in float64 against the restatement layer by layer: the same edge_attr to every layer, the skip term on middle
    layers only, the activation behind it."""
    model = make_transformere_model(in_dim=9, edge_dim=3, hidden=24, layers=layers, heads=3, act="tanh", skip=True).double()
    b = _qm9_like(9, seed=5 + layers)
    ea = np.random.default_rng(layers).uniform(-1, 1, (b.num_edges, 3))
    ei = torch.from_numpy(np.ascontiguousarray(b.coo.T.astype(np.int64)))
    batch = torch.from_numpy(np.repeat(np.arange(b.num_graphs), np.diff(b.node_ptr)).astype(np.int64))
    with torch.no_grad():
        out = model(torch.from_numpy(b.x).double(), ei, batch, torch.from_numpy(ea))
    assert out.shape == (b.num_graphs, 19) and torch.isfinite(out).all()
    h = b.x.astype(np.float64)
    for l, conv in enumerate(model.gnn_convs):
        y = transformere_layer(h, b.coo, ea, layer_weights(conv.conv), 3)
        h = np.tanh(y + h if 0 < l < layers - 1 else y)
    with torch.no_grad():
        want = model.mlp_head(model.global_pooling(torch.from_numpy(h), batch)).numpy()
    assert np.abs(out.numpy() - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_value_errors():
    with pytest.raises(ValueError, match="divisible"):
        gnnb.TransformerEConv_GNNB(9, 30, 4, heads=4)
    for bad in (0, 9, -1, 2.0, True):
        with pytest.raises(ValueError, match="heads"):
            gnnb.TransformerEConv_GNNB(9, 32, 4, heads=bad)
    for bad in (0, 17, True, 4.0):
        with pytest.raises(ValueError, match="edge_dim must be an int in 1 .. 16"):
            gnnb.TransformerEConv_GNNB(9, 32, bad, heads=4)
    with pytest.raises(ValueError, match="divisible"):
        make_transformere_model(hidden=30, out_dim=32, heads=4)
    for bad in (0, 9, True):
        with pytest.raises(ValueError, match="TransformerConv model needs gnn_heads"):
            make_transformere_model(heads=bad)
    for bad in (None, 0, 17, True):
        with pytest.raises(ValueError, match="a TransformerE model needs graph_input_edge_dim"):
            make_transformere_model(edge_dim=bad)
    model = make_transformere_model(in_dim=9, edge_dim=3, hidden=16, layers=2, heads=2)
    b = _qm9_like(9, seed=1)
    ei = torch.from_numpy(np.ascontiguousarray(b.coo.T.astype(np.int64)))
    with pytest.raises(ValueError, match="a TransformerE model needs edge_attr"):
        model(torch.from_numpy(b.x), ei)
    # the other convs keep their refusals, word for word
    with pytest.raises(ValueError, match="only a GATv2 model \\(gnn_conv=GATv2Conv_GNNB\\) has attention heads"):
        gnnb.GNNModel(9, None, 16, 2, 16, gnnb.GINConv_GNNB, torch.nn.ReLU, True, gnnb.GlobalPooling(["add"]), gnnb.MLP(16, 2), None, gnn_heads=2)
    with pytest.raises(ValueError, match="a GATv2 model needs gnn_heads, an int in 1 .. 8"):
        gnnb.GNNModel(9, None, 16, 2, 16, gnnb.GATv2Conv_GNNB, torch.nn.ReLU, True, gnnb.GlobalPooling(["add"]), gnnb.MLP(16, 2), None, gnn_heads=9)


def test_project_does_not_generate_such_designs(tmp_path):
    with pytest.raises(NotImplementedError, match="TransformerConv designs with edge features"):
        gnnb.Project("transformere", make_transformere_model(), "regression", build_dir=tmp_path)
