"""``TransformerConv_GNNB`` -- PyG's ``TransformerConv`` in plain torch -- and ``GNNModel`` stacking it (the model definition: what
a user trains and what the accelerated path, ``runtime.CompiledModel.forward``, is held against in tests/test_hip_transformer.py).
``torch_geometric`` is not required: the definition is pinned by the float64 numpy restatement ``transformer_util.transformer_ref``.
No GPU."""
import numpy as np
import pytest
import torch

import gnnbuilder_amd as gnnb
from gnnbuilder_amd import synthetic
from gnnbuilder_amd.batching import pack_graphs
from helpers import looped_graph, make_model
from transformer_util import make_transformer_model, transformer_ref

NAMES = ("key", "query", "value", "skip")  # PyG's registration order


def _conv_operands(conv, x):
    """(q, k, v, r) of ``conv`` (a ``TransformerConv_GNNB`` in float64) on ``x``, as float64 arrays: the four linears are plain
    matrix products here, so that ``transformer_ref`` restates everything behind them."""
    sd = {k: v.numpy().astype(np.float64) for k, v in conv.state_dict().items()}
    x = np.asarray(x, np.float64)
    return tuple(x @ sd[f"conv.lin_{n}.weight"].T + sd[f"conv.lin_{n}.bias"] for n in ("query", "key", "value", "skip"))


def _qm9_like(fin, seed):
    b = synthetic.make_batch("qm9", 6, seed=seed)
    rng = np.random.default_rng(seed)
    return pack_graphs([(rng.uniform(-1, 1, (b.graph(g)[0].shape[0], fin)).astype(np.float32), b.graph(g)[1]) for g in range(6)])


def _apply(conv, x, coo):
    with torch.no_grad():
        return conv(torch.from_numpy(np.asarray(x)).to(next(conv.parameters()).dtype),
                    torch.from_numpy(np.ascontiguousarray(np.asarray(coo).reshape(-1, 2).T.astype(np.int64)))).numpy()


@pytest.mark.parametrize("fin,fout,heads", [(9, 16, 1), (11, 24, 4), (7, 9, 3)])
@pytest.mark.parametrize("graph", ["qm9", "looped"])
def test_conv_matches_the_two_pass_restatement_in_float64(fin, fout, heads, graph):
    torch.manual_seed(fin)
    conv = gnnb.TransformerConv_GNNB(fin, fout, heads=heads).double()
    if graph == "qm9":
        b = _qm9_like(fin, seed=fin)
        x, coo = b.x, b.coo
    else:
        x, coo = looped_graph(40, fin, seed=fin)
        assert (coo[:, 0] == coo[:, 1]).sum() >= 10  # explicit self loops, one node with two
    got = _apply(conv, x, coo)
    q, k, v, r = _conv_operands(conv, x)
    want = transformer_ref(q, k, v, r, None, "none", coo, heads, 1.0 / np.sqrt(fout // heads))
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"TransformerConv_GNNB ({fin}, {fout}, heads {heads}) on {graph} against the two-pass restatement: {err:.3e} relative")
    assert got.shape == (x.shape[0], fout) and err <= 1e-12


def test_an_explicit_self_loop_changes_the_output():
    torch.manual_seed(1)
    conv = gnnb.TransformerConv_GNNB(9, 16, heads=2).double()
    x, coo = looped_graph(40, 9, seed=2)
    loops = coo[:, 0] == coo[:, 1]
    assert loops.sum() >= 10
    with_loops, without = _apply(conv, x, coo), _apply(conv, x, coo[~loops])
    looped = np.unique(coo[loops][:, 1])
    others = np.setdiff1d(np.arange(40), looped)
    assert (np.abs(with_loops - without)[looped].max(1) > 1e-6).all()  # a (v, v) edge is an ordinary edge of v's softmax
    assert np.array_equal(with_loops[others], without[others])


def test_a_node_without_in_edges_gets_lin_skip():
    torch.manual_seed(2)
    conv = gnnb.TransformerConv_GNNB(9, 16, heads=4).double()
    x, coo = looped_graph(40, 9, seed=3)
    lone = np.flatnonzero(np.bincount(coo[:, 1], minlength=40) == 0)
    assert len(lone) >= 3
    r = _conv_operands(conv, x)[3]
    assert np.abs(_apply(conv, x, coo)[lone] - r[lone]).max() <= 1e-15  # (nothing to attend over: the root term alone)
    # ... and a graph without any edge is lin_skip(x) throughout
    assert np.abs(_apply(conv, x, np.zeros((0, 2), np.int64)) - r).max() <= 1e-15


def test_with_a_zero_query_the_layer_is_the_mean_of_the_values_plus_the_root():
    torch.manual_seed(3)
    conv = gnnb.TransformerConv_GNNB(9, 12, heads=3).double()
    with torch.no_grad():
        conv.conv.lin_query.weight.zero_()
        conv.conv.lin_query.bias.zero_()
    x, coo = looped_graph(40, 9, seed=4)
    _, _, v, r = _conv_operands(conv, x)
    want = np.zeros_like(v)
    np.add.at(want, coo[:, 1], v[coo[:, 0]])
    want = want / np.maximum(np.bincount(coo[:, 1], minlength=40), 1)[:, None] + r
    assert np.abs(_apply(conv, x, coo) - want).max() <= 1e-13


def test_state_dict_names_shapes_and_initialisation():
    torch.manual_seed(0)
    conv = gnnb.TransformerConv_GNNB(9, 32, heads=4)
    sd = {k: tuple(v.shape) for k, v in conv.state_dict().items()}
    assert list(sd) == [f"conv.lin_{n}.{t}" for n in NAMES for t in ("weight", "bias")]  # PyG's order; no parameter of the conv's own
    assert all(sd[f"conv.lin_{n}.weight"] == (32, 9) and sd[f"conv.lin_{n}.bias"] == (32,) for n in NAMES)
    assert all(isinstance(getattr(conv.conv, f"lin_{n}"), torch.nn.Linear) for n in NAMES)
    bound = 1.0 / 9 ** 0.5  # torch's default nn.Linear initialisation: uniform(+-1 / sqrt(in)) for weight and bias
    for name, t in conv.state_dict().items():
        assert t.abs().max() <= bound and t.abs().max() > 0.5 * bound, name
    assert conv.heads == 4 and conv.in_channels == 9 and conv.out_channels == 32 and conv.conv.out_channels == 8
    assert not hasattr(conv, "negative_slope")
    for word in ("edge_dim", "beta", "concat", "root_weight", "ropout", "edge_attr"):
        assert word in gnnb.TransformerConv_GNNB.__doc__, word


def test_gnn_model_spec_and_parameter_names():
    model = make_transformer_model(in_dim=9, hidden=32, layers=3, heads=4)
    spec = model.spec()
    assert spec["conv"] == "transformer" and spec["heads"] == 4 and "negative_slope" not in spec and spec["num_layers"] == 3
    assert spec["edge_dim"] == 0 and spec["gin_eps"] == 0.0
    assert "heads" not in make_model("gin", hidden=16).spec()  # (the other convs' specs are what they were)
    assert gnnb.TransformerConv_GNNB in gnnb.models.SUPPORTED_GNN_CONVS
    assert gnnb.models._CONV_NAME[gnnb.TransformerConv_GNNB] == "transformer"
    names = model.canonical_param_names()
    per_layer = ["conv_lin_key_weight", "conv_lin_key_bias", "conv_lin_query_weight", "conv_lin_query_bias",
                 "conv_lin_value_weight", "conv_lin_value_bias", "conv_lin_skip_weight", "conv_lin_skip_bias"]
    assert names[:24] == [f"gnn_convs_{l}_{p}" for l in range(3) for p in per_layer]
    assert names[24:] == [f"mlp_head_linear_layers_{i}_{p}" for i in range(3) for p in ("weight", "bias")]
    shapes = [tuple(p.shape) for p in model.canonical_params()]
    assert shapes[:8] == [(32, 9), (32,)] * 4 and shapes[8:16] == [(32, 32), (32,)] * 4
    params = model.canonical_params()
    assert params[2] is not params[0] and torch.equal(params[2], model.gnn_convs[0].conv.lin_query.weight)
    one = make_transformer_model(heads=1)  # (gnn_heads defaults to 1)
    assert one.spec()["heads"] == 1


@pytest.mark.parametrize("layers", [1, 2, 3])
def test_gnn_model_stacks_layers_with_skip(layers):
    """The stack in float64 against the restatement layer by layer: the skip term on middle layers only, the activation behind it."""
    model = make_transformer_model(in_dim=9, hidden=24, layers=layers, heads=3, act="tanh", skip=True).double()
    b = _qm9_like(9, seed=5 + layers)
    # (graph_input_edge_dim and edge_attr are ignored: the same output with and without)
    ei = torch.from_numpy(np.ascontiguousarray(b.coo.T.astype(np.int64)))
    batch = torch.from_numpy(np.repeat(np.arange(b.num_graphs), np.diff(b.node_ptr)).astype(np.int64))
    with torch.no_grad():
        out = model(torch.from_numpy(b.x).double(), ei, batch)
        out_ea = model(torch.from_numpy(b.x).double(), ei, batch, torch.ones(b.num_edges, 3, dtype=torch.float64))
    assert out.shape == (b.num_graphs, 19) and torch.isfinite(out).all() and torch.equal(out, out_ea)
    h = b.x.astype(np.float64)
    for l, conv in enumerate(model.gnn_convs):
        q, k, v, r = _conv_operands(conv, h)
        skip = h if (0 < l < layers - 1) else None
        h = transformer_ref(q, k, v, r, skip, "tanh", b.coo, 3, 1.0 / np.sqrt(8))
    with torch.no_grad():
        want = model.mlp_head(model.global_pooling(torch.from_numpy(h), batch)).numpy()
    assert np.abs(out.numpy() - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_value_errors():
    with pytest.raises(ValueError, match="divisible"):
        gnnb.TransformerConv_GNNB(9, 30, heads=4)
    for bad in (0, 9, -1, 2.0, True):
        with pytest.raises(ValueError, match="heads"):
            gnnb.TransformerConv_GNNB(9, 32, heads=bad)
    with pytest.raises(ValueError, match="divisible"):
        make_transformer_model(hidden=30, out_dim=32, heads=4)
    with pytest.raises(ValueError, match="divisible"):
        make_transformer_model(hidden=32, out_dim=30, heads=4)
    for bad in (0, 9, True):
        with pytest.raises(ValueError, match="TransformerConv model needs gnn_heads"):
            make_transformer_model(heads=bad)
    # the other convs keep their refusals, word for word
    with pytest.raises(ValueError, match="only a GATv2 model \\(gnn_conv=GATv2Conv_GNNB\\) has attention heads"):
        gnnb.GNNModel(9, None, 16, 2, 16, gnnb.GINConv_GNNB, torch.nn.ReLU, True, gnnb.GlobalPooling(["add"]), gnnb.MLP(16, 2), None, gnn_heads=2)
    with pytest.raises(ValueError, match="a GATv2 model needs gnn_heads, an int in 1 .. 8"):
        gnnb.GNNModel(9, None, 16, 2, 16, gnnb.GATv2Conv_GNNB, torch.nn.ReLU, True, gnnb.GlobalPooling(["add"]), gnnb.MLP(16, 2), None, gnn_heads=9)
    # a one-layer model has no hidden width to divide
    assert make_transformer_model(hidden=30, out_dim=32, layers=1, heads=4).spec()["out_dim"] == 32
    # the stub stays a stub
    with pytest.raises(NotImplementedError):
        gnnb.GATConv_GNNB(4, 4)


def test_project_does_not_generate_transformer_designs(tmp_path):
    with pytest.raises(NotImplementedError, match="TransformerConv"):
        gnnb.Project("transformer", make_transformer_model(), "regression", build_dir=tmp_path)
