"""``ResGatedGraphConv_GNNB`` -- PyG's ``ResGatedGraphConv`` in plain torch -- and ``GNNModel`` stacking it (the model definition:
what a user trains and what the accelerated path, ``runtime.CompiledModel.forward``, is held against in tests/test_hip_resgated.py).
``torch_geometric`` is not required: the definition is pinned by the float64 numpy restatement ``resgated_util.resgated_ref``.
No GPU."""
import numpy as np
import pytest
import torch

import gnnbuilder_amd as gnnb
from gnnbuilder_amd import synthetic
from gnnbuilder_amd.batching import pack_graphs
from helpers import looped_graph, make_model
from resgated_util import make_resgated_model, resgated_ref

KEYS = ["conv.bias", "conv.lin_key.weight", "conv.lin_key.bias", "conv.lin_query.weight", "conv.lin_query.bias",
        "conv.lin_value.weight", "conv.lin_value.bias", "conv.lin_skip.weight"]  # (a module's own parameters come first in torch)


def _conv_operands(conv, x):
    """(k, q, v, r) of ``conv`` (a ``ResGatedGraphConv_GNNB`` in float64) on ``x``, as float64 arrays: the four linears are
    explicit ``x @ W.T + b`` here -- ``r = x @ W_skip.T + bias``, lin_skip has no bias of its own --, so that ``resgated_ref``
    restates everything behind them."""
    sd = {k: v.numpy().astype(np.float64) for k, v in conv.state_dict().items()}
    x = np.asarray(x, np.float64)
    k, q, v = (x @ sd[f"conv.lin_{n}.weight"].T + sd[f"conv.lin_{n}.bias"] for n in ("key", "query", "value"))
    return k, q, v, x @ sd["conv.lin_skip.weight"].T + sd["conv.bias"]


def _qm9_like(fin, seed):
    b = synthetic.make_batch("qm9", 6, seed=seed)
    rng = np.random.default_rng(seed)
    return pack_graphs([(rng.uniform(-1, 1, (b.graph(g)[0].shape[0], fin)).astype(np.float32), b.graph(g)[1]) for g in range(6)])


def _apply(conv, x, coo):
    with torch.no_grad():
        return conv(torch.from_numpy(np.asarray(x)).to(next(conv.parameters()).dtype),
                    torch.from_numpy(np.ascontiguousarray(np.asarray(coo).reshape(-1, 2).T.astype(np.int64)))).numpy()


def _conv(fin, fout, seed):
    torch.manual_seed(seed)
    conv = gnnb.ResGatedGraphConv_GNNB(fin, fout).double()
    with torch.no_grad():
        conv.conv.bias.uniform_(-0.1, 0.1)  # (zero-initialised: a zero bias would not show where it is added)
    return conv


@pytest.mark.parametrize("fin,fout", [(9, 16), (11, 24), (7, 9)])
def test_conv_matches_the_restatement_in_float64(fin, fout):
    conv = _conv(fin, fout, fin)
    x, coo = looped_graph(40, fin, seed=fin)
    deg = np.bincount(coo[:, 1], minlength=40)
    # explicit self loops, duplicate edges and isolated nodes
    assert (coo[:, 0] == coo[:, 1]).sum() >= 10 and len(np.unique(coo, axis=0)) < len(coo) and (deg == 0).sum() >= 3
    got = _apply(conv, x, coo)
    k, q, v, r = _conv_operands(conv, x)
    want = resgated_ref(k, q, v, r, None, "none", coo)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"ResGatedGraphConv_GNNB ({fin}, {fout}) on the looped graph against the restatement: {err:.3e} relative")
    assert got.shape == (40, fout) and err <= 1e-12
    # a node without in-edges gets exactly lin_skip(x) + bias
    with torch.no_grad():
        lone = (conv.conv.lin_skip(torch.from_numpy(x).double()) + conv.conv.bias).numpy()
    assert np.array_equal(got[deg == 0], lone[deg == 0])
    # ... and a graph without any edge is that throughout
    assert np.array_equal(_apply(conv, x, np.zeros((0, 2), np.int64)), lone)


def test_the_destinations_key_meets_the_sources_query():
    """One edge 0 -> 1: ``out_1 = sigmoid(k_1 + q_0) * v_0 + r_1`` -- not ``k_0 + q_1``."""
    conv = _conv(5, 6, 11)
    x = np.random.default_rng(0).uniform(-1, 1, (2, 5))
    k, q, v, r = _conv_operands(conv, x)
    got = _apply(conv, x, np.array([[0, 1]]))
    want1 = v[0] / (1.0 + np.exp(-(k[1] + q[0]))) + r[1]
    wrong = v[0] / (1.0 + np.exp(-(k[0] + q[1]))) + r[1]
    assert np.abs(got[1] - want1).max() <= 1e-14 and np.abs(got[1] - wrong).max() > 1e-4
    assert np.abs(got[0] - r[0]).max() <= 1e-15


def test_an_explicit_self_loop_and_a_duplicate_edge_change_the_output():
    conv = _conv(9, 16, 1)
    x, coo = looped_graph(40, 9, seed=2)
    loops = coo[:, 0] == coo[:, 1]
    assert loops.sum() >= 10
    with_loops, without = _apply(conv, x, coo), _apply(conv, x, coo[~loops])
    looped = np.unique(coo[loops][:, 1])
    others = np.setdiff1d(np.arange(40), looped)
    assert (np.abs(with_loops - without)[looped].max(1) > 1e-6).all()  # a (v, v) edge is an ordinary edge
    assert np.array_equal(with_loops[others], without[others])
    twice = _apply(conv, x, np.concatenate([coo, coo[:1]]))
    assert np.abs(twice - with_loops)[coo[0, 1]].max() > 1e-6  # a duplicate edge counts as often as it occurs


def test_state_dict_names_shapes_and_initialisation():
    torch.manual_seed(0)
    conv = gnnb.ResGatedGraphConv_GNNB(9, 32)
    sd = {k: tuple(v.shape) for k, v in conv.state_dict().items()}
    assert sorted(sd) == sorted(KEYS) and "conv.lin_skip.bias" not in sd  # lin_skip has no bias: the conv's own is its
    assert all(sd[f"conv.lin_{n}.weight"] == (32, 9) for n in ("key", "query", "value", "skip"))
    assert all(sd[f"conv.lin_{n}.bias"] == (32,) for n in ("key", "query", "value")) and sd["conv.bias"] == (32,)
    assert all(isinstance(getattr(conv.conv, f"lin_{n}"), torch.nn.Linear) for n in ("key", "query", "value", "skip"))
    assert isinstance(conv.conv.bias, torch.nn.Parameter) and not conv.conv.bias.any()  # zero-initialised
    bound = 1.0 / 9 ** 0.5  # torch's default nn.Linear initialisation: uniform(+-1 / sqrt(in)) for weight and bias
    for name, t in conv.state_dict().items():
        if name != "conv.bias":
            assert t.abs().max() <= bound and t.abs().max() > 0.5 * bound, name
    assert conv.in_channels == 9 and conv.out_channels == 32 and not hasattr(conv, "heads")
    for word in ("edge_dim", "edge_attr", "root_weight", "bias=False", "Project"):
        assert word in gnnb.ResGatedGraphConv_GNNB.__doc__, word
    for word in ("sigmoid", "lin_skip", "self loop", "(v, v)", "without", "lin_key", "zero-initialised"):
        assert word in gnnb.models._ResGatedGraphConv.__doc__, word


def test_gnn_model_spec_and_parameter_names():
    model = make_resgated_model(in_dim=9, hidden=32, layers=3)
    spec = model.spec()
    assert spec["conv"] == "resgated" and "heads" not in spec and "negative_slope" not in spec and spec["num_layers"] == 3
    assert spec["edge_dim"] == 0 and spec["gin_eps"] == 0.0
    assert make_model("gin", hidden=16).spec()["conv"] == "gin"  # (the other convs' specs are what they were)
    assert gnnb.ResGatedGraphConv_GNNB in gnnb.models.SUPPORTED_GNN_CONVS and "ResGatedGraphConv_GNNB" in gnnb.__all__
    assert gnnb.models._CONV_NAME[gnnb.ResGatedGraphConv_GNNB] == "resgated"
    names = model.canonical_param_names()
    per_layer = ["conv_lin_key_weight", "conv_lin_key_bias", "conv_lin_query_weight", "conv_lin_query_bias",
                 "conv_lin_value_weight", "conv_lin_value_bias", "conv_lin_skip_weight", "conv_bias"]
    assert names[:24] == [f"gnn_convs_{l}_{p}" for l in range(3) for p in per_layer]
    assert names[24:] == [f"mlp_head_linear_layers_{i}_{p}" for i in range(3) for p in ("weight", "bias")]
    shapes = [tuple(p.shape) for p in model.canonical_params()]
    assert shapes[:8] == [(32, 9), (32,)] * 3 + [(32, 9), (32,)] and shapes[8:16] == [(32, 32), (32,)] * 4
    params = model.canonical_params()
    assert torch.equal(params[2], model.gnn_convs[0].conv.lin_query.weight) and torch.equal(params[6], model.gnn_convs[0].conv.lin_skip.weight)
    assert torch.equal(params[7], model.gnn_convs[0].conv.bias) and params[7].abs().max() > 0
    keys = [k for k in model.state_dict() if k.startswith("gnn_convs.1.")]
    assert sorted(keys) == sorted("gnn_convs.1." + k for k in KEYS)


@pytest.mark.parametrize("skip", [True, False])
@pytest.mark.parametrize("layers", [1, 2, 3])
def test_gnn_model_stacks_layers(layers, skip):
    """The stack in float64 against the restatement layer by layer: the skip term on middle layers only, the activation behind it."""
    model = make_resgated_model(in_dim=9, hidden=24, layers=layers, act="tanh", skip=skip).double()
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
        k, q, v, r = _conv_operands(conv, h)
        h = resgated_ref(k, q, v, r, h if (skip and 0 < l < layers - 1) else None, "tanh", b.coo)
    with torch.no_grad():
        want = model.mlp_head(model.global_pooling(torch.from_numpy(h), batch)).numpy()
    assert np.abs(out.numpy() - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_value_errors():
    for bad in (2, 0):  # (no heads: the refusal every conv without attention has)
        with pytest.raises(ValueError, match="gnn_heads"):
            gnnb.GNNModel(9, None, 16, 2, 16, gnnb.ResGatedGraphConv_GNNB, torch.nn.ReLU, True, gnnb.GlobalPooling(["add"]), gnnb.MLP(16, 2),
                          None, gnn_heads=bad)
    with pytest.raises(TypeError):
        gnnb.ResGatedGraphConv_GNNB(9, 16, heads=2)  # (no heads: a gate per column)
    # the stub stays a stub
    with pytest.raises(NotImplementedError):
        gnnb.GATConv_GNNB(4, 4)


def test_project_does_not_generate_resgated_designs(tmp_path):
    with pytest.raises(NotImplementedError, match="ResGatedGraphConv"):
        gnnb.Project("resgated", make_resgated_model(), "regression", build_dir=tmp_path)
