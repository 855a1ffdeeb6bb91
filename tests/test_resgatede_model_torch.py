"""``ResGatedGraphEConv_GNNB`` -- PyG's ``ResGatedGraphConv(edge_dim=d)`` in plain torch -- and ``GNNModel`` stacking it (the model
definition: what a user trains and what the accelerated path, ``runtime.CompiledModel.forward_edges``, is held against in
tests/test_hip_resgatede.py).  ``torch_geometric`` is not required: the definition is pinned by an independent float64 restatement
that walks the edges one at a time (``resgatede_util.resgatede_layer``), and the split the accelerated path relies on -- the x
column blocks per node, ``W_ke + W_qe`` and ``W_ve`` per edge -- by ``resgatede_util.resgatede_ref``.  No GPU."""
import numpy as np
import pytest
import torch

import gnnbuilder_amd as gnnb
from gnnbuilder_amd import synthetic
from gnnbuilder_amd.batching import pack_graphs
from helpers import looped_graph, make_model
from resgated_util import make_resgated_model
from resgatede_util import layer_weights, make_resgatede_model, resgatede_layer, resgatede_ref

KEYS = ["conv.bias", "conv.lin_key.weight", "conv.lin_key.bias", "conv.lin_query.weight", "conv.lin_query.bias",
        "conv.lin_value.weight", "conv.lin_value.bias", "conv.lin_skip.weight"]  # (a module's own parameters come first in torch)


def _qm9_like(fin, seed):
    b = synthetic.make_batch("qm9", 6, seed=seed)
    rng = np.random.default_rng(seed)
    return pack_graphs([(rng.uniform(-1, 1, (b.graph(g)[0].shape[0], fin)).astype(np.float32), b.graph(g)[1]) for g in range(6)])


def _apply(conv, x, coo, ea):
    dtype = next(conv.parameters()).dtype
    with torch.no_grad():
        return conv(torch.from_numpy(np.asarray(x)).to(dtype), torch.from_numpy(np.ascontiguousarray(np.asarray(coo).reshape(-1, 2).T.astype(np.int64))),
                    torch.from_numpy(np.asarray(ea)).to(dtype)).numpy()


def _conv(fin, fout, d, seed):
    torch.manual_seed(seed)
    conv = gnnb.ResGatedGraphEConv_GNNB(fin, fout, d).double()
    with torch.no_grad():
        conv.conv.bias.uniform_(-0.1, 0.1)  # (zero-initialised: a zero bias would not show where it is added)
    return conv


def _split(conv, x):
    """The operands of the accelerated path's split, in float64: (k, q, v, r) from the x column blocks, W_g = W_ke + W_qe, W_v."""
    w = layer_weights(conv.conv)
    x = np.asarray(x, np.float64)
    fi = x.shape[1]
    k, q, v = (x @ w[n][0][:, :fi].T + w[n][1] for n in ("key", "query", "value"))
    return k, q, v, x @ w["skip"].T + w["bias"], w["key"][0][:, fi:] + w["query"][0][:, fi:], w["value"][0][:, fi:]


@pytest.mark.parametrize("fin,fout,d", [(9, 16, 4), (11, 24, 3), (7, 9, 16), (5, 8, 1)])
def test_conv_matches_the_per_edge_restatement_in_float64(fin, fout, d):
    conv = _conv(fin, fout, d, fin)
    x, coo = looped_graph(40, fin, seed=fin)
    ea = np.random.default_rng(d).uniform(-1, 1, (len(coo), d))
    deg = np.bincount(coo[:, 1], minlength=40)
    # explicit self loops, duplicate edges and isolated nodes
    assert (coo[:, 0] == coo[:, 1]).sum() >= 10 and len(np.unique(coo, axis=0)) < len(coo) and (deg == 0).sum() >= 3
    got = _apply(conv, x, coo, ea)
    want = resgatede_layer(x, coo, ea, layer_weights(conv.conv))
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"ResGatedGraphEConv_GNNB ({fin}, {fout}, edge_dim {d}) on the looped graph against the per-edge loop: {err:.3e} relative")
    assert got.shape == (40, fout) and err <= 1e-12
    # ... and the split the accelerated path computes is the same function
    k, q, v, r, wg, wv = _split(conv, x)
    split = resgatede_ref(k, q, v, r, None, "none", coo, ea, wg, wv)
    assert np.abs(split - want).max() / np.abs(want).max() <= 1e-12
    # the edge attributes matter, in the gate and in the value
    assert np.abs(resgatede_ref(k, q, v, r, None, "none", coo, ea, None, wv) - want).max() > 1e-4
    assert np.abs(resgatede_ref(k, q, v, r, None, "none", coo, ea, wg, None) - want).max() > 1e-4
    # a node without in-edges gets exactly lin_skip(x) + bias
    with torch.no_grad():
        lone = (conv.conv.lin_skip(torch.from_numpy(x).double()) + conv.conv.bias).numpy()
    assert np.array_equal(got[deg == 0], lone[deg == 0])
    assert np.array_equal(_apply(conv, x, np.zeros((0, 2), np.int64), np.zeros((0, d))), lone)


def test_the_attributes_are_concatenated_behind_x():
    """One edge 0 -> 1: the key sees [x_1 | e], query and value see [x_0 | e] -- e in the LAST d columns of each weight."""
    conv = _conv(5, 6, 3, 11)
    w = layer_weights(conv.conv)
    rng = np.random.default_rng(0)
    x, e = rng.uniform(-1, 1, (2, 5)), rng.uniform(-1, 1, (1, 3))
    got = _apply(conv, x, np.array([[0, 1]]), e)
    lin = lambda n, z: w[n][0] @ z + w[n][1]  # noqa: E731
    z1, z0 = np.concatenate([x[1], e[0]]), np.concatenate([x[0], e[0]])
    r = x @ w["skip"].T + w["bias"]
    want1 = lin("value", z0) / (1.0 + np.exp(-(lin("key", z1) + lin("query", z0)))) + r[1]
    front = lin("value", np.concatenate([e[0], x[0]])[:8]) / (1.0 + np.exp(-(lin("key", z1) + lin("query", z0)))) + r[1]
    assert np.abs(got[1] - want1).max() <= 1e-14 and np.abs(got[1] - front).max() > 1e-4
    assert np.abs(got[0] - r[0]).max() <= 1e-15


@pytest.mark.parametrize("fin,fout,d", [(9, 16, 4), (7, 9, 3)])
def test_with_zero_attributes_it_is_the_plain_conv_of_the_x_column_blocks(fin, fout, d):
    conv = _conv(fin, fout, d, 3)
    torch.manual_seed(0)
    plain = gnnb.ResGatedGraphConv_GNNB(fin, fout).double()
    with torch.no_grad():
        for n in ("key", "query", "value"):
            getattr(plain.conv, f"lin_{n}").weight.copy_(getattr(conv.conv, f"lin_{n}").weight[:, :fin])
            getattr(plain.conv, f"lin_{n}").bias.copy_(getattr(conv.conv, f"lin_{n}").bias)
        plain.conv.lin_skip.weight.copy_(conv.conv.lin_skip.weight)
        plain.conv.bias.copy_(conv.conv.bias)
    x, coo = looped_graph(40, fin, seed=4)
    with torch.no_grad():
        want = plain(torch.from_numpy(x).double(), torch.from_numpy(np.ascontiguousarray(coo.T.astype(np.int64)))).numpy()
    got = _apply(conv, x, coo, np.zeros((len(coo), d)))
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    assert np.abs(_apply(conv, x, coo, np.ones((len(coo), d))) - want).max() > 1e-4


def test_state_dict_names_shapes_and_initialisation():
    torch.manual_seed(0)
    conv = gnnb.ResGatedGraphEConv_GNNB(9, 32, 4)
    sd = {k: tuple(v.shape) for k, v in conv.state_dict().items()}
    assert sorted(sd) == sorted(KEYS) and "conv.lin_skip.bias" not in sd and "conv.lin_edge.weight" not in sd  # PyG's names: no lin_edge
    assert all(sd[f"conv.lin_{n}.weight"] == (32, 13) for n in ("key", "query", "value")) and sd["conv.lin_skip.weight"] == (32, 9)
    assert all(sd[f"conv.lin_{n}.bias"] == (32,) for n in ("key", "query", "value")) and sd["conv.bias"] == (32,)
    assert all(isinstance(getattr(conv.conv, f"lin_{n}"), torch.nn.Linear) for n in ("key", "query", "value", "skip"))
    assert isinstance(conv.conv.bias, torch.nn.Parameter) and not conv.conv.bias.any()  # zero-initialised
    assert conv.in_channels == 9 and conv.out_channels == 32 and conv.edge_dim == 4 and not hasattr(conv, "heads")
    # nothing of the accelerated path's split in the definition
    assert not any(word in name for name in sd for word in ("gate", "w_g", "fold"))
    for word in ("edge_dim", "forward_edges", "root_weight", "bias=False", "Project", "gnnb_resgated_edge.h"):
        assert word in gnnb.ResGatedGraphEConv_GNNB.__doc__, word
    for word in ("sigmoid", "lin_skip", "self loop", "(v, v)", "without", "lin_key", "in + d", "state_dict"):
        assert word in gnnb.models._ResGatedGraphEConv.__doc__, word
    assert "ResGatedGraphEConv_GNNB" in gnnb.ResGatedGraphConv_GNNB.__doc__  # (the plain conv points to it)


def test_gnn_model_spec_and_parameter_names():
    model = make_resgatede_model(in_dim=9, edge_dim=4, hidden=32, layers=3)
    spec = model.spec()
    assert spec["conv"] == "resgatede" and "heads" not in spec and "negative_slope" not in spec and spec["num_layers"] == 3
    assert spec["edge_dim"] == 4 and spec["gin_eps"] == 0.0
    assert make_resgated_model(hidden=16).spec()["conv"] == "resgated" and make_resgated_model(hidden=16).spec()["edge_dim"] == 0
    assert make_model("gin", hidden=16).spec()["conv"] == "gin"  # (the other convs' specs are what they were)
    assert gnnb.ResGatedGraphEConv_GNNB in gnnb.models.SUPPORTED_GNN_CONVS and "ResGatedGraphEConv_GNNB" in gnnb.__all__
    assert gnnb.models._CONV_NAME[gnnb.ResGatedGraphEConv_GNNB] == "resgatede"
    assert gnnb.models._EDGE_CONVS[gnnb.ResGatedGraphEConv_GNNB] == "ResGatedE"
    assert all(c.edge_dim == 4 for c in model.gnn_convs)
    names = model.canonical_param_names()
    per_layer = ["conv_lin_key_weight", "conv_lin_key_bias", "conv_lin_query_weight", "conv_lin_query_bias",
                 "conv_lin_value_weight", "conv_lin_value_bias", "conv_lin_skip_weight", "conv_bias"]
    assert names[:24] == [f"gnn_convs_{l}_{p}" for l in range(3) for p in per_layer]
    assert names[24:] == [f"mlp_head_linear_layers_{i}_{p}" for i in range(3) for p in ("weight", "bias")]
    shapes = [tuple(p.shape) for p in model.canonical_params()]
    assert shapes[:8] == [(32, 13), (32,)] * 3 + [(32, 9), (32,)] and shapes[8:16] == [(32, 36), (32,)] * 3 + [(32, 32), (32,)]
    params = model.canonical_params()
    assert torch.equal(params[2], model.gnn_convs[0].conv.lin_query.weight) and torch.equal(params[6], model.gnn_convs[0].conv.lin_skip.weight)
    assert torch.equal(params[7], model.gnn_convs[0].conv.bias) and params[7].abs().max() > 0
    keys = [k for k in model.state_dict() if k.startswith("gnn_convs.1.")]
    assert sorted(keys) == sorted("gnn_convs.1." + k for k in KEYS)


@pytest.mark.parametrize("skip", [True, False])
@pytest.mark.parametrize("layers", [1, 2, 3])
def test_gnn_model_stacks_layers(layers, skip):
    """The stack in float64 against the per-edge restatement layer by layer: the same edge_attr to every layer, the skip term on
    middle layers only, the activation behind it."""
    d = 3
    model = make_resgatede_model(in_dim=9, edge_dim=d, hidden=24, layers=layers, act="tanh", skip=skip).double()
    b = _qm9_like(9, seed=5 + layers)
    ea = np.random.default_rng(layers).uniform(-1, 1, (b.num_edges, d))
    ei = torch.from_numpy(np.ascontiguousarray(b.coo.T.astype(np.int64)))
    batch = torch.from_numpy(np.repeat(np.arange(b.num_graphs), np.diff(b.node_ptr)).astype(np.int64))
    with torch.no_grad():
        out = model(torch.from_numpy(b.x).double(), ei, batch, torch.from_numpy(ea))
    assert out.shape == (b.num_graphs, 19) and torch.isfinite(out).all()
    with pytest.raises(ValueError, match="ResGatedE model needs edge_attr"):
        model(torch.from_numpy(b.x).double(), ei, batch)
    h = b.x.astype(np.float64)
    for l, conv in enumerate(model.gnn_convs):
        nxt = resgatede_layer(h, b.coo, ea, layer_weights(conv.conv))
        if skip and 0 < l < layers - 1:
            nxt = nxt + h
        h = np.tanh(nxt)
    with torch.no_grad():
        want = model.mlp_head(model.global_pooling(torch.from_numpy(h), batch)).numpy()
    assert np.abs(out.numpy() - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_value_errors():
    mk = lambda d, **kw: gnnb.GNNModel(9, d, 16, 2, 16, gnnb.ResGatedGraphEConv_GNNB, torch.nn.ReLU, True, gnnb.GlobalPooling(["add"]),  # noqa: E731
                                       gnnb.MLP(16, 2), None, **kw)
    for bad in (None, 0, 17, 4.0, True):
        with pytest.raises(ValueError, match="ResGatedE model needs graph_input_edge_dim"):
            mk(bad)
    for bad in (0, 17, 2.5, True):
        with pytest.raises(ValueError, match="edge_dim must be an int in 1 .. 16"):
            gnnb.ResGatedGraphEConv_GNNB(9, 16, bad)
    for bad in (2, 0):  # (no heads: the refusal every conv without attention has)
        with pytest.raises(ValueError, match="gnn_heads"):
            mk(4, gnn_heads=bad)
    with pytest.raises(TypeError):
        gnnb.ResGatedGraphEConv_GNNB(9, 16, 4, heads=2)  # (no heads: a gate per column)
    assert mk(16).spec()["edge_dim"] == 16 and mk(1).spec()["edge_dim"] == 1


def test_project_does_not_generate_such_designs(tmp_path):
    with pytest.raises(NotImplementedError, match="ResGatedGraphConv designs with edge features"):
        gnnb.Project("resgatede", make_resgatede_model(), "regression", build_dir=tmp_path)
    with pytest.raises(NotImplementedError, match="ResGatedGraphConv designs:"):  # (the plain one keeps its message)
        gnnb.Project("resgated", make_resgated_model(), "regression", build_dir=tmp_path)
