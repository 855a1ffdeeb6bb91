"""``GatedGraphConv_GNNB`` -- PyG's ``GatedGraphConv`` in plain torch -- and ``GNNModel`` stacking it (the model definition: what a
user trains and what the accelerated path, ``runtime.CompiledModel.forward``, is held against in tests/test_hip_ggnn.py).
``torch_geometric`` is not required: the definition is pinned by an independent loop over the edges around ``torch.nn.GRUCell``
and by the float64 numpy restatement ``ggnn_util.ggnn_ref``.  No GPU."""
import numpy as np
import pytest
import torch

import gnnbuilder_amd as gnnb
from gnnbuilder_amd import synthetic
from gnnbuilder_amd.batching import pack_graphs
from ggnn_util import ggnn_ref, make_ggnn_model
from helpers import looped_graph, make_model

KEYS = ["conv.weight", "conv.rnn.weight_ih", "conv.rnn.weight_hh", "conv.rnn.bias_ih", "conv.rnn.bias_hh"]


def _ei(coo):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(coo).reshape(-1, 2).T.astype(np.int64)))


def _apply(conv, x, coo):
    with torch.no_grad():
        return conv(torch.from_numpy(np.asarray(x)).to(next(conv.parameters()).dtype), _ei(coo))


def _edge_loop(conv, x, coo):
    """The layer by an independent loop over the edges: messages added one edge at a time, a ``torch.nn.GRUCell`` of its own that
    holds the conv's cell's tensors."""
    c = conv.conv
    out = c.out_channels
    cell = torch.nn.GRUCell(out, out).double()
    cell.load_state_dict({k[len("rnn."):]: v for k, v in c.state_dict().items() if k.startswith("rnn.")})
    h = torch.zeros(x.shape[0], out, dtype=torch.float64)
    h[:, :x.shape[1]] = torch.from_numpy(np.asarray(x, np.float64))
    with torch.no_grad():
        for t in range(c.num_layers):
            m = torch.zeros_like(h)
            for s, d in np.asarray(coo).reshape(-1, 2):
                m[d] += h[s] @ c.weight[t]
            h = cell(m, h)
    return h


def _qm9_like(fin, seed):
    b = synthetic.make_batch("qm9", 6, seed=seed)
    rng = np.random.default_rng(seed)
    return pack_graphs([(rng.uniform(-1, 1, (b.graph(g)[0].shape[0], fin)).astype(np.float32), b.graph(g)[1]) for g in range(6)])


def _step_operands(conv, h, t):
    """(p, gh, b_ih) of step ``t`` of ``conv`` (float64) on the state ``h`` [N, out]: the fold ``W_p[t] = weight_ih @ weight[t]^T``
    restated, so that ``ggnn_ref`` restates everything behind the GEMM."""
    sd = {k: v.numpy().astype(np.float64) for k, v in conv.state_dict().items()}
    w_p = sd["conv.rnn.weight_ih"] @ sd["conv.weight"][t].T
    return h @ w_p.T, h @ sd["conv.rnn.weight_hh"].T + sd["conv.rnn.bias_hh"], sd["conv.rnn.bias_ih"]


def _layer_by_ref(conv, x, coo, skip, act):
    out = conv.out_channels
    h = np.zeros((x.shape[0], out))
    h[:, :x.shape[1]] = x
    steps = conv.conv.num_layers
    for t in range(steps):
        p, gh, b_ih = _step_operands(conv, h, t)
        last = t == steps - 1
        h = ggnn_ref(p, gh, h, b_ih, skip if last else None, act if last else "none", coo)
    return h


@pytest.mark.parametrize("fin,fout,steps", [(9, 16, 1), (11, 24, 3), (16, 16, 3), (1, 9, 2)])
def test_conv_matches_an_edge_loop_and_the_restatement(fin, fout, steps):
    torch.manual_seed(fin)
    conv = gnnb.GatedGraphConv_GNNB(fin, fout, steps=steps).double()
    x, coo = looped_graph(40, fin, seed=fin)
    deg = np.bincount(coo[:, 1], minlength=40)
    # explicit self loops, duplicate edges and isolated nodes
    assert (coo[:, 0] == coo[:, 1]).sum() >= 10 and len(np.unique(coo, axis=0)) < len(coo) and (deg == 0).sum() >= 3
    got = _apply(conv, x, coo)
    want = _edge_loop(conv, x, coo)
    assert got.shape == (40, fout) and (got - want).abs().max() <= 1e-12
    ref = _layer_by_ref(conv, np.asarray(x, np.float64), coo, None, "none")
    assert np.abs(got.numpy() - ref).max() <= 1e-12
    # a row without in-edges is GRUCell(0, h) at every step of ITS state: at step 0, of [x | 0]
    one = gnnb.GatedGraphConv_GNNB(fin, fout, steps=1).double()
    one.load_state_dict({"conv.weight": conv.state_dict()["conv.weight"][:1], **{k: v for k, v in conv.state_dict().items() if "rnn" in k}})
    h0 = torch.zeros(40, fout, dtype=torch.float64)
    h0[:, :fin] = torch.from_numpy(np.asarray(x, np.float64))
    with torch.no_grad():
        lone = one.conv.rnn(torch.zeros_like(h0), h0)
    assert torch.equal(_apply(one, x, coo)[deg == 0], lone[deg == 0])
    # explicit self loops count as edges: without them the output is another one
    no_loops = _apply(conv, x, coo[coo[:, 0] != coo[:, 1]])
    assert (no_loops - got).abs().max() > 1e-3


def test_zero_padding_and_width_rules():
    torch.manual_seed(3)
    conv = gnnb.GatedGraphConv_GNNB(5, 12, steps=2).double()
    x, coo = looped_graph(30, 5, seed=2)
    padded = np.concatenate([np.asarray(x, np.float64), np.zeros((30, 7))], 1)
    same = gnnb.GatedGraphConv_GNNB(12, 12, steps=2).double()
    same.load_state_dict(conv.state_dict())
    assert torch.equal(_apply(conv, x, coo), _apply(same, padded, coo))  # in < out is in == out on [x | 0]
    with pytest.raises(ValueError, match="exceed"):
        gnnb.GatedGraphConv_GNNB(13, 12)
    with pytest.raises(ValueError):
        conv(torch.zeros(30, 13, dtype=torch.float64), _ei(coo))


def test_state_dict_has_pygs_names_and_shapes():
    torch.manual_seed(0)
    conv = gnnb.GatedGraphConv_GNNB(9, 32, steps=3)
    sd = {k: tuple(v.shape) for k, v in conv.state_dict().items()}
    assert list(sd) == KEYS
    assert sd == {"conv.weight": (3, 32, 32), "conv.rnn.weight_ih": (96, 32), "conv.rnn.weight_hh": (96, 32), "conv.rnn.bias_ih": (96,),
                  "conv.rnn.bias_hh": (96,)}
    assert isinstance(conv.conv.rnn, torch.nn.GRUCell)  # ONE cell, shared by all steps
    assert len([m for m in conv.modules() if isinstance(m, torch.nn.GRUCell)]) == 1
    bound = 1.0 / 32 ** 0.5
    for name, t in conv.state_dict().items():
        assert t.abs().max() <= bound and t.abs().max() > 0.5 * bound, name
    assert conv.in_channels == 9 and conv.out_channels == 32 and conv.steps == 3
    for word in ("edge_attr", "bias=False", "edge_weight", "Project", "gnn_steps"):
        assert word in gnnb.GatedGraphConv_GNNB.__doc__, word
    for word in ("GRUCell", "self loop", "(v, v)", "without", "zero columns", "rnn.weight_ih"):
        assert word in gnnb.models._GatedGraphConv.__doc__, word


def test_gnn_model_spec_and_parameter_names():
    model = make_ggnn_model(in_dim=9, hidden=32, layers=3, steps=3)
    spec = model.spec()
    assert spec["conv"] == "ggnn" and spec["steps"] == 3 and "heads" not in spec and "negative_slope" not in spec
    assert spec["edge_dim"] == 0 and spec["gin_eps"] == 0.0 and spec["num_layers"] == 3
    assert make_ggnn_model(steps=1).spec()["steps"] == 1
    assert "steps" not in make_model("gin", hidden=16).spec()  # (the key is this conv's alone, as "heads" is the head convs')
    assert gnnb.GatedGraphConv_GNNB in gnnb.models.SUPPORTED_GNN_CONVS and "GatedGraphConv_GNNB" in gnnb.__all__
    assert gnnb.models._CONV_NAME[gnnb.GatedGraphConv_GNNB] == "ggnn"
    names = model.canonical_param_names()
    per_layer = ["conv_weight", "conv_rnn_weight_ih", "conv_rnn_weight_hh", "conv_rnn_bias_ih", "conv_rnn_bias_hh"]
    assert names[:15] == [f"gnn_convs_{l}_{p}" for l in range(3) for p in per_layer]
    assert names[15:] == [f"mlp_head_linear_layers_{i}_{p}" for i in range(3) for p in ("weight", "bias")]
    shapes = [tuple(p.shape) for p in model.canonical_params()]
    assert shapes[:5] == [(3, 32, 32), (96, 32), (96, 32), (96,), (96,)] and shapes[5:10] == shapes[:5]
    params = model.canonical_params()
    assert torch.equal(params[0], model.gnn_convs[0].conv.weight) and torch.equal(params[3], model.gnn_convs[0].conv.rnn.bias_ih)
    keys = [k for k in model.state_dict() if k.startswith("gnn_convs.1.")]
    assert sorted(keys) == sorted("gnn_convs.1." + k for k in KEYS)


@pytest.mark.parametrize("skip", [True, False])
@pytest.mark.parametrize("layers,steps", [(1, 3), (2, 1), (3, 2)])
def test_gnn_model_stacks_layers(layers, steps, skip):
    """The stack in float64 against the restatement layer by layer and step by step: the skip term on middle layers only and
    behind the last step only, the activation behind it."""
    model = make_ggnn_model(in_dim=9, hidden=24, layers=layers, steps=steps, act="tanh", skip=skip).double()
    b = _qm9_like(9, seed=5 + layers)
    ei = torch.from_numpy(np.ascontiguousarray(b.coo.T.astype(np.int64)))
    batch = torch.from_numpy(np.repeat(np.arange(b.num_graphs), np.diff(b.node_ptr)).astype(np.int64))
    with torch.no_grad():
        out = model(torch.from_numpy(b.x).double(), ei, batch)
        out_ea = model(torch.from_numpy(b.x).double(), ei, batch, torch.ones(b.num_edges, 3, dtype=torch.float64))
    assert out.shape == (b.num_graphs, 19) and torch.isfinite(out).all() and torch.equal(out, out_ea)
    h = b.x.astype(np.float64)
    for l, conv in enumerate(model.gnn_convs):
        h = _layer_by_ref(conv, h, b.coo, h if (skip and 0 < l < layers - 1) else None, "tanh")
    with torch.no_grad():
        want = model.mlp_head(model.global_pooling(torch.from_numpy(h), batch)).numpy()
    assert np.abs(out.numpy() - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def _gnn(in_dim, hidden, layers, out_dim, conv=None, **kw):
    return gnnb.GNNModel(in_dim, None, hidden, layers, out_dim, conv or gnnb.GatedGraphConv_GNNB, torch.nn.ReLU, True,
                         gnnb.GlobalPooling(["add"]), gnnb.MLP(out_dim, 2), None, **kw)


def test_value_errors():
    for bad in (0, 9, 2.0, True, None):
        with pytest.raises(ValueError, match="gnn_steps"):
            _gnn(9, 16, 2, 16, gnn_steps=bad)
    assert _gnn(9, 16, 2, 16, gnn_steps=8).gnn_steps == 8 and _gnn(9, 16, 2, 16).gnn_steps == 1
    for conv in (gnnb.GINConv_GNNB, gnnb.ResGatedGraphConv_GNNB):  # (steps are this conv's alone)
        with pytest.raises(ValueError, match="gnn_steps"):
            _gnn(9, 16, 2, 16, conv=conv, gnn_steps=2)
        assert _gnn(9, 16, 2, 16, conv=conv, gnn_steps=1).gnn_steps == 1
    with pytest.raises(ValueError, match="gnn_heads"):
        _gnn(9, 16, 2, 16, gnn_heads=2)
    # a layer cannot narrow its input: in > hidden, hidden > out; with one layer in > out (hidden is not a layer's width there)
    for in_dim, hidden, layers, out_dim in ((17, 16, 2, 16), (9, 16, 2, 12), (9, 16, 3, 12), (17, 32, 1, 16)):
        with pytest.raises(ValueError, match="wider"):
            _gnn(in_dim, hidden, layers, out_dim)
    assert _gnn(16, 16, 3, 16).gnn_layer_sizes == [(16, 16)] * 3 and _gnn(9, 4, 1, 9).gnn_layer_sizes == [(9, 9)]
    # the stub stays a stub
    with pytest.raises(NotImplementedError):
        gnnb.GATConv_GNNB(4, 4)


def test_project_does_not_generate_ggnn_designs(tmp_path):
    with pytest.raises(NotImplementedError, match="GatedGraphConv"):
        gnnb.Project("ggnn", make_ggnn_model(), "regression", build_dir=tmp_path)
