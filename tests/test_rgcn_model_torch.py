"""``RGCNConv_GNNB`` -- PyG's ``RGCNConv`` in plain torch -- and ``GNNModel`` stacking it (the model definition: what a user
trains and what the accelerated path, ``runtime.CompiledModel.forward_types``, is held against in tests/test_hip_rgcn.py).
``torch_geometric`` is not required: the definition is pinned by an independent float64 loop over the edges and by the numpy
restatement ``rgcn_util.rgcn_ref``.  No GPU."""
import numpy as np
import pytest
import torch

import gnnbuilder_amd as gnnb
from gnnbuilder_amd import synthetic
from gnnbuilder_amd.batching import pack_graphs
from helpers import looped_graph, make_model
from rgcn_util import make_rgcn_model, rgcn_ref

KEYS = ["conv.weight", "conv.root", "conv.bias"]


def _ei(coo):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(coo).reshape(-1, 2).T.astype(np.int64)))


def _apply(conv, x, coo, types):
    with torch.no_grad():
        return conv(torch.from_numpy(np.asarray(x)).to(next(conv.parameters()).dtype), _ei(coo), torch.from_numpy(np.asarray(types, np.int64)))


def _edge_loop(conv, x, coo, types):
    """The formula of the header, independently: one edge at a time into per-(node, relation) sums of TRANSFORMED rows and
    counts, then ``x @ root + bias + sum_r sums_r / count_r``."""
    c = conv.conv
    w, root, bias = (t.detach().double().numpy() for t in (c.weight, c.root, c.bias))
    x = np.asarray(x, np.float64)
    n, R = x.shape[0], c.num_relations
    sums, cnt = np.zeros((n, R, c.out_channels)), np.zeros((n, R))
    for (s, d), r in zip(np.asarray(coo).reshape(-1, 2), types):
        sums[d, r] += x[s] @ w[r]
        cnt[d, r] += 1
    return x @ root + bias + (sums / np.maximum(cnt, 1)[:, :, None]).sum(1)


@pytest.mark.parametrize("fin,fout,relations", [(9, 16, 4), (11, 7, 3), (16, 16, 1), (1, 9, 8)])
def test_conv_matches_an_edge_loop_and_the_restatement(fin, fout, relations):
    torch.manual_seed(fin)
    conv = gnnb.RGCNConv_GNNB(fin, fout, relations=relations).double()
    with torch.no_grad():
        conv.conv.bias.uniform_(-0.5, 0.5)
    x, coo = looped_graph(40, fin, seed=fin)
    types = np.random.default_rng(fin).integers(0, relations, len(coo))
    deg = np.bincount(coo[:, 1], minlength=40)
    # explicit self loops, duplicate edges and isolated nodes
    assert (coo[:, 0] == coo[:, 1]).sum() >= 10 and len(np.unique(coo, axis=0)) < len(coo) and (deg == 0).sum() >= 3
    got = _apply(conv, x, coo, types)
    want = _edge_loop(conv, x, coo, types)
    assert got.shape == (40, fout) and np.abs(got.numpy() - want).max() <= 1e-12
    # ... and the restatement behind the GEMM: p_r = x @ weight[r], root = x @ root + bias
    x64 = np.asarray(x, np.float64)
    sd = {k: v.numpy() for k, v in conv.state_dict().items()}
    p = np.concatenate([x64 @ sd["conv.weight"][r] for r in range(relations)], 1)
    ref = rgcn_ref(p, x64 @ sd["conv.root"] + sd["conv.bias"], None, "none", coo, types, relations)
    assert np.abs(got.numpy() - ref).max() <= 1e-12
    # a row without in-edges is x @ root + bias
    assert np.abs(got.numpy()[deg == 0] - (x64 @ sd["conv.root"] + sd["conv.bias"])[deg == 0]).max() <= 1e-14
    # explicit self loops count as edges, and the types matter
    keep = coo[:, 0] != coo[:, 1]
    assert (_apply(conv, x, coo[keep], types[keep]) - got).abs().max() > 1e-3
    if relations > 1:
        assert (_apply(conv, x, coo, (types + 1) % relations) - got).abs().max() > 1e-3


def test_types_are_checked():
    conv = gnnb.RGCNConv_GNNB(5, 6, relations=3)
    x, coo = looped_graph(30, 5, seed=2)
    t = np.zeros(len(coo), np.int64)
    for bad in (3, -1):
        t2 = t.copy()
        t2[7] = bad
        with pytest.raises(ValueError, match=r"\[0, 3\)"):
            _apply(conv, x, coo, t2)
    with pytest.raises(ValueError, match="one type per edge"):
        _apply(conv, x, coo, t[:-1])
    none = _apply(conv, x, np.zeros((0, 2), np.int64), np.zeros(0, np.int64))  # (no edge: nothing to check)
    assert none.shape == (30, 6)


def test_state_dict_has_pygs_names_and_shapes():
    torch.manual_seed(0)
    conv = gnnb.RGCNConv_GNNB(9, 32, relations=4)
    sd = {k: tuple(v.shape) for k, v in conv.state_dict().items()}
    assert list(sd) == KEYS and sd == {"conv.weight": (4, 9, 32), "conv.root": (9, 32), "conv.bias": (32,)}
    bound = (6.0 / (9 + 32)) ** 0.5  # glorot, glorot, zeros
    for name in ("conv.weight", "conv.root"):
        t = conv.state_dict()[name]
        assert t.abs().max() <= bound and t.abs().max() > 0.8 * bound, name
    assert not conv.state_dict()["conv.bias"].any()
    assert conv.in_channels == 9 and conv.out_channels == 32 and conv.relations == 4 and conv.conv.num_relations == 4
    for word in ("edge_type", "gnn_relations", "forward_types", "Project", "edge_attr"):
        assert word in gnnb.RGCNConv_GNNB.__doc__, word
    for word in ("num_bases", "num_blocks", "root_weight=False", "bias=False", "self loop", "(v, v)", "glorot"):
        assert word in gnnb.models._RGCNConv.__doc__, word


def test_gnn_model_spec_and_parameter_names():
    model = make_rgcn_model(in_dim=9, hidden=32, layers=3, relations=4)
    spec = model.spec()
    assert spec["conv"] == "rgcn" and spec["relations"] == 4 and "heads" not in spec and "steps" not in spec
    assert spec["edge_dim"] == 0 and spec["num_layers"] == 3
    assert "relations" not in make_model("gin", hidden=16).spec()
    assert gnnb.RGCNConv_GNNB in gnnb.models.SUPPORTED_GNN_CONVS and "RGCNConv_GNNB" in gnnb.__all__
    assert gnnb.models._CONV_NAME[gnnb.RGCNConv_GNNB] == "rgcn" and gnnb.models.MAX_RGCN_RELATIONS == 8
    names = model.canonical_param_names()
    assert names[:9] == [f"gnn_convs_{l}_{p}" for l in range(3) for p in ("conv_weight", "conv_root", "conv_bias")]
    assert names[9:] == [f"mlp_head_linear_layers_{i}_{p}" for i in range(3) for p in ("weight", "bias")]
    shapes = [tuple(p.shape) for p in model.canonical_params()]
    assert shapes[:6] == [(4, 9, 32), (9, 32), (32,), (4, 32, 32), (32, 32), (32,)]
    params = model.canonical_params()
    assert torch.equal(params[0], model.gnn_convs[0].conv.weight) and torch.equal(params[2], model.gnn_convs[0].conv.bias)
    keys = [k for k in model.state_dict() if k.startswith("gnn_convs.1.")]
    assert sorted(keys) == sorted("gnn_convs.1." + k for k in KEYS)


def _qm9_like(fin, seed):
    b = synthetic.make_batch("qm9", 6, seed=seed)
    rng = np.random.default_rng(seed)
    return pack_graphs([(rng.uniform(-1, 1, (b.graph(g)[0].shape[0], fin)).astype(np.float32), b.graph(g)[1]) for g in range(6)])


@pytest.mark.parametrize("skip", [True, False])
@pytest.mark.parametrize("layers", [1, 2, 3])
def test_gnn_model_stacks_layers(layers, skip):
    """The stack in float64 against the restatement layer by layer: the skip term on middle layers only, the activation behind
    it; the same ``edge_type`` for every layer; ``edge_attr`` ignored."""
    model = make_rgcn_model(in_dim=9, hidden=24, layers=layers, relations=3, act="tanh", skip=skip).double()
    b = _qm9_like(9, seed=5 + layers)
    types = np.random.default_rng(layers).integers(0, 3, b.num_edges)
    ei, et = _ei(b.coo), torch.from_numpy(types)
    batch = torch.from_numpy(np.repeat(np.arange(b.num_graphs), np.diff(b.node_ptr)).astype(np.int64))
    with torch.no_grad():
        out = model(torch.from_numpy(b.x).double(), ei, batch, edge_type=et)
        out_ea = model(torch.from_numpy(b.x).double(), ei, batch, torch.ones(b.num_edges, 3, dtype=torch.float64), edge_type=et)
    assert out.shape == (b.num_graphs, 19) and torch.isfinite(out).all() and torch.equal(out, out_ea)
    h = b.x.astype(np.float64)
    for l, conv in enumerate(model.gnn_convs):
        sd = {k: v.numpy() for k, v in conv.state_dict().items()}
        p = np.concatenate([h @ sd["conv.weight"][r] for r in range(3)], 1)
        h = rgcn_ref(p, h @ sd["conv.root"] + sd["conv.bias"], h if (skip and 0 < l < layers - 1) else None, "tanh", b.coo, types, 3)
    with torch.no_grad():
        want = model.mlp_head(model.global_pooling(torch.from_numpy(h), batch)).numpy()
    assert np.abs(out.numpy() - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def _gnn(in_dim, hidden, layers, out_dim, conv=None, **kw):
    return gnnb.GNNModel(in_dim, None, hidden, layers, out_dim, conv or gnnb.RGCNConv_GNNB, torch.nn.ReLU, True,
                         gnnb.GlobalPooling(["add"]), gnnb.MLP(out_dim, 2), None, **kw)


def test_value_errors():
    for bad in (0, 9, 2.0, True, None):
        with pytest.raises(ValueError, match="gnn_relations"):
            _gnn(9, 16, 2, 16, gnn_relations=bad)
    assert _gnn(9, 16, 2, 16, gnn_relations=8).gnn_relations == 8 and _gnn(9, 16, 2, 16).gnn_relations == 1
    for conv in (gnnb.GINConv_GNNB, gnnb.GatedGraphConv_GNNB):  # (relations are this conv's alone)
        with pytest.raises(ValueError, match="gnn_relations"):
            _gnn(9, 16, 2, 16, conv=conv, gnn_relations=2)
        assert _gnn(9, 16, 2, 16, conv=conv, gnn_relations=1).gnn_relations == 1
    with pytest.raises(ValueError, match="gnn_heads"):
        _gnn(9, 16, 2, 16, gnn_heads=2)
    with pytest.raises(ValueError, match="gnn_steps"):
        _gnn(9, 16, 2, 16, gnn_steps=2)
    assert _gnn(17, 16, 2, 12, gnn_relations=2).gnn_layer_sizes == [(17, 16), (16, 12)]  # (a layer may narrow its input)
    # edge_type is required by such a model, refused out of range, and ignored by the others
    model = _gnn(5, 8, 2, 8, gnn_relations=3)
    x, coo = looped_graph(30, 5, seed=2)
    xt, ei = torch.from_numpy(x), _ei(coo)
    with pytest.raises(ValueError, match="needs edge_type"):
        model(xt, ei)
    with pytest.raises(ValueError, match=r"\[0, 3\)"):
        model(xt, ei, edge_type=torch.full((len(coo),), 3, dtype=torch.int64))
    assert model(xt, ei, edge_type=torch.zeros(len(coo), dtype=torch.int64)).shape == (1, 2)
    gin = _gnn(5, 8, 2, 8, conv=gnnb.GINConv_GNNB)
    with torch.no_grad():
        assert torch.equal(gin(xt, ei), gin(xt, ei, edge_type=torch.full((len(coo),), 99, dtype=torch.int64)))


def test_project_does_not_generate_rgcn_designs(tmp_path):
    with pytest.raises(NotImplementedError, match="RGCNConv"):
        gnnb.Project("rgcn", make_rgcn_model(), "regression", build_dir=tmp_path)
