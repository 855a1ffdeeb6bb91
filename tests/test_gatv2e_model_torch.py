"""``GATv2EConv_GNNB`` -- PyG's ``GATv2Conv(edge_dim=d, fill_value='mean')`` in plain torch -- and ``GNNModel`` stacking it (the
model definition: what a user trains and what the accelerated path, ``runtime.CompiledModel.forward_edges``, is held against in
tests/test_hip_gatv2e.py).  No GPU."""
import numpy as np
import pytest
import torch

import gnnbuilder_amd as gnnb
from gatv2_util import make_gatv2_model
from gatv2e_util import gatv2e_ref, make_gatv2e_model
from helpers import looped_graph, make_model


def _conv_operands(conv, x):
    """(xl, xr, att, bias, w_edge) of ``conv`` (a ``GATv2EConv_GNNB`` in float64) on ``x``, as float64 arrays: the two linears are
    plain matrix products here, so that ``gatv2e_ref`` restates everything behind them."""
    sd = {k: v.numpy().astype(np.float64) for k, v in conv.state_dict().items()}
    x = np.asarray(x, np.float64)
    return (x @ sd["conv.lin_l.weight"].T + sd["conv.lin_l.bias"], x @ sd["conv.lin_r.weight"].T + sd["conv.lin_r.bias"],
            sd["conv.att"].reshape(-1), sd["conv.bias"], sd["conv.lin_edge.weight"])


def _randomise_biases(conv, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in conv.named_parameters():
            if n.endswith("bias"):
                p.copy_(torch.rand(p.shape, generator=g, dtype=p.dtype) * 0.2 - 0.1)


def _apply(conv, x, coo, ea):
    dtype = next(conv.parameters()).dtype
    with torch.no_grad():
        return conv(torch.from_numpy(np.asarray(x)).to(dtype), torch.from_numpy(np.ascontiguousarray(np.asarray(coo).reshape(-1, 2).T.astype(np.int64))),
                    torch.from_numpy(np.asarray(ea)).to(dtype)).numpy()


def _conv(fin, fout, d, heads, slope=0.2, seed=0):
    torch.manual_seed(seed)
    conv = gnnb.GATv2EConv_GNNB(fin, fout, d, heads=heads, negative_slope=slope).double()
    _randomise_biases(conv, seed + 1)
    return conv


def _against_ref(conv, x, coo, ea, heads, slope):
    got = _apply(conv, x, coo, ea)
    xl, xr, att, bias, we = _conv_operands(conv, x)
    want = gatv2e_ref(xl, xr, att, bias, None, "none", coo, ea, we, heads, slope)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"GATv2EConv_GNNB against the two-pass restatement: {err:.3e} relative")
    assert got.shape == want.shape and err <= 1e-12
    return got, (xl, xr, att, bias, we)


# five nodes by hand: node 0 has no in-edge, node 1 has in-degree 3 (a mean that is not dyadic), node 2 in-degree 2, 3 and 4 one each
HAND_COO = np.array([[0, 1], [2, 1], [3, 1], [1, 2], [4, 2], [2, 3], [0, 4]], np.int64)


@pytest.mark.parametrize("d,heads,fout", [(1, 1, 8), (3, 3, 9), (4, 2, 8), (16, 4, 16)])
def test_hand_made_graph_with_a_node_of_in_degree_0_and_one_of_in_degree_3(d, heads, fout):
    rng = np.random.default_rng(d)
    x, ea = rng.uniform(-1, 1, (5, 6)), rng.uniform(-1, 1, (len(HAND_COO), d))
    deg = np.bincount(HAND_COO[:, 1], minlength=5)
    assert deg[0] == 0 and deg[1] == 3
    conv = _conv(6, fout, d, heads, seed=d)
    got, (xl, xr, att, bias, we) = _against_ref(conv, x, HAND_COO, ea, heads, 0.2)
    assert np.abs(got[0] - (xl[0] + bias)).max() <= 1e-15  # in-degree 0: the self term alone (its attribute is 0, its weight 1)
    # the mean matters: with the self loops' attributes 0 the result differs on the rows that have in-edges, and only there
    zero_fill = gatv2e_ref(xl, xr, att, bias, None, "none", HAND_COO, ea, we, heads, 0.2, fill=0)
    diff = np.abs(got - zero_fill).max(1)
    assert diff[0] <= 1e-15 and (diff[1:] > 1e-6).all()
    # ... and so do the attributes at all: W_e = 0 gives another result on those rows
    no_edge = gatv2e_ref(xl, xr, att, bias, None, "none", HAND_COO, ea, np.zeros_like(we), heads, 0.2)
    assert (np.abs(got - no_edge).max(1)[1:] > 1e-6).all()


@pytest.mark.parametrize("fin,fout,d,heads,slope", [(9, 16, 3, 1, 0.2), (11, 24, 4, 4, 0.2), (7, 9, 16, 3, 0.05)])
def test_conv_matches_the_two_pass_restatement_on_a_looped_graph(fin, fout, d, heads, slope):
    x, coo = looped_graph(40, fin, seed=fin)
    assert (coo[:, 0] == coo[:, 1]).sum() >= 10
    ea = np.random.default_rng(fin).uniform(-1, 1, (len(coo), d))
    _against_ref(_conv(fin, fout, d, heads, slope, seed=fin), x, coo, ea, heads, slope)


def test_explicit_self_loops_with_nan_attributes_change_nothing():
    x, coo = looped_graph(40, 9, seed=2)
    loops = coo[:, 0] == coo[:, 1]
    assert loops.sum() >= 10
    ea = np.random.default_rng(3).uniform(-1, 1, (len(coo), 4))
    ea[loops] = np.nan  # removed together with their edges: never read, never part of a mean
    conv = _conv(9, 16, 4, 2, seed=1)
    with_loops = _apply(conv, x, coo, ea)
    assert np.isfinite(with_loops).all()
    assert np.array_equal(with_loops, _apply(conv, x, coo[~loops], ea[~loops]))


def test_without_edges_every_row_is_lin_l_plus_bias():
    conv = _conv(6, 8, 3, 2, seed=4)
    x = np.random.default_rng(0).uniform(-1, 1, (4, 6))
    got = _apply(conv, x, np.zeros((0, 2), np.int64), np.zeros((0, 3)))
    xl, _, _, bias, _ = _conv_operands(conv, x)
    assert np.abs(got - (xl + bias)).max() <= 1e-15


def test_state_dict_names_shapes_and_initialisation():
    torch.manual_seed(0)
    conv = gnnb.GATv2EConv_GNNB(9, 32, 3, heads=4)
    sd = {k: tuple(v.shape) for k, v in conv.state_dict().items()}
    assert sd == {"conv.att": (1, 4, 8), "conv.bias": (32,), "conv.lin_l.weight": (32, 9), "conv.lin_l.bias": (32,),
                  "conv.lin_r.weight": (32, 9), "conv.lin_r.bias": (32,), "conv.lin_edge.weight": (32, 3)}  # (lin_edge has no bias)
    bound = (6 / (32 + 3)) ** 0.5  # glorot
    v = conv.state_dict()["conv.lin_edge.weight"]
    assert v.abs().max() <= bound and v.abs().max() > 0.5 * bound
    assert conv.heads == 4 and conv.edge_dim == 3 and conv.negative_slope == 0.2 and conv.in_channels == 9 and conv.out_channels == 32


def test_gnn_model_spec_and_parameter_names():
    model = make_gatv2e_model(in_dim=9, edge_dim=3, hidden=32, layers=3, heads=4)
    spec = model.spec()
    assert spec["conv"] == "gatv2e" and spec["heads"] == 4 and spec["negative_slope"] == 0.2 and spec["edge_dim"] == 3 and spec["num_layers"] == 3
    assert gnnb.GATv2EConv_GNNB in gnnb.models.SUPPORTED_GNN_CONVS and gnnb.models._CONV_NAME[gnnb.GATv2EConv_GNNB] == "gatv2e"
    assert gnnb.models._EDGE_CONVS[gnnb.GATv2EConv_GNNB] == "GATv2E"
    names = model.canonical_param_names()
    per_layer = ["conv_lin_l_weight", "conv_lin_l_bias", "conv_lin_r_weight", "conv_lin_r_bias", "conv_att", "conv_bias", "conv_lin_edge_weight"]
    assert names[:21] == [f"gnn_convs_{l}_{p}" for l in range(3) for p in per_layer]
    assert names[21:] == [f"mlp_head_linear_layers_{i}_{p}" for i in range(3) for p in ("weight", "bias")]
    shapes = [tuple(p.shape) for p in model.canonical_params()]
    assert shapes[:7] == [(32, 9), (32,), (32, 9), (32,), (1, 4, 8), (32,), (32, 3)]
    assert shapes[7:14] == [(32, 32), (32,), (32, 32), (32,), (1, 4, 8), (32,), (32, 3)]
    x, coo = looped_graph(40, 9, seed=5)
    ea = torch.from_numpy(np.random.default_rng(5).uniform(-1, 1, (len(coo), 3)).astype(np.float32))
    ei = torch.from_numpy(np.ascontiguousarray(coo.T.astype(np.int64)))
    with torch.no_grad():
        out = model(torch.from_numpy(x), ei, None, ea)
    assert out.shape == (1, 19) and torch.isfinite(out).all()
    with pytest.raises(ValueError, match="GATv2E model needs edge_attr"):
        model(torch.from_numpy(x), ei)


def test_the_plain_gatv2_model_is_what_it_was():
    plain = make_gatv2_model(in_dim=9, hidden=32, layers=3, heads=4)
    assert plain.spec() == {"conv": "gatv2", "num_layers": 3, "in_dim": 9, "hidden_dim": 32, "out_dim": 32, "activation": "relu", "skip": True,
                            "pools": ["add", "mean", "max"], "mlp_hidden_layers": 2, "mlp_hidden": 64, "mlp_out": 19, "mlp_activation": "relu",
                            "gin_eps": 0.0, "edge_dim": 0, "pna_delta": 1.0, "output_activation": None, "heads": 4, "negative_slope": 0.2}
    assert len(plain.canonical_param_names()) == 6 * 3 + 2 * 3
    assert "conv.lin_edge.weight" not in plain.gnn_convs[0].state_dict()
    # ... and it still ignores graph_input_edge_dim and edge_attr
    torch.manual_seed(0)
    m = gnnb.GNNModel(9, 4, 16, 2, 16, gnnb.GATv2Conv_GNNB, torch.nn.ReLU, True, gnnb.GlobalPooling(["add"]), gnnb.MLP(16, 2), None, gnn_heads=2)
    assert m.spec()["edge_dim"] == 0 and m.spec()["conv"] == "gatv2"
    assert "heads" not in make_model("gcn", hidden=16).spec()


def test_value_errors():
    with pytest.raises(ValueError, match="divisible"):
        gnnb.GATv2EConv_GNNB(9, 30, 4, heads=4)
    for bad in (0, 9, -1, 2.0, True):
        with pytest.raises(ValueError, match="heads"):
            gnnb.GATv2EConv_GNNB(9, 32, 4, heads=bad)
    for bad in (0, 17, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="edge_dim"):
            gnnb.GATv2EConv_GNNB(9, 32, bad, heads=4)
        with pytest.raises(ValueError, match="GATv2E model needs graph_input_edge_dim"):
            make_gatv2e_model(edge_dim=bad)
    with pytest.raises(ValueError, match="divisible"):
        make_gatv2e_model(hidden=30, out_dim=32, heads=4)
    with pytest.raises(ValueError, match="divisible"):
        make_gatv2e_model(hidden=32, out_dim=30, heads=4)
    for bad in (0, 9, True):
        with pytest.raises(ValueError, match="gnn_heads"):
            make_gatv2e_model(heads=bad)
    assert make_gatv2e_model(hidden=30, out_dim=32, layers=1, heads=4).spec()["out_dim"] == 32


def test_project_does_not_generate_such_designs(tmp_path):
    with pytest.raises(NotImplementedError, match="GATv2 designs with edge features"):
        gnnb.Project("gatv2e", make_gatv2e_model(), "regression", build_dir=tmp_path)


def test_equal_to_pyg_after_load_state_dict():
    pyg_nn = pytest.importorskip("torch_geometric.nn")
    ours = _conv(9, 24, 4, 3, seed=5)
    theirs = pyg_nn.GATv2Conv(9, 8, heads=3, concat=True, negative_slope=0.2, add_self_loops=True, bias=True, share_weights=False, edge_dim=4,
                              fill_value="mean").double()
    theirs.load_state_dict({k[len("conv."):]: v for k, v in ours.state_dict().items()})
    x, coo = looped_graph(40, 9, seed=6)
    ea = np.random.default_rng(6).uniform(-1, 1, (len(coo), 4))
    with torch.no_grad():
        want = theirs(torch.from_numpy(x).double(), torch.from_numpy(np.ascontiguousarray(coo.T.astype(np.int64))), torch.from_numpy(ea)).numpy()
    assert np.abs(_apply(ours, x, coo, ea) - want).max() <= 1e-12
