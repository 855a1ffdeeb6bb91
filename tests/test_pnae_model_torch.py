"""``PNAEConv_GNNB`` -- PNA with edge features, PyG's ``PNAConv(edge_dim=...)`` in plain torch -- and ``GNNModel`` stacking it (the
model definition: what a user trains and what the accelerated path, ``runtime.CompiledModel.forward_edges``, is held against in
tests/test_hip_pnae.py).  No GPU."""
import numpy as np
import pytest
import torch

import gnnbuilder_amd as gnnb
from gine_util import edge_attrs, run
from gnnbuilder_amd.batching import pack_graphs
from helpers import batch_vector, edge_batch, hub_graph, looped_graph, make_model
from pnae_util import make_pnae_model, pnae_conv64


def _graph(fin, seed):
    """``looped_graph(40, ...)`` (self loops, duplicates, isolated nodes) and a small hub graph in one batch, plus two more isolated nodes"""
    iso = (np.random.default_rng(seed).uniform(-1, 1, (2, fin)).astype(np.float32), np.zeros((0, 2), np.int32))
    return pack_graphs([looped_graph(40, fin, seed), hub_graph(30, fin, 90, seed + 1), iso])


@pytest.mark.parametrize("fin,fout,edge_dim,delta", [(9, 16, 3, 1.0), (12, 12, 5, 0.7)])
def test_conv_matches_a_per_edge_restatement_in_float64(fin, fout, edge_dim, delta):
    torch.manual_seed(fin)
    conv = gnnb.PNAEConv_GNNB(fin, fout, edge_dim, delta=delta).double()
    b = _graph(fin, seed=fin)
    deg = np.bincount(b.coo[:, 1], minlength=b.num_nodes)
    assert (deg == 0).sum() >= 5 and deg.max() >= 90
    ea = edge_attrs(b.num_edges, edge_dim, seed=fin + 1)
    with torch.no_grad():
        got = conv(torch.from_numpy(b.x).double(), torch.from_numpy(b.coo.T.astype(np.int64)), torch.from_numpy(ea).double()).numpy()
    # (delta as the model holds it, an fp32 value: PNAConv_GNNB.delta_scaler, which spec()["pna_delta"] hands to the C side)
    assert conv.delta_scaler == float(np.float32(delta))
    want = pnae_conv64(b.x, b.coo, ea, {k[len("conv."):]: v.numpy() for k, v in conv.state_dict().items()}, conv.delta_scaler)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"PNAEConv_GNNB ({fin}, {fout}, edge_dim {edge_dim}) against the per-edge restatement: {err:.3e} relative")
    assert err <= 1e-12


def test_without_the_edge_block_the_layer_is_pna_bit_for_bit():
    """W_pre[:, 2F:] = 0: the third block adds exact zeros to every message, so the layer IS ``PNAConv_GNNB`` with W_pre[:, :2F]
    -- the conv the reference's golden pins (tests/test_models_torch.py) -- in fp32, to the bit."""
    F, out, ed = 9, 16, 3
    torch.manual_seed(0)
    e, p = gnnb.PNAEConv_GNNB(F, out, ed, delta=0.8), gnnb.PNAConv_GNNB(F, out, delta=0.8)
    with torch.no_grad():
        e.conv.pre_nns[0][0].weight[:, 2 * F:] = 0.0
        p.conv.pre_nns[0][0].weight.copy_(e.conv.pre_nns[0][0].weight[:, :2 * F])
        for name in ("pre_nns.0.0.bias", "post_nns.0.0.weight", "post_nns.0.0.bias", "lin.weight", "lin.bias"):
            p.conv.state_dict()[name].copy_(e.conv.state_dict()[name])
        b = _graph(F, seed=4)
        x, ei = torch.from_numpy(b.x), torch.from_numpy(b.coo.T.astype(np.int64))
        got = e(x, ei, torch.from_numpy(edge_attrs(b.num_edges, ed, seed=5)))
        want = p(x, ei)
    assert got.dtype == torch.float32 and torch.equal(got, want)


def test_spec_parameter_names_and_state_dict():
    model = make_pnae_model(in_dim=9, edge_dim=3, hidden=32, layers=3)
    spec = model.spec()
    assert spec["conv"] == "pnae" and spec["edge_dim"] == 3 and spec["num_layers"] == 3 and spec["pna_delta"] == 1.0
    assert make_model("pna", hidden=16).spec()["edge_dim"] == 0  # (PNAConv_GNNB does not read graph_input_edge_dim)
    assert gnnb.PNAEConv_GNNB in gnnb.models.SUPPORTED_GNN_CONVS and gnnb.models._CONV_NAME[gnnb.PNAEConv_GNNB] == "pnae"
    names = model.canonical_param_names()
    per_layer = ["conv_pre_nns_0_0_weight", "conv_pre_nns_0_0_bias", "conv_post_nns_0_0_weight", "conv_post_nns_0_0_bias",
                 "conv_lin_weight", "conv_lin_bias", "conv_edge_encoder_weight", "conv_edge_encoder_bias"]
    assert names[:24] == [f"gnn_convs_{l}_{p}" for l in range(3) for p in per_layer]
    assert names[24:] == [f"mlp_head_linear_layers_{i}_{p}" for i in range(3) for p in ("weight", "bias")]
    shapes = [tuple(p.shape) for p in model.canonical_params()]
    assert shapes[:8] == [(9, 27), (9,), (32, 117), (32,), (32, 32), (32,), (9, 3), (9,)]
    assert shapes[8:16] == [(32, 96), (32,), (32, 13 * 32), (32,), (32, 32), (32,), (32, 3), (32,)]
    sd = {k: tuple(v.shape) for k, v in model.gnn_convs[1].state_dict().items()}
    assert sd == {"conv.pre_nns.0.0.weight": (32, 96), "conv.pre_nns.0.0.bias": (32,), "conv.post_nns.0.0.weight": (32, 416),
                  "conv.post_nns.0.0.bias": (32,), "conv.lin.weight": (32, 32), "conv.lin.bias": (32,),
                  "conv.edge_encoder.weight": (32, 3), "conv.edge_encoder.bias": (32,)}
    # PNAConv_GNNB keeps its state_dict: scripts written against the reference pass graph_input_edge_dim with every conv
    torch.manual_seed(0)
    pna = gnnb.GNNModel(9, 3, 16, 2, 16, gnnb.PNAConv_GNNB, torch.nn.ReLU, True, gnnb.GlobalPooling(["add"]), gnnb.MLP(16, 2), None)
    assert tuple(pna.gnn_convs[0].state_dict()["conv.pre_nns.0.0.weight"].shape) == (9, 18) and pna.spec()["conv"] == "pna"
    assert not any("edge_encoder" in k for k in pna.state_dict())


def test_a_pnae_model_needs_its_edge_features():
    model = make_pnae_model()
    b = edge_batch(4, 9, seed=3, hub=False)
    ei = torch.from_numpy(np.ascontiguousarray(b.coo.T.astype(np.int64)))
    with pytest.raises(ValueError, match="edge_attr"):
        model(torch.from_numpy(b.x), ei, torch.from_numpy(batch_vector(b)))
    for bad in (None, 0, 17):
        with pytest.raises(ValueError, match="graph_input_edge_dim"):
            make_pnae_model(edge_dim=bad)
    ea = edge_attrs(b.num_edges, 3, seed=4)
    with torch.no_grad():
        out = model(torch.from_numpy(b.x), ei, torch.from_numpy(batch_vector(b)), torch.from_numpy(ea))
        other = model(torch.from_numpy(b.x), ei, torch.from_numpy(batch_vector(b)), torch.from_numpy(-ea))
    assert out.shape == (b.num_graphs, 19) and torch.isfinite(out).all() and not torch.equal(out, other)
    assert np.array_equal(out.numpy(), run(model, b, b.x, ea))  # (the layer walk the GPU tests use as their reference)


def test_project_does_not_generate_pnae_designs(tmp_path):
    with pytest.raises(NotImplementedError, match="PNAE"):
        gnnb.Project("pnae", make_pnae_model(), "regression", build_dir=tmp_path)
