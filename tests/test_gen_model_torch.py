"""GENConv's plain-torch definition (models.py, _GENConv) on the CPU against the formula's numpy restatement; argument checks; names."""
import numpy as np
import pytest
import torch

import gen_util as U
import gnnbuilder_amd as gnnb
from gnnbuilder_amd.models import _GENConv
from helpers import ACTS

# 7 nodes: node 5 has no in-edge, (0 -> 1) occurs three times, (2, 2) is an explicit self loop
COO = np.array([(0, 1), (2, 1), (0, 1), (3, 0), (2, 2), (0, 1), (4, 3), (1, 0), (6, 4), (5, 6), (3, 2), (1, 3)], np.int64)


def _layer(fi, fo, d, t, seed=3):
    torch.manual_seed(seed)
    conv = _GENConv(fi, fo, d, t).double()
    rng = np.random.default_rng(seed)
    return conv, rng.uniform(-1, 1, (7, fi)), (rng.uniform(-1, 1, (len(COO), d)) if d else None)


@pytest.mark.parametrize("d", [0, 5])
@pytest.mark.parametrize("t", [0.0, 1.0, -2.0])
@pytest.mark.parametrize("fi,fo", [(4, 4), (3, 6)])
def test_the_torch_definition_is_the_formula(fi, fo, d, t):
    conv, x, e = _layer(fi, fo, d, t)
    p = {k: v.detach().numpy() for k, v in conv.named_parameters()}
    s, r = (x, x) if fi == fo else (x @ p["lin_src.weight"].T + p["lin_src.bias"], x @ p["lin_dst.weight"].T + p["lin_dst.bias"])
    agg = U.aggregate_ref(s, COO, r, e, p.get("lin_edge.weight"), p.get("lin_edge.bias"), t)
    want = np.maximum(agg @ p["mlp.0.weight"].T + p["mlp.0.bias"], 0) @ p["mlp.2.weight"].T + p["mlp.2.bias"]
    with torch.no_grad():
        got = conv(torch.from_numpy(x), torch.from_numpy(COO.T.copy()), None if e is None else torch.from_numpy(e)).numpy()
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    base = U.aggregate_ref(s, COO, r, e, p.get("lin_edge.weight"), p.get("lin_edge.bias"), t, np.float32)
    assert np.isfinite(base).all() and 0 < np.abs(base - agg).max() < 1e-5  # (the fp32 base of the GPU tests: finite, not trivial)


def test_t_zero_is_the_mean_of_the_messages():
    _, x, e = _layer(4, 4, 5, 0.0)
    rng = np.random.default_rng(0)
    we, be = rng.uniform(-1, 1, (4, 5)), rng.uniform(-1, 1, 4)
    m = U.messages(x, COO, e, we, be)
    mean = np.zeros((7, 4))
    np.add.at(mean, COO[:, 1], m)
    mean /= np.maximum(np.bincount(COO[:, 1], minlength=7), 1)[:, None]
    np.testing.assert_allclose(U.aggregate_ref(x, COO, None, e, we, be, 0.0), mean, rtol=1e-14, atol=0)
    assert not mean[5].any()


def test_gnnmodel_argument_checks(tmp_path):
    head = lambda: (gnnb.GlobalPooling(["add"]), gnnb.MLP(8, 2, 8, 1), None)  # noqa: E731
    with pytest.raises(ValueError, match="gnn_softmax_t"):
        gnnb.GNNModel(4, None, 8, 2, 8, gnnb.GINConv_GNNB, ACTS["relu"], True, *head(), gnn_softmax_t=2.0)
    with pytest.raises(ValueError, match="graph_input_edge_dim"):
        gnnb.GNNModel(4, None, 8, 2, 8, gnnb.GENEConv_GNNB, ACTS["relu"], True, *head())
    with pytest.raises(ValueError, match="gnn_aggr"):  # (NNConv's check is what it was)
        gnnb.GNNModel(4, None, 8, 2, 8, gnnb.GENConv_GNNB, ACTS["relu"], True, *head(), gnn_aggr="mean")
    for conv, d in ((gnnb.GENConv_GNNB, None), (gnnb.GENEConv_GNNB, 3)):
        with pytest.raises(NotImplementedError, match="GENConv"):
            gnnb.Project("gen", gnnb.GNNModel(4, d, 8, 2, 8, conv, ACTS["relu"], True, *head()), "regression", build_dir=tmp_path)


def test_state_dict_keys_and_canonical_order():
    model = U.make_model(9, 12, 2, 4, t=2.0)
    conv = ["lin_src.weight", "lin_src.bias", "lin_dst.weight", "lin_dst.bias", "lin_edge.weight", "lin_edge.bias", "mlp.0.weight",
            "mlp.0.bias", "mlp.2.weight", "mlp.2.bias"]
    keys = [k for k in model.state_dict() if k.startswith("gnn_convs.")]
    assert keys == [f"gnn_convs.0.conv.{k}" for k in ["t"] + conv] + [f"gnn_convs.1.conv.{k}" for k in ["t"] + conv[4:]]
    assert model.canonical_param_names()[:16] == [f"gnn_convs_0_conv_{k.replace('.', '_')}" for k in conv] + [
        f"gnn_convs_1_conv_{k.replace('.', '_')}" for k in conv[4:]]
    assert model.spec()["conv"] == "gene" and model.spec()["softmax_t"] == [2.0, 1.75] and model.spec()["edge_dim"] == 4
    plain = U.make_model(9, 12, 2, 0)
    assert plain.spec()["conv"] == "gen" and plain.spec()["edge_dim"] == 0 and len(plain.canonical_params()) == 8 + 4 + 4
