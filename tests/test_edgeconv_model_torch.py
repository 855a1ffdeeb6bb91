"""EdgeConv's plain-torch definition (models.py, EdgeConv_GNNB) on the CPU against the formula's numpy restatement and, where it imports,
PyG's EdgeConv; the fold of its first linear; the parameter order; include/gnnb_edgeconv.h against ``runtime.ABI_EDGECONV``.  No GPU."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import edgeconv_util as U
import gnnbuilder_amd as gnnb
from gnnbuilder_amd import runtime
from test_abi import ctype_ok
from test_abi_gat import prototypes

# 7 nodes: node 5 has no in-edge, (0 -> 1) occurs three times, (2, 2) is an explicit self loop
COO = np.array([(0, 1), (2, 1), (0, 1), (3, 0), (2, 2), (0, 1), (4, 3), (1, 0), (6, 4), (5, 6), (3, 2), (1, 3)], np.int64)
NAMES = ["nn.0.weight", "nn.0.bias", "nn.2.weight", "nn.2.bias"]


def _layer(fi, fo, seed=3):
    torch.manual_seed(seed)
    conv = gnnb.EdgeConv_GNNB(fi, fo).double()
    with torch.no_grad():
        conv.nn[2].bias.uniform_(-0.75, -0.25)
    return conv, np.random.default_rng(seed).uniform(-1, 1, (7, fi))


@pytest.mark.parametrize("fi,fo", [(4, 4), (3, 6), (7, 32)])
def test_the_torch_definition_is_the_formula_and_so_is_the_fold(fi, fo):
    conv, x = _layer(fi, fo)
    p = {k: v.detach().numpy() for k, v in conv.named_parameters()}
    assert list(p) == NAMES
    want = U.layer_ref(x, COO, *(p[n] for n in NAMES))
    with torch.no_grad():
        got = conv(torch.from_numpy(x), torch.from_numpy(COO.T.copy())).numpy()
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    assert not want[5].any() and (want[[0, 1, 2, 3, 4, 6]] < 0).any()  # (no in-edge: 0, no bias; negative maxima survive)
    # the fold [(W1a - W1b) ; W1b], the difference in double and rounded once: a_i + b_j is nn.0([x_i | x_j - x_i]) up to that one rounding
    w1, b1 = p["nn.0.weight"].astype(np.float32), p["nn.0.bias"].astype(np.float32)
    w_ec = np.concatenate([(w1[:, :fi].astype(np.float64) - w1[:, fi:]).astype(np.float32), w1[:, fi:]]).astype(np.float64)
    ab = x @ w_ec.T + np.concatenate([b1, np.zeros_like(b1)])
    folded = U.stage_ref(ab, COO, p["nn.2.weight"], p["nn.2.bias"])
    np.testing.assert_allclose(folded, U.layer_ref(x, COO, w1, b1, p["nn.2.weight"], p["nn.2.bias"]), rtol=0, atol=1e-6)


def test_pygs_edgeconv_agrees():
    pyg = pytest.importorskip("torch_geometric.nn")
    conv, x = _layer(6, 6)
    ref = pyg.EdgeConv(torch.nn.Sequential(torch.nn.Linear(12, 6), torch.nn.ReLU(), torch.nn.Linear(6, 6)), aggr="max").double()
    ref.load_state_dict(conv.state_dict())
    with torch.no_grad():
        want = ref(torch.from_numpy(x), torch.from_numpy(COO.T.copy()))
        got = conv(torch.from_numpy(x), torch.from_numpy(COO.T.copy()))
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-12, atol=1e-12)


def test_canonical_order_parameter_count_and_aggr(tmp_path):
    model = U.make_model(7, 12, 2)
    assert model.canonical_param_names()[:8] == [f"gnn_convs_{l}_{n.replace('.', '_')}" for l in range(2) for n in NAMES]
    assert [tuple(p.shape) for p in model.canonical_params()[:4]] == [(12, 14), (12,), (12, 12), (12,)]
    spec = model.spec()
    assert spec["conv"] == "edgeconv" and spec["edge_dim"] == 0 and gnnb.EdgeConv_GNNB in gnnb.models.SUPPORTED_GNN_CONVS
    lib, d = runtime.load_library(require_gpu=False), runtime.make_desc(spec)
    assert d.conv_type == runtime.CONV["gin"] and lib.gnnb_edgeconv_model_num_params(C.byref(d)) == len(model.canonical_params()) == 4 * 2 + 2 * 2
    fpx = runtime.make_desc({**spec, "fpx": (16, 8)})
    assert lib.gnnb_edgeconv_model_num_params(C.byref(fpx)) == -1 and b"fpx_w" in lib.gnnb_last_error()
    assert lib.gnnb_aggregate_edgeconv(None, None, 8, 4, None, 4, None, 4, None, 4, None, 4, None) == -1 and b"prepared" in lib.gnnb_last_error()
    for aggr in ("add", "mean"):
        with pytest.raises(ValueError, match="'max'.*aggregate-first"):
            gnnb.GNNModel(7, None, 12, 2, 12, gnnb.EdgeConv_GNNB, torch.nn.ReLU, True, gnnb.GlobalPooling(["add"]), gnnb.MLP(12, 19, 64, 1), None,
                          gnn_aggr=aggr)
    with pytest.raises(NotImplementedError, match="EdgeConv"):
        gnnb.Project("edgeconv", model, "regression", build_dir=tmp_path)


def test_binding_signatures_match_the_extension_header_and_the_library_exports_them():
    protos = prototypes(Path(__file__).resolve().parent.parent / "include" / "gnnb_edgeconv.h")
    assert [name for _, name, _ in protos] == list(runtime.ABI_EDGECONV) == ["gnnb_edgeconv_model_num_params", "gnnb_edgeconv_model_create",
                                                                            "gnnb_model_edgeconv", "gnnb_aggregate_edgeconv"]
    others = [t for t in dir(runtime) if t.startswith("ABI") and t != "ABI_EDGECONV"]
    assert len(others) >= 17 and not any(set(runtime.ABI_EDGECONV) & set(getattr(runtime, t)) for t in others)
    for ret, name, args in protos:
        restype, argtypes = runtime.ABI_EDGECONV[name]
        params = [a.strip() for a in args.split(",")]
        assert ctype_ok(ret, restype, is_return=True) and len(params) == len(argtypes), name
        for p, ct in zip(params, argtypes):
            assert ctype_ok(re.sub(r"\w+$", "", p), ct), (name, p, ct)
    assert runtime.load_library(require_gpu=False).gnnb_version() == 104 and len(runtime.ABI) == 45  # (builds the library if need be)
    out = subprocess.run(["nm", "-D", "--defined-only", str(runtime.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert not [f for f in runtime.ABI_EDGECONV if f not in set(re.findall(r"\sT\s+(gnnb_[a-z0-9_]+)", out))]
