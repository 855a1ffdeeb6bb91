"""SchNet's plain-torch definition (models.py, _SchNetConv) on the CPU against the formula's numpy restatement and, where it imports,
PyG's InteractionBlock; the parameter order; include/gnnb_schnet.h against ``runtime.ABI_SCHNET``.  No GPU."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import schnet_util as U
from gnnbuilder_amd import runtime
from gnnbuilder_amd.models import _SchNetConv
from test_abi import ctype_ok
from test_abi_gat import prototypes

HEADER = Path(__file__).resolve().parent.parent / "include" / "gnnb_schnet.h"
# 7 nodes: node 5 has no in-edge, (0 -> 1) occurs three times, (2, 2) is an explicit self loop
COO = np.array([(0, 1), (2, 1), (0, 1), (3, 0), (2, 2), (0, 1), (4, 3), (1, 0), (6, 4), (5, 6), (3, 2), (1, 3)], np.int64)
NAMES = ["conv.lin1.weight", "mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias", "conv.lin2.weight", "conv.lin2.bias", "lin.weight",
         "lin.bias"]


def _layer(fi, fo, g, cutoff, seed=3):
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    return _SchNetConv(fi, fo, g, cutoff).double(), rng.uniform(-1, 1, (7, fi)), rng.uniform(0.3, 1.1 * cutoff, (len(COO), 1))


@pytest.mark.parametrize("fi,fo,g", [(4, 4, 1), (3, 6, 5), (9, 12, 50)])
def test_the_torch_definition_is_the_formula(fi, fo, g):
    conv, x, d = _layer(fi, fo, g, 5.0)
    p = {k: v.detach().numpy() for k, v in conv.named_parameters()}
    assert list(p) == NAMES[1:5] + NAMES[:1] + NAMES[5:]  # (the filter MLP is registered first; conv.nn.* are its second names)
    x1 = x @ p["conv.lin1.weight"].T
    agg = U.aggregate_ref(x1, COO, d, p["mlp.0.weight"], p["mlp.0.bias"], p["mlp.2.weight"], p["mlp.2.bias"], 5.0)
    want = U.ssp(agg @ p["conv.lin2.weight"].T + p["conv.lin2.bias"]) @ p["lin.weight"].T + p["lin.bias"]
    with torch.no_grad():
        got = conv(torch.from_numpy(x), torch.from_numpy(COO.T.copy()), torch.from_numpy(d)).numpy()
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    assert not agg[5].any()
    base = U.aggregate_ref(x1, COO, d, p["mlp.0.weight"], p["mlp.0.bias"], p["mlp.2.weight"], p["mlp.2.bias"], 5.0, np.float32)
    assert np.isfinite(base).all() and 0 < np.abs(base - agg).max() < 1e-5  # (the fp32 base of the GPU tests: finite, not trivial)


def test_pygs_interaction_block_agrees():
    schnet = pytest.importorskip("torch_geometric.nn.models.schnet")
    conv, x, d = _layer(6, 6, 20, 5.0)
    block = schnet.InteractionBlock(6, 20, 6, 5.0).double()
    block.load_state_dict(conv.state_dict())
    dist = torch.from_numpy(d).reshape(-1)
    with torch.no_grad():
        want = block(torch.from_numpy(x), torch.from_numpy(COO.T.copy()), dist, schnet.GaussianSmearing(0.0, 5.0, 20).double()(dist))
        got = conv(torch.from_numpy(x), torch.from_numpy(COO.T.copy()), torch.from_numpy(d))
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-12, atol=1e-12)


def test_canonical_order_and_parameter_count():
    model = U.make_model(9, 12, 2, 5, 5.0)
    assert model.canonical_param_names()[:18] == [f"gnn_convs_{l}_conv_{n.replace('.', '_')}" for l in range(2) for n in NAMES]
    shapes = [tuple(p.shape) for p in model.canonical_params()[:9]]
    assert shapes == [(12, 9), (12, 5), (12,), (12, 12), (12,), (12, 12), (12,), (12, 12), (12,)]
    spec = model.spec()
    assert spec["conv"] == "schnet" and spec["edge_dim"] == 1 and spec["gaussians"] == 5 and spec["cutoff"] == 5.0
    lib, d = runtime.load_library(require_gpu=False), runtime.make_desc(spec)
    assert d.conv_type == runtime.CONV["gin"] and lib.gnnb_schnet_model_num_params(C.byref(d), 5) == len(model.canonical_params()) == 9 * 2 + 2 * 2
    for g in (0, 65):
        assert lib.gnnb_schnet_model_num_params(C.byref(d), g) == -1 and b"gaussians" in lib.gnnb_last_error()
    assert lib.gnnb_model_schnet(None) == 0
    assert lib.gnnb_aggregate_cfconv(None, None, 4, 4, None, None, 3, None, None, 4, None, 3, 5.0, None, 4, None) == -1 and b"prepared" in lib.gnnb_last_error()


def test_binding_signatures_match_the_extension_header_and_the_library_exports_them():
    protos = prototypes(HEADER)
    assert [name for _, name, _ in protos] == list(runtime.ABI_SCHNET) == ["gnnb_schnet_model_num_params", "gnnb_schnet_model_create",
                                                                          "gnnb_model_schnet", "gnnb_aggregate_cfconv"]
    others = [t for t in dir(runtime) if t.startswith("ABI") and t != "ABI_SCHNET"]
    assert len(others) >= 16 and not any(set(runtime.ABI_SCHNET) & set(getattr(runtime, t)) for t in others)
    for ret, name, args in protos:
        restype, argtypes = runtime.ABI_SCHNET[name]
        params = [a.strip() for a in args.split(",")]
        assert ctype_ok(ret, restype, is_return=True) and len(params) == len(argtypes), name
        for p, ct in zip(params, argtypes):
            assert ctype_ok(re.sub(r"\w+$", "", p), ct), (name, p, ct)
    if not runtime.LIB_PATH.exists():
        runtime.build_library()
    out = subprocess.run(["nm", "-D", "--defined-only", str(runtime.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert not [f for f in runtime.ABI_SCHNET if f not in set(re.findall(r"\sT\s+(gnnb_[a-z0-9_]+)", out))]
    assert runtime.load_library(require_gpu=False).gnnb_version() == 104 and len(runtime.ABI) == 45
