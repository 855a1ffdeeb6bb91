"""The extension header include/gnnb_gat_edge.h (GATv2 models with edge features: their creation and the fused attention aggregate
with the edge projection as a stage entry) against ``runtime.ABI_GAT_EDGE``, the way tests/test_abi_gat.py holds
include/gnnb_gat.h against ``runtime.ABI_GAT``: every prototype, in the header's order, with matching ctypes types; the library
exports each one; the refusals that need no GPU.  No GPU, no compute calls."""
import ctypes as C
import re
import subprocess
from pathlib import Path

from gnnbuilder_amd import runtime
from test_abi import ctype_ok
from test_abi_gat import prototypes

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "gnnb_gat_edge.h"


def test_binding_signatures_match_the_extension_header():
    protos = prototypes(HEADER)
    assert len(protos) == 3 and [name for _, name, _ in protos] == list(runtime.ABI_GAT_EDGE)  # all of them, in the header's order
    others = set(runtime.ABI) | set(runtime.ABI_ORDER) | set(runtime.ABI_EDGE) | set(runtime.ABI_PNA_EDGE) | set(runtime.ABI_GAT)
    assert not set(runtime.ABI_GAT_EDGE) & others
    for ret, name, args in protos:
        restype, argtypes = runtime.ABI_GAT_EDGE[name]
        assert ctype_ok(ret, restype, is_return=True), (name, ret, restype)
        params = [a.strip() for a in args.split(",")]
        assert len(params) == len(argtypes), (name, params, argtypes)
        for p, ct in zip(params, argtypes):
            assert ctype_ok(re.sub(r"\w+$", "", p), ct), (name, p, ct)


def test_extension_header_builds_on_the_other_headers():
    text = HEADER.read_text()
    assert '#include "gnnb_gat.h"' in text and "#define GNNB_VERSION" not in text  # (the version is gnnb_hip.h's: 104)
    assert 'extern "C"' in text
    assert text.count("_GATv2EConv") >= 2 and "fill_value" in text
    assert "Summation order" in text and "GNNB_CONV_GCN" in text and "LAST" in text  # the header states the self-term-last order
    # the other extension headers keep their prototypes
    inc = ROOT / "include"
    assert [len(prototypes(inc / h)) for h in ("gnnb_edge.h", "gnnb_pna_edge.h", "gnnb_gat.h")] == [10, 3, 4]


def test_library_exports_and_binds_the_extension():
    if not runtime.LIB_PATH.exists():
        runtime.build_library()  # hipcc cross-compiles gfx950 without a GPU
    out = subprocess.run(["nm", "-D", "--defined-only", str(runtime.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\sT\s+(gnnb_[a-z0-9_]+)", out))
    assert not [f for f in runtime.ABI_GAT_EDGE if f not in exported]
    lib = runtime.load_library(require_gpu=False)
    assert lib.gnnb_version() == 104
    for name, (restype, argtypes) in runtime.ABI_GAT_EDGE.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes


def test_model_descriptions_are_checked_on_the_host():
    """``gnnb_gat_edge_model_num_params``: 7 tensors per layer + the head's; what ``gnnb_gat_model_num_params`` refuses and an
    ``edge_dim`` outside 1 .. 16 are refused; ``gnnb_gat_edge_model_create`` runs the same checks in front of the device."""
    from gatv2e_util import make_gatv2e_model
    from helpers import make_model
    lib = runtime.load_library(require_gpu=False)
    spec = make_gatv2e_model(hidden=32, layers=3, heads=4, edge_dim=3).spec()
    assert runtime._DESC_BASE["gatv2e"] == "gcn"
    d = runtime.make_desc(spec)
    assert d.conv_type == runtime.CONV["gcn"]  # a GCN description: heads, negative_slope and edge_dim travel beside it
    assert lib.gnnb_model_num_params(C.byref(d)) == 3 * 2 + 2 * 3 and lib.gnnb_gat_model_num_params(C.byref(d), 4) == 3 * 6 + 2 * 3
    for heads in (1, 2, 4, 8):
        for ed in (1, 3, 4, 16):
            assert lib.gnnb_gat_edge_model_num_params(C.byref(d), heads, ed) == 3 * 7 + 2 * 3
    for bad in (0, -1, 17):
        assert lib.gnnb_gat_edge_model_num_params(C.byref(d), 4, bad) == -1 and b"edge_dim" in lib.gnnb_last_error()
    for bad in (0, -1, 9):
        assert lib.gnnb_gat_edge_model_num_params(C.byref(d), bad, 4) == -1 and b"heads" in lib.gnnb_last_error()
    assert lib.gnnb_gat_edge_model_num_params(C.byref(d), 3, 4) == -1 and b"divisible" in lib.gnnb_last_error()
    wide = runtime.make_desc(make_gatv2e_model(hidden=32, out_dim=264, layers=2, heads=4).spec())
    assert lib.gnnb_gat_edge_model_num_params(C.byref(wide), 4, 4) == -1 and b"256" in lib.gnnb_last_error()
    for conv in ("gin", "sage", "pna"):
        g = runtime.make_desc(make_model(conv, hidden=16).spec())
        assert lib.gnnb_gat_edge_model_num_params(C.byref(g), 4, 4) == -1 and b"GCN" in lib.gnnb_last_error()
    n = 3 * 7 + 2 * 3
    arr = (C.c_void_p * n)()
    handle = C.c_void_p()
    assert lib.gnnb_gat_edge_model_create(C.byref(d), 4, float("nan"), 3, arr, n, C.byref(handle)) == -1 and not handle
    assert b"negative_slope" in lib.gnnb_last_error()
    assert lib.gnnb_gat_edge_model_create(C.byref(d), 0, 0.2, 3, arr, n, C.byref(handle)) == -1 and b"heads" in lib.gnnb_last_error()
    assert lib.gnnb_gat_edge_model_create(C.byref(d), 4, 0.2, 0, arr, n, C.byref(handle)) == -1 and b"edge_dim" in lib.gnnb_last_error()
    assert lib.gnnb_gat_edge_model_create(C.byref(d), 4, 0.2, 17, arr, n, C.byref(handle)) == -1 and b"edge_dim" in lib.gnnb_last_error()
    assert lib.gnnb_gat_edge_model_create(C.byref(d), 4, 0.2, 3, arr, n - 1, C.byref(handle)) == -1 and b"expected 27" in lib.gnnb_last_error()
    d.fpx_w, d.fpx_i = 16, 8
    assert lib.gnnb_gat_edge_model_num_params(C.byref(d), 4, 3) == -1 and b"fixed-point" in lib.gnnb_last_error()
    assert lib.gnnb_gat_edge_model_create(C.byref(d), 4, 0.2, 3, arr, n, C.byref(handle)) == -1 and not handle
    # the models without edge features count what they counted
    assert lib.gnnb_model_edge_dim(None) == 0 and lib.gnnb_model_gat_heads(None) == 0


def test_the_stage_entry_refuses_on_the_host():
    """``gnnb_aggregate_gatv2_edges`` without a prepared workspace: GNNB_ERR_INVALID, nothing launched (no GPU needed)."""
    lib = runtime.load_library(require_gpu=False)
    assert lib.gnnb_aggregate_gatv2_edges(None, None, 32, None, 32, None, None, None, 4, 4, 0.2, None, 4, None, 4, None, 32, None) == -1
    assert b"prepared" in lib.gnnb_last_error()
