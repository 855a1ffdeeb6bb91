"""The extension header include/gnnb_gatconv_edge.h (GAT v1 models with edge features: their creation and the fused attention
aggregate with the edge term as a stage entry) against ``runtime.ABI_GATCONV_EDGE``, the way tests/test_abi_gatconv.py holds
include/gnnb_gatconv.h against ``runtime.ABI_GATCONV``: every prototype, in the header's order, with matching ctypes types; the
library exports each one; the refusals that need no GPU.  No GPU, no compute calls."""
import ctypes as C
import re
import subprocess
from pathlib import Path

from gnnbuilder_amd import runtime
from test_abi import ctype_ok, header_text

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "gnnb_gatconv_edge.h"
PROTO = r"^([A-Za-z_][\w \*]*?)\b(gnnb_\w+)\s*\(([^)]*)\)\s*;"
OTHER_TABLES = ("ABI", "ABI_ORDER", "ABI_EDGE", "ABI_PNA_EDGE", "ABI_GAT", "ABI_GAT_EDGE", "ABI_TRANSFORMER", "ABI_TRANSFORMER_EDGE",
                "ABI_RESGATED", "ABI_RESGATED_EDGE", "ABI_GATCONV")


def prototypes(header=HEADER):
    return re.findall(PROTO, header_text(header), flags=re.M)


def test_binding_signatures_match_the_extension_header():
    protos = prototypes()
    assert len(protos) == 3 and [name for _, name, _ in protos] == list(runtime.ABI_GATCONV_EDGE)  # all of them, in the header's order
    assert list(runtime.ABI_GATCONV_EDGE) == ["gnnb_gatconv_edge_model_num_params", "gnnb_gatconv_edge_model_create", "gnnb_aggregate_gat_edges"]
    for table in OTHER_TABLES:
        assert not set(runtime.ABI_GATCONV_EDGE) & set(getattr(runtime, table)), table
    for ret, name, args in protos:
        restype, argtypes = runtime.ABI_GATCONV_EDGE[name]
        assert ctype_ok(ret, restype, is_return=True), (name, ret, restype)
        params = [a.strip() for a in args.split(",")]
        assert len(params) == len(argtypes), (name, params, argtypes)
        for p, ct in zip(params, argtypes):
            assert ctype_ok(re.sub(r"\w+$", "", p), ct), (name, p, ct)


def test_extension_header_builds_on_the_gat_header():
    text = HEADER.read_text()
    assert '#include "gnnb_gatconv.h"' in text and "#define GNNB_VERSION" not in text  # (the version is gnnb_hip.h's: 104)
    assert 'extern "C"' in text
    assert text.count("_GATEConv") >= 2 and text.count("models.py") >= 3 and "GATv1EConv_GNNB" in text
    assert "Summation order" in text and "GNNB_CONV_GCN" in text and "tsum" in text  # the header states them
    # the other extension headers keep their prototypes
    assert len(prototypes(ROOT / "include" / "gnnb_gatconv.h")) == 4 and len(prototypes(ROOT / "include" / "gnnb_gat_edge.h")) == 3
    assert len(prototypes(ROOT / "include" / "gnnb_gat.h")) == 4


def test_library_exports_and_binds_the_extension():
    if not runtime.LIB_PATH.exists():
        runtime.build_library()  # hipcc cross-compiles gfx950 without a GPU
    out = subprocess.run(["nm", "-D", "--defined-only", str(runtime.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\sT\s+(gnnb_[a-z0-9_]+)", out))
    assert not [f for f in runtime.ABI_GATCONV_EDGE if f not in exported]
    lib = runtime.load_library(require_gpu=False)
    assert lib.gnnb_version() == 104
    for name, (restype, argtypes) in runtime.ABI_GATCONV_EDGE.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    assert lib.gnnb_model_gatconv_heads(None) == 0 and lib.gnnb_model_gat_heads(None) == 0 and lib.gnnb_model_edge_dim(None) == 0


def test_model_descriptions_are_checked_on_the_host():
    """``gnnb_gatconv_edge_model_num_params``: 6 tensors per layer + the head's; what ``gnnb_gatconv_model_num_params`` refuses and
    edge_dim outside 1 .. 16 are refused; ``gnnb_gatconv_edge_model_create`` refuses a negative_slope that is not finite, before it
    looks for a device (no GPU needed).  The neighbouring kinds count what they counted."""
    from gate_util import make_gate_model
    from helpers import make_model
    lib = runtime.load_library(require_gpu=False)
    d = runtime.make_desc(make_gate_model(hidden=32, layers=3, heads=4, edge_dim=4).spec())
    assert d.conv_type == runtime.CONV["gcn"]  # a GCN description: heads, negative_slope and edge_dim travel beside it
    assert lib.gnnb_model_num_params(C.byref(d)) == 3 * 2 + 2 * 3
    for heads in (1, 2, 4, 8):
        for ed in (1, 3, 4, 16):
            assert lib.gnnb_gatconv_edge_model_num_params(C.byref(d), heads, ed) == 3 * 6 + 2 * 3
            assert lib.gnnb_gat_edge_model_num_params(C.byref(d), heads, ed) == 3 * 7 + 2 * 3  # (GATv2E's count is what it was)
        assert lib.gnnb_gatconv_model_num_params(C.byref(d), heads) == 3 * 4 + 2 * 3  # (... and the plain GAT model's)
    for bad in (0, -1, 17):
        assert lib.gnnb_gatconv_edge_model_num_params(C.byref(d), 4, bad) == -1 and b"edge_dim" in lib.gnnb_last_error()
    for bad in (0, -1, 9):
        assert lib.gnnb_gatconv_edge_model_num_params(C.byref(d), bad, 4) == -1 and b"heads" in lib.gnnb_last_error()
    assert lib.gnnb_gatconv_edge_model_num_params(C.byref(d), 3, 4) == -1 and b"divisible" in lib.gnnb_last_error()
    wide = runtime.make_desc(make_gate_model(hidden=32, out_dim=264, layers=2, heads=4).spec())
    assert lib.gnnb_gatconv_edge_model_num_params(C.byref(wide), 4, 4) == -1 and b"256" in lib.gnnb_last_error()
    wide.out_dim = 256
    assert lib.gnnb_gatconv_edge_model_num_params(C.byref(wide), 4, 4) == 2 * 6 + 2 * 3
    for conv in ("gin", "sage", "pna"):
        g = runtime.make_desc(make_model(conv, hidden=16).spec())
        assert lib.gnnb_gatconv_edge_model_num_params(C.byref(g), 4, 4) == -1 and b"GCN" in lib.gnnb_last_error()
    # anything gnnb_model_num_params refuses
    broken = runtime.make_desc(make_gate_model(hidden=32, layers=3, heads=4).spec())
    broken.num_pools = 0
    assert lib.gnnb_model_num_params(C.byref(broken)) == -1 and lib.gnnb_gatconv_edge_model_num_params(C.byref(broken), 4, 4) == -1
    # create: the same checks, the parameter count, and a finite negative_slope -- all in front of the device
    n = 3 * 6 + 2 * 3
    arr = (C.c_void_p * n)()
    handle = C.c_void_p()
    for slope in (float("nan"), float("inf"), float("-inf")):
        assert lib.gnnb_gatconv_edge_model_create(C.byref(d), 4, slope, 4, arr, n, C.byref(handle)) == -1 and not handle
        assert b"negative_slope" in lib.gnnb_last_error()
    assert lib.gnnb_gatconv_edge_model_create(C.byref(d), 0, 0.2, 4, arr, n, C.byref(handle)) == -1 and b"heads" in lib.gnnb_last_error()
    for bad in (0, 17, -1):
        assert lib.gnnb_gatconv_edge_model_create(C.byref(d), 4, 0.2, bad, arr, n, C.byref(handle)) == -1 and b"edge_dim" in lib.gnnb_last_error()
        assert not handle
    assert lib.gnnb_gatconv_edge_model_create(C.byref(d), 4, 0.2, 4, arr, n - 1, C.byref(handle)) == -1 and b"expected 24" in lib.gnnb_last_error()
    assert lib.gnnb_gatconv_edge_model_create(C.byref(d), 4, 0.2, 4, arr, 3 * 4 + 2 * 3, C.byref(handle)) == -1  # (the plain model's count)
    assert lib.gnnb_gatconv_edge_model_create(C.byref(d), 4, 0.2, 4, None, n, C.byref(handle)) == -1 and not handle
    assert lib.gnnb_gatconv_edge_model_create(C.byref(d), 4, 0.2, 4, arr, n, None) == -1
    d.fpx_w, d.fpx_i = 16, 8
    assert lib.gnnb_gatconv_edge_model_num_params(C.byref(d), 4, 4) == -1 and b"fixed-point" in lib.gnnb_last_error()
    assert lib.gnnb_gatconv_edge_model_create(C.byref(d), 4, 0.2, 4, arr, n, C.byref(handle)) == -1 and not handle


def test_the_stage_entry_refuses_on_the_host():
    """``gnnb_aggregate_gat_edges`` without a prepared workspace: GNNB_ERR_INVALID, nothing launched (no GPU needed)."""
    lib = runtime.load_library(require_gpu=False)
    assert lib.gnnb_aggregate_gat_edges(None, None, 32, None, 4, None, 4, None, None, 4, 4, 0.2, None, 4, None, 4, None, 32, None) == -1
    assert b"prepared" in lib.gnnb_last_error()
