"""The extension header include/gnnb_transformer_edge.h (TransformerConv models with edge features: their creation and the fused
attention aggregate with the edge term as a stage entry) against ``runtime.ABI_TRANSFORMER_EDGE``, the way
tests/test_abi_transformer.py holds include/gnnb_transformer.h against ``runtime.ABI_TRANSFORMER``: every prototype, in the header's
order, with matching ctypes types; the library exports each one; the refusals that need no GPU.  No GPU, no compute calls."""
import ctypes as C
import re
import subprocess
from pathlib import Path

from gnnbuilder_amd import runtime
from test_abi import ctype_ok
from test_abi_gat import prototypes

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "gnnb_transformer_edge.h"
OTHER_TABLES = ("ABI", "ABI_ORDER", "ABI_EDGE", "ABI_PNA_EDGE", "ABI_GAT", "ABI_GAT_EDGE", "ABI_TRANSFORMER")


def test_binding_signatures_match_the_extension_header():
    protos = prototypes(HEADER)
    assert len(protos) == 3 and [name for _, name, _ in protos] == list(runtime.ABI_TRANSFORMER_EDGE)  # all of them, in the header's order
    for table in OTHER_TABLES:
        assert not set(runtime.ABI_TRANSFORMER_EDGE) & set(getattr(runtime, table)), table
    for ret, name, args in protos:
        restype, argtypes = runtime.ABI_TRANSFORMER_EDGE[name]
        assert ctype_ok(ret, restype, is_return=True), (name, ret, restype)
        params = [a.strip() for a in args.split(",")]
        assert len(params) == len(argtypes), (name, params, argtypes)
        for p, ct in zip(params, argtypes):
            assert ctype_ok(re.sub(r"\w+$", "", p), ct), (name, p, ct)


def test_extension_header_builds_on_the_main_header():
    text = HEADER.read_text()
    assert '#include "gnnb_hip.h"' in text and "#define GNNB_VERSION" not in text  # (the version is gnnb_hip.h's: 104)
    assert 'extern "C"' in text
    assert text.count("_TransformerEConv") >= 1 and text.count("models.py") >= 2
    assert "Summation order" in text and "GNNB_CONV_GIN" in text and "dot, then edge dot, then scale" in text
    for out_of_scope in ("beta", "concat", "root_weight", "dropout"):
        assert out_of_scope in text
    # the other extension headers keep their prototypes, and gnnb_transformer.h no longer calls edge_dim a follow-up
    counts = {h: len(prototypes(ROOT / "include" / h)) for h in ("gnnb_edge.h", "gnnb_pna_edge.h", "gnnb_gat.h", "gnnb_gat_edge.h", "gnnb_transformer.h")}
    assert counts == {"gnnb_edge.h": 10, "gnnb_pna_edge.h": 3, "gnnb_gat.h": 4, "gnnb_gat_edge.h": 3, "gnnb_transformer.h": 4}
    plain = (ROOT / "include" / "gnnb_transformer.h").read_text()
    assert "follow-up" not in plain and "gnnb_transformer_edge.h" in plain


def test_library_exports_and_binds_the_extension():
    if not runtime.LIB_PATH.exists():
        runtime.build_library()  # hipcc cross-compiles gfx950 without a GPU
    out = subprocess.run(["nm", "-D", "--defined-only", str(runtime.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\sT\s+(gnnb_[a-z0-9_]+)", out))
    assert not [f for f in runtime.ABI_TRANSFORMER_EDGE if f not in exported]
    lib = runtime.load_library(require_gpu=False)
    assert lib.gnnb_version() == 104
    for name, (restype, argtypes) in runtime.ABI_TRANSFORMER_EDGE.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    assert lib.gnnb_model_transformer_heads(None) == 0 and lib.gnnb_model_edge_dim(None) == 0


def test_model_descriptions_are_checked_on_the_host():
    """``gnnb_transformer_edge_model_num_params``: 9 tensors per layer + the head's; what ``gnnb_transformer_model_num_params``
    refuses, and ``edge_dim`` outside 1 .. 16; ``gnnb_transformer_edge_model_create`` makes the same checks and counts the parameters
    before it looks for a device (no GPU needed)."""
    from helpers import make_model
    from transformere_util import make_transformere_model
    lib = runtime.load_library(require_gpu=False)
    num = lib.gnnb_transformer_edge_model_num_params
    d = runtime.make_desc(make_transformere_model(hidden=32, layers=3, heads=4, edge_dim=3).spec())
    assert d.conv_type == runtime.CONV["gin"]  # a GIN description: heads and edge_dim travel beside it
    assert lib.gnnb_model_num_params(C.byref(d)) == 3 * 4 + 2 * 3 and lib.gnnb_transformer_model_num_params(C.byref(d), 4) == 3 * 8 + 2 * 3
    for heads in (1, 2, 4, 8):
        for ed in (1, 3, 4, 16):
            assert num(C.byref(d), heads, ed) == 3 * 9 + 2 * 3
    for bad in (0, -1, 17):
        assert num(C.byref(d), 4, bad) == -1 and b"edge_dim" in lib.gnnb_last_error()
    for bad in (0, -1, 9):
        assert num(C.byref(d), bad, 4) == -1 and b"heads" in lib.gnnb_last_error()
    assert num(C.byref(d), 3, 4) == -1 and b"divisible" in lib.gnnb_last_error()
    wide = runtime.make_desc(make_transformere_model(hidden=32, out_dim=264, layers=2, heads=4).spec())
    assert num(C.byref(wide), 4, 4) == -1 and b"256" in lib.gnnb_last_error()
    wide.out_dim = 256
    assert num(C.byref(wide), 4, 16) == 2 * 9 + 2 * 3
    for conv in ("gcn", "sage", "pna"):
        g = runtime.make_desc(make_model(conv, hidden=16).spec())
        assert num(C.byref(g), 4, 4) == -1 and b"GIN" in lib.gnnb_last_error()
    broken = runtime.make_desc(make_transformere_model(hidden=32, layers=3, heads=4).spec())
    broken.num_pools = 0
    assert lib.gnnb_model_num_params(C.byref(broken)) == -1 and num(C.byref(broken), 4, 4) == -1
    # create: the same checks and the parameter count -- all in front of the device
    n = 3 * 9 + 2 * 3
    arr = (C.c_void_p * n)()
    handle = C.c_void_p()
    create = lib.gnnb_transformer_edge_model_create
    for bad in (0, -1, 9):
        assert create(C.byref(d), bad, 4, arr, n, C.byref(handle)) == -1 and not handle and b"heads" in lib.gnnb_last_error()
    for bad in (0, -1, 17):
        assert create(C.byref(d), 4, bad, arr, n, C.byref(handle)) == -1 and not handle and b"edge_dim" in lib.gnnb_last_error()
    assert create(C.byref(d), 3, 4, arr, n, C.byref(handle)) == -1 and b"divisible" in lib.gnnb_last_error()
    for conv in ("gcn", "sage", "pna"):
        g = runtime.make_desc(make_model(conv, hidden=16).spec())
        assert create(C.byref(g), 4, 4, arr, n, C.byref(handle)) == -1 and b"GIN" in lib.gnnb_last_error()
    assert create(C.byref(d), 4, 4, arr, n - 1, C.byref(handle)) == -1 and b"expected 33" in lib.gnnb_last_error()
    assert create(C.byref(d), 4, 4, arr, 3 * 8 + 2 * 3, C.byref(handle)) == -1 and b"expected 33" in lib.gnnb_last_error()  # (the plain model's count)
    d.fpx_w, d.fpx_i = 16, 8
    assert num(C.byref(d), 4, 4) == -1 and b"fixed-point" in lib.gnnb_last_error()
    assert create(C.byref(d), 4, 4, arr, n, C.byref(handle)) == -1 and not handle and b"fixed-point" in lib.gnnb_last_error()


def test_the_stage_entry_refuses_on_the_host():
    """``gnnb_aggregate_transformer_edges`` without a prepared workspace: GNNB_ERR_INVALID, nothing launched (no GPU needed)."""
    lib = runtime.load_library(require_gpu=False)
    assert lib.gnnb_aggregate_transformer_edges(None, None, 32, None, 32, None, 32, None, 16, None, 32, None, 4, 4, 0.25, None, 4, None, 4, None,
                                                32, None) == -1
    assert b"prepared" in lib.gnnb_last_error()
