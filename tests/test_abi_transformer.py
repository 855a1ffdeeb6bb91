"""The extension header include/gnnb_transformer.h (TransformerConv models: their creation, the heads query and the fused
dot-product attention aggregate as a stage entry) against ``runtime.ABI_TRANSFORMER``, the way tests/test_abi_gat.py holds
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
HEADER = ROOT / "include" / "gnnb_transformer.h"
OTHER_TABLES = ("ABI", "ABI_ORDER", "ABI_EDGE", "ABI_PNA_EDGE", "ABI_GAT", "ABI_GAT_EDGE")


def test_binding_signatures_match_the_extension_header():
    protos = prototypes(HEADER)
    assert len(protos) == 4 and [name for _, name, _ in protos] == list(runtime.ABI_TRANSFORMER)  # all of them, in the header's order
    for table in OTHER_TABLES:
        assert not set(runtime.ABI_TRANSFORMER) & set(getattr(runtime, table)), table
    for ret, name, args in protos:
        restype, argtypes = runtime.ABI_TRANSFORMER[name]
        assert ctype_ok(ret, restype, is_return=True), (name, ret, restype)
        params = [a.strip() for a in args.split(",")]
        assert len(params) == len(argtypes), (name, params, argtypes)
        for p, ct in zip(params, argtypes):
            assert ctype_ok(re.sub(r"\w+$", "", p), ct), (name, p, ct)


def test_extension_header_builds_on_the_main_header():
    text = HEADER.read_text()
    assert '#include "gnnb_hip.h"' in text and "#define GNNB_VERSION" not in text  # (the version is gnnb_hip.h's: 104)
    assert 'extern "C"' in text
    assert text.count("_TransformerConv") >= 2 and text.count("models.py") >= 3
    assert "Summation order" in text and "GNNB_CONV_GIN" in text  # the header states both
    for out_of_scope in ("edge_dim", "beta", "concat", "root_weight", "dropout"):
        assert out_of_scope in text
    # the other extension headers keep their prototypes
    counts = {h: len(prototypes(ROOT / "include" / h)) for h in ("gnnb_edge.h", "gnnb_pna_edge.h", "gnnb_gat.h", "gnnb_gat_edge.h")}
    assert counts == {"gnnb_edge.h": 10, "gnnb_pna_edge.h": 3, "gnnb_gat.h": 4, "gnnb_gat_edge.h": len(runtime.ABI_GAT_EDGE)}
    assert len(runtime.ABI_GAT_EDGE) == 3


def test_library_exports_and_binds_the_extension():
    if not runtime.LIB_PATH.exists():
        runtime.build_library()  # hipcc cross-compiles gfx950 without a GPU
    out = subprocess.run(["nm", "-D", "--defined-only", str(runtime.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\sT\s+(gnnb_[a-z0-9_]+)", out))
    assert not [f for f in runtime.ABI_TRANSFORMER if f not in exported]
    lib = runtime.load_library(require_gpu=False)
    assert lib.gnnb_version() == 104
    for name, (restype, argtypes) in runtime.ABI_TRANSFORMER.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    assert lib.gnnb_model_transformer_heads(None) == 0 and lib.gnnb_model_gat_heads(None) == 0


def test_transformer_model_descriptions_are_checked_on_the_host():
    """``gnnb_transformer_model_num_params``: 8 tensors per layer + the head's; heads outside 1 .. 8, a layer width heads does not
    divide or above 256, a conv type other than GIN and the fixed-point emulation are refused; ``gnnb_transformer_model_create``
    makes the same checks and counts the parameters before it looks for a device (no GPU needed)."""
    from helpers import make_model
    from transformer_util import make_transformer_model
    lib = runtime.load_library(require_gpu=False)
    d = runtime.make_desc(make_transformer_model(hidden=32, layers=3, heads=4).spec())
    assert d.conv_type == runtime.CONV["gin"]  # a GIN description: heads travels beside it
    assert lib.gnnb_model_num_params(C.byref(d)) == 3 * 4 + 2 * 3
    for heads in (1, 2, 4, 8):
        assert lib.gnnb_transformer_model_num_params(C.byref(d), heads) == 3 * 8 + 2 * 3
    for bad in (0, -1, 9):
        assert lib.gnnb_transformer_model_num_params(C.byref(d), bad) == -1 and b"heads" in lib.gnnb_last_error()
    assert lib.gnnb_transformer_model_num_params(C.byref(d), 3) == -1 and b"divisible" in lib.gnnb_last_error()
    wide = runtime.make_desc(make_transformer_model(hidden=32, out_dim=264, layers=2, heads=4).spec())
    assert lib.gnnb_transformer_model_num_params(C.byref(wide), 4) == -1 and b"256" in lib.gnnb_last_error()
    wide.out_dim = 256
    assert lib.gnnb_transformer_model_num_params(C.byref(wide), 4) == 2 * 8 + 2 * 3
    one = runtime.make_desc(make_transformer_model(hidden=32, layers=1, heads=2, mlp_layers=1).spec())
    assert lib.gnnb_transformer_model_num_params(C.byref(one), 2) == 8 + 2 * one.mlp_num_linear and one.mlp_num_linear in (1, 2)
    for conv in ("gcn", "sage", "pna"):
        g = runtime.make_desc(make_model(conv, hidden=16).spec())
        assert lib.gnnb_transformer_model_num_params(C.byref(g), 4) == -1 and b"GIN" in lib.gnnb_last_error()
    # anything gnnb_model_num_params refuses
    broken = runtime.make_desc(make_transformer_model(hidden=32, layers=3, heads=4).spec())
    broken.num_pools = 0
    assert lib.gnnb_model_num_params(C.byref(broken)) == -1 and lib.gnnb_transformer_model_num_params(C.byref(broken), 4) == -1
    # create: the same checks and the parameter count -- all in front of the device
    n = 3 * 8 + 2 * 3
    arr = (C.c_void_p * n)()
    handle = C.c_void_p()
    create = lib.gnnb_transformer_model_create
    for bad in (0, -1, 9):
        assert create(C.byref(d), bad, arr, n, C.byref(handle)) == -1 and not handle and b"heads" in lib.gnnb_last_error()
    assert create(C.byref(d), 3, arr, n, C.byref(handle)) == -1 and b"divisible" in lib.gnnb_last_error()
    assert create(C.byref(wide), 4, arr, n, C.byref(handle)) == -1 and b"expected 22" in lib.gnnb_last_error()
    wide.out_dim = 264
    assert create(C.byref(wide), 4, arr, 22, C.byref(handle)) == -1 and b"256" in lib.gnnb_last_error()
    for conv in ("gcn", "sage", "pna"):
        g = runtime.make_desc(make_model(conv, hidden=16).spec())
        assert create(C.byref(g), 4, arr, n, C.byref(handle)) == -1 and b"GIN" in lib.gnnb_last_error()
    assert create(C.byref(d), 4, arr, n - 1, C.byref(handle)) == -1 and b"expected 30" in lib.gnnb_last_error()
    assert create(C.byref(d), 4, arr, 3 * 4 + 2 * 3, C.byref(handle)) == -1 and b"expected 30" in lib.gnnb_last_error()  # (GIN's count)
    d.fpx_w, d.fpx_i = 16, 8
    assert lib.gnnb_transformer_model_num_params(C.byref(d), 4) == -1 and b"fixed-point" in lib.gnnb_last_error()
    assert create(C.byref(d), 4, arr, n, C.byref(handle)) == -1 and not handle and b"fixed-point" in lib.gnnb_last_error()


def test_the_stage_entry_refuses_on_the_host():
    """``gnnb_aggregate_transformer`` without a prepared workspace: GNNB_ERR_INVALID, nothing launched (no GPU needed)."""
    lib = runtime.load_library(require_gpu=False)
    assert lib.gnnb_aggregate_transformer(None, None, 32, None, 32, None, 32, None, 32, None, 4, 4, 0.25, None, 32, None) == -1
    assert b"prepared" in lib.gnnb_last_error()
