"""The extension header include/gnnb_resgated_edge.h (ResGatedGraphConv models with edge features: their creation and the fused
gated aggregate with its edge terms as a stage entry) against ``runtime.ABI_RESGATED_EDGE``, the way tests/test_abi_resgated.py
holds include/gnnb_resgated.h against ``runtime.ABI_RESGATED``: every prototype, in the header's order, with matching ctypes
types; the library exports each one; the refusals that need no GPU.  No GPU, no compute calls."""
import ctypes as C
import re
import subprocess
from pathlib import Path

from gnnbuilder_amd import runtime
from test_abi import ctype_ok
from test_abi_gat import prototypes

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "gnnb_resgated_edge.h"
OTHER_TABLES = ("ABI", "ABI_ORDER", "ABI_EDGE", "ABI_PNA_EDGE", "ABI_GAT", "ABI_GAT_EDGE", "ABI_TRANSFORMER", "ABI_TRANSFORMER_EDGE",
                "ABI_RESGATED")


def test_binding_signatures_match_the_extension_header():
    protos = prototypes(HEADER)
    assert len(protos) == 3 and [name for _, name, _ in protos] == list(runtime.ABI_RESGATED_EDGE)  # all of them, in the header's order
    assert list(runtime.ABI_RESGATED_EDGE) == ["gnnb_resgated_edge_model_num_params", "gnnb_resgated_edge_model_create",
                                               "gnnb_aggregate_resgated_edges"]
    for table in OTHER_TABLES:
        assert not set(runtime.ABI_RESGATED_EDGE) & set(getattr(runtime, table)), table
    for ret, name, args in protos:
        restype, argtypes = runtime.ABI_RESGATED_EDGE[name]
        assert ctype_ok(ret, restype, is_return=True), (name, ret, restype)
        params = [a.strip() for a in args.split(",")]
        assert len(params) == len(argtypes), (name, params, argtypes)
        for p, ct in zip(params, argtypes):
            assert ctype_ok(re.sub(r"\w+$", "", p), ct), (name, p, ct)


def test_extension_header_builds_on_the_main_header():
    text = HEADER.read_text()
    assert '#include "gnnb_hip.h"' in text and "#define GNNB_VERSION" not in text  # (the version is gnnb_hip.h's: 104)
    assert 'extern "C"' in text
    assert text.count("_ResGatedGraphEConv") >= 1 and text.count("models.py") >= 2
    # the layer, the split, the fold, the gate, the order, the refusals
    for phrase in ("x columns first", "W_g = W_ke + W_qe", "in double, rounded once", "b_q is NOT folded", "Summation order", "d increasing",
                   "exactly 0", "GNNB_CONV_GIN", "gnnb_forward_pyg_ordered", "separate operands on purpose", "bit for bit"):
        assert phrase in text, phrase
    for out_of_scope in ("root_weight = False", "bias = False", "other than sigmoid", "above 256", "above 16"):
        assert out_of_scope in text
    # gnnb_resgated.h keeps its four prototypes and points here; the other extension headers keep theirs
    assert "gnnb_resgated_edge.h" in (ROOT / "include" / "gnnb_resgated.h").read_text()
    counts = {h: len(prototypes(ROOT / "include" / h)) for h in ("gnnb_edge.h", "gnnb_pna_edge.h", "gnnb_gat.h", "gnnb_gat_edge.h",
                                                                 "gnnb_transformer.h", "gnnb_transformer_edge.h", "gnnb_resgated.h")}
    assert counts == {"gnnb_edge.h": 10, "gnnb_pna_edge.h": 3, "gnnb_gat.h": 4, "gnnb_gat_edge.h": 3, "gnnb_transformer.h": 4,
                      "gnnb_transformer_edge.h": 3, "gnnb_resgated.h": 4}


def test_library_exports_and_binds_the_extension():
    if not runtime.LIB_PATH.exists():
        runtime.build_library()  # hipcc cross-compiles gfx950 without a GPU
    out = subprocess.run(["nm", "-D", "--defined-only", str(runtime.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\sT\s+(gnnb_[a-z0-9_]+)", out))
    assert not [f for f in runtime.ABI_RESGATED_EDGE if f not in exported]
    lib = runtime.load_library(require_gpu=False)
    assert lib.gnnb_version() == 104
    for name, (restype, argtypes) in runtime.ABI_RESGATED_EDGE.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    assert lib.gnnb_model_is_resgated(None) == 0 and lib.gnnb_model_edge_dim(None) == 0


def test_model_descriptions_are_checked_on_the_host():
    """``gnnb_resgated_edge_model_num_params``: 8 tensors per layer + the head's; what ``gnnb_resgated_model_num_params`` refuses and
    an ``edge_dim`` outside 1 .. 16 are refused with a message; ``gnnb_resgated_edge_model_create`` makes the same checks and counts
    the parameters before it looks for a device (no GPU needed)."""
    from helpers import make_model
    from resgatede_util import make_resgatede_model
    lib = runtime.load_library(require_gpu=False)
    num = lib.gnnb_resgated_edge_model_num_params
    for layers in (1, 2, 3):
        for mlp_layers in (1, 2):
            dd = runtime.make_desc(make_resgatede_model(hidden=32, layers=layers, mlp_layers=mlp_layers).spec())
            for ed in (1, 4, 16):
                assert num(C.byref(dd), ed) == 8 * layers + 2 * (mlp_layers + 1)
    d = runtime.make_desc(make_resgatede_model(hidden=32, layers=3).spec())
    assert d.conv_type == runtime.CONV["gin"]  # a GIN description: the "gated" mark and edge_dim travel beside it
    assert lib.gnnb_resgated_model_num_params(C.byref(d)) == 3 * 8 + 2 * 3 and lib.gnnb_edge_model_num_params(C.byref(d), 4) == 3 * 6 + 2 * 3
    for ed in (0, -1, 17):
        assert num(C.byref(d), ed) == -1 and b"1 .. 16" in lib.gnnb_last_error(), ed
    wide = runtime.make_desc(make_resgatede_model(hidden=32, out_dim=264, layers=2).spec())
    assert num(C.byref(wide), 4) == -1 and b"256" in lib.gnnb_last_error()
    wide.out_dim = 256
    assert num(C.byref(wide), 16) == 2 * 8 + 2 * 3
    for conv in ("gcn", "sage", "pna"):
        g = runtime.make_desc(make_model(conv, hidden=16).spec())
        assert num(C.byref(g), 4) == -1 and b"GIN" in lib.gnnb_last_error()
    broken = runtime.make_desc(make_resgatede_model(hidden=32, layers=3).spec())
    broken.num_pools = 0
    assert num(C.byref(broken), 4) == -1
    # create: the same checks and the parameter count -- all in front of the device
    n = 3 * 8 + 2 * 3
    arr = (C.c_void_p * n)()
    handle = C.c_void_p()
    create = lib.gnnb_resgated_edge_model_create
    for conv in ("gcn", "sage", "pna"):
        g = runtime.make_desc(make_model(conv, hidden=16).spec())
        assert create(C.byref(g), 4, arr, n, C.byref(handle)) == -1 and not handle and b"GIN" in lib.gnnb_last_error()
    assert create(C.byref(broken), 4, arr, n, C.byref(handle)) == -1 and not handle
    for ed in (0, 17):
        assert create(C.byref(d), ed, arr, n, C.byref(handle)) == -1 and not handle and b"1 .. 16" in lib.gnnb_last_error()
    assert create(C.byref(d), 4, arr, n - 1, C.byref(handle)) == -1 and b"expected 30" in lib.gnnb_last_error()
    assert create(C.byref(d), 4, arr, 3 * 6 + 2 * 3, C.byref(handle)) == -1 and b"expected 30" in lib.gnnb_last_error()  # (a GINE model's count)
    assert create(C.byref(d), 4, arr, n, C.byref(handle)) == -1 and not handle and b"parameter 0 is NULL" in lib.gnnb_last_error()
    assert create(C.byref(d), 4, arr, n, None) == -1 and b"out_model" in lib.gnnb_last_error()
    d.fpx_w, d.fpx_i = 16, 8
    assert num(C.byref(d), 4) == -1 and b"fixed-point" in lib.gnnb_last_error()
    assert create(C.byref(d), 4, arr, n, C.byref(handle)) == -1 and not handle and b"fixed-point" in lib.gnnb_last_error()


def test_the_stage_entry_refuses_on_the_host():
    """``gnnb_aggregate_resgated_edges`` without a prepared workspace: GNNB_ERR_INVALID, nothing launched (no GPU needed)."""
    lib = runtime.load_library(require_gpu=False)
    assert lib.gnnb_aggregate_resgated_edges(None, None, 32, None, 32, None, 32, None, 32, None, 4, None, 4, None, 4, None, 4, None, 32,
                                             None) == -1
    assert b"prepared" in lib.gnnb_last_error()
