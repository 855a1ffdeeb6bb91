"""The extension header include/gnnb_rgcn.h (RGCNConv models with integer edge types: their creation, the _types forwards, the
type ingest and the two stage entries) against ``runtime.ABI_RGCN``, the way tests/test_abi_ggnn.py holds include/gnnb_ggnn.h
against ``runtime.ABI_GGNN``: every prototype, in the header's order, with matching ctypes types; the library exports each one;
the refusals that need no GPU.  No GPU, no compute calls."""
import ctypes as C
import re
import subprocess
from pathlib import Path

from gnnbuilder_amd import runtime
from test_abi import ctype_ok
from test_abi_gat import prototypes

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "gnnb_rgcn.h"
OTHER_TABLES = ("ABI", "ABI_ORDER", "ABI_EDGE", "ABI_PNA_EDGE", "ABI_GAT", "ABI_GAT_EDGE", "ABI_TRANSFORMER", "ABI_TRANSFORMER_EDGE",
                "ABI_RESGATED", "ABI_RESGATED_EDGE", "ABI_GATCONV", "ABI_GATCONV_EDGE", "ABI_GGNN")


def test_binding_signatures_match_the_extension_header():
    protos = prototypes(HEADER)
    assert len(protos) == 11 and [name for _, name, _ in protos] == list(runtime.ABI_RGCN)  # all of them, in the header's order
    assert list(runtime.ABI_RGCN) == ["gnnb_rgcn_model_num_params", "gnnb_rgcn_model_create", "gnnb_model_rgcn_relations",
                                      "gnnb_forward_batched_types", "gnnb_forward_prepared_types", "gnnb_type_ingest_bytes",
                                      "gnnb_workspace_enable_type_ingest", "gnnb_ingest_pyg_types", "gnnb_forward_pyg_types",
                                      "gnnb_rgcn_slots", "gnnb_aggregate_rgcn"]
    for table in OTHER_TABLES:
        assert not set(runtime.ABI_RGCN) & set(getattr(runtime, table)), table
    for ret, name, args in protos:
        restype, argtypes = runtime.ABI_RGCN[name]
        assert ctype_ok(ret, restype, is_return=True), (name, ret, restype)
        params = [a.strip() for a in args.split(",")]
        assert len(params) == len(argtypes), (name, params, argtypes)
        for p, ct in zip(params, argtypes):
            assert ctype_ok(re.sub(r"\w+$", "", p), ct), (name, p, ct)


def test_extension_header_builds_on_the_main_header():
    text = HEADER.read_text()
    assert '#include "gnnb_hip.h"' in text and "#define GNNB_VERSION" not in text  # (the version is gnnb_hip.h's: 104)
    assert 'extern "C"' in text
    assert text.count("_RGCNConv") >= 1 and text.count("models.py") >= 2
    assert "Summation order" in text and "GNNB_CONV_GIN" in text and "take NO bias" in text and "flag 256" in text
    assert "w_rgcn = [weight[0]^T ; .. ; weight[R-1]^T ; root^T]" in text and "b_rgcn = [0 | .. | 0 | bias]" in text
    for out_of_scope in ("num_bases", "num_blocks", "aggr other than mean", "root_weight = False", "bias = False", "more than 8 relations",
                         "widths above 256", "per-layer edge types", "the ordered ingest", "the host-array forward", "Project",
                         "fixed-point emulation", "aggregate-first order"):
        assert out_of_scope in text, out_of_scope
    # every other header keeps its prototypes
    counts = {h: len(prototypes(ROOT / "include" / h)) for h in ("gnnb_order.h", "gnnb_edge.h", "gnnb_pna_edge.h", "gnnb_gat.h", "gnnb_gat_edge.h",
                                                                 "gnnb_transformer.h", "gnnb_transformer_edge.h", "gnnb_resgated.h",
                                                                 "gnnb_resgated_edge.h", "gnnb_gatconv.h", "gnnb_gatconv_edge.h", "gnnb_ggnn.h")}
    assert counts == {"gnnb_order.h": 4, "gnnb_edge.h": 10, "gnnb_pna_edge.h": 3, "gnnb_gat.h": 4, "gnnb_gat_edge.h": 3, "gnnb_transformer.h": 4,
                      "gnnb_transformer_edge.h": 3, "gnnb_resgated.h": 4, "gnnb_resgated_edge.h": 3, "gnnb_gatconv.h": 4,
                      "gnnb_gatconv_edge.h": 3, "gnnb_ggnn.h": 4}
    assert len(runtime.ABI) == 45  # (gnnb_hip.h: tests/test_abi.py holds the table against the header)
    internal = (ROOT / "gnn-builder_amd" / "csrc" / "gnnb_internal.h").read_text()
    assert re.search(r"GNNB_FLAG_EDGE_TYPE = 256;", internal)


def test_library_exports_and_binds_the_extension():
    if not runtime.LIB_PATH.exists():
        runtime.build_library()  # hipcc cross-compiles gfx950 without a GPU
    out = subprocess.run(["nm", "-D", "--defined-only", str(runtime.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\sT\s+(gnnb_[a-z0-9_]+)", out))
    assert not [f for f in runtime.ABI_RGCN if f not in exported]
    lib = runtime.load_library(require_gpu=False)
    assert lib.gnnb_version() == 104
    for name, (restype, argtypes) in runtime.ABI_RGCN.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    # the NULL queries
    assert lib.gnnb_model_rgcn_relations(None) == 0 and lib.gnnb_model_ggnn_steps(None) == 0 and lib.gnnb_model_edge_dim(None) == 0
    # host arithmetic: int32 per edge, whole 256-byte pieces, at least one
    assert runtime.type_ingest_bytes(0) == 256 and runtime.type_ingest_bytes(64) == 256 and runtime.type_ingest_bytes(65) == 512
    assert runtime.type_ingest_bytes(-1) == 0


def test_model_descriptions_are_checked_on_the_host():
    """``gnnb_rgcn_model_num_params``: 3 tensors per layer + the head's; ``relations`` outside 1 .. 8, a non-GIN description,
    ``fpx_w != 0``, a layer output width above 256 and a description ``gnnb_model_num_params`` refuses are refused with a message;
    ``gnnb_rgcn_model_create`` makes the same checks and counts the parameters before it looks for a device (no GPU needed)."""
    from helpers import make_model
    from rgcn_util import make_rgcn_model
    lib = runtime.load_library(require_gpu=False)
    num = lib.gnnb_rgcn_model_num_params
    for layers in (1, 2, 3):
        for mlp_layers in (1, 2):
            for relations in (1, 4, 8):
                dd = runtime.make_desc(make_rgcn_model(hidden=32, layers=layers, mlp_layers=mlp_layers, relations=relations).spec())
                assert num(C.byref(dd), relations) == 3 * layers + 2 * (mlp_layers + 1)
    d = runtime.make_desc(make_rgcn_model(hidden=32, layers=3, relations=2).spec())
    assert d.conv_type == runtime.CONV["gin"]  # a GIN description: the relations travel beside it
    assert lib.gnnb_model_num_params(C.byref(d)) == 3 * 4 + 2 * 3 and num(C.byref(d), 2) == 3 * 3 + 2 * 3
    for relations in (0, -1, 9):
        assert num(C.byref(d), relations) == -1 and b"relations" in lib.gnnb_last_error()
    wide = runtime.make_desc(make_rgcn_model(hidden=32, out_dim=264, layers=2).spec())
    assert num(C.byref(wide), 1) == -1 and b"256" in lib.gnnb_last_error()
    wide.out_dim = 256
    assert num(C.byref(wide), 1) == 2 * 3 + 2 * 3
    wide.hidden_dim = 257
    assert num(C.byref(wide), 1) == -1
    narrowing = runtime.make_desc(make_rgcn_model(in_dim=40, hidden=32, layers=2, out_dim=8).spec())  # (a layer may narrow its input)
    assert num(C.byref(narrowing), 3) == 2 * 3 + 2 * 3
    for conv in ("gcn", "sage", "pna"):
        g = runtime.make_desc(make_model(conv, hidden=16).spec())
        assert num(C.byref(g), 1) == -1 and b"GIN" in lib.gnnb_last_error()
    broken = runtime.make_desc(make_rgcn_model(hidden=32, layers=3).spec())
    broken.num_pools = 0
    assert lib.gnnb_model_num_params(C.byref(broken)) == -1 and num(C.byref(broken), 1) == -1
    # create: the same checks and the parameter count -- all in front of the device
    n = 3 * 3 + 2 * 3
    arr = (C.c_void_p * n)()
    handle = C.c_void_p()
    create = lib.gnnb_rgcn_model_create
    for conv in ("gcn", "sage", "pna"):
        g = runtime.make_desc(make_model(conv, hidden=16).spec())
        assert create(C.byref(g), 1, arr, n, C.byref(handle)) == -1 and not handle and b"GIN" in lib.gnnb_last_error()
    assert create(C.byref(broken), 1, arr, n, C.byref(handle)) == -1 and not handle
    for relations in (0, 9):
        assert create(C.byref(d), relations, arr, n, C.byref(handle)) == -1 and not handle and b"relations" in lib.gnnb_last_error()
    assert create(C.byref(d), 2, arr, n - 1, C.byref(handle)) == -1 and b"expected 15" in lib.gnnb_last_error()
    assert create(C.byref(d), 2, arr, 3 * 4 + 2 * 3, C.byref(handle)) == -1 and b"expected 15" in lib.gnnb_last_error()  # (a GIN model's count)
    assert create(C.byref(d), 2, arr, n, C.byref(handle)) == -1 and not handle and b"parameter 0 is NULL" in lib.gnnb_last_error()
    assert create(C.byref(d), 2, arr, n, None) == -1 and b"out_model" in lib.gnnb_last_error()
    d.fpx_w, d.fpx_i = 16, 8
    assert num(C.byref(d), 2) == -1 and b"fixed-point" in lib.gnnb_last_error()
    assert create(C.byref(d), 2, arr, n, C.byref(handle)) == -1 and not handle and b"fixed-point" in lib.gnnb_last_error()


def test_the_entries_refuse_on_the_host():
    """Without a model, a workspace or a prepared batch: GNNB_ERR_INVALID, nothing launched (no GPU needed)."""
    lib = runtime.load_library(require_gpu=False)
    assert lib.gnnb_rgcn_slots(None, None, 4, None, None) == -1 and b"prepared" in lib.gnnb_last_error()
    assert lib.gnnb_aggregate_rgcn(None, None, None, 96, 3, None, 0, None, 4, None, 32, None) == -1 and b"prepared" in lib.gnnb_last_error()
    assert lib.gnnb_forward_batched_types(None, None, None, None, None, None, None, 0, 0, 0, None, None) == -1
    assert b"gnnb_forward_batched_types" in lib.gnnb_last_error()
    assert lib.gnnb_forward_prepared_types(None, None, None, None, None, None) == -1 and b"gnnb_forward_prepared_types" in lib.gnnb_last_error()
    assert lib.gnnb_forward_pyg_types(None, None, None, None, None, None, None, 0, 0, 0, None, None) == -1
    assert b"gnnb_forward_pyg_types" in lib.gnnb_last_error()
    assert lib.gnnb_workspace_enable_type_ingest(None) == -1 and b"null workspace" in lib.gnnb_last_error()
    out = (C.c_void_p * 4)()
    assert lib.gnnb_ingest_pyg_types(None, None, None, None, None, 0, 0, 0, out, out, out, out, None) == -1
    assert b"gnnb_ingest_pyg_types" in lib.gnnb_last_error()
