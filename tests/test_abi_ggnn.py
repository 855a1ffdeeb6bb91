"""The extension header include/gnnb_ggnn.h (GatedGraphConv models: their creation and the fused GRU aggregate as a stage entry)
against ``runtime.ABI_GGNN``, the way tests/test_abi_resgated.py holds include/gnnb_resgated.h against ``runtime.ABI_RESGATED``:
every prototype, in the header's order, with matching ctypes types; the library exports each one; the refusals that need no
GPU.  No GPU, no compute calls."""
import ctypes as C
import re
import subprocess
from pathlib import Path

from gnnbuilder_amd import runtime
from test_abi import ctype_ok
from test_abi_gat import prototypes

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "gnnb_ggnn.h"
OTHER_TABLES = ("ABI", "ABI_ORDER", "ABI_EDGE", "ABI_PNA_EDGE", "ABI_GAT", "ABI_GAT_EDGE", "ABI_TRANSFORMER", "ABI_TRANSFORMER_EDGE",
                "ABI_RESGATED", "ABI_RESGATED_EDGE", "ABI_GATCONV", "ABI_GATCONV_EDGE")


def test_binding_signatures_match_the_extension_header():
    protos = prototypes(HEADER)
    assert len(protos) == 4 and [name for _, name, _ in protos] == list(runtime.ABI_GGNN)  # all of them, in the header's order
    for table in OTHER_TABLES:
        assert not set(runtime.ABI_GGNN) & set(getattr(runtime, table)), table
    for ret, name, args in protos:
        restype, argtypes = runtime.ABI_GGNN[name]
        assert ctype_ok(ret, restype, is_return=True), (name, ret, restype)
        params = [a.strip() for a in args.split(",")]
        assert len(params) == len(argtypes), (name, params, argtypes)
        for p, ct in zip(params, argtypes):
            assert ctype_ok(re.sub(r"\w+$", "", p), ct), (name, p, ct)


def test_extension_header_builds_on_the_main_header():
    text = HEADER.read_text()
    assert '#include "gnnb_hip.h"' in text and "#define GNNB_VERSION" not in text  # (the version is gnnb_hip.h's: 104)
    assert 'extern "C"' in text
    assert text.count("_GatedGraphConv") >= 1 and text.count("models.py") >= 2
    assert "Summation order" in text and "GNNB_CONV_GIN" in text and "takes NO bias" in text and "saturate exactly" in text
    for out_of_scope in ("aggr other than add", "bias = False", "edge_weight", "edge features", "above 256", "steps above 8",
                         "fused into the GEMM's epilogue"):
        assert out_of_scope in text
    # the other extension headers keep their prototypes
    counts = {h: len(prototypes(ROOT / "include" / h)) for h in ("gnnb_edge.h", "gnnb_pna_edge.h", "gnnb_gat.h", "gnnb_gat_edge.h",
                                                                 "gnnb_transformer.h", "gnnb_transformer_edge.h", "gnnb_resgated.h",
                                                                 "gnnb_resgated_edge.h", "gnnb_gatconv.h", "gnnb_gatconv_edge.h")}
    assert counts == {"gnnb_edge.h": 10, "gnnb_pna_edge.h": 3, "gnnb_gat.h": 4, "gnnb_gat_edge.h": 3, "gnnb_transformer.h": 4,
                      "gnnb_transformer_edge.h": 3, "gnnb_resgated.h": 4, "gnnb_resgated_edge.h": 3, "gnnb_gatconv.h": 4,
                      "gnnb_gatconv_edge.h": 3}


def test_library_exports_and_binds_the_extension():
    if not runtime.LIB_PATH.exists():
        runtime.build_library()  # hipcc cross-compiles gfx950 without a GPU
    out = subprocess.run(["nm", "-D", "--defined-only", str(runtime.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\sT\s+(gnnb_[a-z0-9_]+)", out))
    assert not [f for f in runtime.ABI_GGNN if f not in exported]
    lib = runtime.load_library(require_gpu=False)
    assert lib.gnnb_version() == 104
    for name, (restype, argtypes) in runtime.ABI_GGNN.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    # the NULL queries
    assert lib.gnnb_model_ggnn_steps(None) == 0 and lib.gnnb_model_is_resgated(None) == 0 and lib.gnnb_model_transformer_heads(None) == 0
    assert lib.gnnb_model_gat_heads(None) == 0 and lib.gnnb_model_gatconv_heads(None) == 0 and lib.gnnb_model_edge_dim(None) == 0


def test_model_descriptions_are_checked_on_the_host():
    """``gnnb_ggnn_model_num_params``: 5 tensors per layer + the head's; ``steps`` outside 1 .. 8, a layer that would narrow its
    input, a non-GIN description, ``fpx_w != 0``, a layer output width above 256 and a description ``gnnb_model_num_params``
    refuses are refused with a message; ``gnnb_ggnn_model_create`` makes the same checks and counts the parameters before it looks
    for a device (no GPU needed)."""
    from ggnn_util import make_ggnn_model
    from helpers import make_model
    lib = runtime.load_library(require_gpu=False)
    num = lib.gnnb_ggnn_model_num_params
    for layers in (1, 2, 3):
        for mlp_layers in (1, 2):
            for steps in (1, 3, 8):
                dd = runtime.make_desc(make_ggnn_model(hidden=32, layers=layers, mlp_layers=mlp_layers, steps=steps).spec())
                assert num(C.byref(dd), steps) == 5 * layers + 2 * (mlp_layers + 1)
    d = runtime.make_desc(make_ggnn_model(hidden=32, layers=3, steps=2).spec())
    assert d.conv_type == runtime.CONV["gin"]  # a GIN description: the steps travel beside it
    assert lib.gnnb_model_num_params(C.byref(d)) == 3 * 4 + 2 * 3 and num(C.byref(d), 2) == 3 * 5 + 2 * 3
    for steps in (0, -1, 9):
        assert num(C.byref(d), steps) == -1 and b"steps" in lib.gnnb_last_error()
    wide = runtime.make_desc(make_ggnn_model(hidden=32, out_dim=264, layers=2).spec())
    assert num(C.byref(wide), 1) == -1 and b"256" in lib.gnnb_last_error()
    wide.out_dim = 256
    assert num(C.byref(wide), 1) == 2 * 5 + 2 * 3
    wide.hidden_dim = 257  # (a hidden layer's output width: above the cap, and above the last layer's)
    assert num(C.byref(wide), 1) == -1
    narrow = runtime.make_desc(make_ggnn_model(in_dim=9, hidden=32, layers=2).spec())
    narrow.in_dim = 33  # in > hidden
    assert num(C.byref(narrow), 1) == -1 and b"exceeds its output width" in lib.gnnb_last_error()
    narrow.in_dim, narrow.out_dim = 9, 31  # hidden > out
    assert num(C.byref(narrow), 1) == -1 and b"exceeds its output width" in lib.gnnb_last_error()
    one = runtime.make_desc(make_ggnn_model(in_dim=9, hidden=4, layers=1, out_dim=16).spec())  # (one layer: hidden is no layer's width)
    assert num(C.byref(one), 1) == 5 + 2 * 3
    one.in_dim = 17
    assert num(C.byref(one), 1) == -1 and b"exceeds its output width" in lib.gnnb_last_error()
    for conv in ("gcn", "sage", "pna"):
        g = runtime.make_desc(make_model(conv, hidden=16).spec())
        assert num(C.byref(g), 1) == -1 and b"GIN" in lib.gnnb_last_error()
    broken = runtime.make_desc(make_ggnn_model(hidden=32, layers=3).spec())
    broken.num_pools = 0
    assert lib.gnnb_model_num_params(C.byref(broken)) == -1 and num(C.byref(broken), 1) == -1
    # create: the same checks and the parameter count -- all in front of the device
    n = 3 * 5 + 2 * 3
    arr = (C.c_void_p * n)()
    handle = C.c_void_p()
    create = lib.gnnb_ggnn_model_create
    for conv in ("gcn", "sage", "pna"):
        g = runtime.make_desc(make_model(conv, hidden=16).spec())
        assert create(C.byref(g), 1, arr, n, C.byref(handle)) == -1 and not handle and b"GIN" in lib.gnnb_last_error()
    assert create(C.byref(broken), 1, arr, n, C.byref(handle)) == -1 and not handle
    for steps in (0, 9):
        assert create(C.byref(d), steps, arr, n, C.byref(handle)) == -1 and not handle and b"steps" in lib.gnnb_last_error()
    assert create(C.byref(d), 2, arr, n - 1, C.byref(handle)) == -1 and b"expected 21" in lib.gnnb_last_error()
    assert create(C.byref(d), 2, arr, 3 * 4 + 2 * 3, C.byref(handle)) == -1 and b"expected 21" in lib.gnnb_last_error()  # (a GIN model's count)
    assert create(C.byref(d), 2, arr, n, C.byref(handle)) == -1 and not handle and b"parameter 0 is NULL" in lib.gnnb_last_error()
    assert create(C.byref(d), 2, arr, n, None) == -1 and b"out_model" in lib.gnnb_last_error()
    assert create(C.byref(narrow), 1, arr, 2 * 5 + 2 * 3, C.byref(handle)) == -1 and b"exceeds its output width" in lib.gnnb_last_error()
    d.fpx_w, d.fpx_i = 16, 8
    assert num(C.byref(d), 2) == -1 and b"fixed-point" in lib.gnnb_last_error()
    assert create(C.byref(d), 2, arr, n, C.byref(handle)) == -1 and not handle and b"fixed-point" in lib.gnnb_last_error()


def test_the_stage_entry_refuses_on_the_host():
    """``gnnb_aggregate_ggnn`` without a prepared workspace: GNNB_ERR_INVALID, nothing launched (no GPU needed)."""
    lib = runtime.load_library(require_gpu=False)
    assert lib.gnnb_aggregate_ggnn(None, None, 96, None, 96, None, 32, 32, None, None, 4, None, 32, None) == -1
    assert b"prepared" in lib.gnnb_last_error()
