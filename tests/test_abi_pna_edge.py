"""The extension header include/gnnb_pna_edge.h (PNA models with edge features: their creation and the fused edge aggregate as a
stage entry) against ``runtime.ABI_PNA_EDGE``, the way tests/test_abi_edge.py holds include/gnnb_edge.h against
``runtime.ABI_EDGE``: every prototype, in the header's order, with matching ctypes types; the library exports each one.  No GPU,
no compute calls."""
import re
import subprocess
from pathlib import Path

from gnnbuilder_amd import runtime
from test_abi import ctype_ok, header_text

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "gnnb_pna_edge.h"


def prototypes():
    return re.findall(r"^([A-Za-z_][\w \*]*?)\b(gnnb_\w+)\s*\(([^)]*)\)\s*;", header_text(HEADER), flags=re.M)


def test_binding_signatures_match_the_extension_header():
    protos = prototypes()
    assert len(protos) == 3 and [name for _, name, _ in protos] == list(runtime.ABI_PNA_EDGE)  # all of them, in the header's order
    assert not set(runtime.ABI_PNA_EDGE) & (set(runtime.ABI) | set(runtime.ABI_ORDER) | set(runtime.ABI_EDGE))
    for ret, name, args in protos:
        restype, argtypes = runtime.ABI_PNA_EDGE[name]
        assert ctype_ok(ret, restype, is_return=True), (name, ret, restype)
        params = [a.strip() for a in args.split(",")]
        assert len(params) == len(argtypes), (name, params, argtypes)
        for p, ct in zip(params, argtypes):
            assert ctype_ok(re.sub(r"\w+$", "", p), ct), (name, p, ct)


def test_extension_header_builds_on_the_main_header():
    text = HEADER.read_text()
    assert '#include "gnnb_hip.h"' in text and "#define GNNB_VERSION" not in text  # (the version is gnnb_hip.h's: 104)
    assert 'extern "C"' in text
    # every entry says which reference or models.py lines it replaces, as the other headers do
    assert len(re.findall(r"(model\.cpp\.jinja|gnn_builder_lib\.h|models\.py):\d+", text)) >= 3
    assert text.count("_PNAEConv") >= 3 and text.count("models.py") >= 4
    # gnnb_edge.h keeps its ten prototypes
    edge = re.findall(r"^[A-Za-z_][\w \*]*?\bgnnb_\w+\s*\([^)]*\)\s*;", header_text(ROOT / "include" / "gnnb_edge.h"), flags=re.M)
    assert len(edge) == 10


def test_library_exports_and_binds_the_extension():
    if not runtime.LIB_PATH.exists():
        runtime.build_library()  # hipcc cross-compiles gfx950 without a GPU
    out = subprocess.run(["nm", "-D", "--defined-only", str(runtime.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\sT\s+(gnnb_[a-z0-9_]+)", out))
    assert not [f for f in runtime.ABI_PNA_EDGE if f not in exported]
    lib = runtime.load_library(require_gpu=False)
    assert lib.gnnb_version() == 104
    for name, (restype, argtypes) in runtime.ABI_PNA_EDGE.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes


def test_pna_edge_model_descriptions_are_checked_on_the_host():
    """``gnnb_pna_edge_model_num_params``: 8 tensors per layer + the head's; edge_dim outside 1 .. 16, a conv type other than PNA
    and the fixed-point emulation are refused (no GPU needed).  ``gnnb_edge_model_num_params`` still refuses a PNA description."""
    import ctypes as C
    from helpers import make_model
    from pnae_util import make_pnae_model
    lib = runtime.load_library(require_gpu=False)
    d = runtime.make_desc(make_pnae_model(hidden=16, layers=3).spec())
    assert d.conv_type == runtime.CONV["pna"]
    assert lib.gnnb_model_num_params(C.byref(d)) == 3 * 6 + 2 * 3
    assert lib.gnnb_pna_edge_model_num_params(C.byref(d), 3) == 3 * 8 + 2 * 3
    for bad in (0, -1, 17):
        assert lib.gnnb_pna_edge_model_num_params(C.byref(d), bad) == -1 and b"edge" in lib.gnnb_last_error()
    assert lib.gnnb_edge_model_num_params(C.byref(d), 3) == -1 and b"GIN" in lib.gnnb_last_error()
    d.fpx_w, d.fpx_i = 16, 8
    assert lib.gnnb_pna_edge_model_num_params(C.byref(d), 3) == -1 and b"fixed-point" in lib.gnnb_last_error()
    for conv in ("gin", "gcn", "sage"):
        g = runtime.make_desc(make_model(conv, hidden=16).spec())
        assert lib.gnnb_pna_edge_model_num_params(C.byref(g), 3) == -1 and b"PNA" in lib.gnnb_last_error()
