"""The extension header include/gnnb_order.h (the ordered ingest's entry points) against ``runtime.ABI_ORDER``, the way
tests/test_abi.py holds include/gnnb_hip.h against ``runtime.ABI``: every prototype, in the header's order, with matching
ctypes types; the library exports each one.  No GPU, no compute calls."""
import re
import subprocess
from pathlib import Path

from gnnbuilder_amd import runtime
from test_abi import ctype_ok, header_text

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "gnnb_order.h"


def prototypes():
    return re.findall(r"^([A-Za-z_][\w \*]*?)\b(gnnb_\w+)\s*\(([^)]*)\)\s*;", header_text(HEADER), flags=re.M)


def test_binding_signatures_match_the_extension_header():
    protos = prototypes()
    assert len(protos) == 4 and [name for _, name, _ in protos] == list(runtime.ABI_ORDER)  # all of them, in the header's order
    assert not set(runtime.ABI_ORDER) & set(runtime.ABI)
    for ret, name, args in protos:
        restype, argtypes = runtime.ABI_ORDER[name]
        assert ctype_ok(ret, restype, is_return=True), (name, ret, restype)
        params = [a.strip() for a in args.split(",")]
        assert len(params) == len(argtypes), (name, params, argtypes)
        for p, ct in zip(params, argtypes):
            assert ctype_ok(re.sub(r"\w+$", "", p), ct), (name, p, ct)


def test_extension_header_builds_on_the_main_header():
    text = HEADER.read_text()
    assert '#include "gnnb_hip.h"' in text and "#define GNNB_VERSION" not in text  # (the version is gnnb_hip.h's: 104)
    assert 'extern "C"' in text


def test_library_exports_and_binds_the_extension():
    if not runtime.LIB_PATH.exists():
        runtime.build_library()  # hipcc cross-compiles gfx950 without a GPU
    out = subprocess.run(["nm", "-D", "--defined-only", str(runtime.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\sT\s+(gnnb_[a-z0-9_]+)", out))
    assert not [f for f in runtime.ABI_ORDER if f not in exported]
    lib = runtime.load_library(require_gpu=False)
    assert lib.gnnb_version() == 104
    for name, (restype, argtypes) in runtime.ABI_ORDER.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
