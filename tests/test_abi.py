"""The C-ABI library loads on a CPU-only machine and exports every symbol include/gnnb_hip.h
declares; the product path refuses to run without a GPU (no fallback).  No compute calls here."""
import re
import subprocess
from pathlib import Path

import pytest
import torch

from gnnbuilder_amd import runtime

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lib_path():
    if not runtime.LIB_PATH.exists():
        runtime.build_library()  # hipcc cross-compiles gfx950 without a GPU
    return runtime.LIB_PATH


def header_functions():
    text = (ROOT / "include" / "gnnb_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gnnb_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_what_runtime_binds():
    assert sorted(runtime.EXPORTED_SYMBOLS) == header_functions()


def header_text(path=ROOT / "include" / "gnnb_hip.h"):
    text = re.sub(r"/\*.*?\*/", "", path.read_text(), flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def ctype_ok(c_type, ct, is_return=False):
    """One C type of a prototype against the binding's ctypes type: any pointer -> c_void_p / c_char_p / POINTER(...),
    int -> c_int, float -> c_float, size_t -> c_size_t, a void return -> None."""
    import ctypes as C
    c_type = " ".join(c_type.replace("const", " ").split())
    if "*" in c_type:
        return ct in (C.c_void_p, C.c_char_p) or (isinstance(ct, type) and issubclass(ct, C._Pointer))
    if c_type == "void":
        return is_return and ct is None
    return ct is {"int": C.c_int, "float": C.c_float, "size_t": C.c_size_t}[c_type]


def test_binding_signatures_match_the_header():
    """Every prototype of the header against runtime.ABI: a function left without argtypes, or bound with an int where the
    header has a pointer or a size_t, passes a truncated value from 2 GiB up.  Needs no library."""
    protos = re.findall(r"^([A-Za-z_][\w \*]*?)\b(gnnb_\w+)\s*\(([^)]*)\)\s*;", header_text(), flags=re.M)
    assert len(protos) == 45 and [name for _, name, _ in protos] == list(runtime.ABI)  # all of them, in the header's order
    for ret, name, args in protos:
        restype, argtypes = runtime.ABI[name]
        assert ctype_ok(ret, restype, is_return=True), (name, ret, restype)
        params = [] if args.strip() == "void" else [a.strip() for a in args.split(",")]
        assert len(params) == len(argtypes), (name, params, argtypes)
        for p, ct in zip(params, argtypes):
            c_type = re.sub(r"\w+$", "", p)  # (the parameter's name goes; `*` stays with the type)
            assert ctype_ok(c_type, ct), (name, p, ct)


def test_constants_match_the_headers():
    """The values runtime.py restates, against the enums of include/gnnb_hip.h and the constants of csrc/gnnb_internal.h:
    every member has a Python entry with the header's value."""
    values = {name: int(v) for name, v in re.findall(r"\b(GNNB_[A-Z0-9_]+)\s*=\s*(-?\d+)", header_text())}
    # (a member written without `= <int>` would not be in `values`: every member named in an enum body must be)
    members = [m for body in re.findall(r"\benum\b[^{;]*\{([^}]*)\}", header_text())
               for m in re.findall(r"\bGNNB_(?:CONV|ACT|POOL|OUT|AGG|PATH)_\w+", body)]
    assert members and not [m for m in members if m not in values], members
    tables = {"GNNB_CONV_": runtime.CONV, "GNNB_ACT_": runtime.ACT, "GNNB_POOL_": runtime.POOL, "GNNB_OUT_": runtime.OUT_ACT,
              "GNNB_AGG_": runtime.AGG}
    seen = {prefix: 0 for prefix in list(tables) + ["GNNB_PATH_"]}
    for name, v in values.items():
        for prefix, table in tables.items():
            if name.startswith(prefix):
                assert table[name[len(prefix):].lower()] == v, name
                seen[prefix] += 1
        if name == "GNNB_PATH_LARGE_LAYERWISE":
            assert runtime.PATH_LARGE_LAYERWISE == v == 16
        elif name.startswith("GNNB_PATH_"):
            assert runtime.PATH_NAMES[v] == name[len("GNNB_PATH_"):].lower(), name
            assert v < runtime.PATH_LARGE_LAYERWISE  # (last_path masks the flag off)
            seen["GNNB_PATH_"] += 1
    # nothing was skipped because a pattern stopped matching, and the Python tables name no value the header lacks
    assert len(members) == sum(seen.values()) + 1  # (+ GNNB_PATH_LARGE_LAYERWISE)
    assert seen == {"GNNB_CONV_": 4, "GNNB_ACT_": 5, "GNNB_POOL_": 3, "GNNB_OUT_": 3, "GNNB_AGG_": 7, "GNNB_PATH_": 4}
    for prefix, table in tables.items():
        assert sorted(set(table.values())) == sorted(v for n, v in values.items() if n.startswith(prefix)), prefix
    assert len(runtime.PATH_NAMES) == seen["GNNB_PATH_"]
    assert runtime.OUT_ACT[None] == values["GNNB_OUT_NONE"]
    assert runtime.GNNB_OK == values["GNNB_OK"] == 0 and runtime.GNNB_ERR_RANGE == values["GNNB_ERR_RANGE"]
    internal = header_text(ROOT / "gnn-builder_amd" / "csrc" / "gnnb_internal.h")
    for name in ("INGEST_TILE", "INGEST_DIGIT_BITS"):
        (v,) = re.findall(rf"\bconstexpr int {name}\s*=\s*(\d+)\s*;", internal)
        assert getattr(runtime, name) == int(v), name


def test_library_exports_every_declared_symbol(lib_path):
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib_path)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\sT\s+(gnnb_[a-z0-9_]+)", out))
    missing = [f for f in header_functions() if f not in exported]
    assert not missing, f"libgnnb_hip.so lacks {missing}"


def test_library_has_gfx950_code_object(lib_path):
    blob = lib_path.read_bytes()
    assert b"gfx950" in blob and b"k_aggregate" in blob and b"k_linear" in blob


def test_library_loads_and_reports_version(lib_path):
    lib = runtime.load_library(require_gpu=False)
    assert lib.gnnb_version() == 104
    for sym in runtime.EXPORTED_SYMBOLS:
        assert hasattr(lib, sym)


def test_struct_layout_matches_header():
    # 19 int32/float fields (version 103: + math) + pools[3] = 21 * 4 bytes, in the header's order
    import ctypes
    import re
    assert ctypes.sizeof(runtime.ModelDesc) == 21 * 4
    hdr = (ROOT / "include" / "gnnb_hip.h").read_text()
    body = hdr[hdr.index("typedef struct gnnb_model_desc {"):hdr.index("} gnnb_model_desc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(?:int32_t|float)\s+(\w+)(?:\[\d+\])?;", body)
    assert names == [f[0] for f in runtime.ModelDesc._fields_]
    assert ctypes.sizeof(runtime.GemmSeg) == 24


@pytest.mark.skipif(torch.cuda.is_available(), reason="needs a machine WITHOUT a GPU")
def test_product_path_fails_loudly_without_gpu(lib_path):
    with pytest.raises(runtime.GnnbUnavailable):
        runtime.load_library(require_gpu=True)
    from helpers import make_model
    with pytest.raises(runtime.GnnbUnavailable):
        runtime.CompiledModel.from_model(make_model("gcn", hidden=16), 4, 64, 128)


def test_invalid_description_is_rejected_on_host(lib_path):
    import ctypes as C
    lib = runtime.load_library(require_gpu=False)
    from helpers import make_model
    d = runtime.make_desc(make_model("gcn", hidden=16).spec())
    assert lib.gnnb_model_num_params(C.byref(d)) == 2 * 2 + 2 * 3
    d.conv_type = 9
    assert lib.gnnb_model_num_params(C.byref(d)) < 0
    assert b"conv_type" in lib.gnnb_last_error()
