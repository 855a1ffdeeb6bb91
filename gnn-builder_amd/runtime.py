"""Python binding of the C ABI in ``include/gnnb_hip.h`` and its extensions ``include/gnnb_order.h`` and ``include/gnnb_edge.h``
(``libgnnb_hip.so``).

This is the accelerated product path.  It has NO fallback: if the HIP library is not built, or no
MI355X is visible, every entry point raises ``GnnbUnavailable`` -- it never routes to PyTorch or
to the CPU oracle.

PyTorch is used here only as plumbing: device tensors give us HBM allocations and the current
HIP stream; the kernels themselves are the hand-written ones in ``csrc/``.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path
from typing import Optional, Sequence

import numpy as np

PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("GNNB_HIP_LIB", PKG_DIR / "libgnnb_hip.so"))  # override: diagnostic builds only
CSRC_DIR = PKG_DIR / "csrc"

# ---------------------------------------------------------------------- values restated from the C headers
# (tests/test_abi.py reads include/gnnb_hip.h and csrc/gnnb_internal.h and compares every one of them)
GNNB_OK = 0                                                                      # gnnb_status
GNNB_ERR_RANGE = -6                                                              # gnnb_status
CONV = {"gcn": 0, "gin": 1, "sage": 2, "pna": 3}                                 # gnnb_conv
MAX_EDGE_DIM = 16  # of a GINE model (include/gnnb_edge.h): its description is GIN's, edge_dim travels beside it; likewise PNA with edge features (gnnb_pna_edge.h)
_EDGE_BASE = {"gine": "gin", "pnae": "pna"}  # spec["conv"] of an edge model -> the conv its description carries
MAX_GAT_HEADS, MAX_GAT_WIDTH = 8, 256  # of a GATv2 model (include/gnnb_gat.h): its description is GCN's, heads and negative_slope travel beside it
_DESC_BASE = {**_EDGE_BASE, "gatv2": "gcn", "gatv2e": "gcn", "transformer": "gin", "transformere": "gin", "resgated": "gin", "resgatede": "gin", "gat": "gcn", "gate": "gcn", "ggnn": "gin", "rgcn": "gin"}  # spec["conv"] -> the conv its description carries, where that is another
# spec["conv"] of the models with edge_dim beside the description ("gatv2e": include/gnnb_gat_edge.h, "transformere": gnnb_transformer_edge.h,
# "resgatede": gnnb_resgated_edge.h, "gate": gnnb_gatconv_edge.h)
_EDGE_CONVS = (*_EDGE_BASE, "gatv2e", "transformere", "resgatede", "gate")
_GAT_CONVS = ("gatv2", "gatv2e")       # ... and of those with heads and negative_slope beside it
# a GAT v1 model (include/gnnb_gatconv.h, spec["conv"] == "gat"): a GCN description, heads and negative_slope beside it, within GATv2's
# limits -- a model kind of its own; with edge features ("gate", include/gnnb_gatconv_edge.h) edge_dim too
_GATCONV_CONVS = ("gat", "gate")
# a TransformerConv model (include/gnnb_transformer.h, spec["conv"] == "transformer"): its description is GIN's -- the tables keep
# explicit (v, v) edges --, heads travels beside it; with edge features ("transformere", include/gnnb_transformer_edge.h) edge_dim too
_TRANSFORMER_CONVS = ("transformer", "transformere")
MAX_TRANSFORMER_HEADS, MAX_TRANSFORMER_WIDTH = 8, 256
# a ResGatedGraphConv model (include/gnnb_resgated.h, spec["conv"] == "resgated"): its description is GIN's too, a "gated" mark beside it
# ... with edge features ("resgatede", include/gnnb_resgated_edge.h): edge_dim beside it too
MAX_RESGATED_WIDTH = 256
# a GatedGraphConv model (include/gnnb_ggnn.h, spec["conv"] == "ggnn"): its description is GIN's too, steps per layer beside it
MAX_GGNN_STEPS, MAX_GGNN_WIDTH = 8, 256
# an RGCNConv model (include/gnnb_rgcn.h, spec["conv"] == "rgcn"): its description is GIN's too, the relation count beside it
MAX_RGCN_RELATIONS, MAX_RGCN_WIDTH = 8, 256
ACT = {"relu": 0, "gelu": 1, "sigmoid": 2, "tanh": 3, "none": 4}                 # gnnb_act
POOL = {"add": 0, "mean": 1, "max": 2}                                           # gnnb_pool
OUT_ACT = {None: 0, "none": 0, "softmax": 1, "log_softmax": 2}                   # gnnb_out_act
AGG = {"gcn": 0, "sum": 1, "mean": 2, "pna": 3, "lg": 4, "simple": 5, "copy": 6}  # gnnb_agg
MATH_MODES = {"fp32": 0, "bf16x6": 1, "bf16x3": 2, "f16x3": 3}                   # gnnb_model_desc::math (no enum: its comment)
PATH_NAMES = {0: "none", 1: "layerwise", 2: "stack", 3: "stack_zf"}              # GNNB_PATH_* (the anonymous enum), low bits
PATH_LARGE_LAYERWISE = 16                                                        # GNNB_PATH_LARGE_LAYERWISE: a flag or-ed to them
# k_ingest.hip (gnnb_internal.h INGEST_TILE / INGEST_DIGIT_BITS): edges per workgroup and bits of the graph id per radix pass
INGEST_TILE = 1024
INGEST_DIGIT_BITS = 8


class GnnbError(RuntimeError):
    pass


class GnnbUnavailable(GnnbError):
    """The HIP extension or the GPU is missing: the product path cannot run (no fallback)."""


class GnnbRangeError(GnnbError):
    """A reduced-precision math mode (bf16x3 / f16x3) produced a non-finite value (``GNNB_ERR_RANGE``): fp16's range was
    exceeded by an activation or a weight.  The flagged forward's results are unspecified; run the model with math="fp32"."""


class ModelDesc(C.Structure):
    # field-for-field gnnb_model_desc (include/gnnb_hip.h)
    _fields_ = [
        ("conv_type", C.c_int32),
        ("num_layers", C.c_int32),
        ("in_dim", C.c_int32),
        ("hidden_dim", C.c_int32),
        ("out_dim", C.c_int32),
        ("activation", C.c_int32),
        ("skip", C.c_int32),
        ("num_pools", C.c_int32),
        ("pools", C.c_int32 * 3),
        ("mlp_num_linear", C.c_int32),
        ("mlp_hidden", C.c_int32),
        ("mlp_out", C.c_int32),
        ("mlp_activation", C.c_int32),
        ("gin_eps", C.c_float),
        ("pna_delta", C.c_float),
        ("output_activation", C.c_int32),
        ("fpx_w", C.c_int32),
        ("fpx_i", C.c_int32),
        ("math", C.c_int32),
    ]


class GemmSeg(C.Structure):
    _fields_ = [("a_dev", C.c_void_p), ("rowscale_dev", C.c_void_p), ("lda", C.c_int32), ("k", C.c_int32)]


# ---------------------------------------------------------------------- the C ABI: every function of include/gnnb_hip.h
# name -> (restype, argtypes), in the header's order; load_library applies it, tests/test_abi.py compares it with the header's
# prototypes (no library needed).  A function left without argtypes takes a Python integer as a C int: a pointer or a size_t
# from 2 GiB up would be truncated -- so none is left without.
_P, _I, _F, _Z = C.c_void_p, C.c_int, C.c_float, C.c_size_t
_PP, _PF, _PI, _DESC = C.POINTER(C.c_void_p), C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(ModelDesc)
ABI = {
    "gnnb_version": (_I, []),
    "gnnb_last_error": (C.c_char_p, []),
    "gnnb_device_count": (_I, []),
    "gnnb_stream_sync": (_I, [_P]),
    "gnnb_model_num_params": (_I, [_DESC]),
    "gnnb_model_create": (_I, [_DESC, _PP, _I, _PP]),
    "gnnb_model_destroy": (None, [_P]),
    "gnnb_model_get_desc": (_I, [_P, _DESC]),
    "gnnb_workspace_create": (_I, [_P, _I, _I, _I, _PP]),
    "gnnb_workspace_destroy": (None, [_P]),
    "gnnb_workspace_bytes": (_Z, [_P]),
    "gnnb_workspace_set_max_graph_nodes": (_I, [_P, _I]),
    "gnnb_workspace_set_max_degree": (_I, [_P, _I]),
    "gnnb_workspace_last_path": (_I, [_P]),
    "gnnb_workspace_set_large_segment": (_I, [_P, _I, _I, _I]),
    "gnnb_forward_batched": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P]),
    "gnnb_forward_prepared": (_I, [_P, _P, _P, _P, _P]),
    "gnnb_forward_prepared_prep_next": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "gnnb_forward_batched_host": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "gnnb_workspace_check": (_I, [_P, _P]),
    "gnnb_ingest_bytes": (_Z, [_I, _I, _I]),
    "gnnb_workspace_enable_ingest": (_I, [_P]),
    "gnnb_ingest_pyg": (_I, [_P, _P, _P, _P, _I, _I, _I, _PP, _PP, _PP, _P]),
    "gnnb_forward_pyg": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P]),
    "gnnb_graph_prep": (_I, [_P, _P, _P, _P, _I, _I, _I, _F, _P]),
    "gnnb_graph_tables_to_host": (_I, [_P, _P, _P, _P, _P]),
    "gnnb_aggregate": (_I, [_P, _I, _P, _P, _P, _I, _F, _P]),
    "gnnb_pna_product_aggregate": (_I, [_P, _P, _P, _I, _P, _I, _P]),
    "gnnb_aggregate_edges": (_I, [_P, _P, _P, _P, _I, _F, _P]),
    "gnnb_edge_index_table_to_host": (_I, [_P, _P, _P]),
    "gnnb_linear": (_I, [C.POINTER(GemmSeg), _I, _P, _I, _P, _P, _P, _I, _I, _I, _P]),
    "gnnb_debug_stream_k_guard": (_I, [_P, _P]),
    "gnnb_global_pool": (_I, [_P, _P, _I, C.POINTER(C.c_int32), _I, _P, _P]),
    "gnnb_event_create": (_I, [_PP]),
    "gnnb_event_record": (_I, [_P, _P]),
    "gnnb_event_elapsed_ms": (_I, [_P, _P, _PF]),
    "gnnb_event_destroy": (None, [_P]),
    "gnnb_aggregate_timed": (_I, [_P, _I, _P, _P, _P, _I, _I, _F, _I, _P, _PF]),
    "gnnb_linear_timed": (_I, [_P, _I, _I, _P, _I, _P, _P, _I, _I, _I, _I, _P, _PF]),
    "gnnb_gcn_stack_timed": (_I, [_P, _P, _P, _I, _P, _PF]),
    "gnnb_malloc": (_I, [_PP, _Z]),
    "gnnb_free": (None, [_P]),
    "gnnb_memcpy_h2d": (_I, [_P, _P, _Z, _P]),
    "gnnb_memcpy_d2h": (_I, [_P, _P, _Z, _P]),
    "gnnb_set_option": (_I, [C.c_char_p, _I]),
}
EXPORTED_SYMBOLS = list(ABI)  # (tests check the .so exports each one)
# ... and every function of the extension header include/gnnb_order.h, in its order (tests/test_abi_order.py compares the two)
ABI_ORDER = {
    "gnnb_order_bytes": (_Z, [_I, _I, _I, _I, _I]),
    "gnnb_workspace_enable_ordered_ingest": (_I, [_P]),
    "gnnb_ingest_pyg_ordered": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _PP, _PP, _PP, _PP, _PP, _PI, _PI, _PI, _P]),
    "gnnb_forward_pyg_ordered": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P]),
}
# ... and of include/gnnb_edge.h (GINE models), in its order (tests/test_abi_edge.py)
ABI_EDGE = {
    "gnnb_edge_model_num_params": (_I, [_DESC, _I]),
    "gnnb_edge_model_create": (_I, [_DESC, _I, _PP, _I, _PP]),
    "gnnb_model_edge_dim": (_I, [_P]),
    "gnnb_forward_batched_edges": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P]),
    "gnnb_forward_prepared_edges": (_I, [_P, _P, _P, _P, _P, _P]),
    "gnnb_aggregate_edges_fused": (_I, [_P, _P, _P, _I, _P, _I, _P, _P, _I, _F, _P]),
    "gnnb_edge_ingest_bytes": (_Z, [_I, _I]),
    "gnnb_workspace_enable_edge_ingest": (_I, [_P]),
    "gnnb_ingest_pyg_edges": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _PP, _PP, _PP, _PP, _P]),
    "gnnb_forward_pyg_edges": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P]),
}


# ... and of include/gnnb_pna_edge.h (PNA models with edge features), in its order (tests/test_abi_pna_edge.py)
ABI_PNA_EDGE = {
    "gnnb_pna_edge_model_num_params": (_I, [_DESC, _I]),
    "gnnb_pna_edge_model_create": (_I, [_DESC, _I, _PP, _I, _PP]),
    "gnnb_aggregate_pna_edges": (_I, [_P, _P, _P, _P, _I, _P, _I, _P, _P, _I, _P]),
}


# ... and of include/gnnb_gat.h (GATv2 models), in its order (tests/test_abi_gat.py)
ABI_GAT = {
    "gnnb_gat_model_num_params": (_I, [_DESC, _I]),
    "gnnb_gat_model_create": (_I, [_DESC, _I, _F, _PP, _I, _PP]),
    "gnnb_model_gat_heads": (_I, [_P]),
    "gnnb_aggregate_gatv2": (_I, [_P, _P, _I, _P, _I, _P, _P, _P, _I, _I, _F, _P, _I, _P]),
}


# ... and of include/gnnb_gat_edge.h (GATv2 models with edge features), in its order (tests/test_abi_gat_edge.py)
ABI_GAT_EDGE = {
    "gnnb_gat_edge_model_num_params": (_I, [_DESC, _I, _I]),
    "gnnb_gat_edge_model_create": (_I, [_DESC, _I, _F, _I, _PP, _I, _PP]),
    "gnnb_aggregate_gatv2_edges": (_I, [_P, _P, _I, _P, _I, _P, _P, _P, _I, _I, _F, _P, _I, _P, _I, _P, _I, _P]),
}


# ... and of include/gnnb_transformer.h (TransformerConv models), in its order (tests/test_abi_transformer.py)
ABI_TRANSFORMER = {
    "gnnb_transformer_model_num_params": (_I, [_DESC, _I]),
    "gnnb_transformer_model_create": (_I, [_DESC, _I, _PP, _I, _PP]),
    "gnnb_model_transformer_heads": (_I, [_P]),
    "gnnb_aggregate_transformer": (_I, [_P, _P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _I, _F, _P, _I, _P]),
}


# ... and of include/gnnb_transformer_edge.h (TransformerConv models with edge features), in its order
# (tests/test_abi_transformer_edge.py)
ABI_TRANSFORMER_EDGE = {
    "gnnb_transformer_edge_model_num_params": (_I, [_DESC, _I, _I]),
    "gnnb_transformer_edge_model_create": (_I, [_DESC, _I, _I, _PP, _I, _PP]),
    "gnnb_aggregate_transformer_edges": (_I, [_P, _P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _I, _F, _P, _I, _P, _I, _P, _I, _P]),
}


# ... and of include/gnnb_resgated.h (ResGatedGraphConv models), in its order (tests/test_abi_resgated.py)
ABI_RESGATED = {
    "gnnb_resgated_model_num_params": (_I, [_DESC]),
    "gnnb_resgated_model_create": (_I, [_DESC, _PP, _I, _PP]),
    "gnnb_model_is_resgated": (_I, [_P]),
    "gnnb_aggregate_resgated": (_I, [_P, _P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _P]),
}


# ... and of include/gnnb_resgated_edge.h (ResGatedGraphConv models with edge features), in its order (tests/test_abi_resgated_edge.py)
ABI_RESGATED_EDGE = {
    "gnnb_resgated_edge_model_num_params": (_I, [_DESC, _I]),
    "gnnb_resgated_edge_model_create": (_I, [_DESC, _I, _PP, _I, _PP]),
    "gnnb_aggregate_resgated_edges": (_I, [_P, _P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _P]),
}


# ... and of include/gnnb_gatconv.h (GAT v1 models), in its order (tests/test_abi_gatconv.py)
ABI_GATCONV = {
    "gnnb_gatconv_model_num_params": (_I, [_DESC, _I]),
    "gnnb_gatconv_model_create": (_I, [_DESC, _I, _F, _PP, _I, _PP]),
    "gnnb_model_gatconv_heads": (_I, [_P]),
    "gnnb_aggregate_gat": (_I, [_P, _P, _I, _P, _I, _P, _I, _P, _P, _I, _I, _F, _P, _I, _P]),
}


# ... and of include/gnnb_gatconv_edge.h (GAT v1 models with edge features), in its order (tests/test_abi_gatconv_edge.py)
ABI_GATCONV_EDGE = {
    "gnnb_gatconv_edge_model_num_params": (_I, [_DESC, _I, _I]),
    "gnnb_gatconv_edge_model_create": (_I, [_DESC, _I, _F, _I, _PP, _I, _PP]),
    "gnnb_aggregate_gat_edges": (_I, [_P, _P, _I, _P, _I, _P, _I, _P, _P, _I, _I, _F, _P, _I, _P, _I, _P, _I, _P]),
}


# ... and of include/gnnb_ggnn.h (GatedGraphConv models), in its order (tests/test_abi_ggnn.py)
ABI_GGNN = {
    "gnnb_ggnn_model_num_params": (_I, [_DESC, _I]),
    "gnnb_ggnn_model_create": (_I, [_DESC, _I, _PP, _I, _PP]),
    "gnnb_model_ggnn_steps": (_I, [_P]),
    "gnnb_aggregate_ggnn": (_I, [_P, _P, _I, _P, _I, _P, _I, _I, _P, _P, _I, _P, _I, _P]),
}


# ... and of include/gnnb_rgcn.h (RGCNConv models with integer edge types), in its order (tests/test_abi_rgcn.py)
ABI_RGCN = {
    "gnnb_rgcn_model_num_params": (_I, [_DESC, _I]),
    "gnnb_rgcn_model_create": (_I, [_DESC, _I, _PP, _I, _PP]),
    "gnnb_model_rgcn_relations": (_I, [_P]),
    "gnnb_forward_batched_types": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P]),
    "gnnb_forward_prepared_types": (_I, [_P, _P, _P, _P, _P, _P]),
    "gnnb_type_ingest_bytes": (_Z, [_I]),
    "gnnb_workspace_enable_type_ingest": (_I, [_P]),
    "gnnb_ingest_pyg_types": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _PP, _PP, _PP, _PP, _P]),
    "gnnb_forward_pyg_types": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P]),
    "gnnb_rgcn_slots": (_I, [_P, _P, _I, _P, _P]),
    "gnnb_aggregate_rgcn": (_I, [_P, _P, _P, _I, _I, _P, _I, _P, _I, _P, _I, _P]),
}


def ingest_bytes(max_graphs: int, max_nodes: int, max_edges: int) -> int:
    """Size of the allocation ``CompiledModel.enable_ingest`` makes for a workspace of these capacities
    (``gnnb_ingest_bytes``): the three output arrays and the sort scratch.  Pure host arithmetic, no GPU needed."""
    return int(load_library(require_gpu=False).gnnb_ingest_bytes(int(max_graphs), int(max_nodes), int(max_edges)))


def order_bytes(max_graphs: int, max_nodes: int, max_edges: int, in_dim: int, mlp_out: int) -> int:
    """Size of the allocation ``CompiledModel.enable_ordered_ingest`` makes beside the ingest's (``gnnb_order_bytes``): the
    ordered ``x`` / ``coo`` / ptr arrays, ``perm``, the per-graph shifts and the staged outputs.  Pure host arithmetic, no GPU needed."""
    return int(load_library(require_gpu=False).gnnb_order_bytes(int(max_graphs), int(max_nodes), int(max_edges), int(in_dim), int(mlp_out)))


def edge_ingest_bytes(max_edges: int, edge_dim: int) -> int:
    """Size of the allocation ``CompiledModel.enable_edge_ingest`` makes beside the ingest's (``gnnb_edge_ingest_bytes``): the edge
    attributes in COO row order.  Pure host arithmetic, no GPU needed; 0 for an ``edge_dim`` outside 1 .. 16."""
    return int(load_library(require_gpu=False).gnnb_edge_ingest_bytes(int(max_edges), int(edge_dim)))


def type_ingest_bytes(max_edges: int) -> int:
    """Size of the allocation ``CompiledModel.enable_type_ingest`` makes beside the ingest's (``gnnb_type_ingest_bytes``): the edge
    types in COO row order, int32.  Pure host arithmetic, no GPU needed."""
    return int(load_library(require_gpu=False).gnnb_type_ingest_bytes(int(max_edges)))


def build_library(force: bool = False) -> Path:
    """Compile csrc/*.hip for gfx950 with hipcc (cross-compiles without a GPU)."""
    if force and LIB_PATH.exists():
        LIB_PATH.unlink()
    proc = subprocess.run(["make", "-C", str(CSRC_DIR)], capture_output=True, text=True)
    if proc.returncode != 0 or not LIB_PATH.exists():
        raise GnnbError(f"hipcc build of libgnnb_hip.so failed:\n{proc.stdout}\n{proc.stderr}")
    return LIB_PATH


_lib: Optional[C.CDLL] = None


def load_library(require_gpu: bool = True) -> C.CDLL:
    """dlopen libgnnb_hip.so.  torch is imported first on purpose: its bundled libamdhip64 has the
    same SONAME as the one the library was linked against, so both share ONE HIP runtime and
    device pointers / streams can cross the boundary."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise GnnbUnavailable(
                f"{LIB_PATH} is not built; run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C gnn-builder_amd/csrc`.  There is no CPU fallback.")
        import torch  # noqa: F401  (HIP runtime first, see docstring)
        lib = C.CDLL(str(LIB_PATH))
        for name, (restype, argtypes) in {**ABI, **ABI_ORDER, **ABI_EDGE, **ABI_PNA_EDGE, **ABI_GAT, **ABI_GAT_EDGE, **ABI_TRANSFORMER,
                                           **ABI_TRANSFORMER_EDGE, **ABI_RESGATED, **ABI_RESGATED_EDGE, **ABI_GATCONV,
                                           **ABI_GATCONV_EDGE, **ABI_GGNN, **ABI_RGCN}.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = lib
    if require_gpu and _lib.gnnb_device_count() <= 0:
        raise GnnbUnavailable("libgnnb_hip.so loaded but no MI355X (HIP device) is visible; "
                              "the product path has no CPU fallback")
    return _lib


def _check(rc: int) -> None:
    if rc != GNNB_OK:
        msg = load_library(require_gpu=False).gnnb_last_error()
        raise (GnnbRangeError if rc == GNNB_ERR_RANGE else GnnbError)(f"libgnnb_hip error {rc}: {msg.decode() if msg else '?'}")


def set_option(name: str, value: int) -> None:
    _check(load_library(require_gpu=False).gnnb_set_option(name.encode(), int(value)))


def make_desc(spec: dict) -> ModelDesc:
    d = ModelDesc()
    # (GINE: GIN's description, "pnae": PNA's, edge_dim beside it; "gatv2": GCN's, heads and negative_slope beside it; "gatv2e": GCN's,
    # all three beside it)
    d.conv_type = CONV[_DESC_BASE.get(spec["conv"], spec["conv"])]
    d.num_layers = spec["num_layers"]
    d.in_dim = spec["in_dim"]
    d.hidden_dim = spec["hidden_dim"]
    d.out_dim = spec["out_dim"]
    d.activation = ACT[spec["activation"]]
    d.skip = int(bool(spec["skip"]))
    d.num_pools = len(spec["pools"])
    for i, p in enumerate(spec["pools"]):
        d.pools[i] = POOL[p]
    d.mlp_num_linear = spec["mlp_hidden_layers"] + 1
    d.mlp_hidden = spec["mlp_hidden"]
    d.mlp_out = spec["mlp_out"]
    d.mlp_activation = ACT[spec["mlp_activation"]]
    d.gin_eps = spec.get("gin_eps", 0.0)
    d.pna_delta = spec.get("pna_delta", 1.0)
    d.output_activation = OUT_ACT[spec.get("output_activation")]
    fpx = spec.get("fpx") or (0, 0)            # (W, I) of the reference's FPX, or None for float
    d.fpx_w, d.fpx_i = int(fpx[0]), int(fpx[1])
    # the design's arithmetic (reference: Project(float_or_fixed, fpx) baked into the generated design): a mode name or
    # number fixes it for this model whatever set_option("math") says later; None = -1 = every launch follows the
    # process-wide option as it stands at that launch (A/B measurements and the tests that toggle it)
    m = spec.get("math")
    d.math = -1 if m is None else (MATH_MODES[m] if isinstance(m, str) else int(m))
    return d


def _stream_ptr(stream=None) -> int:
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return int(s.cuda_stream)


def _dptr(t) -> int:
    return int(t.data_ptr())


def _optr(t) -> Optional[int]:
    """Device pointer of an operand the header lets be NULL."""
    return _dptr(t) if t is not None else None


def _require(t, name: str, dtype, ndim: int, last: Optional[int] = None):
    """A raw pointer crosses the C ABI: a tensor of another dtype / layout / device would be silently reinterpreted
    (a PyG edge_index, int64 [2, E], read as int32 [E, 2] is garbage edges) -- refuse it here."""
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise GnnbError(f"{name} must be a CUDA (HIP) tensor")
    if t.dtype != dtype:
        raise GnnbError(f"{name} must be {dtype}, got {t.dtype}")
    if t.dim() != ndim or (last is not None and t.shape[-1] != last):
        raise GnnbError(f"{name} has shape {tuple(t.shape)}; expected {ndim} dimensions" +
                        (f" with last dimension {last}" if last is not None else ""))
    if not t.is_contiguous():
        raise GnnbError(f"{name} must be contiguous")


def _require_rows(t, name: str, rows: int, width: int, like) -> None:
    """``_require`` for a second input that the kernels read as exactly [rows, width] fp32 beside ``like``."""
    import torch
    _require(t, name, torch.float32, 2, width)
    if t.shape[0] != rows or t.device != like.device:
        raise GnnbError(f"{name} must be [{rows}, {width}] on {like.device}, got {tuple(t.shape)} on {t.device}")


def _out(out, rows: int, width: int, x):
    """The result tensor of an entry point: a new [rows, width] fp32 one on ``x``'s device, or the caller's, checked to be that
    (on the forwards' issue path: no call deeper than ``_require``)."""
    import torch
    if out is None:
        return torch.empty((rows, width), dtype=torch.float32, device=x.device)
    _require(out, "out", torch.float32, 2, width)
    if out.shape[0] != rows or out.device != x.device:
        raise GnnbError(f"out must be [{rows}, {width}] on {x.device}, got {tuple(out.shape)} on {out.device}")
    return out


def _require_strided(t, name: str, rows: Optional[int] = None, min_cols: int = 0) -> None:
    """A matrix whose row stride crosses the ABI beside its pointer (``lda`` / ``ldw``): fp32, CUDA, 2-D with unit column
    stride -- a column slice of a wider buffer is legal, a transposed or column-strided view is not."""
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or \
            (t.shape[1] > 1 and t.stride(1) != 1):
        raise GnnbError(f"{name} must be a 2-D float32 CUDA (HIP) tensor with unit column stride")
    if (rows is not None and t.shape[0] != rows) or t.shape[1] < min_cols:
        raise GnnbError(f"{name} has shape {tuple(t.shape)}; expected " +
                        (f"at least {min_cols} columns" if rows is None else f"{rows} rows"))


# the add-ons of a workspace (CompiledModel.enable_*): the refusal of a call made before its enable
_NOT_ENABLED = {
    "ingest": "ingest is not enabled on this model's workspace: call enable_ingest() once after construction",
    "ordered": "the ordered ingest is not enabled on this model's workspace: call enable_ordered_ingest() once after construction",
    "edges": "the edge ingest is not enabled on this model's workspace: call enable_edge_ingest() once after construction",
    "types": "the type ingest is not enabled on this model's workspace: call enable_type_ingest() once after construction",
}
_INGEST_OUTS = {"ingest": 3, "ordered": 5, "edges": 4, "types": 4}  # arrays its ingest returns (CompiledModel._view_specs)


class _Borrowed:
    """Device memory of a workspace as ``__cuda_array_interface__``: ``torch.as_tensor`` makes a view of it (no copy) that
    keeps this object -- and through it the owner of the memory -- alive."""

    def __init__(self, ptr: int, shape, owner, typestr: str = "<i4"):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}
        self._owner = owner


class CompiledModel:
    """Device-resident model: weights uploaded once (the reference's copy_parameters_flag=1 call),
    plus one workspace sized for the largest batch it will see."""

    def __init__(self, spec: dict, params: Sequence, max_graphs: int, max_nodes: int, max_edges: int,
                 max_graph_nodes: int = 0):
        # every attribute first: close() / __del__ also run on an object whose construction raised part-way
        self.lib = None
        self._model, self._ws = C.c_void_p(), C.c_void_p()
        self._B = self._N = self._E = 0  # sizes of the prepared batch (_prepared)
        self._keep = None  # its index tensors, which the device still reads
        self._addons = set()  # what the enable_* calls have allocated beside the workspace: "ingest", "ordered", "edges"
        self._views = {}  # add-on -> (device pointers, views of its whole arrays): _borrowed_views
        self.edge_dim = int(spec.get("edge_dim", 0) or 0) if spec.get("conv") in _EDGE_CONVS else 0
        self.gat_heads = int(spec.get("heads", 1) or 0) if spec.get("conv") in _GAT_CONVS else 0
        self.transformer_heads = int(spec.get("heads", 1) or 0) if spec.get("conv") in _TRANSFORMER_CONVS else 0
        self.gatconv_heads = int(spec.get("heads", 1) or 0) if spec.get("conv") in _GATCONV_CONVS else 0
        self.ggnn_steps = int(spec.get("steps", 1) or 0) if spec.get("conv") == "ggnn" else 0
        self.rgcn_relations = int(spec.get("relations", 1) or 0) if spec.get("conv") == "rgcn" else 0
        self.spec, self.desc = dict(spec), None
        self.max_graphs, self.max_nodes, self.max_edges = int(max_graphs), int(max_nodes), int(max_edges)
        self.lib = load_library(require_gpu=True)
        self.desc = make_desc(spec)
        host = [np.ascontiguousarray(np.asarray(p.detach().cpu().numpy() if hasattr(p, "detach") else p,
                                                dtype=np.float32)) for p in params]
        if spec.get("conv") in _EDGE_CONVS and not 1 <= self.edge_dim <= MAX_EDGE_DIM:
            raise GnnbError(f"a {spec['conv'].upper()} model needs spec['edge_dim'] in 1 .. {MAX_EDGE_DIM}, got {spec.get('edge_dim')!r}")
        # (an edge model's own pair of entries: gnnb_edge.h for GINE, gnnb_pna_edge.h for PNA with edge features)
        num_params, create = ((self.lib.gnnb_pna_edge_model_num_params, self.lib.gnnb_pna_edge_model_create) if spec.get("conv") == "pnae" else
                              (self.lib.gnnb_edge_model_num_params, self.lib.gnnb_edge_model_create))
        n_expect = (self.lib.gnnb_gat_edge_model_num_params(C.byref(self.desc), self.gat_heads, self.edge_dim) if spec.get("conv") == "gatv2e" else
                    self.lib.gnnb_transformer_edge_model_num_params(C.byref(self.desc), self.transformer_heads, self.edge_dim)
                    if spec.get("conv") == "transformere" else
                    self.lib.gnnb_resgated_edge_model_num_params(C.byref(self.desc), self.edge_dim) if spec.get("conv") == "resgatede" else
                    self.lib.gnnb_gatconv_edge_model_num_params(C.byref(self.desc), self.gatconv_heads, self.edge_dim)
                    if spec.get("conv") == "gate" else
                    num_params(C.byref(self.desc), self.edge_dim) if self.edge_dim else
                    self.lib.gnnb_gat_model_num_params(C.byref(self.desc), self.gat_heads) if spec.get("conv") == "gatv2" else
                    self.lib.gnnb_transformer_model_num_params(C.byref(self.desc), self.transformer_heads) if spec.get("conv") == "transformer" else
                    self.lib.gnnb_resgated_model_num_params(C.byref(self.desc)) if spec.get("conv") == "resgated" else
                    self.lib.gnnb_gatconv_model_num_params(C.byref(self.desc), self.gatconv_heads) if spec.get("conv") == "gat" else
                    self.lib.gnnb_ggnn_model_num_params(C.byref(self.desc), self.ggnn_steps) if spec.get("conv") == "ggnn" else
                    self.lib.gnnb_rgcn_model_num_params(C.byref(self.desc), self.rgcn_relations) if spec.get("conv") == "rgcn" else
                    self.lib.gnnb_model_num_params(C.byref(self.desc)))
        if n_expect < 0:
            _check(n_expect)
        if len(host) != n_expect:
            raise GnnbError(f"model needs {n_expect} parameter tensors, got {len(host)}")
        arr = (C.c_void_p * len(host))(*[h.ctypes.data for h in host])
        if spec.get("conv") == "gatv2e":  # (gnnb_gat_edge.h: a GCN description, heads, negative_slope and edge_dim beside it)
            _check(self.lib.gnnb_gat_edge_model_create(C.byref(self.desc), self.gat_heads, float(spec.get("negative_slope", 0.2)), self.edge_dim,
                                                       arr, len(host), C.byref(self._model)))
        elif spec.get("conv") == "transformere":  # (gnnb_transformer_edge.h: a GIN description, heads and edge_dim beside it)
            _check(self.lib.gnnb_transformer_edge_model_create(C.byref(self.desc), self.transformer_heads, self.edge_dim, arr, len(host),
                                                               C.byref(self._model)))
        elif spec.get("conv") == "resgatede":  # (gnnb_resgated_edge.h: a GIN description, the "gated" mark and edge_dim beside it)
            _check(self.lib.gnnb_resgated_edge_model_create(C.byref(self.desc), self.edge_dim, arr, len(host), C.byref(self._model)))
        elif spec.get("conv") == "gate":  # (gnnb_gatconv_edge.h: a GCN description, heads, negative_slope and edge_dim beside it)
            _check(self.lib.gnnb_gatconv_edge_model_create(C.byref(self.desc), self.gatconv_heads, float(spec.get("negative_slope", 0.2)),
                                                           self.edge_dim, arr, len(host), C.byref(self._model)))
        elif self.edge_dim:
            _check(create(C.byref(self.desc), self.edge_dim, arr, len(host), C.byref(self._model)))
        elif spec.get("conv") == "gatv2":  # (gnnb_gat.h: a GCN description, heads and negative_slope beside it)
            _check(self.lib.gnnb_gat_model_create(C.byref(self.desc), self.gat_heads, float(spec.get("negative_slope", 0.2)), arr, len(host),
                                                  C.byref(self._model)))
        elif spec.get("conv") == "transformer":  # (gnnb_transformer.h: a GIN description, heads beside it)
            _check(self.lib.gnnb_transformer_model_create(C.byref(self.desc), self.transformer_heads, arr, len(host), C.byref(self._model)))
        elif spec.get("conv") == "resgated":  # (gnnb_resgated.h: a GIN description, the "gated" mark beside it)
            _check(self.lib.gnnb_resgated_model_create(C.byref(self.desc), arr, len(host), C.byref(self._model)))
        elif spec.get("conv") == "gat":  # (gnnb_gatconv.h: a GCN description, heads and negative_slope beside it)
            _check(self.lib.gnnb_gatconv_model_create(C.byref(self.desc), self.gatconv_heads, float(spec.get("negative_slope", 0.2)), arr,
                                                      len(host), C.byref(self._model)))
        elif spec.get("conv") == "ggnn":  # (gnnb_ggnn.h: a GIN description, steps beside it)
            _check(self.lib.gnnb_ggnn_model_create(C.byref(self.desc), self.ggnn_steps, arr, len(host), C.byref(self._model)))
        elif spec.get("conv") == "rgcn":  # (gnnb_rgcn.h: a GIN description, the relation count beside it)
            _check(self.lib.gnnb_rgcn_model_create(C.byref(self.desc), self.rgcn_relations, arr, len(host), C.byref(self._model)))
        else:
            _check(self.lib.gnnb_model_create(C.byref(self.desc), arr, len(host), C.byref(self._model)))
        rc = self.lib.gnnb_workspace_create(self._model, self.max_graphs, self.max_nodes, self.max_edges, C.byref(self._ws))
        if rc != GNNB_OK:
            self.close()
            _check(rc)
        if max_graph_nodes:
            self.set_max_graph_nodes(max_graph_nodes)

    @classmethod
    def from_model(cls, model, max_graphs: int, max_nodes: int, max_edges: int,
                   max_graph_nodes: int = 0, fpx=None, math=None) -> "CompiledModel":
        """``model``: a ``gnnbuilder_amd.models.GNNModel``.  ``max_graph_nodes``: promise on the largest
        graph (0 = none); small molecules enable the LDS-resident fused kernels, and the promise is
        validated on the device (``check()`` raises if a batch breaks it).  ``fpx``: ``(W, I)`` or a
        ``code_gen.FPX`` = layer-boundary emulation of the reference's ``ap_fixed<W, I>`` build (None: float).
        ``math``: "fp32" | "bf16x6" | "bf16x3" | "f16x3" (or 0..3) = the model's own arithmetic, captured at creation
        (``gnnb_model_desc::math``); None = follow ``set_option("math", ...)`` at every launch.  In the reduced modes
        ``check()`` raises ``GnnbRangeError`` when a kernel produced a non-finite value (fp16's range)."""
        spec = model.spec()
        if math is not None:
            spec["math"] = math
        if fpx is not None:
            spec["fpx"] = (int(fpx.W), int(fpx.I)) if hasattr(fpx, "W") else (int(fpx[0]), int(fpx[1]))
        return cls(spec, model.canonical_params(), max_graphs, max_nodes, max_edges, max_graph_nodes)

    def set_max_graph_nodes(self, n: int) -> None:
        """Promise on the largest graph of the following batches (0 = none).  Like ``set_max_degree`` and ``set_large_segment`` it
        takes effect at the NEXT graph prep (``graph_prep``, or the one inside ``forward`` / ``forward_edges`` / ``forward_pyg*`` /
        ``forward_prepared_prep_next``'s ``nxt``): a batch that is already prepared runs ``forward_prepared`` /
        ``forward_prepared_edges`` / ``forward_prepared_prep_next`` by what its own prep validated and baked into the tables,
        whatever has been set since -- the same route and the same bits as without the call."""
        _check(self.lib.gnnb_workspace_set_max_graph_nodes(self._ws, int(n)))

    def set_max_degree(self, d: int) -> None:
        """Promise on the largest in-degree of the following batches (0 = none; a bound, where the reference's ``degree_guess`` is a hint): PNA models
        then run their post-NN products in the degree-class form (d <= 15).  Validated on the device (``check()``).  Takes effect at
        the next graph prep (``set_max_graph_nodes``): the class tables belong to the prepared batch."""
        _check(self.lib.gnnb_workspace_set_max_degree(self._ws, int(d)))

    def stream_k_guard(self, stream=None) -> None:
        """Diagnostics (``gnnb_debug_stream_k_guard``): raises unless this workspace's stream-K scratch has every arrival
        counter at zero and an untouched guard region behind the counters.  Synchronises the stream."""
        _check(self.lib.gnnb_debug_stream_k_guard(self._ws, _stream_ptr(stream)))

    def last_path(self) -> str:
        """Which kernels the last forward on this workspace ran: "layerwise", "stack" (k_gcn2_fused) or "stack_zf"
        (k_gcn2_zf); "none" before the first forward.  Diagnostics only."""
        v = int(self.lib.gnnb_workspace_last_path(self._ws))
        return PATH_NAMES.get(v & (PATH_LARGE_LAYERWISE - 1), "?") + ("+large_layerwise" if v & PATH_LARGE_LAYERWISE else "")

    def set_large_segment(self, first_graph: int = -1, first_node: int = -1, first_edge: int = -1) -> None:
        """Graphs [first_graph, B) of the following batches are exempt from the max_graph_nodes promise and run layer by
        layer while the rest takes the LDS-resident stack (``gnnb_workspace_set_large_segment``); the caller orders the
        batch so that they come last (``batching.order_large_last``).  No arguments: no large segment.  Takes effect at the next
        graph prep (``set_max_graph_nodes``): a prepared batch keeps the segment it was prepared with, the one that was checked
        against it."""
        _check(self.lib.gnnb_workspace_set_large_segment(self._ws, int(first_graph), int(first_node), int(first_edge)))

    @property
    def out_dim(self) -> int:
        return int(self.desc.mlp_out)

    @property
    def workspace_bytes(self) -> int:
        return int(self.lib.gnnb_workspace_bytes(self._ws))

    def close(self) -> None:
        self._views = {}  # (they borrow the workspace: dropped with it)
        if self._ws:
            self.lib.gnnb_workspace_destroy(self._ws)
            self._ws = C.c_void_p()
        if self._model:
            self.lib.gnnb_model_destroy(self._model)
            self._model = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ whole forward
    def _prepared(self, B: int, N: int, E: int, keep) -> None:
        """The workspace now holds the tables of a batch of these sizes: the stage-level entry points may follow, and check their
        operands against them.  ``keep``: the batch's index tensors, which the device reads for as long as the batch is prepared."""
        self._B, self._N, self._E, self._keep = B, N, E, keep

    def _require_x(self, x, width: Optional[int] = None) -> None:
        """``x`` of an entry point that runs on the prepared batch: the kernels read a row of it for every node of that batch."""
        import torch
        _require(x, "x", torch.float32, 2, width)
        if int(x.shape[0]) != self._N:
            raise GnnbError(f"x has {int(x.shape[0])} rows, the prepared batch has {self._N} nodes")

    def forward(self, x, coo, node_ptr, edge_ptr, out=None, stream=None):
        """All arguments are torch CUDA tensors (fp32 / int32, contiguous; ``coo`` is [E, 2] (src, dst) rows, NOT a PyG
        ``edge_index`` [2, E] -- transpose it); returns ``out`` [B, mlp_out].  Asynchronous on the current torch stream.
        With a ``max_graph_nodes`` promise set, call ``check()`` on the batch: a broken promise is flagged there, and
        the results of a flagged batch are unspecified.  Without a ``check()`` the flag still surfaces: the next call
        on this workspace after a flagged batch has run raises ``GnnbError`` ("an earlier batch ...", no synchronisation,
        best effort)."""
        return self._forward_batched(False, x, None, coo, node_ptr, edge_ptr, out, stream)

    def _forward_batched(self, edges: bool, x, edge_attr, coo, node_ptr, edge_ptr, out, stream):
        """``forward`` and, with ``edges``, ``forward_edges`` (``gnnb_forward_batched_edges``: ``edge_attr`` behind ``x``)."""
        B, N, E = self._check_batch(x, coo, node_ptr, edge_ptr)
        ea = self._require_edge_attr(edge_attr, E, x) if edges else None
        out = _out(out, B, self.out_dim, x)
        tail = (_dptr(coo), _dptr(node_ptr), _dptr(edge_ptr), B, N, E, _dptr(out), _stream_ptr(stream))
        _check(self.lib.gnnb_forward_batched_edges(self._model, self._ws, _dptr(x), ea, *tail) if edges else
               self.lib.gnnb_forward_batched(self._model, self._ws, _dptr(x), *tail))
        self._prepared(B, N, E, (coo, node_ptr, edge_ptr))
        return out

    def _check_batch(self, x, coo, node_ptr, edge_ptr, num_nodes=None):
        """Checks of a batch's tensors (raw pointers cross the C ABI); returns (B, N, E) -- N from ``x``, or ``num_nodes`` without one."""
        import torch
        if x is not None:
            _require(x, "x", torch.float32, 2, int(self.desc.in_dim))
        _require(coo, "coo", torch.int32, 2, 2)
        _require(node_ptr, "node_ptr", torch.int32, 1)
        _require(edge_ptr, "edge_ptr", torch.int32, 1)
        if node_ptr.numel() != edge_ptr.numel() or node_ptr.numel() < 1:
            raise GnnbError("node_ptr and edge_ptr must both have num_graphs + 1 entries")
        return int(node_ptr.numel()) - 1, int(num_nodes if x is None else x.shape[0]), int(coo.shape[0])

    def graph_prep(self, coo, node_ptr, edge_ptr, num_nodes: int, stream=None) -> None:
        B, N, E = self._check_batch(None, coo, node_ptr, edge_ptr, num_nodes)
        _check(self.lib.gnnb_graph_prep(self._ws, _dptr(coo), _dptr(node_ptr), _dptr(edge_ptr), B, N, E,
                                        float(self.desc.pna_delta), _stream_ptr(stream)))
        self._prepared(B, N, E, (coo, node_ptr, edge_ptr))

    def forward_prepared(self, x, out=None, stream=None):
        self._require_x(x, int(self.desc.in_dim))
        out = _out(out, self._B, self.out_dim, x)
        _check(self.lib.gnnb_forward_prepared(self._model, self._ws, _dptr(x), _dptr(out), _stream_ptr(stream)))
        return out

    def forward_prepared_prep_next(self, x, nxt: "CompiledModel", coo, node_ptr, edge_ptr, num_nodes: int, out=None, stream=None):
        """``forward_prepared(x)`` on this object's prepared batch, then the graph prep of the NEXT batch on the workspace of
        ``nxt`` -- a second ``CompiledModel`` of the same design (two alternate along a stream of batches) -- in one call
        (``gnnb_forward_prepared_prep_next``): where the forward runs the 2-layer GCN stack kernel, the prep runs inside it.
        ``nxt.forward_prepared`` / ``nxt.forward_prepared_prep_next`` is then the next batch's forward."""
        self._require_x(x, int(self.desc.in_dim))
        out = _out(out, self._B, self.out_dim, x)
        B, N, E = self._check_batch(None, coo, node_ptr, edge_ptr, num_nodes)
        _check(self.lib.gnnb_forward_prepared_prep_next(self._model, self._ws, _dptr(x), _dptr(out), nxt._ws, _dptr(coo), _dptr(node_ptr),
                                                        _dptr(edge_ptr), B, N, E, _stream_ptr(stream)))
        nxt._prepared(B, N, E, (coo, node_ptr, edge_ptr))
        return out

    def check(self, stream=None) -> None:
        _check(self.lib.gnnb_workspace_check(self._ws, _stream_ptr(stream)))

    def forward_host(self, x: np.ndarray, coo: np.ndarray, node_ptr: np.ndarray, edge_ptr: np.ndarray) -> np.ndarray:
        """Host-buffer entry (numpy in, numpy out; synchronous)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        coo = np.ascontiguousarray(coo, dtype=np.int32).reshape(-1, 2)
        node_ptr = np.ascontiguousarray(node_ptr, dtype=np.int32)
        edge_ptr = np.ascontiguousarray(edge_ptr, dtype=np.int32)
        B = node_ptr.shape[0] - 1
        out = np.zeros((B, self.out_dim), np.float32)
        _check(self.lib.gnnb_forward_batched_host(
            self._model, self._ws, x.ctypes.data_as(C.c_void_p), coo.ctypes.data_as(C.c_void_p),
            node_ptr.ctypes.data_as(C.c_void_p), edge_ptr.ctypes.data_as(C.c_void_p), B, x.shape[0],
            coo.shape[0], out.ctypes.data_as(C.c_void_p)))
        # (the workspace now holds THIS batch's tables -- its index arrays live in the workspace's staging buffer: without this
        # tables_to_host and the stage entries would size and check their buffers by the batch prepared before)
        self._prepared(B, int(x.shape[0]), int(coo.shape[0]), None)
        return out

    # ------------------------------------------------------------------ PyG mini-batches
    def enable_ingest(self) -> None:
        """One more device allocation (``ingest_bytes`` of the workspace's capacities) for ``ingest_pyg`` / ``forward_pyg``.
        Synchronous: call it once, right after construction, outside stream capture."""
        _check(self.lib.gnnb_workspace_enable_ingest(self._ws))
        self._addons.add("ingest")

    def _view_specs(self, addon: str):
        """(shape, typestr) of the whole arrays an add-on's ingest returns, in the order of its out-pointers."""
        G, cap_e = self.max_graphs, max(self.max_edges, 1)
        coo = [((cap_e, 2), "<i4"), ((G + 1,), "<i4"), ((G + 1,), "<i4")]  # coo, node_ptr, edge_ptr
        return {"ingest": coo,
                "ordered": [((self.max_nodes, max(int(self.desc.in_dim), 1)), "<f4")] + coo + [((G,), "<i4")],  # x_ord ..., perm
                "edges": coo + [((cap_e, self.edge_dim), "<f4")],  # ..., edge_attr_ord
                "types": coo + [((cap_e,), "<i4")]}[addon]  # ..., edge_type_ord

    def _ingest(self, addon: str, fn, lead, batch, ptr, sizes, dev, stream, ints: int = 0):
        """What the three ingests share: ``fn(ws, *lead, batch, ptr, *sizes, <the add-on's out-pointers>, <ints int*>, stream)``;
        returns views of the whole output arrays and the integers.  The views are made the first time the pointers are seen (the
        allocation never moves) and every call slices them: no HIP call per ingest after the first, so a warmed-up ingest can be
        captured into a graph."""
        out_p = [C.c_void_p() for _ in range(_INGEST_OUTS[addon])]
        seg = [C.c_int() for _ in range(ints)]
        _check(fn(self._ws, *lead, _optr(batch), _optr(ptr), *sizes, *[C.byref(p) for p in out_p], *[C.byref(v) for v in seg],
                  _stream_ptr(stream)))
        ptrs = tuple(p.value for p in out_p)
        cached = self._views.get(addon)
        if cached is None or cached[0] != ptrs:
            import torch
            specs = self._view_specs(addon)
            assert len(specs) == len(ptrs), (addon, "_INGEST_OUTS and _view_specs disagree")
            cached = self._views[addon] = (ptrs, [torch.as_tensor(_Borrowed(p, shape, self, typestr), device=dev)
                                                  for p, (shape, typestr) in zip(ptrs, specs)])
        return cached[1], tuple(int(v.value) for v in seg)

    def _pyg_args(self, edge_index, batch, ptr, num_graphs, num_nodes):
        """Checks of a PyG mini-batch's index tensors (raw pointers cross the C ABI); returns (batch or None, ptr or None, B, N, E)."""
        import torch
        if "ingest" not in self._addons:
            raise GnnbError(_NOT_ENABLED["ingest"])
        if isinstance(edge_index, torch.Tensor) and edge_index.dim() == 2 and edge_index.shape[0] != 2 and edge_index.shape[1] == 2:
            raise GnnbError(f"edge_index has shape {tuple(edge_index.shape)}: this is the [E, 2] coo layout; pass the PyG layout "
                            "[2, E] (edge_index.t().contiguous()), or give the [E, 2] int32 rows to forward()")
        _require(edge_index, "edge_index", torch.int64, 2)
        if edge_index.shape[0] != 2:
            raise GnnbError(f"edge_index has shape {tuple(edge_index.shape)}; expected [2, E]")
        E = int(edge_index.shape[1])
        B = None if num_graphs is None else int(num_graphs)
        N = None if num_nodes is None else int(num_nodes)
        if ptr is not None:
            _require(ptr, "ptr", torch.int64, 1)
            if ptr.numel() < 1 or (B is not None and B != ptr.numel() - 1):
                raise GnnbError(f"ptr has {ptr.numel()} entries; expected num_graphs + 1")
            B = int(ptr.numel()) - 1
        if batch is not None:
            _require(batch, "batch", torch.int64, 1)
            if N is not None and N != batch.numel():
                raise GnnbError(f"batch has {batch.numel()} entries; expected one per node ({N})")
            N = int(batch.numel())
            if B is None:
                raise GnnbError("num_graphs is required when only `batch` is given (Batch.num_graphs): reading batch[-1] would be "
                                "a .item() synchronisation hidden in the call; or pass `ptr` as well")
            ptr = None  # (both given: ptr named B; the kernels look graph ids up in batch)
        elif ptr is None:
            if B is None:
                B = 1
            if B != 1:
                raise GnnbError("a batch of more than one graph needs `batch` or `ptr`")
        if N is None:
            raise GnnbError("num_nodes is required when `batch` is not given (x.shape[0])")
        return batch, ptr, B, N, E

    def ingest_pyg(self, edge_index, batch=None, ptr=None, num_graphs=None, stream=None, num_nodes=None):
        """A PyG mini-batch's ``edge_index`` [2, E] int64 with ``batch`` [N] int64 (plus ``num_graphs``: a host integer,
        ``Batch.num_graphs``) or ``ptr`` [B+1] int64 (plus ``num_nodes``) -> ``(coo [E, 2], node_ptr [B+1], edge_ptr [B+1])``,
        int32, computed on the device with no synchronisation -- what ``batching.from_pyg_batch`` computes on the host.  The three
        tensors are VIEWS of this model's workspace: valid until the next ``ingest_pyg`` / ``forward_pyg``.  Malformed input is
        flagged, not refused: ``check()`` raises (flag 0x80), and the arrays of a flagged batch are in range but unspecified."""
        batch, ptr, B, N, E = self._pyg_args(edge_index, batch, ptr, num_graphs, num_nodes)
        (coo, nptr, eptr), _ = self._ingest("ingest", self.lib.gnnb_ingest_pyg, (_dptr(edge_index),), batch, ptr, (B, N, E), edge_index.device, stream)
        return coo[:E], nptr[:B + 1], eptr[:B + 1]

    def forward_pyg(self, x, edge_index, batch=None, ptr=None, num_graphs=None, out=None, stream=None):
        """``forward`` on a PyG mini-batch as the loader holds it on the GPU (``x`` [N, in_dim] fp32, ``edge_index`` [2, E]
        int64, ``batch`` [N] int64 + ``num_graphs``, or ``ptr`` [B+1] int64): ingest and forward on one stream, no host
        synchronisation (``gnnb_forward_pyg``).  The stage-level entry points work afterwards as after ``forward``."""
        return self._forward_pyg(self.lib.gnnb_forward_pyg, "ingest", x, edge_index, None, batch, ptr, num_graphs, out, stream)

    def _forward_pyg(self, fn, addon: str, x, edge_index, edge_attr, batch, ptr, num_graphs, out, stream):
        """``forward_pyg`` ("ingest"), ``forward_pyg_ordered`` ("ordered") and ``forward_pyg_edges`` ("edges": ``edge_attr`` behind
        ``edge_index``) on their C entry ``fn``.  Each refuses in the order it always has: the ordered form names its missing
        add-on before it looks at ``x``, the edge form behind ``x``, the plain form inside ``_pyg_args``."""
        import torch
        if addon == "ordered" and addon not in self._addons:
            raise GnnbError(_NOT_ENABLED[addon])
        _require(x, "x", torch.float32, 2, int(self.desc.in_dim))
        if addon == "edges" and addon not in self._addons:
            raise GnnbError(_NOT_ENABLED[addon])
        batch, ptr, B, N, E = self._pyg_args(edge_index, batch, ptr, num_graphs, int(x.shape[0]))
        ea = self._require_edge_attr(edge_attr, E, x) if addon == "edges" else None
        out = _out(out, B, self.out_dim, x)
        tail = (_optr(batch), _optr(ptr), B, N, E, _dptr(out), _stream_ptr(stream))
        _check(fn(self._model, self._ws, _dptr(x), _dptr(edge_index), ea, *tail) if addon == "edges" else
               fn(self._model, self._ws, _dptr(x), _dptr(edge_index), *tail))
        self._prepared(B, N, E, None)  # (the batch's index arrays, ordered or not, live in the workspace)
        return out

    # ------------------------------------------------------------------ PyG mini-batches, oversized graphs ordered last
    def enable_ordered_ingest(self) -> None:
        """``enable_ingest`` (if that has not been done) and one more device allocation (``order_bytes``) for
        ``ingest_pyg_ordered`` / ``forward_pyg_ordered``.  Synchronous: call it once, right after construction, outside stream
        capture."""
        _check(self.lib.gnnb_workspace_enable_ordered_ingest(self._ws))
        self._addons |= {"ingest", "ordered"}

    def ingest_pyg_ordered(self, x, edge_index, batch=None, ptr=None, num_graphs=None, stream=None):
        """``ingest_pyg`` and, on the device, ``batching.order_large_last`` at this workspace's ``max_graph_nodes`` promise: the
        graphs with more nodes than the promise LAST (stable; promise 0: none is large).  Returns ``(x_ord [N, in_dim], coo
        [E, 2], node_ptr [B+1], edge_ptr [B+1], perm [B], (first_graph, first_node, first_edge))`` -- what
        ``order_large_last(from_pyg_batch(...), promise)`` returns, ``x_ord`` bit for bit; the triple as host integers, which is
        the ONE synchronisation of this path (a wait on ``stream``; not capturable).  The tensors are VIEWS of this model's
        workspace: valid until the next ``ingest_pyg_ordered`` / ``forward_pyg_ordered``."""
        import torch
        if "ordered" not in self._addons:
            raise GnnbError(_NOT_ENABLED["ordered"])
        _require(x, "x", torch.float32, 2, int(self.desc.in_dim))
        batch, ptr, B, N, E = self._pyg_args(edge_index, batch, ptr, num_graphs, int(x.shape[0]))
        (x_ord, coo, nptr, eptr, perm), seg = self._ingest("ordered", self.lib.gnnb_ingest_pyg_ordered, (_dptr(x), _dptr(edge_index)), batch, ptr,
                                                           (B, N, E), edge_index.device, stream, ints=3)
        return x_ord[:N], coo[:E], nptr[:B + 1], eptr[:B + 1], perm[:B], seg

    def forward_pyg_ordered(self, x, edge_index, batch=None, ptr=None, num_graphs=None, out=None, stream=None):
        """``forward_pyg`` for batches that hold a few graphs beyond the ``max_graph_nodes`` promise: ordered ingest, the large
        segment set to its triple (removed when nothing is large), forward, rows put back (``gnnb_forward_pyg_ordered``).
        Returns ``out`` [B, out_dim] in the CALLER's graph order.  Waits once on ``stream`` (three integers; not capturable).  The
        large-segment setting is left on the workspace; the stage-level entry points work afterwards, on the ORDERED batch."""
        return self._forward_pyg(self.lib.gnnb_forward_pyg_ordered, "ordered", x, edge_index, None, batch, ptr, num_graphs, out, stream)

    # ------------------------------------------------------------------ GINE, PNAE, GATv2E and TransformerE models: forwards with edge attributes
    def _require_edge_attr(self, edge_attr, E: int, like, width: Optional[int] = None):
        """``edge_attr`` of an entry point that reads one [edge_dim] row per edge: fp32 [E, edge_dim] on ``like``'s device; an
        empty batch's may be None.  Returns its device pointer (None: NULL)."""
        width = self.edge_dim if width is None else width
        if edge_attr is None:
            if E:
                raise GnnbError(f"edge_attr is required: the batch has {E} edges")
            return None
        _require_rows(edge_attr, "edge_attr", E, width, like)
        return _dptr(edge_attr) if E else None

    def _require_edge_model(self, what: str) -> None:
        if not self.edge_dim:
            raise GnnbError(f"{what} takes a GINE or PNAE model, or GATv2 with edge features (a GNNModel of GINEConv_GNNB, PNAEConv_GNNB or "
                            "GATv2EConv_GNNB layers: edge weights); this model has none")

    def forward_edges(self, x, edge_attr, coo, node_ptr, edge_ptr, out=None, stream=None):
        """``forward`` of a GINE model: ``edge_attr`` [E, edge_dim] fp32, row ``i`` belongs to ``coo`` row ``i``
        (``gnnb_forward_batched_edges``).  Everything else as ``forward``."""
        self._require_edge_model("forward_edges")
        return self._forward_batched(True, x, edge_attr, coo, node_ptr, edge_ptr, out, stream)

    def forward_prepared_edges(self, x, edge_attr, out=None, stream=None):
        """``forward_prepared`` of a GINE model on the batch ``graph_prep`` left in the workspace."""
        self._require_edge_model("forward_prepared_edges")
        self._require_x(x, int(self.desc.in_dim))
        ea = self._require_edge_attr(edge_attr, self._E, x)
        out = _out(out, self._B, self.out_dim, x)
        _check(self.lib.gnnb_forward_prepared_edges(self._model, self._ws, _dptr(x), ea, _dptr(out), _stream_ptr(stream)))
        return out

    def enable_edge_ingest(self) -> None:
        """``enable_ingest`` (if that has not been done) and one more device allocation (``edge_ingest_bytes``) for
        ``ingest_pyg_edges`` / ``forward_pyg_edges``.  Synchronous: call it once, right after construction, outside stream
        capture."""
        self._require_edge_model("enable_edge_ingest")
        _check(self.lib.gnnb_workspace_enable_edge_ingest(self._ws))
        self._addons |= {"ingest", "edges"}

    def ingest_pyg_edges(self, edge_index, edge_attr, batch=None, ptr=None, num_graphs=None, stream=None, num_nodes=None):
        """``ingest_pyg`` with the mini-batch's ``edge_attr`` [E, edge_dim] fp32 (``Batch.edge_attr``, in ``edge_index``'s column
        order): returns ``(coo, node_ptr, edge_ptr, edge_attr_ord)`` with ``edge_attr_ord[i]`` the attributes of ``coo`` row ``i`` --
        what ``batching.from_pyg_batch(..., edge_attr=...)`` computes on the host, with no synchronisation
        (``gnnb_ingest_pyg_edges``).  VIEWS of the workspace: valid until the next ingest on it."""
        if "edges" not in self._addons:
            raise GnnbError(_NOT_ENABLED["edges"])
        batch, ptr, B, N, E = self._pyg_args(edge_index, batch, ptr, num_graphs, num_nodes)
        ea = self._require_edge_attr(edge_attr, E, edge_index)
        (coo, nptr, eptr, ea_ord), _ = self._ingest("edges", self.lib.gnnb_ingest_pyg_edges, (_dptr(edge_index), ea), batch, ptr, (B, N, E),
                                                    edge_index.device, stream)
        return coo[:E], nptr[:B + 1], eptr[:B + 1], ea_ord[:E]

    def forward_pyg_edges(self, x, edge_index, edge_attr, batch=None, ptr=None, num_graphs=None, out=None, stream=None):
        """``forward_pyg`` of a GINE model: ``edge_attr`` [E, edge_dim] fp32 in ``edge_index``'s column order; ingest (the
        attribute rows follow their edges) and forward on one stream, no host synchronisation, capturable
        (``gnnb_forward_pyg_edges``)."""
        self._require_edge_model("forward_pyg_edges")
        return self._forward_pyg(self.lib.gnnb_forward_pyg_edges, "edges", x, edge_index, edge_attr, batch, ptr, num_graphs, out, stream)

    # ------------------------------------------------------------------ RGCNConv models: forwards with integer edge types
    def _require_edge_type(self, edge_type, E: int, like, dtype):
        """``edge_type`` of an entry point that reads one integer per edge: ``dtype`` [E], contiguous, on ``like``'s device; an
        empty batch's may be None.  Returns its device pointer (None: NULL)."""
        if edge_type is None:
            if E:
                raise GnnbError(f"edge_type is required: the batch has {E} edges")
            return None
        _require(edge_type, "edge_type", dtype, 1)
        if edge_type.numel() != E or edge_type.device != like.device:
            raise GnnbError(f"edge_type must be [{E}] on {like.device}, got {tuple(edge_type.shape)} on {edge_type.device}")
        return _dptr(edge_type) if E else None

    def _require_rgcn_model(self, what: str) -> None:
        if not self.rgcn_relations:
            raise GnnbError(f"{what} takes an RGCNConv model (a GNNModel of RGCNConv_GNNB layers: relations); this model has none")

    def forward_types(self, x, edge_type, coo, node_ptr, edge_ptr, out=None, stream=None):
        """``forward`` of an RGCNConv model: ``edge_type`` [E] int32, entry ``i`` belongs to ``coo`` row ``i``
        (``gnnb_forward_batched_types``).  A type outside ``[0, relations)`` is flagged, not refused: ``check()`` raises (flag
        0x100).  Everything else as ``forward``."""
        import torch
        self._require_rgcn_model("forward_types")
        B, N, E = self._check_batch(x, coo, node_ptr, edge_ptr)
        et = self._require_edge_type(edge_type, E, x, torch.int32)
        out = _out(out, B, self.out_dim, x)
        _check(self.lib.gnnb_forward_batched_types(self._model, self._ws, _dptr(x), et, _dptr(coo), _dptr(node_ptr), _dptr(edge_ptr), B, N, E,
                                                   _dptr(out), _stream_ptr(stream)))
        self._prepared(B, N, E, (coo, node_ptr, edge_ptr))
        return out

    def forward_prepared_types(self, x, edge_type, out=None, stream=None):
        """``forward_prepared`` of an RGCNConv model on the batch ``graph_prep`` left in the workspace."""
        import torch
        self._require_rgcn_model("forward_prepared_types")
        self._require_x(x, int(self.desc.in_dim))
        et = self._require_edge_type(edge_type, self._E, x, torch.int32)
        out = _out(out, self._B, self.out_dim, x)
        _check(self.lib.gnnb_forward_prepared_types(self._model, self._ws, _dptr(x), et, _dptr(out), _stream_ptr(stream)))
        return out

    def enable_type_ingest(self) -> None:
        """``enable_ingest`` (if that has not been done) and one more device allocation (``type_ingest_bytes``) for
        ``ingest_pyg_types`` / ``forward_pyg_types``.  Synchronous: call it once, right after construction, outside stream
        capture."""
        self._require_rgcn_model("enable_type_ingest")
        _check(self.lib.gnnb_workspace_enable_type_ingest(self._ws))
        self._addons |= {"ingest", "types"}

    def ingest_pyg_types(self, edge_index, edge_type, batch=None, ptr=None, num_graphs=None, stream=None, num_nodes=None):
        """``ingest_pyg`` with the mini-batch's ``edge_type`` [E] int64 (``Batch.edge_type``, in ``edge_index``'s column order):
        returns ``(coo, node_ptr, edge_ptr, edge_type_ord)`` with ``edge_type_ord[i]`` (int32) the type of ``coo`` row ``i`` -- what
        ``batching.from_pyg_batch(..., edge_type=...)`` computes on the host, with no synchronisation (``gnnb_ingest_pyg_types``).
        VIEWS of the workspace: valid until the next ingest on it."""
        import torch
        if "types" not in self._addons:
            raise GnnbError(_NOT_ENABLED["types"])
        batch, ptr, B, N, E = self._pyg_args(edge_index, batch, ptr, num_graphs, num_nodes)
        et = self._require_edge_type(edge_type, E, edge_index, torch.int64)
        (coo, nptr, eptr, et_ord), _ = self._ingest("types", self.lib.gnnb_ingest_pyg_types, (_dptr(edge_index), et), batch, ptr, (B, N, E),
                                                    edge_index.device, stream)
        return coo[:E], nptr[:B + 1], eptr[:B + 1], et_ord[:E]

    def forward_pyg_types(self, x, edge_index, edge_type, batch=None, ptr=None, num_graphs=None, out=None, stream=None):
        """``forward_pyg`` of an RGCNConv model: ``edge_type`` [E] int64 in ``edge_index``'s column order; ingest (the types
        follow their edges) and forward on one stream, no host synchronisation, capturable (``gnnb_forward_pyg_types``)."""
        import torch
        self._require_rgcn_model("forward_pyg_types")
        _require(x, "x", torch.float32, 2, int(self.desc.in_dim))
        if "types" not in self._addons:
            raise GnnbError(_NOT_ENABLED["types"])
        batch, ptr, B, N, E = self._pyg_args(edge_index, batch, ptr, num_graphs, int(x.shape[0]))
        et = self._require_edge_type(edge_type, E, x, torch.int64)
        out = _out(out, B, self.out_dim, x)
        _check(self.lib.gnnb_forward_pyg_types(self._model, self._ws, _dptr(x), _dptr(edge_index), et, _optr(batch), _optr(ptr), B, N, E,
                                               _dptr(out), _stream_ptr(stream)))
        self._prepared(B, N, E, None)  # (the batch's index arrays live in the workspace)
        return out

    # ------------------------------------------------------------------ stage-level entry points
    # (raw pointers cross the C ABI: each checks every operand's dtype, layout, device and rows against the prepared batch, so
    # that a short, narrower, int64, CPU or strided tensor is refused here instead of read out of bounds or reinterpreted)
    def tables_to_host(self, stream=None):
        row_ptr = np.zeros(self._N + 1, np.int32)
        col = np.zeros(max(self._E, 1), np.int32)
        in_deg = np.zeros(max(self._N, 1), np.int32)
        _check(self.lib.gnnb_graph_tables_to_host(self._ws, row_ptr.ctypes.data_as(C.c_void_p),
                                                  col.ctypes.data_as(C.c_void_p),
                                                  in_deg.ctypes.data_as(C.c_void_p), _stream_ptr(stream)))
        return row_ptr, col[:self._E], in_deg[:self._N]

    def _aggregate_operands(self, kind: str, x, self_term, out, w: Optional[int] = None):
        """Operands of ``gnnb_aggregate``: the kernel reads x[j * w] for every source j of the prepared batch, and the PNA
        destination term beside it; returns (w, out)."""
        self._require_x(x, w)
        w = int(x.shape[1])
        if self_term is not None:
            _require_rows(self_term, "self_term", self._N, w, x)
        return w, _out(out, self._N, 4 * w if kind == "pna" else w, x)

    def aggregate(self, kind: str, x, self_term=None, eps: float = 0.0, out=None, stream=None):
        w, out = self._aggregate_operands(kind, x, self_term, out)
        _check(self.lib.gnnb_aggregate(self._ws, AGG[kind], _dptr(x), _optr(self_term), _dptr(out), w,
                                       float(eps), _stream_ptr(stream)))
        return out

    def pna_product_aggregate(self, x, wb, out=None, stream=None):
        """``max | min | mean | std`` over every node's sources of ``p_j = wb @ x_j`` in one kernel (``k_pna_pagg``); ``wb``:
        [width, ldw] view of the x_j half of the pre-NN weight (``W_pre[:, width:]``: a strided view is fine, the row stride is
        passed on).  Needs the workspace's ``max_graph_nodes`` promise (<= 57 with the default node tiles)."""
        import torch
        self._require_x(x)
        w = int(x.shape[1])
        if wb.dtype != torch.float32 or wb.dim() != 2 or tuple(wb.shape) != (w, w) or wb.stride(1) != 1 or wb.device != x.device:
            raise GnnbError(f"wb must be a [{w}, {w}] float32 view with unit column stride on {x.device}")
        out = _out(out, self._N, 4 * w, x)
        _check(self.lib.gnnb_pna_product_aggregate(self._ws, _dptr(x), _dptr(wb), int(wb.stride(0)), _dptr(out), w, _stream_ptr(stream)))
        return out

    def edge_index_table_to_host(self, stream=None) -> np.ndarray:
        """The reference's edge_index_table of the prepared batch: COO row of every CSR slot."""
        eid = np.zeros(max(self._E, 1), np.int32)
        _check(self.lib.gnnb_edge_index_table_to_host(self._ws, eid.ctypes.data_as(C.c_void_p), _stream_ptr(stream)))
        return eid[:self._E]

    def aggregate_edges(self, x, edge_term, eps: float = 0.0, out=None, stream=None):
        """GINE aggregate: ``(1 + eps) x_i + sum_j relu(x_j + edge_term[e])``; ``edge_term`` [E, width] in COO order."""
        # (the kernel reads edge_term[eid * width] for every CSR slot: one row per COO edge of the prepared batch)
        self._require_x(x)
        w = int(x.shape[1])
        _require_rows(edge_term, "edge_term", self._E, w, x)
        out = _out(out, self._N, w, x)
        _check(self.lib.gnnb_aggregate_edges(self._ws, _dptr(x), _dptr(edge_term), _dptr(out), w,
                                             float(eps), _stream_ptr(stream)))
        return out

    def aggregate_edges_fused(self, x, edge_attr, w_edge, b_edge, eps: float = 0.0, out=None, stream=None):
        """GINE aggregate with the edge projection inside the kernel (``gnnb_aggregate_edges_fused``, csrc/k_gine.hip):
        ``(1 + eps) x_i + sum_j relu(x_j + w_edge e_ij + b_edge)``; ``edge_attr`` [E, edge_dim <= 16] in COO order, ``w_edge``
        [width, edge_dim] (a column slice of a wider matrix is fine: its row stride is passed on), ``b_edge`` [width]."""
        import torch
        self._require_x(x)
        w = int(x.shape[1])
        _require_strided(w_edge, "w_edge", w, 1)
        ed = int(w_edge.shape[1])
        if not 1 <= ed <= MAX_EDGE_DIM or w_edge.device != x.device:
            raise GnnbError(f"w_edge must be [{w}, 1 .. {MAX_EDGE_DIM}] on {x.device}, got {tuple(w_edge.shape)} on {w_edge.device}")
        _require(b_edge, "b_edge", torch.float32, 1, w)
        if b_edge.device != x.device:
            raise GnnbError(f"b_edge must be on {x.device}")
        ea = self._require_edge_attr(edge_attr, self._E, x, ed)
        out = _out(out, self._N, w, x)
        _check(self.lib.gnnb_aggregate_edges_fused(self._ws, _dptr(x), ea, ed, _dptr(w_edge), int(w_edge.stride(0)) if w > 1 else ed,
                                                   _dptr(b_edge), _dptr(out), w, float(eps), _stream_ptr(stream)))
        return out

    def aggregate_pna_edges(self, p, q, edge_attr, w_edge, b_edge, out=None, stream=None):
        """PNA's aggregate with the edge projection inside the kernel (``gnnb_aggregate_pna_edges``, csrc/k_pna_edge.hip):
        ``max | min | mean | std`` over a row's in-edges of ``q_i + p_j + w_edge e_ij + b_edge`` -> [N, 4 width] as
        ``aggregate("pna", ...)``; ``p`` [N, width], ``q`` [N, width] or None (no destination term), ``edge_attr``
        [E, edge_dim <= 16] in COO order, ``w_edge`` [width, edge_dim] (a column slice of a wider matrix is fine: its row stride is
        passed on), ``b_edge`` [width]."""
        import torch
        self._require_x(p)
        w = int(p.shape[1])
        if q is not None:
            _require_rows(q, "q", self._N, w, p)
        _require_strided(w_edge, "w_edge", w, 1)
        ed = int(w_edge.shape[1])
        if not 1 <= ed <= MAX_EDGE_DIM or w_edge.device != p.device:
            raise GnnbError(f"w_edge must be [{w}, 1 .. {MAX_EDGE_DIM}] on {p.device}, got {tuple(w_edge.shape)} on {w_edge.device}")
        _require(b_edge, "b_edge", torch.float32, 1, w)
        if b_edge.device != p.device:
            raise GnnbError(f"b_edge must be on {p.device}")
        ea = self._require_edge_attr(edge_attr, self._E, p, ed)
        out = _out(out, self._N, 4 * w, p)
        _check(self.lib.gnnb_aggregate_pna_edges(self._ws, _dptr(p), _optr(q), ea, ed, _dptr(w_edge), int(w_edge.stride(0)) if w > 1 else ed,
                                                 _dptr(b_edge), _dptr(out), w, _stream_ptr(stream)))
        return out

    def aggregate_gatv2(self, xl, xr, att, bias=None, skip=None, act: str = "none", heads: int = 1, negative_slope: float = 0.2, out=None,
                        stream=None):
        """One GATv2 layer behind its GEMM (``gnnb_aggregate_gatv2``, csrc/k_gatv2.hip) on the prepared batch of a GCN or GATv2
        model's workspace: ``act(sum_j softmax_j(s_ij) xl_j + bias + skip_i)`` over ``j`` in ``N(i)`` and ``i`` itself, per head,
        ``s_ij = att_h . leaky_relu(xl_j + xr_i)`` -> [N, width].  ``xl``, ``xr`` [N, width] (column slices of a wider matrix are
        fine -- the two halves of one [N, 2 width] GEMM output: their row strides are passed on), ``att`` [width] (or PyG's
        [1, heads, width / heads]), ``bias`` [width] or None, ``skip`` [N, width] or None; ``heads`` 1 .. 8 dividing ``width`` <= 256."""
        import torch
        _require_strided(xl, "xl", self._N, 1)
        w = int(xl.shape[1])
        _require_strided(xr, "xr", self._N, w)
        if int(xr.shape[1]) != w or xr.device != xl.device:
            raise GnnbError(f"xr must be [{self._N}, {w}] on {xl.device}, got {tuple(xr.shape)} on {xr.device}")
        if not isinstance(heads, int) or isinstance(heads, bool) or not 1 <= heads <= MAX_GAT_HEADS:
            raise GnnbError(f"heads must be an int in 1 .. {MAX_GAT_HEADS}, got {heads!r}")
        if w > MAX_GAT_WIDTH or w % heads:
            raise GnnbError(f"width {w}: a GATv2 layer is at most {MAX_GAT_WIDTH} wide and divisible by heads ({heads})")
        if act not in ACT:
            raise GnnbError(f"act must be one of {sorted(ACT)}, got {act!r}")
        if not isinstance(att, torch.Tensor) or att.numel() != w:
            raise GnnbError(f"att must hold {w} values ([{w}] or [1, {heads}, {w // heads}])")
        att = att.reshape(w)
        _require(att, "att", torch.float32, 1, w)
        if bias is not None:
            _require(bias, "bias", torch.float32, 1, w)
        if att.device != xl.device or (bias is not None and bias.device != xl.device):
            raise GnnbError(f"att and bias must be on {xl.device}")
        if skip is not None:
            _require_rows(skip, "skip", self._N, w, xl)
        out = _out(out, self._N, w, xl)
        _check(self.lib.gnnb_aggregate_gatv2(self._ws, _dptr(xl), int(xl.stride(0)) if self._N > 1 else w, _dptr(xr),
                                             int(xr.stride(0)) if self._N > 1 else w, _dptr(att), _optr(bias), _optr(skip), ACT[act], heads,
                                             float(negative_slope), _dptr(out), w, _stream_ptr(stream)))
        return out

    def aggregate_gat(self, xl, s_src, s_dst, bias=None, skip=None, act: str = "none", heads: int = 1, negative_slope: float = 0.2,
                      out=None, stream=None):
        """One GAT (v1) layer behind its GEMM (``gnnb_aggregate_gat``, csrc/k_gat.hip) on the prepared batch of a GCN, GATv2 or GAT
        model's workspace: ``act(sum_j softmax_j(s_ij) xl_j + bias + skip_i)`` over ``j`` in ``N(i)`` and ``i`` itself, per head,
        ``s_ij[h] = leaky_relu(s_src[j, h] + s_dst[i, h])`` -> [N, width].  ``xl`` [N, width], ``s_src`` and ``s_dst`` [N, heads]
        (column slices of a wider matrix are fine -- the blocks of one GEMM output: their row strides are passed on), ``bias``
        [width] or None, ``skip`` [N, width] or None; ``heads`` 1 .. 8 dividing ``width`` <= 256."""
        import torch
        _require_strided(xl, "xl", self._N, 1)
        w = int(xl.shape[1])
        if not isinstance(heads, int) or isinstance(heads, bool) or not 1 <= heads <= MAX_GAT_HEADS:
            raise GnnbError(f"heads must be an int in 1 .. {MAX_GAT_HEADS}, got {heads!r}")
        if w > MAX_GAT_WIDTH or w % heads:
            raise GnnbError(f"width {w}: a GAT layer is at most {MAX_GAT_WIDTH} wide and divisible by heads ({heads})")
        for t, name in ((s_src, "s_src"), (s_dst, "s_dst")):
            _require_strided(t, name, self._N, heads)
            if int(t.shape[1]) != heads or t.device != xl.device:
                raise GnnbError(f"{name} must be [{self._N}, {heads}] on {xl.device}, got {tuple(t.shape)} on {t.device}")
        if act not in ACT:
            raise GnnbError(f"act must be one of {sorted(ACT)}, got {act!r}")
        if bias is not None:
            _require(bias, "bias", torch.float32, 1, w)
            if bias.device != xl.device:
                raise GnnbError(f"bias must be on {xl.device}")
        if skip is not None:
            _require_rows(skip, "skip", self._N, w, xl)
        out = _out(out, self._N, w, xl)

        def ld(t, cols):
            return int(t.stride(0)) if self._N > 1 else cols
        _check(self.lib.gnnb_aggregate_gat(self._ws, _dptr(xl), ld(xl, w), _dptr(s_src), ld(s_src, heads), _dptr(s_dst), ld(s_dst, heads),
                                           _optr(bias), _optr(skip), ACT[act], heads, float(negative_slope), _dptr(out), w,
                                           _stream_ptr(stream)))
        return out

    def aggregate_transformer(self, q, k, v, root=None, skip=None, act: str = "none", heads: int = 1, scale: Optional[float] = None,
                              out=None, stream=None):
        """One TransformerConv layer behind its GEMM (``gnnb_aggregate_transformer``, csrc/k_transformer.hip) on the prepared batch
        of a workspace whose tables keep explicit self loops (any but a GCN or GATv2 model's, which is refused):
        ``act((sum_j softmax_j(s_ij) v_j + root_i) + skip_i)`` over ``j`` in ``N(i)`` as the batch holds it, per head,
        ``s_ij = (q_i . k_j) * scale`` -> [N, width].  ``q``, ``k``, ``v`` [N, width] and ``root`` [N, width] or None (column
        slices of a wider matrix are fine -- the four blocks of one [N, 4 width] GEMM output: their row strides are passed on),
        ``skip`` [N, width] contiguous or None; ``heads`` 1 .. 8 dividing ``width`` <= 256; ``scale=None``: ``1 / sqrt(width /
        heads)``."""
        _require_strided(q, "q", self._N, 1)
        w = int(q.shape[1])
        for name, t in (("k", k), ("v", v), ("root", root)):
            if t is None and name == "root":
                continue
            _require_strided(t, name, self._N, w)
            if int(t.shape[1]) != w or t.device != q.device:
                raise GnnbError(f"{name} must be [{self._N}, {w}] on {q.device}, got {tuple(t.shape)} on {t.device}")
        if not isinstance(heads, int) or isinstance(heads, bool) or not 1 <= heads <= MAX_TRANSFORMER_HEADS:
            raise GnnbError(f"heads must be an int in 1 .. {MAX_TRANSFORMER_HEADS}, got {heads!r}")
        if w > MAX_TRANSFORMER_WIDTH or w % heads:
            raise GnnbError(f"width {w}: a TransformerConv layer is at most {MAX_TRANSFORMER_WIDTH} wide and divisible by heads ({heads})")
        if act not in ACT:
            raise GnnbError(f"act must be one of {sorted(ACT)}, got {act!r}")
        if scale is None:
            scale = float(np.float32(1.0) / np.sqrt(np.float32(w // heads)))  # (in fp32, as the layer's own)
        if not np.isfinite(scale):
            raise GnnbError(f"scale must be finite, got {scale!r}")
        if skip is not None:
            _require_rows(skip, "skip", self._N, w, q)
        out = _out(out, self._N, w, q)
        ld = lambda t: int(t.stride(0)) if self._N > 1 else w  # noqa: E731  (one row: any stride describes it)
        _check(self.lib.gnnb_aggregate_transformer(self._ws, _dptr(q), ld(q), _dptr(k), ld(k), _dptr(v), ld(v), _optr(root),
                                                   ld(root) if root is not None else w, _optr(skip), ACT[act], heads, float(scale),
                                                   _dptr(out), w, _stream_ptr(stream)))
        return out

    def aggregate_resgated(self, k, q, v, root=None, skip=None, act: str = "none", out=None, stream=None):
        """One ResGatedGraphConv layer behind its GEMM (``gnnb_aggregate_resgated``, csrc/k_resgated.hip) on the prepared batch of a
        workspace whose tables keep explicit self loops (any but a GCN or GATv2 model's, which is refused):
        ``act((sum_j sigmoid(k_i + q_j) * v_j + root_i) + skip_i)`` over ``j`` in ``N(i)`` as the batch holds it, the gate per
        column -> [N, width].  ``k``, ``q``, ``v`` [N, width] and ``root`` [N, width] or None (column slices of a wider matrix are
        fine -- the four blocks of one [N, 4 width] GEMM output: their row strides are passed on), ``skip`` [N, width] contiguous
        or None; ``width`` <= 256."""
        _require_strided(k, "k", self._N, 1)
        w = int(k.shape[1])
        for name, t in (("q", q), ("v", v), ("root", root)):
            if t is None and name == "root":
                continue
            _require_strided(t, name, self._N, w)
            if int(t.shape[1]) != w or t.device != k.device:
                raise GnnbError(f"{name} must be [{self._N}, {w}] on {k.device}, got {tuple(t.shape)} on {t.device}")
        if w > MAX_RESGATED_WIDTH:
            raise GnnbError(f"width {w}: a ResGatedGraphConv layer is at most {MAX_RESGATED_WIDTH} wide")
        if act not in ACT:
            raise GnnbError(f"act must be one of {sorted(ACT)}, got {act!r}")
        if skip is not None:
            _require_rows(skip, "skip", self._N, w, k)
        out = _out(out, self._N, w, k)
        ld = lambda t: int(t.stride(0)) if self._N > 1 else w  # noqa: E731  (one row: any stride describes it)
        _check(self.lib.gnnb_aggregate_resgated(self._ws, _dptr(k), ld(k), _dptr(q), ld(q), _dptr(v), ld(v), _optr(root),
                                                ld(root) if root is not None else w, _optr(skip), ACT[act], _dptr(out), w,
                                                _stream_ptr(stream)))
        return out

    def aggregate_ggnn(self, p, gh, h, b_ih=None, skip=None, act: str = "none", out=None, stream=None):
        """One GatedGraphConv step behind its GEMM (``gnnb_aggregate_ggnn``, csrc/k_ggnn.hip) on the prepared batch of a workspace
        whose tables keep explicit self loops (any but a GCN, GATv2 or GAT model's, which is refused): with ``acc = sum_j p_j`` over
        ``j`` in ``N(i)`` as the batch holds it and ``gi = acc + b_ih``, per column ``r = sigmoid(gi_r + gh_r)``,
        ``z = sigmoid(gi_z + gh_z)``, ``n = tanh(gi_n + r * gh_n)`` and ``act(n + z * (h - n) + skip)`` -> [N, width].  ``p`` and
        ``gh`` [N, 3 width] in column blocks r | z | n (column slices of a wider matrix are fine -- the two halves of one
        [N, 6 width] GEMM output: their row strides are passed on); ``h`` [N, h_width <= width], its missing columns taken as 0;
        ``b_ih`` [3 width] contiguous or None; ``skip`` [N, width] contiguous or None; ``width`` <= 256."""
        import torch
        _require_strided(p, "p", self._N, 3)
        if int(p.shape[1]) % 3:
            raise GnnbError(f"p must be [{self._N}, 3 width], got {tuple(p.shape)}")
        w = int(p.shape[1]) // 3
        _require_strided(gh, "gh", self._N, 3 * w)
        _require_strided(h, "h", self._N, 1)
        hw = int(h.shape[1])
        if int(gh.shape[1]) != 3 * w or gh.device != p.device or h.device != p.device or hw > w:
            raise GnnbError(f"gh must be [{self._N}, {3 * w}] and h [{self._N}, <= {w}] on {p.device}, got {tuple(gh.shape)} on {gh.device} "
                            f"and {tuple(h.shape)} on {h.device}")
        if w > MAX_GGNN_WIDTH:
            raise GnnbError(f"width {w}: a GatedGraphConv layer is at most {MAX_GGNN_WIDTH} wide")
        if act not in ACT:
            raise GnnbError(f"act must be one of {sorted(ACT)}, got {act!r}")
        if b_ih is not None and (not isinstance(b_ih, torch.Tensor) or b_ih.dtype != torch.float32 or b_ih.device != p.device or
                                 b_ih.dim() != 1 or b_ih.numel() != 3 * w or not b_ih.is_contiguous()):
            raise GnnbError(f"b_ih must be a contiguous float32 [{3 * w}] on {p.device}")
        if skip is not None:
            _require_rows(skip, "skip", self._N, w, p)
        out = _out(out, self._N, w, p)
        ld = lambda t: int(t.stride(0)) if self._N > 1 else int(t.shape[1])  # noqa: E731  (one row: any stride describes it)
        _check(self.lib.gnnb_aggregate_ggnn(self._ws, _dptr(p), ld(p), _dptr(gh), ld(gh), _dptr(h), ld(h), hw, _optr(b_ih), _optr(skip),
                                            ACT[act], _dptr(out), w, _stream_ptr(stream)))
        return out

    def rgcn_slots(self, edge_type, relations: int, stream=None):
        """The slot records of the prepared batch (``gnnb_rgcn_slots``, csrc/k_rgcn.hip) on a workspace whose tables keep explicit
        self loops: ``edge_type`` [E] int32 in COO row order -> an int32 tensor [E, 2], row ``s`` = (relation, the bits of the
        float32 ``1 / |N_rel(i)|``) of CSR slot ``s`` -- ``rec[:, 1].view(torch.float32)`` gives the weights.  A type outside
        ``[0, relations)`` gives (0, 0.0) and flags the batch (``check()``: flag 0x100).  What ``aggregate_rgcn`` takes."""
        import torch
        if not isinstance(relations, int) or isinstance(relations, bool) or not 1 <= relations <= MAX_RGCN_RELATIONS:
            raise GnnbError(f"relations must be an int in 1 .. {MAX_RGCN_RELATIONS}, got {relations!r}")
        if edge_type is None and self._E:
            raise GnnbError(f"edge_type is required: the batch has {self._E} edges")
        if edge_type is not None:
            _require(edge_type, "edge_type", torch.int32, 1)
            if edge_type.numel() != self._E:
                raise GnnbError(f"edge_type must be [{self._E}], got {tuple(edge_type.shape)}")
        dev = edge_type.device if edge_type is not None else torch.device("cuda")
        # (zeros: a slot no row owns -- none on the workspaces this entry accepts -- would otherwise hold what the allocator left)
        rec = torch.zeros((self._E, 2), dtype=torch.int32, device=dev)
        _check(self.lib.gnnb_rgcn_slots(self._ws, _optr(edge_type) if self._E else None, relations, _dptr(rec) if self._E else None,
                                        _stream_ptr(stream)))
        return rec

    def aggregate_rgcn(self, rec, p, relations: int, root=None, skip=None, act: str = "none", out=None, stream=None):
        """One RGCNConv layer behind its GEMM (``gnnb_aggregate_rgcn``, csrc/k_rgcn.hip) on the prepared batch of a workspace whose
        tables keep explicit self loops: ``act((sum_s w_s * p[col_s, rel_s * width + c] + root) + skip)`` -> [N, width] over the
        row's slots ``s`` with ``rec`` (``rgcn_slots``) naming each slot's relation block and mean weight.  ``p`` [N, >= relations
        * width] with ``width = p.shape[1] // relations`` and ``root`` [N, width] or None may be column slices of one wider matrix
        (the blocks of one [N, (relations + 1) width] GEMM output: their row strides are passed on); ``skip`` [N, width] contiguous
        or None; ``width`` <= 256."""
        import torch
        if not isinstance(relations, int) or isinstance(relations, bool) or not 1 <= relations <= MAX_RGCN_RELATIONS:
            raise GnnbError(f"relations must be an int in 1 .. {MAX_RGCN_RELATIONS}, got {relations!r}")
        _require_strided(p, "p", self._N, relations)
        if int(p.shape[1]) % relations:
            raise GnnbError(f"p must be [{self._N}, relations * width], got {tuple(p.shape)} for {relations} relations")
        w = int(p.shape[1]) // relations
        if w > MAX_RGCN_WIDTH:
            raise GnnbError(f"width {w}: an RGCNConv layer is at most {MAX_RGCN_WIDTH} wide")
        _require(rec, "rec", torch.int32, 2, 2)
        if int(rec.shape[0]) != self._E or rec.device != p.device or rec.data_ptr() % 8:
            raise GnnbError(f"rec must be the [{self._E}, 2] int32 records of rgcn_slots on {p.device}, 8-byte aligned; got "
                            f"{tuple(rec.shape)} on {rec.device}")
        if root is not None:
            _require_strided(root, "root", self._N, w)
            if int(root.shape[1]) != w or root.device != p.device:
                raise GnnbError(f"root must be [{self._N}, {w}] on {p.device}, got {tuple(root.shape)} on {root.device}")
        if act not in ACT:
            raise GnnbError(f"act must be one of {sorted(ACT)}, got {act!r}")
        if skip is not None:
            _require_rows(skip, "skip", self._N, w, p)
        out = _out(out, self._N, w, p)
        ld = lambda t: int(t.stride(0)) if self._N > 1 else int(t.shape[1])  # noqa: E731  (one row: any stride describes it)
        _check(self.lib.gnnb_aggregate_rgcn(self._ws, _dptr(rec) if self._E else None, _dptr(p), ld(p), relations, _optr(root),
                                            ld(root) if root is not None else 0, _optr(skip), ACT[act], _dptr(out), w, _stream_ptr(stream)))
        return out

    def aggregate_resgated_edges(self, k, q, v, edge_attr, w_gate, w_value, root=None, skip=None, act: str = "none", out=None, stream=None):
        """One ResGatedGraphConv layer with edge features behind its GEMM (``gnnb_aggregate_resgated_edges``,
        csrc/k_resgated_edge.hip) on the prepared batch of a workspace whose tables keep explicit self loops:
        ``aggregate_resgated`` with the gate ``sigmoid((k_i + q_j) + w_gate e_ij)`` and the value ``v_j + w_value e_ij``, per
        column.  ``k``, ``q``, ``v``, ``root``, ``skip`` as there; ``edge_attr`` [E, edge_dim <= 16] in COO order; ``w_gate`` (the
        layer passes ``W_ke + W_qe``; the entry computes what it is given) and ``w_value`` [width, edge_dim], separate operands;
        column slices of wider matrices are fine for them too: their row strides are passed on."""
        _require_strided(k, "k", self._N, 1)
        w = int(k.shape[1])
        for name, t in (("q", q), ("v", v), ("root", root)):
            if t is None and name == "root":
                continue
            _require_strided(t, name, self._N, w)
            if int(t.shape[1]) != w or t.device != k.device:
                raise GnnbError(f"{name} must be [{self._N}, {w}] on {k.device}, got {tuple(t.shape)} on {t.device}")
        if w > MAX_RESGATED_WIDTH:
            raise GnnbError(f"width {w}: a ResGatedGraphConv layer is at most {MAX_RESGATED_WIDTH} wide")
        if act not in ACT:
            raise GnnbError(f"act must be one of {sorted(ACT)}, got {act!r}")
        if skip is not None:
            _require_rows(skip, "skip", self._N, w, k)
        _require_strided(w_gate, "w_gate", w, 1)
        ed = int(w_gate.shape[1])
        if not 1 <= ed <= MAX_EDGE_DIM or w_gate.device != k.device:
            raise GnnbError(f"w_gate must be [{w}, 1 .. {MAX_EDGE_DIM}] on {k.device}, got {tuple(w_gate.shape)} on {w_gate.device}")
        _require_strided(w_value, "w_value", w, ed)
        if int(w_value.shape[1]) != ed or w_value.device != k.device:
            raise GnnbError(f"w_value must be [{w}, {ed}] on {k.device}, got {tuple(w_value.shape)} on {w_value.device}")
        ea = self._require_edge_attr(edge_attr, self._E, k, ed)
        out = _out(out, self._N, w, k)
        ld = lambda t: int(t.stride(0)) if self._N > 1 else w  # noqa: E731  (one row: any stride describes it)
        ldw = lambda t: int(t.stride(0)) if w > 1 else ed  # noqa: E731
        _check(self.lib.gnnb_aggregate_resgated_edges(self._ws, _dptr(k), ld(k), _dptr(q), ld(q), _dptr(v), ld(v), _optr(root),
                                                      ld(root) if root is not None else w, _optr(skip), ACT[act], ea, ed, _dptr(w_gate),
                                                      ldw(w_gate), _dptr(w_value), ldw(w_value), _dptr(out), w, _stream_ptr(stream)))
        return out

    def aggregate_transformer_edges(self, q, k, v, qe, edge_attr, w_edge, root=None, skip=None, act: str = "none", heads: int = 1,
                                    scale: Optional[float] = None, out=None, stream=None):
        """One TransformerConv layer with edge features behind its GEMM (``gnnb_aggregate_transformer_edges``,
        csrc/k_transformer_edge.hip) on the prepared batch of a workspace whose tables keep explicit self loops:
        ``aggregate_transformer`` with ``s_ij = (q_i . k_j + qe_i[h] . e_ij) * scale`` and ``w_edge (sum_j softmax_j e_ij)`` added to
        the weighted sum of the value rows, per head.  ``q``, ``k``, ``v``, ``root``, ``skip``, ``heads``, ``scale`` as there;
        ``qe`` [N, heads * edge_dim] (the layer passes ``W_e[h]^T q_i[h]``; the entry computes what it is given), ``edge_attr``
        [E, edge_dim <= 16] in COO order, ``w_edge`` [width, edge_dim]; column slices of wider matrices are fine for ``qe`` and
        ``w_edge`` too: their row strides are passed on."""
        _require_strided(q, "q", self._N, 1)
        w = int(q.shape[1])
        for name, t in (("k", k), ("v", v), ("root", root)):
            if t is None and name == "root":
                continue
            _require_strided(t, name, self._N, w)
            if int(t.shape[1]) != w or t.device != q.device:
                raise GnnbError(f"{name} must be [{self._N}, {w}] on {q.device}, got {tuple(t.shape)} on {t.device}")
        if not isinstance(heads, int) or isinstance(heads, bool) or not 1 <= heads <= MAX_TRANSFORMER_HEADS:
            raise GnnbError(f"heads must be an int in 1 .. {MAX_TRANSFORMER_HEADS}, got {heads!r}")
        if w > MAX_TRANSFORMER_WIDTH or w % heads:
            raise GnnbError(f"width {w}: a TransformerConv layer is at most {MAX_TRANSFORMER_WIDTH} wide and divisible by heads ({heads})")
        if act not in ACT:
            raise GnnbError(f"act must be one of {sorted(ACT)}, got {act!r}")
        if scale is None:
            scale = float(np.float32(1.0) / np.sqrt(np.float32(w // heads)))  # (in fp32, as the layer's own)
        if not np.isfinite(scale):
            raise GnnbError(f"scale must be finite, got {scale!r}")
        if skip is not None:
            _require_rows(skip, "skip", self._N, w, q)
        _require_strided(w_edge, "w_edge", w, 1)
        ed = int(w_edge.shape[1])
        if not 1 <= ed <= MAX_EDGE_DIM or w_edge.device != q.device:
            raise GnnbError(f"w_edge must be [{w}, 1 .. {MAX_EDGE_DIM}] on {q.device}, got {tuple(w_edge.shape)} on {w_edge.device}")
        _require_strided(qe, "qe", self._N, heads * ed)
        if int(qe.shape[1]) != heads * ed or qe.device != q.device:
            raise GnnbError(f"qe must be [{self._N}, heads * edge_dim = {heads * ed}] on {q.device}, got {tuple(qe.shape)} on {qe.device}")
        ea = self._require_edge_attr(edge_attr, self._E, q, ed)
        out = _out(out, self._N, w, q)
        ld = lambda t, cols: int(t.stride(0)) if self._N > 1 else cols  # noqa: E731  (one row: any stride describes it)
        _check(self.lib.gnnb_aggregate_transformer_edges(self._ws, _dptr(q), ld(q, w), _dptr(k), ld(k, w), _dptr(v), ld(v, w), _dptr(qe),
                                                         ld(qe, heads * ed), _optr(root), ld(root, w) if root is not None else w, _optr(skip),
                                                         ACT[act], heads, float(scale), ea, ed, _dptr(w_edge),
                                                         int(w_edge.stride(0)) if w > 1 else ed, _dptr(out), w, _stream_ptr(stream)))
        return out

    def aggregate_gatv2_edges(self, xl, xr, att, edge_attr, w_edge, bias=None, skip=None, act: str = "none", heads: int = 1,
                              negative_slope: float = 0.2, out=None, stream=None):
        """One GATv2 layer with edge features behind its GEMM (``gnnb_aggregate_gatv2_edges``, csrc/k_gatv2_edge.hip) on the prepared
        batch of a GCN, GATv2 or GATv2E model's workspace: ``aggregate_gatv2`` with ``s_ij = att_h . leaky_relu(xl_j + xr_i +
        w_edge e_ij)``; the self term's ``e_ii`` is the mean of the row's attribute rows.  ``xl``, ``xr``, ``att``, ``bias``, ``skip``,
        ``heads`` as there; ``edge_attr`` [E, edge_dim <= 16] in COO order, ``w_edge`` [width, edge_dim] (a column slice of a wider
        matrix is fine: its row stride is passed on)."""
        import torch
        _require_strided(xl, "xl", self._N, 1)
        w = int(xl.shape[1])
        _require_strided(xr, "xr", self._N, w)
        if int(xr.shape[1]) != w or xr.device != xl.device:
            raise GnnbError(f"xr must be [{self._N}, {w}] on {xl.device}, got {tuple(xr.shape)} on {xr.device}")
        if not isinstance(heads, int) or isinstance(heads, bool) or not 1 <= heads <= MAX_GAT_HEADS:
            raise GnnbError(f"heads must be an int in 1 .. {MAX_GAT_HEADS}, got {heads!r}")
        if w > MAX_GAT_WIDTH or w % heads:
            raise GnnbError(f"width {w}: a GATv2 layer is at most {MAX_GAT_WIDTH} wide and divisible by heads ({heads})")
        if act not in ACT:
            raise GnnbError(f"act must be one of {sorted(ACT)}, got {act!r}")
        if not isinstance(att, torch.Tensor) or att.numel() != w:
            raise GnnbError(f"att must hold {w} values ([{w}] or [1, {heads}, {w // heads}])")
        att = att.reshape(w)
        _require(att, "att", torch.float32, 1, w)
        if bias is not None:
            _require(bias, "bias", torch.float32, 1, w)
        if att.device != xl.device or (bias is not None and bias.device != xl.device):
            raise GnnbError(f"att and bias must be on {xl.device}")
        if skip is not None:
            _require_rows(skip, "skip", self._N, w, xl)
        _require_strided(w_edge, "w_edge", w, 1)
        ed = int(w_edge.shape[1])
        if not 1 <= ed <= MAX_EDGE_DIM or w_edge.device != xl.device:
            raise GnnbError(f"w_edge must be [{w}, 1 .. {MAX_EDGE_DIM}] on {xl.device}, got {tuple(w_edge.shape)} on {w_edge.device}")
        ea = self._require_edge_attr(edge_attr, self._E, xl, ed)
        out = _out(out, self._N, w, xl)
        _check(self.lib.gnnb_aggregate_gatv2_edges(self._ws, _dptr(xl), int(xl.stride(0)) if self._N > 1 else w, _dptr(xr),
                                                   int(xr.stride(0)) if self._N > 1 else w, _dptr(att), _optr(bias), _optr(skip), ACT[act],
                                                   heads, float(negative_slope), ea, ed, _dptr(w_edge), int(w_edge.stride(0)) if w > 1 else ed,
                                                   _dptr(out), w, _stream_ptr(stream)))
        return out

    def aggregate_gat_edges(self, xl, s_src, s_dst, edge_attr, a_edge, bias=None, skip=None, act: str = "none", heads: int = 1,
                            negative_slope: float = 0.2, out=None, stream=None):
        """One GAT (v1) layer with edge features behind its GEMM (``gnnb_aggregate_gat_edges``, csrc/k_gat_edge.hip) on the prepared
        batch of a GCN, GAT or GATv2 model's workspace: ``aggregate_gat`` with ``s_ij[h] = leaky_relu(s_src[j, h] + s_dst[i, h] +
        a_edge[h] . e_ij)``; the self term's edge term is the mean of the row's.  ``xl``, ``s_src``, ``s_dst``, ``bias``, ``skip``,
        ``heads`` as there; ``edge_attr`` [E, edge_dim <= 16] in COO order, ``a_edge`` [heads, edge_dim]: ``att_edge`` folded into
        ``lin_edge`` (a column slice of a wider matrix is fine: its row stride is passed on)."""
        import torch
        _require_strided(xl, "xl", self._N, 1)
        w = int(xl.shape[1])
        if not isinstance(heads, int) or isinstance(heads, bool) or not 1 <= heads <= MAX_GAT_HEADS:
            raise GnnbError(f"heads must be an int in 1 .. {MAX_GAT_HEADS}, got {heads!r}")
        if w > MAX_GAT_WIDTH or w % heads:
            raise GnnbError(f"width {w}: a GAT layer is at most {MAX_GAT_WIDTH} wide and divisible by heads ({heads})")
        for t, name in ((s_src, "s_src"), (s_dst, "s_dst")):
            _require_strided(t, name, self._N, heads)
            if int(t.shape[1]) != heads or t.device != xl.device:
                raise GnnbError(f"{name} must be [{self._N}, {heads}] on {xl.device}, got {tuple(t.shape)} on {t.device}")
        if act not in ACT:
            raise GnnbError(f"act must be one of {sorted(ACT)}, got {act!r}")
        if bias is not None:
            _require(bias, "bias", torch.float32, 1, w)
            if bias.device != xl.device:
                raise GnnbError(f"bias must be on {xl.device}")
        if skip is not None:
            _require_rows(skip, "skip", self._N, w, xl)
        _require_strided(a_edge, "a_edge", heads, 1)
        ed = int(a_edge.shape[1])
        if not 1 <= ed <= MAX_EDGE_DIM or a_edge.device != xl.device:
            raise GnnbError(f"a_edge must be [{heads}, 1 .. {MAX_EDGE_DIM}] on {xl.device}, got {tuple(a_edge.shape)} on {a_edge.device}")
        ea = self._require_edge_attr(edge_attr, self._E, xl, ed)
        out = _out(out, self._N, w, xl)

        def ld(t, cols):
            return int(t.stride(0)) if self._N > 1 else cols
        _check(self.lib.gnnb_aggregate_gat_edges(self._ws, _dptr(xl), ld(xl, w), _dptr(s_src), ld(s_src, heads), _dptr(s_dst),
                                                 ld(s_dst, heads), _optr(bias), _optr(skip), ACT[act], heads, float(negative_slope), ea, ed,
                                                 _dptr(a_edge), int(a_edge.stride(0)) if heads > 1 else ed, _dptr(out), w,
                                                 _stream_ptr(stream)))
        return out

    def gine_conv(self, x, edge_attr, w_edge, b_edge, w0, b0, w1, b1, eps: float = 0.0, stream=None):
        """One GINEConv layer on the prepared batch (reference gine_conv, gnn_builder_lib.h:1640-1742):
        edge projection (GEMM) -> GINE aggregate -> Linear -> ReLU -> Linear."""
        pe = linear([(edge_attr, None)], w_edge, b_edge, stream=stream)
        z = self.aggregate_edges(x, pe, eps=eps, stream=stream)
        h = linear([(z, None)], w0, b0, act="relu", stream=stream)
        return linear([(h, None)], w1, b1, stream=stream)

    def aggregate_timed(self, kind: str, xs, outs, iters: int, self_term=None, eps: float = 0.0, stream=None) -> float:
        """Mean microseconds per launch over ``iters`` back-to-back launches issued from C,
        rotating over the (x, out) buffer pairs; HIP events on the launch stream."""
        n = len(xs)
        if n < 1 or len(outs) != n or any(out is None for out in outs):
            raise GnnbError(f"aggregate_timed takes as many outs as xs, at least one; got {n} xs and {len(outs)} outs")
        w = None  # (of the first x, every other as wide)
        for x, out in zip(xs, outs):
            w, _ = self._aggregate_operands(kind, x, self_term, out, w)
        xa = (C.c_void_p * n)(*[_dptr(t) for t in xs])
        oa = (C.c_void_p * n)(*[_dptr(t) for t in outs])
        us = C.c_float()
        _check(self.lib.gnnb_aggregate_timed(self._ws, AGG[kind], xa, _optr(self_term), oa, n, w, float(eps), int(iters),
                                             _stream_ptr(stream), C.byref(us)))
        return float(us.value)

    def gcn_stack_timed(self, x, iters: int, stream=None) -> float:
        """Mean microseconds per launch of the fused GCN stack + pooling kernel on the prepared
        batch (``graph_prep`` first); HIP events on the launch stream.  Raises if that path is not eligible."""
        self._require_x(x, int(self.desc.in_dim))
        us = C.c_float()
        _check(self.lib.gnnb_gcn_stack_timed(self._model, self._ws, _dptr(x), int(iters), _stream_ptr(stream),
                                             C.byref(us)))
        return float(us.value)

    def global_pool(self, x, pools: Sequence[str], out=None, stream=None):
        # (gnnb_global_pool reads x up to row node_ptr[B] of the prepared batch)
        self._require_x(x)
        d = int(x.shape[1])
        out = _out(out, self._B, len(pools) * d, x)
        arr = (C.c_int32 * len(pools))(*[POOL[p] for p in pools])
        _check(self.lib.gnnb_global_pool(self._ws, _dptr(x), d, arr, len(pools), _dptr(out), _stream_ptr(stream)))
        return out


def _linear_operands(segments, weight, bias, skip, out):
    """Operands of ``gnnb_linear`` against what the header says it reads: every A_s [M, K_s] with its row stride passed as lda,
    rowscale [M], weight [N, >= sum K_s] with its row stride passed as ldw, bias [N], skip and out [M, N] contiguous.  M = 0 is
    legal (empty tensors).  Returns (M, N, out)."""
    import torch
    M = None  # (of the first segment; every other has as many rows)
    for i, (a, rs) in enumerate(segments):
        _require_strided(a, f"A of segment {i}", M)
        M = int(a.shape[0])
        if rs is not None:
            _require(rs, f"rowscale of segment {i}", torch.float32, 1, M)
    _require_strided(weight, "weight", None, sum(int(a.shape[1]) for a, _ in segments))
    N = int(weight.shape[0])
    if bias is not None:
        _require(bias, "bias", torch.float32, 1, N)
    if skip is not None:
        _require_rows(skip, "skip", M, N, weight)
    return M, N, _out(out, M, N, weight)


def linear(segments, weight, bias=None, skip=None, act: str = "none", out=None, stream=None):
    """``segments``: list of (A [M, K_s] CUDA tensor, rowscale [M] or None).  weight [N, sum K_s]."""
    lib = load_library(require_gpu=True)
    M, N, out = _linear_operands(segments, weight, bias, skip, out)
    segs = (GemmSeg * len(segments))()
    for i, (a, rs) in enumerate(segments):
        segs[i].a_dev = _dptr(a)
        segs[i].rowscale_dev = _optr(rs)
        segs[i].lda = int(a.stride(0))
        segs[i].k = int(a.shape[1])
    _check(lib.gnnb_linear(segs, len(segments), _dptr(weight), int(weight.stride(0)), _optr(bias), _optr(skip), _dptr(out),
                           M, N, ACT[act], _stream_ptr(stream)))
    return out


def stream_k_guard(stream=None) -> None:
    """Diagnostics: the standalone ``linear``'s stream-K scratch of (current device, stream) -- counters zero, guard whole."""
    _check(load_library().gnnb_debug_stream_k_guard(None, _stream_ptr(stream)))


def linear_timed(a, weight, bias, out, act: str, iters: int, stream=None) -> float:
    """Mean microseconds per launch of one ``gnnb_linear`` configuration, launched from C."""
    lib = load_library(require_gpu=True)
    M, N, out = _linear_operands([(a, None)], weight, bias, None, out)
    us = C.c_float()
    _check(lib.gnnb_linear_timed(_dptr(a), int(a.stride(0)), int(a.shape[1]), _dptr(weight), int(weight.stride(0)),
                                 _optr(bias), _dptr(out), M, N, ACT[act], int(iters), _stream_ptr(stream), C.byref(us)))
    return float(us.value)


class HipTimer:
    """hipEvent pair on an explicit stream (bench.py times kernels on the stream they run on)."""

    def __init__(self):
        self.lib = None
        self.a, self.b = C.c_void_p(), C.c_void_p()
        self.lib = load_library(require_gpu=True)
        _check(self.lib.gnnb_event_create(C.byref(self.a)))
        _check(self.lib.gnnb_event_create(C.byref(self.b)))

    def start(self, stream=None):
        _check(self.lib.gnnb_event_record(self.a, _stream_ptr(stream)))

    def stop(self, stream=None):
        _check(self.lib.gnnb_event_record(self.b, _stream_ptr(stream)))

    def elapsed_ms(self) -> float:
        ms = C.c_float()
        _check(self.lib.gnnb_event_elapsed_ms(self.a, self.b, C.byref(ms)))
        return float(ms.value)

    def __del__(self):
        try:
            self.lib.gnnb_event_destroy(self.a)
            self.lib.gnnb_event_destroy(self.b)
        except Exception:
            pass
