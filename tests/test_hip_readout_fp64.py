"""The readout's boundaries against float64 with the fp32-class budget of ref64: the seams of the pooling row walk and every
form of the MLP head at the smallest shapes that reach them.

Row walk (k_global_pool, and phase 1 of k_pool_mlp): the first row seeds sum and max, then blocks of eight (k_pool_mlp only)
and four rows, then the tail -- graphs of 0, 1, 2, 4, 5, 8, 9, 12, 13 and 17 nodes sit on every seam.  ``gnnb_global_pool`` runs
k_global_pool<4> (widths that are multiples of 4) or <1> (width 7); add and max are compared BIT FOR BIT with a sequential fp32
accumulation in row order, which is what the kernel computes (mean is left to the budget: its division is not pinned).

Heads, on a 2-layer GCN (in_dim 11, hidden 64, promise 29) whose graphs have the same ten sizes, through five forms:

  ========  ====================================================  ================================================
  form      options                                               kernel
  ========  ====================================================  ================================================
  paired    head_small = 1, head_pairs = 1                        k_gcn2_zf, then k_head_small (operands in pairs)
  four      head_small = 1, head_pairs = 0                        k_gcn2_zf, then k_head_small (four at once)
  lds       head_small = 0                                        k_gcn2_zf, then k_pool_mlp's pre-pooled form
  from_x    fuse_gcn2 = 0, fuse_zf = 0, head_split = 0            layer by layer, then k_pool_mlp pooling x itself
  zf_head   zf_head = 1                                           k_gcn2_zf with the head as its tail
  ========  ====================================================  ================================================

A hidden width of 33 is no multiple of 4: k_head_small and the tail of k_gcn2_zf decline it, and ``paired``, ``four`` and
``zf_head`` end in k_pool_mlp's pre-pooled form (its scalar-operand path) as ``lds`` does."""
import functools
import itertools

import numpy as np
import pytest

import ref64 as R
from gnnbuilder_amd import runtime
from gnnbuilder_amd.batching import pack_graphs
from helpers import make_model, to_dev
from test_hip_fp64 import _library, check, dev_, hip, references  # noqa: F401  (_library: module fixture)
from test_hip_stage_fp64 import _library as _stage_library, on_device, record  # noqa: F401  (record reports through that module)

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 2, 4, 5, 8, 9, 12, 13, 17)  # seed | + tail | four-deep | + tail | eight-deep | + tail | 8 + 4 (+ tail) | 8 + 8


def ring(n, fin, rng):
    """``n`` nodes with uniform(-1, 1) features on a directed ring (no edge below two nodes)."""
    coo = np.stack([np.arange(n), (np.arange(n) + 1) % n], 1) if n > 1 else np.zeros((0, 2))
    return rng.uniform(-1, 1, (n, fin)).astype(np.float32), coo.astype(np.int32)


# --------------------------------------------------------------------------- the row walk
def _sequential32(x, batch, op):
    """Per graph, rows combined one after the other in float32 (``np.add.accumulate``: no pairwise summation); no rows: 0."""
    out = np.zeros((batch.num_graphs, x.shape[1]), np.float32)
    for g in range(batch.num_graphs):
        rows = x[batch.node_ptr[g]:batch.node_ptr[g + 1]]
        if len(rows):
            out[g] = op.accumulate(rows, axis=0, dtype=np.float32)[-1]
    return out


@pytest.mark.parametrize("d", [4, 20, 64, 7])
def test_row_walk_seams(d):
    rng = np.random.default_rng(d)
    batch = pack_graphs([ring(n, d, rng) for n in SIZES])
    x = batch.x - 0.25  # (most maxima of the short graphs negative: a max that starts at 0 shows)
    cm = runtime.CompiledModel.from_model(make_model("gin", in_dim=4, hidden=8, layers=1, out_dim=8, task_out=2, mlp_layers=1),
                                          batch.num_graphs, batch.num_nodes, max(batch.num_edges, 1))
    _, coo, nptr, eptr = to_dev(batch, dev_())
    cm.graph_prep(coo, nptr, eptr, batch.num_nodes)
    xd = on_device(x)
    exact = {"add": _sequential32(x, batch, np.add), "max": _sequential32(x, batch, np.maximum)}
    base = dict(exact, mean=exact["add"] / np.maximum(np.diff(batch.node_ptr), 1)[:, None].astype(np.float32))
    for pools in (("add", "mean", "max"), ("add",), ("mean",), ("max",)):
        got = cm.global_pool(xd, list(pools)).cpu().numpy()
        cm.check()
        record("readout row_walk", got, R.pool64(x, batch, pools), np.concatenate([base[p] for p in pools], 1))
        assert not got[SIZES.index(0)].any(), "the empty graph pools to 0"
        for i, p in enumerate(pools):
            if p in exact:
                assert np.array_equal(got[:, i * d:(i + 1) * d], exact[p]), (pools, p)
    cm.close()


# --------------------------------------------------------------------------- the heads
FORMS = {"paired": dict(head_small=1, head_pairs=1), "four": dict(head_small=1, head_pairs=0), "lds": dict(head_small=0),
         "from_x": dict(fuse_gcn2=0, fuse_zf=0, head_split=0), "zf_head": dict(zf_head=1)}
# Forms whose outputs agree bit for bit in every case here: operands in pairs or four at once feed the same four accumulator
# chains in the same order (head_small_run's claim).  No other pair does throughout: ``lds`` equals them in 13 of the 15 cases
# (not with eight linears at B = 16, 17), ``zf_head`` splits layer 0's k range over its groups, ``from_x`` pools another stack's rows.
BITWISE = (("paired", "four"),)
HEADS = {  # pools, mlp_hidden, mlp_layers, task_out
    "single": (("add", "mean", "max"), 64, 0, 19),   # one linear
    "eight": (("add", "mean", "max"), 64, 7, 1),     # eight linears: the most a HeadArgs holds
    "kfast": (("add",), 64, 2, 19),                  # every k a multiple of 64: k_pool_mlp's unguarded fetches
    "w20": (("add", "mean", "max"), 20, 2, 1),       # k % 64 != 0, n % 16 != 0
    "w33": (("add", "mean", "max"), 33, 2, 19),      # k & 3 != 0 in the later layers: k_pool_mlp's scalar operands
}


@functools.lru_cache(maxsize=None)
def head_case(head, B):
    pools, mlp_hidden, mlp_layers, task_out = HEADS[head]
    model = make_model("gcn", in_dim=11, hidden=64, layers=2, pools=pools, mlp_hidden=mlp_hidden, mlp_layers=mlp_layers,
                       task_out=task_out, seed=mlp_hidden + mlp_layers)
    rng = np.random.default_rng(B)
    sizes = [13] if B == 1 else list(itertools.islice(itertools.cycle(SIZES), B))
    batch = pack_graphs([ring(n, 11, rng) for n in sizes])
    return model, batch, references(model, batch, batch.x)


@pytest.mark.parametrize("B", [1, 16, 17])  # one graph, a whole tile of 16, a ragged second tile
@pytest.mark.parametrize("head", list(HEADS))
def test_head_forms(head, B):
    model, batch, refs = head_case(head, B)
    got = {}
    for form, opts in FORMS.items():
        layerwise = form == "from_x"
        got[form], path = hip(model, batch, batch.x, promise=0 if layerwise else 29, **opts)
        assert path == ("layerwise" if layerwise else "stack_zf"), (form, path)
        check(f"readout head {form}", got[form], model, batch, batch.x, refs=refs)
    for a, b in BITWISE:
        assert np.array_equal(got[a], got[b]), (a, b)
