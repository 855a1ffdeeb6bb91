"""``rgcn_util.rgcn_ref`` -- the float64 restatement tests/test_hip_rgcn.py holds the kernel against -- and the inputs of that
file, checked on references alone: the helper batches with their seeded types hold the rows every path of the kernels needs, and
the budget (``ref64.budget``, K = 4, F = 2^-22, per in-degree class) REJECTS each of five wrong kernels restated in fp32 on the
stage test's own inputs.  No GPU."""
import numpy as np
import pytest

import ref64 as R
from gine_util import budget_by_degree
from helpers import edge_batch, sweep_batch
from rgcn_util import FAULTS, RELATIONS, UNUSED_AT_8, edge_types, relation_counts, rgcn_ref

BATCHES = {}


def _batch(kind):
    """The two batches of tests/test_hip_rgcn.py's stage test."""
    if kind not in BATCHES:
        BATCHES[kind] = edge_batch(8, 4, seed=21) if kind == "edge" else sweep_batch(24, 4, seed=5)[0]
    return BATCHES[kind]


def _types(kind, relations):
    return edge_types(_batch(kind), relations, seed=100 + relations)  # (tests/test_hip_rgcn.py's seeds)


@pytest.mark.parametrize("kind", ["edge", "sweep"])
def test_the_typed_batches_hold_the_rows_the_kernels_need(kind):
    b = _batch(kind)
    deg = np.bincount(b.coo[:, 1], minlength=b.num_nodes)
    assert (deg == 0).sum() >= 5  # rows without in-edges
    assert (b.coo[:, 0] == b.coo[:, 1]).any() and len(np.unique(b.coo, axis=0)) < len(b.coo)  # explicit self loops, duplicate edges
    for relations in RELATIONS:
        t = _types(kind, relations)
        assert t.dtype == np.int32 and t.shape == (b.num_edges,) and t.min() >= 0 and t.max() < relations
        assert np.array_equal(t, _types(kind, relations))  # seeded
        cnt = relation_counts(b.coo, t, relations, b.num_nodes)
        assert np.array_equal(cnt.sum(1), deg)
        if relations > 1:
            hub = int(np.argmax(deg))
            assert deg[hub] >= 1200 and len(set(cnt[hub][cnt[hub] > 0])) >= 2  # a hub with at least two relations of unlike counts
            assert ((cnt == 0).any(1) & (deg > 0)).any()  # rows where some relation is absent
    if kind == "sweep":
        assert ((deg >= 65) & (deg <= 128)).any()  # rows of two pieces
    # at R = 8 one relation has no edge in the batch
    assert not (_types(kind, 8) == UNUSED_AT_8).any() and len(set(_types(kind, 8).tolist())) == 7


def _stage_inputs(relations=3, width=32):
    b = _batch("edge")
    rng = np.random.default_rng(1000 * width + relations)
    pr = rng.uniform(-1, 1, (b.num_nodes, (relations + 1) * width)).astype(np.float32)
    return b, (pr[:, :relations * width], pr[:, relations * width:], None, "none", b.coo, _types("edge", relations), relations)


def test_the_reference_is_within_its_own_budget():
    """``base`` against ``ref`` passes trivially (e = e32): the rejections below are the faults', not the rule's."""
    b, args = _stage_inputs()
    ref, base = rgcn_ref(*args), rgcn_ref(*args, dtype=np.float32)
    assert ref.dtype == np.float64 and base.dtype == np.float32 and np.isfinite(base).all()
    budget_by_degree(base, ref, base, b.coo, what="base")


def test_one_relation_is_the_mean_aggregate():
    b = _batch("sweep")
    p = np.random.default_rng(3).uniform(-1, 1, (b.num_nodes, 9)).astype(np.float32)
    got = rgcn_ref(p, None, None, "none", b.coo, np.zeros(b.num_edges, np.int32), 1)
    assert np.abs(got - R.mean_agg64(p, b.coo)).max() <= 1e-12


@pytest.mark.parametrize("fault", FAULTS)
def test_the_budget_rejects_a_wrong_kernel(fault):
    """On the inputs of the stage test (edge batch, width 32, three relations): a kernel with ``fault`` restated in fp32 is
    outside K * e32 + F."""
    b, args = _stage_inputs()
    ref, base = rgcn_ref(*args), rgcn_ref(*args, dtype=np.float32)
    wrong = rgcn_ref(*args, dtype=np.float32, fault=fault)
    with pytest.raises(AssertionError, match="e ="):
        budget_by_degree(wrong, ref, base, b.coo, what=fault)
