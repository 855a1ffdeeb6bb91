"""``batching.from_pyg_batch(..., edge_type=)`` -- the host counterpart of the device ingest with edge types
(``CompiledModel.ingest_pyg_types``): the types follow their edges through the stable sort by graph.  No GPU."""
import numpy as np
import pytest

from gnnbuilder_amd import synthetic
from gnnbuilder_amd.batching import from_pyg_batch
from helpers import batch_vector


def _batch():
    return synthetic.make_batch("qm9", 8, seed=3)


def test_grouped_input_keeps_its_types_in_place():
    b = _batch()
    t = np.random.default_rng(0).integers(0, 4, b.num_edges)
    gb, t_ord = from_pyg_batch(b.x, b.coo.T, batch=batch_vector(b), edge_type=t)
    assert np.array_equal(gb.coo, b.coo) and t_ord.dtype == np.int32 and np.array_equal(t_ord, t)
    alone = from_pyg_batch(b.x, b.coo.T, batch=batch_vector(b))
    assert np.array_equal(alone.coo, gb.coo)  # (without types: the batch alone, as before)


def test_shuffled_input_carries_its_types_along():
    b = _batch()
    rng = np.random.default_rng(1)
    perm = rng.permutation(b.num_edges)
    t = np.arange(b.num_edges) % 5  # (a type that names its input position modulo 5)
    ea = rng.uniform(-1, 1, (b.num_edges, 3)).astype(np.float32)
    gb, ea_ord, t_ord, order = from_pyg_batch(b.x, b.coo[perm].T, ptr=b.node_ptr, edge_attr=ea, edge_type=t, return_edge_order=True)
    assert not np.array_equal(order, np.arange(b.num_edges))
    assert np.array_equal(gb.coo, b.coo[perm][order]) and np.array_equal(t_ord, t[order]) and np.array_equal(ea_ord, ea[order])
    assert np.array_equal(gb.edge_ptr, b.edge_ptr)
    gb2, t2 = from_pyg_batch(b.x, b.coo[perm].T, ptr=b.node_ptr, edge_type=t.astype(np.int32))
    assert np.array_equal(t2, t_ord) and np.array_equal(gb2.coo, gb.coo)


def test_bad_types_are_refused():
    b = _batch()
    for bad, what in ((np.zeros(b.num_edges - 1, np.int64), "one type per column"), (np.zeros((b.num_edges, 1), np.int64), "one type per column"),
                      (np.zeros(b.num_edges, np.float32), "integers"), (np.full(b.num_edges, 2 ** 31, np.int64), "int32")):
        with pytest.raises(ValueError, match=what):
            from_pyg_batch(b.x, b.coo.T, batch=batch_vector(b), edge_type=bad)
