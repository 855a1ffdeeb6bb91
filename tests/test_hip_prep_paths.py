"""The boundaries between graph prep's three paths (gnnb_prep.h), bit-exactly.

One batch of small random multigraphs, each with a few explicit self loops and duplicate edges, whose (nodes, edges) sit on
both sides of every bound: the molecule path (<= 64 / <= 64), the register path (<= 256 / <= 256, one to four edge and node
chunks), the scan path with its edges in registers (<= 256 edges) and re-reading them.  A molecule-path graph and an empty
graph lie in between, so that neighbours of different paths share a wave group."""
import numpy as np
import pytest
import torch

import ref64 as R
from gnnbuilder_amd import runtime
from gnnbuilder_amd.batching import pack_graphs
from helpers import canon, make_model, oracle_tables_batched, to_dev
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FIN = 8
SIZES = [(65, 64), (64, 65), (64, 256), (40, 50), (130, 250), (256, 256), (200, 129),   # register path (+ one molecule)
         (257, 0), (257, 256), (0, 0), (300, 200),                                        # scan path, edges in registers (+ empty)
         (64, 257), (257, 257), (300, 700)]                                               # scan path re-reading its edges


@pytest.fixture(scope="module")
def dev():
    runtime.load_library(require_gpu=True)  # fails loudly: no fallback
    return torch.device("cuda:0")


def _graph(rng, n, e):
    coo = np.stack([rng.integers(0, max(n, 1), e), rng.integers(0, max(n, 1), e)], 1).astype(np.int32)
    if e >= 8:
        v = rng.integers(0, n, 3)
        coo[1:4] = np.stack([v, v], 1)  # explicit self loops
        coo[5:8] = coo[0]               # duplicates of edge 0
    return rng.uniform(-1, 1, (n, FIN)).astype(np.float32), coo


@pytest.fixture(scope="module")
def batch():
    rng = np.random.default_rng(23)
    return pack_graphs([_graph(rng, n, e) for n, e in SIZES])


def _prepared(conv, b, dev, promise=0):
    cm = runtime.CompiledModel.from_model(make_model(conv, in_dim=FIN, hidden=8, layers=1, out_dim=8, task_out=3, mlp_layers=0),
                                          b.num_graphs, b.num_nodes, max(b.num_edges, 1), max_graph_nodes=promise)
    _, coo, nptr, eptr = to_dev(b, dev)
    cm.graph_prep(coo, nptr, eptr, b.num_nodes)
    cm.check()
    return cm


def _assert_tables(cm, b, keep_self=True):
    """row_ptr / col / in-degree against the oracle, the edge-index table against the stable sort of COO rows by destination."""
    row_ptr, col, in_deg = cm.tables_to_host()
    eid = cm.edge_index_table_to_host()
    if keep_self:
        rp_ref, col_ref = oracle_tables_batched(b)
        assert np.array_equal(row_ptr, rp_ref)
        assert np.array_equal(col, col_ref)
        assert np.array_equal(in_deg, np.diff(rp_ref))
        assert np.array_equal(eid, np.argsort(b.coo[:, 1], kind="stable"))
        return
    # GCN: explicit self loops are not entered.  The oracle's tables cannot serve here: the device keeps every row start inside
    # the graph's UNFILTERED CSR segment (the dropped edges leave slots unowned), so row_ptr is bounded, not pinned; degrees,
    # sources and COO rows are pinned exactly against the stable sort of the kept edges by destination.
    kept = np.flatnonzero(b.coo[:, 0] != b.coo[:, 1])
    assert np.array_equal(in_deg, np.bincount(b.coo[kept, 1], minlength=b.num_nodes))
    order = kept[np.argsort(b.coo[kept, 1], kind="stable")]
    slots = np.concatenate([np.arange(row_ptr[v], row_ptr[v] + in_deg[v]) for v in range(b.num_nodes)]).astype(np.int64)
    assert np.array_equal(eid[slots], order)
    assert np.array_equal(col[slots], b.coo[order, 0])
    graph_of = np.repeat(np.arange(b.num_graphs), np.diff(b.node_ptr))
    assert np.all(row_ptr[:-1] >= b.edge_ptr[graph_of]) and np.all(row_ptr[:-1] + in_deg <= b.edge_ptr[graph_of + 1])


def test_paths_without_a_promise(dev, batch):
    """k_graph_prep<256, 1> on a GIN-bound workspace, which keeps every edge."""
    cm = _prepared("gin", batch, dev)
    _assert_tables(cm, batch)


def test_paths_drop_self_loops_on_a_gcn_workspace(dev, batch):
    assert (batch.coo[:, 0] == batch.coo[:, 1]).sum() >= 3 * 10
    cm = _prepared("gcn", batch, dev)
    _assert_tables(cm, batch, keep_self=False)


@pytest.mark.parametrize("group", [1, 4])
def test_paths_under_a_promise_of_64_nodes(dev, batch, group):
    """k_graph_prep<64, 1> and <64, 4>: the graphs of <= 64 nodes, repeated to the 2047 graphs the grouped form needs."""
    small = [g for g, (n, _) in enumerate(SIZES) if n <= 64]
    assert len(small) == 5
    b = pack_graphs(([batch.graph(g) for g in small] * 410)[:2050])
    try:
        runtime.set_option("prep_group", group)
        cm = _prepared("gin", b, dev, promise=64)
    finally:
        runtime.set_option("prep_group", 4)  # (the default: the binding has no getter, tests/test_options.py pins the value)
    _assert_tables(cm, b)


@pytest.mark.parametrize("conv", ["pna", "gcn"])
def test_one_layer_forward_reads_the_scalers_and_records(dev, batch, conv):
    """amp / att (PNA), dinv (GCN) and the node records have no host read-back: one layer against float64."""
    model = make_model(conv, in_dim=FIN, hidden=16, layers=1, out_dim=16, task_out=3)
    cm = runtime.CompiledModel.from_model(model, batch.num_graphs, batch.num_nodes, batch.num_edges)
    x, coo, nptr, eptr = to_dev(batch, dev)
    got = cm.forward(x, coo, nptr, eptr).cpu().numpy()
    cm.check()
    base = O.forward_batched(model.spec(), canon(model), batch.x, batch.coo, batch.node_ptr, batch.edge_ptr)
    R.budget(got, R.forward64(model, batch, batch.x), base, what=f"prep paths, {conv}")
