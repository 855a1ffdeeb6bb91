"""PyG mini-batches ingested on the device (csrc/k_ingest.hip; ``CompiledModel.ingest_pyg`` / ``forward_pyg``).

The reference is always ``batching.from_pyg_batch`` on the CPU; every comparison is exact integer equality of ``coo``,
``node_ptr`` and ``edge_ptr``.  Grouped input takes the fast path (two kernels do the work), shuffled edges the stable radix
grouping -- 8 bits of the graph id per pass, so 12 graphs need one pass, 300 two and 70 000 three."""
import re

import numpy as np
import pytest
import torch

from gnnbuilder_amd import runtime, synthetic
from gnnbuilder_amd.batching import from_pyg_batch
from helpers import batch_vector, make_model

pytestmark = pytest.mark.gpu

FIN = 4
CAP = (512, 16384, 32768)  # graphs, nodes, edges of the shared workspace


@pytest.fixture(scope="module")
def dev():
    runtime.load_library(require_gpu=True)  # fails loudly: no fallback
    return torch.device("cuda:0")


def _model(conv="gin", **kw):
    args = dict(in_dim=FIN, hidden=8, layers=1, out_dim=8, task_out=3, mlp_layers=0)
    args.update(kw)
    return make_model(conv, **args)


@pytest.fixture(scope="module")
def cm(dev):
    m = runtime.CompiledModel.from_model(_model(), *CAP)
    m.enable_ingest()
    return m


def _pyg(b):
    """(edge_index [2, E] int64, batch [N] int64) of a GraphBatch: what ``Batch.from_data_list`` holds (grouped edges)."""
    return np.ascontiguousarray(b.coo.T.astype(np.int64)).reshape(2, -1), batch_vector(b)


def _ref(ei, N, batch=None, ptr=None, B=None):
    r = from_pyg_batch(np.zeros((N, 1), np.float32), ei, batch=batch, ptr=ptr, num_graphs=B)
    return r.coo, r.node_ptr, r.edge_ptr


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _ingest(m, dev, ei, N, batch=None, ptr=None, B=None):
    got = m.ingest_pyg(_t(ei, dev), batch=_t(batch, dev), ptr=_t(ptr, dev), num_graphs=B, num_nodes=N)
    assert all(t.dtype == torch.int32 and t.is_cuda for t in got)
    return tuple(t.cpu().numpy() for t in got)


def _same(got, ref):
    for g, r, what in zip(got, ref, ("coo", "node_ptr", "edge_ptr")):
        assert g.dtype == np.int32 and g.shape == r.shape, (what, g.shape, r.shape)
        assert np.array_equal(g, r), what


def _check_against_host(m, dev, ei, N, batch=None, ptr=None, B=None):
    got = _ingest(m, dev, ei, N, batch=batch, ptr=ptr, B=B)
    m.check()
    _same(got, _ref(ei, N, batch=batch, ptr=ptr, B=B))
    return got


# ---------------------------------------------------------------------------------------------------- 1. grouped, fast path
@pytest.mark.parametrize("form", ["batch", "ptr"])
def test_grouped_batch(cm, dev, form):
    b = synthetic.make_batch("qm9", 12, seed=5)
    ei, batch = _pyg(b)
    if form == "batch":
        got = _check_against_host(cm, dev, ei, b.num_nodes, batch=batch, B=12)
    else:
        got = _check_against_host(cm, dev, ei, b.num_nodes, ptr=b.node_ptr.astype(np.int64))
    _same(got, (b.coo, b.node_ptr, b.edge_ptr))  # (grouped input comes back as it was)


def test_outputs_are_views_of_the_workspace(cm, dev):
    b = synthetic.make_batch("qm9", 6, seed=1)
    ei, batch = _pyg(b)
    first = cm.ingest_pyg(_t(ei, dev), batch=_t(batch, dev), num_graphs=6)
    second = cm.ingest_pyg(_t(ei, dev), batch=_t(batch, dev), ptr=_t(b.node_ptr.astype(np.int64), dev))  # (both given: B from ptr)
    assert [t.data_ptr() for t in first] == [t.data_ptr() for t in second]
    cm.check()
    _same(tuple(t.cpu().numpy() for t in second), (b.coo, b.node_ptr, b.edge_ptr))


# ---------------------------------------------------------------------------------------------------- 2. shuffled, general path
@pytest.mark.parametrize("graphs", [12, 300])
@pytest.mark.parametrize("form", ["batch", "ptr"])
def test_shuffled_edges_are_grouped_stably(cm, dev, graphs, form):
    b = synthetic.make_batch("qm9", graphs, seed=graphs)
    ei, batch = _pyg(b)
    ei = np.ascontiguousarray(ei[:, np.random.default_rng(7).permutation(ei.shape[1])])
    if form == "batch":
        _check_against_host(cm, dev, ei, b.num_nodes, batch=batch, B=graphs)
    else:
        _check_against_host(cm, dev, ei, b.num_nodes, ptr=b.node_ptr.astype(np.int64))


# ---------------------------------------------------------------------------------------------------- 3. three radix passes
def test_more_graph_ids_than_two_digit_passes_cover(dev):
    """70 000 two-node graphs with both directed edges each, shuffled: ids need 17 bits = three passes of 8."""
    B = 70_000
    assert 2 ** (2 * runtime.INGEST_DIGIT_BITS) < B
    m = runtime.CompiledModel.from_model(_model(), B, 2 * B, 2 * B)
    m.enable_ingest()
    a = 2 * np.arange(B, dtype=np.int64)
    ei = np.stack([np.concatenate([a, a + 1]), np.concatenate([a + 1, a])])
    ei = np.ascontiguousarray(ei[:, np.random.default_rng(11).permutation(2 * B)])
    _check_against_host(m, dev, ei, 2 * B, batch=np.repeat(np.arange(B, dtype=np.int64), 2), B=B)


# ---------------------------------------------------------------------------------------------------- 4. block edges
@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("E", [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4096, 4097])
def test_edge_counts_around_wave_workgroup_and_tile(cm, dev, E, shuffled):
    """64 lanes, 256 threads, tiles of 1024 edges (one more element closes the ptr arrays: E = 1023 fills a tile exactly).  The
    general path's digit table has 256 entries per tile and is scanned in chunks of 1024: E = 4096 (4 tiles) fills one chunk
    exactly, E = 4097 (5 tiles) carries into a second."""
    assert runtime.INGEST_TILE == 1024
    rng = np.random.default_rng(E)
    sizes = np.array([7, 9, 8, 3, 13])
    nptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    g = rng.integers(0, 5, E)
    if not shuffled:
        g = np.sort(g)
    ei = np.stack([nptr[g] + rng.integers(0, sizes[g]), nptr[g] + rng.integers(0, sizes[g])]).astype(np.int64).reshape(2, E)
    _check_against_host(cm, dev, ei, int(nptr[-1]), batch=np.repeat(np.arange(5), sizes).astype(np.int64), B=5)
    _check_against_host(cm, dev, ei, int(nptr[-1]), ptr=nptr)


# ---------------------------------------------------------------------------------------------------- 5. degenerate graphs
def _degenerate():
    """Graphs without nodes at the start, in the middle and at the end; one with nodes and no edge; duplicates, self loops."""
    sizes = np.array([0, 0, 5, 0, 3, 4, 6, 0, 0])
    nptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    edges = {2: [(0, 1), (1, 1), (0, 1), (4, 3), (0, 1), (2, 2)], 4: [(2, 0), (2, 0), (1, 1)], 6: [(5, 0), (0, 5), (3, 3), (5, 0)]}
    ei = np.array([(nptr[g] + s, nptr[g] + d) for g, es in edges.items() for s, d in es], dtype=np.int64).T
    return np.ascontiguousarray(ei), nptr, np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)


@pytest.mark.parametrize("shuffled", [False, True])
def test_degenerate_graphs(cm, dev, shuffled):
    ei, nptr, batch = _degenerate()
    if shuffled:
        ei = np.ascontiguousarray(ei[:, np.random.default_rng(3).permutation(ei.shape[1])])
    N, B = int(nptr[-1]), len(nptr) - 1
    got = _check_against_host(cm, dev, ei, N, batch=batch, B=B)
    _check_against_host(cm, dev, ei, N, ptr=nptr)
    order = np.argsort(np.searchsorted(nptr, ei[1], "right") - 1, kind="stable")  # duplicates and loops keep their order
    assert np.array_equal(got[0], ei[:, order].T)


def test_one_graph_without_batch_or_ptr(cm, dev):
    rng = np.random.default_rng(2)
    ei = rng.integers(0, 17, (2, 90)).astype(np.int64)
    got = _ingest(cm, dev, ei, 17)
    cm.check()
    _same(got, (ei.T.astype(np.int32), np.array([0, 17], np.int32), np.array([0, 90], np.int32)))
    _same(got, _ref(ei, 17))


def test_no_nodes(cm, dev):
    ei = np.zeros((2, 0), np.int64)
    _check_against_host(cm, dev, ei, 0, batch=np.zeros(0, np.int64), B=3)
    _check_against_host(cm, dev, ei, 0, ptr=np.zeros(4, np.int64))
    got = _ingest(cm, dev, ei, 0, batch=np.zeros(0, np.int64), B=0)
    cm.check()
    _same(got, (np.zeros((0, 2), np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)))


# ---------------------------------------------------------------------------------------------------- 6. malformed input
def _good():
    b = synthetic.make_batch("qm9", 12, seed=9)
    ei, batch = _pyg(b)
    return b, ei, batch


def _defects():
    b, ei, batch = _good()
    N, B = b.num_nodes, b.num_graphs
    k = int(b.edge_ptr[4]) + 1  # an edge of graph 4
    nptr = b.node_ptr.astype(np.int64)

    def edge(row, value):
        e = ei.copy()
        e[row, k] = value
        return dict(ei=e, batch=batch, B=B)

    def nodes(i, value):
        v = batch.copy()
        v[i] = value
        return dict(ei=ei, batch=v, B=B)

    return N, {
        "cross-graph edge": edge(0, int(b.node_ptr[7])),
        "endpoint = N": edge(1, N),
        "endpoint = -1": edge(0, -1),
        "endpoint = 2^32 + valid": edge(1, 2 ** 32 + int(ei[1, k])),
        "batch decreases once": nodes(int(b.node_ptr[5]) + 1, 3),
        "batch id = B": nodes(N - 1, B),
        "ptr not ending at N": dict(ei=ei, ptr=np.concatenate([nptr[:-1], [N - 1]])),
    }


def _flag_bits(exc):
    m = re.search(r"flags 0x([0-9a-f]+)", str(exc))
    assert m, str(exc)
    return int(m.group(1), 16)


@pytest.mark.parametrize("defect", ["cross-graph edge", "endpoint = N", "endpoint = -1", "endpoint = 2^32 + valid",
                                    "batch decreases once", "batch id = B", "ptr not ending at N"])
def test_malformed_input_is_flagged_and_contained(cm, dev, defect):
    N, cases = _defects()
    args = cases[defect]
    E = args["ei"].shape[1]
    coo, nptr, eptr = _ingest(cm, dev, args["ei"], N, batch=args.get("batch"), ptr=args.get("ptr"), B=args.get("B"))  # returns normally
    with pytest.raises(runtime.GnnbError) as err:
        cm.check()
    assert _flag_bits(err.value) & 0x80, str(err.value)
    # containment: every output written, in range and monotone
    assert coo.shape == (E, 2) and nptr.shape == (13,) and eptr.shape == (13,)
    assert nptr[0] == 0 and nptr[-1] == N and np.all(np.diff(nptr) >= 0)
    assert eptr[0] == 0 and eptr[-1] == E and np.all(np.diff(eptr) >= 0)
    assert coo.min() >= 0 and coo.max() < N
    # a well-formed batch on the same workspace is not blamed for it
    b, ei, batch = _good()
    _check_against_host(cm, dev, ei, N, batch=batch, B=12)


def test_flagged_batch_is_reported_by_the_next_forward(dev):
    model = _model("gcn", layers=2, hidden=16, out_dim=16)
    m = runtime.CompiledModel.from_model(model, 16, 512, 1024)
    m.enable_ingest()
    N, cases = _defects()
    bad = cases["endpoint = N"]
    b, ei, batch = _good()
    x = torch.zeros((N, FIN), device=dev)
    m.forward_pyg(x, _t(bad["ei"], dev), batch=_t(batch, dev), num_graphs=12)  # flagged on the device; no check()
    torch.cuda.synchronize()
    with pytest.raises(runtime.GnnbError, match="earlier batch"):
        m.forward_pyg(x, _t(ei, dev), batch=_t(batch, dev), num_graphs=12)
    m.forward_pyg(x, _t(ei, dev), batch=_t(batch, dev), num_graphs=12)  # reported once
    m.check()


# ---------------------------------------------------------------------------------------------------- 7. end to end
@pytest.mark.parametrize("conv,hidden,promise", [("gcn", 32, 29), ("sage", 16, 0)])
def test_forward_pyg_is_forward_on_the_host_adapters_batch(dev, conv, hidden, promise):
    b = synthetic.make_batch("qm9", 12, seed=21)
    ei, batch = _pyg(b)
    ei = np.ascontiguousarray(ei[:, np.random.default_rng(4).permutation(ei.shape[1])])
    model = make_model(conv, in_dim=11, hidden=hidden, layers=2, out_dim=hidden, task_out=5)
    m = runtime.CompiledModel.from_model(model, 12, b.num_nodes, b.num_edges, max_graph_nodes=promise)
    m.enable_ingest()
    x = _t(b.x, dev)
    got = m.forward_pyg(x, _t(ei, dev), batch=_t(batch, dev), num_graphs=12).clone()
    m.check()
    path = m.last_path()
    row_ptr, col, in_deg = m.tables_to_host()  # (the stage-level entry points follow a forward_pyg as they follow a forward)
    ref = from_pyg_batch(b.x, ei, batch=batch, num_graphs=12)
    want = m.forward(x, _t(ref.coo, dev), _t(ref.node_ptr, dev), _t(ref.edge_ptr, dev))
    m.check()
    assert torch.equal(got, want)
    assert m.last_path() == path and path != "none"
    for a, r in zip((row_ptr, col, in_deg), m.tables_to_host()):
        assert np.array_equal(a, r)


def test_one_captured_ingest_replays_on_grouped_and_on_shuffled_edges(cm, dev):
    """The launch sequence depends on the three host integers only: a HIP graph captured once serves both kinds of batch."""
    b = synthetic.make_batch("qm9", 12, seed=13)
    ei, batch = _pyg(b)
    shuffled = np.ascontiguousarray(ei[:, np.random.default_rng(8).permutation(ei.shape[1])])
    ei_dev, batch_dev = _t(ei, dev), _t(batch, dev)
    _same(tuple(t.cpu().numpy() for t in cm.ingest_pyg(ei_dev, batch=batch_dev, num_graphs=12)), (b.coo, b.node_ptr, b.edge_ptr))  # (warm-up)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        out = cm.ingest_pyg(ei_dev, batch=batch_dev, num_graphs=12)
    for edges in (shuffled, ei, shuffled):
        ei_dev.copy_(torch.from_numpy(edges))
        graph.replay()
        torch.cuda.synchronize()
        _same(tuple(t.cpu().numpy() for t in out), _ref(edges, b.num_nodes, batch=batch, B=12))
    cm.check()


# ---------------------------------------------------------------------------------------------------- 8. API errors, no device work
def test_api_errors(cm, dev):
    b, ei, batch = _good()
    ei_dev, batch_dev = _t(ei, dev), _t(batch, dev)
    plain = runtime.CompiledModel.from_model(_model(), 16, 512, 1024)
    with pytest.raises(runtime.GnnbError, match="enable_ingest"):
        plain.ingest_pyg(ei_dev, batch=batch_dev, num_graphs=12)
    with pytest.raises(runtime.GnnbError, match=r"\[2, E\].*contiguous\(\)"):
        cm.ingest_pyg(ei_dev.t().contiguous(), batch=batch_dev, num_graphs=12)
    with pytest.raises(runtime.GnnbError, match="int64"):
        cm.ingest_pyg(ei_dev.to(torch.int32), batch=batch_dev, num_graphs=12)
    with pytest.raises(runtime.GnnbError, match="num_graphs is required"):
        cm.ingest_pyg(ei_dev, batch=batch_dev)
    small = runtime.CompiledModel.from_model(_model(), 4, 512, 1024)
    small.enable_ingest()
    with pytest.raises(runtime.GnnbError, match="error -2.*exceeds workspace"):
        small.ingest_pyg(ei_dev, batch=batch_dev, num_graphs=12)
    # in use: a batch has been prepared on the workspace
    x = torch.zeros((b.num_nodes, FIN), device=dev)
    plain.forward(x, _t(b.coo, dev), _t(b.node_ptr, dev), _t(b.edge_ptr, dev))
    with pytest.raises(runtime.GnnbError, match="in use"):
        plain.enable_ingest()
    plain.check()
