"""The reference at scale (tests/test_hip_large_fp64.py), without a GPU.

Batches of millions of nodes are checked at sampled graphs or rows: ``helpers.sub_batch`` takes the graphs out and the
float64 model and the fp32 oracle run on those alone; ``ref64.agg_rows64`` and ``linear64(rows=...)`` evaluate the stage
restatements at chosen rows.  Every table is local to its graph (GCN's dinv, PNA's degree scalers, pooling), so on a small
batch these must give exactly the full batch's values.  And the rule must see the two faults a 32-bit offset would make
past 2^21 / 2^23 nodes: a row read 2^k rows early (the row-class GEMM's per-lane offset wrapping) and neighbour rows read
from the wrong place of an LDS stage (the ring aggregate's 24-bit products)."""
import numpy as np
import pytest
import torch

import ref64 as R
from helpers import canon, huge_batch, huge_x, make_model, sample_graphs, sub_batch
from oracle import oracle as O

THRESHOLD = 1024  # the small batch's stand-in for 2^21 / 2^23
STAR = np.stack([np.arange(1, 20), np.zeros(19, np.int64)], 1)  # (24 nodes, a hub of in-degree 19)


@pytest.fixture(scope="module")
def batch():
    b = huge_batch(3000, 7, base_graphs=40, place=[(THRESHOLD, STAR, 24), (2000, np.zeros((0, 2)), 5)])
    b.x = huge_x(b.num_nodes, 11, 8).numpy()
    return b


def test_huge_batch_places_graphs_and_tiles(batch):
    b = batch
    b.validate()
    assert b.num_nodes >= 3000 and b.num_nodes < 3000 + 29
    g = int(np.searchsorted(b.node_ptr, THRESHOLD, "right")) - 1
    assert (b.node_ptr[g], b.node_ptr[g + 1]) == (THRESHOLD - 12, THRESHOLD + 12)
    assert np.bincount(b.coo[:, 1])[THRESHOLD - 12] == 19
    g2 = int(np.searchsorted(b.node_ptr, 2000, "right")) - 1
    assert (b.node_ptr[g2], b.node_ptr[g2 + 1], b.edge_ptr[g2 + 1] - b.edge_ptr[g2]) == (1998, 2003, 0)
    # the molecules repeat every 40 graphs (offset arithmetic); the features do not
    sizes = np.diff(b.node_ptr)
    assert np.array_equal(sizes[:20], sizes[40:60])
    assert not np.array_equal(b.x[:b.node_ptr[20]], b.x[b.node_ptr[40]:b.node_ptr[60]])
    # no Python loop per graph: a batch past 2^23 nodes in seconds
    big = huge_batch(2 ** 23 + 1000, 1, place=[(2 ** 23, STAR, 24)])
    g = int(np.searchsorted(big.node_ptr, 2 ** 23, "right")) - 1
    assert big.node_ptr[g] < 2 ** 23 < big.node_ptr[g + 1]


def test_sample_graphs_and_sub_batch(batch):
    b = batch
    gids = sample_graphs(b, 3, count=20, nodes=[THRESHOLD])
    k = int(np.searchsorted(b.node_ptr, THRESHOLD, "right")) - 1
    assert {0, b.num_graphs - 1, k - 1, k, k + 1} <= set(gids.tolist())
    s, rows = sub_batch(b, gids)
    s.validate()
    assert s.num_graphs == len(gids)
    assert np.array_equal(np.diff(s.node_ptr), np.diff(b.node_ptr)[gids])
    assert np.array_equal(s.x, b.x[rows])
    for i, g in enumerate(gids):
        xs, cs = s.graph(i)
        xb, cb = b.graph(int(g))
        assert np.array_equal(xs, xb) and np.array_equal(cs, cb)


def _pna_delta(model, delta):
    for conv in model.gnn_convs:  # (as test_hip_parity: GNNModel never passes delta)
        conv.delta_scaler = delta
        conv.conv.aggr_module.avg_deg_log = torch.Tensor([delta])
    return model


@pytest.mark.parametrize("conv", ["gcn", "gin", "sage", "pna"])
def test_forward_on_sub_batch_equals_full_batch(batch, conv):
    model = make_model(conv, in_dim=11, hidden=32, layers=3, task_out=5, seed=4)
    if conv == "pna":
        _pna_delta(model, 2.5)
    b = batch
    gids = sample_graphs(b, 5, count=30, nodes=[THRESHOLD])
    s, _ = sub_batch(b, gids)
    full64, sub64 = R.forward64(model, b, b.x), R.forward64(model, s, s.x)
    np.testing.assert_allclose(sub64, full64[gids], rtol=0, atol=1e-13 * np.abs(full64).max())
    full32 = O.forward_batched(model.spec(), canon(model), b.x, b.coo, b.node_ptr, b.edge_ptr)
    sub32 = O.forward_batched(model.spec(), canon(model), s.x, s.coo, s.node_ptr, s.edge_ptr)
    np.testing.assert_array_equal(sub32, full32[gids])


@pytest.mark.parametrize("kind,gcn_ws", [("gcn", True), ("gcn", False), ("sum", False), ("mean", False), ("simple", False)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_row_sampled_aggregates_equal_the_full_form(batch, kind, gcn_ws, dtype):
    b = batch
    x = huge_x(b.num_nodes, 20, 9).numpy()
    coo = R.workspace_edges(b.coo, gcn_ws)
    full = {"gcn": lambda: R.gcn_agg64(x, coo, dtype), "sum": lambda: R.sum_agg64(x, coo, 0.25, dtype),
            "mean": lambda: R.mean_agg64(x, coo, dtype), "simple": lambda: R.simple64(x, coo, dtype)}[kind]()
    rows = np.unique(np.concatenate([np.arange(THRESHOLD - 12, THRESHOLD + 12), [0, b.num_nodes - 1],
                                     np.random.default_rng(1).integers(0, b.num_nodes, 100)]))
    fetched = []
    got = R.agg_rows64(kind, coo, b.num_nodes, rows, lambda ids: fetched.append(len(ids)) or x[ids], eps=0.25, dtype=dtype)
    assert got.dtype == dtype
    np.testing.assert_array_equal(got, full[rows])
    assert fetched[0] < b.num_nodes // 4  # (only the rows and their sources are read)


def test_row_sampled_linear_equals_the_full_form():
    g = np.random.default_rng(2)
    a0, a1 = g.uniform(-1, 1, (500, 16)).astype(np.float32), g.uniform(-1, 1, (500, 36)).astype(np.float32)
    rs, w = g.uniform(0.5, 1.5, 500).astype(np.float32), g.uniform(-1, 1, (7, 52)).astype(np.float32)
    b, sk = g.uniform(-1, 1, 7).astype(np.float32), g.uniform(-1, 1, (500, 7)).astype(np.float32)
    rows = np.array([0, 3, 250, 499])
    for dtype in (torch.float64, torch.float32):
        full = R.linear64([(a0, None), (a1, rs)], w, b, sk, "tanh", dtype=dtype)
        for seg0 in (a0, torch.from_numpy(a0)):  # (arrays or tensors: a device tensor gives up only the rows)
            got = R.linear64([(seg0, None), (a1, torch.from_numpy(rs))], w, b, torch.from_numpy(sk), "tanh", dtype=dtype, rows=rows)
            np.testing.assert_allclose(got, full[rows], rtol=0, atol=4 * np.finfo(np.float32 if dtype == torch.float32 else np.float64).eps)


@pytest.mark.parametrize("shift", [1, 6, 9])
def test_budget_rejects_rows_read_early(shift):
    """The row-class GEMM's fault: from row T on, each row's aggregate segment is that of the row 2^shift before it."""
    g = np.random.default_rng(shift)
    M, F, T = 2000, 16, THRESHOLD
    x, agg = g.uniform(-1, 1, (M, F)).astype(np.float32), g.uniform(-1, 1, (M, 4 * F)).astype(np.float32)
    w, b = (g.uniform(-1, 1, (F, 5 * F)) / np.sqrt(5 * F)).astype(np.float32), g.uniform(-0.1, 0.1, F).astype(np.float32)
    bad = agg.copy()
    bad[T:] = agg[T - 2 ** shift:M - 2 ** shift]
    rows = np.concatenate([[0, T - 1, T, M - 1], g.integers(0, M, 50)])
    rows = np.unique(rows)
    segs = [(x, None), (agg, None)]
    ref, base = R.linear64(segs, w, b, act="relu", rows=rows), R.linear64(segs, w, b, act="relu", dtype=torch.float32, rows=rows)
    R.budget(R.linear64([(x, None), (agg.astype(np.float64).astype(np.float32), None)], w, b, act="relu", dtype=torch.float32, rows=rows), ref, base)
    with pytest.raises(AssertionError, match="e = "):
        R.budget(R.linear64([(x, None), (bad, None)], w, b, act="relu", rows=rows), ref, base)


@pytest.mark.parametrize("kind", ["gcn", "sum", "mean", "simple"])
@pytest.mark.parametrize("fault", ["next_row", "zero_row"])
def test_budget_rejects_a_wrong_lds_row(batch, kind, fault):
    """The ring aggregate's fault: in the stage that straddles the threshold, a source row at or past it is read from the
    wrong place of the stage -- another row of it (``next_row``) or past its end, which reads 0 (``zero_row``)."""
    b = batch
    x = huge_x(b.num_nodes, 20, 10).numpy()
    gcn_ws = kind == "gcn"
    coo = R.workspace_edges(b.coo, gcn_ws)
    rows = np.arange(THRESHOLD - 12, THRESHOLD + 12)
    ref = R.agg_rows64(kind, coo, b.num_nodes, rows, lambda ids: x[ids], eps=0.25)
    base = R.agg_rows64(kind, coo, b.num_nodes, rows, lambda ids: x[ids], eps=0.25, dtype=np.float32)
    # (neighbour reads only: the self term comes from the row's own, stage-relative place)
    xz = np.concatenate([x, np.zeros((1, x.shape[1]), np.float32)])  # (node num_nodes: the zeros past the stage)
    src, dst = coo.T
    moved = np.isin(src, np.arange(THRESHOLD, THRESHOLD + 12)) & np.isin(dst, rows)
    assert moved.sum() >= 8
    bad = coo.copy()
    bad[moved, 0] = src[moved] + 1 if fault == "next_row" else b.num_nodes
    got = R.agg_rows64(kind, bad, b.num_nodes + 1, rows, lambda ids: xz[ids], eps=0.25)
    with pytest.raises(AssertionError, match="e = "):
        R.budget(got, ref, base)
