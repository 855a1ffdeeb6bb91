"""Batches past 2^21 / 2^23 nodes and operands past 4 GiB against float64, with the fp32-class budget of ref64.

The C ABI takes any ``max_nodes`` / ``max_edges`` up to INT_MAX, and several kernels keep their address arithmetic in 32 or
24 bits (DESIGN.md section 4 lists every kernel family's index width).  Here each family runs at the sizes where such
arithmetic would wrap:
  * the row-class GEMM of PNA under a degree promise (the C4 route): ``(row * lda * 4)`` as a 32-bit per-lane offset passes
    2^32 from row 2^21 at F = 128 and from row 2^20 at F = 256;
  * the ring aggregate's lean path (GCN / SUM / MEAN / SIMPLE, float4 rows, w <= 256): its LDS addresses are 24-bit
    products of batch-global node ids, which lose their high bits from node 2^23 on unless w % 64 == 0;
  * ``gnnb_linear`` with A past 4 GiB, ``gnnb_global_pool`` on x past 4 GiB, and whole forwards past 2^23 nodes on the
    routes whose global offsets the audit found to be 64-bit (controls).
The batches are ``helpers.huge_batch`` tilings of QM9-shaped molecules with a graph placed across each threshold; features
come from a device generator.  At millions of nodes only sampled graphs (or their rows) are checked -- the first, the ones
on both sides of each threshold, the last and 256 seeded random ones -- with ``helpers.sub_batch`` / ``ref64.agg_rows64``
/ ``linear64(rows=...)`` (tests/test_ref64_scale.py shows these equal the full-batch values).  Outputs start as NaN, so a
skipped row fails.  About 40 GB of device memory at the peak."""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

import ref64 as R
from gnnbuilder_amd import runtime
from helpers import canon, huge_batch, huge_x, make_model, sample_graphs, sub_batch, to_dev
from oracle import oracle as O

pytestmark = pytest.mark.gpu

# the process-wide defaults of every option this file sets (gnnb_runtime.hip options())
DEFAULTS = {"math": 0, "gemm_wlds": 1, "gemm_variant": 0, "gemm_dma": 1, "gemm_tail_split": 2, "agg_form": 0, "agg_balance": 0,
            "pna_classes": 1}
WORST = {}  # case -> worst e / e32 (merged into GNNB_FP64_REPORT=<file> with the other fp64 files')
T20, T21, T23 = 2 ** 20, 2 ** 21, 2 ** 23
GIB4 = 2 ** 32
# a 14-node graph placed across a threshold: a hub of in-degree 12 (<= 15: PNA's degree classes still apply; > 4: the
# aggregates read the CSR tail) with edges back to it, so that neighbours lie on both sides
HUB = np.concatenate([np.stack([np.arange(1, 13), np.zeros(12, np.int64)], 1), np.stack([np.zeros(12, np.int64), np.arange(1, 13)], 1),
                      [[13, 1], [1, 13]]])


@pytest.fixture(scope="module", autouse=True)
def _library():
    runtime.load_library(require_gpu=True)  # fails loudly: no fallback
    yield
    report = os.environ.get("GNNB_FP64_REPORT")
    if report:
        have = {}
        if os.path.exists(report):
            with open(report) as f:
                have = json.load(f)
        have.update(WORST)
        with open(report, "w") as f:
            json.dump(dict(sorted(have.items())), f, indent=1)


@pytest.fixture(autouse=True)
def _free_device_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@contextlib.contextmanager
def options(**kw):
    try:
        for k, v in kw.items():
            runtime.set_option(k, v)
        yield
    finally:
        for k in kw:
            runtime.set_option(k, DEFAULTS[k])


def dev_():
    return torch.device("cuda:0")


def record(entry, got, ref, base, k=R.K):
    e, e32 = R.budget(got, ref, base, k=k, what=entry)
    WORST[entry] = max(WORST.get(entry, 0.0), R.ratio(e, e32))


def nan(shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev_())


def rows_of(x_d, ids):
    return x_d[torch.from_numpy(np.asarray(ids, np.int64)).to(dev_())].cpu().numpy()


def check_forward(what, model, batch, x_d, promise=0, maxdeg=0, want="layerwise", **opts):
    """One forward of the whole batch through the C ABI, checked at the sampled graphs (those across ``what``'s threshold
    included) against the float64 model and the fp32 oracle on the same graphs (``what`` None: not checked); the route must be
    ``want`` (None: any).  Returns (the whole output, the route)."""
    thresholds = [t for t in (T20, T21, T23) if t < batch.num_nodes]
    with options(**opts):
        cm = runtime.CompiledModel.from_model(model, batch.num_graphs, batch.num_nodes, batch.num_edges, max_graph_nodes=promise)
        try:
            if maxdeg:
                cm.set_max_degree(maxdeg)
            assert cm.workspace_bytes < 40e9, cm.workspace_bytes
            _, coo, nptr, eptr = to_dev(batch, dev_())
            out = cm.forward(x_d, coo, nptr, eptr, out=nan((batch.num_graphs, cm.out_dim)))
            cm.check()
            path = cm.last_path()
            got = out.cpu().numpy()
        finally:
            cm.close()
    del coo, nptr, eptr, out
    assert want is None or path == want
    if what is None:
        return got, path
    gids = sample_graphs(batch, batch.num_nodes, nodes=thresholds)
    s, rows = sub_batch(batch, gids)
    s.x = rows_of(x_d, rows)
    ref = R.forward64(model, s, s.x)
    base = O.forward_batched(model.spec(), canon(model), s.x, s.coo, s.node_ptr, s.edge_ptr)
    record(what, got[gids], ref, base)
    return got, path


# --------------------------------------------------------------------------- PNA under a degree promise (C4's route)
# (F, nodes, math): past the row-class GEMM's 32-bit row offsets (16 F bytes per aggregate row: 2^21 rows at F = 128, 2^20 at
# F = 256) and just below them
PNA_CASES = [(128, 2_300_000, 0), (128, T21 - 5000, 0), (128, 2_300_000, 3), (256, 1_100_000, 0), (256, T20 - 5000, 0)]


@pytest.mark.parametrize("hidden,nodes,math", PNA_CASES, ids=[f"F{c[0]}-{c[1]}-math{c[2]}" for c in PNA_CASES])
def test_pna_degree_classes(hidden, nodes, math):
    """The C4 set-up (bench.py: 3 layers, QM9-shaped graphs, both promises, classes / pagg / first at their defaults) with the
    hub graph across 2^21 (F = 128) or 2^20 (F = 256).  Which PNA form ran is not reported (``last_path`` says ``layerwise``
    for both), so it is read from the bits of the same forward with ``pna_classes = 0`` (the general form): other bits below
    the limit -- the degree-class form ran --, the same bits past it at F = 128, where layer 0 runs in k_pna_first and layers 1
    and 2 are past the limit.  (At F = 256 k_pna_first declines -- it takes 64 or 128 outputs -- and layer 0, 11 wide, runs
    the class form far inside its limit: the bits differ there, and the budget alone speaks for layers 1 and 2.)  The general
    form's run is compared by its bits only: it is held to the budget where it is the route (past the limit), and on these
    uniform inputs a PNA std can land next to PyG's 1e-5 variance threshold, where it jumps (tests/helpers.grid_features)."""
    model = make_model("pna", in_dim=11, hidden=hidden, layers=3, act="relu", task_out=3, seed=hidden + math)
    t = T21 if hidden == 128 else T20
    batch = huge_batch(nodes, hidden, place=[(t, HUB, 14)] if nodes > t else [])
    maxdeg = int(np.bincount(batch.coo[:, 1]).max())
    assert maxdeg <= 15
    x = huge_x(batch.num_nodes, 11, nodes, dev_())
    promise = int(np.diff(batch.node_ptr).max())
    got, _ = check_forward(f"large pna F{hidden} math{math}", model, batch, x, promise=promise, maxdeg=maxdeg, math=math)
    general, _ = check_forward(None, model, batch, x, promise=promise, maxdeg=maxdeg, math=math, pna_classes=0)
    below = batch.num_nodes * 16 * hidden + 512 < GIB4  # (gnnb_forward.hip pna_layer: the class form's condition)
    assert below == (nodes < t)
    if below:
        assert not np.array_equal(got, general), "the degree-class form did not run below its limit"
    elif hidden == 128:
        assert np.array_equal(got, general), "the degree-class form ran past its limit"


# --------------------------------------------------------------------------- gnnb_aggregate past 2^23 nodes
@pytest.fixture(scope="module")
def big_batch():
    """8.5M nodes of molecules (past 2^23), the hub graph across node 2^23."""
    b = huge_batch(8_500_000, 23, place=[(T23, HUB, 14)])
    k = int(np.searchsorted(b.node_ptr, T23, "right")) - 1
    assert b.node_ptr[k] < T23 < b.node_ptr[k + 1]
    return b


@pytest.fixture(scope="module")
def big_workspaces(big_batch):
    """(GCN workspace?, agg_balance) -> a CompiledModel with the batch prepared."""
    b = big_batch
    out = {}
    _, coo, nptr, eptr = to_dev(b, dev_())
    for conv in ("gcn", "gin"):
        for bal in (0, 1):
            cm = runtime.CompiledModel.from_model(make_model(conv, in_dim=4, hidden=8, layers=1, out_dim=8, task_out=2, mlp_layers=1),
                                                  b.num_graphs, b.num_nodes, b.num_edges)
            with options(agg_balance=bal):
                cm.graph_prep(coo, nptr, eptr, b.num_nodes)
            out[(conv == "gcn", bal)] = cm
    yield out
    for cm in out.values():
        cm.close()


AGG_KINDS = (("gcn", True), ("gcn", False), ("sum", False), ("mean", False), ("simple", False))


@pytest.mark.parametrize("width", [20, 100, 252, 64, 128])
@pytest.mark.parametrize("kind,gcn_ws", AGG_KINDS, ids=[f"{k}-{'gcn_ws' if g else 'other_ws'}" for k, g in AGG_KINDS])
def test_aggregate_past_2_23_nodes(kind, gcn_ws, width, big_batch, big_workspaces):
    """The ring aggregate's lean path (widths 20 / 100 / 252 need all 32 bits of an LDS address product; 64 / 128 are
    controls) and the register-gather form (64 / 128), on both aggregate forms and both balances, checked at every row of
    the sampled graphs."""
    b = big_batch
    eps = 0.25 if kind == "sum" else 0.0
    x = huge_x(b.num_nodes, width, width, dev_())
    rows = sub_batch(b, sample_graphs(b, width, nodes=[T23]))[1]
    coo = R.workspace_edges(b.coo, gcn_ws)
    ref = R.agg_rows64(kind, coo, b.num_nodes, rows, lambda ids: rows_of(x, ids), eps=eps)
    base = R.agg_rows64(kind, coo, b.num_nodes, rows, lambda ids: rows_of(x, ids), eps=eps, dtype=np.float32)
    out = nan((b.num_nodes, width))
    for form in (0, 1):
        for bal in (0, 1):
            out.fill_(float("nan"))
            with options(agg_form=form, agg_balance=bal):  # (read at graph prep for the cut table AND at launch, which uses it)
                big_workspaces[(gcn_ws, bal)].aggregate(kind, x, eps=eps, out=out)
            big_workspaces[(gcn_ws, bal)].check()
            record(f"large aggregate {kind} w{width} form{form}", rows_of(out, rows), ref, base)


def test_global_pool_past_4_gib(big_batch, big_workspaces):
    b = big_batch
    d = 132
    x = huge_x(b.num_nodes, d, 5, dev_())
    assert x.numel() * 4 > GIB4
    pools = ("add", "mean", "max")
    cm = big_workspaces[(False, 0)]
    got = cm.global_pool(x, list(pools), out=nan((b.num_graphs, 3 * d))).cpu().numpy()
    gids = sample_graphs(b, 6, nodes=[T23, GIB4 // (4 * d)])
    s, rows = sub_batch(b, gids)
    xs = rows_of(x, rows)
    ref = R.pool64(xs, s, pools)
    base = np.concatenate([_pool32(xs, s, p) for p in pools], 1)
    record("large global_pool", got[gids], ref, base)


def _pool32(x, batch, p):
    """fp32 pooling, rows summed in order."""
    out = np.zeros((batch.num_graphs, x.shape[1]), np.float32)
    for g in range(batch.num_graphs):
        rows = x[batch.node_ptr[g]:batch.node_ptr[g + 1]]
        if len(rows):
            s = np.cumsum(rows, 0, dtype=np.float32)[-1]
            out[g] = {"add": s, "max": rows.max(0), "mean": s / np.float32(len(rows))}[p]
    return out


# --------------------------------------------------------------------------- whole forwards past 2^23 nodes (controls)
# (conv, hidden, layers, max_graph_nodes promise, route): the stack kernels keep a workgroup's run of the tile table on chip
# (gnnb_stack_plan.h ZF_TCAP, G2_TCAP: test_stack_at_its_tile_capacity); past that they decline
# before anything is enqueued and the forward runs layer by layer -- which must then be right too
FORWARDS = [("gcn", 128, 2, 29, "layerwise"), ("gin", 128, 3, 29, "layerwise"), ("gcn", 100, 2, 0, "layerwise"), ("sage", 100, 2, 0, "layerwise")]


@pytest.mark.parametrize("conv,hidden,layers,promise,want", FORWARDS, ids=[f"{c[0]}-h{c[1]}-promise{c[3]}" for c in FORWARDS])
def test_forward_past_2_23_nodes(conv, hidden, layers, promise, want, big_batch):
    """The 2-layer GCN and the GIN stack with the promise that selects stack_zf / stack on small batches, and layer by layer GCN
    and SAGE at hidden 100 (the ring aggregate at a width that is not a multiple of 64, inside a forward)."""
    b = big_batch
    model = make_model(conv, in_dim=11, hidden=hidden, layers=layers, act="relu", task_out=5, seed=hidden + layers)
    assert promise == 0 or promise >= int(np.diff(b.node_ptr).max())
    check_forward(f"large {want} {conv}", model, b, huge_x(b.num_nodes, 11, hidden, dev_()), promise=promise, want=want)


def _stack_candidates(conv):
    """Batch sizes at the stack kernels' tile capacity on this device, largest first (gnnb_runtime.hip graph prep;
    gnnb_stack_plan.h ZF_TCAP, G2_TCAP).  Promise 29, in_dim 11: k_gcn2_zf takes its 176-row stages and 128-row tiles, at most 62
    tiles per workgroup and one workgroup per CU; k_gcn2_fused 32-row tiles, at most 63 per workgroup, one or two workgroups
    per CU (its occupancy) -- both are tried, the larger first."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if conv == "gcn":
        return [int(0.97 * 62 * cus * 128)]
    return [int(0.97 * 63 * cus * blocks * 32) for blocks in (2, 1)]


@pytest.mark.parametrize("conv,layers,want", [("gcn", 2, "stack_zf"), ("gin", 3, "stack")])
def test_stack_at_its_tile_capacity(conv, layers, want):
    """The stack kernels at the largest batch they take (about 2M nodes for stack_zf, 0.5M or 1M for the GIN stack on an
    MI355X): their graph-local and stage-relative index arithmetic where it spans the most tiles.  Every size tried is
    checked, whichever route it takes; one must take the stack."""
    model = make_model(conv, in_dim=11, hidden=128, layers=layers, act="relu", task_out=5, seed=layers)
    paths = []
    for nodes in _stack_candidates(conv):
        batch = huge_batch(nodes, layers, place=[(nodes // 2, HUB, 14)])
        assert int(np.diff(batch.node_ptr).max()) <= 29
        _, path = check_forward(f"large {want} {conv}", model, batch, huge_x(batch.num_nodes, 11, nodes, dev_()), promise=29,
                                want=None)
        paths.append((batch.num_nodes, path))
        if path == want:
            break
    assert paths[-1][1] == want, paths


# --------------------------------------------------------------------------- gnnb_linear past 4 GiB
FAMILIES = {"wlds": {}, "reg": {"gemm_wlds": 0}, "dma_tail2": {"gemm_variant": 1}, "dma_tail1": {"gemm_variant": 1, "gemm_tail_split": 1},
            "dma_tail0": {"gemm_variant": 1, "gemm_tail_split": 0}, "generic": {"gemm_variant": 1, "gemm_dma": 0}}


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("segments", ["one", "two"])
def test_linear_past_4_gib(family, segments):
    """M = 9M rows at K = 128: A holds 4.6 GB (row 2^23 starts at 4 GiB); ``two``: a second segment of K = 64, row-scaled, in
    the same buffer behind the first, so it starts past 4 GiB.  Checked at rows on both sides of 4 GiB, the last tile, and
    256 seeded random rows."""
    M, K0, K1, N = 9_000_000, 128, 64, 64
    g = np.random.default_rng(len(family) + len(segments))
    buf = huge_x(M * (K0 + (K1 if segments == "two" else 0)), 1, 77, dev_()).view(-1)
    a0 = buf[:M * K0].view(M, K0)
    segs = [(a0, None)]
    if segments == "two":
        a1 = buf[M * K0:].view(M, K1)
        assert a1.data_ptr() - buf.data_ptr() > GIB4
        segs.append((a1, (torch.rand(M, device=dev_()) + 0.5)))
    K = sum(a.shape[1] for a, _ in segs)
    w = (g.uniform(-1, 1, (N, K)) / np.sqrt(K)).astype(np.float32)
    bias = g.uniform(-0.5, 0.5, N).astype(np.float32)
    out = nan((M, N))
    with options(**FAMILIES[family]):
        runtime.linear(segs, torch.from_numpy(w).to(dev_()), torch.from_numpy(bias).to(dev_()), act="tanh", out=out)
    torch.cuda.synchronize()
    r4 = GIB4 // (4 * K0)
    rows = np.unique(np.concatenate([[0, r4 - 1, r4, r4 + 1], np.arange(M - 130, M), g.integers(0, M, 256)]))
    ref = R.linear64(segs, w, bias, act="tanh", rows=rows)
    base = R.linear64(segs, w, bias, act="tanh", dtype=torch.float32, rows=rows)
    record(f"large linear {family}", rows_of(out, rows), ref, base)
