"""GATv2 models with edge features on the MI355X (include/gnnb_gat_edge.h; csrc/k_gatv2_edge.hip): the fused attention aggregate
with the edge projection as a stage entry, the self loop's mean attribute, its epilogue, its bits, whole models through
``forward_edges`` and ``forward_pyg_edges``, the promises, a captured forward, and the refusals.

Acceptance is ``ref64.budget`` with the project's K = 4, F = 2^-22 -- no tolerance of this file's own -- per
in-degree class (``gine_util.budget_by_degree``), nothing left out of a comparison.  The reference is float64 (``gatv2e_util.
gatv2e_ref``: an explicit per-destination attribute mean and an explicit two-pass softmax; whole models: the model's own torch
definition on a ``.double()`` copy); ``base`` is the same in fp32 on the CPU.  The stage's operands lie on dyadic grids on which
every non-self score ("flat") or every score ("steep") is exact in fp32 -- ASSERTED on the reference alone.  Worst e / e32 per
entry go to GNNB_FP64_REPORT=<file>."""
import json
import os
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import ref64 as R
from gatv2_util import gatv2_ref, make_gatv2_model
from gatv2e_util import SLOPE, assert_exact_scores, edge_case, gatv2e_ref, make_gatv2e_model
from gine_util import budget_by_degree, edge_attrs, forward64, run
from gnnbuilder_amd import runtime, synthetic
from gnnbuilder_amd.batching import from_pyg_batch, pack_graphs
from helpers import EMPTY, ONE, batch_vector, edge_batch, looped_graph, make_model, sweep_batch, to_dev

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope="module")
def dev():
    runtime.load_library(require_gpu=True)  # fails loudly: no fallback
    yield torch.device("cuda:0")
    report = os.environ.get("GNNB_FP64_REPORT")
    if report:
        have = {}
        if os.path.exists(report):
            with open(report) as f:
                have = json.load(f)
        have.update(WORST)
        with open(report, "w") as f:
            json.dump(dict(sorted(have.items())), f, indent=1)


def record_classes(entry, got, ref, base, coo):
    for name, r in budget_by_degree(got, ref, base, coo, what=entry).items():
        WORST[f"{entry}/{name}"] = max(WORST.get(f"{entry}/{name}", 0.0), r)


def record(entry, got, ref, base):
    e, e32, _ = R.errors(got, ref, base)
    print(f"{entry}: e = {e:.3e}, e32 = {e32:.3e}, e / e32 = {R.ratio(e, e32):.2f}")
    R.budget(got, ref, base, what=entry)
    WORST[entry] = max(WORST.get(entry, 0.0), R.ratio(e, e32))


def misses_the_budget(wrong, ref, base):
    """Would ``wrong`` in place of the kernel's result fail ``ref64.budget``?  (The gap assertions, on the references alone.)"""
    e, e32, _ = R.errors(wrong, ref, base)
    return e > R.K * e32 + R.F


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _offset(a, dev):
    """``a`` as a contiguous CUDA tensor that starts one float past a 16-byte boundary of its buffer."""
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32))
    buf = torch.zeros(t.numel() + 4, dtype=torch.float32, device=dev)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _workspace(batch, slack=1):
    """A GCN workspace for the stage entry (graph prep drops explicit (v, v) edges there; its tables do not depend on the model
    otherwise): of exactly the batch's size, or ``slack`` times as large."""
    return runtime.CompiledModel.from_model(make_model("gcn", in_dim=8, hidden=8, layers=1, out_dim=8), slack * batch.num_graphs,
                                            slack * max(batch.num_nodes, 1), slack * batch.num_edges)


def _prep(cm, batch, dev):
    _, cood, nptr, eptr = to_dev(batch, dev)
    cm.graph_prep(cood, nptr, eptr, batch.num_nodes)


# ---------------------------------------------------------------------------------------------------- 1. the stage against float64
BATCHES, PREPARED, CASES = {}, {}, {}


def _batch(kind, w):
    if (kind, w) not in BATCHES:
        BATCHES[kind, w] = edge_batch(8, w, seed=21) if kind == "edge" else sweep_batch(24, w, seed=5)[0]
    return BATCHES[kind, w]


def _prepared(kind, w, dev):
    """One prepared workspace per batch, shared by the tests of this file (nothing below changes its tables)."""
    if (kind, w) not in PREPARED:
        cm = _workspace(_batch(kind, w))
        _prep(cm, _batch(kind, w), dev)
        PREPARED[kind, w] = cm
    return PREPARED[kind, w]


def _refs(kind, width, heads, d, operands):
    """The operands of one stage case and its references, computed once and shared (never changed): dict with ``c`` (operands),
    ``ref`` / ``base`` (with bias, no skip, no activation), ``coo`` (the workspace's edges), ``deg``."""
    key = (kind, width, heads, d, operands)
    if key not in CASES:
        b = _batch(kind, width)
        c = edge_case(b.coo, b.num_nodes, width, heads, d, operands)
        coo = R.workspace_edges(b.coo, True)  # (the tables hold no explicit self loop; the layer adds one per node)
        args = (c["xl"], c["xr"], c["att"], c["bias"], None, "none", b.coo, c["edge_attr"], c["w_edge"], heads, SLOPE)
        CASES[key] = dict(c=c, coo=coo, deg=np.bincount(coo[:, 1], minlength=b.num_nodes), ref=gatv2e_ref(*args), base=gatv2e_ref(*args, np.float32))
    return CASES[key]


SHAPES = [(32, 1), (32, 4), (9, 3), (130, 2), (24, 2), (256, 8)]  # (width, heads): C = 32, 8, 3 (scalar), 65 (scalar, two strides), 12 (3 lanes of 4), 32
EDGE_DIMS = (1, 3, 4, 16)
# the covering set: every edge_dim at (32, 4) and (9, 3) -- the 16-byte and the scalar form --, every shape at edge_dim 4
STAGE = [(w, h, d) for w, h in SHAPES for d in EDGE_DIMS if d == 4 or (w, h) in ((32, 4), (9, 3))]


def _stage(cm, c, dev, heads, bias=True, skip=False, act="none", place=_t):
    return cm.aggregate_gatv2_edges(place(c["xl"], dev), place(c["xr"], dev), _t(c["att"], dev), place(c["edge_attr"], dev), place(c["w_edge"], dev),
                                    bias=_t(c["bias"], dev) if bias else None, skip=place(c["skip"], dev) if skip else None, act=act,
                                    heads=heads, negative_slope=SLOPE)


@pytest.mark.parametrize("operands", ["flat", "steep"])
@pytest.mark.parametrize("kind", ["edge", "sweep"])
@pytest.mark.parametrize("width,heads,d", STAGE)
def test_stage_against_float64(dev, width, heads, d, kind, operands):
    b = _batch(kind, width)
    r = _refs(kind, width, heads, d, operands)
    c, coo, deg = r["c"], r["coo"], r["deg"]
    # the hub (in-degree >= 1200 in the batch, a few explicit self loops fewer in the tables): a row split over the workgroup;
    # rows without in-edges
    assert np.bincount(b.coo[:, 1]).max() >= 1200 and deg.max() >= 1150 and (deg == 0).any()
    dst, s64, _ = assert_exact_scores(c, b.coo, heads, operands)
    if operands == "steep":
        big = np.zeros((b.num_nodes, heads))
        np.maximum.at(big, dst, np.abs(s64))
        assert (big.max(1) > 200.0).sum() >= 100  # exp without the max subtraction overflows there
    cm = _prepared(kind, width, dev)
    got = _stage(cm, c, dev, heads)
    cm.check()
    got = got.cpu().numpy()
    assert got.shape == (b.num_nodes, width) and np.isfinite(got).all()
    assert np.array_equal(got[deg == 0], (c["xl"] + c["bias"])[deg == 0])  # in-degree 0: xl_i + bias, bit for bit
    record_classes(f"aggregate_gatv2_edges/{kind}-w{width}-h{heads}-d{d}-{operands}", got, r["ref"], r["base"], coo)


@pytest.mark.parametrize("d", [3, 4])
def test_every_operand_one_float_off_alignment(dev, d):
    """Width 32, heads 4: xl, xr, skip, out, edge_attr and w_edge all start 4 bytes past a 16-byte boundary -- the scalar form, and
    the attribute rows in single floats at edge_dim 4 too."""
    width, heads = 32, 4
    b = _batch("edge", width)
    r = _refs("edge", width, heads, d, "flat")
    c = r["c"]
    cm = _prepared("edge", width, dev)
    out = _offset(np.zeros((b.num_nodes, width), np.float32), dev)
    got = cm.aggregate_gatv2_edges(_offset(c["xl"], dev), _offset(c["xr"], dev), _t(c["att"], dev), _offset(c["edge_attr"], dev),
                                   _offset(c["w_edge"], dev), bias=_t(c["bias"], dev), heads=heads, negative_slope=SLOPE, out=out)
    cm.check()
    assert got.data_ptr() == out.data_ptr()
    got = got.cpu().numpy()
    assert np.array_equal(got[r["deg"] == 0], (c["xl"] + c["bias"])[r["deg"] == 0])
    record_classes(f"aggregate_gatv2_edges/edge-w{width}-h{heads}-d{d}-offset", got, r["ref"], r["base"], r["coo"])


@pytest.mark.parametrize("width,heads,d", [(32, 4, 4), (9, 3, 3), (130, 2, 16)])
def test_zero_edge_weights_give_the_layer_without_edge_features(dev, width, heads, d):
    b = _batch("edge", width)
    c = dict(_refs("edge", width, heads, d, "flat")["c"])
    c["w_edge"] = np.zeros_like(c["w_edge"])
    coo = R.workspace_edges(b.coo, True)
    ref = gatv2_ref(c["xl"], c["xr"], c["att"], c["bias"], None, "none", b.coo, heads, SLOPE)
    base = gatv2_ref(c["xl"], c["xr"], c["att"], c["bias"], None, "none", b.coo, heads, SLOPE, np.float32)
    cm = _prepared("edge", width, dev)
    got = _stage(cm, c, dev, heads)
    cm.check()
    record_classes(f"aggregate_gatv2_edges/edge-w{width}-h{heads}-d{d}-we0", got.cpu().numpy(), ref, base, coo)


@pytest.mark.parametrize("width,heads,d", [(32, 4, 4), (9, 3, 3), (130, 2, 16)])
def test_zero_attention_is_the_mean_over_the_closed_neighbourhood(dev, width, heads, d):
    b = _batch("edge", width)
    c = dict(_refs("edge", width, heads, d, "flat")["c"])
    c["att"] = np.zeros(width, np.float32)
    coo = R.workspace_edges(b.coo, True)
    cnt = 1.0 + np.bincount(coo[:, 1], minlength=b.num_nodes)

    def mean(dtype):
        acc = np.zeros_like(c["xl"], dtype=dtype)  # (the in-edges in slot order, then the self term)
        np.add.at(acc, coo[:, 1], c["xl"].astype(dtype)[coo[:, 0]])
        return (acc + c["xl"].astype(dtype)) / cnt.astype(dtype)[:, None] + c["bias"].astype(dtype)

    cm = _prepared("edge", width, dev)
    got = _stage(cm, c, dev, heads)
    cm.check()
    record_classes(f"aggregate_gatv2_edges/edge-w{width}-h{heads}-d{d}-att0", got.cpu().numpy(), mean(np.float64), mean(np.float32), coo)


@pytest.mark.parametrize("width,heads,d", [(32, 4, 4), (9, 3, 1), (32, 1, 4)])
def test_the_edge_term_is_not_ignored(dev, width, heads, d):
    """A kernel that dropped the edge term would compute the layer without edge features: that result misses the budget (asserted
    on the references), the kernel's meets it."""
    b = _batch("edge", width)
    r = _refs("edge", width, heads, d, "flat")
    c = r["c"]
    without = gatv2_ref(c["xl"], c["xr"], c["att"], c["bias"], None, "none", b.coo, heads, SLOPE)
    assert misses_the_budget(without, r["ref"], r["base"])
    has = r["deg"] >= 1
    assert misses_the_budget(without[has], r["ref"][has], r["base"][has])
    cm = _prepared("edge", width, dev)
    got = _stage(cm, c, dev, heads).cpu().numpy()
    cm.check()
    record_classes(f"aggregate_gatv2_edges/edge-w{width}-h{heads}-d{d}-not-ignored", got, r["ref"], r["base"], r["coo"])


@pytest.mark.parametrize("width,heads,d", [(32, 4, 4), (9, 3, 3), (32, 1, 16)])
def test_the_self_loop_attribute_is_the_mean_not_zero(dev, width, heads, d):
    """A kernel that took the self loop's attribute as 0 would compute ``fill = 0``: on the rows of in-degree >= 1 that variant
    misses the budget (asserted on the references, on those rows together and per in-degree class), the kernel's result meets it."""
    from gine_util import degree_classes
    b = _batch("edge", width)
    r = _refs("edge", width, heads, d, "flat")
    c = r["c"]
    zero_fill = gatv2e_ref(c["xl"], c["xr"], c["att"], c["bias"], None, "none", b.coo, c["edge_attr"], c["w_edge"], heads, SLOPE, fill=0)
    has = r["deg"] >= 1
    assert np.array_equal(zero_fill[~has], r["ref"][~has]) and misses_the_budget(zero_fill[has], r["ref"][has], r["base"][has])
    for name, m in degree_classes(r["coo"], b.num_nodes).items():  # (the hub too: its self term is one of > 1150 and still shows)
        assert misses_the_budget(zero_fill[m & has], r["ref"][m & has], r["base"][m & has]), name
    cm = _prepared("edge", width, dev)
    got = _stage(cm, c, dev, heads).cpu().numpy()
    cm.check()
    record_classes(f"aggregate_gatv2_edges/edge-w{width}-h{heads}-d{d}-mean", got, r["ref"], r["base"], r["coo"])
    record(f"aggregate_gatv2_edges/edge-w{width}-h{heads}-d{d}-mean/deg>=1", got[has], r["ref"][has], r["base"][has])


# ---------------------------------------------------------------------------------------------------- 2. the epilogue
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("with_skip", [True, False])
@pytest.mark.parametrize("act", ["relu", "gelu", "sigmoid", "tanh"])
def test_epilogue_bias_skip_and_activation(dev, act, with_skip, with_bias):
    """Width 32, heads 4, edge_dim 4: ``xl`` / ``xr`` as the two halves of one [N, 64] tensor (row stride 64: the vector form)."""
    width, heads, d = 32, 4, 4
    b = _batch("edge", width)
    r = _refs("edge", width, heads, d, "flat")
    c = r["c"]
    bias, skip = (c["bias"] if with_bias else None), (c["skip"] if with_skip else None)
    args = (c["xl"], c["xr"], c["att"], bias, skip, act, b.coo, c["edge_attr"], c["w_edge"], heads, SLOPE)
    ref, base = gatv2e_ref(*args), gatv2e_ref(*args, np.float32)
    cm = _prepared("edge", width, dev)
    both = _t(np.concatenate([c["xl"], c["xr"]], 1), dev)
    assert both.shape == (b.num_nodes, 64) and both[:, 32:].data_ptr() % 16 == 0
    got = cm.aggregate_gatv2_edges(both[:, :32], both[:, 32:], _t(c["att"], dev), _t(c["edge_attr"], dev), _t(c["w_edge"], dev),
                                   bias=None if bias is None else _t(bias, dev), skip=None if skip is None else _t(skip, dev), act=act, heads=heads,
                                   negative_slope=SLOPE)
    cm.check()
    entry = f"aggregate_gatv2_edges/epilogue-{act}" + ("" if with_bias else "-nobias") + ("-skip" if with_skip else "")
    record_classes(entry, got.cpu().numpy(), ref, base, r["coo"])


# ---------------------------------------------------------------------------------------------------- 3. bits
@pytest.mark.parametrize("width,heads,d", [(32, 4, 4), (9, 3, 3), (130, 2, 16)])
def test_a_repeat_launch_and_another_workspace_give_the_same_bits(dev, width, heads, d):
    b = _batch("edge", width)
    c = _refs("edge", width, heads, d, "flat")["c"]
    cm = _prepared("edge", width, dev)
    first = _stage(cm, c, dev, heads, skip=True, act="tanh")
    assert torch.equal(_stage(cm, c, dev, heads, skip=True, act="tanh"), first)
    # the same batch on a workspace with far larger capacities: graph prep cuts other node tiles there.  The kernel's grid is cut
    # from the batch alone (launch_gatv2_edge_aggregate); other grids, with other rows per lane group, are
    # test_many_steps_per_workgroup's
    big = _workspace(b, slack=16)
    _prep(big, b, dev)
    assert torch.equal(_stage(big, c, dev, heads, skip=True, act="tanh"), first)
    cm.check(), big.check()


def _lane_groups(width, heads):
    """Lane groups per 256-lane workgroup of ``launch_gatv2_edge_aggregate`` on aligned operands: an item = (row, head) takes the
    smallest power of two >= C / VEC lanes, at most 64."""
    c = width // heads
    nvec = c // 4 if c % 4 == 0 else c
    lanes = 1
    while lanes < nvec and lanes < 64:
        lanes *= 2
    return 256 // lanes


def _wg_per_cu():
    """``GAE_WG_PER_CU`` of csrc/k_gatv2_edge.hip: the most workgroups per CU the grid is cut for."""
    src = (Path(runtime.CSRC_DIR) / "k_gatv2_edge.hip").read_text()
    return int(re.search(r"constexpr int GAE_WG_PER_CU = (\d+);", src).group(1))


# (width, heads, edge_dim, copies, operand set): the 16-byte form at 8 lanes per item, the scalar form over four strides of a wave,
# the 16-byte form at 32 lanes per item (a wave shuffle in the score sum)
MANY_STEPS = [(256, 8, 4, 8, "flat"), (130, 2, 3, 4, "steep"), (128, 1, 16, 12, "flat")]


@pytest.mark.parametrize("width,heads,d,copies,operands", MANY_STEPS)
def test_many_steps_per_workgroup(dev, width, heads, d, copies, operands):
    """``copies`` copies of the sweep batch in one batch, every copy with the first copy's operand rows: more rows than one sweep
    of the grid can take at ``GAE_WG_PER_CU`` workgroups per CU on this device (ASSERTED), so every lane group walks two rows or
    more -- the three-deep pipeline's rotation, the slot prefetch of the next step, the long rows' second walk at a later step --
    and the last copy's rows, hubs included, are taken at a later step and by another lane group than the first copy's.  All rows
    are held against float64 (a copy's graphs are closed, so its reference is the one batch's); every copy has the first copy's
    bits, and those are the bits of the one batch launched alone on its own, smaller grid."""
    b = _batch("sweep", width)
    n = b.num_nodes
    long = pack_graphs([b.graph(g) for g in range(b.num_graphs)] * copies)
    assert long.num_nodes == copies * n and np.array_equal(long.coo[:b.num_edges], b.coo)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    rows_per_sweep = _wg_per_cu() * cus * _lane_groups(width, heads) // heads  # (at most: a lane group keeps one head)
    assert long.num_nodes > rows_per_sweep  # two sweeps or more
    assert (copies - 1) * n >= -(-long.num_nodes // 2)  # the last copy begins behind the first sweep
    r = _refs("sweep", width, heads, d, operands)
    c = r["c"]
    assert_exact_scores(c, b.coo, heads, operands)
    tiled = {k: (np.tile(v, (copies, 1)) if k in ("xl", "xr", "skip", "edge_attr") else v) for k, v in c.items()}
    cl = _workspace(long)
    _prep(cl, long, dev)
    got = _stage(cl, tiled, dev, heads)
    cl.check()
    alone = _stage(_prepared("sweep", width, dev), c, dev, heads)
    assert torch.equal(got[:n], alone)
    for k in range(1, copies):
        assert torch.equal(got[k * n:(k + 1) * n], got[:n]), k
    coo = R.workspace_edges(long.coo, True)
    assert np.bincount(coo[:, 1], minlength=long.num_nodes)[(copies - 1) * n:].max() >= 1150  # (a hub in the last copy)
    record_classes(f"aggregate_gatv2_edges/sweep-x{copies}-w{width}-h{heads}-d{d}-{operands}", got.cpu().numpy(), np.tile(r["ref"], (copies, 1)),
                   np.tile(r["base"], (copies, 1)), coo)


@pytest.mark.parametrize("d", [3, 4])
def test_explicit_self_loops_with_nan_attributes_give_the_bits_of_the_batch_without_them(dev, d):
    width, heads = 24, 2
    x, coo = looped_graph(40, width, seed=3)
    assert (coo[:, 0] == coo[:, 1]).sum() >= 10
    others = [ONE(width), (x[:7], np.array([[0, 1], [1, 0], [2, 1], [5, 1]], np.int32))]
    with_loops = pack_graphs([(x, coo)] + others)
    keep = with_loops.coo[:, 0] != with_loops.coo[:, 1]
    without = pack_graphs([(x, coo[coo[:, 0] != coo[:, 1]])] + others)
    assert with_loops.num_edges > without.num_edges and np.array_equal(with_loops.coo[keep], without.coo)
    c = edge_case(with_loops.coo, with_loops.num_nodes, width, heads, d, "flat")
    c["edge_attr"][~keep] = np.nan  # dropped with their edges: never read, never part of a mean
    outs = []
    for b, ea in ((with_loops, c["edge_attr"]), (without, c["edge_attr"][keep])):
        cm = _workspace(b)
        _prep(cm, b, dev)
        outs.append(_stage(cm, dict(c, edge_attr=np.ascontiguousarray(ea)), dev, heads))
        cm.check()
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
    args = (c["xl"], c["xr"], c["att"], c["bias"], None, "none", with_loops.coo, c["edge_attr"], c["w_edge"], heads, SLOPE)
    record(f"aggregate_gatv2_edges/looped-d{d}", outs[0].cpu().numpy(), gatv2e_ref(*args), gatv2e_ref(*args, np.float32))


# ---------------------------------------------------------------------------------------------------- 4. whole models
def _model_batch(graphs, in_dim, seed):
    """``graphs`` synthetic qm9-like graphs with seeded features of width ``in_dim``, an empty and a one-node graph among them"""
    mols, rng = synthetic.make_batch("qm9", graphs, seed=seed), np.random.default_rng(seed)
    gs = [(rng.uniform(-1, 1, (mols.graph(g)[0].shape[0], in_dim)).astype(np.float32), mols.graph(g)[1]) for g in range(graphs)]
    return pack_graphs(gs[:graphs // 2] + [EMPTY(in_dim), ONE(in_dim)] + gs[graphs // 2:] + [EMPTY(in_dim)])


def _model(layers, heads, in_dim, hidden, d, seed=0):
    return make_gatv2e_model(in_dim=in_dim, edge_dim=d, hidden=hidden, layers=layers, heads=heads, skip=True, pools=("add", "mean", "max"),
                             mlp_layers=1, out_act=torch.nn.LogSoftmax, seed=seed)


def _compiled(model, b, promise=0, degree=0, ingest=False):
    cm = runtime.CompiledModel.from_model(model, b.num_graphs, b.num_nodes, b.num_edges)
    if ingest:  # (right after construction: before a batch is prepared on the workspace)
        cm.enable_edge_ingest()
    if promise:
        cm.set_max_graph_nodes(promise)
    if degree:
        cm.set_max_degree(degree)
    return cm


@pytest.mark.parametrize("in_dim,hidden,graphs,d", [(9, 32, 64, 4), (11, 128, 12, 3)])
@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("layers", [1, 2, 3])
def test_whole_models_against_float64(dev, layers, heads, in_dim, hidden, graphs, d):
    model = _model(layers, heads, in_dim, hidden, d, seed=layers)
    b = _model_batch(graphs, in_dim, seed=31 + layers)
    ea = edge_attrs(b.num_edges, d, seed=32 + layers)
    assert b.num_graphs == graphs + 3
    cm = _compiled(model, b)
    assert cm.lib.gnnb_model_gat_heads(cm._model) == heads and cm.lib.gnnb_model_edge_dim(cm._model) == d
    xd, cood, nptr, eptr = to_dev(b, dev)
    ead = _t(ea, dev)
    out = cm.forward_edges(xd, ead, cood, nptr, eptr)
    cm.check()
    assert cm.last_path() == "layerwise" and out.shape == (b.num_graphs, 19)
    record(f"forward_edges/gatv2e-L{layers}-h{heads}-in{in_dim}-w{hidden}-d{d}", out.cpu().numpy(), forward64(model, b, b.x, ea), run(model, b, b.x, ea))
    # the same forward again, and the prepared form, give the same bits (no atomics, a fixed summation order)
    assert torch.equal(cm.forward_edges(xd, ead, cood, nptr, eptr), out)
    assert torch.equal(cm.forward_prepared_edges(xd, ead), out)


@pytest.fixture(scope="module")
def pyg():
    """A 300-graph batch (two radix passes), in 11, edge_dim 4, grouped and with edges + edge_attr rows under one seeded permutation."""
    b = synthetic.make_batch("qm9", 300, seed=41)
    rng = np.random.default_rng(42)
    x = rng.uniform(-1, 1, (b.num_nodes, 11)).astype(np.float32)
    ei = np.ascontiguousarray(b.coo.T.astype(np.int64))
    ea = edge_attrs(b.num_edges, 4, seed=43)
    perm = rng.permutation(b.num_edges)
    model = make_gatv2e_model(in_dim=11, edge_dim=4, hidden=32, layers=2, heads=4, seed=3)
    cm = runtime.CompiledModel.from_model(model, 512, 16384, 32768)
    cm.enable_edge_ingest()
    return dict(b=b, x=x, ei=ei, ea=ea, ei_sh=np.ascontiguousarray(ei[:, perm]), ea_sh=np.ascontiguousarray(ea[perm]), cm=cm, model=model,
                batch=batch_vector(b))


def test_pyg_batches_grouped_and_shuffled(pyg, dev):
    cm, model = pyg["cm"], pyg["model"]
    xd, batch_dev = _t(pyg["x"], dev), _t(pyg["batch"], dev)
    for kind, ei, ea in (("grouped", pyg["ei"], pyg["ea"]), ("shuffled", pyg["ei_sh"], pyg["ea_sh"])):
        gb, ea_ord = from_pyg_batch(pyg["x"], ei, edge_attr=ea, batch=pyg["batch"], num_graphs=300)
        out = cm.forward_pyg_edges(xd, _t(ei, dev), _t(ea, dev), batch=batch_dev, num_graphs=300).clone()
        cm.check()
        assert cm.last_path() == "layerwise"
        record(f"forward_pyg_edges/gatv2e-{kind}", out.cpu().numpy(), forward64(model, gb, pyg["x"], ea_ord), run(model, gb, pyg["x"], ea_ord))
        host = cm.forward_edges(xd, _t(ea_ord, dev), _t(gb.coo, dev), _t(gb.node_ptr, dev), _t(gb.edge_ptr, dev))
        assert torch.equal(out, host)  # (the ingest's arrays are the host's, so are the bits)


def test_promises_change_neither_the_path_nor_a_bit(dev):
    model = _model(3, 4, 9, 32, 4, seed=5)
    b = _model_batch(12, 9, seed=23)
    ea = edge_attrs(b.num_edges, 4, seed=24)
    assert np.diff(b.node_ptr).max() <= 64 and np.bincount(b.coo[:, 1]).max() <= 15
    xd, cood, nptr, eptr = to_dev(b, dev)
    outs = []
    for promise, degree in ((0, 0), (64, 0), (0, 15), (64, 15)):
        cm = _compiled(model, b, promise, degree)
        outs.append(cm.forward_edges(xd, _t(ea, dev), cood, nptr, eptr))
        cm.check()  # (the promises hold)
        assert cm.last_path() == "layerwise"
    assert all(torch.equal(o, outs[0]) for o in outs[1:])
    record("forward_edges/gatv2e-L3-h4-promises", outs[-1].cpu().numpy(), forward64(model, b, b.x, ea), run(model, b, b.x, ea))


def test_a_captured_forward_replays_with_the_eager_bits(dev):
    model = _model(3, 4, 9, 32, 4, seed=6)
    b = _model_batch(12, 9, seed=24)
    ea = edge_attrs(b.num_edges, 4, seed=25)
    cm = _compiled(model, b)
    xd, cood, nptr, eptr = to_dev(b, dev)
    ead = _t(ea, dev)
    eager = cm.forward_edges(xd, ead, cood, nptr, eptr).clone()  # (also the warm-up outside the capture: kernel attributes, caches)
    out = torch.zeros_like(eager)
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        cm.forward_edges(xd, ead, cood, nptr, eptr, out=out)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    x2 = np.random.default_rng(2).uniform(-1, 1, b.x.shape).astype(np.float32)  # fresh features and attributes in the captured buffers
    ea2 = edge_attrs(b.num_edges, 4, seed=26)
    xd.copy_(torch.from_numpy(x2)), ead.copy_(torch.from_numpy(ea2))
    graph.replay()
    torch.cuda.synchronize()
    record("forward_edges/gatv2e-captured", out.cpu().numpy(), forward64(model, b, x2, ea2), run(model, b, x2, ea2))
    cm.check()


# ---------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals(dev):
    model = _model(2, 4, 9, 32, 4)
    b = _model_batch(12, 9, seed=25)
    cm = _compiled(model, b)
    xd, cood, nptr, eptr = to_dev(b, dev)
    ea = _t(edge_attrs(b.num_edges, 4, seed=27), dev)
    good = cm.forward_edges(xd, ea, cood, nptr, eptr).clone()
    ei, batch_dev = _t(np.ascontiguousarray(b.coo.T.astype(np.int64)).reshape(2, -1), dev), _t(batch_vector(b), dev)
    # the entries without edge attributes refuse the model, and name the entry that takes them
    with pytest.raises(runtime.GnnbError, match="gnnb_forward_batched_edges"):
        cm.forward(xd, cood, nptr, eptr)
    with pytest.raises(runtime.GnnbError, match="gnnb_forward_prepared_edges"):
        cm.forward_prepared(xd)
    ingest = _compiled(model, b, ingest=True)  # (gnnb_workspace_enable_edge_ingest accepts the workspace)
    with pytest.raises(runtime.GnnbError, match="gnnb_forward_pyg_edges"):
        ingest.forward_pyg(xd, ei, batch=batch_dev, num_graphs=b.num_graphs)
    assert torch.equal(ingest.forward_pyg_edges(xd, ei, ea, batch=batch_dev, num_graphs=b.num_graphs), good)
    ordered = _compiled(model, b)
    ordered.enable_ordered_ingest()
    with pytest.raises(runtime.GnnbError, match="gnnb_forward_pyg_edges"):
        ordered.forward_pyg_ordered(xd, ei, batch=batch_dev, num_graphs=b.num_graphs)
    # a model does not run on the workspace of one with another edge_dim, other heads, another slope, or none of them
    N, E = b.num_nodes, b.num_edges
    for other_model, ea_w in ((_model(2, 4, 9, 32, 3), 3), (_model(2, 2, 9, 32, 4), 4), (make_gatv2_model(in_dim=9, hidden=32, layers=2, heads=4, mlp_layers=1, out_act=torch.nn.LogSoftmax), 4)):
        other = _compiled(other_model, b)
        assert bytes(cm.desc) == bytes(other.desc)
        other.graph_prep(cood, nptr, eptr, N)
        assert cm.lib.gnnb_forward_prepared_edges(cm._model, other._ws, xd.data_ptr(), ea.data_ptr(), good.data_ptr(), None) == -1
        assert b"different model" in cm.lib.gnnb_last_error()
    slope = make_gatv2e_model(in_dim=9, edge_dim=4, hidden=32, layers=2, heads=4, mlp_layers=1, out_act=torch.nn.LogSoftmax)
    for conv in slope.gnn_convs:
        conv.negative_slope = conv.conv.negative_slope = 0.1
    other = _compiled(slope, b)
    other.graph_prep(cood, nptr, eptr, N)
    assert cm.lib.gnnb_forward_prepared_edges(cm._model, other._ws, xd.data_ptr(), ea.data_ptr(), good.data_ptr(), None) == -1
    assert b"different model" in cm.lib.gnnb_last_error()
    # edge_attr of another shape, dtype or device is refused before any launch
    for bad, what in ((ea[:-1], "edge_attr must be"), (torch.zeros((E, 5), device=dev), "edge_attr has shape"), (ea.double(), "float32"),
                      (ea.cpu(), "CUDA"), (None, "edge_attr is required")):
        with pytest.raises(runtime.GnnbError, match=what):
            cm.forward_edges(xd, bad, cood, nptr, eptr)
    # the stage entry checks its operands on the host, before any launch
    cm.graph_prep(cood, nptr, eptr, N)
    z = lambda *shape: torch.zeros(shape, device=dev)  # noqa: E731
    with pytest.raises(runtime.GnnbError, match="divisible by heads"):
        cm.aggregate_gatv2_edges(z(N, 30), z(N, 30), z(30), z(E, 4), z(30, 4), heads=4)
    with pytest.raises(runtime.GnnbError, match="at most 256"):
        cm.aggregate_gatv2_edges(z(N, 264), z(N, 264), z(264), z(E, 4), z(264, 4), heads=4)
    for heads in (9, 0):
        with pytest.raises(runtime.GnnbError, match="heads must be"):
            cm.aggregate_gatv2_edges(z(N, 32), z(N, 32), z(32), z(E, 4), z(32, 4), heads=heads)
    for bad, what in ((dict(xr=z(N, 16)), "xr"), (dict(xl=z(N - 1, 32)), "xl"), (dict(att=z(16)), "att must hold"), (dict(bias=z(16)), "bias"),
                      (dict(skip=z(N, 16)), "skip has shape"), (dict(skip=z(N - 1, 32)), "skip must be"), (dict(out=z(N, 16)), "out"), (dict(act="swish"), "act must be"),
                      (dict(xl=z(N, 32).double()), "xl"), (dict(att=z(32).cpu()), "att"), (dict(w_edge=z(32, 17)), "w_edge must be"),
                      (dict(w_edge=z(16, 4)), "w_edge"), (dict(w_edge=z(32, 4).cpu()), "w_edge"), (dict(edge_attr=z(E, 3)), "edge_attr has shape"),
                      (dict(edge_attr=z(E - 1, 4)), "edge_attr must be"), (dict(edge_attr=None), "edge_attr is required"),
                      (dict(edge_attr=z(E, 4).double()), "float32")):
        args = dict(xl=z(N, 32), xr=z(N, 32), att=z(32), edge_attr=z(E, 4), w_edge=z(32, 4), heads=4)
        args.update(bad)
        with pytest.raises(runtime.GnnbError, match=what):
            cm.aggregate_gatv2_edges(args.pop("xl"), args.pop("xr"), args.pop("att"), args.pop("edge_attr"), args.pop("w_edge"), **args)
    # ... and the C entry itself: heads that do not divide the width, width > 256, heads > 8, a stride below the width, edge_dim out
    # of range, ldwe below edge_dim, NULL edge_attr for a batch with edges, a workspace whose tables keep explicit self loops
    xl = z(max(N, E), 264)
    p = xl.data_ptr()
    call = lambda ws, ld, heads, width, ea_ptr=p, ed=4, ldwe=4: cm.lib.gnnb_aggregate_gatv2_edges(  # noqa: E731
        ws, p, ld, p, ld, p, None, None, 4, heads, 0.2, ea_ptr, ed, p, ldwe, p, width, None)
    for ld, heads, width in ((32, 3, 32), (264, 4, 264), (32, 9, 36), (16, 4, 32)):
        assert call(cm._ws, ld, heads, width) == -1 and b"bad argument" in cm.lib.gnnb_last_error()
    for kw in (dict(ed=0), dict(ed=17, ldwe=17), dict(ed=4, ldwe=3), dict(ea_ptr=None)):
        assert E > 0 and call(cm._ws, 32, 4, 32, **kw) == -1 and b"bad argument" in cm.lib.gnnb_last_error()
    gin = runtime.CompiledModel.from_model(make_model("gin", in_dim=9, hidden=8, layers=1, out_dim=8), b.num_graphs, N, E)
    gin.graph_prep(cood, nptr, eptr, N)
    assert call(gin._ws, 32, 4, 32) == -1 and b"GCN workspace" in cm.lib.gnnb_last_error()
    # nothing above left a flag or changed a result
    cm.check()
    assert torch.equal(cm.forward_edges(xd, ea, cood, nptr, eptr), good)
