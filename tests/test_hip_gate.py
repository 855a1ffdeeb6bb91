"""GAT (v1) models with edge features on the MI355X (include/gnnb_gatconv_edge.h; csrc/k_gat_edge.hip): the fused attention
aggregate with the folded edge term as a stage entry, the self loop's mean, its epilogue, its bits, whole models through
``forward_edges`` and ``forward_pyg_edges``, the promises, a captured forward, one workspace across unlike batches, and the
refusals.

Acceptance is ``ref64.budget`` with the project's K = 4, F = 2^-22 -- no tolerance of this file's own -- per
in-degree class (``gine_util.budget_by_degree``), nothing left out of a comparison.  The reference is float64 (``gate_util.
gate_ref``: an explicit per-destination attribute MEAN, projected afterwards -- PyG's order, not the kernel's, which takes the mean
of the projected terms -- and an explicit two-pass softmax; whole models: the model's own torch definition on a ``.double()``
copy); ``base`` is the same in fp32 on the CPU.  The stage's operands lie on dyadic grids on which every non-self score ("flat") or
every score ("steep") is exact in fp32 -- ASSERTED on the reference alone.  Worst e / e32 per entry go to GNNB_FP64_REPORT=<file>
(DESIGN.md section 4)."""
import json
import os
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import ref64 as R
from gat_util import gat_ref, make_gat_model
from gate_util import SLOPE, assert_exact_scores, edge_case, gate_ref, make_gate_model
from gatv2e_util import make_gatv2e_model
from gine_util import budget_by_degree, degree_classes, edge_attrs, forward64, run
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
    """``a`` as a CUDA tensor of unit column stride that starts one float past a 16-byte boundary of its buffer."""
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


def _args(c, coo, heads, bias=True, skip=False, act="none"):
    return (c["xl"], c["s_src"], c["s_dst"], c["a_edge"], c["bias"] if bias else None, c["skip"] if skip else None, act, coo, c["edge_attr"],
            heads, SLOPE)


def _refs(kind, width, heads, d, operands, seed=None):
    """The operands of one stage case and its references, computed once and shared (never changed): dict with ``c`` (operands),
    ``ref`` / ``base`` (with bias, no skip, no activation), ``coo`` (the workspace's edges), ``deg``."""
    key = (kind, width, heads, d, operands, seed)
    if key not in CASES:
        b = _batch(kind, width)
        c = edge_case(b.coo, b.num_nodes, width, heads, d, operands, seed=seed)
        coo = R.workspace_edges(b.coo, True)  # (the tables hold no explicit self loop; the layer adds one per node)
        args = _args(c, b.coo, heads)
        CASES[key] = dict(c=c, coo=coo, deg=np.bincount(coo[:, 1], minlength=b.num_nodes), ref=gate_ref(*args), base=gate_ref(*args, np.float32))
    return CASES[key]


# (width, heads, edge_dim): every edge_dim at (32, 4) -- the 16-byte form -- and (9, 3) -- the scalar form; at edge_dim 4 also
# one head, three strides with the head boundary inside a stride (130, 2), 3 lanes of 4 per head (24, 2), C = 3 at a width that is
# a multiple of 4 (24, 8: must be scalar), a wave per row (256, 8); and a 16-byte attribute piece plus a tail (32, 4, 5)
EDGE_DIMS = (1, 3, 4, 16)
STAGE = ([(w, h, d) for w, h in ((32, 4), (9, 3)) for d in EDGE_DIMS] + [(w, h, 4) for w, h in ((32, 1), (130, 2), (24, 2), (24, 8), (256, 8))] +
         [(32, 4, 5)])


def _stage(cm, c, dev, heads, bias=True, skip=False, act="none", place=_t):
    return cm.aggregate_gat_edges(place(c["xl"], dev), place(c["s_src"], dev), place(c["s_dst"], dev), place(c["edge_attr"], dev),
                                  place(c["a_edge"], dev), bias=_t(c["bias"], dev) if bias else None,
                                  skip=place(c["skip"], dev) if skip else None, act=act, heads=heads, negative_slope=SLOPE)


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
    dst, s64, _ = assert_exact_scores(c, b.coo, operands)
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
    record_classes(f"aggregate_gat_edges/{kind}-w{width}-h{heads}-d{d}-{operands}", got, r["ref"], r["base"], coo)


@pytest.mark.parametrize("d", [3, 4])
def test_every_operand_one_float_off_alignment(dev, d):
    """Width 32, heads 4: xl, s_src, s_dst, skip, out, edge_attr and a_edge all start 4 bytes past a 16-byte boundary -- the scalar
    form, and the attribute rows in single floats at edge_dim 4 too."""
    width, heads = 32, 4
    b = _batch("edge", width)
    r = _refs("edge", width, heads, d, "flat")
    c = r["c"]
    args = _args(c, b.coo, heads, skip=True)
    ref, base = gate_ref(*args), gate_ref(*args, np.float32)
    cm = _prepared("edge", width, dev)
    out = _offset(np.zeros((b.num_nodes, width), np.float32), dev)
    got = cm.aggregate_gat_edges(_offset(c["xl"], dev), _offset(c["s_src"], dev), _offset(c["s_dst"], dev), _offset(c["edge_attr"], dev),
                                 _offset(c["a_edge"], dev), bias=_t(c["bias"], dev), skip=_offset(c["skip"], dev), heads=heads,
                                 negative_slope=SLOPE, out=out)
    cm.check()
    assert got.data_ptr() == out.data_ptr()
    got = got.cpu().numpy()
    assert np.array_equal(got[r["deg"] == 0], ((c["xl"] + c["bias"]) + c["skip"])[r["deg"] == 0])
    record_classes(f"aggregate_gat_edges/edge-w{width}-h{heads}-d{d}-offset", got, ref, base, r["coo"])


@pytest.mark.parametrize("width,heads,d", [(32, 4, 4), (9, 3, 3), (130, 2, 16)])
def test_zero_a_edge_gives_the_layer_without_edge_features(dev, width, heads, d):
    """Not its bits -- the self term moves from first to last --, so the comparison goes through the budget.  On the references
    alone: ``gate_ref`` with a zero ``a_edge`` IS ``gat_ref``."""
    b = _batch("edge", width)
    c = dict(_refs("edge", width, heads, d, "flat")["c"])
    c["a_edge"] = np.zeros_like(c["a_edge"])
    coo = R.workspace_edges(b.coo, True)
    plain = (c["xl"], c["s_src"], c["s_dst"], c["bias"], None, "none", b.coo, heads, SLOPE)
    ref, base = gat_ref(*plain), gat_ref(*plain, np.float32)
    assert np.array_equal(gate_ref(*_args(c, b.coo, heads)), ref) and np.array_equal(gate_ref(*_args(c, b.coo, heads), np.float32), base)
    cm = _prepared("edge", width, dev)
    got = _stage(cm, c, dev, heads)
    cm.check()
    record_classes(f"aggregate_gat_edges/edge-w{width}-h{heads}-d{d}-ae0", got.cpu().numpy(), ref, base, coo)


@pytest.mark.parametrize("width,heads,d", [(32, 4, 4), (9, 3, 1), (32, 1, 16)])
def test_the_edge_term_is_not_ignored(dev, width, heads, d):
    """A kernel that dropped the edge term would compute the layer without edge features: that result misses the budget (asserted
    on the references), the kernel's meets it."""
    b = _batch("edge", width)
    r = _refs("edge", width, heads, d, "flat")
    c = r["c"]
    without = gat_ref(c["xl"], c["s_src"], c["s_dst"], c["bias"], None, "none", b.coo, heads, SLOPE)
    assert misses_the_budget(without, r["ref"], r["base"])
    has = r["deg"] >= 1
    assert misses_the_budget(without[has], r["ref"][has], r["base"][has])
    cm = _prepared("edge", width, dev)
    got = _stage(cm, c, dev, heads).cpu().numpy()
    cm.check()
    record_classes(f"aggregate_gat_edges/edge-w{width}-h{heads}-d{d}-not-ignored", got, r["ref"], r["base"], r["coo"])


@pytest.mark.parametrize("width,heads,d,seed", [(32, 4, 4, None), (9, 3, 3, None), (32, 1, 16, 1)])
def test_the_self_loop_attribute_is_the_mean_not_zero(dev, width, heads, d, seed):
    """A kernel that took the self loop's edge term as 0 would compute ``fill = 0``: on the rows of in-degree >= 1 that variant
    misses the budget (asserted on the references, on those rows together and per in-degree class), the kernel's result meets it.
    (Operand seed 1 at (32, 1, 16), chosen on the CPU: under the default seed the hub's class, where the self term is one of more
    than 1150, stays inside the budget with ``fill = 0``; the kernel plays no part in the choice.)"""
    b = _batch("edge", width)
    r = _refs("edge", width, heads, d, "flat", seed)
    c = r["c"]
    zero_fill = gate_ref(*_args(c, b.coo, heads), fill=0)
    has = r["deg"] >= 1
    assert np.array_equal(zero_fill[~has], r["ref"][~has]) and misses_the_budget(zero_fill[has], r["ref"][has], r["base"][has])
    for name, m in degree_classes(r["coo"], b.num_nodes).items():  # (the hub too: its self term is one of > 1150 and still shows)
        assert misses_the_budget(zero_fill[m & has], r["ref"][m & has], r["base"][m & has]), name
    cm = _prepared("edge", width, dev)
    got = _stage(cm, c, dev, heads).cpu().numpy()
    cm.check()
    record_classes(f"aggregate_gat_edges/edge-w{width}-h{heads}-d{d}-mean", got, r["ref"], r["base"], r["coo"])
    record(f"aggregate_gat_edges/edge-w{width}-h{heads}-d{d}-mean/deg>=1", got[has], r["ref"][has], r["base"][has])


# ---------------------------------------------------------------------------------------------------- 2. the epilogue
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("with_skip", [True, False])
@pytest.mark.parametrize("act", ["relu", "gelu", "sigmoid", "tanh"])
def test_epilogue_bias_skip_and_activation(dev, act, with_skip, with_bias):
    """Width 32, heads 4, edge_dim 4: ``xl``, ``s_src`` and ``s_dst`` as column blocks of one [N, 40] tensor, the layer's GEMM
    output (row stride 40: the vector form)."""
    width, heads, d = 32, 4, 4
    b = _batch("edge", width)
    r = _refs("edge", width, heads, d, "flat")
    c = r["c"]
    args = _args(c, b.coo, heads, bias=with_bias, skip=with_skip, act=act)
    ref, base = gate_ref(*args), gate_ref(*args, np.float32)
    cm = _prepared("edge", width, dev)
    both = _t(np.concatenate([c["xl"], c["s_src"], c["s_dst"]], 1), dev)
    assert both.shape == (b.num_nodes, 40) and both.data_ptr() % 16 == 0
    got = cm.aggregate_gat_edges(both[:, :32], both[:, 32:36], both[:, 36:40], _t(c["edge_attr"], dev), _t(c["a_edge"], dev),
                                 bias=_t(c["bias"], dev) if with_bias else None, skip=_t(c["skip"], dev) if with_skip else None, act=act,
                                 heads=heads, negative_slope=SLOPE)
    cm.check()
    entry = f"aggregate_gat_edges/epilogue-{act}" + ("" if with_bias else "-nobias") + ("-skip" if with_skip else "")
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
    # from the batch alone (launch_gat_edge_aggregate); other grids, with more steps per workgroup, are
    # test_many_steps_per_workgroup's
    big = _workspace(b, slack=16)
    _prep(big, b, dev)
    assert torch.equal(_stage(big, c, dev, heads, skip=True, act="tanh"), first)
    cm.check(), big.check()


@pytest.mark.parametrize("operands", ["flat", "steep"])
@pytest.mark.parametrize("width,heads,d", [(32, 4, 4), (9, 3, 3)])
def test_an_h_head_launch_equals_h_one_head_launches_on_the_column_slices(dev, width, heads, d, operands):
    """A column's bits depend on the batch and on the form only: not on the lane group (8 lanes per row against 2 at width 32, 16
    against 4 at width 9) and not on heads beyond which scalars and which row of ``a_edge`` the column reads."""
    C = width // heads
    c = _refs("edge", width, heads, d, operands)["c"]
    cm = _prepared("edge", width, dev)
    xl, ss, sd, bias, skip, ea, ae = (_t(c[k], dev) for k in ("xl", "s_src", "s_dst", "bias", "skip", "edge_attr", "a_edge"))
    whole = cm.aggregate_gat_edges(xl, ss, sd, ea, ae, bias=bias, skip=skip, act="tanh", heads=heads, negative_slope=SLOPE)
    for h in range(heads):
        cols = slice(h * C, (h + 1) * C)
        one = cm.aggregate_gat_edges(xl[:, cols], ss[:, h:h + 1], sd[:, h:h + 1], ea, ae[h:h + 1], bias=bias[cols].contiguous(),
                                     skip=skip[:, cols].contiguous(), act="tanh", heads=1, negative_slope=SLOPE)
        assert xl[:, cols].stride(0) == width and one.shape == (xl.shape[0], C)
        assert torch.equal(one, whole[:, cols]), h
    cm.check()


def _launch_steps(num_nodes, width, heads):
    """(steps, lane groups per workgroup) of ``launch_gat_edge_aggregate`` on aligned operands: a lane group of the smallest power
    of two >= width / VEC lanes (at most 64) per ROW, VEC = 4 when C % 4 == 0, a step = one row per lane group of a 256-lane
    workgroup."""
    c = width // heads
    nvec = width // 4 if c % 4 == 0 else width
    lanes = 1
    while lanes < nvec and lanes < 64:
        lanes *= 2
    groups = 256 // lanes
    return -(-num_nodes // groups), groups


def _wg_per_cu():
    """``GATE_WG_PER_CU`` of csrc/k_gat_edge.hip: the most workgroups per CU the grid is cut for."""
    src = (Path(runtime.CSRC_DIR) / "k_gat_edge.hip").read_text()
    return int(re.search(r"constexpr int GATE_WG_PER_CU = (\d+);", src).group(1))


@pytest.mark.parametrize("width,heads,d", [(256, 8, 4), (32, 4, 4)])
def test_many_steps_per_workgroup(dev, width, heads, d):
    """The smallest number of copies of the edge batch in one batch, every copy with the first copy's operand rows, at which
    ``att_grid`` gives three steps or more per workgroup: the grid holds at most ``GATE_WG_PER_CU`` workgroups per CU of this
    device (fewer if the kernel's occupancy is lower, which only adds steps), so ``steps > 2 * GATE_WG_PER_CU * CUs`` is what it
    takes -- derived here from the grid rule, ASSERTED, not guessed.  The three-deep pipeline's rotation, the slot prefetch of the
    next step and the long rows' second walk at a later step all run, and the last copy's rows, the hub included, are taken at the
    last step by another workgroup and lane group than the first copy's.  All rows are held against float64 (a copy's graphs are
    closed, so its reference is the one batch's); every copy has the first copy's bits, and those are the bits of the one batch
    launched alone on its own, smaller grid."""
    b = _batch("edge", width)
    n = b.num_nodes
    max_grid = _wg_per_cu() * torch.cuda.get_device_properties(dev).multi_processor_count
    groups = _launch_steps(n, width, heads)[1]
    copies = (2 * max_grid * groups) // n + 1  # the smallest with copies * n > 2 * max_grid * groups
    long = pack_graphs([b.graph(g) for g in range(b.num_graphs)] * copies)
    assert long.num_nodes == copies * n and np.array_equal(long.coo[:b.num_edges], b.coo)
    iters = lambda k: -(-_launch_steps(k * n, width, heads)[0] // max_grid)  # noqa: E731  (att_grid's, at the largest grid)
    assert iters(copies) >= 3 and (copies == 1 or iters(copies - 1) < 3)
    r = _refs("edge", width, heads, d, "flat")
    c = r["c"]
    tiled = {k: (np.tile(v, (copies, 1)) if k in ("xl", "s_src", "s_dst", "skip", "edge_attr") else v) for k, v in c.items()}
    cl = _workspace(long)
    _prep(cl, long, dev)
    got = _stage(cl, tiled, dev, heads)
    cl.check()
    alone = _stage(_prepared("edge", width, dev), c, dev, heads)
    assert torch.equal(got[:n], alone)
    assert torch.equal(got.view(copies, n, width), got[:n].expand(copies, n, width))
    coo = R.workspace_edges(long.coo, True)
    assert np.bincount(coo[:, 1], minlength=long.num_nodes)[(copies - 1) * n:].max() >= 1150  # (a hub in the last copy)
    record_classes(f"aggregate_gat_edges/edge-x{copies}-w{width}-h{heads}-d{d}", got.cpu().numpy(), np.tile(r["ref"], (copies, 1)),
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
    args = _args(c, with_loops.coo, heads)
    record(f"aggregate_gat_edges/looped-d{d}", outs[0].cpu().numpy(), gate_ref(*args), gate_ref(*args, np.float32))


# ---------------------------------------------------------------------------------------------------- 4. whole models
def _model_batch(graphs, in_dim, seed):
    """``graphs`` synthetic qm9-like graphs with seeded features of width ``in_dim``, an empty and a one-node graph among them"""
    mols, rng = synthetic.make_batch("qm9", graphs, seed=seed), np.random.default_rng(seed)
    gs = [(rng.uniform(-1, 1, (mols.graph(g)[0].shape[0], in_dim)).astype(np.float32), mols.graph(g)[1]) for g in range(graphs)]
    return pack_graphs(gs[:graphs // 2] + [EMPTY(in_dim), ONE(in_dim)] + gs[graphs // 2:] + [EMPTY(in_dim)])


def _model(layers, heads, in_dim, hidden, d, seed=0):
    return make_gate_model(in_dim=in_dim, edge_dim=d, hidden=hidden, layers=layers, heads=heads, skip=True, pools=("add", "mean", "max"),
                           mlp_layers=1, out_act=torch.nn.LogSoftmax, seed=seed)


def _compiled(model, b, promise=0, degree=0, ingest=False, caps=None):
    cm = runtime.CompiledModel.from_model(model, *(caps or (b.num_graphs, b.num_nodes, b.num_edges)))
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
    # the kind: GAT v1's heads, the edge models' edge_dim, and not a GATv2 model
    assert cm.lib.gnnb_model_gatconv_heads(cm._model) == heads and cm.lib.gnnb_model_edge_dim(cm._model) == d
    assert cm.lib.gnnb_model_gat_heads(cm._model) == 0
    xd, cood, nptr, eptr = to_dev(b, dev)
    ead = _t(ea, dev)
    out = cm.forward_edges(xd, ead, cood, nptr, eptr)
    cm.check()
    assert cm.last_path() == "layerwise" and out.shape == (b.num_graphs, 19)
    record(f"forward_edges/gate-L{layers}-h{heads}-in{in_dim}-w{hidden}-d{d}", out.cpu().numpy(), forward64(model, b, b.x, ea), run(model, b, b.x, ea))
    # the same forward again, and the prepared form, give the same bits (no atomics, a fixed summation order)
    assert torch.equal(cm.forward_edges(xd, ead, cood, nptr, eptr), out)
    assert torch.equal(cm.forward_prepared_edges(xd, ead), out)


def test_the_neighbouring_kinds_report_what_they_reported(dev):
    b = _model_batch(6, 9, seed=30)
    plain = _compiled(make_gat_model(in_dim=9, hidden=32, layers=2, heads=4), b)
    v2e = _compiled(make_gatv2e_model(in_dim=9, edge_dim=4, hidden=32, layers=2, heads=4), b)
    lib = plain.lib
    assert (lib.gnnb_model_gatconv_heads(plain._model), lib.gnnb_model_edge_dim(plain._model), lib.gnnb_model_gat_heads(plain._model)) == (4, 0, 0)
    assert (lib.gnnb_model_gatconv_heads(v2e._model), lib.gnnb_model_edge_dim(v2e._model), lib.gnnb_model_gat_heads(v2e._model)) == (0, 4, 4)


@pytest.fixture(scope="module")
def pyg():
    """A 300-graph batch (two radix passes), in 11, edge_dim 4, grouped and with edges + edge_attr rows under one seeded permutation."""
    b = synthetic.make_batch("qm9", 300, seed=41)
    rng = np.random.default_rng(42)
    x = rng.uniform(-1, 1, (b.num_nodes, 11)).astype(np.float32)
    ei = np.ascontiguousarray(b.coo.T.astype(np.int64))
    ea = edge_attrs(b.num_edges, 4, seed=43)
    perm = rng.permutation(b.num_edges)
    model = make_gate_model(in_dim=11, edge_dim=4, hidden=32, layers=2, heads=4, seed=3)
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
        record(f"forward_pyg_edges/gate-{kind}", out.cpu().numpy(), forward64(model, gb, pyg["x"], ea_ord), run(model, gb, pyg["x"], ea_ord))
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
    record("forward_edges/gate-L3-h4-promises", outs[-1].cpu().numpy(), forward64(model, b, b.x, ea), run(model, b, b.x, ea))


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
    record("forward_edges/gate-captured", out.cpu().numpy(), forward64(model, b, x2, ea2), run(model, b, x2, ea2))
    cm.check()


# ---------------------------------------------------------------------------------------------------- 5. one workspace, unlike batches
def test_one_workspace_across_unlike_batches(dev):
    """Four batches of different node, edge and graph counts -- one with the 1200-edge hub, explicit self loops and duplicate edges,
    one without a single edge -- in turn, twice, on ONE long-lived workspace, through ``forward_edges`` and, every other step, the
    prepared form; after each forward the stage entry runs on the prepared batch into an output pre-filled with NaN.  Each step
    gives the bits of a fresh workspace of the batch's own size, and the stage result is held against float64 per in-degree
    class."""
    d, heads = 4, 4
    model = _model(2, heads, 9, 32, d, seed=8)
    lonely = pack_graphs([ONE(9)] * 5 + [EMPTY(9)] + [ONE(9)] * 3)
    batches = [_model_batch(20, 9, seed=41), edge_batch(8, 9, seed=44), lonely, _model_batch(7, 9, seed=42)]
    assert lonely.num_edges == 0 and np.bincount(batches[1].coo[:, 1]).max() >= 1200
    assert len({b.num_graphs for b in batches}) == 4 and len({b.num_nodes for b in batches}) == 4 and len({b.num_edges for b in batches}) == 4
    eas = [edge_attrs(b.num_edges, d, seed=43 + i) for i, b in enumerate(batches)]
    stages = [edge_case(b.coo, b.num_nodes, 32, heads, d, "flat", seed=50 + i) for i, b in enumerate(batches)]
    for c, ea in zip(stages, eas):
        c["edge_attr"] = ea  # (the forward's attributes: the stage reads what the batch brought)

    def stage(cm, b, c):
        out = torch.full((b.num_nodes, 32), float("nan"), dtype=torch.float32, device=dev)
        ead = _t(c["edge_attr"], dev) if b.num_edges else None
        got = cm.aggregate_gat_edges(_t(c["xl"], dev), _t(c["s_src"], dev), _t(c["s_dst"], dev), ead, _t(c["a_edge"], dev),
                                     bias=_t(c["bias"], dev), heads=heads, negative_slope=SLOPE, out=out)
        assert got.data_ptr() == out.data_ptr() and not torch.isnan(got).any()
        return got

    want = []
    for b, ea, c in zip(batches, eas, stages):
        fresh = _compiled(model, b, caps=(b.num_graphs, b.num_nodes, max(b.num_edges, 1)))
        xd, cood, nptr, eptr = to_dev(b, dev)
        want.append((fresh.forward_edges(xd, _t(ea, dev), cood, nptr, eptr).clone(), stage(fresh, b, c).clone()))
        fresh.check()
    caps = tuple(max(getattr(b, k) for b in batches) for k in ("num_graphs", "num_nodes", "num_edges"))
    cm = _compiled(model, batches[0], caps=caps)
    for turn in range(2):
        for i, (b, ea, c) in enumerate(zip(batches, eas, stages)):
            xd, cood, nptr, eptr = to_dev(b, dev)
            if (turn + i) % 2:
                cm.graph_prep(cood, nptr, eptr, b.num_nodes)
                got = cm.forward_prepared_edges(xd, _t(ea, dev))
            else:
                got = cm.forward_edges(xd, _t(ea, dev), cood, nptr, eptr)
            cm.check()
            assert cm.last_path() == "layerwise" and got.shape == (b.num_graphs, 19) and torch.equal(got, want[i][0]), (turn, i)
            assert torch.equal(stage(cm, b, c), want[i][1]), (turn, i)
            cm.check()
    for i, (b, ea, c) in enumerate(zip(batches, eas, stages)):
        record(f"forward_edges/gate-stream-{i}", want[i][0].cpu().numpy(), forward64(model, b, b.x, ea), run(model, b, b.x, ea))
        args = _args(c, b.coo, heads)
        record_classes(f"aggregate_gat_edges/stream-{i}", want[i][1].cpu().numpy(), gate_ref(*args), gate_ref(*args, np.float32),
                       R.workspace_edges(b.coo, True))


# ---------------------------------------------------------------------------------------------------- 6. refusals
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
    # a model does not run on the workspace of a plain GAT model, of a GATv2 model with edge features and the same numbers, of one
    # with another edge_dim, other heads or another slope
    N, E = b.num_nodes, b.num_edges
    kw = dict(in_dim=9, hidden=32, layers=2, heads=4, mlp_layers=1, out_act=torch.nn.LogSoftmax)
    slope = make_gate_model(edge_dim=4, **kw)
    for conv in slope.gnn_convs:
        conv.negative_slope = conv.conv.negative_slope = 0.1
    for other_model in (make_gat_model(**kw), make_gatv2e_model(edge_dim=4, **kw), _model(2, 4, 9, 32, 3), _model(2, 2, 9, 32, 4), slope):
        other = _compiled(other_model, b)
        assert bytes(cm.desc) == bytes(other.desc)
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
        cm.aggregate_gat_edges(z(N, 30), z(N, 4), z(N, 4), z(E, 4), z(4, 4), heads=4)
    with pytest.raises(runtime.GnnbError, match="at most 256"):
        cm.aggregate_gat_edges(z(N, 264), z(N, 4), z(N, 4), z(E, 4), z(4, 4), heads=4)
    for heads in (9, 0):
        with pytest.raises(runtime.GnnbError, match="heads must be"):
            cm.aggregate_gat_edges(z(N, 32), z(N, 4), z(N, 4), z(E, 4), z(4, 4), heads=heads)
    for bad, what in ((dict(s_src=z(N, 3)), "s_src"), (dict(s_dst=z(N - 1, 4)), "s_dst"), (dict(xl=z(N - 1, 32)), "xl"), (dict(bias=z(16)), "bias"),
                      (dict(skip=z(N, 16)), "skip has shape"), (dict(skip=z(N - 1, 32)), "skip must be"), (dict(out=z(N, 16)), "out"),
                      (dict(act="swish"), "act must be"), (dict(xl=z(N, 32).double()), "xl"), (dict(a_edge=z(4, 17)), "a_edge must be"),
                      (dict(a_edge=z(3, 4)), "a_edge"), (dict(a_edge=z(4, 4).cpu()), "a_edge"), (dict(edge_attr=z(E, 3)), "edge_attr has shape"),
                      (dict(edge_attr=z(E - 1, 4)), "edge_attr must be"), (dict(edge_attr=None), "edge_attr is required"),
                      (dict(edge_attr=z(E, 4).double()), "float32")):
        args = dict(xl=z(N, 32), s_src=z(N, 4), s_dst=z(N, 4), edge_attr=z(E, 4), a_edge=z(4, 4), heads=4)
        args.update(bad)
        with pytest.raises(runtime.GnnbError, match=what):
            cm.aggregate_gat_edges(args.pop("xl"), args.pop("s_src"), args.pop("s_dst"), args.pop("edge_attr"), args.pop("a_edge"), **args)
    # ... and the C entry itself, every GNNB_ERR_INVALID with nothing launched (the output keeps its NaN): heads that do not divide
    # the width, width > 256, heads > 8, a stride below its row, a NULL operand, a gnnb_act out of range, a negative_slope that is
    # not finite, edge_dim out of range, ldae below edge_dim, a NULL a_edge, a NULL edge_attr for a batch with edges, an unprepared
    # workspace, a workspace whose tables keep explicit self loops
    xl = z(max(N, E), 264)
    p = xl.data_ptr()
    out = torch.full((N, 264), float("nan"), device=dev)
    o = out.data_ptr()

    def call(ws, ld=32, heads=4, width=32, xl_ptr=p, ss_ptr=p, sd_ptr=p, lds=4, ldd=4, act=4, slope=0.2, ea_ptr=p, ed=4, ae_ptr=p, ldae=4, out_ptr=o):
        return cm.lib.gnnb_aggregate_gat_edges(ws, xl_ptr, ld, ss_ptr, lds, sd_ptr, ldd, None, None, act, heads, slope, ea_ptr, ed, ae_ptr, ldae,
                                               out_ptr, width, None)
    assert E > 0
    for kw in (dict(heads=3), dict(ld=264, width=264), dict(heads=9, width=36), dict(ld=16), dict(lds=3), dict(ldd=3), dict(width=0), dict(heads=0),
               dict(xl_ptr=None), dict(ss_ptr=None), dict(sd_ptr=None), dict(out_ptr=None), dict(act=5), dict(act=-1), dict(slope=float("nan")),
               dict(slope=float("inf")), dict(ed=0), dict(ed=17, ldae=17), dict(ed=4, ldae=3), dict(ae_ptr=None), dict(ea_ptr=None)):
        assert call(cm._ws, **kw) == -1 and b"bad argument" in cm.lib.gnnb_last_error(), kw
    unprepared = _compiled(model, b)
    assert call(unprepared._ws) == -1 and b"prepared" in cm.lib.gnnb_last_error()
    assert call(None) == -1 and b"prepared" in cm.lib.gnnb_last_error()
    gin = runtime.CompiledModel.from_model(make_model("gin", in_dim=9, hidden=8, layers=1, out_dim=8), b.num_graphs, N, E)
    gin.graph_prep(cood, nptr, eptr, N)
    assert call(gin._ws) == -1 and b"GCN workspace" in cm.lib.gnnb_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all()  # nothing was launched
    assert call(cm._ws) == 0  # (the same call with every argument in range runs)
    torch.cuda.synchronize()
    assert not torch.isnan(out.reshape(-1)[:N * 32]).any()  # ([N, 32] rows, back to back)
    # nothing above left a flag or changed a result
    cm.check()
    assert torch.equal(cm.forward_edges(xd, ea, cood, nptr, eptr), good)
