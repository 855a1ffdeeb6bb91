"""GAT (v1) models on the MI355X (include/gnnb_gatconv.h; csrc/k_gat.hip): the fused attention aggregate as a stage entry, its
epilogue, its bits, whole models through ``forward`` and ``forward_pyg``, the promises, a captured forward, and the refusals.

Acceptance is ``ref64.budget`` with the project's K = 4, F = 2^-22 -- no tolerance of this file's own -- per
in-degree class (``gine_util.budget_by_degree``), nothing left out of a comparison.  The reference is float64 (``gat_util.gat_ref``:
an explicit two-pass softmax; whole models: the model's own torch definition on a ``.double()`` copy); ``base`` is the same in fp32
on the CPU.  The stage's operands lie on dyadic grids on which every score is exact in fp32 -- ASSERTED on the reference alone --
so only ``exp`` and the sums differ between ``got``, ``base`` and ``ref``; the folded score columns of the layer's GEMM are held to
the budget by the whole-model tests.  Worst e / e32 per entry go to GNNB_FP64_REPORT=<file>."""
import json
import os

import numpy as np
import pytest
import torch

import ref64 as R
from gat_util import SLOPE, gat_ref, gat_scores, make_gat_model, stage_case
from gatv2_util import make_gatv2_model
from gine_util import budget_by_degree
from gnnbuilder_amd import runtime, synthetic
from gnnbuilder_amd.batching import pack_graphs
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
BATCHES, PREPARED, REFS = {}, {}, {}


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


def _refs(kind, width, heads, operands):
    """(case, ref, base) of the plain stage (bias, no skip, no activation) on a batch: computed once, shared, left unchanged."""
    key = (kind, width, heads, operands)
    if key not in REFS:
        b = _batch(kind, width)
        c = stage_case(b.num_nodes, width, heads, operands)
        ref = gat_ref(c["xl"], c["s_src"], c["s_dst"], c["bias"], None, "none", b.coo, heads, SLOPE)
        base = gat_ref(c["xl"], c["s_src"], c["s_dst"], c["bias"], None, "none", b.coo, heads, SLOPE, np.float32)
        REFS[key] = (c, ref, base)
    return REFS[key]


# (width, heads): the 16-byte form with one head and with four; the scalar form at C = 3; the scalar form over three strides with
# the head boundary (column 65) inside a stride; C = 12, six lanes in a group of 8; width % 4 == 0 but C = 3, which must be scalar;
# a whole wave per row
SHAPES = [(32, 1), (32, 4), (9, 3), (130, 2), (24, 2), (24, 8), (256, 8)]


def _stage(cm, c, dev, heads, bias=True, skip=False, act="none"):
    return cm.aggregate_gat(_t(c["xl"], dev), _t(c["s_src"], dev), _t(c["s_dst"], dev), bias=_t(c["bias"], dev) if bias else None,
                            skip=_t(c["skip"], dev) if skip else None, act=act, heads=heads, negative_slope=SLOPE)


def _check_scores_exact(c, coo):
    _, dst, s64 = gat_scores(c["s_src"], c["s_dst"], coo, SLOPE, np.float64)
    _, _, s32 = gat_scores(c["s_src"], c["s_dst"], coo, SLOPE, np.float32)
    assert s32.dtype == np.float32 and np.array_equal(s32.astype(np.float64), s64)  # every score is exact in fp32
    return dst, s64


@pytest.mark.parametrize("operands", ["flat", "steep"])
@pytest.mark.parametrize("kind", ["edge", "sweep"])
@pytest.mark.parametrize("width,heads", SHAPES)
def test_stage_against_float64(dev, width, heads, kind, operands):
    b = _batch(kind, width)
    coo = R.workspace_edges(b.coo, True)  # (the tables hold no explicit self loop; the layer adds one per node)
    deg = np.bincount(coo[:, 1], minlength=b.num_nodes)
    # the hub (a row split over the workgroup) and rows without in-edges
    assert deg.max() >= 1150 and (deg == 0).any()
    c, ref, base = _refs(kind, width, heads, operands)
    dst, s64 = _check_scores_exact(c, b.coo)
    if operands == "flat":
        _, a, adst = gat_ref(c["xl"], c["s_src"], c["s_dst"], c["bias"], None, "none", b.coo, heads, SLOPE, return_weights=True)
        assert np.abs(s64).max() <= 2.0
        heavy = np.zeros((b.num_nodes, heads), np.int64)
        np.add.at(heavy, adst, a > 0.05)
        assert (heavy.max(1) >= 3).sum() >= 100  # many neighbours carry weight
    else:
        big = np.zeros((b.num_nodes, heads))
        np.maximum.at(big, dst, np.abs(s64))
        assert (big.max(1) > 200.0).sum() >= 100  # exp without the max subtraction overflows there
    cm = _prepared(kind, width, dev)
    got = _stage(cm, c, dev, heads)
    cm.check()
    got = got.cpu().numpy()
    assert got.shape == (b.num_nodes, width) and np.isfinite(got).all()
    assert np.array_equal(got[deg == 0], (c["xl"] + c["bias"])[deg == 0])  # in-degree 0: xl_i + bias, bit for bit
    record_classes(f"aggregate_gat/{kind}-w{width}-h{heads}-{operands}", got, ref, base, coo)


# ---------------------------------------------------------------------------------------------------- 2. zero scores
@pytest.mark.parametrize("width,heads", SHAPES)
def test_zero_scores_give_the_mean_over_the_closed_neighbourhood(dev, width, heads):
    b = _batch("edge", width)
    coo = R.workspace_edges(b.coo, True)
    c, _, _ = _refs("edge", width, heads, "flat")
    zero = np.zeros((b.num_nodes, heads), np.float32)
    cnt = 1.0 + np.bincount(coo[:, 1], minlength=b.num_nodes)

    def mean(dtype):
        acc = c["xl"].astype(dtype).copy()  # (the self term first, then the in-edges in slot order)
        np.add.at(acc, coo[:, 1], c["xl"].astype(dtype)[coo[:, 0]])
        return acc / cnt.astype(dtype)[:, None] + c["bias"].astype(dtype)

    cm = _prepared("edge", width, dev)
    got = cm.aggregate_gat(_t(c["xl"], dev), _t(zero, dev), _t(zero, dev), bias=_t(c["bias"], dev), heads=heads, negative_slope=SLOPE)
    cm.check()
    record_classes(f"aggregate_gat/edge-w{width}-h{heads}-zero", got.cpu().numpy(), mean(np.float64), mean(np.float32), coo)


# ---------------------------------------------------------------------------------------------------- 3. the epilogue
@pytest.mark.parametrize("with_skip", [True, False])
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("act", ["relu", "gelu", "sigmoid", "tanh", "none"])
def test_epilogue_bias_skip_and_activation(dev, act, with_bias, with_skip):
    """Width 32, heads 4: ``xl``, ``s_src`` and ``s_dst`` as the column blocks of one [N, 40] tensor, as the layer's GEMM leaves
    them (row stride 40: the 16-byte form; the score blocks at strides above ``heads``)."""
    width, heads = 32, 4
    b = _batch("edge", width)
    coo = R.workspace_edges(b.coo, True)
    c, _, _ = _refs("edge", width, heads, "flat")
    bias, skip = c["bias"] if with_bias else None, c["skip"] if with_skip else None
    ref = gat_ref(c["xl"], c["s_src"], c["s_dst"], bias, skip, act, b.coo, heads, SLOPE)
    base = gat_ref(c["xl"], c["s_src"], c["s_dst"], bias, skip, act, b.coo, heads, SLOPE, np.float32)
    cm = _prepared("edge", width, dev)
    blocks = _t(np.concatenate([c["xl"], c["s_src"], c["s_dst"]], 1), dev)
    assert blocks.shape == (b.num_nodes, 40) and blocks.data_ptr() % 16 == 0
    got = cm.aggregate_gat(blocks[:, :32], blocks[:, 32:36], blocks[:, 36:40], bias=None if bias is None else _t(bias, dev),
                           skip=None if skip is None else _t(skip, dev), act=act, heads=heads, negative_slope=SLOPE)
    cm.check()
    if act == "none":  # the separate, contiguous operands give the same bits
        assert torch.equal(got, _stage(cm, c, dev, heads, bias=with_bias, skip=with_skip))
    entry = f"aggregate_gat/epilogue-{act}" + ("" if with_bias else "-nobias") + ("" if with_skip else "-noskip")
    record_classes(entry, got.cpu().numpy(), ref, base, coo)


# ---------------------------------------------------------------------------------------------------- 4. bits
@pytest.mark.parametrize("width,heads", [(32, 4), (9, 3), (130, 2), (24, 8)])
def test_a_repeat_launch_and_another_grid_give_the_same_bits(dev, width, heads):
    b = _batch("edge", width)
    c, _, _ = _refs("edge", width, heads, "flat")
    cm = _prepared("edge", width, dev)
    first = _stage(cm, c, dev, heads, skip=True, act="tanh")
    assert torch.equal(_stage(cm, c, dev, heads, skip=True, act="tanh"), first)
    # the same batch on a workspace with far larger capacities: graph prep cuts other node tiles there.  The kernel's grid is cut
    # from the batch alone (launch_gat_aggregate), so this is the same grid on other tables; other grids and several steps per
    # workgroup are test_many_steps_per_workgroup's
    big = _workspace(b, slack=16)
    _prep(big, b, dev)
    assert torch.equal(_stage(big, c, dev, heads, skip=True, act="tanh"), first)
    cm.check(), big.check()


def _launch_steps(num_nodes, width, heads):
    """(steps, lane groups per workgroup) of ``launch_gat_aggregate`` on aligned operands: a lane group of the smallest power of
    two >= width / VEC lanes (at most 64) per ROW, VEC = 4 when C % 4 == 0, a step = one row per lane group of a 256-lane
    workgroup."""
    c = width // heads
    nvec = width // 4 if c % 4 == 0 else width
    lanes = 1
    while lanes < nvec and lanes < 64:
        lanes *= 2
    groups = 256 // lanes
    return -(-num_nodes // groups), groups


def _wg_per_cu():
    """``GAT1_WG_PER_CU`` of csrc/k_gat.hip: the most workgroups per CU the grid is cut for."""
    import re
    from pathlib import Path
    src = (Path(runtime.CSRC_DIR) / "k_gat.hip").read_text()
    return int(re.search(r"constexpr int GAT1_WG_PER_CU = (\d+);", src).group(1))


# (width, heads, copies, operand set): the 16-byte form with a whole wave per row; the scalar form over four strides of a wave
MANY_STEPS = [(256, 8, 6, "flat"), (130, 2, 6, "steep")]


@pytest.mark.parametrize("width,heads,copies,operands", MANY_STEPS)
def test_many_steps_per_workgroup(dev, width, heads, copies, operands):
    """``copies`` copies of the sweep batch in one batch, every copy with the first copy's operand rows: more steps than the grid
    can hold at ``GAT1_WG_PER_CU`` workgroups per CU on this device (ASSERTED), so every workgroup walks two steps or more -- the
    three-deep pipeline's rotation, the slot prefetch of the next step, the long rows' second walk at a later step -- and the last
    copy's rows, hubs included, are taken at a later step by another workgroup and lane group than the first copy's.  All rows
    are held against float64 (a copy's graphs are closed, so its reference is the one batch's); every copy has the first copy's
    bits, and those are the bits of the one batch launched alone on its own, smaller grid."""
    b = _batch("sweep", width)
    n = b.num_nodes
    long = pack_graphs([b.graph(g) for g in range(b.num_graphs)] * copies)
    assert long.num_nodes == copies * n
    steps, groups = _launch_steps(long.num_nodes, width, heads)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert steps > _wg_per_cu() * cus  # the grid holds at most that many workgroups: two steps or more for each
    assert (copies - 1) * n // groups >= (steps + 1) // 2  # the last copy begins behind the grid's first sweep
    c, ref, base = _refs("sweep", width, heads, operands)
    _check_scores_exact(c, b.coo)
    tiled = {k: (np.tile(v, (copies, 1)) if v.ndim == 2 else v) for k, v in c.items()}
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
    record_classes(f"aggregate_gat/sweep-x{copies}-w{width}-h{heads}-{operands}", got.cpu().numpy(), np.tile(ref, (copies, 1)),
                   np.tile(base, (copies, 1)), coo)


@pytest.mark.parametrize("operands", ["flat", "steep"])
@pytest.mark.parametrize("width,heads", [(32, 4), (9, 3)])
def test_an_h_head_launch_equals_h_one_head_launches_on_the_column_slices(dev, width, heads, operands):
    """A column's bits depend on the batch and on the form only: not on the lane group (8 lanes per row against 2 at width 32, 16
    against 4 at width 9) and not on heads beyond which scalar the column reads."""
    C = width // heads
    c, _, _ = _refs("edge", width, heads, operands)
    cm = _prepared("edge", width, dev)
    xl, ss, sd, bias, skip = (_t(c[k], dev) for k in ("xl", "s_src", "s_dst", "bias", "skip"))
    whole = cm.aggregate_gat(xl, ss, sd, bias=bias, skip=skip, act="tanh", heads=heads, negative_slope=SLOPE)
    for h in range(heads):
        cols = slice(h * C, (h + 1) * C)
        one = cm.aggregate_gat(xl[:, cols], ss[:, h:h + 1], sd[:, h:h + 1], bias=bias[cols].contiguous(), skip=skip[:, cols].contiguous(),
                               act="tanh", heads=1, negative_slope=SLOPE)
        assert xl[:, cols].stride(0) == width and one.shape == (xl.shape[0], C)
        assert torch.equal(one, whole[:, cols]), h
    cm.check()


def test_explicit_self_loops_give_the_bits_of_the_batch_without_them(dev):
    width, heads = 24, 2
    x, coo = looped_graph(40, width, seed=3)
    assert (coo[:, 0] == coo[:, 1]).sum() >= 10
    others = [ONE(width), (x[:7], np.array([[0, 1], [1, 0], [2, 1], [5, 1]], np.int32))]
    with_loops = pack_graphs([(x, coo)] + others)
    without = pack_graphs([(x, coo[coo[:, 0] != coo[:, 1]])] + others)
    assert with_loops.num_edges > without.num_edges and with_loops.num_nodes == without.num_nodes
    c = stage_case(with_loops.num_nodes, width, heads, "flat")
    outs = []
    for b in (with_loops, without):
        cm = _workspace(b)
        _prep(cm, b, dev)
        outs.append(_stage(cm, c, dev, heads))
        cm.check()
    assert torch.equal(outs[0], outs[1])
    ref = gat_ref(c["xl"], c["s_src"], c["s_dst"], c["bias"], None, "none", with_loops.coo, heads, SLOPE)
    base = gat_ref(c["xl"], c["s_src"], c["s_dst"], c["bias"], None, "none", with_loops.coo, heads, SLOPE, np.float32)
    record("aggregate_gat/looped", outs[0].cpu().numpy(), ref, base)


@pytest.mark.parametrize("width,heads", [(32, 4), (256, 8)])
def test_xl_off_a_16_byte_boundary_takes_the_scalar_form(dev, width, heads):
    """``xl`` one float past a 16-byte boundary: scalar accesses (16-byte ones would fault or read other floats), the result within
    the budget.  At width 256 the scalar form walks four strides, each with a state of its own, where the 16-byte form has one."""
    b = _batch("edge", width)
    coo = R.workspace_edges(b.coo, True)
    c, ref, base = _refs("edge", width, heads, "flat")
    cm = _prepared("edge", width, dev)
    got = cm.aggregate_gat(_offset(c["xl"], dev), _t(c["s_src"], dev), _t(c["s_dst"], dev), bias=_t(c["bias"], dev), heads=heads,
                           negative_slope=SLOPE)
    cm.check()
    record_classes(f"aggregate_gat/edge-w{width}-h{heads}-offset", got.cpu().numpy(), ref, base, coo)


# ---------------------------------------------------------------------------------------------------- 5. whole models
def _model_batch(graphs, in_dim, seed):
    """``graphs`` synthetic qm9-like graphs with seeded features of width ``in_dim``, an empty and a one-node graph among them"""
    mols, rng = synthetic.make_batch("qm9", graphs, seed=seed), np.random.default_rng(seed)
    gs = [(rng.uniform(-1, 1, (mols.graph(g)[0].shape[0], in_dim)).astype(np.float32), mols.graph(g)[1]) for g in range(graphs)]
    return pack_graphs(gs[:graphs // 2] + [EMPTY(in_dim), ONE(in_dim)] + gs[graphs // 2:] + [EMPTY(in_dim)])


def _model(layers, heads, in_dim, hidden, seed=0, skip=True):
    return make_gat_model(in_dim=in_dim, hidden=hidden, layers=layers, heads=heads, skip=skip, pools=("add", "mean", "max"), mlp_layers=1,
                          out_act=torch.nn.LogSoftmax, seed=seed)


def _compiled(model, b, promise=0, degree=0, ingest=False):
    cm = runtime.CompiledModel.from_model(model, b.num_graphs, b.num_nodes, b.num_edges)
    if ingest:  # (right after construction: before a batch is prepared on the workspace)
        cm.enable_ingest()
    if promise:
        cm.set_max_graph_nodes(promise)
    if degree:
        cm.set_max_degree(degree)
    return cm


# layers 1 .. 3 x heads 1, 2, 4 at two widths with skip connections; without them where they exist (three layers)
MODELS = [(L, h, True, i, d, g) for (i, d, g) in ((9, 32, 64), (11, 128, 12)) for h in (1, 2, 4) for L in (1, 2, 3)] + \
         [(3, h, False, i, d, g) for (i, d, g) in ((9, 32, 64), (11, 128, 12)) for h in (1, 2, 4)]


@pytest.mark.parametrize("layers,heads,skip,in_dim,hidden,graphs", MODELS)
def test_whole_models_against_float64(dev, layers, heads, skip, in_dim, hidden, graphs):
    model = _model(layers, heads, in_dim, hidden, seed=layers, skip=skip)
    b = _model_batch(graphs, in_dim, seed=31 + layers)
    assert b.num_graphs == graphs + 3
    cm = _compiled(model, b, ingest=True)
    assert cm.lib.gnnb_model_gatconv_heads(cm._model) == heads and cm.lib.gnnb_model_gat_heads(cm._model) == 0
    assert cm.lib.gnnb_model_edge_dim(cm._model) == 0 and cm.lib.gnnb_model_transformer_heads(cm._model) == 0
    xd, cood, nptr, eptr = to_dev(b, dev)
    out = cm.forward(xd, cood, nptr, eptr)
    cm.check()
    assert cm.last_path() == "layerwise" and out.shape == (b.num_graphs, 19)
    ref, base = R.forward64(model, b, b.x), R.run(model, b, b.x)
    entry = f"forward/gat-L{layers}-h{heads}-in{in_dim}-d{hidden}" + ("" if skip else "-noskip")
    record(entry, out.cpu().numpy(), ref, base)
    # the same forward again, and the prepared form, give the same bits (no atomics, a fixed summation order)
    assert torch.equal(cm.forward(xd, cood, nptr, eptr), out)
    assert torch.equal(cm.forward_prepared(xd), out)
    # ... and so does the PyG mini-batch from a device edge_index + batch (the ingest's arrays are the host's)
    ei = _t(np.ascontiguousarray(b.coo.T.astype(np.int64)).reshape(2, -1), dev)
    pyg = cm.forward_pyg(xd, ei, batch=_t(batch_vector(b), dev), num_graphs=b.num_graphs)
    cm.check()
    assert cm.last_path() == "layerwise"
    record(entry + "-pyg", pyg.cpu().numpy(), ref, base)
    assert torch.equal(pyg, out)


def test_promises_change_neither_the_path_nor_a_bit(dev):
    model = _model(3, 4, 9, 32, seed=5)
    b = _model_batch(12, 9, seed=23)
    assert np.diff(b.node_ptr).max() <= 64 and np.bincount(b.coo[:, 1]).max() <= 15
    xd, cood, nptr, eptr = to_dev(b, dev)
    outs = []
    for promise, degree in ((0, 0), (64, 0), (0, 15), (64, 15)):
        cm = _compiled(model, b, promise, degree)
        outs.append(cm.forward(xd, cood, nptr, eptr))
        cm.check()  # (the promises hold)
        assert cm.last_path() == "layerwise"
    assert all(torch.equal(o, outs[0]) for o in outs[1:])
    record("forward/gat-L3-h4-promises", outs[-1].cpu().numpy(), R.forward64(model, b, b.x), R.run(model, b, b.x))


def test_forward_with_the_next_batchs_prep(dev):
    """``forward_prepared_prep_next`` over two alternating workspaces under a promise of 64 nodes (a GAT workspace needs nothing
    launched behind its tables, so the next batch's prep may run as a guest of the readout): the bits of ``forward`` per batch."""
    model = _model(2, 4, 9, 32, seed=7)
    batches = [_model_batch(12, 9, seed=26), _model_batch(20, 9, seed=27), _model_batch(12, 9, seed=28)]
    cap = [max(getattr(b, k) for b in batches) for k in ("num_graphs", "num_nodes", "num_edges")]
    want = []
    for b in batches:
        cm = _compiled(model, b, promise=64)
        want.append(cm.forward(*to_dev(b, dev)))
        cm.check()
    pair = [runtime.CompiledModel.from_model(model, *cap, max_graph_nodes=64) for _ in range(2)]
    args = [to_dev(b, dev) for b in batches]
    pair[0].graph_prep(args[0][1], args[0][2], args[0][3], batches[0].num_nodes)
    for i, b in enumerate(batches):
        cur, nxt = pair[i & 1], pair[(i + 1) & 1]
        if i + 1 < len(batches):
            a = args[i + 1]
            out = cur.forward_prepared_prep_next(args[i][0], nxt, a[1], a[2], a[3], batches[i + 1].num_nodes)
        else:
            out = cur.forward_prepared(args[i][0])
        assert cur.last_path() == "layerwise" and torch.equal(out, want[i]), i
    for cm in pair:
        cm.check()


def test_a_captured_forward_replays_with_the_eager_bits(dev):
    model = _model(3, 4, 9, 32, seed=6)
    b = _model_batch(12, 9, seed=24)
    cm = _compiled(model, b)
    xd, cood, nptr, eptr = to_dev(b, dev)
    eager = cm.forward(xd, cood, nptr, eptr).clone()  # (also the warm-up outside the capture: kernel attributes, caches)
    out = torch.zeros_like(eager)
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        cm.forward(xd, cood, nptr, eptr, out=out)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    x2 = np.random.default_rng(2).uniform(-1, 1, b.x.shape).astype(np.float32)  # fresh features in the captured input buffer
    xd.copy_(torch.from_numpy(x2))
    graph.replay()
    torch.cuda.synchronize()
    record("forward/gat-captured", out.cpu().numpy(), R.forward64(model, b, x2), R.run(model, b, x2))
    cm.check()


# ---------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals(dev):
    model = _model(2, 4, 9, 32)
    b = _model_batch(12, 9, seed=25)
    cm = _compiled(model, b)
    xd, cood, nptr, eptr = to_dev(b, dev)
    good = cm.forward(xd, cood, nptr, eptr).clone()
    ea = torch.zeros((b.num_edges, 3), device=dev)
    # no edge attributes: the _edges entries refuse the model as one without edge weights
    with pytest.raises(runtime.GnnbError, match="GINE or PNAE"):
        cm.forward_edges(xd, ea, cood, nptr, eptr)
    assert cm.lib.gnnb_forward_batched_edges(cm._model, cm._ws, xd.data_ptr(), ea.data_ptr(), cood.data_ptr(), nptr.data_ptr(), eptr.data_ptr(),
                                             b.num_graphs, b.num_nodes, b.num_edges, good.data_ptr(), None) == -1
    assert b"gnnb_forward_batched_edges" in cm.lib.gnnb_last_error() and b"no edge weights" in cm.lib.gnnb_last_error()
    cm.graph_prep(cood, nptr, eptr, b.num_nodes)
    assert cm.lib.gnnb_forward_prepared_edges(cm._model, cm._ws, xd.data_ptr(), ea.data_ptr(), good.data_ptr(), None) == -1
    assert b"gnnb_forward_prepared_edges" in cm.lib.gnnb_last_error() and b"no edge weights" in cm.lib.gnnb_last_error()
    with pytest.raises(runtime.GnnbError, match="GINE or PNAE"):
        cm.enable_edge_ingest()
    # the ordered ingest serves the stack kernels' promise: refused, naming the entry that runs the model
    ordered = _compiled(model, b)
    ordered.enable_ordered_ingest()
    ei, batch_dev = _t(np.ascontiguousarray(b.coo.T.astype(np.int64)).reshape(2, -1), dev), _t(batch_vector(b), dev)
    with pytest.raises(runtime.GnnbError, match=r"gnnb_forward_pyg_ordered: a GAT model \(gnnb_gatconv_model_create\).*call gnnb_forward_pyg "):
        ordered.forward_pyg_ordered(xd, ei, batch=batch_dev, num_graphs=b.num_graphs)
    # a model does not run on the workspace of one with other heads, another slope, or another kind with the same description
    kw = dict(in_dim=9, hidden=32, layers=2, mlp_layers=1, out_act=torch.nn.LogSoftmax)
    steeper = make_gat_model(heads=4, **kw)
    for conv in steeper.gnn_convs:
        conv.negative_slope = conv.conv.negative_slope = 0.1
    for other_model in (make_gat_model(heads=2, **kw), steeper, make_gatv2_model(heads=4, **kw), make_model("gcn", in_dim=9, hidden=32, layers=2)):
        other = _compiled(other_model, b)
        if bytes(cm.desc) != bytes(other.desc):  # (the plain GCN model of helpers has its own head)
            continue
        other.graph_prep(cood, nptr, eptr, b.num_nodes)
        assert cm.lib.gnnb_forward_prepared(cm._model, other._ws, xd.data_ptr(), good.data_ptr(), None) == -1
        assert b"different model" in cm.lib.gnnb_last_error()
        assert cm.lib.gnnb_forward_prepared(other._model, cm._ws, xd.data_ptr(), good.data_ptr(), None) == -1
        assert b"different model" in cm.lib.gnnb_last_error()
    v2 = _compiled(make_gatv2_model(heads=4, **kw), b)
    assert bytes(cm.desc) == bytes(v2.desc) and v2.lib.gnnb_model_gatconv_heads(v2._model) == 0 and v2.lib.gnnb_model_gat_heads(v2._model) == 4
    # the stage entry checks its operands on the host, before any launch
    N = b.num_nodes
    z = lambda *shape: torch.zeros(shape, device=dev)  # noqa: E731
    with pytest.raises(runtime.GnnbError, match="divisible by heads"):
        cm.aggregate_gat(z(N, 30), z(N, 4), z(N, 4), heads=4)
    with pytest.raises(runtime.GnnbError, match="at most 256"):
        cm.aggregate_gat(z(N, 264), z(N, 4), z(N, 4), heads=4)
    for heads in (9, 0):
        with pytest.raises(runtime.GnnbError, match="heads must be"):
            cm.aggregate_gat(z(N, 32), z(N, 4), z(N, 4), heads=heads)
    for bad, what in ((dict(s_src=z(N, 2)), "s_src"), (dict(s_dst=z(N, 8)), "s_dst must be"), (dict(s_src=z(N - 1, 4)), "s_src"),
                      (dict(xl=z(N - 1, 32)), "xl"), (dict(bias=z(16)), "bias"), (dict(skip=z(N, 16)), "skip has shape"),
                      (dict(skip=z(N - 1, 32)), "skip must be"), (dict(out=z(N, 16)), "out"), (dict(act="swish"), "act must be"),
                      (dict(xl=z(N, 32).double()), "xl"), (dict(s_dst=z(N, 4).cpu()), "s_dst"), (dict(bias=z(32).cpu()), "bias")):
        args = dict(xl=z(N, 32), s_src=z(N, 4), s_dst=z(N, 4), heads=4)
        args.update(bad)
        with pytest.raises(runtime.GnnbError, match=what):
            cm.aggregate_gat(args.pop("xl"), args.pop("s_src"), args.pop("s_dst"), **args)
    # ... and the C entry itself: heads that do not divide the width, width > 256, heads > 8, a row stride below the width, score
    # strides below heads, a slope that is not finite, a NULL operand, a workspace whose tables keep explicit self loops
    xl = z(N, 264)
    call = lambda ws, ld, heads, width, lds=8, ldd=8, slope=0.2, ss=xl.data_ptr(): cm.lib.gnnb_aggregate_gat(  # noqa: E731
        ws, xl.data_ptr(), ld, ss, lds, xl.data_ptr(), ldd, None, None, 4, heads, slope, xl.data_ptr(), width, None)
    for kwargs in (dict(ld=32, heads=3, width=32), dict(ld=264, heads=4, width=264), dict(ld=36, heads=9, width=36), dict(ld=16, heads=4, width=32),
                   dict(ld=32, heads=4, width=32, lds=3), dict(ld=32, heads=4, width=32, ldd=3), dict(ld=32, heads=4, width=32, slope=float("nan")),
                   dict(ld=32, heads=4, width=32, ss=None)):
        assert call(cm._ws, **kwargs) == -1 and b"bad argument" in cm.lib.gnnb_last_error(), kwargs
    gin = runtime.CompiledModel.from_model(make_model("gin", in_dim=9, hidden=8, layers=1, out_dim=8), b.num_graphs, b.num_nodes, b.num_edges)
    gin.graph_prep(cood, nptr, eptr, b.num_nodes)
    assert call(gin._ws, 32, 4, 32) == -1 and b"GCN workspace" in cm.lib.gnnb_last_error()
    # nothing above left a flag or changed a result
    cm.check()
    assert torch.equal(cm.forward(xd, cood, nptr, eptr), good)
