"""TransformerConv models with edge features on the MI355X (include/gnnb_transformer_edge.h; csrc/k_transformer_edge.hip): the
fused dot-product attention aggregate with its edge term as a stage entry, the score term and the value term apart, zero
attributes, its epilogue, its bits, explicit self loops as edges with their attributes, whole models through ``forward_edges`` and
``forward_pyg_edges``, the promises, a captured forward, and the refusals.

Acceptance is ``ref64.budget`` with the project's K = 4, F = 2^-22 -- no tolerance of this file's own -- per
in-degree class (``gine_util.budget_by_degree``), nothing left out of a comparison.  The reference is float64
(``transformere_util.transformere_ref``: the projected edge term formed explicitly per edge, an explicit two-pass softmax; whole
models: the model's own torch definition on a ``.double()`` copy); ``base`` is the same in fp32 on the CPU.  The stage's operands
lie on dyadic grids and the scale is a power of two, so every score is exact in fp32 -- ASSERTED on the reference alone -- and only
``exp`` and the sums differ between ``got``, ``base`` and ``ref``.  Worst e / e32 per entry go to GNNB_FP64_REPORT=<file>
(DESIGN.md section 4)."""
import json
import os
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import ref64 as R
from gine_util import budget_by_degree, edge_attrs, forward64, run
from gnnbuilder_amd import runtime, synthetic
from gnnbuilder_amd.batching import from_pyg_batch, pack_graphs
from helpers import EMPTY, ONE, batch_vector, edge_batch, looped_graph, make_model, sweep_batch, to_dev
from transformer_util import SHAPES, make_transformer_model
from transformere_util import EDGE_DIMS, assert_exact_scores, edge_case, make_transformere_model, transformere_ref

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


def _workspace(batch, slack=1, conv="gin"):
    """A GIN workspace for the stage entry (graph prep keeps explicit (v, v) edges there; its tables do not depend on the model
    otherwise): of exactly the batch's size, or ``slack`` times as large."""
    return runtime.CompiledModel.from_model(make_model(conv, in_dim=8, hidden=8, layers=1, out_dim=8), slack * batch.num_graphs,
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


def _ref_pair(c, coo, heads, root=True, skip=False, act="none", **kw):
    args = (c["q"], c["k"], c["v"], c["qe"], c["root"] if root else None, c["skip"] if skip else None, act, coo, c["edge_attr"], c["w_edge"],
            heads, c["scale"])
    return transformere_ref(*args, **kw), transformere_ref(*args, dtype=np.float32)


def _refs(kind, width, heads, d, operands):
    """The operands of one stage case and its references (with root, no skip, no activation), computed once and shared (never
    changed)."""
    key = (kind, width, heads, d, operands)
    if key not in CASES:
        b = _batch(kind, width)
        c = edge_case(b.coo, b.num_nodes, width, heads, d, operands)
        (ref, a, adst, s), base = _ref_pair(c, b.coo, heads, return_weights=True)
        CASES[key] = dict(c=c, ref=ref, base=base, a=a, adst=adst, s=s)
    return CASES[key]


# the covering set: every edge_dim at the 16-byte form of 8 lanes, the scalar form, the scalar form of four strides and the widest
# layer; edge_dim 4 at the others
FULL = ((32, 4), (9, 3), (130, 2), (256, 8))
STAGE = [(w, h, d) for w, h in SHAPES for d in EDGE_DIMS if d == 4 or (w, h) in FULL]


def _stage(cm, c, dev, heads, root=True, skip=False, act="none", place=_t, out=None):
    return cm.aggregate_transformer_edges(place(c["q"], dev), place(c["k"], dev), place(c["v"], dev), place(c["qe"], dev),
                                          place(c["edge_attr"], dev), place(c["w_edge"], dev), root=place(c["root"], dev) if root else None,
                                          skip=place(c["skip"], dev) if skip else None, act=act, heads=heads, scale=c["scale"], out=out)


def _batch_preconditions(b):
    coo = b.coo
    deg = np.bincount(coo[:, 1], minlength=b.num_nodes)
    # the hub: a row split over the workgroup; rows without in-edges; and the COO rows are NOT in CSR-by-destination order, so a
    # kernel that indexed the attributes by CSR slot and not through eid would read other rows
    assert deg.max() >= 1200 and (deg == 0).sum() >= 5
    assert not np.array_equal(np.argsort(coo[:, 1], kind="stable"), np.arange(len(coo)))
    return deg


@pytest.mark.parametrize("operands", ["flat", "steep"])
@pytest.mark.parametrize("kind", ["edge", "sweep"])
@pytest.mark.parametrize("width,heads,d", STAGE)
def test_stage_against_float64(dev, width, heads, d, kind, operands):
    b = _batch(kind, width)
    deg = _batch_preconditions(b)
    r = _refs(kind, width, heads, d, operands)
    c = r["c"]
    dst, s64 = assert_exact_scores(c, b.coo, heads)
    if operands == "flat":
        assert np.abs(s64).max() <= (width // heads + d) * c["scale"]
        heavy = np.zeros((b.num_nodes, heads), np.int64)
        np.add.at(heavy, r["adst"], r["a"] > 0.05)
        assert (heavy.max(1) >= 3).sum() >= 60  # many neighbours carry weight
    else:
        big = np.zeros((b.num_nodes, heads))
        np.maximum.at(big, dst, np.abs(s64))
        assert (big.max(1) > 200.0).sum() >= 200  # exp without the max subtraction overflows there
    cm = _prepared(kind, width, dev)
    got = _stage(cm, c, dev, heads)
    cm.check()
    got = got.cpu().numpy()
    assert got.shape == (b.num_nodes, width) and np.isfinite(got).all()
    assert np.array_equal(got[deg == 0].view(np.uint32), c["root"][deg == 0].view(np.uint32))  # in-degree 0: root, bit for bit
    record_classes(f"aggregate_transformer_edges/{kind}-w{width}-h{heads}-d{d}-{operands}", got, r["ref"], r["base"], b.coo)


# ---------------------------------------------------------------------------------------------------- 2. the two terms apart
APART = [(32, 4, 4), (9, 3, 3), (130, 2, 16), (24, 2, 1)]


@pytest.mark.parametrize("width,heads,d", APART)
def test_the_score_term_alone(dev, width, heads, d):
    """``w_edge = 0`` with ``qe != 0``: the attributes move the weights and nothing else."""
    b = _batch("edge", width)
    c = dict(_refs("edge", width, heads, d, "flat")["c"])
    c["w_edge"] = np.zeros_like(c["w_edge"])
    ref, base = _ref_pair(c, b.coo, heads)
    no_edges = _ref_pair(dict(c, qe=np.zeros_like(c["qe"])), b.coo, heads)[0]
    assert np.abs(ref - no_edges).max() > 1e-3  # (the term is there, on the reference)
    cm = _prepared("edge", width, dev)
    got = _stage(cm, c, dev, heads)
    cm.check()
    record_classes(f"aggregate_transformer_edges/edge-w{width}-h{heads}-d{d}-score-only", got.cpu().numpy(), ref, base, b.coo)


@pytest.mark.parametrize("width,heads,d", APART)
def test_the_value_term_alone(dev, width, heads, d):
    """``qe = 0`` with ``w_edge != 0``: the weights are the plain layer's, the projected attributes ride on the values."""
    b = _batch("edge", width)
    c = dict(_refs("edge", width, heads, d, "flat")["c"])
    c["qe"] = np.zeros_like(c["qe"])
    ref, base = _ref_pair(c, b.coo, heads)
    no_edges = _ref_pair(dict(c, w_edge=np.zeros_like(c["w_edge"])), b.coo, heads)[0]
    assert np.abs(ref - no_edges).max() > 1e-3
    cm = _prepared("edge", width, dev)
    got = _stage(cm, c, dev, heads)
    cm.check()
    record_classes(f"aggregate_transformer_edges/edge-w{width}-h{heads}-d{d}-value-only", got.cpu().numpy(), ref, base, b.coo)


@pytest.mark.parametrize("width,heads,d", APART)
def test_zero_queries_give_the_mean_of_the_messages(dev, width, heads, d):
    b = _batch("edge", width)
    coo = b.coo
    c = dict(_refs("edge", width, heads, d, "flat")["c"])
    c["q"], c["qe"] = np.zeros_like(c["q"]), np.zeros_like(c["qe"])
    cnt = np.bincount(coo[:, 1], minlength=b.num_nodes)

    def mean(dtype):
        msg = c["v"].astype(dtype)[coo[:, 0]] + c["edge_attr"].astype(dtype) @ c["w_edge"].astype(dtype).T
        acc = np.zeros(c["v"].shape, dtype)
        np.add.at(acc, coo[:, 1], msg.astype(dtype))
        return acc / np.maximum(cnt, 1).astype(dtype)[:, None] + c["root"].astype(dtype)

    cm = _prepared("edge", width, dev)
    got = _stage(cm, c, dev, heads)
    cm.check()
    record_classes(f"aggregate_transformer_edges/edge-w{width}-h{heads}-d{d}-q0", got.cpu().numpy(), mean(np.float64), mean(np.float32), coo)


# ---------------------------------------------------------------------------------------------------- 3. zero attributes
@pytest.mark.parametrize("kind", ["edge", "sweep"])
@pytest.mark.parametrize("width,heads,d", [(32, 4, 4), (9, 3, 3), (130, 2, 16), (256, 8, 16), (32, 1, 1)])
def test_zero_attributes_give_the_values_of_aggregate_transformer(dev, width, heads, d, kind):
    c = dict(_refs(kind, width, heads, d, "flat")["c"])
    c["edge_attr"] = np.zeros_like(c["edge_attr"])
    assert np.abs(c["qe"]).max() > 0 and np.abs(c["w_edge"]).max() > 0
    cm = _prepared(kind, width, dev)
    got = _stage(cm, c, dev, heads, skip=True, act="tanh")
    plain = cm.aggregate_transformer(_t(c["q"], dev), _t(c["k"], dev), _t(c["v"], dev), root=_t(c["root"], dev), skip=_t(c["skip"], dev),
                                     act="tanh", heads=heads, scale=c["scale"])
    cm.check()
    assert torch.equal(got, plain)  # (value equality: a signed zero does not matter)


# ---------------------------------------------------------------------------------------------------- 4. the epilogue
@pytest.mark.parametrize("with_root", [True, False])
@pytest.mark.parametrize("act", ["relu", "gelu", "sigmoid", "tanh"])
@pytest.mark.parametrize("d", [4, 3])
def test_epilogue_root_skip_and_activation(dev, act, with_root, d):
    """Width 32, heads 4, with ``skip``: ``q`` / ``k`` / ``v`` / ``root`` / ``qe`` as the column blocks of one
    [N, 4 w + roundup4(H d)] tensor (the layer's GEMM output: the 16-byte form) and as separate tensors one float past a 16-byte
    boundary with ``edge_attr`` and ``w_edge`` misaligned too (the scalar form), ``out=`` given."""
    width, heads = 32, 4
    b = _batch("edge", width)
    coo = b.coo
    c = _refs("edge", width, heads, d, "flat")["c"]
    ref, base = _ref_pair(c, coo, heads, root=with_root, skip=True, act=act)
    cm = _prepared("edge", width, dev)
    hd = heads * d
    pad = np.zeros((b.num_nodes, -hd % 4), np.float32)
    five = _t(np.concatenate([c["q"], c["k"], c["v"], c["root"], c["qe"], pad], 1), dev)
    assert five.shape == (b.num_nodes, 4 * width + (hd + 3) // 4 * 4) and all(five[:, i * 32:].data_ptr() % 16 == 0 for i in range(5))
    kw = dict(act=act, heads=heads, scale=c["scale"])
    blocks = cm.aggregate_transformer_edges(five[:, :32], five[:, 32:64], five[:, 64:96], five[:, 128:128 + hd], _t(c["edge_attr"], dev),
                                            _t(c["w_edge"], dev), root=five[:, 96:128] if with_root else None, skip=_t(c["skip"], dev), **kw)
    out = _offset(np.zeros((b.num_nodes, width), np.float32), dev)
    scalar = _stage(cm, c, dev, heads, root=with_root, skip=True, act=act, place=_offset, out=out)
    cm.check()
    assert scalar.data_ptr() == out.data_ptr()
    entry = f"aggregate_transformer_edges/epilogue-d{d}-{act}" + ("" if with_root else "-noroot")
    record_classes(entry + "/blocks", blocks.cpu().numpy(), ref, base, coo)
    record_classes(entry + "/scalar", scalar.cpu().numpy(), ref, base, coo)
    if act == "relu":  # in-degree 0: relu(root_i + skip_i), or relu(skip_i) without root -- one fp32 add at most, exact bits
        lone = np.bincount(coo[:, 1], minlength=b.num_nodes) == 0
        want = np.maximum((c["root"] + c["skip"]) if with_root else c["skip"], np.float32(0))[lone]
        assert np.array_equal(blocks.cpu().numpy()[lone], want) and np.array_equal(scalar.cpu().numpy()[lone], want)


# ---------------------------------------------------------------------------------------------------- 5. bits
@pytest.mark.parametrize("width,heads,d", [(32, 4, 4), (9, 3, 3), (130, 2, 16)])
def test_a_repeat_launch_and_another_grid_give_the_same_bits(dev, width, heads, d):
    b = _batch("edge", width)
    c = _refs("edge", width, heads, d, "flat")["c"]
    cm = _prepared("edge", width, dev)
    first = _stage(cm, c, dev, heads, skip=True, act="tanh")
    assert torch.equal(_stage(cm, c, dev, heads, skip=True, act="tanh"), first)
    # the same batch on a workspace with 16 times the capacities: graph prep cuts other node tiles there.  The kernel's grid is cut
    # from the batch alone; other grids and several steps per workgroup are test_many_steps_per_workgroup's
    big = _workspace(b, slack=16)
    _prep(big, b, dev)
    assert torch.equal(_stage(big, c, dev, heads, skip=True, act="tanh"), first)
    cm.check(), big.check()


def _launch_steps(num_nodes, width, heads):
    """(steps, lane groups per workgroup) of ``launch_transformer_edge_aggregate`` on aligned operands: an item = (row, head), a
    lane group of the smallest power of two >= C / VEC lanes (at most 64) per item, a step = one item per lane group of a 256-lane
    workgroup."""
    c = width // heads
    nvec = c // 4 if c % 4 == 0 else c
    lanes = 1
    while lanes < nvec and lanes < 64:
        lanes *= 2
    groups = 256 // lanes
    return -(-num_nodes * heads // groups), groups


def _wg_per_cu():
    """``TFE_WG_PER_CU`` of csrc/k_transformer_edge.hip: the most workgroups per CU the grid is cut for."""
    src = (Path(runtime.CSRC_DIR) / "k_transformer_edge.hip").read_text()
    return int(re.search(r"constexpr int TFE_WG_PER_CU = (\d+);", src).group(1))


# (width, heads, copies, edge_dim, operand set): the 16-byte form at 8 lanes per item and the scalar form over four strides of a
# wave at edge_dim 16, the 16-byte form at 32 lanes per item (a wave shuffle in the score sum) at edge_dim 3
MANY_STEPS = [(256, 8, 8, 16, "flat"), (130, 2, 4, 16, "steep"), (128, 1, 12, 3, "flat")]


@pytest.mark.parametrize("width,heads,copies,d,operands", MANY_STEPS)
def test_many_steps_per_workgroup(dev, width, heads, copies, d, operands):
    """``copies`` copies of the sweep batch in one batch, every copy with the first copy's operand rows: more steps than the grid
    can hold at ``TFE_WG_PER_CU`` workgroups per CU on this device (ASSERTED), so every workgroup walks two steps or more -- the
    three-deep pipeline's rotation, the slot prefetch of the next step, the long rows' second walk at a later step -- and the last
    copy's rows, hubs included, are taken at a later step by another workgroup and lane group than the first copy's.  All rows are
    held against float64 (a copy's graphs are closed, so its reference is the one batch's); every copy has the first copy's bits,
    and those are the bits of the one batch launched alone on its own, smaller grid."""
    b = _batch("sweep", width)
    n = b.num_nodes
    long = pack_graphs([b.graph(g) for g in range(b.num_graphs)] * copies)
    assert long.num_nodes == copies * n and long.num_edges == copies * b.num_edges
    # (a copy's COO rows follow the copy before it, so the tiled attribute rows belong to the tiled edges)
    assert np.array_equal(long.coo[b.num_edges:2 * b.num_edges] - n, b.coo)
    steps, groups = _launch_steps(long.num_nodes, width, heads)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert steps > _wg_per_cu() * cus  # the grid holds at most that many workgroups: two steps or more for each
    assert (copies - 1) * n * heads // groups >= (steps + 1) // 2  # the last copy begins behind the grid's first sweep
    r = _refs("sweep", width, heads, d, operands)
    c = r["c"]
    assert_exact_scores(c, b.coo, heads)
    tiled = {k: (np.tile(v, (copies, 1)) if k in ("q", "k", "v", "qe", "root", "skip", "edge_attr") else v) for k, v in c.items()}
    cl = _workspace(long)
    _prep(cl, long, dev)
    got = _stage(cl, tiled, dev, heads)
    cl.check()
    alone = _stage(_prepared("sweep", width, dev), c, dev, heads)
    assert torch.equal(got[:n], alone)
    for k in range(1, copies):
        assert torch.equal(got[k * n:(k + 1) * n], got[:n]), k
    assert np.bincount(long.coo[:, 1], minlength=long.num_nodes)[(copies - 1) * n:].max() >= 1200  # (a hub in the last copy)
    record_classes(f"aggregate_transformer_edges/sweep-x{copies}-w{width}-h{heads}-d{d}-{operands}", got.cpu().numpy(),
                   np.tile(r["ref"], (copies, 1)), np.tile(r["base"], (copies, 1)), long.coo)


# ---------------------------------------------------------------------------------------------------- 6. explicit self loops
@pytest.mark.parametrize("d", [3, 4])
def test_explicit_self_loops_are_edges_with_their_attributes(dev, d):
    width, heads = 24, 2
    x, coo = looped_graph(40, width, seed=3)
    assert (coo[:, 0] == coo[:, 1]).sum() >= 10
    others = [ONE(width), (x[:7], np.array([[0, 1], [1, 0], [2, 1], [5, 1]], np.int32))]
    b = pack_graphs([(x, coo)] + others)
    loops = b.coo[:, 0] == b.coo[:, 1]
    c = edge_case(b.coo, b.num_nodes, width, heads, d, "flat")
    moved = dict(c, edge_attr=np.where(loops[:, None], -c["edge_attr"] + np.float32(0.25), c["edge_attr"]).astype(np.float32))
    looped = np.unique(b.coo[loops][:, 1])
    cm = _workspace(b)
    _prep(cm, b, dev)
    first, second = _stage(cm, c, dev, heads), _stage(cm, moved, dev, heads)
    cm.check()
    # changing only the (v, v) rows' attributes changes v's output, and no other row's
    diff = (first != second).any(1).cpu().numpy()
    assert diff[looped].all() and not np.delete(diff, looped).any()
    for name, case, got in (("looped", c, first), ("looped-moved", moved, second)):
        ref, base = _ref_pair(case, b.coo, heads)
        record(f"aggregate_transformer_edges/{name}-d{d}", got.cpu().numpy(), ref, base)
    # a GCN workspace's tables have dropped the (v, v) edges: the stage call is refused, nothing launched
    gcn = _workspace(b, conv="gcn")
    _prep(gcn, b, dev)
    with pytest.raises(runtime.GnnbError, match="explicit self loops"):
        _stage(gcn, c, dev, heads)
    gcn.check()


# ---------------------------------------------------------------------------------------------------- 7. whole models
def _model_batch(graphs, in_dim, seed):
    """``graphs`` synthetic qm9-like graphs with seeded features of width ``in_dim``, an empty and a one-node graph among them"""
    mols, rng = synthetic.make_batch("qm9", graphs, seed=seed), np.random.default_rng(seed)
    gs = [(rng.uniform(-1, 1, (mols.graph(g)[0].shape[0], in_dim)).astype(np.float32), mols.graph(g)[1]) for g in range(graphs)]
    return pack_graphs(gs[:graphs // 2] + [EMPTY(in_dim), ONE(in_dim)] + gs[graphs // 2:] + [EMPTY(in_dim)])


def _model(layers, heads, in_dim, hidden, d, seed=0):
    return make_transformere_model(in_dim=in_dim, edge_dim=d, hidden=hidden, layers=layers, heads=heads, skip=True,
                                   pools=("add", "mean", "max"), mlp_layers=1, out_act=torch.nn.LogSoftmax, seed=seed)


def _compiled(model, b, promise=0, degree=0, ingest=False):
    cm = runtime.CompiledModel.from_model(model, b.num_graphs, b.num_nodes, b.num_edges)
    if ingest:  # (right after construction: before a batch is prepared on the workspace)
        cm.enable_edge_ingest()
    if promise:
        cm.set_max_graph_nodes(promise)
    if degree:
        cm.set_max_degree(degree)
    return cm


# (in, hidden, graphs, edge_dim) x heads x layers; the second has heads * edge_dim no multiple of 4 (padding columns in the GEMM
# output); the last is the widest layer the model kind takes: 4 * 256 + 8 * 16 = 1152 GEMM columns
MODELS = [(layers, heads, in_dim, hidden, graphs, d) for in_dim, hidden, graphs, d in ((9, 32, 64, 4), (11, 128, 12, 3)) for heads in (1, 4)
          for layers in (1, 2, 3)] + [(2, 8, 9, 256, 12, 16)]


@pytest.mark.parametrize("layers,heads,in_dim,hidden,graphs,d", MODELS)
def test_whole_models_against_float64(dev, layers, heads, in_dim, hidden, graphs, d):
    model = _model(layers, heads, in_dim, hidden, d, seed=layers)
    b = _model_batch(graphs, in_dim, seed=31 + layers)
    ea = edge_attrs(b.num_edges, d, seed=32 + layers)
    assert b.num_graphs == graphs + 3
    cm = _compiled(model, b, ingest=True)
    assert cm.lib.gnnb_model_transformer_heads(cm._model) == heads and cm.lib.gnnb_model_edge_dim(cm._model) == d
    assert cm.lib.gnnb_model_gat_heads(cm._model) == 0
    xd, cood, nptr, eptr = to_dev(b, dev)
    ead = _t(ea, dev)
    out = cm.forward_edges(xd, ead, cood, nptr, eptr)
    cm.check()
    assert cm.last_path() == "layerwise" and out.shape == (b.num_graphs, 19)
    entry = f"forward_edges/transformere-L{layers}-h{heads}-in{in_dim}-w{hidden}-d{d}"
    record(entry, out.cpu().numpy(), forward64(model, b, b.x, ea), run(model, b, b.x, ea))
    # the same forward again, and the prepared form, give the same bits (no atomics, a fixed summation order)
    assert torch.equal(cm.forward_edges(xd, ead, cood, nptr, eptr), out)
    assert torch.equal(cm.forward_prepared_edges(xd, ead), out)
    # ... and the PyG mini-batch through the device ingest, its edges and attribute rows shuffled together: the ingest's arrays are
    # the host's for that input, and so are the bits
    perm = np.random.default_rng(layers).permutation(b.num_edges)
    ei_sh = np.ascontiguousarray(b.coo.T.astype(np.int64)[:, perm])
    ea_sh = np.ascontiguousarray(ea[perm])
    gb, ea_ord = from_pyg_batch(b.x, ei_sh, edge_attr=ea_sh, batch=batch_vector(b), num_graphs=b.num_graphs)
    pyg = cm.forward_pyg_edges(xd, _t(ei_sh, dev), _t(ea_sh, dev), batch=_t(batch_vector(b), dev), num_graphs=b.num_graphs).clone()
    cm.check()
    assert cm.last_path() == "layerwise"
    record(entry + "-pyg", pyg.cpu().numpy(), forward64(model, gb, b.x, ea_ord), run(model, gb, b.x, ea_ord))
    host = cm.forward_edges(xd, _t(ea_ord, dev), _t(gb.coo, dev), _t(gb.node_ptr, dev), _t(gb.edge_ptr, dev))
    assert torch.equal(pyg, host)


# ---------------------------------------------------------------------------------------------------- 8. the other forwards
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
    record("forward_edges/transformere-L3-h4-promises", outs[-1].cpu().numpy(), forward64(model, b, b.x, ea), run(model, b, b.x, ea))


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
    record("forward_edges/transformere-captured", out.cpu().numpy(), forward64(model, b, x2, ea2), run(model, b, x2, ea2))
    cm.check()


# ---------------------------------------------------------------------------------------------------- 9. refusals
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
    with pytest.raises(runtime.GnnbError, match="gnnb_forward_pyg_ordered.*gnnb_forward_pyg_edges"):
        ordered.forward_pyg_ordered(xd, ei, batch=batch_dev, num_graphs=b.num_graphs)
    # a model does not run on the workspace of one with another edge_dim or other heads, nor on a plain TransformerConv model's,
    # nor that one on this model's -- all with the same description
    N, E = b.num_nodes, b.num_edges
    plain = _compiled(make_transformer_model(in_dim=9, hidden=32, layers=2, heads=4, mlp_layers=1, out_act=torch.nn.LogSoftmax), b)
    for other in (_compiled(_model(2, 4, 9, 32, 3), b), _compiled(_model(2, 2, 9, 32, 4), b), plain):
        assert bytes(cm.desc) == bytes(other.desc)
        other.graph_prep(cood, nptr, eptr, N)
        assert cm.lib.gnnb_forward_prepared_edges(cm._model, other._ws, xd.data_ptr(), ea.data_ptr(), good.data_ptr(), None) == -1
        assert b"different model" in cm.lib.gnnb_last_error()
    cm.graph_prep(cood, nptr, eptr, N)
    assert cm.lib.gnnb_forward_prepared(plain._model, cm._ws, xd.data_ptr(), good.data_ptr(), None) == -1
    assert b"gnnb_forward_prepared_edges" in cm.lib.gnnb_last_error()  # (the workspace is an edge model's: the entry says so)
    assert cm.lib.gnnb_forward_prepared_edges(plain._model, cm._ws, xd.data_ptr(), ea.data_ptr(), good.data_ptr(), None) == -1
    assert b"no edge weights" in cm.lib.gnnb_last_error()
    # edge_attr of another shape, dtype or device is refused before any launch
    for bad, what in ((ea[:-1], "edge_attr must be"), (torch.zeros((E, 5), device=dev), "edge_attr has shape"), (ea.double(), "float32"),
                      (ea.cpu(), "CUDA"), (None, "edge_attr is required")):
        with pytest.raises(runtime.GnnbError, match=what):
            cm.forward_edges(xd, bad, cood, nptr, eptr)
    # the stage entry checks its operands on the host, before any launch
    z = lambda *shape: torch.zeros(shape, device=dev)  # noqa: E731
    with pytest.raises(runtime.GnnbError, match="divisible by heads"):
        cm.aggregate_transformer_edges(z(N, 30), z(N, 30), z(N, 30), z(N, 16), z(E, 4), z(30, 4), heads=4)
    with pytest.raises(runtime.GnnbError, match="at most 256"):
        cm.aggregate_transformer_edges(z(N, 264), z(N, 264), z(N, 264), z(N, 16), z(E, 4), z(264, 4), heads=4)
    for heads in (9, 0, True):
        with pytest.raises(runtime.GnnbError, match="heads must be"):
            cm.aggregate_transformer_edges(z(N, 32), z(N, 32), z(N, 32), z(N, 16), z(E, 4), z(32, 4), heads=heads)
    for bad, what in ((dict(k=z(N, 16)), "k "), (dict(v=z(N, 16)), "v "), (dict(q=z(N - 1, 32)), "q "), (dict(root=z(N, 16)), "root"),
                      (dict(skip=z(N, 16)), "skip has shape"), (dict(skip=z(N - 1, 32)), "skip must be"), (dict(out=z(N, 16)), "out"),
                      (dict(act="swish"), "act must be"), (dict(q=z(N, 32).double()), "q "), (dict(k=z(N, 32).cpu()), "k "),
                      (dict(scale=float("inf")), "scale"), (dict(qe=z(N, 12)), "qe "), (dict(qe=z(N - 1, 16)), "qe "), (dict(qe=z(N, 20)), "qe must be"),
                      (dict(qe=z(N, 16).cpu()), "qe "), (dict(w_edge=z(32, 17)), "w_edge must be"), (dict(w_edge=z(16, 4)), "w_edge"),
                      (dict(w_edge=z(32, 4).cpu()), "w_edge"), (dict(edge_attr=z(E, 3)), "edge_attr has shape"),
                      (dict(edge_attr=z(E - 1, 4)), "edge_attr must be"), (dict(edge_attr=None), "edge_attr is required"),
                      (dict(edge_attr=z(E, 4).double()), "float32")):
        args = dict(q=z(N, 32), k=z(N, 32), v=z(N, 32), qe=z(N, 16), edge_attr=z(E, 4), w_edge=z(32, 4), heads=4)
        args.update(bad)
        with pytest.raises(runtime.GnnbError, match=what):
            cm.aggregate_transformer_edges(args.pop("q"), args.pop("k"), args.pop("v"), args.pop("qe"), args.pop("edge_attr"), args.pop("w_edge"),
                                           **args)
    # ... and the C entry itself: what gnnb_aggregate_transformer refuses (heads that do not divide the width, width > 256, heads > 8, a
    # stride below the width), edge_dim out of range, ldqe < heads * edge_dim, ldwe < edge_dim, NULL qe, we, edge_attr (the batch has
    # edges), and a GCN workspace
    x = z(max(N, E), 264)
    p = x.data_ptr()

    def call(ws, lds=(32,) * 4, heads=4, width=32, root=None, qe=p, ldqe=16, ea_ptr=p, ed=4, we=p, ldwe=4):
        return cm.lib.gnnb_aggregate_transformer_edges(ws, p, lds[0], p, lds[1], p, lds[2], qe, ldqe, root, lds[3], None, 4, heads, 0.5, ea_ptr, ed,
                                                       we, ldwe, p, width, None)

    assert E > 0
    for kw in (dict(heads=3), dict(lds=(264,) * 4, width=264), dict(lds=(36,) * 4, heads=9, width=36, ldqe=36), dict(lds=(16, 32, 32, 32)),
               dict(lds=(32, 16, 32, 32)), dict(lds=(32, 32, 16, 32)), dict(lds=(32, 32, 32, 16), root=p), dict(ed=0), dict(ed=17, ldqe=68, ldwe=17),
               dict(ldqe=15), dict(ldwe=3), dict(qe=None), dict(we=None), dict(ea_ptr=None)):
        assert call(cm._ws, **kw) == -1 and b"bad argument" in cm.lib.gnnb_last_error(), kw
    gcn = runtime.CompiledModel.from_model(make_model("gcn", in_dim=9, hidden=8, layers=1, out_dim=8), b.num_graphs, N, E)
    gcn.graph_prep(cood, nptr, eptr, N)
    assert call(gcn._ws) == -1 and b"explicit self loops" in cm.lib.gnnb_last_error()
    gcn.check()
    # nothing above left a flag or changed a result
    cm.check()
    assert torch.equal(cm.forward_edges(xd, ea, cood, nptr, eptr), good)
