"""TransformerConv models on the MI355X (include/gnnb_transformer.h; csrc/k_transformer.hip): the fused dot-product attention
aggregate as a stage entry, its epilogue, its bits, explicit self loops as edges, whole models through ``forward`` and
``forward_pyg``, the promises, a captured forward, and the refusals.

Acceptance is ``ref64.budget`` with the project's K = 4, F = 2^-22 -- no tolerance of this file's own -- per
in-degree class (``gine_util.budget_by_degree``), nothing left out of a comparison.  The reference is float64 (``transformer_util.
transformer_ref``: an explicit two-pass softmax; whole models: the model's own torch definition on a ``.double()`` copy); ``base``
is the same in fp32 on the CPU.  The stage's operands lie on dyadic grids and the scale is a power of two, so every score is exact
in fp32 -- ASSERTED on the reference alone -- and only ``exp`` and the sums differ between ``got``, ``base`` and ``ref``.  Worst
e / e32 per entry go to GNNB_FP64_REPORT=<file>."""
import json
import os
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import gnnbuilder_amd as gnnb
import ref64 as R
from gine_util import budget_by_degree
from gnnbuilder_amd import runtime, synthetic
from gnnbuilder_amd.batching import pack_graphs
from helpers import EMPTY, ONE, batch_vector, edge_batch, looped_graph, make_model, sweep_batch, to_dev
from transformer_util import SHAPES, make_transformer_model, stage_case, transformer_ref, transformer_scores

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
BATCHES, PREPARED = {}, {}


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


def _stage(cm, c, dev, heads, root=True, skip=False, act="none"):
    return cm.aggregate_transformer(_t(c["q"], dev), _t(c["k"], dev), _t(c["v"], dev), root=_t(c["root"], dev) if root else None,
                                    skip=_t(c["skip"], dev) if skip else None, act=act, heads=heads, scale=c["scale"])


def _refs(c, coo, heads, root=True, skip=False, act="none", **kw):
    args = (c["q"], c["k"], c["v"], c["root"] if root else None, c["skip"] if skip else None, act, coo, heads, c["scale"])
    return transformer_ref(*args, **kw), transformer_ref(*args, dtype=np.float32)


def _scores_are_exact(c, coo, heads):
    _, dst, s64 = transformer_scores(c["q"], c["k"], coo, heads, c["scale"], np.float64)
    _, _, s32 = transformer_scores(c["q"], c["k"], coo, heads, c["scale"], np.float32)
    assert s32.dtype == np.float32 and np.array_equal(s32.astype(np.float64), s64)  # every score is exact in fp32
    return dst, s64


@pytest.mark.parametrize("operands", ["flat", "steep"])
@pytest.mark.parametrize("kind", ["edge", "sweep"])
@pytest.mark.parametrize("width,heads", SHAPES)
def test_stage_against_float64(dev, width, heads, kind, operands):
    b = _batch(kind, width)
    coo = b.coo  # (a GIN workspace's tables: the batch's edges as they are)
    deg = np.bincount(coo[:, 1], minlength=b.num_nodes)
    # the hub: a row split over the workgroup; rows without in-edges
    assert deg.max() >= 1200 and (deg == 0).sum() >= 5
    c = stage_case(b.num_nodes, width, heads, operands)
    dst, s64 = _scores_are_exact(c, coo, heads)
    (ref, a, adst, _), base = _refs(c, coo, heads, return_weights=True)
    if operands == "flat":
        assert np.abs(s64).max() <= 2.0
        heavy = np.zeros((b.num_nodes, heads), np.int64)
        np.add.at(heavy, adst, a > 0.05)
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
    record_classes(f"aggregate_transformer/{kind}-w{width}-h{heads}-{operands}", got, ref, base, coo)


@pytest.mark.parametrize("width,heads", SHAPES)
def test_zero_query_is_the_mean_of_the_values(dev, width, heads):
    b = _batch("edge", width)
    coo = b.coo
    c = dict(stage_case(b.num_nodes, width, heads, "flat"))
    c["q"] = np.zeros_like(c["q"])
    cnt = np.bincount(coo[:, 1], minlength=b.num_nodes)

    def mean(dtype):
        acc = np.zeros(c["v"].shape, dtype)
        np.add.at(acc, coo[:, 1], c["v"].astype(dtype)[coo[:, 0]])
        return acc / np.maximum(cnt, 1).astype(dtype)[:, None] + c["root"].astype(dtype)

    cm = _prepared("edge", width, dev)
    got = _stage(cm, c, dev, heads)
    cm.check()
    record_classes(f"aggregate_transformer/edge-w{width}-h{heads}-q0", got.cpu().numpy(), mean(np.float64), mean(np.float32), coo)


# ---------------------------------------------------------------------------------------------------- 2. the epilogue
@pytest.mark.parametrize("with_root", [True, False])
@pytest.mark.parametrize("act", ["relu", "gelu", "sigmoid", "tanh"])
def test_epilogue_root_skip_and_activation(dev, act, with_root):
    """Width 32, heads 4, with ``skip``: ``q`` / ``k`` / ``v`` / ``root`` as the four column blocks of one [N, 128] tensor (row
    stride 128: the 16-byte form) and as separate tensors one float past a 16-byte boundary (the scalar form), ``out=`` given."""
    width, heads = 32, 4
    b = _batch("edge", width)
    coo = b.coo
    c = stage_case(b.num_nodes, width, heads, "flat")
    ref, base = _refs(c, coo, heads, root=with_root, skip=True, act=act)
    cm = _prepared("edge", width, dev)
    four = _t(np.concatenate([c["q"], c["k"], c["v"], c["root"]], 1), dev)
    assert four.shape == (b.num_nodes, 128) and all(four[:, i * 32:].data_ptr() % 16 == 0 for i in range(4))
    kw = dict(act=act, heads=heads, scale=c["scale"])
    blocks = cm.aggregate_transformer(four[:, :32], four[:, 32:64], four[:, 64:96], root=four[:, 96:] if with_root else None,
                                      skip=_t(c["skip"], dev), **kw)
    out = _offset(np.zeros((b.num_nodes, width), np.float32), dev)
    scalar = cm.aggregate_transformer(_offset(c["q"], dev), _offset(c["k"], dev), _offset(c["v"], dev),
                                      root=_offset(c["root"], dev) if with_root else None, skip=_offset(c["skip"], dev), out=out, **kw)
    cm.check()
    assert scalar.data_ptr() == out.data_ptr()
    entry = f"aggregate_transformer/epilogue-{act}" + ("" if with_root else "-noroot")
    record_classes(entry + "/blocks", blocks.cpu().numpy(), ref, base, coo)
    record_classes(entry + "/scalar", scalar.cpu().numpy(), ref, base, coo)
    if act == "relu":  # in-degree 0: relu(root_i + skip_i), or relu(skip_i) without root -- one fp32 add at most, exact bits
        lone = np.bincount(coo[:, 1], minlength=b.num_nodes) == 0
        want = np.maximum((c["root"] + c["skip"]) if with_root else c["skip"], np.float32(0))[lone]
        assert np.array_equal(blocks.cpu().numpy()[lone], want) and np.array_equal(scalar.cpu().numpy()[lone], want)


# ---------------------------------------------------------------------------------------------------- 3. bits
@pytest.mark.parametrize("width,heads", [(32, 4), (9, 3), (130, 2)])
def test_a_repeat_launch_and_another_grid_give_the_same_bits(dev, width, heads):
    b = _batch("edge", width)
    c = stage_case(b.num_nodes, width, heads, "flat")
    cm = _prepared("edge", width, dev)
    first = _stage(cm, c, dev, heads, skip=True, act="tanh")
    assert torch.equal(_stage(cm, c, dev, heads, skip=True, act="tanh"), first)
    # the same batch on a workspace with 16 times the capacities: graph prep cuts other node tiles there.  The kernel's grid is cut
    # from the batch alone (launch_transformer_aggregate); other grids and several steps per workgroup are
    # test_many_steps_per_workgroup's
    big = _workspace(b, slack=16)
    _prep(big, b, dev)
    assert torch.equal(_stage(big, c, dev, heads, skip=True, act="tanh"), first)
    cm.check(), big.check()


def _launch_steps(num_nodes, width, heads):
    """(steps, lane groups per workgroup) of ``launch_transformer_aggregate`` on aligned operands: an item = (row, head), a lane
    group of the smallest power of two >= C / VEC lanes (at most 64) per item, a step = one item per lane group of a 256-lane
    workgroup."""
    c = width // heads
    nvec = c // 4 if c % 4 == 0 else c
    lanes = 1
    while lanes < nvec and lanes < 64:
        lanes *= 2
    groups = 256 // lanes
    return -(-num_nodes * heads // groups), groups


def _wg_per_cu():
    """``TF_WG_PER_CU`` of csrc/k_transformer.hip: the most workgroups per CU the grid is cut for."""
    src = (Path(runtime.CSRC_DIR) / "k_transformer.hip").read_text()
    return int(re.search(r"constexpr int TF_WG_PER_CU = (\d+);", src).group(1))


# (width, heads, copies, operand set): the 16-byte form at 8 lanes per item, the scalar form over four strides of a wave, the
# 16-byte form at 32 lanes per item (a wave shuffle in the score sum)
MANY_STEPS = [(256, 8, 8, "flat"), (130, 2, 4, "steep"), (128, 1, 12, "flat")]


@pytest.mark.parametrize("width,heads,copies,operands", MANY_STEPS)
def test_many_steps_per_workgroup(dev, width, heads, copies, operands):
    """``copies`` copies of the sweep batch in one batch, every copy with the first copy's operand rows: more steps than the
    grid can hold at ``TF_WG_PER_CU`` workgroups per CU on this device (ASSERTED), so every workgroup walks two steps or more --
    the three-deep pipeline's rotation, the slot prefetch of the next step, the long rows' second walk at a later step -- and the
    last copy's rows, hubs included, are taken at a later step by another workgroup and lane group than the first copy's.  All
    rows are held against float64 (a copy's graphs are closed, so its reference is the one batch's); every copy has the first
    copy's bits, and those are the bits of the one batch launched alone on its own, smaller grid."""
    b = _batch("sweep", width)
    n = b.num_nodes
    long = pack_graphs([b.graph(g) for g in range(b.num_graphs)] * copies)
    assert long.num_nodes == copies * n
    steps, groups = _launch_steps(long.num_nodes, width, heads)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert steps > _wg_per_cu() * cus  # the grid holds at most that many workgroups: two steps or more for each
    assert (copies - 1) * n * heads // groups >= (steps + 1) // 2  # the last copy begins behind the grid's first sweep
    c = stage_case(n, width, heads, operands)
    _scores_are_exact(c, b.coo, heads)
    ref, base = _refs(c, b.coo, heads)
    tiled = {k: (np.tile(v, (copies, 1)) if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    cl = _workspace(long)
    _prep(cl, long, dev)
    got = _stage(cl, tiled, dev, heads)
    cl.check()
    alone = _stage(_prepared("sweep", width, dev), c, dev, heads)
    assert torch.equal(got[:n], alone)
    for k in range(1, copies):
        assert torch.equal(got[k * n:(k + 1) * n], got[:n]), k
    assert np.bincount(long.coo[:, 1], minlength=long.num_nodes)[(copies - 1) * n:].max() >= 1200  # (a hub in the last copy)
    record_classes(f"aggregate_transformer/sweep-x{copies}-w{width}-h{heads}-{operands}", got.cpu().numpy(), np.tile(ref, (copies, 1)),
                   np.tile(base, (copies, 1)), long.coo)


# ---------------------------------------------------------------------------------------------------- 4. explicit self loops
def test_explicit_self_loops_are_edges(dev):
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
    assert not torch.equal(outs[0], outs[1])  # a (v, v) edge is an ordinary edge: it takes part in the softmax
    ref, base = _refs(c, with_loops.coo, heads)
    record("aggregate_transformer/looped", outs[0].cpu().numpy(), ref, base)
    ref, base = _refs(c, without.coo, heads)
    record("aggregate_transformer/unlooped", outs[1].cpu().numpy(), ref, base)
    # a GCN workspace's tables have dropped the (v, v) edges: the stage call is refused, nothing launched
    gcn = _workspace(with_loops, conv="gcn")
    _prep(gcn, with_loops, dev)
    with pytest.raises(runtime.GnnbError, match="explicit self loops"):
        _stage(gcn, c, dev, heads)
    gcn.check()


# ---------------------------------------------------------------------------------------------------- 5. whole models
def _model_batch(graphs, in_dim, seed):
    """``graphs`` synthetic qm9-like graphs with seeded features of width ``in_dim``, an empty and a one-node graph among them"""
    mols, rng = synthetic.make_batch("qm9", graphs, seed=seed), np.random.default_rng(seed)
    gs = [(rng.uniform(-1, 1, (mols.graph(g)[0].shape[0], in_dim)).astype(np.float32), mols.graph(g)[1]) for g in range(graphs)]
    return pack_graphs(gs[:graphs // 2] + [EMPTY(in_dim), ONE(in_dim)] + gs[graphs // 2:] + [EMPTY(in_dim)])


def _model(layers, heads, in_dim, hidden, seed=0):
    return make_transformer_model(in_dim=in_dim, hidden=hidden, layers=layers, heads=heads, skip=True, pools=("add", "mean", "max"),
                                  mlp_layers=1, out_act=torch.nn.LogSoftmax, seed=seed)


def _compiled(model, b, promise=0, degree=0, ingest=False):
    cm = runtime.CompiledModel.from_model(model, b.num_graphs, b.num_nodes, b.num_edges)
    if ingest:  # (right after construction: before a batch is prepared on the workspace)
        cm.enable_ingest()
    if promise:
        cm.set_max_graph_nodes(promise)
    if degree:
        cm.set_max_degree(degree)
    return cm


@pytest.mark.parametrize("in_dim,hidden,graphs", [(9, 32, 64), (11, 128, 12)])
@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("layers", [1, 2, 3])
def test_whole_models_against_float64(dev, layers, heads, in_dim, hidden, graphs):
    model = _model(layers, heads, in_dim, hidden, seed=layers)
    b = _model_batch(graphs, in_dim, seed=31 + layers)
    assert b.num_graphs == graphs + 3
    cm = _compiled(model, b, ingest=True)
    assert cm.lib.gnnb_model_transformer_heads(cm._model) == heads
    assert cm.lib.gnnb_model_gat_heads(cm._model) == 0 and cm.lib.gnnb_model_edge_dim(cm._model) == 0
    xd, cood, nptr, eptr = to_dev(b, dev)
    out = cm.forward(xd, cood, nptr, eptr)
    cm.check()
    assert cm.last_path() == "layerwise" and out.shape == (b.num_graphs, 19)
    ref, base = R.forward64(model, b, b.x), R.run(model, b, b.x)
    entry = f"forward/transformer-L{layers}-h{heads}-in{in_dim}-d{hidden}"
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


# ---------------------------------------------------------------------------------------------------- 6. the other forwards
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
    record("forward/transformer-L3-h4-promises", outs[-1].cpu().numpy(), R.forward64(model, b, b.x), R.run(model, b, b.x))


def test_forward_with_the_next_batchs_prep(dev):
    """``forward_prepared_prep_next`` over two alternating workspaces under a promise of 64 nodes: the bits of ``forward`` per
    batch."""
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
    record("forward/transformer-captured", out.cpu().numpy(), R.forward64(model, b, x2), R.run(model, b, x2))
    cm.check()


# ---------------------------------------------------------------------------------------------------- 7. refusals
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
    assert b"no edge weights" in cm.lib.gnnb_last_error()
    with pytest.raises(runtime.GnnbError, match="GINE or PNAE"):
        cm.enable_edge_ingest()
    # the ordered ingest serves the stack kernels' promise: refused, naming the entry that runs the model
    ordered = _compiled(model, b)
    ordered.enable_ordered_ingest()
    ei, batch_dev = _t(np.ascontiguousarray(b.coo.T.astype(np.int64)).reshape(2, -1), dev), _t(batch_vector(b), dev)
    with pytest.raises(runtime.GnnbError, match="TransformerConv.*gnnb_forward_pyg"):
        ordered.forward_pyg_ordered(xd, ei, batch=batch_dev, num_graphs=b.num_graphs)
    # a model does not run on the workspace of one with other heads, nor on a GIN model's of the same description
    other = _compiled(make_transformer_model(in_dim=9, hidden=32, layers=2, heads=2, mlp_layers=1, out_act=torch.nn.LogSoftmax), b)
    assert bytes(cm.desc) == bytes(other.desc)
    other.graph_prep(cood, nptr, eptr, b.num_nodes)
    assert cm.lib.gnnb_forward_prepared(cm._model, other._ws, xd.data_ptr(), good.data_ptr(), None) == -1
    assert b"different model" in cm.lib.gnnb_last_error()
    gin_model = gnnb.GNNModel(9, None, 32, 2, 32, gnnb.GINConv_GNNB, torch.nn.ReLU, True, gnnb.GlobalPooling(["add", "mean", "max"]),
                              gnnb.MLP(96, 19, 64, 1), torch.nn.LogSoftmax).eval()
    gin = runtime.CompiledModel.from_model(gin_model, b.num_graphs, b.num_nodes, b.num_edges)
    assert bytes(gin.desc) == bytes(cm.desc)  # (the same description: only the kind tells them apart)
    gin.graph_prep(cood, nptr, eptr, b.num_nodes)
    assert cm.lib.gnnb_forward_prepared(cm._model, gin._ws, xd.data_ptr(), good.data_ptr(), None) == -1
    assert b"different model" in cm.lib.gnnb_last_error()
    assert cm.lib.gnnb_forward_prepared(gin._model, cm._ws, xd.data_ptr(), good.data_ptr(), None) == -1
    assert b"different model" in cm.lib.gnnb_last_error()
    # the stage entry checks its operands on the host, before any launch
    cm.graph_prep(cood, nptr, eptr, b.num_nodes)
    N = b.num_nodes
    z = lambda *shape: torch.zeros(shape, device=dev)  # noqa: E731
    with pytest.raises(runtime.GnnbError, match="divisible by heads"):
        cm.aggregate_transformer(z(N, 30), z(N, 30), z(N, 30), heads=4)
    with pytest.raises(runtime.GnnbError, match="at most 256"):
        cm.aggregate_transformer(z(N, 264), z(N, 264), z(N, 264), heads=4)
    for heads in (9, 0, True):
        with pytest.raises(runtime.GnnbError, match="heads must be"):
            cm.aggregate_transformer(z(N, 32), z(N, 32), z(N, 32), heads=heads)
    for bad, what in ((dict(k=z(N, 16)), "k "), (dict(v=z(N, 16)), "v "), (dict(q=z(N - 1, 32)), "q "), (dict(root=z(N, 16)), "root"),
                      (dict(skip=z(N, 16)), "skip has shape"), (dict(skip=z(N - 1, 32)), "skip must be"), (dict(out=z(N, 16)), "out"),
                      (dict(act="swish"), "act must be"), (dict(q=z(N, 32).double()), "q "), (dict(k=z(N, 32).cpu()), "k "),
                      (dict(v=z(N, 32).cpu()), "v "), (dict(scale=float("inf")), "scale")):
        args = dict(q=z(N, 32), k=z(N, 32), v=z(N, 32), heads=4)
        args.update(bad)
        with pytest.raises(runtime.GnnbError, match=what):
            cm.aggregate_transformer(args.pop("q"), args.pop("k"), args.pop("v"), **args)
    # ... and the C entry itself: heads that do not divide the width, width > 256, heads > 8, a stride below the width (q, k, v, root)
    x = z(N, 264)
    p = x.data_ptr()
    call = lambda ws, lds, heads, width, root=None: cm.lib.gnnb_aggregate_transformer(  # noqa: E731
        ws, p, lds[0], p, lds[1], p, lds[2], root, lds[3], None, 4, heads, 0.5, p, width, None)
    for lds, heads, width, root in (((32,) * 4, 3, 32, None), ((264,) * 4, 4, 264, None), ((36,) * 4, 9, 36, None), ((16, 32, 32, 32), 4, 32, None),
                                    ((32, 16, 32, 32), 4, 32, None), ((32, 32, 16, 32), 4, 32, None), ((32, 32, 32, 16), 4, 32, p)):
        assert call(cm._ws, lds, heads, width, root) == -1 and b"bad argument" in cm.lib.gnnb_last_error()
    # nothing above left a flag or changed a result
    cm.check()
    assert torch.equal(cm.forward(xd, cood, nptr, eptr), good)
