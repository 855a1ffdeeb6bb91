"""ResGatedGraphConv models with edge features on the MI355X (include/gnnb_resgated_edge.h; csrc/k_resgated_edge.hip): the fused
gated aggregate with its two edge terms as a stage entry, the terms apart, its epilogue, saturated gates, its forms and strides,
its bits, explicit self loops as edges with their attributes, whole models through ``forward_edges`` and ``forward_pyg_edges``,
the promises, a captured forward, one workspace across unlike batches, and the refusals.

Acceptance is ``ref64.budget`` with the project's K = 4, F = 2^-22 -- no tolerance of this file's own -- per
in-degree class (``gine_util.budget_by_degree``), nothing left out of a comparison.  The reference is float64
(``resgatede_util.resgatede_ref``; whole models: the model's own torch definition on a ``.double()`` copy); ``base`` is the same in
fp32 on the CPU.  The stage's operands lie on dyadic grids, so every gate argument and every gated value is exact in fp32 --
ASSERTED on the reference alone -- and only the gate and the sums differ between ``got``, ``base`` and ``ref``.  Worst e / e32 per
entry go to GNNB_FP64_REPORT=<file>."""
import json
import os

import numpy as np
import pytest
import torch

import gnnbuilder_amd as gnnb
import ref64 as R
from gine_util import budget_by_degree, edge_attrs, forward64, make_gine_model, run
from gnnbuilder_amd import runtime, synthetic
from gnnbuilder_amd.batching import from_pyg_batch, pack_graphs
from helpers import EMPTY, ONE, batch_vector, edge_batch, looped_graph, make_model, sweep_batch, to_dev
from resgated_util import gates, make_resgated_model
from resgatede_util import SHAPES, assert_exact_terms, edge_case, make_resgatede_model, resgatede_ref

pytestmark = pytest.mark.gpu

WORST = {}
ACT_NAMES = ["relu", "gelu", "sigmoid", "tanh", "none"]  # every gnnb_act


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


def _torch_act(v, act):
    t = torch.from_numpy(np.ascontiguousarray(v, np.float32))
    f = {"none": lambda a: a, "relu": torch.relu, "gelu": torch.nn.functional.gelu, "sigmoid": torch.sigmoid, "tanh": torch.tanh}[act]
    return f(t).numpy()


# ---------------------------------------------------------------------------------------------------- 1. the stage against float64
BATCHES, PREPARED, REFS = {}, {}, {}


def _batch(kind):
    """The batches do not depend on the width (the stage's operands are ``edge_case``'s, not the batch's features)."""
    if kind not in BATCHES:
        BATCHES[kind] = edge_batch(8, 4, seed=21) if kind == "edge" else sweep_batch(24, 4, seed=5)[0]
    return BATCHES[kind]


def _prepared(kind, dev):
    """One prepared workspace per batch, shared by the tests of this file (nothing below changes its tables)."""
    if kind not in PREPARED:
        cm = _workspace(_batch(kind))
        _prep(cm, _batch(kind), dev)
        PREPARED[kind] = cm
    return PREPARED[kind]


def _stage(cm, c, dev, root=True, skip=False, act="none", w_gate=None, w_value=None):
    return cm.aggregate_resgated_edges(_t(c["k"], dev), _t(c["q"], dev), _t(c["v"], dev), _t(c["edge_attr"], dev),
                                       _t(c["w_gate"] if w_gate is None else w_gate, dev),
                                       _t(c["w_value"] if w_value is None else w_value, dev), root=_t(c["root"], dev) if root else None,
                                       skip=_t(c["skip"], dev) if skip else None, act=act)


def _refs(c, coo, root=True, skip=False, act="none", gate_term=True, value_term=True):
    args = (c["k"], c["q"], c["v"], c["root"] if root else None, c["skip"] if skip else None, act, coo, c["edge_attr"],
            c["w_gate"] if gate_term else None, c["w_value"] if value_term else None)
    return resgatede_ref(*args), resgatede_ref(*args, dtype=np.float32)


def _shared_refs(kind, width, d, operands):
    """(case, ref, base) of the plain stage call (root, no skip, no activation): computed once, shared, left unchanged."""
    key = (kind, width, d, operands)
    if key not in REFS:
        c = edge_case(_batch(kind).coo, _batch(kind).num_nodes, width, d, operands)
        REFS[key] = (c,) + _refs(c, _batch(kind).coo)
    return REFS[key]


@pytest.mark.parametrize("operands", ["flat", "steep"])
@pytest.mark.parametrize("kind", ["edge", "sweep"])
@pytest.mark.parametrize("width,d", SHAPES)
def test_stage_against_float64(dev, width, d, kind, operands):
    b = _batch(kind)
    coo = b.coo  # (a GIN workspace's tables: the batch's edges as they are)
    deg = np.bincount(coo[:, 1], minlength=b.num_nodes)
    # the hub: a row split over the workgroup; rows without in-edges
    assert deg.max() >= 1200 and (deg == 0).sum() >= 5
    c, ref, base = _shared_refs(kind, width, d, operands)
    _, s32, _ = assert_exact_terms(c, coo)
    g32 = gates(s32)
    assert not np.isnan(g32).any()
    if operands == "flat":
        assert np.abs(s32).max() <= 8.0 and g32.min() > 0.0 and g32.max() < 1.0  # every fp32 gate strictly inside (0, 1)
    else:
        assert np.abs(s32).max() >= 200.0 and (g32 == 0.0).any() and (g32 == 1.0).any()  # exp overflows: gates of exactly 0 and 1
    cm = _prepared(kind, dev)
    got = _stage(cm, c, dev)
    cm.check()
    got = got.cpu().numpy()
    assert got.shape == (b.num_nodes, width) and np.isfinite(got).all()
    assert np.array_equal(got[deg == 0].view(np.uint32), c["root"][deg == 0].view(np.uint32))  # in-degree 0: root, bit for bit
    record_classes(f"aggregate_resgated_edges/{kind}-w{width}-d{d}-{operands}", got, ref, base, coo)


# ---------------------------------------------------------------------------------------------------- 2. the terms apart
@pytest.mark.parametrize("kind", ["edge", "sweep"])
@pytest.mark.parametrize("width,d", [(32, 4), (9, 3), (130, 16)])
def test_the_gate_term_and_the_value_term_apart(dev, width, d, kind):
    """``w_value = 0``: the reference without the value term; ``w_gate = 0``: without the gate term -- the two operands are
    separate on purpose.  All-zero ``edge_attr``: ``aggregate_resgated``'s result, bit for bit."""
    b = _batch(kind)
    coo = b.coo
    c, full, _ = _shared_refs(kind, width, d, "flat")
    cm = _prepared(kind, dev)
    zero = np.zeros_like(c["w_gate"])
    for name, kw, terms in (("novalue", dict(w_value=zero), dict(value_term=False)), ("nogate", dict(w_gate=zero), dict(gate_term=False))):
        got = _stage(cm, c, dev, **kw).cpu().numpy()
        ref, base = _refs(c, coo, **terms)
        assert np.abs(ref - full).max() > 1e-3 * np.abs(full).max()  # (the removed term matters)
        record_classes(f"aggregate_resgated_edges/{name}-{kind}-w{width}-d{d}", got, ref, base, coo)
    plain = cm.aggregate_resgated(_t(c["k"], dev), _t(c["q"], dev), _t(c["v"], dev), root=_t(c["root"], dev), skip=_t(c["skip"], dev),
                                  act="tanh")
    no_attr = _stage(cm, dict(c, edge_attr=np.zeros_like(c["edge_attr"])), dev, skip=True, act="tanh")
    cm.check()
    assert torch.equal(no_attr, plain)


# ---------------------------------------------------------------------------------------------------- 3. the epilogue
@pytest.mark.parametrize("with_skip", [True, False])
@pytest.mark.parametrize("with_root", [True, False])
@pytest.mark.parametrize("act", ACT_NAMES)
def test_epilogue_root_skip_and_activation(dev, act, with_root, with_skip):
    """Width 32, edge_dim 4: ``root`` / ``skip`` present or absent, every activation.  Rows without in-edges are
    ``act(root + skip)`` evaluated in torch fp32: to the bit for the activations that round nothing (none, relu), and within the
    budget with the other rows for the others."""
    width, d = 32, 4
    b = _batch("edge")
    coo = b.coo
    c = _shared_refs("edge", width, d, "flat")[0]
    ref, base = _refs(c, coo, root=with_root, skip=with_skip, act=act)
    cm = _prepared("edge", dev)
    got = _stage(cm, c, dev, root=with_root, skip=with_skip, act=act)
    cm.check()
    got = got.cpu().numpy()
    record_classes(f"aggregate_resgated_edges/epilogue-{act}" + ("" if with_root else "-noroot") + ("" if with_skip else "-noskip"), got,
                   ref, base, coo)
    lone = np.bincount(coo[:, 1], minlength=b.num_nodes) == 0
    zero = np.zeros_like(c["root"])
    pre = (c["root"] if with_root else zero) + (c["skip"] if with_skip else zero)  # (one fp32 add at most: exact on the grids)
    want = _torch_act(pre, act)[lone]
    if act in ("none", "relu"):
        assert np.array_equal(got[lone].view(np.uint32), want.view(np.uint32))
    if not with_root and not with_skip:  # act(0): 0, or sigmoid's 1/2 -- exact in any evaluation
        assert np.array_equal(got[lone], np.broadcast_to(_torch_act(np.zeros(1, np.float32), act), got[lone].shape))


# ---------------------------------------------------------------------------------------------------- 4. saturation
@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("width,d", [(32, 4), (1, 4), (9, 3)])
def test_saturated_gates_are_clean(dev, width, d, act):
    """``steep``: arguments reach +-260.  The output is finite, and an element all of whose gates are exactly 0 in fp32 is
    ``act(root + skip)`` to the bit: 0 * u adds nothing."""
    b = _batch("edge")
    coo = b.coo
    c = _shared_refs("edge", width, d, "steep")[0]
    dst, s32, _ = assert_exact_terms(c, coo)
    open_gate = np.zeros((b.num_nodes, width), np.int64)
    np.add.at(open_gate, dst, gates(s32) != 0.0)
    deg = np.bincount(coo[:, 1], minlength=b.num_nodes)
    shut = (open_gate == 0) & (deg > 0)[:, None]  # (row, column) with in-edges whose gates are all exactly 0
    assert shut.sum() >= (20 if width > 1 else 5)
    cm = _prepared("edge", dev)
    got = _stage(cm, c, dev, root=True, skip=True, act=act).cpu().numpy()
    cm.check()
    assert np.isfinite(got).all() and not np.isnan(got).any()
    want = _torch_act(c["root"] + c["skip"], act)
    assert np.array_equal(got[shut].view(np.uint32), want[shut].view(np.uint32))
    ref, base = _refs(c, coo, root=True, skip=True, act=act)
    record_classes(f"aggregate_resgated_edges/saturated-w{width}-d{d}-{act}", got, ref, base, coo)


# ---------------------------------------------------------------------------------------------------- 5. forms and strides
@pytest.mark.parametrize("width,d", [(32, 4), (9, 3), (130, 16)])
def test_column_blocks_and_offset_buffers(dev, width, d):
    """``k`` / ``q`` / ``v`` / ``root`` as the four column blocks of one [N, 4 width] tensor and ``w_gate`` / ``w_value`` as the
    two row blocks of one [2 width, d] tensor -- the layer's own operands -- give the bits of the same operands apart.  Row
    operands one float past a 16-byte boundary (the scalar row form at any width) are within the budget; ``edge_attr`` alone
    offset likewise (scalar attribute loads) gives the SAME bits as aligned: its values do not depend on the form."""
    b = _batch("edge")
    coo = b.coo
    c, ref, base = _shared_refs("edge", width, d, "flat")
    cm = _prepared("edge", dev)
    four = _t(np.concatenate([c["k"], c["q"], c["v"], c["root"]], 1), dev)
    gv = _t(np.concatenate([c["w_gate"], c["w_value"]], 0), dev)
    assert four.shape == (b.num_nodes, 4 * width) and gv.shape == (2 * width, d)
    ea = _t(c["edge_attr"], dev)
    blocks = cm.aggregate_resgated_edges(four[:, :width], four[:, width:2 * width], four[:, 2 * width:3 * width], ea, gv[:width], gv[width:],
                                         root=four[:, 3 * width:])
    plain = _stage(cm, c, dev)
    assert torch.equal(blocks, plain)
    moved = cm.aggregate_resgated_edges(_t(c["k"], dev), _t(c["q"], dev), _t(c["v"], dev), _offset(c["edge_attr"], dev),
                                        _offset(c["w_gate"], dev), _offset(c["w_value"], dev), root=_t(c["root"], dev))
    assert torch.equal(moved, plain)
    out = _offset(np.zeros((b.num_nodes, width), np.float32), dev)
    scalar = cm.aggregate_resgated_edges(_offset(c["k"], dev), _offset(c["q"], dev), _offset(c["v"], dev), _offset(c["edge_attr"], dev),
                                         _t(c["w_gate"], dev), _t(c["w_value"], dev), root=_offset(c["root"], dev), out=out)
    cm.check()
    assert scalar.data_ptr() == out.data_ptr()
    record_classes(f"aggregate_resgated_edges/blocks-w{width}-d{d}", blocks.cpu().numpy(), ref, base, coo)
    record_classes(f"aggregate_resgated_edges/offset-w{width}-d{d}", scalar.cpu().numpy(), ref, base, coo)


# ---------------------------------------------------------------------------------------------------- 6. determinism
@pytest.mark.parametrize("width,d", [(32, 4), (9, 3), (130, 16)])
def test_a_repeat_launch_and_another_grid_give_the_same_bits(dev, width, d):
    b = _batch("edge")
    c = _shared_refs("edge", width, d, "flat")[0]
    cm = _prepared("edge", dev)
    first = _stage(cm, c, dev, skip=True, act="tanh")
    assert torch.equal(_stage(cm, c, dev, skip=True, act="tanh"), first)
    big = _workspace(b, slack=3)  # three times the capacities: graph prep cuts other node tiles there
    _prep(big, b, dev)
    assert torch.equal(_stage(big, c, dev, skip=True, act="tanh"), first)
    cm.check(), big.check()


@pytest.mark.parametrize("copies", [2, 5, 7])
@pytest.mark.parametrize("width,d,operands", [(32, 4, "flat"), (130, 16, "steep"), (256, 16, "flat")])
def test_rows_keep_their_bits_behind_copies_of_the_batch(dev, width, d, operands, copies):
    """The sweep batch behind ``copies`` copies of itself, every copy with the first copy's operand rows and attribute rows:
    the last copy's rows, hubs included, are taken at other steps by other workgroups and lane groups -- on another grid --
    and have the bits of the batch launched alone."""
    b = _batch("sweep")
    n = b.num_nodes
    long = pack_graphs([b.graph(g) for g in range(b.num_graphs)] * (copies + 1))
    assert long.num_nodes == (copies + 1) * n and long.num_edges == (copies + 1) * b.num_edges
    assert np.bincount(long.coo[:, 1], minlength=long.num_nodes)[copies * n:].max() >= 1200  # (a hub in the last copy)
    assert np.array_equal(long.coo[copies * b.num_edges:] - copies * n, b.coo)  # (a copy's edges keep their order)
    c, ref, base = _shared_refs("sweep", width, d, operands)
    tiled = {k: np.tile(v, (copies + 1, 1)) if k not in ("w_gate", "w_value") else v for k, v in c.items()}
    cl = _workspace(long)
    _prep(cl, long, dev)
    got = _stage(cl, tiled, dev)
    cl.check()
    alone = _stage(_prepared("sweep", dev), c, dev)
    for k in range(copies + 1):
        assert torch.equal(got[k * n:(k + 1) * n], alone), k
    record_classes(f"aggregate_resgated_edges/sweep-x{copies + 1}-w{width}-d{d}-{operands}", got[copies * n:].cpu().numpy(), ref, base,
                   b.coo)


# ---------------------------------------------------------------------------------------------------- 7. explicit self loops
@pytest.mark.parametrize("d", [3, 4])
def test_explicit_self_loops_are_edges_with_their_attributes(dev, d):
    width = 24
    x, coo = looped_graph(40, width, seed=3)
    assert (coo[:, 0] == coo[:, 1]).sum() >= 10
    others = [ONE(width), (x[:7], np.array([[0, 1], [1, 0], [2, 1], [5, 1]], np.int32))]
    b = pack_graphs([(x, coo)] + others)
    loops = b.coo[:, 0] == b.coo[:, 1]
    c = edge_case(b.coo, b.num_nodes, width, d, "flat")
    moved = dict(c, edge_attr=np.where(loops[:, None], -c["edge_attr"] + np.float32(0.25), c["edge_attr"]).astype(np.float32))
    looped = np.unique(b.coo[loops][:, 1])
    cm = _workspace(b)
    _prep(cm, b, dev)
    first, second = _stage(cm, c, dev), _stage(cm, moved, dev)
    cm.check()
    # changing only the (v, v) rows' attributes changes v's output, and no other row's
    diff = (first != second).any(1).cpu().numpy()
    assert diff[looped].all() and not np.delete(diff, looped).any()
    for name, case, got in (("looped", c, first), ("looped-moved", moved, second)):
        ref, base = _refs(case, b.coo)
        record(f"aggregate_resgated_edges/{name}-d{d}", got.cpu().numpy(), ref, base)
    # a GCN workspace's tables have dropped the (v, v) edges: the stage call is refused, nothing launched
    gcn = _workspace(b, conv="gcn")
    _prep(gcn, b, dev)
    with pytest.raises(runtime.GnnbError, match="explicit self loops"):
        _stage(gcn, c, dev)
    gcn.check()


# ---------------------------------------------------------------------------------------------------- 8. whole models
def _model_batch(graphs, in_dim, seed):
    """``graphs`` synthetic qm9-like graphs with seeded features of width ``in_dim``; a graph with explicit self loops, an empty
    and a one-node graph among them"""
    mols, rng = synthetic.make_batch("qm9", graphs, seed=seed), np.random.default_rng(seed)
    gs = [(rng.uniform(-1, 1, (mols.graph(g)[0].shape[0], in_dim)).astype(np.float32), mols.graph(g)[1]) for g in range(graphs)]
    return pack_graphs(gs[:graphs // 2] + [EMPTY(in_dim), looped_graph(40, in_dim, seed), ONE(in_dim)] + gs[graphs // 2:] + [EMPTY(in_dim)])


def _model(layers, d, in_dim=9, hidden=32, skip=True, act="relu", pools=("add", "mean", "max"), seed=0):
    return make_resgatede_model(in_dim=in_dim, edge_dim=d, hidden=hidden, layers=layers, skip=skip, act=act, pools=pools, mlp_layers=1,
                                out_act=torch.nn.LogSoftmax, seed=seed)


def _compiled(model, b, promise=0, degree=0, ingest=False, caps=None):
    caps = (b.num_graphs, b.num_nodes, b.num_edges) if caps is None else caps
    cm = runtime.CompiledModel.from_model(model, *caps)
    if ingest:  # (right after construction: before a batch is prepared on the workspace)
        cm.enable_edge_ingest()
    if promise:
        cm.set_max_graph_nodes(promise)
    if degree:
        cm.set_max_degree(degree)
    return cm


# test_hip_resgated.py's shapes, each at an edge_dim of {3, 4, 16}
MODELS = [(1, True, "relu", ("add", "mean", "max"), 9, 32, 24, 4), (2, True, "tanh", ("add",), 9, 32, 24, 3),
          (2, False, "relu", ("max",), 11, 128, 12, 16), (3, True, "relu", ("add", "mean", "max"), 9, 32, 24, 16),
          (3, False, "tanh", ("mean",), 11, 128, 12, 4), (3, True, "tanh", ("mean", "max"), 7, 9, 12, 3)]


@pytest.mark.parametrize("layers,skip,act,pools,in_dim,hidden,graphs,d", MODELS)
def test_whole_models_against_float64(dev, layers, skip, act, pools, in_dim, hidden, graphs, d):
    model = _model(layers, d, in_dim, hidden, skip, act, pools, seed=layers)
    b = _model_batch(graphs, in_dim, seed=31 + layers)
    ea = edge_attrs(b.num_edges, d, seed=32 + layers)
    assert b.num_graphs == graphs + 4 and (b.coo[:, 0] == b.coo[:, 1]).sum() >= 10  # explicit self loops: a GCN-style table would drop them
    cm = _compiled(model, b, ingest=True)
    assert cm.lib.gnnb_model_is_resgated(cm._model) == 1 and cm.lib.gnnb_model_edge_dim(cm._model) == d
    assert cm.lib.gnnb_model_gat_heads(cm._model) == 0 and cm.lib.gnnb_model_transformer_heads(cm._model) == 0
    xd, cood, nptr, eptr = to_dev(b, dev)
    ead = _t(ea, dev)
    out = cm.forward_edges(xd, ead, cood, nptr, eptr)
    cm.check()
    assert cm.last_path() == "layerwise" and out.shape == (b.num_graphs, 19)
    ref, base = forward64(model, b, b.x, ea), run(model, b, b.x, ea)
    entry = f"forward_edges/resgatede-L{layers}-{'skip' if skip else 'noskip'}-{act}-in{in_dim}-w{hidden}-d{d}"
    record(entry, out.cpu().numpy(), ref, base)
    # the edge attributes matter: without them the reference is another one
    assert np.abs(forward64(model, b, b.x, np.zeros_like(ea)) - ref).max() > 1e-4 * np.abs(ref).max()
    # the same forward again, and the prepared form, give the same bits (no atomics, a fixed summation order)
    assert torch.equal(cm.forward_edges(xd, ead, cood, nptr, eptr), out)
    assert torch.equal(cm.forward_prepared_edges(xd, ead), out)
    # ... and the PyG mini-batch through the device ingest, its edges and attribute rows shuffled together, with ``batch`` and
    # with ``ptr``: the ingest's arrays are the host's for that input, and so are the bits
    perm = np.random.default_rng(layers).permutation(b.num_edges)
    ei_sh = np.ascontiguousarray(b.coo.T.astype(np.int64)[:, perm])
    ea_sh = np.ascontiguousarray(ea[perm])
    gb, ea_ord = from_pyg_batch(b.x, ei_sh, edge_attr=ea_sh, batch=batch_vector(b), num_graphs=b.num_graphs)
    pyg = cm.forward_pyg_edges(xd, _t(ei_sh, dev), _t(ea_sh, dev), batch=_t(batch_vector(b), dev), num_graphs=b.num_graphs).clone()
    cm.check()
    assert cm.last_path() == "layerwise"
    record(entry + "-pyg", pyg.cpu().numpy(), forward64(model, gb, b.x, ea_ord), run(model, gb, b.x, ea_ord))
    assert torch.equal(cm.forward_pyg_edges(xd, _t(ei_sh, dev), _t(ea_sh, dev), ptr=_t(b.node_ptr.astype(np.int64), dev)), pyg)
    host = cm.forward_edges(xd, _t(ea_ord, dev), _t(gb.coo, dev), _t(gb.node_ptr, dev), _t(gb.edge_ptr, dev))
    assert torch.equal(pyg, host)


# ---------------------------------------------------------------------------------------------------- 9. promises and capture
def test_promises_change_neither_the_path_nor_a_bit(dev):
    model = _model(3, 4, seed=5)
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
    record("forward_edges/resgatede-L3-promises", outs[-1].cpu().numpy(), forward64(model, b, b.x, ea), run(model, b, b.x, ea))


def test_a_captured_forward_replays_with_the_eager_bits(dev):
    model = _model(3, 4, seed=6)
    b = _model_batch(12, 9, seed=24)
    ea = edge_attrs(b.num_edges, 4, seed=25)
    cm = _compiled(model, b)
    xd, cood, nptr, eptr = to_dev(b, dev)
    ead = _t(ea, dev)
    eager = cm.forward_edges(xd, ead, cood, nptr, eptr).clone()  # (also the warm-up outside the capture: kernel attributes, caches)
    out = torch.zeros_like(eager)
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):  # (one stream, no parallel branches)
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
    record("forward_edges/resgatede-captured", out.cpu().numpy(), forward64(model, b, x2, ea2), run(model, b, x2, ea2))
    cm.check()


# ---------------------------------------------------------------------------------------------------- 10. one workspace, unlike batches
def test_one_workspace_across_three_unlike_batches(dev):
    """Three batches of different node, edge and graph counts, one of them without a single edge, in turn -- twice -- on ONE
    workspace: each gives the bits of a fresh workspace of its own size."""
    d = 4
    model = _model(2, d, seed=8)
    lonely = pack_graphs([ONE(9)] * 5 + [EMPTY(9)] + [ONE(9)] * 3)
    batches = [_model_batch(20, 9, seed=41), lonely, _model_batch(6, 9, seed=42)]
    assert lonely.num_edges == 0 and lonely.num_nodes == 8
    assert len({b.num_graphs for b in batches}) == 3 and len({b.num_nodes for b in batches}) == 3 and len({b.num_edges for b in batches}) == 3
    eas = [edge_attrs(b.num_edges, d, seed=43 + i) for i, b in enumerate(batches)]
    want = []
    for b, ea in zip(batches, eas):
        fresh = _compiled(model, b, caps=(b.num_graphs, b.num_nodes, max(b.num_edges, 1)))
        want.append(fresh.forward_edges(*to_dev(b, dev)[:1], _t(ea, dev), *to_dev(b, dev)[1:]).clone())
        fresh.check()
    caps = tuple(max(getattr(b, k) for b in batches) for k in ("num_graphs", "num_nodes", "num_edges"))
    cm = _compiled(model, batches[0], caps=caps)
    for turn in range(2):
        for i, (b, ea) in enumerate(zip(batches, eas)):
            xd, cood, nptr, eptr = to_dev(b, dev)
            got = cm.forward_edges(xd, _t(ea, dev), cood, nptr, eptr)
            cm.check()
            assert got.shape == (b.num_graphs, 19) and torch.equal(got, want[i]), (turn, i)
    record("forward_edges/resgatede-stream", want[0].cpu().numpy(), forward64(model, batches[0], batches[0].x, eas[0]),
           run(model, batches[0], batches[0].x, eas[0]))
    record("forward_edges/resgatede-noedges", want[1].cpu().numpy(), forward64(model, lonely, lonely.x, eas[1]),
           run(model, lonely, lonely.x, eas[1]))


# ---------------------------------------------------------------------------------------------------- 11. refusals
def test_refusals(dev):
    model = _model(2, 4)
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
    # a model does not run on the workspace of one with another edge_dim, nor on a plain ResGatedGraphConv model's, nor on a GINE
    # model's of the same description and edge_dim -- nor those on this model's
    N, E = b.num_nodes, b.num_edges
    plain = runtime.CompiledModel.from_model(make_resgated_model(in_dim=9, hidden=32, layers=2, mlp_layers=1, out_act=torch.nn.LogSoftmax),
                                             b.num_graphs, N, E)
    gine = runtime.CompiledModel.from_model(make_gine_model(in_dim=9, edge_dim=4, hidden=32, layers=2, mlp_layers=1,
                                                            out_act=torch.nn.LogSoftmax), b.num_graphs, N, E)
    assert gine.lib.gnnb_model_is_resgated(gine._model) == 0 and gine.lib.gnnb_model_edge_dim(gine._model) == 4
    assert plain.lib.gnnb_model_is_resgated(plain._model) == 1 and plain.lib.gnnb_model_edge_dim(plain._model) == 0
    for other in (_compiled(_model(2, 3), b), plain, gine):
        assert bytes(cm.desc) == bytes(other.desc)  # (the same description: only what travels beside it tells them apart)
        other.graph_prep(cood, nptr, eptr, N)
        assert cm.lib.gnnb_forward_prepared_edges(cm._model, other._ws, xd.data_ptr(), ea.data_ptr(), good.data_ptr(), None) == -1
        assert b"different model" in cm.lib.gnnb_last_error()
    cm.graph_prep(cood, nptr, eptr, N)
    assert cm.lib.gnnb_forward_prepared_edges(gine._model, cm._ws, xd.data_ptr(), ea.data_ptr(), good.data_ptr(), None) == -1
    assert b"different model" in cm.lib.gnnb_last_error()
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
    with pytest.raises(runtime.GnnbError, match="at most 256"):
        cm.aggregate_resgated_edges(z(N, 264), z(N, 264), z(N, 264), z(E, 4), z(264, 4), z(264, 4))
    for bad, what in ((dict(q=z(N, 16)), "q "), (dict(v=z(N, 16)), "v "), (dict(k=z(N - 1, 32)), "k "), (dict(root=z(N, 16)), "root"),
                      (dict(skip=z(N, 16)), "skip has shape"), (dict(skip=z(N - 1, 32)), "skip must be"), (dict(out=z(N, 16)), "out"),
                      (dict(act="swish"), "act must be"), (dict(k=z(N, 32).double()), "k "), (dict(q=z(N, 32).cpu()), "q "),
                      (dict(w_gate=z(32, 17)), "w_gate must be"), (dict(w_gate=z(16, 4)), "w_gate"), (dict(w_gate=z(32, 4).cpu()), "w_gate"),
                      (dict(w_value=z(32, 3)), "w_value"), (dict(w_value=z(16, 4)), "w_value"), (dict(w_value=z(32, 4).cpu()), "w_value"),
                      (dict(edge_attr=z(E, 3)), "edge_attr has shape"), (dict(edge_attr=z(E - 1, 4)), "edge_attr must be"),
                      (dict(edge_attr=None), "edge_attr is required"), (dict(edge_attr=z(E, 4).double()), "float32")):
        args = dict(k=z(N, 32), q=z(N, 32), v=z(N, 32), edge_attr=z(E, 4), w_gate=z(32, 4), w_value=z(32, 4))
        args.update(bad)
        with pytest.raises(runtime.GnnbError, match=what):
            cm.aggregate_resgated_edges(args.pop("k"), args.pop("q"), args.pop("v"), args.pop("edge_attr"), args.pop("w_gate"),
                                        args.pop("w_value"), **args)
    # ... and the C entry itself: what gnnb_aggregate_resgated refuses (width > 256 or 0, a stride below the width, a NULL operand),
    # edge_dim out of range, ldwg or ldwv < edge_dim, NULL wg, wv, edge_attr (the batch has edges), and a GCN workspace
    x = z(max(N, E), 264)
    p = x.data_ptr()

    def call(ws, lds=(32,) * 4, width=32, k=p, q=p, v=p, root=None, out=p, ea_ptr=p, ed=4, wg=p, ldwg=4, wv=p, ldwv=4):
        return cm.lib.gnnb_aggregate_resgated_edges(ws, k, lds[0], q, lds[1], v, lds[2], root, lds[3], None, 4, ea_ptr, ed, wg, ldwg, wv, ldwv,
                                                    out, width, None)

    assert E > 0
    for kw in (dict(lds=(264,) * 4, width=264), dict(lds=(16, 32, 32, 32)), dict(lds=(32, 16, 32, 32)), dict(lds=(32, 32, 16, 32)),
               dict(lds=(32, 32, 32, 16), root=p), dict(width=0), dict(k=None), dict(q=None), dict(v=None), dict(out=None), dict(ed=0),
               dict(ed=17, ldwg=17, ldwv=17), dict(ldwg=3), dict(ldwv=3), dict(wg=None), dict(wv=None), dict(ea_ptr=None)):
        assert call(cm._ws, **kw) == -1 and b"bad argument to gnnb_aggregate_resgated_edges" in cm.lib.gnnb_last_error(), kw
    gcn = runtime.CompiledModel.from_model(make_model("gcn", in_dim=9, hidden=8, layers=1, out_dim=8), b.num_graphs, N, E)
    gcn.graph_prep(cood, nptr, eptr, N)
    assert call(gcn._ws) == -1 and b"explicit self loops" in cm.lib.gnnb_last_error()
    gcn.check()
    # nothing above left a flag or changed a result
    cm.check()
    assert torch.equal(cm.forward_edges(xd, ea, cood, nptr, eptr), good)
