"""ResGatedGraphConv models on the MI355X (include/gnnb_resgated.h; csrc/k_resgated.hip): the fused gated aggregate as a stage
entry, its epilogue, saturated gates, its forms and strides, its bits, whole models through ``forward``, ``forward_pyg``,
``forward_prepared_prep_next`` and ``forward_host``, the promises, a captured forward, and the refusals.

Acceptance is ``ref64.budget`` with the project's K = 4, F = 2^-22 -- no tolerance of this file's own -- per
in-degree class (``gine_util.budget_by_degree``), nothing left out of a comparison.  The reference is float64
(``resgated_util.resgated_ref``; whole models: the model's own torch definition on a ``.double()`` copy); ``base`` is the same in
fp32 on the CPU.  The stage's operands lie on dyadic grids, so every gate argument ``k_i + q_j`` is exact in fp32 -- ASSERTED on
the reference alone -- and only the gate and the sums differ between ``got``, ``base`` and ``ref``.  Worst e / e32 per entry go to
GNNB_FP64_REPORT=<file>."""
import json
import os

import numpy as np
import pytest
import torch

import gnnbuilder_amd as gnnb
import ref64 as R
from gine_util import budget_by_degree
from gnnbuilder_amd import runtime, synthetic
from gnnbuilder_amd.batching import pack_graphs
from helpers import EMPTY, ONE, batch_vector, edge_batch, looped_graph, make_model, sweep_batch, to_dev
from resgated_util import WIDTHS, gate_arguments, gates, make_resgated_model, resgated_ref, stage_case

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
    """The batches do not depend on the width (the stage's operands are ``stage_case``'s, not the batch's features)."""
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


def _stage(cm, c, dev, root=True, skip=False, act="none"):
    return cm.aggregate_resgated(_t(c["k"], dev), _t(c["q"], dev), _t(c["v"], dev), root=_t(c["root"], dev) if root else None,
                                 skip=_t(c["skip"], dev) if skip else None, act=act)


def _refs(c, coo, root=True, skip=False, act="none"):
    args = (c["k"], c["q"], c["v"], c["root"] if root else None, c["skip"] if skip else None, act, coo)
    return resgated_ref(*args), resgated_ref(*args, dtype=np.float32)


def _shared_refs(kind, width, operands):
    """(case, ref, base) of the plain stage call (root, no skip, no activation): computed once, shared, left unchanged."""
    key = (kind, width, operands)
    if key not in REFS:
        c = stage_case(_batch(kind).num_nodes, width, operands)
        REFS[key] = (c,) + _refs(c, _batch(kind).coo)
    return REFS[key]


def _arguments_are_exact(c, coo):
    _, dst, s64 = gate_arguments(c["k"], c["q"], coo, np.float64)
    _, _, s32 = gate_arguments(c["k"], c["q"], coo, np.float32)
    assert s32.dtype == np.float32 and np.array_equal(s32.astype(np.float64), s64)  # every k_i + q_j is exact in fp32
    return dst, s32


@pytest.mark.parametrize("operands", ["flat", "steep"])
@pytest.mark.parametrize("kind", ["edge", "sweep"])
@pytest.mark.parametrize("width", WIDTHS)
def test_stage_against_float64(dev, width, kind, operands):
    b = _batch(kind)
    coo = b.coo  # (a GIN workspace's tables: the batch's edges as they are)
    deg = np.bincount(coo[:, 1], minlength=b.num_nodes)
    # the hub: a row split over the workgroup; rows without in-edges
    assert deg.max() >= 1200 and (deg == 0).sum() >= 5
    c, ref, base = _shared_refs(kind, width, operands)
    _, s32 = _arguments_are_exact(c, coo)
    g32 = gates(s32)
    assert not np.isnan(g32).any()
    if operands == "flat":
        assert np.abs(s32).max() <= 4.0 and g32.min() > 0.0179 and g32.max() < 0.9821  # sigmoid(-4) = 0.01799, sigmoid(4) = 0.98201
    else:
        assert np.abs(s32).max() >= 200.0 and (g32 == 0.0).any() and (g32 == 1.0).any()  # exp overflows: gates of exactly 0 and 1
    cm = _prepared(kind, dev)
    got = _stage(cm, c, dev)
    cm.check()
    got = got.cpu().numpy()
    assert got.shape == (b.num_nodes, width) and np.isfinite(got).all()
    assert np.array_equal(got[deg == 0].view(np.uint32), c["root"][deg == 0].view(np.uint32))  # in-degree 0: root, bit for bit
    record_classes(f"aggregate_resgated/{kind}-w{width}-{operands}", got, ref, base, coo)


# ---------------------------------------------------------------------------------------------------- 2. the epilogue
@pytest.mark.parametrize("with_skip", [True, False])
@pytest.mark.parametrize("with_root", [True, False])
@pytest.mark.parametrize("act", ACT_NAMES)
def test_epilogue_root_skip_and_activation(dev, act, with_root, with_skip):
    """Width 32: ``root`` / ``skip`` present or absent, every activation.  Rows without in-edges are ``act(root + skip)`` --
    ``act(skip)``, ``act(root)``, ``act(0)`` -- evaluated in torch fp32: to the bit for the activations that round nothing (none,
    relu), and -- the kernel's gelu / sigmoid / tanh are not torch's -- within the budget with the other rows for the others."""
    width = 32
    b = _batch("edge")
    coo = b.coo
    c = stage_case(b.num_nodes, width, "flat")
    ref, base = _refs(c, coo, root=with_root, skip=with_skip, act=act)
    cm = _prepared("edge", dev)
    got = _stage(cm, c, dev, root=with_root, skip=with_skip, act=act)
    cm.check()
    got = got.cpu().numpy()
    record_classes(f"aggregate_resgated/epilogue-{act}" + ("" if with_root else "-noroot") + ("" if with_skip else "-noskip"), got, ref,
                   base, coo)
    lone = np.bincount(coo[:, 1], minlength=b.num_nodes) == 0
    zero = np.zeros_like(c["root"])
    pre = (c["root"] if with_root else zero) + (c["skip"] if with_skip else zero)  # (one fp32 add at most: exact on the grids)
    want = _torch_act(pre, act)[lone]
    if act in ("none", "relu"):
        assert np.array_equal(got[lone].view(np.uint32), want.view(np.uint32))
    if not with_root and not with_skip:  # act(0): 0, or sigmoid's 1/2 -- exact in any evaluation
        assert np.array_equal(got[lone], np.broadcast_to(_torch_act(np.zeros(1, np.float32), act), got[lone].shape))


# ---------------------------------------------------------------------------------------------------- 3. saturation
@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("width", [32, 1, 9])
def test_saturated_gates_are_clean(dev, width, act):
    """``steep``: arguments reach +-256.  The output is finite, and an element all of whose gates are exactly 0 in fp32 is
    ``act(root + skip)`` to the bit: 0 * v adds nothing."""
    b = _batch("edge")
    coo = b.coo
    c = stage_case(b.num_nodes, width, "steep")
    dst, s32 = _arguments_are_exact(c, coo)
    open_gate = np.zeros((b.num_nodes, width), np.int64)
    np.add.at(open_gate, dst, gates(s32) != 0.0)
    deg = np.bincount(coo[:, 1], minlength=b.num_nodes)
    shut = (open_gate == 0) & (deg > 0)[:, None]  # (row, column) with in-edges whose gates are all exactly 0
    assert shut.sum() >= (20 if width > 1 else 5)
    cm = _prepared("edge", dev)
    got = _stage(cm, c, dev, root=True, skip=True, act=act).cpu().numpy()
    cm.check()
    assert np.isfinite(got).all()
    want = _torch_act(c["root"] + c["skip"], act)
    assert np.array_equal(got[shut].view(np.uint32), want[shut].view(np.uint32))
    ref, base = _refs(c, coo, root=True, skip=True, act=act)
    record_classes(f"aggregate_resgated/saturated-w{width}-{act}", got, ref, base, coo)


# ---------------------------------------------------------------------------------------------------- 4. forms and strides
@pytest.mark.parametrize("width", [32, 9, 130])
def test_column_blocks_and_offset_buffers(dev, width):
    """``k`` / ``q`` / ``v`` / ``root`` as the four column blocks of one [N, 4 width] tensor give the bits of the same operands
    contiguous (width 32: the 16-byte form both times; 9, 130: ``width % 4 != 0``, the scalar form), and separate tensors one float
    past a 16-byte boundary (the scalar form at any width) are within the budget."""
    b = _batch("edge")
    coo = b.coo
    c, ref, base = _shared_refs("edge", width, "flat")
    cm = _prepared("edge", dev)
    four = _t(np.concatenate([c["k"], c["q"], c["v"], c["root"]], 1), dev)
    assert four.shape == (b.num_nodes, 4 * width)
    if width % 4 == 0:
        assert all(four[:, i * width:].data_ptr() % 16 == 0 for i in range(4))
    blocks = cm.aggregate_resgated(four[:, :width], four[:, width:2 * width], four[:, 2 * width:3 * width], root=four[:, 3 * width:])
    plain = _stage(cm, c, dev)
    assert torch.equal(blocks, plain)
    out = _offset(np.zeros((b.num_nodes, width), np.float32), dev)
    scalar = cm.aggregate_resgated(_offset(c["k"], dev), _offset(c["q"], dev), _offset(c["v"], dev), root=_offset(c["root"], dev), out=out)
    cm.check()
    assert scalar.data_ptr() == out.data_ptr()
    record_classes(f"aggregate_resgated/blocks-w{width}", blocks.cpu().numpy(), ref, base, coo)
    record_classes(f"aggregate_resgated/offset-w{width}", scalar.cpu().numpy(), ref, base, coo)


# ---------------------------------------------------------------------------------------------------- 5. determinism
@pytest.mark.parametrize("width", [32, 9, 130])
def test_a_repeat_launch_and_another_grid_give_the_same_bits(dev, width):
    b = _batch("edge")
    c = stage_case(b.num_nodes, width, "flat")
    cm = _prepared("edge", dev)
    first = _stage(cm, c, dev, skip=True, act="tanh")
    assert torch.equal(_stage(cm, c, dev, skip=True, act="tanh"), first)
    big = _workspace(b, slack=3)  # three times the capacities: graph prep cuts other node tiles there
    _prep(big, b, dev)
    assert torch.equal(_stage(big, c, dev, skip=True, act="tanh"), first)
    cm.check(), big.check()


@pytest.mark.parametrize("copies", [2, 5, 7])
@pytest.mark.parametrize("width,operands", [(32, "flat"), (130, "steep"), (256, "flat")])
def test_rows_keep_their_bits_behind_copies_of_the_batch(dev, width, operands, copies):
    """The sweep batch behind ``copies`` copies of itself, every copy with the first copy's operand rows: the last copy's rows,
    hubs included, are taken at other steps by other workgroups and lane groups -- on another grid -- and have the bits of the
    batch launched alone.  (A copy's graphs are closed, so its rows see the same neighbours' values.)  Widths 130 (the scalar
    form) and 256 (the 16-byte form) give a row a whole wave, four rows per workgroup and step: from six copies on that is more
    steps (2427) than the grid holds workgroups at ``RG_WG_PER_CU`` = 8 per CU of a 256-CU device, so every workgroup walks
    several steps -- the three-deep pipeline's rotation, the long rows' second walk at a later step."""
    b = _batch("sweep")
    n = b.num_nodes
    long = pack_graphs([b.graph(g) for g in range(b.num_graphs)] * (copies + 1))
    assert long.num_nodes == (copies + 1) * n
    assert np.bincount(long.coo[:, 1], minlength=long.num_nodes)[copies * n:].max() >= 1200  # (a hub in the last copy)
    if width >= 130 and copies >= 5:  # (64 lanes per row: four rows per step of a 256-lane workgroup)
        assert -(-long.num_nodes // 4) > 8 * torch.cuda.get_device_properties(dev).multi_processor_count
    c, ref, base = _shared_refs("sweep", width, operands)
    tiled ={k: np.tile(v, (copies + 1, 1)) for k, v in c.items()}
    cl = _workspace(long)
    _prep(cl, long, dev)
    got = _stage(cl, tiled, dev)
    cl.check()
    alone = _stage(_prepared("sweep", dev), c, dev)
    for k in range(copies + 1):
        assert torch.equal(got[k * n:(k + 1) * n], alone), k
    record_classes(f"aggregate_resgated/sweep-x{copies + 1}-w{width}-{operands}", got[copies * n:].cpu().numpy(), ref, base, b.coo)


# ---------------------------------------------------------------------------------------------------- 6. whole models
def _model_batch(graphs, in_dim, seed):
    """``graphs`` synthetic qm9-like graphs with seeded features of width ``in_dim``; a graph with explicit self loops, an empty
    and a one-node graph among them"""
    mols, rng = synthetic.make_batch("qm9", graphs, seed=seed), np.random.default_rng(seed)
    gs = [(rng.uniform(-1, 1, (mols.graph(g)[0].shape[0], in_dim)).astype(np.float32), mols.graph(g)[1]) for g in range(graphs)]
    return pack_graphs(gs[:graphs // 2] + [EMPTY(in_dim), looped_graph(40, in_dim, seed), ONE(in_dim)] + gs[graphs // 2:] + [EMPTY(in_dim)])


def _model(layers, in_dim=9, hidden=32, skip=True, act="relu", pools=("add", "mean", "max"), seed=0):
    return make_resgated_model(in_dim=in_dim, hidden=hidden, layers=layers, skip=skip, act=act, pools=pools, mlp_layers=1,
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


MODELS = [(1, True, "relu", ("add", "mean", "max"), 9, 32, 24), (2, True, "tanh", ("add",), 9, 32, 24), (2, False, "relu", ("max",), 11, 128, 12),
          (3, True, "relu", ("add", "mean", "max"), 9, 32, 24), (3, False, "tanh", ("mean",), 11, 128, 12), (3, True, "tanh", ("mean", "max"), 7, 9, 12)]


@pytest.mark.parametrize("layers,skip,act,pools,in_dim,hidden,graphs", MODELS)
def test_whole_models_against_float64(dev, layers, skip, act, pools, in_dim, hidden, graphs):
    model = _model(layers, in_dim, hidden, skip, act, pools, seed=layers)
    b = _model_batch(graphs, in_dim, seed=31 + layers)
    assert b.num_graphs == graphs + 4 and (b.coo[:, 0] == b.coo[:, 1]).sum() >= 10  # explicit self loops: a GCN-style table would drop them
    cm = _compiled(model, b, ingest=True)
    assert cm.lib.gnnb_model_is_resgated(cm._model) == 1 and cm.lib.gnnb_model_transformer_heads(cm._model) == 0
    assert cm.lib.gnnb_model_gat_heads(cm._model) == 0 and cm.lib.gnnb_model_edge_dim(cm._model) == 0
    xd, cood, nptr, eptr = to_dev(b, dev)
    out = cm.forward(xd, cood, nptr, eptr)
    cm.check()
    assert cm.last_path() == "layerwise" and out.shape == (b.num_graphs, 19)
    ref, base = R.forward64(model, b, b.x), R.run(model, b, b.x)
    entry = f"forward/resgated-L{layers}-{'skip' if skip else 'noskip'}-{act}-in{in_dim}-d{hidden}"
    record(entry, out.cpu().numpy(), ref, base)
    # without the self loops the reference is another one: the tables kept them
    no_loops = R.forward64(model, b, b.x, coo=b.coo[b.coo[:, 0] != b.coo[:, 1]])
    assert np.abs(no_loops - ref).max() > 1e-4 * np.abs(ref).max()
    # the same forward again, and the prepared form, give the same bits (no atomics, a fixed summation order)
    assert torch.equal(cm.forward(xd, cood, nptr, eptr), out)
    assert torch.equal(cm.forward_prepared(xd), out)
    # ... and so does the PyG mini-batch from a device edge_index + batch, or + ptr (the ingest's arrays are the host's)
    ei = _t(np.ascontiguousarray(b.coo.T.astype(np.int64)).reshape(2, -1), dev)
    pyg = cm.forward_pyg(xd, ei, batch=_t(batch_vector(b), dev), num_graphs=b.num_graphs)
    cm.check()
    assert cm.last_path() == "layerwise"
    record(entry + "-pyg", pyg.cpu().numpy(), ref, base)
    assert torch.equal(pyg, out)
    assert torch.equal(cm.forward_pyg(xd, ei, ptr=_t(b.node_ptr.astype(np.int64), dev)), out)
    # ... and the host-buffer entry
    host = cm.forward_host(b.x, b.coo, b.node_ptr, b.edge_ptr)
    record(entry + "-host", host, ref, base)


def test_promises_change_neither_the_path_nor_a_bit(dev):
    model = _model(3, seed=5)
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
    record("forward/resgated-L3-promises", outs[-1].cpu().numpy(), R.forward64(model, b, b.x), R.run(model, b, b.x))


def test_forward_with_the_next_batchs_prep(dev):
    """``forward_prepared_prep_next`` over two alternating workspaces under a promise of 64 nodes: the bits of ``forward`` per
    batch."""
    model = _model(2, seed=7)
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


# ---------------------------------------------------------------------------------------------------- 7. a captured forward
def test_a_captured_forward_replays_with_the_eager_bits(dev):
    model = _model(3, seed=6)
    b = _model_batch(12, 9, seed=24)
    cm = _compiled(model, b)
    xd, cood, nptr, eptr = to_dev(b, dev)
    eager = cm.forward(xd, cood, nptr, eptr).clone()  # (also the warm-up outside the capture: kernel attributes, caches)
    out = torch.zeros_like(eager)
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):  # (one stream, no parallel branches)
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
    record("forward/resgated-captured", out.cpu().numpy(), R.forward64(model, b, x2), R.run(model, b, x2))
    cm.check()


# ---------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals(dev):
    model = _model(2)
    b = _model_batch(12, 9, seed=25)
    cm = _compiled(model, b)
    xd, cood, nptr, eptr = to_dev(b, dev)
    good = cm.forward(xd, cood, nptr, eptr).clone()
    ea = torch.zeros((b.num_edges, 3), device=dev)
    # no edge attributes: the _edges entries refuse the model as one without edge weights
    with pytest.raises(runtime.GnnbError, match="GINE or PNAE"):
        cm.forward_edges(xd, ea, cood, nptr, eptr)
    with pytest.raises(runtime.GnnbError, match="no edge weights"):
        runtime._check(cm.lib.gnnb_forward_batched_edges(cm._model, cm._ws, xd.data_ptr(), ea.data_ptr(), cood.data_ptr(), nptr.data_ptr(),
                                                         eptr.data_ptr(), b.num_graphs, b.num_nodes, b.num_edges, good.data_ptr(), None))
    # the ordered ingest serves the stack kernels' promise: refused, naming the entry that runs the model
    ordered = _compiled(model, b)
    ordered.enable_ordered_ingest()
    ei, batch_dev = _t(np.ascontiguousarray(b.coo.T.astype(np.int64)).reshape(2, -1), dev), _t(batch_vector(b), dev)
    with pytest.raises(runtime.GnnbError, match="ResGatedGraphConv.*gnnb_forward_pyg"):
        ordered.forward_pyg_ordered(xd, ei, batch=batch_dev, num_graphs=b.num_graphs)
    # a gated model does not run on a GIN model's workspace of the same description, nor a GIN model on a gated workspace
    gin_model = gnnb.GNNModel(9, None, 32, 2, 32, gnnb.GINConv_GNNB, torch.nn.ReLU, True, gnnb.GlobalPooling(["add", "mean", "max"]),
                              gnnb.MLP(96, 19, 64, 1), torch.nn.LogSoftmax).eval()
    gin = runtime.CompiledModel.from_model(gin_model, b.num_graphs, b.num_nodes, b.num_edges)
    assert bytes(gin.desc) == bytes(cm.desc)  # (the same description: only the mark tells them apart)
    assert gin.lib.gnnb_model_is_resgated(gin._model) == 0
    gin.graph_prep(cood, nptr, eptr, b.num_nodes)
    with pytest.raises(runtime.GnnbError, match="different model"):
        runtime._check(cm.lib.gnnb_forward_prepared(cm._model, gin._ws, xd.data_ptr(), good.data_ptr(), None))
    with pytest.raises(runtime.GnnbError, match="different model"):
        runtime._check(cm.lib.gnnb_forward_prepared(gin._model, cm._ws, xd.data_ptr(), good.data_ptr(), None))
    # the stage entry on a GCN workspace: its tables have dropped the (v, v) edges
    N = b.num_nodes
    z = lambda *shape: torch.zeros(shape, device=dev)  # noqa: E731
    gcn = _workspace(b, conv="gcn")
    _prep(gcn, b, dev)
    with pytest.raises(runtime.GnnbError, match="explicit self loops"):
        gcn.aggregate_resgated(z(N, 32), z(N, 32), z(N, 32))
    gcn.check()
    # the stage entry checks its operands on the host, before any launch
    cm.graph_prep(cood, nptr, eptr, b.num_nodes)
    with pytest.raises(runtime.GnnbError, match="at most 256"):
        cm.aggregate_resgated(z(N, 257), z(N, 257), z(N, 257))
    for bad, what in ((dict(q=z(N, 16)), "q "), (dict(v=z(N, 16)), "v "), (dict(k=z(N - 1, 32)), "k "), (dict(root=z(N, 16)), "root"),
                      (dict(skip=z(N, 16)), "skip has shape"), (dict(skip=z(N - 1, 32)), "skip must be"), (dict(out=z(N, 16)), "out"),
                      (dict(act="swish"), "act must be"), (dict(k=z(N, 32).double()), "k "), (dict(q=z(N, 32).cpu()), "q ")):
        args = dict(k=z(N, 32), q=z(N, 32), v=z(N, 32))
        args.update(bad)
        with pytest.raises(runtime.GnnbError, match=what):
            cm.aggregate_resgated(args.pop("k"), args.pop("q"), args.pop("v"), **args)
    # ... and the C entry itself: width 257, a stride below the width (k, q, v, root), a NULL operand (k, q, v, out)
    x = z(N, 260)
    p = x.data_ptr()

    def call(lds, width, k=p, q=p, v=p, root=None, out=p):
        return cm.lib.gnnb_aggregate_resgated(cm._ws, k, lds[0], q, lds[1], v, lds[2], root, lds[3], None, 4, out, width, None)

    for kw in (dict(lds=(260,) * 4, width=257), dict(lds=(16, 32, 32, 32), width=32), dict(lds=(32, 16, 32, 32), width=32),
               dict(lds=(32, 32, 16, 32), width=32), dict(lds=(32, 32, 32, 16), width=32, root=p), dict(lds=(32,) * 4, width=0),
               dict(lds=(32,) * 4, width=32, k=None), dict(lds=(32,) * 4, width=32, q=None), dict(lds=(32,) * 4, width=32, v=None),
               dict(lds=(32,) * 4, width=32, out=None)):
        with pytest.raises(runtime.GnnbError, match="bad argument to gnnb_aggregate_resgated"):
            runtime._check(call(**kw))
    # nothing above left a flag or changed a result
    cm.check()
    assert torch.equal(cm.forward(xd, cood, nptr, eptr), good)
