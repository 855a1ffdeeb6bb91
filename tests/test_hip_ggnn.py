"""GatedGraphConv models on the MI355X (include/gnnb_ggnn.h; csrc/k_ggnn.hip): the fused GRU aggregate as a stage entry, its
forms, strides and absent terms, saturated gates, its bits, whole models through ``forward``, ``forward_pyg``,
``forward_prepared_prep_next`` and ``forward_host``, the promises, a captured forward, and the refusals.

Acceptance is ``ref64.budget`` with the project's K = 4, F = 2^-22 -- no tolerance of this file's own -- per
in-degree class (``gine_util.budget_by_degree``), nothing left out of a comparison.  The reference is float64
(``ggnn_util.ggnn_ref``; whole models: the model's own torch definition on a ``.double()`` copy); ``base`` is the same in fp32 on
the CPU.  The stage's operands lie on dyadic grids, so every sum of ``p_j`` and every r and z argument is exact in fp32 --
ASSERTED on the reference alone -- and only the gates, the tanh and the blend differ between ``got``, ``base`` and ``ref``.
Worst e / e32 per entry go to GNNB_FP64_REPORT=<file>."""
import json
import os

import numpy as np
import pytest
import torch

import gnnbuilder_amd as gnnb
import ref64 as R
from ggnn_util import WIDTHS, arguments_are_exact, ggnn_ref, make_ggnn_model, neighbour_sums, sigmoid, stage_case
from gine_util import budget_by_degree
from gnnbuilder_amd import runtime, synthetic
from gnnbuilder_amd.batching import pack_graphs
from helpers import EMPTY, ONE, batch_vector, edge_batch, looped_graph, make_model, sweep_batch, to_dev

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
    a = np.ascontiguousarray(a)
    if a.size == 0:  # (an empty batch's operands: torch.from_numpy gives an empty array zero strides, not a row stride)
        return torch.empty(a.shape, dtype=torch.from_numpy(a).dtype, device=dev)
    return torch.from_numpy(a).to(dev)


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


def _stage(cm, c, dev, b_ih=True, skip=False, act="none"):
    return cm.aggregate_ggnn(_t(c["p"], dev), _t(c["gh"], dev), _t(c["h"], dev), b_ih=_t(c["b_ih"], dev) if b_ih else None,
                             skip=_t(c["skip"], dev) if skip else None, act=act)


def _refs(c, coo, b_ih=True, skip=False, act="none"):
    args = (c["p"], c["gh"], c["h"], c["b_ih"] if b_ih else None, c["skip"] if skip else None, act, coo)
    return ggnn_ref(*args), ggnn_ref(*args, dtype=np.float32)


def _shared_refs(kind, width, h_width, operands):
    """(case, ref, base) of the plain stage call (b_ih, no skip, no activation): computed once, shared, left unchanged."""
    key = (kind, width, h_width, operands)
    if key not in REFS:
        c = stage_case(_batch(kind).num_nodes, width, h_width, operands)
        REFS[key] = (c,) + _refs(c, _batch(kind).coo)
    return REFS[key]


def _h_widths(width):
    """Equal to the width, a multiple of 4 below it, an odd value below it (the scalar form whatever the width) and 1."""
    return sorted(v for v in {width, 4 * ((width - 1) // 4), (width - 2) | 1, 1} if 1 <= v <= width)


@pytest.mark.parametrize("operands", ["flat", "steep"])
@pytest.mark.parametrize("kind", ["edge", "sweep"])
@pytest.mark.parametrize("width", WIDTHS)
def test_stage_against_float64(dev, width, kind, operands):
    b = _batch(kind)
    coo = b.coo  # (a GIN workspace's tables: the batch's edges as they are)
    deg = np.bincount(coo[:, 1], minlength=b.num_nodes)
    # a hub (a row of more than 128 in-edges, split over the workgroup; the sweep batch also holds rows of 65 .. 128:
    # tests/test_ggnn_ref.py), rows without in-edges
    assert deg.max() >= 1200 and (deg == 0).sum() >= 5
    cm = _prepared(kind, dev)
    for h_width in (_h_widths(width) if kind == "edge" else [width]):
        c, ref, base = _shared_refs(kind, width, h_width, operands)
        r32, z32 = arguments_are_exact(c, coo)
        if operands == "steep":  # the reference's gates reach exactly 0 and 1, its tanh exactly +-1
            g = np.concatenate([sigmoid(r32), sigmoid(z32)])
            assert np.abs(r32).max() >= 200.0 and (g == 0.0).any() and (g == 1.0).any() and not np.isnan(g).any()
        got = _stage(cm, c, dev)
        cm.check()
        got = got.cpu().numpy()
        assert got.shape == (b.num_nodes, width) and np.isfinite(got).all()
        record_classes(f"aggregate_ggnn/{kind}-w{width}-h{h_width}-{operands}", got, ref, base, coo)


# ---------------------------------------------------------------------------------------------------- 2. absent terms, activations
@pytest.mark.parametrize("with_skip", [True, False])
@pytest.mark.parametrize("with_b_ih", [True, False])
@pytest.mark.parametrize("act", ACT_NAMES)
def test_epilogue_bias_skip_and_activation(dev, act, with_b_ih, with_skip):
    """Width 32, ``h_width`` 12: ``b_ih`` / ``skip`` present or absent, every activation."""
    width = 32
    b = _batch("edge")
    c = stage_case(b.num_nodes, width, 12, "flat")
    ref, base = _refs(c, b.coo, b_ih=with_b_ih, skip=with_skip, act=act)
    cm = _prepared("edge", dev)
    got = _stage(cm, c, dev, b_ih=with_b_ih, skip=with_skip, act=act)
    cm.check()
    record_classes(f"aggregate_ggnn/epilogue-{act}" + ("" if with_b_ih else "-nobias") + ("" if with_skip else "-noskip"),
                   got.cpu().numpy(), ref, base, b.coo)


# ---------------------------------------------------------------------------------------------------- 3. saturation
@pytest.mark.parametrize("width", [32, 1, 9])
def test_saturated_gates_are_clean(dev, width):
    """``steep``: arguments reach +-200 and beyond.  Where the reference's z is exactly 1 the output is ``h`` to the bit
    (``fma(1, h - n, n)`` with ``h - n`` and the sum exact on the grid when n is exactly +-1); where z is exactly 0 and the tanh
    is exactly +-1 the output is that +-1 to the bit.  Everything is finite."""
    b = _batch("edge")
    coo = b.coo
    c = stage_case(b.num_nodes, width, width, "steep")
    r32, z32 = arguments_are_exact(c, coo)
    ref, base = _refs(c, coo)
    z, r = sigmoid(z32), sigmoid(r32)
    # far inside the saturated range (fp32 gates are exactly 1 from an argument of 17 on, exactly 0 below -89): the reference's
    # gates are exactly 0 / 1 there, and the tanh argument is exact -- gi_n where r is 0, gi_n + gh_n where r is 1
    r0, r1, z0, z1 = r32 <= -100.0, r32 >= 32.0, z32 <= -100.0, z32 >= 32.0
    assert (r[r0] == 0.0).all() and (r[r1] == 1.0).all() and (z[z0] == 0.0).all() and (z[z1] == 1.0).all()
    gi_n = (neighbour_sums(c["p"], coo, np.float32)[:, 2 * width:] + c["b_ih"][None, 2 * width:]).astype(np.float32)
    arg = np.where(r0, gi_n, gi_n + c["gh"][:, 2 * width:])
    sure = (r0 | r1) & (np.abs(arg) >= 64.0)  # tanh is exactly +-1 in fp32 from |x| of about 9 on
    n = np.sign(arg).astype(np.float32)
    shut, open_ = sure & z0, sure & z1
    assert shut.sum() >= (20 if width > 1 else 3) and open_.sum() >= (20 if width > 1 else 3)
    cm = _prepared("edge", dev)
    got = _stage(cm, c, dev).cpu().numpy()
    cm.check()
    assert np.isfinite(got).all()
    assert np.array_equal(got[shut], n[shut]) and np.array_equal(got[open_], c["h"][open_])
    assert np.array_equal(base[shut], n[shut]) and np.array_equal(base[open_], c["h"][open_])  # (the reference's do too)
    record_classes(f"aggregate_ggnn/saturated-w{width}", got, ref, base, coo)


# ---------------------------------------------------------------------------------------------------- 4. forms and strides
@pytest.mark.parametrize("width,h_width", [(32, 32), (32, 12), (9, 9), (130, 64), (24, 5)])
def test_column_blocks_and_offset_buffers(dev, width, h_width):
    """``p`` / ``gh`` as the two halves of one [N, 6 width] tensor give the bits of the same operands in separate tensors (width 32
    and 24 with ``h_width`` % 4 == 0: the 16-byte form both times; otherwise the scalar form), and separate tensors one float past
    a 16-byte boundary (the scalar form at any width) give those bits too: the summation order is per column, the same in both
    forms."""
    b = _batch("edge")
    coo = b.coo
    c, ref, base = _shared_refs("edge", width, h_width, "flat")
    cm = _prepared("edge", dev)
    six = _t(np.concatenate([c["p"], c["gh"]], 1), dev)
    assert six.shape == (b.num_nodes, 6 * width)
    bi = _t(c["b_ih"], dev)
    blocks = cm.aggregate_ggnn(six[:, :3 * width], six[:, 3 * width:], _t(c["h"], dev), b_ih=bi)
    plain = _stage(cm, c, dev)
    assert torch.equal(blocks, plain)
    # h as the leading columns of a wider state buffer (its stride is passed on)
    wide_h = _t(np.concatenate([c["h"], np.full((b.num_nodes, 7), 3.0, np.float32)], 1), dev)
    assert torch.equal(cm.aggregate_ggnn(six[:, :3 * width], six[:, 3 * width:], wide_h[:, :h_width], b_ih=bi), plain)
    out = _offset(np.zeros((b.num_nodes, width), np.float32), dev)
    scalar = cm.aggregate_ggnn(_offset(c["p"], dev), _offset(c["gh"], dev), _offset(c["h"], dev), b_ih=_offset(c["b_ih"], dev), out=out)
    cm.check()
    assert scalar.data_ptr() == out.data_ptr()
    one_off = cm.aggregate_ggnn(_t(c["p"], dev), _t(c["gh"], dev), _offset(c["h"], dev), b_ih=bi)  # (one operand off the boundary)
    assert torch.equal(scalar, plain) and torch.equal(one_off, plain)
    record_classes(f"aggregate_ggnn/blocks-w{width}-h{h_width}", blocks.cpu().numpy(), ref, base, coo)


# ---------------------------------------------------------------------------------------------------- 5. small batches, determinism
@pytest.mark.parametrize("width", [32, 9])
def test_empty_and_one_node_batches_and_a_larger_workspace(dev, width):
    for name, graphs in (("empty", [EMPTY(8)]), ("one", [ONE(8)]), ("mixed", [EMPTY(8), ONE(8), looped_graph(40, 8, 3), EMPTY(8)])):
        b = pack_graphs(graphs)
        cm = _workspace(b, slack=3)  # (a workspace larger than the batch)
        _prep(cm, b, dev)
        c = stage_case(b.num_nodes, width, width, "flat")
        got = _stage(cm, c, dev, skip=True, act="tanh")
        cm.check()
        assert got.shape == (b.num_nodes, width)
        if b.num_nodes:
            ref, base = _refs(c, b.coo, skip=True, act="tanh")
            record_classes(f"aggregate_ggnn/{name}-w{width}", got.cpu().numpy(), ref, base, b.coo)


@pytest.mark.parametrize("width,h_width", [(32, 32), (9, 4), (130, 130)])
def test_a_repeat_launch_and_another_grid_give_the_same_bits(dev, width, h_width):
    b = _batch("edge")
    c = stage_case(b.num_nodes, width, h_width, "flat")
    cm = _prepared("edge", dev)
    first = _stage(cm, c, dev, skip=True, act="tanh")
    assert torch.equal(_stage(cm, c, dev, skip=True, act="tanh"), first)
    big = _workspace(b, slack=3)  # three times the capacities: graph prep cuts other node tiles there
    _prep(big, b, dev)
    assert torch.equal(_stage(big, c, dev, skip=True, act="tanh"), first)
    cm.check(), big.check()


# ---------------------------------------------------------------------------------------------------- 6. whole models
def _model_batch(graphs, in_dim, seed):
    """``graphs`` synthetic qm9-like graphs with seeded features of width ``in_dim``; a graph with explicit self loops, an empty
    and a one-node graph among them"""
    mols, rng = synthetic.make_batch("qm9", graphs, seed=seed), np.random.default_rng(seed)
    gs = [(rng.uniform(-1, 1, (mols.graph(g)[0].shape[0], in_dim)).astype(np.float32), mols.graph(g)[1]) for g in range(graphs)]
    return pack_graphs(gs[:graphs // 2] + [EMPTY(in_dim), looped_graph(40, in_dim, seed), ONE(in_dim)] + gs[graphs // 2:] + [EMPTY(in_dim)])


def _model(layers, in_dim=9, hidden=32, steps=1, skip=True, act="relu", pools=("add", "mean", "max"), seed=0):
    return make_ggnn_model(in_dim=in_dim, hidden=hidden, layers=layers, steps=steps, skip=skip, act=act, pools=pools, mlp_layers=1,
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


# (layers, steps, skip, act, pools, in_dim, hidden): in 9 / hidden 32 / 3 layers with and without skip; 1 layer, steps 3; in == out
MODELS = [(3, 1, True, "relu", ("add", "mean", "max"), 9, 32), (3, 2, False, "tanh", ("mean",), 9, 32), (1, 3, True, "relu", ("add",), 9, 32),
          (2, 3, True, "tanh", ("mean", "max"), 32, 32), (3, 8, True, "relu", ("max",), 7, 9)]


@pytest.mark.parametrize("layers,steps,skip,act,pools,in_dim,hidden", MODELS)
def test_whole_models_against_float64(dev, layers, steps, skip, act, pools, in_dim, hidden):
    graphs = 24
    model = _model(layers, in_dim, hidden, steps, skip, act, pools, seed=layers + steps)
    b = _model_batch(graphs, in_dim, seed=31 + layers)
    assert b.num_graphs == graphs + 4 and (b.coo[:, 0] == b.coo[:, 1]).sum() >= 10  # explicit self loops: a GCN-style table would drop them
    cm = _compiled(model, b, ingest=True)
    lib = cm.lib
    assert lib.gnnb_model_ggnn_steps(cm._model) == steps and lib.gnnb_model_is_resgated(cm._model) == 0
    assert lib.gnnb_model_transformer_heads(cm._model) == 0 and lib.gnnb_model_gat_heads(cm._model) == 0
    assert lib.gnnb_model_gatconv_heads(cm._model) == 0 and lib.gnnb_model_edge_dim(cm._model) == 0
    xd, cood, nptr, eptr = to_dev(b, dev)
    out = cm.forward(xd, cood, nptr, eptr)
    cm.check()
    assert cm.last_path() == "layerwise" and out.shape == (b.num_graphs, 19)
    ref, base = R.forward64(model, b, b.x), R.run(model, b, b.x)
    entry = f"forward/ggnn-L{layers}-T{steps}-{'skip' if skip else 'noskip'}-{act}-in{in_dim}-d{hidden}"
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
    model = _model(3, steps=2, seed=5)
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
    record("forward/ggnn-L3-T2-promises", outs[-1].cpu().numpy(), R.forward64(model, b, b.x), R.run(model, b, b.x))


def test_forward_with_the_next_batchs_prep(dev):
    """``forward_prepared_prep_next`` over two alternating workspaces under a promise of 64 nodes: the bits of ``forward`` per
    batch."""
    model = _model(2, steps=3, seed=7)
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
    model = _model(3, steps=3, seed=6)
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
    record("forward/ggnn-captured", out.cpu().numpy(), R.forward64(model, b, x2), R.run(model, b, x2))
    cm.check()


# ---------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals(dev):
    model = _model(2, steps=2)
    b = _model_batch(12, 9, seed=25)
    cm = _compiled(model, b)
    xd, cood, nptr, eptr = to_dev(b, dev)
    good = cm.forward(xd, cood, nptr, eptr).clone()
    ea = torch.zeros((b.num_edges, 3), device=dev)
    # no edge attributes: the _edges entries refuse the model as one without edge weights
    with pytest.raises(runtime.GnnbError):
        cm.forward_edges(xd, ea, cood, nptr, eptr)
    with pytest.raises(runtime.GnnbError, match="no edge weights"):
        runtime._check(cm.lib.gnnb_forward_batched_edges(cm._model, cm._ws, xd.data_ptr(), ea.data_ptr(), cood.data_ptr(), nptr.data_ptr(),
                                                         eptr.data_ptr(), b.num_graphs, b.num_nodes, b.num_edges, good.data_ptr(), None))
    # the ordered ingest serves the stack kernels' promise: refused, naming the entry that runs the model
    ordered = _compiled(model, b)
    ordered.enable_ordered_ingest()
    ei, batch_dev = _t(np.ascontiguousarray(b.coo.T.astype(np.int64)).reshape(2, -1), dev), _t(batch_vector(b), dev)
    with pytest.raises(runtime.GnnbError, match="GatedGraphConv.*gnnb_forward_pyg"):
        ordered.forward_pyg_ordered(xd, ei, batch=batch_dev, num_graphs=b.num_graphs)
    # a ggnn model runs neither on a workspace of other steps, nor on a GIN model's of the same description, nor a GIN model on its
    other = _compiled(_model(2, steps=3), b)
    assert bytes(other.desc) == bytes(cm.desc)  # (the same description: only the steps tell them apart)
    other.graph_prep(cood, nptr, eptr, b.num_nodes)
    with pytest.raises(runtime.GnnbError, match="different model"):
        runtime._check(cm.lib.gnnb_forward_prepared(cm._model, other._ws, xd.data_ptr(), good.data_ptr(), None))
    gin_model = gnnb.GNNModel(9, None, 32, 2, 32, gnnb.GINConv_GNNB, torch.nn.ReLU, True, gnnb.GlobalPooling(["add", "mean", "max"]),
                              gnnb.MLP(96, 19, 64, 1), torch.nn.LogSoftmax).eval()
    gin = runtime.CompiledModel.from_model(gin_model, b.num_graphs, b.num_nodes, b.num_edges)
    assert bytes(gin.desc) == bytes(cm.desc) and gin.lib.gnnb_model_ggnn_steps(gin._model) == 0
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
        gcn.aggregate_ggnn(z(N, 96), z(N, 96), z(N, 32))
    gcn.check()
    # the stage entry checks its operands on the host, before any launch
    cm.graph_prep(cood, nptr, eptr, b.num_nodes)
    with pytest.raises(runtime.GnnbError, match="at most 256"):
        cm.aggregate_ggnn(z(N, 3 * 257), z(N, 3 * 257), z(N, 257))
    for bad, what in ((dict(p=z(N, 95)), "3 width"), (dict(gh=z(N, 48)), "gh "), (dict(p=z(N - 1, 96)), "p "), (dict(h=z(N, 33)), "h "),
                      (dict(h=z(N - 1, 32)), "h "), (dict(b_ih=z(95)), "b_ih"), (dict(b_ih=z(1, 96)), "b_ih"),
                      (dict(skip=z(N, 16)), "skip has shape"), (dict(skip=z(N - 1, 32)), "skip must be"), (dict(out=z(N, 16)), "out"),
                      (dict(act="swish"), "act must be"), (dict(p=z(N, 96).double()), "p "), (dict(gh=z(N, 96).cpu()), "gh ")):
        args = dict(p=z(N, 96), gh=z(N, 96), h=z(N, 32))
        args.update(bad)
        with pytest.raises(runtime.GnnbError, match=what):
            cm.aggregate_ggnn(args.pop("p"), args.pop("gh"), args.pop("h"), **args)
    # ... and the C entry itself: width 257 and 0, h_width 0 and above the width, a stride too small (p, gh, h), a NULL operand
    # (p, gh, h, out), an act that is none
    x = z(N, 3 * 260)
    q = x.data_ptr()

    def call(lds=(96, 96, 32), width=32, h_width=32, p=q, gh=q, h=q, out=q, act=4):
        return cm.lib.gnnb_aggregate_ggnn(cm._ws, p, lds[0], gh, lds[1], h, lds[2], h_width, None, None, act, out, width, None)

    for kw in (dict(lds=(780, 780, 260), width=257, h_width=257), dict(width=0, h_width=0), dict(h_width=0), dict(h_width=33),
               dict(lds=(95, 96, 32)), dict(lds=(96, 95, 32)), dict(lds=(96, 96, 31)), dict(p=None), dict(gh=None), dict(h=None),
               dict(out=None), dict(act=5), dict(act=-1)):
        with pytest.raises(runtime.GnnbError, match="bad argument to gnnb_aggregate_ggnn"):
            runtime._check(call(**kw))
    # nothing above left a flag or changed a result
    cm.check()
    assert torch.equal(cm.forward(xd, cood, nptr, eptr), good)
