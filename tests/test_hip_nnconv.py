"""NNConv models on the MI355X (include/gnnb_nnconv.h; csrc/k_nnconv.hip): the aggregate as a stage entry against ``A``'s float64
definition, whole models through ``forward_edges`` and ``forward_pyg_edges``, and the refusals.

Acceptance is ``ref64.budget`` with the project's K = 4, F = 2^-22 -- no tolerance of this file's own --, every
element compared.  The reference is float64 numpy (``nnconv_util``; whole models: the model's own torch definition on a ``.double()``
copy); ``base`` is the same in fp32 on the CPU."""
import numpy as np
import pytest
import torch

import gnnbuilder_amd as gnnb
import nnconv_util as U
import ref64 as R
from gnnbuilder_amd import runtime, synthetic
from gnnbuilder_amd.batching import pack_graphs
from helpers import EMPTY, ONE, batch_vector, edge_batch, looped_graph, make_model, star_graph, to_dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    runtime.load_library(require_gpu=True)  # fails loudly: no fallback
    return torch.device("cuda:0")


def _t(a, dev):
    a = np.ascontiguousarray(a)
    return torch.empty(a.shape, dtype=torch.from_numpy(a).dtype, device=dev) if a.size == 0 else torch.from_numpy(a).to(dev)


def _offset(shape, dev):
    """A contiguous CUDA tensor of ``shape`` that starts one float past a 16-byte boundary of its buffer."""
    n = int(np.prod(shape))
    v = torch.zeros(n + 4, dtype=torch.float32, device=dev)[1:1 + n].view(shape)
    assert v.data_ptr() % 16 == 4
    return v


BATCHES, PREPARED = {}, {}


def _batch(kind):
    """"edge": molecules, self loops, a hub of in-degree 1200, an empty and a one-node graph; "loop": a looped graph (rows of
    in-degree 0) and a graph whose node 0 has exactly 130 in-edges (three pieces, the last partial) and whose node 1 has none."""
    if kind not in BATCHES:
        BATCHES[kind] = edge_batch(8, 4, seed=21) if kind == "edge" else pack_graphs(
            [looped_graph(40, 4, 7), star_graph(60, 4, (130, 0, 3, 64, 65, 1), 8)])
    return BATCHES[kind]


def _prepared(kind, dev):
    """One GIN workspace per batch (graph prep keeps explicit (v, v) edges there), prepared once."""
    if kind not in PREPARED:
        b = _batch(kind)
        cm = runtime.CompiledModel.from_model(make_model("gin", in_dim=8, hidden=8, layers=1, out_dim=8), b.num_graphs, b.num_nodes, b.num_edges)
        _, cood, nptr, eptr = to_dev(b, dev)
        cm.graph_prep(cood, nptr, eptr, b.num_nodes)
        PREPARED[kind] = cm
    return PREPARED[kind]


def _operands(b, fi, d, hidden, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (b.num_nodes, fi)).astype(np.float32)
    e = rng.uniform(-1, 1, (b.num_edges, d)).astype(np.float32)
    if not hidden:
        return x, e, None, None
    return x, e, (rng.uniform(-1, 1, (hidden, d)) / d).astype(np.float32), rng.uniform(-0.5, 0.5, hidden).astype(np.float32)


# (in, d, K, aggr): every value of each axis at least once, the extremes together; 3 and 67: the scalar form, 67: two column passes,
# 256: the full 64-vector group; d and K off the padded ladder (5) and on it
STAGE = [(1, 1, 0, "add"), (3, 5, 1, "mean"), (4, 16, 16, "add"), (12, 1, 16, "mean"), (67, 5, 0, "add"), (67, 16, 1, "mean"),
         (128, 16, 0, "mean"), (128, 5, 16, "add"), (256, 16, 16, "mean"), (256, 1, 1, "add"), (1, 16, 16, "mean"), (256, 16, 0, "add")]


@pytest.mark.parametrize("kind", ["edge", "loop"])
@pytest.mark.parametrize("fi,d,hidden,aggr", STAGE)
def test_stage_against_float64(dev, kind, fi, d, hidden, aggr):
    b, cm = _batch(kind), _prepared(kind, dev)
    x, e, w1, b1 = _operands(b, fi, d, hidden, seed=fi + 16 * d + hidden)
    got = cm.aggregate_nnconv(_t(x, dev), _t(e, dev), None if w1 is None else _t(w1, dev), None if b1 is None else _t(b1, dev), aggr=aggr)
    ref, base = U.aggregate_ref(x, b.coo, e, w1, b1, aggr), U.aggregate_ref(x, b.coo, e, w1, b1, aggr, np.float32)
    assert got.shape == ref.shape == (b.num_nodes, ((hidden or d) + 1) * fi)
    e_, e32 = R.budget(got.cpu().numpy(), ref, base, what=f"aggregate_nnconv/{kind}-in{fi}-d{d}-K{hidden}-{aggr}")
    print(f"aggregate_nnconv/{kind}-in{fi}-d{d}-K{hidden}-{aggr}: e = {e_:.3e}, e32 = {e32:.3e}")
    deg = np.bincount(b.coo[:, 1], minlength=b.num_nodes)
    assert (deg == 0).any() and not got[torch.from_numpy(deg == 0).to(dev)].any()  # a row without in-edges: written, and 0


@pytest.mark.parametrize("hidden", [0, 16])
def test_operands_off_the_16_byte_grid_take_the_scalar_form(dev, hidden):
    b, cm = _batch("loop"), _prepared("loop", dev)
    x, e, w1, b1 = _operands(b, 12, 4, hidden, seed=5)
    xd = _offset(x.shape, dev)
    xd.copy_(torch.from_numpy(x))
    out = _offset((b.num_nodes, ((hidden or 4) + 1) * 12), dev)
    cm.aggregate_nnconv(xd, _t(e, dev), None if w1 is None else _t(w1, dev), None if b1 is None else _t(b1, dev), out=out)
    R.budget(out.cpu().numpy(), U.aggregate_ref(x, b.coo, e, w1, b1), U.aggregate_ref(x, b.coo, e, w1, b1, dtype=np.float32), what="offset")


def test_the_empty_batch(dev):
    b = pack_graphs([EMPTY(4)])
    cm = runtime.CompiledModel.from_model(make_model("gin", in_dim=8, hidden=8, layers=1, out_dim=8), 1, 1, 4)
    _, cood, nptr, eptr = to_dev(b, dev)
    cm.graph_prep(_t(b.coo, dev), nptr, eptr, 0)
    out = cm.aggregate_nnconv(_t(np.zeros((0, 4), np.float32), dev), _t(np.zeros((0, 3), np.float32), dev))
    assert out.shape == (0, 16)


# ---------------------------------------------------------------------------------------------------- whole models
def _model_batch(graphs, in_dim, d, seed):
    mols, rng = synthetic.make_batch("qm9", graphs, seed=seed), np.random.default_rng(seed)
    gs = [(rng.uniform(-1, 1, (mols.graph(g)[0].shape[0], in_dim)).astype(np.float32), mols.graph(g)[1]) for g in range(graphs)]
    b = pack_graphs(gs[:graphs // 2] + [EMPTY(in_dim), looped_graph(40, in_dim, seed), ONE(in_dim)] + gs[graphs // 2:])
    return b, rng.uniform(-1, 1, (b.num_edges, d)).astype(np.float32)


# (layers, hidden width, edge_dim, K, aggr): both variants, 1 and 3 layers with skip, first-layer in = 9, widths 12 and 128, both aggr
MODELS = [(1, 12, 4, 0, "add"), (3, 12, 5, 5, "mean"), (3, 128, 4, 0, "mean"), (1, 128, 3, 16, "add"), (3, 12, 16, 16, "add")]


@pytest.mark.parametrize("layers,width,d,hidden,aggr", MODELS)
def test_whole_models_against_float64(dev, layers, width, d, hidden, aggr):
    model = U.make_model(9, width, layers, d, hidden, aggr, seed=layers + width)
    b0, ea0 = _model_batch(8, 9, d, seed=40 + layers)
    perm = np.random.default_rng(layers).permutation(b0.num_edges)  # the edges as a loader may hold them: shuffled
    ei_np, ea_in = np.ascontiguousarray(b0.coo[perm].T.astype(np.int64)), ea0[perm]
    b, ea = gnnb.from_pyg_batch(b0.x, ei_np, batch=batch_vector(b0), num_graphs=b0.num_graphs, edge_attr=ea_in)
    assert (b.coo[:, 0] == b.coo[:, 1]).sum() >= 10  # explicit self loops stay
    cm = runtime.CompiledModel.from_model(model, b.num_graphs, b.num_nodes, b.num_edges)
    cm.enable_edge_ingest()
    assert cm.lib.gnnb_model_nnconv_hidden(cm._model) == hidden and cm.lib.gnnb_model_edge_dim(cm._model) == d
    xd, cood, nptr, eptr = to_dev(b, dev)
    out = cm.forward_edges(xd, _t(ea, dev), cood, nptr, eptr).clone()
    cm.check()
    assert cm.last_path() == "layerwise"
    ref, base = U.forward64(model, b, b.x, ea), U.run(model, b, b.x, ea)
    what = f"forward_edges/nnconv-L{layers}-w{width}-d{d}-K{hidden}-{aggr}"
    e_, e32 = R.budget(out.cpu().numpy(), ref, base, what=what)
    print(f"{what}: e = {e_:.3e}, e32 = {e32:.3e}")
    bd = _t(batch_vector(b), dev)
    pyg = cm.forward_pyg_edges(xd, _t(ei_np, dev), _t(ea_in, dev), batch=bd, num_graphs=b.num_graphs)
    cm.check()
    assert torch.equal(pyg, out)  # (the ingest's arrays are the host's, the summation order is the batch's)


def test_a_captured_forward_pyg_edges_replays_with_the_eager_bits(dev):
    model = U.make_model(9, 12, 3, 4, 5, "mean", seed=6)
    b, ea = _model_batch(8, 9, 4, seed=24)
    cm = runtime.CompiledModel.from_model(model, b.num_graphs, b.num_nodes, b.num_edges)
    cm.enable_edge_ingest()
    xd, ei, ead, bd = _t(b.x, dev), _t(np.ascontiguousarray(b.coo.T.astype(np.int64)), dev), _t(ea, dev), _t(batch_vector(b), dev)
    eager = cm.forward_pyg_edges(xd, ei, ead, batch=bd, num_graphs=b.num_graphs).clone()  # (also the warm-up outside the capture)
    out = torch.zeros_like(eager)
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):  # (one stream, no parallel branches)
        cm.forward_pyg_edges(xd, ei, ead, batch=bd, num_graphs=b.num_graphs, out=out)
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    R.budget(out.cpu().numpy(), U.forward64(model, b, b.x, ea), U.run(model, b, b.x, ea), what="forward_pyg_edges/nnconv-captured")


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals(dev):
    model = U.make_model(9, 12, 2, 4, 5)
    b, ea = _model_batch(8, 9, 4, seed=25)
    cm = runtime.CompiledModel.from_model(model, b.num_graphs, b.num_nodes, b.num_edges)
    xd, cood, nptr, eptr = to_dev(b, dev)
    with pytest.raises(runtime.GnnbError, match="gnnb_forward_batched_edges"):
        cm.forward(xd, cood, nptr, eptr)
    cm.graph_prep(cood, nptr, eptr, b.num_nodes)
    with pytest.raises(runtime.GnnbError, match="gnnb_forward_prepared_edges"):
        cm.forward_prepared(xd)
    for kw, msg in (({"edge_dim": 17}, "edge_dim"), ({"edge_hidden": 17}, "hidden 17"), ({"hidden_dim": 260, "out_dim": 260}, "at most 256")):
        spec = {**model.spec(), **kw}
        with pytest.raises(runtime.GnnbError, match=msg):
            runtime.CompiledModel(spec, model.canonical_params(), 4, 64, 256)
