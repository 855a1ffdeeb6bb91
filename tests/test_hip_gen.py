"""GENConv models on the MI355X (include/gnnb_gen.h; csrc/k_gen.hip): the softmax aggregate as a stage entry against its float64
restatement, the branches of the state update, whole models through the plain and the ``_edges`` forwards, and the refusals.

Acceptance is ``ref64.budget`` with the project's K = 4, F = 2^-22 -- no tolerance of this file's own --, every
element compared.  The reference is float64 numpy (``gen_util.aggregate_ref``, two passes; whole models: the model's own torch
definition on a ``.double()`` copy); ``base`` is the same in fp32 on the CPU.  Operands in [-1, 1] and |t| <= 8 keep |t m| <= 32."""
import numpy as np
import pytest
import torch

import gen_util as U
import gnnbuilder_amd as gnnb
import ref64 as R
from gnnbuilder_amd import runtime, synthetic
from gnnbuilder_amd.batching import pack_graphs
from helpers import EMPTY, ONE, batch_vector, edge_batch, looped_graph, make_model, star_graph, to_dev

pytestmark = pytest.mark.gpu

STAR = (130, 0, 3, 64, 65, 1)  # in-degrees: three pieces with the last partial, none, a short row, one piece, two pieces, one edge


@pytest.fixture(scope="module")
def dev():
    runtime.load_library(require_gpu=True)  # fails loudly: no fallback
    return torch.device("cuda:0")


def _t(a, dev):
    a = np.ascontiguousarray(a)
    return torch.empty(a.shape, dtype=torch.from_numpy(a).dtype, device=dev) if a.size == 0 else torch.from_numpy(a).to(dev)


def _offset(a, dev):  # ``a`` on the device, contiguous, starting one float past a 16-byte boundary of its buffer
    v = torch.zeros(a.size + 4, dtype=torch.float32, device=dev)[1:1 + a.size].view(a.shape)
    assert v.data_ptr() % 16 == 4
    return v.copy_(torch.from_numpy(a))


def _ordered_star():
    """The star graph's in-degrees with CHOSEN sources (6, 7, ... in that order): a row's messages in slot order are its sources'."""
    coo = np.array([(6 + k, i) for i, deg in enumerate(STAR) for k in range(deg)], np.int32)
    return np.zeros((140, 4), np.float32), coo


BATCHES, PREPARED = {}, {}


def _batch(kind):
    if kind not in BATCHES:
        BATCHES[kind] = (edge_batch(8, 4, seed=21) if kind == "edge" else pack_graphs([_ordered_star()]) if kind == "ordered" else
                         pack_graphs([looped_graph(40, 4, 7), star_graph(60, 4, STAR, 8)]))
    return BATCHES[kind]


def _prepared(kind, dev, conv="gin"):  # one workspace per batch (a GIN one keeps explicit (v, v) edges), prepared once
    if (kind, conv) not in PREPARED:
        b = _batch(kind)
        cm = runtime.CompiledModel.from_model(make_model(conv, in_dim=8, hidden=8, layers=1, out_dim=8), b.num_graphs, b.num_nodes, b.num_edges)
        _, cood, nptr, eptr = to_dev(b, dev)
        cm.graph_prep(cood, nptr, eptr, b.num_nodes)
        PREPARED[kind, conv] = cm
    return PREPARED[kind, conv]


def _operands(b, w, d, seed):
    rng = np.random.default_rng(seed)
    sr = rng.uniform(-1, 1, (b.num_nodes, 2 * w)).astype(np.float32)  # [s | r]
    if not d:
        return sr, None, None, None
    return (sr, rng.uniform(-1, 1, (b.num_edges, d)).astype(np.float32), (rng.uniform(-1, 1, (w, d)) / d).astype(np.float32),
            rng.uniform(-0.5, 0.5, w).astype(np.float32))


def _run(cm, dev, s, r, e, we, be, t, **kw):
    return cm.aggregate_gen(s, r, *(None if a is None else _t(a, dev) for a in (e, we, be)), t=t, **kw)


# (width, d, t, operands): every axis value once, the extremes together.  3, 67: the scalar form; 67: two column passes; 256: the full
# group.  "blocks": s and r are the column blocks of one [N, 2 w] tensor (lds = ldr = 2 w); "own": their own tensors; "bare": r = None
STAGE = [(1, 0, 1.0, "own"), (3, 1, 0.0, "blocks"), (4, 5, -2.0, "blocks"), (12, 16, 8.0, "own"), (67, 0, 8.0, "blocks"), (67, 5, 1.0, "own"),
         (128, 16, 0.0, "blocks"), (128, 0, -2.0, "bare"), (256, 16, 8.0, "blocks"), (256, 1, 1.0, "own"), (12, 0, 1.0, "blocks"),
         (4, 16, -2.0, "bare")]


@pytest.mark.parametrize("kind", ["edge", "loop"])
@pytest.mark.parametrize("w,d,t,how", STAGE)
def test_stage_against_float64(dev, kind, w, d, t, how):
    b, cm = _batch(kind), _prepared(kind, dev)
    sr, e, we, be = _operands(b, w, d, seed=w + 16 * d)
    s, r = sr[:, :w], (None if how == "bare" else sr[:, w:])
    srd = _t(sr, dev)
    sd, rd = (srd[:, :w], srd[:, w:]) if how == "blocks" else (_t(s, dev), None if r is None else _t(r, dev))
    got = _run(cm, dev, sd, rd, e, we, be, t)
    ref, base = U.aggregate_ref(s, b.coo, r, e, we, be, t), U.aggregate_ref(s, b.coo, r, e, we, be, t, np.float32)
    assert got.shape == ref.shape == (b.num_nodes, w)
    R.budget(got.cpu().numpy(), ref, base, what=f"aggregate_gen/{kind}-w{w}-d{d}-t{t:g}-{how}")
    lone = torch.from_numpy(np.bincount(b.coo[:, 1], minlength=b.num_nodes) == 0).to(dev)
    assert lone.any() and torch.equal(got[lone], torch.zeros_like(got[lone]) if rd is None else rd[lone])  # no in-edge: r exactly


@pytest.mark.parametrize("t", [8.0, -2.0])
@pytest.mark.parametrize("pattern", ["rising", "falling", "equal", "killed"])
def test_the_state_updates_branches(dev, pattern, t):
    """A row's messages in slot order: strictly rising (a new max at every step for t > 0, never for t < 0), falling, equal, all eps_m."""
    b, cm = _batch("ordered"), _prepared("ordered", dev)
    j = np.arange(b.num_nodes, dtype=np.float32)[:, None] / b.num_nodes + np.float32(0.125) * np.arange(4, dtype=np.float32)
    s = {"rising": j, "falling": 2 - j, "equal": np.full_like(j, 0.5), "killed": -2 - j}[pattern].astype(np.float32)
    got = _run(cm, dev, _t(s, dev), None, None, None, None, t).cpu().numpy()
    R.budget(got, U.aggregate_ref(s, b.coo, t=t), U.aggregate_ref(s, b.coo, t=t, dtype=np.float32), what=f"{pattern}-t{t:g}")


@pytest.mark.parametrize("d", [0, 4])
def test_operands_off_the_16_byte_grid_take_the_scalar_form(dev, d):
    b, cm = _batch("loop"), _prepared("loop", dev)
    sr, e, we, be = _operands(b, 12, d, seed=5)
    s, r = np.ascontiguousarray(sr[:, :12]), np.ascontiguousarray(sr[:, 12:])
    out = _offset(np.zeros_like(s), dev)
    _run(cm, dev, _offset(s, dev), _offset(r, dev), e, we, be, 1.0, out=out)
    R.budget(out.cpu().numpy(), U.aggregate_ref(s, b.coo, r, e, we, be), U.aggregate_ref(s, b.coo, r, e, we, be, dtype=np.float32), what="offset")
    aligned = _run(cm, dev, _t(s, dev), _t(r, dev), e, we, be, 1.0)
    assert torch.equal(out, aligned)  # (the two forms: the same bits)


def test_the_empty_batch(dev):
    b = pack_graphs([EMPTY(4)])
    cm = runtime.CompiledModel.from_model(make_model("gin", in_dim=8, hidden=8, layers=1, out_dim=8), 1, 1, 4)
    _, cood, nptr, eptr = to_dev(b, dev)
    cm.graph_prep(_t(b.coo, dev), nptr, eptr, 0)
    z = _t(np.zeros((0, 4), np.float32), dev)
    assert cm.aggregate_gen(z, z.clone(), _t(np.zeros((0, 3), np.float32), dev), _t(np.ones((4, 3), np.float32), dev),
                            _t(np.ones(4, np.float32), dev)).shape == (0, 4)


def _model_batch(graphs, in_dim, d, seed):
    mols, rng = synthetic.make_batch("qm9", graphs, seed=seed), np.random.default_rng(seed)
    gs = [(rng.uniform(-1, 1, (mols.graph(g)[0].shape[0], in_dim)).astype(np.float32), mols.graph(g)[1]) for g in range(graphs)]
    b = pack_graphs(gs[:graphs // 2] + [EMPTY(in_dim), looped_graph(40, in_dim, seed), ONE(in_dim)] + gs[graphs // 2:])
    return b, (rng.uniform(-1, 1, (b.num_edges, d)).astype(np.float32) if d else None)


def _loader_batch(layers, d, seed):
    """The batch with its edges shuffled as a loader may hold them -> (batch, edge_attr in COO order, edge_index, edge_attr as given)."""
    b0, ea0 = _model_batch(8, 9, d, seed)
    perm = np.random.default_rng(layers).permutation(b0.num_edges)
    ei = np.ascontiguousarray(b0.coo[perm].T.astype(np.int64))
    if not d:
        return gnnb.from_pyg_batch(b0.x, ei, batch=batch_vector(b0), num_graphs=b0.num_graphs), None, ei, None
    b, ea = gnnb.from_pyg_batch(b0.x, ei, batch=batch_vector(b0), num_graphs=b0.num_graphs, edge_attr=ea0[perm])
    return b, ea, ei, ea0[perm]


# (layers, hidden width, edge_dim, t): first-layer in = 9, so layer 0 takes the [s | r] GEMM and the middle layers take none; skip on
MODELS = [(1, 12, 4, 1.0), (3, 12, 5, -2.0), (3, 128, 4, 1.0), (3, 12, 0, 8.0), (2, 128, 0, 0.0)]


@pytest.mark.parametrize("layers,width,d,t", MODELS)
def test_whole_models_against_float64(dev, layers, width, d, t):
    model = U.make_model(9, width, layers, d, t, seed=layers + width)
    b, ea, ei, ea_in = _loader_batch(layers, d, seed=40 + layers)
    assert (b.coo[:, 0] == b.coo[:, 1]).sum() >= 10  # explicit self loops stay
    cm = runtime.CompiledModel.from_model(model, b.num_graphs, b.num_nodes, b.num_edges)
    assert cm.lib.gnnb_model_gen(cm._model) == 1 and cm.lib.gnnb_model_edge_dim(cm._model) == d
    xd, cood, nptr, eptr = to_dev(b, dev)
    bd, eid = _t(batch_vector(b), dev), _t(ei, dev)
    if d:
        cm.enable_edge_ingest()
        out = cm.forward_edges(xd, _t(ea, dev), cood, nptr, eptr).clone()
    else:
        cm.enable_ingest()
        out = cm.forward(xd, cood, nptr, eptr).clone()
    cm.check()
    assert cm.last_path() == "layerwise"
    R.budget(out.cpu().numpy(), U.forward64(model, b, b.x, ea), U.run(model, b, b.x, ea), what=f"forward/gen-L{layers}-w{width}-d{d}-t{t:g}")
    pyg = (cm.forward_pyg_edges(xd, eid, _t(ea_in, dev), batch=bd, num_graphs=b.num_graphs) if d else
           cm.forward_pyg(xd, eid, batch=bd, num_graphs=b.num_graphs))
    cm.check()
    assert torch.equal(pyg, out) and cm.last_path() == "layerwise"  # (the ingest's arrays are the host's, the order is the batch's)


def test_a_captured_forward_pyg_edges_replays_with_the_eager_bits(dev):
    model = U.make_model(9, 12, 3, 4, 1.0, seed=6)
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


def test_refusals(dev):
    edge, plain = U.make_model(9, 12, 2, 4), U.make_model(9, 12, 2, 0)
    b, ea = _model_batch(8, 9, 4, seed=25)
    xd, cood, nptr, eptr = to_dev(b, dev)
    cm = runtime.CompiledModel.from_model(edge, b.num_graphs, b.num_nodes, b.num_edges)
    with pytest.raises(runtime.GnnbError, match="gnnb_forward_batched_edges"):
        cm.forward(xd, cood, nptr, eptr)
    cm.graph_prep(cood, nptr, eptr, b.num_nodes)
    with pytest.raises(runtime.GnnbError, match="gnnb_forward_prepared_edges"):
        cm.forward_prepared(xd)
    cp = runtime.CompiledModel.from_model(plain, b.num_graphs, b.num_nodes, b.num_edges)
    with pytest.raises(runtime.GnnbError, match="call forward$"):
        cp.forward_edges(xd, _t(ea, dev), cood, nptr, eptr)
    for spec, msg in (({**edge.spec(), "edge_dim": 17}, "edge_dim"), ({**plain.spec(), "hidden_dim": 260, "out_dim": 260}, "at most 256")):
        with pytest.raises(runtime.GnnbError, match=msg):
            runtime.CompiledModel(spec, (edge if spec["edge_dim"] else plain).canonical_params(), 4, 64, 256)
    gcn, bl = _prepared("loop", dev, "gcn"), _batch("loop")
    with pytest.raises(runtime.GnnbError, match="explicit self loops"):
        gcn.aggregate_gen(_t(np.zeros((bl.num_nodes, 4), np.float32), dev))
