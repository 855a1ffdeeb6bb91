"""SchNet models on the MI355X (include/gnnb_schnet.h; csrc/k_schnet.hip): the continuous-filter aggregate as a stage entry against its
float64 restatement, whole models through the ``_edges`` forwards, one captured replay, and the refusals.

Acceptance is ``ref64.budget`` with the project's K = 4, F = 2^-22 -- no tolerance of this file's own --, every
element compared.  The reference is float64 numpy (``schnet_util.aggregate_ref``; whole models: the model's own torch definition on a
``.double()`` copy); ``base`` is the same in fp32 on the CPU."""
import numpy as np
import pytest
import torch

import gnnbuilder_amd as gnnb
import ref64 as R
import schnet_util as U
from gnnbuilder_amd import runtime, synthetic
from gnnbuilder_amd.batching import pack_graphs
from helpers import EMPTY, ONE, batch_vector, edge_batch, looped_graph, make_model, star_graph, to_dev

pytestmark = pytest.mark.gpu

CUTOFF = 5.0
# in-degrees of the star graph behind looped_graph(40)'s 139 edges, for tiles of 32 AND 64 slots: a row that ends exactly on a tile
# boundary (139 + 53 = 192), one that straddles the next (192 .. 262 over 256), none, one over at least three tiles (262 .. 462), one edge
STAR = (53, 70, 0, 200, 1, 3, 5)


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


BATCHES, PREPARED = {}, {}


def _batch(kind):
    if kind not in BATCHES:
        small = (np.zeros((3, 4), np.float32), np.array([(0, 1), (2, 1), (1, 1)], np.int32))  # (three edges into node 1, one a self loop)
        BATCHES[kind] = (edge_batch(8, 4, seed=21) if kind == "edge" else pack_graphs([small]) if kind == "small" else
                         pack_graphs([looped_graph(40, 4, 7), star_graph(60, 4, STAR, 8)]))
        if kind == "loop":  # (rows in node order, no edge dropped: a row starts where the in-degrees before it end)
            deg = np.bincount(BATCHES[kind].coo[:, 1], minlength=BATCHES[kind].num_nodes)
            start = np.cumsum(deg) - deg
            for te in (32, 64):
                first, last = start // te, (start + deg - 1) // te
                assert ((deg > 0) & ((start + deg) % te == 0)).any() and ((deg > 0) & (last == first + 1)).any() and (last[deg > 0] - first[deg > 0] >= 2).any()
            assert (deg == 0).any() and (deg == 1).any()
    return BATCHES[kind]


def _prepared(kind, dev, conv="gin"):  # one workspace per batch (a GIN one keeps explicit (v, v) edges), prepared once
    if (kind, conv) not in PREPARED:
        b = _batch(kind)
        cm = runtime.CompiledModel.from_model(make_model(conv, in_dim=8, hidden=8, layers=1, out_dim=8), b.num_graphs, b.num_nodes, b.num_edges)
        _, cood, nptr, eptr = to_dev(b, dev)
        cm.graph_prep(cood, nptr, eptr, b.num_nodes)
        PREPARED[kind, conv] = cm
    return PREPARED[kind, conv]


def _stage(cm, dev, b, ops, place=_t):
    x1, dist, w1, b1, w2, b2 = ops
    out = place(np.zeros_like(x1), dev)
    U.cfconv(cm, place(x1, dev), _t(dist, dev), *(_t(a, dev) for a in (w1, b1, w2, b2)), CUTOFF, out=out)
    return out


# (width, gaussians): every axis once.  67: the scalar form, a width that is no multiple of 16; (128, 50): W2 resident; (144, 50): W2
# streamed at 64 slots per tile; (256, 64): streamed at 32
STAGE = [(4, 1), (12, 3), (16, 50), (67, 5), (128, 50), (256, 64), (144, 50)]


@pytest.mark.parametrize("kind", ["edge", "loop", "small"])  # "small": fewer edges than one tile
@pytest.mark.parametrize("w,g", STAGE)
def test_stage_against_float64(dev, kind, w, g):
    b, cm = _batch(kind), _prepared(kind, dev)
    ops = U.operands(b.num_nodes, b.num_edges, w, g, CUTOFF, seed=w + 7 * g)
    got = _stage(cm, dev, b, ops)
    ref, base = U.aggregate_ref(ops[0], b.coo, *ops[1:], CUTOFF), U.aggregate_ref(ops[0], b.coo, *ops[1:], CUTOFF, np.float32)
    assert got.shape == ref.shape == (b.num_nodes, w)
    R.budget(got.cpu().numpy(), ref, base, what=f"cfconv/{kind}-w{w}-g{g}")
    lone = torch.from_numpy(np.bincount(b.coo[:, 1], minlength=b.num_nodes) == 0).to(dev)
    assert lone.any() and not got[lone].any()  # no in-edge: exactly 0


@pytest.mark.parametrize("w,g", [(12, 3), (128, 50)])
def test_operands_off_the_16_byte_grid_give_the_same_bits(dev, w, g):
    b, cm = _batch("loop"), _prepared("loop", dev)
    ops = U.operands(b.num_nodes, b.num_edges, w, g, CUTOFF, seed=5)
    assert torch.equal(_stage(cm, dev, b, ops, place=_offset), _stage(cm, dev, b, ops))


def test_the_empty_batch(dev):
    b = pack_graphs([EMPTY(4)])
    cm = runtime.CompiledModel.from_model(make_model("gin", in_dim=8, hidden=8, layers=1, out_dim=8), 1, 1, 4)
    _, cood, nptr, eptr = to_dev(b, dev)
    cm.graph_prep(_t(b.coo, dev), nptr, eptr, 0)
    assert _stage(cm, dev, b, U.operands(0, 0, 4, 3, CUTOFF, seed=1)).shape == (0, 4)


def _model_batch(graphs, in_dim, seed):
    """QM9-shaped molecules with an empty graph, a graph with explicit self loops and a one-node graph among them; distances [E, 1]."""
    mols, rng = synthetic.make_batch("qm9", graphs, seed=seed), np.random.default_rng(seed)
    gs = [(rng.uniform(-1, 1, (mols.graph(g)[0].shape[0], in_dim)).astype(np.float32), mols.graph(g)[1]) for g in range(graphs)]
    b = pack_graphs(gs[:graphs // 2] + [EMPTY(in_dim), looped_graph(40, in_dim, seed), ONE(in_dim)] + gs[graphs // 2:])
    return b, rng.uniform(0.3, 1.1 * CUTOFF, (b.num_edges, 1)).astype(np.float32)


# (layers, width, gaussians): first-layer in = 9; skip on, the three pools
MODELS = [(1, 12, 3), (3, 12, 50), (2, 128, 50), (2, 144, 20)]


@pytest.mark.parametrize("layers,width,g", MODELS)
def test_whole_models_against_float64(dev, layers, width, g):
    model = U.make_model(9, width, layers, g, CUTOFF, seed=layers + width)
    b0, d0 = _model_batch(8, 9, seed=40 + layers)
    perm = np.random.default_rng(layers).permutation(b0.num_edges)  # (the edges shuffled as a loader may hold them)
    ei = np.ascontiguousarray(b0.coo[perm].T.astype(np.int64))
    b, dist = gnnb.from_pyg_batch(b0.x, ei, batch=batch_vector(b0), num_graphs=b0.num_graphs, edge_attr=d0[perm])
    assert (b.coo[:, 0] == b.coo[:, 1]).sum() >= 10  # explicit self loops stay
    cm = runtime.CompiledModel.from_model(model, b.num_graphs, b.num_nodes, b.num_edges)
    assert cm.lib.gnnb_model_schnet(cm._model) == g and cm.lib.gnnb_model_edge_dim(cm._model) == 1
    xd, cood, nptr, eptr = to_dev(b, dev)
    cm.enable_edge_ingest()
    out = cm.forward_edges(xd, _t(dist, dev), cood, nptr, eptr).clone()
    cm.check()
    assert cm.last_path() == "layerwise"
    R.budget(out.cpu().numpy(), U.forward64(model, b, b.x, dist), U.run(model, b, b.x, dist), what=f"forward/schnet-L{layers}-w{width}-g{g}")
    pyg = cm.forward_pyg_edges(xd, _t(ei, dev), _t(d0[perm], dev), batch=_t(batch_vector(b), dev), num_graphs=b.num_graphs)
    cm.check()
    assert torch.equal(pyg, out) and cm.last_path() == "layerwise"  # (the ingest's arrays are the host's, the order is the batch's)


def test_a_captured_forward_pyg_edges_replays_with_the_eager_bits(dev):
    model = U.make_model(9, 12, 3, 50, CUTOFF, seed=6)
    b, dist = _model_batch(8, 9, seed=24)
    cm = runtime.CompiledModel.from_model(model, b.num_graphs, b.num_nodes, b.num_edges)
    cm.enable_edge_ingest()
    xd, ei, dd, bd = _t(b.x, dev), _t(np.ascontiguousarray(b.coo.T.astype(np.int64)), dev), _t(dist, dev), _t(batch_vector(b), dev)
    eager = cm.forward_pyg_edges(xd, ei, dd, batch=bd, num_graphs=b.num_graphs).clone()  # (also the warm-up outside the capture)
    out = torch.zeros_like(eager)
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):  # (one stream, no parallel branches)
        cm.forward_pyg_edges(xd, ei, dd, batch=bd, num_graphs=b.num_graphs, out=out)
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_refusals(dev):
    model = U.make_model(9, 12, 2, 5, CUTOFF)
    b, dist = _model_batch(8, 9, seed=25)
    xd, cood, nptr, eptr = to_dev(b, dev)
    cm = runtime.CompiledModel.from_model(model, b.num_graphs, b.num_nodes, b.num_edges)
    with pytest.raises(runtime.GnnbError, match="gnnb_forward_batched_edges"):
        cm.forward(xd, cood, nptr, eptr)
    spec = model.spec()
    for bad, msg in (({"edge_dim": 2}, "edge_dim"), ({"gaussians": 0}, "gaussians"), ({"gaussians": 65}, "gaussians"), ({"cutoff": 0.0}, "cutoff"),
                     ({"cutoff": -1.0}, "cutoff"), ({"hidden_dim": 260, "out_dim": 260}, "at most 256")):
        with pytest.raises(runtime.GnnbError, match=msg):
            runtime.CompiledModel({**spec, **bad}, model.canonical_params(), 4, 64, 256)
    gcn, bl = _prepared("loop", dev, "gcn"), _batch("loop")
    with pytest.raises(runtime.GnnbError, match="explicit self loops"):
        _stage(gcn, dev, bl, U.operands(bl.num_nodes, bl.num_edges, 4, 3, CUTOFF, seed=2))
