"""EdgeConv on the MI355X (include/gnnb_edgeconv.h; csrc/k_edgeconv.hip): the stage entry against its float64 restatement, its bits, whole
models (reference: the torch definition in double, which test_edgeconv_model_torch.py holds to the formula) with a captured replay, the
empty batch, the refusals.  Acceptance: ``ref64.budget``, K = 4, F = 2^-22; ``base``: the reference in fp32."""
import functools

import numpy as np
import pytest
import torch

import edgeconv_util as U
import ref64 as R
from gnnbuilder_amd import runtime
from gnnbuilder_amd.batching import pack_graphs
from helpers import EMPTY, batch_vector, edge_batch, looped_graph, make_model, star_graph, to_dev

pytestmark = pytest.mark.gpu

# in-degrees behind looped_graph(40)'s 139 edges: a row that ends on a tile boundary (192), one over the next, none, a hub (262 .. 462)
STAR = (53, 70, 0, 200, 1, 3, 5)
SPARSE = (0, 0) + (1, 2, 0, 1, 1, 2, 0, 0, 2, 1) * 14 + (0,)  # many short rows; rows without in-edges first, last and in between


@pytest.fixture(scope="module")
def dev():
    runtime.load_library(require_gpu=True)  # fails loudly: no fallback
    return torch.device("cuda:0")


def _t(a, dev):
    a = np.ascontiguousarray(a)
    return torch.empty(a.shape, dtype=torch.from_numpy(a).dtype, device=dev) if a.size == 0 else torch.from_numpy(a).to(dev)


def _prepare(b, dev):  # a GIN workspace (it keeps explicit (v, v) edges) with the batch prepared
    cm = runtime.CompiledModel.from_model(make_model("gin", in_dim=8, hidden=8, layers=1, out_dim=8), b.num_graphs, max(b.num_nodes, 1), max(b.num_edges, 4))
    _, cood, nptr, eptr = to_dev(b, dev)
    cm.graph_prep(_t(b.coo, dev), nptr, eptr, b.num_nodes)
    return cm


@functools.lru_cache(maxsize=None)
def _case(kind, dev):
    """(batch, the edges graph prep keeps, prepared workspace); "gap": dropped edges leave slots no row owns."""
    b = pack_graphs([looped_graph(40, 4, 7), star_graph(60, 4, STAR, 8)] if kind in ("hub", "gap") else
                    [star_graph(200, 4, SPARSE, 9)] if kind == "sparse" else [star_graph(20, 4, (64, 64, 0, 32, 32), 10)])
    keep = np.ones(b.num_edges, bool)
    if kind == "gap":  # (every fifth edge of the first graph points into the second)
        b.coo[:139:5, 1], keep[:139:5] = 45, False
    deg = np.bincount(b.coo[keep, 1], minlength=b.num_nodes)
    start = np.cumsum(deg) - deg  # (rows in node order: without dropped edges a row starts where the in-degrees before it end)
    assert kind != "hub" or (deg.max() > 2 * 64 + 1 and ((start + deg - 1) // 64 - start // 64).max() >= 2)
    assert kind != "sparse" or (deg[0] == 0 and deg[-1] == 0 and (deg[1:-1] == 0).any() and deg.max() == 2)
    assert kind != "boundary" or set((start + deg)[deg > 0] % 32) == {0}
    cm = _prepare(b, dev)
    if kind == "gap":  # (the dropped edges are reported; the tables stand)
        with pytest.raises(runtime.GnnbError):
            cm.check()
    return b, b.coo[keep], cm


def _stage(cm, dev, ops, place=_t):  # ops: ab, w2, b2 (edgeconv_util.operands)
    return U.edgeconv(cm, place(ops[0], dev), _t(ops[1], dev), _t(ops[2], dev), place(np.zeros((len(ops[0]), len(ops[1])), np.float32), dev))


# 4: one partial 16-column slice; 18: off the 4-float grid (scalar gathers); 128: W2 resident; 144: streamed, 64 slots per tile; 256: 32
@pytest.mark.parametrize("kind", ["hub", "sparse", "gap", "boundary"])
@pytest.mark.parametrize("w", [4, 18, 128, 144, 256])
def test_stage_against_float64(dev, kind, w):
    b, kept, cm = _case(kind, dev)
    ops = U.operands(b.num_nodes, w, seed=w)
    ref, base = U.stage_ref(ops[0], kept, *ops[1:]), U.stage_ref(ops[0], kept, *ops[1:], np.float32)
    has = np.bincount(kept[:, 1], minlength=b.num_nodes) > 0
    assert (ref[has] < 0).mean() >= 0.25 and ops[2].all() and not has.all()  # (a max seeded with 0, a bias on an empty row: cannot pass)
    got = _stage(cm, dev, ops)
    R.budget(got.cpu().numpy(), ref, base, what=f"edgeconv/{kind}-w{w}")
    assert not got[_t(~has, dev)].any()  # no in-edge: exactly 0


def test_operands_off_the_16_byte_grid_give_the_same_bits(dev):
    def offset(a, dev):  # one float past a 16-byte boundary
        v = torch.zeros(a.size + 4, dtype=torch.float32, device=dev)[1:1 + a.size].view(a.shape)
        assert v.data_ptr() % 16 == 4
        return v.copy_(torch.from_numpy(a))
    b, _, cm = _case("hub", dev)
    ops = U.operands(b.num_nodes, 128, seed=5)
    assert torch.equal(_stage(cm, dev, ops, place=offset), _stage(cm, dev, ops))


def test_the_hub_gives_the_same_bits_wherever_its_row_is_split(dev):
    x, coo = star_graph(60, 4, STAR, 8)
    ab, w2, b2 = U.operands(60, 128, seed=6)
    outs = []
    for order in (np.arange(60), 59 - np.arange(60)):  # (node v becomes order[v]: the hub's slots are 123 .. 323, then 9 .. 209)
        moved = np.empty_like(ab)
        moved[order] = ab
        outs.append(_stage(_prepare(pack_graphs([(x, order[coo].astype(np.int32))]), dev), dev, (moved, w2, b2))[_t(order, dev)])
    assert torch.equal(outs[0], outs[1]) and outs[0][3].any()


def _model_case(dev, width, layers, seed):
    """A seeded model on ``edge_batch``'s graphs (self loops, an empty and a one-node graph); ``forward_pyg``'s edges shuffled."""
    b, model = edge_batch(8, 7, seed, hub=False), U.make_model(7, width, layers, seed)
    cm = runtime.CompiledModel.from_model(model, b.num_graphs, b.num_nodes, b.num_edges)
    cm.enable_ingest()
    ei = np.ascontiguousarray(b.coo[np.random.default_rng(seed).permutation(b.num_edges)].T.astype(np.int64))
    return model, b, cm, dict(edge_index=_t(ei, dev), batch=_t(batch_vector(b), dev), num_graphs=b.num_graphs)


@pytest.mark.parametrize("layers", [1, 3])  # (3: the skip term on the middle layer)
@pytest.mark.parametrize("width", [32, 128])
def test_whole_models_against_float64_and_a_captured_replay(dev, layers, width):
    model, b, cm, pyg = _model_case(dev, width, layers, seed=40 + layers)
    assert (b.coo[:, 0] == b.coo[:, 1]).sum() >= 10 and cm.lib.gnnb_model_edgeconv(cm._model) == 1  # (explicit self loops stay)
    xd = _t(b.x, dev)
    eager = cm.forward(*to_dev(b, dev)).clone()
    cm.check()
    R.budget(eager.cpu().numpy(), R.run(U.make_model(7, width, layers, 40 + layers).double(), b, b.x), R.run(model, b, b.x), what=f"forward/edgeconv-L{layers}-w{width}")
    assert torch.equal(cm.forward_pyg(xd, **pyg), eager) and cm.last_path() == "layerwise"  # (max is order-free: the same bits)
    out, side, graph = torch.zeros_like(eager), torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):  # (one stream, no parallel branches)
        cm.forward_pyg(xd, **pyg, out=out)
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_the_empty_batch_and_the_refusals(dev):
    assert _stage(_prepare(pack_graphs([EMPTY(4)]), dev), dev, U.operands(0, 4, seed=1)).shape == (0, 4)
    model, b, cm, _ = _model_case(dev, 12, 2, seed=25)
    xd, cood, nptr, eptr = to_dev(b, dev)
    for call in (cm.forward_edges, cm.forward_types):
        with pytest.raises(runtime.GnnbError, match="call forward$"):
            call(xd, torch.zeros((b.num_edges, 1), device=dev), cood, nptr, eptr)
    cm.graph_prep(cood, nptr, eptr, b.num_nodes)
    out = torch.zeros((b.num_graphs, 19), device=dev)
    for entry in ("gnnb_forward_prepared_edges", "gnnb_forward_prepared_types"):  # (the C entries behind the Python refusals)
        rc = getattr(cm.lib, entry)(cm._model, cm._ws, xd.data_ptr(), None, out.data_ptr(), None)
        assert rc == -1 and b"call gnnb_forward_prepared " in cm.lib.gnnb_last_error()
    rc = cm.lib.gnnb_forward_pyg_ordered(cm._model, cm._ws, None, None, None, None, 0, 0, 0, None, None)
    assert rc == -1 and b"call gnnb_forward_pyg " in cm.lib.gnnb_last_error()
    with pytest.raises(runtime.GnnbError, match="fpx_w"):
        runtime.CompiledModel({**model.spec(), "fpx": (16, 8)}, model.canonical_params(), 4, 64, 256)
