"""GINE models on the MI355X (include/gnnb_edge.h; csrc/k_gine.hip): the fused edge aggregate as a stage entry, whole models
through ``forward_edges``, PyG mini-batches with ``edge_attr`` through the device ingest, and the refusals.

The float64 reference of a whole model is its own PyTorch definition on a ``.double()`` copy (``gine_util.forward64``: the layer
walk of ``ref64.run``, so trailing empty graphs are pooled); ``base`` is the same definition in fp32 on the CPU; acceptance is
``ref64.budget`` with the project's K = 4, F = 2^-22 -- no tolerance of this file's own.  The stage entry is held against
``ref64.gine_agg64`` composed with the projection in float64 (``base``: both in float32), and against the reference's golden.
Worst e / e32 per entry go to GNNB_FP64_REPORT=<file> beside the other routes' (DESIGN.md section 4)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import golden_util as G
import ref64 as R
from gine_util import edge_attrs, forward64, make_gine_model, run
from gnnbuilder_amd import runtime, synthetic
from gnnbuilder_amd.batching import from_pyg_batch, pack_graphs
from helpers import EMPTY, ONE, batch_vector, edge_batch, make_model, to_dev

pytestmark = pytest.mark.gpu

CAP = (64, 2048, 8192)  # graphs, nodes, edges: every edge_batch(8, ...) of this file
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


@pytest.fixture(scope="module")
def stage_cm(dev):
    """A workspace for the stage entry: its tables do not depend on the model (GIN: explicit self loops are ordinary edges)."""
    return runtime.CompiledModel.from_model(make_model("gin", in_dim=8, hidden=8, layers=1, out_dim=8), *CAP)


def _prep(cm, batch, dev):
    xd, cood, nptr, eptr = to_dev(batch, dev)
    cm.graph_prep(cood, nptr, eptr, batch.num_nodes)
    return xd


# ---------------------------------------------------------------------------------------------------- 1. the reference's golden
def test_fused_aggregate_and_two_linears_match_reference_golden(stage_cm, dev):
    x, coo = G.graph()
    xd = _prep(stage_cm, pack_graphs([(x, coo)]), dev)
    we, be, w0, b0, w1, b1 = (_t(np.array(t), dev) for t in G.gine_weights())
    z = stage_cm.aggregate_edges_fused(xd, _t(G.edge_features(), dev), we, be, eps=G.conv_kwargs("gine")["eps"])
    y = runtime.linear([(runtime.linear([(z, None)], w0, b0, act="relu"), None)], w1, b1)
    torch.cuda.synchronize()
    assert np.abs(y.cpu().numpy() - G.f32("tb_gine_output", (G.N, G.F))).max() < 2e-6  # (test_gine_conv_matches_reference_golden's bound)


# ---------------------------------------------------------------------------------------------------- 2. the stage kernel
def _stage_refs(x, coo, ea, we, be, eps):
    ref = R.gine_agg64(x, coo, ea.astype(np.float64) @ we.astype(np.float64).T + be.astype(np.float64), eps)
    base = R.gine_agg64(x, coo, (ea @ we.T + be).astype(np.float32), eps, dtype=np.float32)
    return ref, base


def _stage_case(width, edge_dim, seed):
    b = edge_batch(8, width, seed)
    rng = np.random.default_rng(seed + 100)
    return b, edge_attrs(b.num_edges, edge_dim, seed + 200), rng.uniform(-0.5, 0.5, (width, edge_dim)).astype(np.float32), \
        rng.uniform(-0.5, 0.5, width).astype(np.float32)


@pytest.mark.parametrize("eps", [0.0, 0.3])
@pytest.mark.parametrize("width,edge_dim", [(128, 4), (9, 3), (36, 1), (130, 16), (256, 5)])
def test_fused_aggregate_against_float64(stage_cm, dev, width, edge_dim, eps):
    b, ea, we, be = _stage_case(width, edge_dim, seed=width + edge_dim)
    assert np.bincount(b.coo[:, 1]).max() >= 1200  # (the hub: a row split over the workgroup)
    xd = _prep(stage_cm, b, dev)
    got = stage_cm.aggregate_edges_fused(xd, _t(ea, dev), _t(we, dev), _t(be, dev), eps=eps)
    stage_cm.check()
    ref, base = _stage_refs(b.x, b.coo, ea, we, be, eps)
    record(f"aggregate_edges_fused/w{width}-ed{edge_dim}", got.cpu().numpy(), ref, base)


def test_fused_aggregate_scalar_form_on_offset_operands(stage_cm, dev):
    """x and out one float past a 16-byte boundary: width 128 then takes the scalar form, with the same results as the vector form
    (the summation order does not depend on the form)."""
    b, ea, we, be = _stage_case(128, 4, seed=7)
    xd = _prep(stage_cm, b, dev)
    args = (_t(ea, dev), _t(we, dev), _t(be, dev))
    out = _offset(np.zeros_like(b.x), dev)
    got = stage_cm.aggregate_edges_fused(_offset(b.x, dev), *args, eps=0.3, out=out)
    assert got.data_ptr() == out.data_ptr()
    vec = stage_cm.aggregate_edges_fused(xd, *args, eps=0.3)
    # w_edge as a column slice of a wider matrix (its row stride crosses the ABI), edge attributes off their 16-byte boundary
    wide = torch.zeros((128, 7), device=dev)
    wide[:, 2:6] = args[1]
    sliced = stage_cm.aggregate_edges_fused(xd, _offset(ea, dev), wide[:, 2:6], args[2], eps=0.3)
    stage_cm.check()
    ref, base = _stage_refs(b.x, b.coo, ea, we, be, 0.3)
    record("aggregate_edges_fused/w128-ed4-offset", got.cpu().numpy(), ref, base)
    assert torch.equal(got, vec) and torch.equal(sliced, vec)


def test_fused_aggregate_without_edges(stage_cm, dev):
    rng = np.random.default_rng(3)
    b = pack_graphs([ONE(12), EMPTY(12), (rng.uniform(-1, 1, (5, 12)).astype(np.float32), np.zeros((0, 2), np.int32))])
    assert b.num_edges == 0
    xd = _prep(stage_cm, b, dev)
    we, be = _t(rng.uniform(-1, 1, (12, 4)).astype(np.float32), dev), _t(rng.uniform(-1, 1, 12).astype(np.float32), dev)
    got = stage_cm.aggregate_edges_fused(xd, None, we, be, eps=0.3)  # (NULL edge_attr)
    stage_cm.check()
    assert np.array_equal(got.cpu().numpy(), b.x * (np.float32(1) + np.float32(0.3)))


# ---------------------------------------------------------------------------------------------------- 3. whole models
def _forward(model, batch, ea, dev, promise=0):
    cm = runtime.CompiledModel.from_model(model, *CAP)
    if promise:
        cm.set_max_graph_nodes(promise)
    xd, cood, nptr, eptr = to_dev(batch, dev)
    out = cm.forward_edges(xd, _t(ea, dev), cood, nptr, eptr)
    cm.check()
    assert cm.last_path() == "layerwise"
    return cm, out


MODELS = {
    "L3-h128-skip": dict(in_dim=9, edge_dim=3, hidden=128, layers=3, skip=True, pools=("add", "mean", "max")),
    "L1": dict(in_dim=9, edge_dim=3, hidden=32, layers=1, skip=False, pools=("add", "mean", "max")),
    "L2-h64-gelu-softmax": dict(in_dim=9, edge_dim=3, hidden=64, layers=2, act="gelu", out_act=torch.nn.Softmax, pools=("mean",)),
}


@pytest.mark.parametrize("name", list(MODELS))
def test_whole_models_against_float64(dev, name):
    model = make_gine_model(seed=4, **MODELS[name])
    b = edge_batch(8, 9, seed=21)
    ea = edge_attrs(b.num_edges, 3, seed=22)
    cm, out = _forward(model, b, ea, dev)
    record(f"forward_edges/{name}", out.cpu().numpy(), forward64(model, b, b.x, ea), run(model, b, b.x, ea))
    # the same forward again gives the same bits (no atomics, a fixed summation order)
    xd, cood, nptr, eptr = to_dev(b, dev)
    assert torch.equal(cm.forward_edges(xd, _t(ea, dev), cood, nptr, eptr), out)
    cm.graph_prep(cood, nptr, eptr, b.num_nodes)
    assert torch.equal(cm.forward_prepared_edges(xd, _t(ea, dev)), out)


def test_trailing_empty_graphs_are_pooled(dev):
    model = make_gine_model(seed=4, **MODELS["L3-h128-skip"])
    mols = synthetic.make_batch("qm9", 6, seed=31)
    b = pack_graphs([(mols.graph(g)[0][:, :9], mols.graph(g)[1]) for g in range(6)] + [EMPTY(9), EMPTY(9)])
    ea = edge_attrs(b.num_edges, 3, seed=32)
    _, out = _forward(model, b, ea, dev)
    assert out.shape == (8, 19)
    record("forward_edges/trailing-empty", out.cpu().numpy(), forward64(model, b, b.x, ea), run(model, b, b.x, ea))


def test_a_promise_changes_neither_the_path_nor_a_bit(dev):
    model = make_gine_model(seed=4, **MODELS["L3-h128-skip"])
    b = edge_batch(8, 9, seed=23, hub=False)
    assert np.diff(b.node_ptr).max() <= 64
    ea = edge_attrs(b.num_edges, 3, seed=24)
    _, plain = _forward(model, b, ea, dev)
    _, promised = _forward(model, b, ea, dev, promise=64)  # (asserts "layerwise", and check(): the promise holds)
    assert torch.equal(plain, promised)
    record("forward_edges/L3-h128-skip-promise64", promised.cpu().numpy(), forward64(model, b, b.x, ea), run(model, b, b.x, ea))


# ---------------------------------------------------------------------------------------------------- 5. PyG mini-batches
ICAP = (512, 16384, 32768)


@pytest.fixture(scope="module")
def pyg(dev):
    """A 300-graph batch (two radix passes), in 11, edge_dim 4, grouped and with edges + edge_attr rows under one seeded permutation."""
    b = synthetic.make_batch("qm9", 300, seed=41)
    rng = np.random.default_rng(42)
    x = rng.uniform(-1, 1, (b.num_nodes, 11)).astype(np.float32)
    ei = np.ascontiguousarray(b.coo.T.astype(np.int64)).reshape(2, -1)
    ea = edge_attrs(b.num_edges, 4, seed=43)
    perm = rng.permutation(b.num_edges)
    model = make_gine_model(in_dim=11, edge_dim=4, hidden=32, layers=2, seed=5)
    cm = runtime.CompiledModel.from_model(model, *ICAP)
    cm.enable_edge_ingest()
    cm.enable_edge_ingest()  # (a second call is a no-op)
    return dict(b=b, x=x, ei=ei, ea=ea, ei_sh=np.ascontiguousarray(ei[:, perm]), ea_sh=np.ascontiguousarray(ea[perm]), cm=cm,
                batch=batch_vector(b), ptr=b.node_ptr.astype(np.int64))


def _forms(p, form, dev):
    return {"batch": _t(p["batch"], dev), "num_graphs": 300} if form == "batch" else {"ptr": _t(p["ptr"], dev)}


@pytest.mark.parametrize("form", ["batch", "ptr"])
def test_ingest_carries_edge_attributes(pyg, dev, form):
    cm, b = pyg["cm"], pyg["b"]
    host_kw = {"batch": pyg["batch"], "num_graphs": 300} if form == "batch" else {"ptr": pyg["ptr"]}
    gb, ea_ord = from_pyg_batch(pyg["x"], pyg["ei_sh"], edge_attr=pyg["ea_sh"], **host_kw)
    got = cm.ingest_pyg_edges(_t(pyg["ei_sh"], dev), _t(pyg["ea_sh"], dev), num_nodes=b.num_nodes, **_forms(pyg, form, dev))
    cm.check()
    for g, r in zip(got, (gb.coo, gb.node_ptr, gb.edge_ptr, ea_ord)):
        assert g.cpu().numpy().dtype == r.dtype and np.array_equal(g.cpu().numpy(), r)
    # forward_pyg_edges == forward_edges on the host-made arrays, bit for bit
    xd = _t(pyg["x"], dev)
    out = cm.forward_pyg_edges(xd, _t(pyg["ei_sh"], dev), _t(pyg["ea_sh"], dev), **_forms(pyg, form, dev)).clone()
    cm.check()
    assert cm.last_path() == "layerwise"
    host = cm.forward_edges(xd, _t(ea_ord, dev), _t(gb.coo, dev), _t(gb.node_ptr, dev), _t(gb.edge_ptr, dev))
    assert torch.equal(out, host)
    # grouped input comes back as it was
    got = cm.ingest_pyg_edges(_t(pyg["ei"], dev), _t(pyg["ea"], dev), num_nodes=b.num_nodes, **_forms(pyg, form, dev))
    cm.check()
    for g, r in zip(got, (b.coo, b.node_ptr, b.edge_ptr, pyg["ea"])):
        assert np.array_equal(g.cpu().numpy(), r)


def test_one_captured_forward_replays_on_grouped_and_on_shuffled_edges(pyg, dev):
    """The launch sequence depends on the host integers only: a HIP graph captured once serves both kinds of batch
    (the set-up of test_hip_ingest.test_one_captured_ingest_replays_on_grouped_and_on_shuffled_edges)."""
    cm, b = pyg["cm"], pyg["b"]
    xd, batch_dev = _t(pyg["x"], dev), _t(pyg["batch"], dev)
    want = {}
    for kind, ei, ea in (("grouped", pyg["ei"], pyg["ea"]), ("shuffled", pyg["ei_sh"], pyg["ea_sh"])):
        gb, ea_ord = from_pyg_batch(pyg["x"], ei, edge_attr=ea, batch=pyg["batch"], num_graphs=300)
        want[kind] = cm.forward_edges(xd, _t(ea_ord, dev), _t(gb.coo, dev), _t(gb.node_ptr, dev), _t(gb.edge_ptr, dev)).clone()
    assert not torch.equal(want["grouped"], want["shuffled"])  # (another neighbour order: other last bits)
    ei_dev, ea_dev = _t(pyg["ei"], dev), _t(pyg["ea"], dev)
    out = torch.zeros((300, cm.out_dim), device=dev)
    cm.forward_pyg_edges(xd, ei_dev, ea_dev, batch=batch_dev, num_graphs=300, out=out)  # (warm-up)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        cm.forward_pyg_edges(xd, ei_dev, ea_dev, batch=batch_dev, num_graphs=300, out=out)
    for kind in ("shuffled", "grouped", "shuffled"):
        ei_dev.copy_(torch.from_numpy(pyg["ei_sh" if kind == "shuffled" else "ei"]))
        ea_dev.copy_(torch.from_numpy(pyg["ea_sh" if kind == "shuffled" else "ea"]))
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want[kind]), kind
    cm.check()


def test_flagged_batch_is_reported_by_the_next_forward(dev):
    """tests/test_hip_ingest.py's test of this name for ``forward_pyg_edges``: what the ingest kernels of a call flag (an
    endpoint = N, contained by design) is reported by the NEXT call on the workspace -- not by the call's own graph prep --
    and once."""
    b = synthetic.make_batch("qm9", 12, seed=9)
    ei = np.ascontiguousarray(b.coo.T.astype(np.int64)).reshape(2, -1)
    N = b.num_nodes
    bad = ei.copy()
    bad[1, int(b.edge_ptr[4]) + 1] = N
    m = runtime.CompiledModel.from_model(make_gine_model(in_dim=4, edge_dim=4, hidden=16, layers=2, seed=5), 16, 512, 1024)
    m.enable_edge_ingest()
    x, ea, batch_dev = torch.zeros((N, 4), device=dev), _t(edge_attrs(b.num_edges, 4, seed=44), dev), _t(batch_vector(b), dev)
    m.forward_pyg_edges(x, _t(bad, dev), ea, batch=batch_dev, num_graphs=12)  # flagged on the device; no check()
    torch.cuda.synchronize()
    with pytest.raises(runtime.GnnbError, match="earlier batch"):
        m.forward_pyg_edges(x, _t(ei, dev), ea, batch=batch_dev, num_graphs=12)
    m.forward_pyg_edges(x, _t(ei, dev), ea, batch=batch_dev, num_graphs=12)  # reported once
    m.check()


# ---------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals(pyg, dev):
    cm, b = pyg["cm"], pyg["b"]
    xd, ei, ea, batch_dev = _t(pyg["x"], dev), _t(pyg["ei"], dev), _t(pyg["ea"], dev), _t(pyg["batch"], dev)
    cood, nptr, eptr = _t(b.coo, dev), _t(b.node_ptr, dev), _t(b.edge_ptr, dev)
    good = cm.forward_edges(xd, ea, cood, nptr, eptr).clone()
    # the entries without edge attributes refuse a GINE model, and name the entry that takes them
    with pytest.raises(runtime.GnnbError, match="gnnb_forward_batched_edges"):
        cm.forward(xd, cood, nptr, eptr)
    with pytest.raises(runtime.GnnbError, match="gnnb_forward_prepared_edges"):
        cm.forward_prepared(xd)
    with pytest.raises(runtime.GnnbError, match="gnnb_forward_pyg_edges"):
        cm.forward_pyg(xd, ei, batch=batch_dev, num_graphs=300)
    ordered = runtime.CompiledModel.from_model(make_gine_model(in_dim=11, edge_dim=4, hidden=32, layers=2, seed=5), *ICAP)
    ordered.enable_ordered_ingest()
    with pytest.raises(runtime.GnnbError, match="gnnb_forward_pyg_edges"):
        ordered.forward_pyg_ordered(xd, ei, batch=batch_dev, num_graphs=300)
    with pytest.raises(runtime.GnnbError, match="gnnb_forward_prepared_edges"):
        cm.gcn_stack_timed(xd, 1)
    # ... and the _edges entries a model without edge weights, in Python and in C
    gcn = runtime.CompiledModel.from_model(make_model("gcn", in_dim=11, hidden=32), *ICAP)
    assert gcn.edge_dim == 0 and gcn.lib.gnnb_model_edge_dim(gcn._model) == 0 and cm.lib.gnnb_model_edge_dim(cm._model) == 4
    with pytest.raises(runtime.GnnbError, match="GINE"):
        gcn.forward_edges(xd, ea, cood, nptr, eptr)
    with pytest.raises(runtime.GnnbError, match="GINE"):
        gcn.enable_edge_ingest()
    out = torch.zeros((300, gcn.out_dim), device=dev)
    args = [C.c_void_p(t.data_ptr()) for t in (xd, ea, cood, nptr, eptr)]
    assert gcn.lib.gnnb_forward_batched_edges(gcn._model, gcn._ws, *args, 300, b.num_nodes, b.num_edges, C.c_void_p(out.data_ptr()), None) == -1
    assert b"gnnb_edge_model_create" in gcn.lib.gnnb_last_error()
    assert gcn.lib.gnnb_workspace_enable_edge_ingest(gcn._ws) == -1
    # edge_attr of another shape or dtype is refused before any launch
    for bad, what in ((ea[:-1], "edge_attr must be"), (torch.zeros((b.num_edges, 5), device=dev), "edge_attr has shape"),
                      (ea.double(), "float32"), (ea.cpu(), "CUDA"), (None, "edge_attr is required")):
        with pytest.raises(runtime.GnnbError, match=what):
            cm.forward_edges(xd, bad, cood, nptr, eptr)
        with pytest.raises(runtime.GnnbError, match=what):
            cm.forward_pyg_edges(xd, ei, bad, batch=batch_dev, num_graphs=300)
    with pytest.raises(runtime.GnnbError, match="edge_attr must be"):
        cm.forward_prepared_edges(xd, ea[:-1])
    # a batch beyond the workspace's capacity
    small = runtime.CompiledModel.from_model(make_gine_model(in_dim=11, edge_dim=4, hidden=32, layers=2, seed=5), 16, 256, 512)
    with pytest.raises(runtime.GnnbError, match="error -2.*exceeds workspace"):
        small.forward_edges(xd, ea, cood, nptr, eptr)
    small.enable_edge_ingest()
    with pytest.raises(runtime.GnnbError, match="error -2.*exceeds workspace"):
        small.forward_pyg_edges(xd, ei, ea, batch=batch_dev, num_graphs=300)
    # in use: a batch has been prepared on the workspace
    late = runtime.CompiledModel.from_model(make_gine_model(in_dim=11, edge_dim=4, hidden=32, layers=2, seed=5), *ICAP)
    late.forward_edges(xd, ea, cood, nptr, eptr)
    with pytest.raises(runtime.GnnbError, match="in use"):
        late.enable_edge_ingest()
    # nothing above left a flag or changed a result
    cm.check()
    assert torch.equal(cm.forward_edges(xd, ea, cood, nptr, eptr), good)
