"""PNA models with edge features on the MI355X (include/gnnb_pna_edge.h; csrc/k_pna_edge.hip): the fused edge aggregate as a stage
entry, whole models through ``forward_edges``, the promises, PyG mini-batches with ``edge_attr`` through the device ingest, and the
refusals.

Acceptance is ``ref64.budget`` with the project's K = 4, F = 2^-22 -- no tolerance of this file's own -- per
in-degree class (``gine_util.budget_by_degree``).  The reference is float64; ``base`` is the same formula (the stage) or the model's
own torch definition (whole models) in fp32 on the CPU.  PyG's std jumps at a variance of 1e-5 (to 0 below it), where float64 and
fp32 could legitimately land on two sides: the stage's operands lie on grids on which every message is exact, and the whole
models' seed is chosen so that no variance of the float64 reference comes near the threshold; both are ASSERTED on the reference
alone, nothing is left out of a comparison.  Worst e / e32 per entry go to GNNB_FP64_REPORT=<file>."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import ref64 as R
from gine_util import budget_by_degree, edge_attrs, forward64, run
from gnnbuilder_amd import runtime, synthetic
from gnnbuilder_amd.batching import from_pyg_batch, pack_graphs
from helpers import EMPTY, ONE, batch_vector, edge_batch, make_model, sweep_batch, to_dev
from pnae_util import layer_variances, make_pnae_model, stage_case, stage_messages, stage_ref

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


def _workspace(batch):
    """A workspace of exactly the batch's size for the stage entry (its tables do not depend on the model)."""
    return runtime.CompiledModel.from_model(make_model("gin", in_dim=8, hidden=8, layers=1, out_dim=8), batch.num_graphs,
                                            max(batch.num_nodes, 1), batch.num_edges)


def _prep(cm, batch, dev):
    _, cood, nptr, eptr = to_dev(batch, dev)
    cm.graph_prep(cood, nptr, eptr, batch.num_nodes)


# ---------------------------------------------------------------------------------------------------- 1. the stage against float64
BATCHES = {}


def _batch(kind, w):
    if (kind, w) not in BATCHES:
        BATCHES[kind, w] = edge_batch(8, w, seed=21) if kind == "edge" else sweep_batch(24, w, seed=5)[0]
    return BATCHES[kind, w]


VAR_WINDOW = (2.5e-6, 4e-5)  # around PyG's std threshold 1e-5: no variance of the float64 reference may lie here


@pytest.mark.parametrize("with_q", [True, False])
@pytest.mark.parametrize("kind", ["edge", "sweep"])
@pytest.mark.parametrize("width,edge_dim", [(32, 4), (9, 3), (130, 16), (256, 5)])
def test_stage_against_float64(dev, width, edge_dim, kind, with_q):
    b = _batch(kind, width)
    deg = np.bincount(b.coo[:, 1], minlength=b.num_nodes)
    assert deg.max() >= 1200 and (deg == 0).any()  # (the hub: a row split over the workgroup; rows without in-edges)
    c = stage_case(b, width, edge_dim)
    q = c["q"] if with_q else None
    h64, h32 = stage_messages(b.coo, c, q, np.float64), stage_messages(b.coo, c, q, np.float32)
    assert np.array_equal(h32.astype(np.float64), h64)  # every message is exact in fp32
    ref, var, _ = stage_ref(b.coo, b.num_nodes, h64)
    base, _, _ = stage_ref(b.coo, b.num_nodes, h32)
    assert not ((var >= VAR_WINDOW[0]) & (var <= VAR_WINDOW[1])).any()  # (on the reference alone; nothing is left out below)
    assert (var[deg > 0] == 0).sum() >= 100  # ... and many are exactly 0, where the clamp decides
    cm = _workspace(b)
    _prep(cm, b, dev)
    got = cm.aggregate_pna_edges(_t(c["p"], dev), None if q is None else _t(q, dev), _t(c["ea"], dev), _t(c["we"], dev), _t(c["be"], dev))
    cm.check()
    got = got.cpu().numpy()
    assert got.shape == (b.num_nodes, 4 * width)
    assert np.array_equal(got[:, :2 * width], ref[:, :2 * width].astype(np.float32))  # max | min: equal
    assert not got[deg == 0].any()  # in-degree 0: four zeros
    entry = f"aggregate_pna_edges/{kind}-w{width}-ed{edge_dim}" + ("" if with_q else "-noq")
    record_classes(entry + "/mean", got[:, 2 * width:3 * width], ref[:, 2 * width:3 * width], base[:, 2 * width:3 * width], b.coo)
    record_classes(entry + "/std", got[:, 3 * width:], ref[:, 3 * width:], base[:, 3 * width:], b.coo)


# ---------------------------------------------------------------------------------------------------- 2. bits
def test_stage_bits(dev):
    """A repeat launch is identical; operands one float past a 16-byte boundary take the scalar form at width 32 and give the bits
    of the vector form (the summation order does not depend on the form); w_edge as a column slice of a wider matrix."""
    b = _batch("edge", 32)
    c = stage_case(b, 32, 4)
    cm = _workspace(b)
    _prep(cm, b, dev)
    args = (_t(c["ea"], dev), _t(c["we"], dev), _t(c["be"], dev))
    vec = cm.aggregate_pna_edges(_t(c["p"], dev), _t(c["q"], dev), *args)
    assert torch.equal(cm.aggregate_pna_edges(_t(c["p"], dev), _t(c["q"], dev), *args), vec)
    out = _offset(np.zeros((b.num_nodes, 128), np.float32), dev)
    got = cm.aggregate_pna_edges(_offset(c["p"], dev), _offset(c["q"], dev), *args, out=out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(got, vec)
    wide = torch.zeros((32, 7), device=dev)
    wide[:, 2:6] = args[1]
    assert torch.equal(cm.aggregate_pna_edges(_t(c["p"], dev), _t(c["q"], dev), _offset(c["ea"], dev), wide[:, 2:6], args[2]), vec)
    noq = cm.aggregate_pna_edges(_t(c["p"], dev), None, *args)
    assert torch.equal(cm.aggregate_pna_edges(_offset(c["p"], dev), None, *args), noq) and not torch.equal(noq, vec)
    cm.check()


def test_stage_without_edges(dev):
    rng = np.random.default_rng(3)
    b = pack_graphs([ONE(12), EMPTY(12), (rng.uniform(-1, 1, (5, 12)).astype(np.float32), np.zeros((0, 2), np.int32))])
    assert b.num_edges == 0
    cm = _workspace(b)
    _prep(cm, b, dev)
    we, be = _t(rng.uniform(-1, 1, (12, 4)).astype(np.float32), dev), _t(rng.uniform(-1, 1, 12).astype(np.float32), dev)
    out = torch.full((b.num_nodes, 48), 7.0, device=dev)
    got = cm.aggregate_pna_edges(_t(b.x, dev), _t(b.x, dev), None, we, be, out=out)  # (NULL edge_attr)
    cm.check()
    assert not got.cpu().numpy().any()


# ---------------------------------------------------------------------------------------------------- 3. whole models
# Seeds of the models' weights, chosen on the CPU so that assert_no_variance_near_the_threshold holds with nothing excluded: of
# seeds 0 .. 11 the three MODELS pass at 0, 2, 3, 4, 6, 9 and 11 (9 has the widest margin, and also passes on the promise and the
# trailing-empty batches); the 300-graph PyG batch has ~170 k (node, column) pairs per layer and a pair within the margin at every
# seed of 0 .. 79 but 17
SEED, PYG_SEED = 9, 17
MODELS = {
    "L3-h128-skip": dict(in_dim=9, edge_dim=3, hidden=128, layers=3, skip=True, pools=("add", "mean", "max")),
    "L1": dict(in_dim=9, edge_dim=3, hidden=32, layers=1, skip=False, pools=("add", "mean", "max")),
    "L2-h64-gelu-softmax": dict(in_dim=9, edge_dim=3, hidden=64, layers=2, act="gelu", out_act=torch.nn.Softmax, pools=("mean",)),
}


def _forward(model, batch, ea, dev, promise=0, degree=0):
    cm = runtime.CompiledModel.from_model(model, *CAP)
    if promise:
        cm.set_max_graph_nodes(promise)
    if degree:
        cm.set_max_degree(degree)
    xd, cood, nptr, eptr = to_dev(batch, dev)
    out = cm.forward_edges(xd, _t(ea, dev), cood, nptr, eptr)
    cm.check()
    assert cm.last_path() == "layerwise"
    return cm, out


def assert_no_variance_near_the_threshold(model, batch, x, ea):
    """Every layer's per-(node, column) variance of the float64 reference stays 16 * 2^-24 * max_j h_ij^2 -- sixteen roundings of
    the largest square in the row's sum -- away from PyG's 1e-5: fp32 decides the std's clamp and mask as float64 does."""
    for l, (var, hi) in enumerate(layer_variances(model, batch, x, ea)):
        near = np.abs(var - R.PNA_STD_EPS) <= 16 * 2.0 ** -24 * hi
        assert not near.any(), (l, int(near.sum()), var[near][:4], hi[near][:4])


@pytest.mark.parametrize("name", list(MODELS))
def test_whole_models_against_float64(dev, name):
    model = make_pnae_model(seed=SEED, **MODELS[name])
    b = edge_batch(8, 9, seed=21)
    ea = edge_attrs(b.num_edges, 3, seed=22)
    assert_no_variance_near_the_threshold(model, b, b.x, ea)
    cm, out = _forward(model, b, ea, dev)
    record(f"forward_edges/pnae-{name}", out.cpu().numpy(), forward64(model, b, b.x, ea), run(model, b, b.x, ea))
    # the same forward again gives the same bits (no atomics, a fixed summation order)
    xd, cood, nptr, eptr = to_dev(b, dev)
    assert torch.equal(cm.forward_edges(xd, _t(ea, dev), cood, nptr, eptr), out)
    cm.graph_prep(cood, nptr, eptr, b.num_nodes)
    assert torch.equal(cm.forward_prepared_edges(xd, _t(ea, dev)), out)
    assert cm.last_path() == "layerwise" and cm.lib.gnnb_model_edge_dim(cm._model) == 3


# ---------------------------------------------------------------------------------------------------- 4. promises
def test_promises_change_neither_the_path_nor_a_bit(dev):
    model = make_pnae_model(seed=SEED, **MODELS["L3-h128-skip"])
    mols, rng = synthetic.make_batch("qm9", 12, seed=23), np.random.default_rng(23)
    b = pack_graphs([(rng.uniform(-1, 1, (mols.graph(g)[0].shape[0], 9)).astype(np.float32), mols.graph(g)[1]) for g in range(12)])
    assert np.diff(b.node_ptr).max() <= 64 and np.bincount(b.coo[:, 1]).max() <= 15
    ea = edge_attrs(b.num_edges, 3, seed=24)
    assert_no_variance_near_the_threshold(model, b, b.x, ea)
    _, plain = _forward(model, b, ea, dev)
    _, nodes = _forward(model, b, ea, dev, promise=64)  # (asserts "layerwise", and check(): the promise holds)
    _, degree = _forward(model, b, ea, dev, degree=15)
    _, both = _forward(model, b, ea, dev, promise=64, degree=15)
    assert torch.equal(plain, nodes) and torch.equal(plain, degree) and torch.equal(plain, both)
    record("forward_edges/pnae-L3-h128-skip-promises", both.cpu().numpy(), forward64(model, b, b.x, ea), run(model, b, b.x, ea))


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
    model = make_pnae_model(in_dim=11, edge_dim=4, hidden=32, layers=2, seed=PYG_SEED)
    cm = runtime.CompiledModel.from_model(model, *ICAP)
    cm.enable_edge_ingest()
    cm.enable_edge_ingest()  # (a second call is a no-op)
    return dict(b=b, x=x, ei=ei, ea=ea, ei_sh=np.ascontiguousarray(ei[:, perm]), ea_sh=np.ascontiguousarray(ea[perm]), cm=cm, model=model,
                batch=batch_vector(b))


def test_pyg_batches_grouped_and_permuted(pyg, dev):
    cm, b, model = pyg["cm"], pyg["b"], pyg["model"]
    xd, batch_dev = _t(pyg["x"], dev), _t(pyg["batch"], dev)
    for kind, ei, ea in (("grouped", pyg["ei"], pyg["ea"]), ("permuted", pyg["ei_sh"], pyg["ea_sh"])):
        gb, ea_ord = from_pyg_batch(pyg["x"], ei, edge_attr=ea, batch=pyg["batch"], num_graphs=300)
        assert_no_variance_near_the_threshold(model, gb, pyg["x"], ea_ord)
        out = cm.forward_pyg_edges(xd, _t(ei, dev), _t(ea, dev), batch=batch_dev, num_graphs=300).clone()
        cm.check()
        assert cm.last_path() == "layerwise"
        record(f"forward_pyg_edges/pnae-{kind}", out.cpu().numpy(), forward64(model, gb, pyg["x"], ea_ord), run(model, gb, pyg["x"], ea_ord))
        host = cm.forward_edges(xd, _t(ea_ord, dev), _t(gb.coo, dev), _t(gb.node_ptr, dev), _t(gb.edge_ptr, dev))
        assert torch.equal(out, host)  # (the ingest's arrays are the host's, so are the bits)


def test_trailing_empty_graphs_are_pooled(dev):
    model = make_pnae_model(seed=SEED, **MODELS["L3-h128-skip"])
    mols = synthetic.make_batch("qm9", 6, seed=31)
    b = pack_graphs([(mols.graph(g)[0][:, :9], mols.graph(g)[1]) for g in range(6)] + [EMPTY(9), EMPTY(9)])
    ea = edge_attrs(b.num_edges, 3, seed=32)
    assert_no_variance_near_the_threshold(model, b, b.x, ea)
    _, out = _forward(model, b, ea, dev)
    assert out.shape == (8, 19)
    record("forward_edges/pnae-trailing-empty", out.cpu().numpy(), forward64(model, b, b.x, ea), run(model, b, b.x, ea))


# ---------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals(pyg, dev):
    cm, b = pyg["cm"], pyg["b"]
    xd, ei, ea, batch_dev = _t(pyg["x"], dev), _t(pyg["ei"], dev), _t(pyg["ea"], dev), _t(pyg["batch"], dev)
    cood, nptr, eptr = _t(b.coo, dev), _t(b.node_ptr, dev), _t(b.edge_ptr, dev)
    good = cm.forward_edges(xd, ea, cood, nptr, eptr).clone()
    # the entries without edge attributes refuse the model, and name the entry that takes them
    with pytest.raises(runtime.GnnbError, match="gnnb_forward_batched_edges"):
        cm.forward(xd, cood, nptr, eptr)
    with pytest.raises(runtime.GnnbError, match="gnnb_forward_prepared_edges"):
        cm.forward_prepared(xd)
    with pytest.raises(runtime.GnnbError, match="gnnb_forward_pyg_edges"):
        cm.forward_pyg(xd, ei, batch=batch_dev, num_graphs=300)
    ordered = runtime.CompiledModel.from_model(pyg["model"], *ICAP)
    ordered.enable_ordered_ingest()
    with pytest.raises(runtime.GnnbError, match="gnnb_forward_pyg_edges"):
        ordered.forward_pyg_ordered(xd, ei, batch=batch_dev, num_graphs=300)
    with pytest.raises(runtime.GnnbError, match="gnnb_forward_prepared_edges"):
        cm.gcn_stack_timed(xd, 1)
    # gnnb_pna_edge_model_create refuses a GIN description (and gnnb_edge_model_create a PNA one)
    gin = make_model("gin", in_dim=11, hidden=32)
    host = [np.ascontiguousarray(p.numpy()) for p in gin.canonical_params()]
    arr = (C.c_void_p * len(host))(*[h.ctypes.data for h in host])
    handle, d = C.c_void_p(), runtime.make_desc(gin.spec())
    assert cm.lib.gnnb_pna_edge_model_create(C.byref(d), 4, arr, len(host), C.byref(handle)) == -1 and not handle
    assert b"PNA" in cm.lib.gnnb_last_error()
    assert cm.lib.gnnb_edge_model_create(C.byref(cm.desc), 4, arr, len(host), C.byref(handle)) == -1 and not handle
    # a model without edge weights is refused by the _edges entries
    pna = runtime.CompiledModel.from_model(make_model("pna", in_dim=11, hidden=32), *ICAP)
    assert pna.edge_dim == 0 and cm.edge_dim == 4 and cm.lib.gnnb_model_edge_dim(cm._model) == 4
    with pytest.raises(runtime.GnnbError, match="GINE"):
        pna.forward_edges(xd, ea, cood, nptr, eptr)
    # edge_attr of another shape, dtype or device is refused before any launch
    for bad, what in ((ea[:-1], "edge_attr must be"), (torch.zeros((b.num_edges, 5), device=dev), "edge_attr has shape"),
                      (ea.double(), "float32"), (ea.cpu(), "CUDA"), (None, "edge_attr is required")):
        with pytest.raises(runtime.GnnbError, match=what):
            cm.forward_edges(xd, bad, cood, nptr, eptr)
        with pytest.raises(runtime.GnnbError, match=what):
            cm.forward_pyg_edges(xd, ei, bad, batch=batch_dev, num_graphs=300)
    with pytest.raises(runtime.GnnbError, match="edge_attr must be"):
        cm.forward_prepared_edges(xd, ea[:-1])
    with pytest.raises(runtime.GnnbError, match="q must be"):
        cm.aggregate_pna_edges(xd, xd[:-1], ea, torch.zeros((11, 4), device=dev), torch.zeros(11, device=dev))
    # nothing above left a flag or changed a result
    cm.check()
    assert torch.equal(cm.forward_edges(xd, ea, cood, nptr, eptr), good)
