"""``k_nnconv_aggregate`` (csrc/k_nnconv.hip) and ``nnconv_layer``'s GEMM where ``tests/test_hip_nnconv.py`` does not reach:

a. a batch of ~21 k nodes, so that every workgroup walks several steps (the software pipeline's hand-over, long rows met in a
   later step, the last sweep partly filled, the ``node = N`` tail of ``row_of``), in-degrees on both sides of NN_R = 4, NN_CHUNK =
   64 and of a round-robin round;
b. bit identity of a row across its placement (the kernel header: the summation order depends on the batch, never on the launch
   shape);
c. every instantiation -- (L) at every ``d`` 1 ... 16, (H) at each of the 18 (KP, ED) pairs on the rung and strictly inside it --
   in the 16-byte and the scalar form, ``edge_attr`` off the 16-byte grid, ``out`` as a column slice of a wider matrix;
d. whole models whose second layer's GEMM has K = ``(K' + 2) hidden`` up to 4608 in two K-segments ``[A | x]`` cut at odd places,
   on the workspace's stream-K scratch.

Acceptance is ``ref64.budget`` with the project's K = 4, F = 2^-22, every element compared -- no tolerance
of this file's own.  Stage results are judged per in-degree class with the class's own ``max|ref|`` and as a whole
(``gine_util.budget_by_degree``: one hub of 1200 messages otherwise sets the scale of every molecule's row).  The reference is
float64 numpy from ``nnconv_util`` (``aggregate_ref``; the many-sweep batch: ``aggregate_ref_blocks``, one coefficient block at a
time; whole models: ``forward64``), ``base`` the same in fp32.  Worst e / e32 per entry and class go to GNNB_FP64_REPORT=<file>.

The stage entry takes widths up to 256 (``runtime.MAX_NNCONV_WIDTH``), so GINE's two-pass 16-byte case at width 260 has no twin
here: the fifth many-sweep case is (256, d 2) instead -- the 16-byte form at the linear variant's rung 2."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import nnconv_util as U
import ref64 as R
from gine_util import budget_by_degree, degree_classes, edge_attrs
from gnnbuilder_amd import runtime
from helpers import STAR_IN_DEGREES, batch_vector, edge_batch, make_model, sample_graphs, sub_batch, sub_edge_rows, sweep_batch, to_dev
from test_hip_layer_widths import widths_batch

pytestmark = pytest.mark.gpu

GRAPHS = 1100
WG, WG_PER_CU = 256, 8  # k_nnconv.hip: threads of a workgroup, NN_WG_PER_CU (the most workgroups per CU the grid is cut for)
RUNGS, EDS = (1, 2, 4, 8, 12, 16), (4, 8, 16)  # nn_rung's ladder of K'; the hidden variant's padded edge_dim
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


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _offset(a, dev):
    """``a`` as a contiguous CUDA tensor that starts one float past a 16-byte boundary of its buffer."""
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32))
    v = torch.zeros(t.numel() + 4, dtype=torch.float32, device=dev)[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def record_classes(entry, got, ref, base, coo):
    for name, r in budget_by_degree(got, ref, base, coo, what=entry).items():
        WORST[f"{entry}/{name}"] = max(WORST.get(f"{entry}/{name}", 0.0), r)


def _workspace(batch, scale=1):
    """A workspace of ``scale`` times the batch's size for the stage entry (a GIN workspace: its tables keep explicit (v, v)
    edges, and they do not depend on the model)."""
    return runtime.CompiledModel.from_model(make_model("gin", in_dim=8, hidden=8, layers=1, out_dim=8), scale * batch.num_graphs,
                                            scale * batch.num_nodes, scale * batch.num_edges)


def _prepared(batch, dev, scale=1):
    cm = _workspace(batch, scale)
    _, cood, nptr, eptr = to_dev(batch, dev)
    cm.graph_prep(cood, nptr, eptr, batch.num_nodes)
    return cm


def _groups(width):
    """Rows per step of a workgroup: 256 >> glog2, a lane group = the smallest power of two >= width / VEC, at most a wave."""
    nvec = width // 4 if width % 4 == 0 else width
    g = 1
    while g < min(nvec, 64):
        g *= 2
    return WG // g


# ---------------------------------------------------------------------------------------------------- the edge network (H)
def edge_net(K, d, seed):
    """(w1 [K, d] uniform(-1, 1) / sqrt(d), b1 [K] uniform(-0.3, 0.3)); K = 0: (None, None), the linear variant."""
    if not K:
        return None, None
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (K, d)) / np.sqrt(d)).astype(np.float32), rng.uniform(-0.3, 0.3, K).astype(np.float32)


def relu_cuts_and_passes(ea, w1, b1):
    """On the float64 coefficients alone: every hidden unit is exactly 0 on some edge and positive on another -- a missing ReLU
    or a ``b1`` in the wrong place changes ``A``."""
    hid = U.coefs(ea, w1, b1, np.float64)[:, :-1]
    return bool((hid == 0).any(0).all() and (hid > 0).any(0).all())


# ---------------------------------------------------------------------------------------------------- a. a many-sweep batch
# (width, d, K, aggr), every one at 4 rows per step: (33, 16, 0) scalar, one column pass, (L) rung 16; (33, 5, 12) scalar, (H)
# rung 12 / ED 8; (130, 3, 2) scalar, three column passes; (256, 4, 0) the 16-byte form; (256, 2, 0) the 16-byte form at (L) rung 2
# (module docstring: width 260 is refused); (256, 16, 16) the instantiation that runs one wave per SIMD
SWEEPS = [(33, 16, 0, "add"), (33, 5, 12, "mean"), (130, 3, 2, "add"), (256, 4, 0, "mean"), (256, 2, 0, "add"), (256, 16, 16, "mean")]
# edge_net seeds of the (H) cases: 2000 + 20 K + d -- 2245, 2043, 2336; tried on the CPU, each passes relu_cuts_and_passes on its
# case's edge_attr (asserted where the operands are made)


@pytest.fixture(scope="module")
def big(dev):
    """The batch (features of width 9: the whole model's; the stage cases draw their own), its stars' graph ids, its in-degrees,
    a prepared workspace of its size, and the cases' operands and references, made once."""
    b, stars = sweep_batch(GRAPHS, 9, seed=51)
    return dict(b=b, stars=stars, cm=_prepared(b, dev), deg=np.bincount(b.coo[:, 1], minlength=b.num_nodes), cache={})


def _inputs(big, width, d, K):
    key = ("in", width, d, K)
    if key not in big["cache"]:
        b, seed = big["b"], 1000 * width + 20 * K + d
        x = np.random.default_rng(seed).uniform(-1, 1, (b.num_nodes, width)).astype(np.float32)
        ea = edge_attrs(b.num_edges, d, seed + 200)
        w1, b1 = edge_net(K, d, 2000 + 20 * K + d)
        assert not K or relu_cuts_and_passes(ea, w1, b1)
        big["cache"][key] = (x, ea, w1, b1)
    return big["cache"][key]


def _refs(big, width, d, K, aggr):
    """(float64 reference, fp32 ``base``), one coefficient block at a time: the ``[E, K' + 1, w]`` tensor is never built."""
    key = ("ref", width, d, K, aggr)
    if key not in big["cache"]:
        x, ea, w1, b1 = _inputs(big, width, d, K)
        big["cache"][key] = tuple(U.aggregate_ref_blocks(x, big["b"].coo, ea, w1, b1, aggr, t) for t in (np.float64, np.float32))
    return big["cache"][key]


def sweeps_guaranteed(num_nodes, groups, cus):
    """Sweeps every workgroup walks at the kernel's highest possible occupancy (fewer resident workgroups: more sweeps)."""
    return -(-(-(-num_nodes // groups)) // (WG_PER_CU * cus))


def _sweeps_precondition(big, width):
    """From the batch and the CU count alone: every listed in-degree occurs, all three in-degree classes do, and with 4 rows per
    step the batch has more than 2 * NN_WG_PER_CU * CUs steps -- at least three sweeps whatever occupancy the launch measures."""
    assert set(STAR_IN_DEGREES) <= set(np.unique(big["deg"]).tolist())
    assert len(degree_classes(big["b"].coo, big["b"].num_nodes)) == 3
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    groups = _groups(width)
    assert groups == 4
    steps = -(-big["b"].num_nodes // groups)
    assert steps > 2 * WG_PER_CU * cus, (steps, cus)
    assert sweeps_guaranteed(big["b"].num_nodes, groups, cus) >= 3


def _run_big(cm, big, dev, width, d, K, aggr):
    x, ea, w1, b1 = _inputs(big, width, d, K)
    got = cm.aggregate_nnconv(_t(x, dev), _t(ea, dev), None if w1 is None else _t(w1, dev), None if b1 is None else _t(b1, dev), aggr=aggr)
    cm.check()
    return got


@pytest.mark.parametrize("width,d,K,aggr", SWEEPS)
def test_many_sweeps_against_float64(big, dev, width, d, K, aggr):
    _sweeps_precondition(big, width)
    got = _run_big(big["cm"], big, dev, width, d, K, aggr)
    ref, base = _refs(big, width, d, K, aggr)
    assert got.shape == ref.shape == (big["b"].num_nodes, ((K or d) + 1) * width)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(f"CUs {cus}, nodes {big['b'].num_nodes}: at least {sweeps_guaranteed(big['b'].num_nodes, 4, cus)} sweeps")
    record_classes(f"aggregate_nnconv/sweeps-w{width}-d{d}-K{K}-{aggr}", got.cpu().numpy(), ref, base, big["b"].coo)
    none = big["deg"] == 0  # rows without an in-edge: there are some, the reference is 0 there, and the result is written and exactly 0
    assert none.any() and not ref[none].any() and not got[torch.from_numpy(none).to(dev)].any()


# ---------------------------------------------------------------------------------------------------- b. placement
@pytest.mark.parametrize("width,d,K,aggr", [(256, 4, 0, "mean"), (33, 5, 12, "mean")])
def test_a_row_has_the_same_bits_wherever_it_is_placed(big, dev, width, d, K, aggr):
    """A second launch; the stars and 64 sampled graphs as a batch of their own -- one step per workgroup, other workgroups and
    lane groups --; a workspace of three times the capacities: the bits of the several-sweep run."""
    _sweeps_precondition(big, width)
    first = _run_big(big["cm"], big, dev, width, d, K, aggr)
    assert torch.equal(_run_big(big["cm"], big, dev, width, d, K, aggr), first), "a second launch"
    x, ea, w1, b1 = _inputs(big, width, d, K)
    b = big["b"]
    gids = np.union1d(big["stars"], sample_graphs(b, seed=7, count=64))
    sub, rows = sub_batch(dataclasses.replace(b, x=x), gids)
    assert np.array_equal(sub.x, x[rows]) and set(STAR_IN_DEGREES) <= set(np.bincount(sub.coo[:, 1]).tolist())
    # one step per workgroup: 4 workgroups per CU are resident for (L) <4, 4> and for (H) <1, 12, 8> (DESIGN.md section 3.2n's table:
    # 4 waves per SIMD, a workgroup is one wave on each)
    assert -(-sub.num_nodes // _groups(width)) <= 4 * torch.cuda.get_device_properties(0).multi_processor_count
    small = _prepared(sub, dev)
    got = small.aggregate_nnconv(_t(sub.x, dev), _t(ea[sub_edge_rows(b, gids)], dev), None if w1 is None else _t(w1, dev),
                                 None if b1 is None else _t(b1, dev), aggr=aggr)
    small.check()
    assert torch.equal(got, first[torch.from_numpy(rows).to(dev)]), "the rows in a batch of their own"
    assert torch.equal(_run_big(_prepared(b, dev, scale=3), big, dev, width, d, K, aggr), first), "a workspace of three times the capacities"


# ---------------------------------------------------------------------------------------------------- c. every instantiation
# (K, d).  (L): every d.  (H): each of the 18 (KP, ED) pairs on the rung (K = KP, d = ED) and inside it (d = ED - 1; K = KP - 1 where
# that stays above the rung below -- KP 4, 8, 12, 16 --, else K = KP).  ``aggr`` alternates with K + d and is the other one at the
# other width, so every case -- and with it every rung -- runs both
INSTANCES = [(0, d) for d in range(1, 17)] + [(kp, ed) for kp in RUNGS for ed in EDS] + \
            [(kp - 1 if kp >= 4 else kp, ed - 1) for kp in RUNGS for ed in EDS]
# edge_net seeds of the (H) cases: 1000 + 20 K + d (1023 ... 1336); tried on the CPU, every one passes relu_cuts_and_passes on its
# case's edge_attr -- the same rows at both widths -- and every test asserts it
STAGE_SEED = 70


@pytest.fixture(scope="module")
def stage(dev):
    """``edge_batch(8, width, STAGE_SEED)`` at both widths -- the same graphs up to the order of some edges, so as many attribute
    rows -- with a hub of in-degree 1200, self loops, duplicate edges and rows without in-edges; a prepared workspace each."""
    bs = {w: edge_batch(8, w, seed=STAGE_SEED) for w in (8, 6)}
    assert bs[8].num_edges == bs[6].num_edges and np.array_equal(bs[8].node_ptr, bs[6].node_ptr)
    return dict(b=bs, cm={w: _prepared(b, dev) for w, b in bs.items()})


def stage_attrs(num_edges, d):
    return edge_attrs(num_edges, d, seed=300 + d)


@pytest.mark.parametrize("width", [8, 6])  # the 16-byte form / the scalar form
@pytest.mark.parametrize("K,d", INSTANCES, ids=[f"K{k}-d{d}" for k, d in INSTANCES])
def test_every_instantiation_against_float64(stage, dev, width, K, d):
    b, cm = stage["b"][width], stage["cm"][width]
    aggr = ("add", "mean")[(K + d + (width == 6)) % 2]
    ea = stage_attrs(b.num_edges, d)
    w1, b1 = edge_net(K, d, 1000 + 20 * K + d)
    assert not K or relu_cuts_and_passes(ea, w1, b1)
    xd, net = _t(b.x, dev), (None if w1 is None else _t(w1, dev), None if b1 is None else _t(b1, dev))
    got = cm.aggregate_nnconv(xd, _t(ea, dev), *net, aggr=aggr)
    cm.check()
    ref, base = U.aggregate_ref(b.x, b.coo, ea, w1, b1, aggr), U.aggregate_ref(b.x, b.coo, ea, w1, b1, aggr, np.float32)
    cols = ((K or d) + 1) * width
    assert got.shape == ref.shape == (b.num_nodes, cols)
    record_classes(f"aggregate_nnconv/w{width}-d{d}-K{K}", got.cpu().numpy(), ref, base, b.coo)
    if d in (4, 8, 12, 16):  # attribute rows of whole 16-byte pieces: off their boundary they are read float by float
        off = cm.aggregate_nnconv(xd, _offset(ea, dev), *net, aggr=aggr)
        cm.check()
        assert torch.equal(off, got), "edge_attr one float off a 16-byte boundary"
    for extra in (3, 4):  # out as the leading columns of a wider matrix: row stride % 4 != 0 (the scalar form) and == 0
        wide = torch.full((b.num_nodes, cols + extra), float("nan"), dtype=torch.float32, device=dev)
        assert (wide.stride(0) % 4 == 0) == (extra == 4 and cols % 4 == 0)
        out = cm.aggregate_nnconv(xd, _t(ea, dev), *net, aggr=aggr, out=wide[:, :cols])
        cm.check()
        assert out.data_ptr() == wide.data_ptr() and torch.equal(wide[:, :cols], got), f"out in a matrix {extra} columns wider"
        assert torch.isnan(wide[:, cols:]).all(), "a column behind out was written: a padded block is stored"


# ---------------------------------------------------------------------------------------------------- d. the layer's GEMM
def _model_checks(cm, model, b, ea, dev, entry, ref, base):
    """``forward_edges`` against float64, a clean ``check()`` and stream-K guard, the bits again from a second call and from
    ``forward_pyg_edges`` on the batch's own edge order."""
    xd, cood, nptr, eptr = to_dev(b, dev)
    ead = _t(ea, dev)
    out = cm.forward_edges(xd, ead, cood, nptr, eptr).clone()
    cm.check()
    cm.stream_k_guard()
    assert cm.last_path() == "layerwise" and out.shape == (b.num_graphs, 19)
    got = out.cpu().numpy()
    e, e32, _ = R.errors(got, ref, base)
    print(f"{entry}: e = {e:.3e}, e32 = {e32:.3e}, e / e32 = {R.ratio(e, e32):.2f}")
    WORST[entry] = max(WORST.get(entry, 0.0), R.ratio(e, e32))
    R.budget(got, ref, base, what=entry)
    assert torch.equal(cm.forward_edges(xd, ead, cood, nptr, eptr), out), "a second call"
    ei = _t(np.ascontiguousarray(b.coo.T.astype(np.int64)).reshape(2, -1), dev)
    pyg = cm.forward_pyg_edges(xd, ei, ead, batch=_t(batch_vector(b), dev), num_graphs=b.num_graphs)
    assert torch.equal(pyg, out), "forward_pyg_edges"
    cm.check()
    cm.stream_k_guard()


# (hidden, d, K, aggr, K of the second layer's GEMM = (K' + 2) hidden): 4352 | 256, the largest; 1139 | 67, scalar segments; 1152 | 128
MODELS = [(256, 16, 16, "add", 4608), (67, 4, 16, "mean", 1206), (128, 8, 0, "add", 1280)]


@pytest.mark.parametrize("hidden,d,K,aggr,gemm_k", MODELS)
def test_the_layers_gemm_at_large_and_odd_k(dev, hidden, d, K, aggr, gemm_k):
    """in 9 -> hidden -> hidden, skip on, on molhiv-40 with an empty and a one-node graph (1052 nodes): the second layer's GEMM
    runs K = (K' + 2) hidden on the workspace's stream-K scratch (from K = 1024 on)."""
    model = U.make_model(9, hidden, 2, d, K, aggr, seed=hidden + d)
    assert ((K or d) + 2) * hidden == gemm_k >= 1024
    b, _ = widths_batch()
    ea = edge_attrs(b.num_edges, d, seed=500 + d)
    cm = runtime.CompiledModel.from_model(model, b.num_graphs, b.num_nodes, b.num_edges)
    cm.enable_edge_ingest()
    _model_checks(cm, model, b, ea, dev, f"forward_edges/nnconv-gemm-h{hidden}-d{d}-K{K}-{aggr}", U.forward64(model, b, b.x, ea), U.run(model, b, b.x, ea))


def test_whole_model_over_several_sweeps(big, dev):
    """hidden 256, d 4, K 0, two layers over the many-sweep batch: the second layer's aggregate takes several sweeps at width 256
    and its GEMM has K = 1536 (1280 | 256) over ~21 k rows.  The reference is ``forward64`` a few graphs at a time: the model's
    ``[E, in, out]`` tensor of the whole batch would take 26 GB."""
    _sweeps_precondition(big, 256)
    b = big["b"]
    model = U.make_model(9, 256, 2, 4, 0, "mean", seed=8)
    ea = edge_attrs(b.num_edges, 4, seed=53)
    cm = runtime.CompiledModel.from_model(model, b.num_graphs, b.num_nodes, b.num_edges)
    cm.enable_edge_ingest()
    ref, base = U.forward_by_graphs(model, b, b.x, ea), U.forward_by_graphs(model, b, b.x, ea, double=False)
    _model_checks(cm, model, b, ea, dev, "forward_edges/nnconv-sweeps-L2-h256-d4-K0", ref, base)
