"""``k_gine_aggregate`` (csrc/k_gine.hip) where ``tests/test_hip_gine.py`` does not reach: a batch of ~21 k nodes, so that every
workgroup walks several steps (the software pipeline, long rows in more than one step, the last sweep partly filled, the row
index of a later step), in-degrees on both sides of GINE_R = 4, GINE_CHUNK = 64 and of a round-robin round, every
``edge_dim`` 1 ... 16 in both forms, bit identity of a row across its placement, a whole model over several sweeps, and
``k_edge_attr_order`` at row lengths other than 4.

The float64 reference and the fp32 ``base`` of the stage entry are ``test_hip_gine._stage_refs``; acceptance is ``ref64.budget``
with the project's K = 4, F = 2^-22, applied to the rows of each in-degree class with the class's own ``max|ref|`` and to the
whole array (``gine_util.budget_by_degree``: one hub of 1200 messages otherwise sets the scale of every molecule's row) -- no
tolerance of this file's own.  Worst e / e32 per entry and class go to GNNB_FP64_REPORT=<file>."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import ref64 as R
import test_hip_gine as TG
from gine_util import budget_by_degree, degree_classes, edge_attrs, forward64, make_gine_model, run, stage_weights
from gnnbuilder_amd import runtime
from gnnbuilder_amd.batching import from_pyg_batch
from helpers import STAR_IN_DEGREES, edge_batch, make_model, sample_graphs, sub_batch, sub_edge_rows, sweep_batch, to_dev

pytestmark = pytest.mark.gpu

GRAPHS = 1100
WG, WG_PER_CU = 256, 8  # k_gine.hip: threads of a workgroup, GINE_WG_PER_CU (the most workgroups per CU the grid is cut for)
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


def _workspace(batch):
    """A workspace of exactly the batch's size for the stage entry (its tables do not depend on the model)."""
    return runtime.CompiledModel.from_model(make_model("gin", in_dim=8, hidden=8, layers=1, out_dim=8), batch.num_graphs,
                                            batch.num_nodes, batch.num_edges)


def _groups(width):
    """Rows per step of a workgroup: 256 >> glog2, a lane group = the smallest power of two >= width / VEC, at most a wave."""
    nvec = width // 4 if width % 4 == 0 else width
    g = 1
    while g < min(nvec, 64):
        g *= 2
    return WG // g


# ---------------------------------------------------------------------------------------------------- 1. a many-sweep batch
@pytest.fixture(scope="module")
def big(dev):
    """The batch (features of width 9: the whole model's; the stage cases draw their own), its stars' graph ids, its
    in-degrees and a prepared workspace of its size."""
    b, stars = sweep_batch(GRAPHS, 9, seed=51)
    cm = _workspace(b)
    _, cood, nptr, eptr = to_dev(b, dev)
    cm.graph_prep(cood, nptr, eptr, b.num_nodes)
    return dict(b=b, stars=stars, cm=cm, deg=np.bincount(b.coo[:, 1], minlength=b.num_nodes), cache={})


def _inputs(big, width, edge_dim):
    key = ("in", width, edge_dim)
    if key not in big["cache"]:
        b, seed = big["b"], 1000 * width + edge_dim
        x = np.random.default_rng(seed).uniform(-1, 1, (b.num_nodes, width)).astype(np.float32)
        big["cache"][key] = (x, edge_attrs(b.num_edges, edge_dim, seed + 200)) + stage_weights(width, edge_dim, seed + 100)
    return big["cache"][key]


def _refs(big, width, edge_dim, eps):
    key = ("ref", width, edge_dim, eps)
    if key not in big["cache"]:
        x, ea, we, be = _inputs(big, width, edge_dim)
        big["cache"][key] = TG._stage_refs(x, big["b"].coo, ea, we, be, eps)
    return big["cache"][key]


def _sweeps_precondition(big, width):
    """Every listed in-degree occurs, and the batch is at least 3 sweeps (2 at width 128: 8 rows per step) at the kernel's
    highest possible occupancy -- whatever the occupancy the launch measures."""
    assert set(STAR_IN_DEGREES) <= set(np.unique(big["deg"]).tolist())
    assert len(degree_classes(big["b"].coo, big["b"].num_nodes)) == 3
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    groups = _groups(width)
    assert groups == (8 if width == 128 else 4)
    steps = -(-big["b"].num_nodes // groups)
    assert steps > (1 if width == 128 else 2) * WG_PER_CU * cus, (steps, cus)


def _run_big(big, dev, width, edge_dim, eps):
    x, ea, we, be = _inputs(big, width, edge_dim)
    got = big["cm"].aggregate_edges_fused(TG._t(x, dev), TG._t(ea, dev), TG._t(we, dev), TG._t(be, dev), eps=eps)
    big["cm"].check()
    return got


# (33, 3): scalar, G = 64, one column pass; (130, 5): scalar, three passes; (256, 4): float4, one pass; (260, 16): float4, two
# passes, the lowest occupancy; (128, 8): float4, 8 rows per step, attribute rows of two float4
@pytest.mark.parametrize("width,edge_dim,eps", [(33, 3, 0.3), (130, 5, 0.3), (256, 4, 0.3), (260, 16, 0.3), (128, 8, 0.3), (256, 4, 0.0)])
def test_many_sweeps_against_float64(big, dev, width, edge_dim, eps):
    _sweeps_precondition(big, width)
    got = _run_big(big, dev, width, edge_dim, eps)
    ref, base = _refs(big, width, edge_dim, eps)
    record_classes(f"aggregate_edges_fused/sweeps-w{width}-ed{edge_dim}" + ("" if eps else "-eps0"), got.cpu().numpy(), ref, base,
                   big["b"].coo)


# ---------------------------------------------------------------------------------------------------- 3. placement
@pytest.mark.parametrize("width,edge_dim", [(256, 4), (33, 3)])
def test_a_row_has_the_same_bits_wherever_it_is_placed(big, dev, width, edge_dim):
    """The summation order depends on the batch, never on the launch shape (k_gine.hip's header): the stars and 64 sampled
    graphs as a batch of their own -- one step per workgroup, other workgroups and lane groups -- give the bits of the
    several-sweep run."""
    _sweeps_precondition(big, width)
    first = _run_big(big, dev, width, edge_dim, 0.3)
    assert torch.equal(_run_big(big, dev, width, edge_dim, 0.3), first)
    x, ea, we, be = _inputs(big, width, edge_dim)
    b = big["b"]
    gids = np.union1d(big["stars"], sample_graphs(b, seed=7, count=64))
    sub, rows = sub_batch(dataclasses.replace(b, x=x), gids)
    assert np.array_equal(sub.x, x[rows]) and set(STAR_IN_DEGREES) <= set(np.bincount(sub.coo[:, 1]).tolist())
    # one step per workgroup: 4 workgroups per CU are resident for <4, 4>, 6 for <1, 3>
    assert -(-sub.num_nodes // _groups(width)) <= 4 * torch.cuda.get_device_properties(0).multi_processor_count
    small = _workspace(sub)
    xd, cood, nptr, eptr = to_dev(sub, dev)
    small.graph_prep(cood, nptr, eptr, sub.num_nodes)
    got = small.aggregate_edges_fused(xd, TG._t(ea[sub_edge_rows(b, gids)], dev), TG._t(we, dev), TG._t(be, dev), eps=0.3)
    small.check()
    assert torch.equal(got, first[torch.from_numpy(rows).to(dev)])


# ---------------------------------------------------------------------------------------------------- 4. every instantiation
@pytest.fixture(scope="module")
def stage_cm(dev):
    return runtime.CompiledModel.from_model(make_model("gin", in_dim=8, hidden=8, layers=1, out_dim=8), *TG.CAP)


@pytest.mark.parametrize("width", [8, 6])  # float4 / scalar
@pytest.mark.parametrize("edge_dim", range(1, 17))
def test_every_instantiation_against_float64(stage_cm, dev, width, edge_dim):
    b = edge_batch(8, width, seed=60 + width)
    ea = edge_attrs(b.num_edges, edge_dim, seed=300 + edge_dim)
    we, be = stage_weights(width, edge_dim, seed=400 + edge_dim)
    xd = TG._prep(stage_cm, b, dev)
    args = (TG._t(we, dev), TG._t(be, dev))
    got = stage_cm.aggregate_edges_fused(xd, TG._t(ea, dev), *args, eps=0.3)
    stage_cm.check()
    ref, base = TG._stage_refs(b.x, b.coo, ea, we, be, 0.3)
    record_classes(f"aggregate_edges_fused/w{width}-ed{edge_dim}", got.cpu().numpy(), ref, base, b.coo)
    if edge_dim in (8, 12, 16):  # attribute rows of several float4: off their 16-byte boundary they are read float by float
        off = stage_cm.aggregate_edges_fused(xd, TG._offset(ea, dev), *args, eps=0.3)
        stage_cm.check()
        assert torch.equal(off, got)


# ---------------------------------------------------------------------------------------------------- 5. a whole model
def test_whole_model_over_several_sweeps(big, dev):
    _sweeps_precondition(big, 256)
    b = big["b"]
    model = make_gine_model(in_dim=9, edge_dim=16, hidden=256, layers=2, pools=("add", "mean", "max"), seed=6)
    ea = edge_attrs(b.num_edges, 16, seed=52)
    cm = runtime.CompiledModel.from_model(model, b.num_graphs, b.num_nodes, b.num_edges)
    xd, cood, nptr, eptr = to_dev(b, dev)
    out = cm.forward_edges(xd, TG._t(ea, dev), cood, nptr, eptr)
    cm.check()
    assert cm.last_path() == "layerwise" and out.shape == (b.num_graphs, 19)
    got, ref, base = out.cpu().numpy(), forward64(model, b, b.x, ea), run(model, b, b.x, ea)
    e, e32, _ = R.errors(got, ref, base)
    print(f"forward_edges/sweeps-L2-h256-ed16: e = {e:.3e}, e32 = {e32:.3e}, e / e32 = {R.ratio(e, e32):.2f}")
    R.budget(got, ref, base, what="forward_edges/sweeps-L2-h256-ed16")
    WORST["forward_edges/sweeps-L2-h256-ed16"] = R.ratio(e, e32)


# ---------------------------------------------------------------------------------------------------- 6. the ingest's attribute rows
@pytest.fixture(scope="module")
def ingest_cms(dev):
    made = {}

    def get(edge_dim):
        if edge_dim not in made:
            made[edge_dim] = runtime.CompiledModel.from_model(make_gine_model(in_dim=4, edge_dim=edge_dim, hidden=8, layers=1, seed=5),
                                                              8, 64, 8192)
            made[edge_dim].enable_edge_ingest()
        return made[edge_dim]
    return get


@pytest.mark.parametrize("E", [1, 255, 257, 4097])
@pytest.mark.parametrize("edge_dim", [1, 3, 16])
def test_ingest_orders_attribute_rows_of_other_lengths(ingest_cms, dev, edge_dim, E):
    """``k_edge_attr_order`` at rows of 1, 3 and 16 floats around a workgroup and past four tiles, on shuffled edges (the
    batches of test_hip_ingest.test_edge_counts_around_wave_workgroup_and_tile)."""
    m = ingest_cms(edge_dim)
    rng = np.random.default_rng(100 * E + edge_dim)
    sizes = np.array([7, 9, 8, 3, 13])
    nptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    g = rng.integers(0, 5, E)
    ei = np.stack([nptr[g] + rng.integers(0, sizes[g]), nptr[g] + rng.integers(0, sizes[g])]).astype(np.int64).reshape(2, E)
    ea = edge_attrs(E, edge_dim, seed=E + edge_dim)
    N, batch = int(nptr[-1]), np.repeat(np.arange(5), sizes).astype(np.int64)
    for host_kw in ({"batch": batch, "num_graphs": 5}, {"ptr": nptr}):
        gb, ea_ord = from_pyg_batch(np.zeros((N, 1), np.float32), ei, edge_attr=ea, **host_kw)
        assert E < 2 or not np.array_equal(ea_ord, ea)  # (the rows do move)
        dev_kw = {k: (TG._t(v, dev) if isinstance(v, np.ndarray) else v) for k, v in host_kw.items()}
        got = m.ingest_pyg_edges(TG._t(ei, dev), TG._t(ea, dev), num_nodes=N, **dev_kw)
        m.check()
        for t, r in zip(got, (gb.coo, gb.node_ptr, gb.edge_ptr, ea_ord)):
            assert t.cpu().numpy().dtype == r.dtype and t.shape == r.shape and np.array_equal(t.cpu().numpy(), r)
