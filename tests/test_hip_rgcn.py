"""RGCNConv models with integer edge types on the MI355X (include/gnnb_rgcn.h; csrc/k_rgcn.hip): the slot records, the flag for a
type out of range, the aggregate as a stage entry in its forms, layouts and absent terms, its bits, whole models through
``forward_types``, ``forward_prepared_types`` and ``forward_pyg_types``, degenerate batches, stale records, a captured forward,
and the refusals.

Acceptance is ``ref64.budget`` with the project's K = 4, F = 2^-22 -- no tolerance of this file's own -- per
in-degree class (``gine_util.budget_by_degree``), nothing left out of a comparison.  The reference is float64
(``rgcn_util.rgcn_ref``; whole models: the model's own torch definition on a ``.double()`` copy); ``base`` is the same in fp32 on
the CPU in PyG's order.  Worst e / e32 per entry go to GNNB_FP64_REPORT=<file>."""
import json
import os

import numpy as np
import pytest
import torch

import gnnbuilder_amd as gnnb
import ref64 as R
import rgcn_util as U
from ggnn_util import WIDTHS
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
    """A GIN workspace for the stage entries (graph prep keeps explicit (v, v) edges there): of exactly the batch's size, or
    ``slack`` times as large."""
    return runtime.CompiledModel.from_model(make_model(conv, in_dim=8, hidden=8, layers=1, out_dim=8), slack * batch.num_graphs,
                                            slack * max(batch.num_nodes, 1), slack * batch.num_edges)


def _prep(cm, batch, dev):
    _, cood, nptr, eptr = to_dev(batch, dev)
    cm.graph_prep(cood, nptr, eptr, batch.num_nodes)


BATCHES, PREPARED, RECS, CASES = {}, {}, {}, {}


def _batch(kind):
    if kind not in BATCHES:
        BATCHES[kind] = edge_batch(8, 4, seed=21) if kind == "edge" else sweep_batch(24, 4, seed=5)[0]
    return BATCHES[kind]


def _types(kind, relations):
    return U.edge_types(_batch(kind), relations, seed=100 + relations)


def _prepared(kind, dev):
    """One prepared workspace per batch, shared by the tests of this file (nothing below changes its tables)."""
    if kind not in PREPARED:
        cm = _workspace(_batch(kind))
        _prep(cm, _batch(kind), dev)
        PREPARED[kind] = cm
    return PREPARED[kind]


def _rec(kind, relations, dev):
    """The device's slot records of (batch, relations): built once, shared, left unchanged."""
    if (kind, relations) not in RECS:
        cm = _prepared(kind, dev)
        RECS[kind, relations] = cm.rgcn_slots(_t(_types(kind, relations), dev), relations)
        cm.check()
    return RECS[kind, relations]


def _case(kind, width, relations):
    """(pr [N, (R + 1) width] -- the relation blocks and the root block, as one GEMM output --, skip [N, width], ref, base) of the
    plain stage call (root, no skip, no activation): computed once, shared, left unchanged."""
    key = (kind, width, relations)
    if key not in CASES:
        b = _batch(kind)
        rng = np.random.default_rng(1000 * width + relations)
        pr = rng.uniform(-1, 1, (b.num_nodes, (relations + 1) * width)).astype(np.float32)
        skip = rng.uniform(-1, 1, (b.num_nodes, width)).astype(np.float32)
        args = (pr[:, :relations * width], pr[:, relations * width:], None, "none", b.coo, _types(kind, relations), relations)
        CASES[key] = (pr, skip, U.rgcn_ref(*args), U.rgcn_ref(*args, dtype=np.float32))
    return CASES[key]


def _stage(cm, rec, pr, width, relations, dev, root=True, skip=None, act="none"):
    prd = _t(pr, dev)
    return cm.aggregate_rgcn(rec, prd[:, :relations * width], relations, root=prd[:, relations * width:] if root else None,
                             skip=_t(skip, dev) if skip is not None else None, act=act)


# ---------------------------------------------------------------------------------------------------- 1. the slot records
@pytest.mark.parametrize("kind", ["edge", "sweep"])
@pytest.mark.parametrize("relations", U.RELATIONS)
def test_slot_records_equal_numpys_to_the_bit(dev, relations, kind):
    b = _batch(kind)
    cm = _prepared(kind, dev)
    types = _types(kind, relations)
    rec = _rec(kind, relations, dev).cpu().numpy()
    row_ptr, _, in_deg = cm.tables_to_host()
    eid = cm.edge_index_table_to_host()
    assert np.array_equal(in_deg, np.bincount(b.coo[:, 1], minlength=b.num_nodes))  # (a GIN workspace: every edge has its slot)
    want = U.slot_records(types, b.coo, row_ptr, in_deg, eid, relations)
    assert rec.dtype == np.int32 and rec.shape == (b.num_edges, 2)
    assert np.array_equal(rec[:, 0], want[:, 0])  # the relations
    assert np.array_equal(rec[:, 1], want[:, 1])  # the weights' bits: 1.0f / (float)count, correctly rounded
    cnt = U.relation_counts(b.coo, types, relations, b.num_nodes)
    hub = int(np.argmax(in_deg))
    s = np.arange(row_ptr[hub], row_ptr[hub] + in_deg[hub])
    assert in_deg[hub] >= 1200 and np.array_equal(rec[s, 1], want[s, 1])
    if relations > 1:  # the hub holds relations with unlike counts; some row lacks a relation and has in-edges
        assert len(set(cnt[hub][cnt[hub] > 0])) >= 2 and ((cnt == 0).any(1) & (in_deg > 0)).any()
        w = rec[s, 1].view(np.float32)
        assert len(set(w.tolist())) >= 2 and np.array_equal(w, (np.float32(1) / cnt[hub, rec[s, 0]].astype(np.float32)))


# ---------------------------------------------------------------------------------------------------- 2. a type out of range
def test_a_type_out_of_range_is_flagged_once_and_adds_nothing(dev):
    relations, width, kind = 3, 32, "edge"
    b = _batch(kind)
    cm = _workspace(b)  # (its own workspace: the flag is the workspace's)
    _prep(cm, b, dev)
    types = _types(kind, relations).copy()
    bad = np.array([5, b.num_edges - 7])
    types[bad[0]], types[bad[1]] = relations, -1
    rec = cm.rgcn_slots(_t(types, dev), relations)
    with pytest.raises(runtime.GnnbError, match="flags 0x100"):
        cm.check()
    cm.check()  # reported once: clean now
    row_ptr, _, in_deg = cm.tables_to_host()
    eid = cm.edge_index_table_to_host()
    got = rec.cpu().numpy()
    assert np.array_equal(got, U.slot_records(types, b.coo, row_ptr, in_deg, eid, relations))
    slots = np.flatnonzero(np.isin(eid, bad))
    assert len(slots) == 2 and (got[slots] == 0).all()  # {0, 0.0f}
    pr, _, _, _ = _case(kind, width, relations)
    out = _stage(cm, rec, pr, width, relations, dev).cpu().numpy()
    cm.check()
    assert np.isfinite(out).all()
    # the lazy report: the next entry call on the workspace raises, once
    cm.rgcn_slots(_t(types, dev), relations)
    torch.cuda.synchronize()
    xd, cood, nptr, eptr = to_dev(b, dev)
    with pytest.raises(runtime.GnnbError, match="earlier batch"):
        cm.graph_prep(cood, nptr, eptr, b.num_nodes)
    cm.graph_prep(cood, nptr, eptr, b.num_nodes)
    cm.check()


# ---------------------------------------------------------------------------------------------------- 3. the stage against float64
@pytest.mark.parametrize("kind", ["edge", "sweep"])
@pytest.mark.parametrize("relations", U.RELATIONS)
@pytest.mark.parametrize("width", WIDTHS)
def test_stage_against_float64(dev, width, relations, kind):
    b = _batch(kind)
    deg = np.bincount(b.coo[:, 1], minlength=b.num_nodes)
    assert deg.max() >= 1200 and (deg == 0).sum() >= 5
    cm = _prepared(kind, dev)
    pr, _, ref, base = _case(kind, width, relations)
    got = _stage(cm, _rec(kind, relations, dev), pr, width, relations, dev)
    cm.check()
    got = got.cpu().numpy()
    assert got.shape == (b.num_nodes, width) and np.isfinite(got).all()
    record_classes(f"aggregate_rgcn/{kind}-w{width}-R{relations}", got, ref, base, b.coo)


# ---------------------------------------------------------------------------------------------------- 4. the scalar form, forced
@pytest.mark.parametrize("which", ["p", "root", "skip", "out"])
def test_an_operand_off_the_16_byte_grid_takes_the_scalar_form(dev, which):
    width, relations, kind = 32, 3, "edge"
    b = _batch(kind)
    cm = _prepared(kind, dev)
    pr, skip, _, _ = _case(kind, width, relations)
    p, root = np.ascontiguousarray(pr[:, :relations * width]), np.ascontiguousarray(pr[:, relations * width:])
    args = (p, root, skip, "none", b.coo, _types(kind, relations), relations)
    ref, base = U.rgcn_ref(*args), U.rgcn_ref(*args, dtype=np.float32)
    ops = dict(p=_t(p, dev), root=_t(root, dev), skip=_t(skip, dev), out=torch.empty((b.num_nodes, width), device=dev))
    ops[which] = _offset(dict(p=p, root=root, skip=skip, out=np.zeros((b.num_nodes, width), np.float32))[which], dev)
    got = cm.aggregate_rgcn(_rec(kind, relations, dev), ops["p"], relations, root=ops["root"], skip=ops["skip"], out=ops["out"])
    cm.check()
    record_classes(f"aggregate_rgcn/offset-{which}", got.cpu().numpy(), ref, base, b.coo)


# ---------------------------------------------------------------------------------------------------- 5. two layouts
@pytest.mark.parametrize("width", [32, 9])
def test_blocks_of_one_matrix_and_separate_tensors_agree(dev, width):
    relations, kind = 3, "sweep"
    b = _batch(kind)
    cm = _prepared(kind, dev)
    rec = _rec(kind, relations, dev)
    pr, _, ref, base = _case(kind, width, relations)
    one = _stage(cm, rec, pr, width, relations, dev)
    p, root = _t(pr[:, :relations * width], dev), _t(pr[:, relations * width:], dev)
    assert p.stride(0) == relations * width and root.stride(0) == width
    two = cm.aggregate_rgcn(rec, p, relations, root=root)
    cm.check()
    record_classes(f"aggregate_rgcn/blocks-w{width}", one.cpu().numpy(), ref, base, b.coo)
    record_classes(f"aggregate_rgcn/separate-w{width}", two.cpu().numpy(), ref, base, b.coo)
    if width % 4 == 0:  # (both layouts take the 16-byte form: the same summation order, the same bits)
        assert torch.equal(one, two)


# ---------------------------------------------------------------------------------------------------- 6. absent terms, activations
@pytest.mark.parametrize("with_skip", [True, False])
@pytest.mark.parametrize("with_root", [True, False])
@pytest.mark.parametrize("act", ACT_NAMES)
def test_epilogue_root_skip_and_activation(dev, act, with_root, with_skip):
    width, relations, kind = 24, 3, "edge"
    b = _batch(kind)
    cm = _prepared(kind, dev)
    pr, skip, _, _ = _case(kind, width, relations)
    args = (pr[:, :relations * width], pr[:, relations * width:] if with_root else None, skip if with_skip else None, act, b.coo,
            _types(kind, relations), relations)
    ref, base = U.rgcn_ref(*args), U.rgcn_ref(*args, dtype=np.float32)
    got = _stage(cm, _rec(kind, relations, dev), pr, width, relations, dev, root=with_root, skip=skip if with_skip else None, act=act)
    cm.check()
    record_classes(f"aggregate_rgcn/epilogue-{act}" + ("" if with_root else "-noroot") + ("" if with_skip else "-noskip"),
                   got.cpu().numpy(), ref, base, b.coo)


# ---------------------------------------------------------------------------------------------------- 7. one relation: the mean
@pytest.mark.parametrize("kind", ["edge", "sweep"])
@pytest.mark.parametrize("width", [32, 9])
def test_one_relation_without_root_is_the_mean_aggregate(dev, width, kind):
    b = _batch(kind)
    cm = _prepared(kind, dev)
    pr, _, _, _ = _case(kind, width, 1)
    p = np.ascontiguousarray(pr[:, :width])
    got = cm.aggregate_rgcn(_rec(kind, 1, dev), _t(p, dev), 1)
    cm.check()
    record_classes(f"aggregate_rgcn/mean-{kind}-w{width}", got.cpu().numpy(), R.mean_agg64(p, b.coo), R.mean_agg64(p, b.coo, dtype=np.float32), b.coo)


# ---------------------------------------------------------------------------------------------------- 8. the bits
@pytest.mark.parametrize("width", [32, 9, 130])
def test_a_repeat_launch_and_another_grid_give_the_same_bits(dev, width):
    relations, kind = 3, "sweep"
    b = _batch(kind)
    cm = _prepared(kind, dev)
    rec = _rec(kind, relations, dev)
    pr, skip, _, _ = _case(kind, width, relations)
    first = _stage(cm, rec, pr, width, relations, dev, skip=skip, act="tanh")
    assert torch.equal(_stage(cm, rec, pr, width, relations, dev, skip=skip, act="tanh"), first)
    big = _workspace(b, slack=3)  # (another capacity: other tile tables; the rows' steps fall to other workgroups)
    _prep(big, b, dev)
    rec3 = big.rgcn_slots(_t(_types(kind, relations), dev), relations)
    assert torch.equal(rec3, rec)
    assert torch.equal(_stage(big, rec3, pr, width, relations, dev, skip=skip, act="tanh"), first)
    cm.check()
    big.check()


# ---------------------------------------------------------------------------------------------------- 9. whole models
def _model_batch(graphs, in_dim, seed):
    """``graphs`` synthetic qm9-like graphs with seeded features of width ``in_dim``; a graph with explicit self loops, an empty
    and a one-node graph among them"""
    mols, rng = synthetic.make_batch("qm9", graphs, seed=seed), np.random.default_rng(seed)
    gs = [(rng.uniform(-1, 1, (mols.graph(g)[0].shape[0], in_dim)).astype(np.float32), mols.graph(g)[1]) for g in range(graphs)]
    return pack_graphs(gs[:graphs // 2] + [EMPTY(in_dim), looped_graph(40, in_dim, seed), ONE(in_dim)] + gs[graphs // 2:] + [EMPTY(in_dim)])


def _model(layers, in_dim=9, hidden=33, out_dim=32, relations=4, skip=True, act="relu", pools=("add", "mean", "max"), seed=0):
    return U.make_rgcn_model(in_dim=in_dim, hidden=hidden, layers=layers, out_dim=out_dim, relations=relations, skip=skip, act=act,
                             pools=pools, mlp_layers=1, out_act=torch.nn.LogSoftmax, seed=seed)


def _compiled(model, b, ingest=False):
    cm = runtime.CompiledModel.from_model(model, b.num_graphs, b.num_nodes, b.num_edges)
    if ingest:  # (right after construction: before a batch is prepared on the workspace)
        cm.enable_type_ingest()
    return cm


def _shuffled(b, types, seed):
    """The batch's edges in a shuffled order, as a PyG loader may hold them, with types CORRELATED with the input position (so
    that types left in input order, or permuted the wrong way, give another result): (edge_index int64 [2, E], input types int64
    [E], the host ingest's batch and its types in COO row order)."""
    perm = np.random.default_rng(seed).permutation(b.num_edges)
    ei = np.ascontiguousarray(b.coo[perm].T.astype(np.int64))
    t_in = ((np.arange(b.num_edges) * 4) // max(b.num_edges, 1)).astype(np.int64)  # quarter of the input position
    hb, t_ord = gnnb.from_pyg_batch(b.x, ei, batch=batch_vector(b), num_graphs=b.num_graphs, edge_type=t_in)
    return ei, t_in, hb, t_ord


# (layers, skip, act, pools, in_dim, hidden, out_dim): widths 9 -> 33 -> 32 and 4 -> 128
MODELS = [(3, True, "relu", ("add", "mean", "max"), 9, 33, 32), (3, False, "tanh", ("mean",), 9, 33, 32), (2, True, "gelu", ("mean", "max"), 9, 33, 32),
          (1, True, "sigmoid", ("add",), 4, 128, 128), (2, False, "relu", ("max",), 4, 128, 128)]


@pytest.mark.parametrize("layers,skip,act,pools,in_dim,hidden,out_dim", MODELS)
def test_whole_models_against_float64(dev, layers, skip, act, pools, in_dim, hidden, out_dim):
    graphs, relations = 24, 4
    model = _model(layers, in_dim, hidden, out_dim, relations, skip, act, pools, seed=layers + in_dim)
    b0 = _model_batch(graphs, in_dim, seed=31 + layers)
    ei_np, t_in, b, t_ord = _shuffled(b0, None, seed=layers)
    assert b.num_graphs == graphs + 4 and (b.coo[:, 0] == b.coo[:, 1]).sum() >= 10  # explicit self loops
    assert not np.array_equal(b.coo, ei_np.T) and len(set(t_ord.tolist())) == relations  # the ingest must sort; every relation occurs
    cm = _compiled(model, b, ingest=True)
    lib = cm.lib
    assert lib.gnnb_model_rgcn_relations(cm._model) == relations and lib.gnnb_model_ggnn_steps(cm._model) == 0
    assert lib.gnnb_model_is_resgated(cm._model) == 0 and lib.gnnb_model_edge_dim(cm._model) == 0
    xd, cood, nptr, eptr = to_dev(b, dev)
    td = _t(t_ord, dev)
    out = cm.forward_types(xd, td, cood, nptr, eptr)
    cm.check()
    assert cm.last_path() == "layerwise" and out.shape == (b.num_graphs, 19)
    ref, base = U.forward64(model, b, b.x, t_ord), U.run(model, b, b.x, t_ord)
    entry = f"forward_types/rgcn-L{layers}-{'skip' if skip else 'noskip'}-{act}-in{in_dim}-d{hidden}"
    record(entry, out.cpu().numpy(), ref, base)
    # types that did not follow their edges give another reference: the comparison above would see it
    wrong = U.forward64(model, b, b.x, np.sort(t_ord))
    assert np.abs(wrong - ref).max() > 1e-4 * np.abs(ref).max()
    # the same forward again, and the prepared form, give the same bits (no atomics, a fixed summation order)
    assert torch.equal(cm.forward_types(xd, td, cood, nptr, eptr), out)
    cm.graph_prep(cood, nptr, eptr, b.num_nodes)
    assert torch.equal(cm.forward_prepared_types(xd, td), out)
    # ... and so does the PyG mini-batch from a shuffled device edge_index + its int64 types (the ingest's arrays are the host's)
    ei, ti = _t(ei_np, dev), _t(t_in, dev)
    coo_i, _, _, t_i = cm.ingest_pyg_types(ei, ti, batch=_t(batch_vector(b), dev), num_graphs=b.num_graphs)
    assert t_i.dtype == torch.int32 and np.array_equal(t_i.cpu().numpy(), t_ord) and np.array_equal(coo_i.cpu().numpy(), b.coo)
    pyg = cm.forward_pyg_types(xd, ei, ti, batch=_t(batch_vector(b), dev), num_graphs=b.num_graphs)
    cm.check()
    assert cm.last_path() == "layerwise"
    record(entry + "-pyg", pyg.cpu().numpy(), ref, base)
    assert torch.equal(pyg, out)
    assert torch.equal(cm.forward_pyg_types(xd, ei, ti, ptr=_t(b.node_ptr.astype(np.int64), dev)), out)


def test_the_ingest_narrows_types_that_do_not_fit(dev):
    model = _model(1)
    b = _model_batch(8, 9, seed=3)
    cm = _compiled(model, b, ingest=True)
    ei = _t(np.ascontiguousarray(b.coo.T.astype(np.int64)), dev)
    t = np.zeros(b.num_edges, np.int64)
    t[1], t[2], t[3] = 2 ** 31, -(2 ** 40), 3
    _, _, _, t_i = cm.ingest_pyg_types(ei, _t(t, dev), batch=_t(batch_vector(b), dev), num_graphs=b.num_graphs)
    got = t_i.cpu().numpy()
    cm.check()  # (the ingest flags nothing: the slot pass does)
    assert got[1] == -1 and got[2] == -1 and got[3] == 3 and (np.delete(got, [1, 2, 3]) == 0).all()
    out = cm.forward_pyg_types(_t(b.x, dev), ei, _t(t, dev), batch=_t(batch_vector(b), dev), num_graphs=b.num_graphs)
    with pytest.raises(runtime.GnnbError, match="flags 0x100"):
        cm.check()
    assert torch.isfinite(out).all()


# ---------------------------------------------------------------------------------------------------- 10. degenerate batches
def test_empty_and_one_node_batches(dev):
    model = _model(2, seed=4)
    # a batch without a node: the stage entries launch nothing and read no operand
    b = pack_graphs([EMPTY(9)])
    cm = _workspace(b, slack=3)
    _prep(cm, b, dev)
    rec = cm.rgcn_slots(None, 4)
    got = cm.aggregate_rgcn(rec, torch.empty((0, 4 * 32), device=dev), 4, root=torch.empty((0, 32), device=dev), act="tanh")
    cm.check()
    assert rec.shape == (0, 2) and got.shape == (0, 32)
    for name, graphs in (("one", [ONE(9)]), ("no-edges", [ONE(9), EMPTY(9), ONE(9)])):
        b = pack_graphs(graphs)
        assert b.num_edges == 0
        cm = runtime.CompiledModel.from_model(model, max(b.num_graphs, 1), max(b.num_nodes, 1), 4)
        cm.enable_type_ingest()
        xd, cood, nptr, eptr = to_dev(b, dev)
        t = np.zeros(0, np.int32)
        out = cm.forward_types(xd, None, cood, nptr, eptr)  # E = 0: NULL types
        cm.check()
        assert torch.equal(cm.forward_types(xd, _t(t, dev), cood, nptr, eptr), out)
        assert torch.equal(cm.forward_prepared_types(xd, None), out)
        ei = torch.zeros((2, 0), dtype=torch.int64, device=dev)
        assert torch.equal(cm.forward_pyg_types(xd, ei, None, batch=_t(batch_vector(b), dev), num_graphs=b.num_graphs), out)
        cm.check()
        record(f"forward_types/rgcn-{name}", out.cpu().numpy(), U.forward64(model, b, b.x, t), U.run(model, b, b.x, t))
        # the stage entries on such a batch launch nothing
        rec = cm.rgcn_slots(None, 4)
        assert rec.shape == (0, 2)
        cm.check()


# ---------------------------------------------------------------------------------------------------- 11. stale records
def test_one_workspace_rebuilds_its_records_for_every_batch(dev):
    model = _model(2, seed=8)
    b = _model_batch(16, 9, seed=41)
    ta, tb = U.edge_types(b, 4, seed=1), U.edge_types(b, 4, seed=2)
    assert (ta != tb).mean() > 0.5
    xd, cood, nptr, eptr = to_dev(b, dev)
    fresh = []
    for t in (ta, tb):
        cm = _compiled(model, b)
        fresh.append(cm.forward_types(xd, _t(t, dev), cood, nptr, eptr))
        cm.check()
    assert not torch.equal(fresh[0], fresh[1])
    cm = _compiled(model, b)
    for i, t in enumerate((ta, tb, ta)):
        assert torch.equal(cm.forward_types(xd, _t(t, dev), cood, nptr, eptr), fresh[i % 2]), i
    # ... and the prepared form on the tables left there
    assert torch.equal(cm.forward_prepared_types(xd, _t(tb, dev)), fresh[1])
    cm.check()
    record("forward_types/rgcn-stream", fresh[1].cpu().numpy(), U.forward64(model, b, b.x, tb), U.run(model, b, b.x, tb))


# ---------------------------------------------------------------------------------------------------- 12. a captured forward
def test_a_captured_forward_pyg_types_replays_with_the_eager_bits(dev):
    model = _model(3, seed=6)
    b0 = _model_batch(12, 9, seed=24)
    ei_np, t_in, b, t_ord = _shuffled(b0, None, seed=9)
    cm = _compiled(model, b, ingest=True)
    xd, ei, ti, bd = _t(b.x, dev), _t(ei_np, dev), _t(t_in, dev), _t(batch_vector(b), dev)
    eager = cm.forward_pyg_types(xd, ei, ti, batch=bd, num_graphs=b.num_graphs).clone()  # (also the warm-up outside the capture)
    out = torch.zeros_like(eager)
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):  # (one stream, no parallel branches)
        cm.forward_pyg_types(xd, ei, ti, batch=bd, num_graphs=b.num_graphs, out=out)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    record("forward_pyg_types/rgcn-captured", out.cpu().numpy(), U.forward64(model, b, b.x, t_ord), U.run(model, b, b.x, t_ord))
    cm.check()


# ---------------------------------------------------------------------------------------------------- 13. refusals
def test_refusals(dev):
    model = _model(2)
    b = _model_batch(12, 9, seed=25)
    t = U.edge_types(b, 4, seed=3)
    cm = _compiled(model, b, ingest=True)
    xd, cood, nptr, eptr = to_dev(b, dev)
    td = _t(t, dev)
    good = cm.forward_types(xd, td, cood, nptr, eptr).clone()
    ei, batch_dev = _t(np.ascontiguousarray(b.coo.T.astype(np.int64)).reshape(2, -1), dev), _t(batch_vector(b), dev)
    ea = torch.zeros((b.num_edges, 3), device=dev)
    q = lambda v: v.data_ptr()  # noqa: E731
    B, N, E = b.num_graphs, b.num_nodes, b.num_edges
    lib, chk = cm.lib, runtime._check
    # every whole-model entry of gnnb_hip.h, gnnb_order.h and gnnb_edge.h refuses the model and names the _types entry
    for call, name in (
            (lambda: lib.gnnb_forward_batched(cm._model, cm._ws, q(xd), q(cood), q(nptr), q(eptr), B, N, E, q(good), None), "gnnb_forward_batched_types"),
            (lambda: lib.gnnb_forward_prepared(cm._model, cm._ws, q(xd), q(good), None), "gnnb_forward_prepared_types"),
            (lambda: lib.gnnb_forward_prepared_prep_next(cm._model, cm._ws, q(xd), q(good), cm._ws, q(cood), q(nptr), q(eptr), B, N, E, None),
             "gnnb_forward_prepared_types"),
            (lambda: lib.gnnb_forward_batched_host(cm._model, cm._ws, b.x.ctypes.data, b.coo.ctypes.data, b.node_ptr.ctypes.data,
                                                   b.edge_ptr.ctypes.data, B, N, E, b.x.ctypes.data), "gnnb_forward_batched_types"),
            (lambda: lib.gnnb_forward_pyg(cm._model, cm._ws, q(xd), q(ei), q(batch_dev), None, B, N, E, q(good), None), "gnnb_forward_pyg_types"),
            (lambda: lib.gnnb_forward_pyg_ordered(cm._model, cm._ws, q(xd), q(ei), q(batch_dev), None, B, N, E, q(good), None), "gnnb_forward_pyg_types"),
            (lambda: lib.gnnb_forward_batched_edges(cm._model, cm._ws, q(xd), q(ea), q(cood), q(nptr), q(eptr), B, N, E, q(good), None),
             "gnnb_forward_batched_types"),
            (lambda: lib.gnnb_forward_prepared_edges(cm._model, cm._ws, q(xd), q(ea), q(good), None), "gnnb_forward_prepared_types"),
            (lambda: lib.gnnb_forward_pyg_edges(cm._model, cm._ws, q(xd), q(ei), q(ea), q(batch_dev), None, B, N, E, q(good), None),
             "gnnb_forward_pyg_types"),
            (lambda: lib.gnnb_gcn_stack_timed(cm._model, cm._ws, q(xd), 1, None, C_FLOAT()), "gnnb_forward_prepared_types")):
        with pytest.raises(runtime.GnnbError, match="RGCNConv.*" + name):
            chk(call())
    with pytest.raises(runtime.GnnbError):
        cm.forward(xd, cood, nptr, eptr)
    # the _types entries refuse every other model; the type ingest refuses its workspace
    gin_model = gnnb.GNNModel(9, None, 33, 2, 32, gnnb.GINConv_GNNB, torch.nn.ReLU, True, gnnb.GlobalPooling(["add", "mean", "max"]),
                              gnnb.MLP(96, 19, 64, 1), torch.nn.LogSoftmax).eval()
    gin = runtime.CompiledModel.from_model(gin_model, B, N, E)
    assert bytes(gin.desc) == bytes(cm.desc) and lib.gnnb_model_rgcn_relations(gin._model) == 0
    with pytest.raises(runtime.GnnbError, match="RGCNConv model"):
        gin.forward_types(xd, td, cood, nptr, eptr)
    with pytest.raises(runtime.GnnbError, match="RGCNConv model"):
        gin.enable_type_ingest()
    with pytest.raises(runtime.GnnbError, match="gnnb_rgcn_model_create"):
        chk(lib.gnnb_forward_batched_types(gin._model, gin._ws, q(xd), q(td), q(cood), q(nptr), q(eptr), B, N, E, q(good), None))
    with pytest.raises(runtime.GnnbError, match="without relations"):
        chk(lib.gnnb_workspace_enable_type_ingest(gin._ws))
    gin.enable_ingest()
    with pytest.raises(runtime.GnnbError, match="gnnb_rgcn_model_create"):
        chk(lib.gnnb_forward_pyg_types(gin._model, gin._ws, q(xd), q(ei), q(ei), q(batch_dev), None, B, N, E, q(good), None))
    # a model runs neither on a workspace of another relation count, nor on a GIN model's of the same description, nor a GIN model on its
    other = _compiled(_model(2, relations=3), b)
    assert bytes(other.desc) == bytes(cm.desc)  # (the same description: only the relations tell them apart)
    other.graph_prep(cood, nptr, eptr, N)
    gin.graph_prep(cood, nptr, eptr, N)
    for ws in (other._ws, gin._ws):
        with pytest.raises(runtime.GnnbError, match="different model"):
            chk(lib.gnnb_forward_prepared_types(cm._model, ws, q(xd), q(td), q(good), None))
    with pytest.raises(runtime.GnnbError, match="RGCNConv.*gnnb_forward_prepared_types"):  # (the workspace is an RGCNConv model's)
        chk(lib.gnnb_forward_prepared(gin._model, cm._ws, q(xd), q(good), None))
    # before its enable, and with operands of the wrong kind
    plain = _compiled(model, b)
    with pytest.raises(runtime.GnnbError, match="enable_type_ingest"):
        plain.forward_pyg_types(xd, ei, td.long(), batch=batch_dev, num_graphs=B)
    for bad, what in ((td.long(), "torch.int32"), (td[:-1], "edge_type must be"), (td.cpu(), "CUDA"), (None, "required")):
        with pytest.raises(runtime.GnnbError, match=what):
            cm.forward_types(xd, bad, cood, nptr, eptr)
    with pytest.raises(runtime.GnnbError, match="torch.int64"):
        cm.forward_pyg_types(xd, ei, td, batch=batch_dev, num_graphs=B)
    with pytest.raises(runtime.GnnbError, match="NULL"):
        chk(lib.gnnb_forward_batched_types(cm._model, cm._ws, q(xd), None, q(cood), q(nptr), q(eptr), B, N, E, q(good), None))
    # the stage entries on a GCN workspace: its tables have dropped the (v, v) edges
    z = lambda *shape: torch.zeros(shape, device=dev)  # noqa: E731
    zi = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)  # noqa: E731
    gcn = _workspace(b, conv="gcn")
    _prep(gcn, b, dev)
    with pytest.raises(runtime.GnnbError, match="explicit self loops"):
        gcn.rgcn_slots(td, 4)
    with pytest.raises(runtime.GnnbError, match="explicit self loops"):
        gcn.aggregate_rgcn(zi(E, 2), z(N, 96), 3)
    gcn.check()
    # the stage entries check their operands on the host, before any launch
    cm.graph_prep(cood, nptr, eptr, N)
    for rel in (0, 9, True, 2.0):
        with pytest.raises(runtime.GnnbError, match="relations must be"):
            cm.rgcn_slots(td, rel)
    for bad, what in ((td.long(), "torch.int32"), (td[:-1], r"edge_type must be"), (td.cpu(), "CUDA"), (None, "required")):
        with pytest.raises(runtime.GnnbError, match=what):
            cm.rgcn_slots(bad, 4)
    with pytest.raises(runtime.GnnbError, match="at most 256"):
        cm.aggregate_rgcn(zi(E, 2), z(N, 2 * 257), 2)
    for bad, what in ((dict(p=z(N, 95)), "relations \\* width"), (dict(p=z(N - 1, 96)), "p "), (dict(rec=zi(E - 1, 2)), "rec must be"),
                      (dict(rec=zi(E, 2).long()), "rec must be"), (dict(rec=zi(E + 1, 2).view(-1)[1:2 * E + 1].view(E, 2)), "8-byte"),
                      (dict(root=z(N, 33)), "root must be"), (dict(root=z(N - 1, 32)), "root "), (dict(skip=z(N, 16)), "skip has shape"),
                      (dict(skip=z(N - 1, 32)), "skip must be"), (dict(out=z(N, 16)), "out"), (dict(act="swish"), "act must be"),
                      (dict(p=z(N, 96).double()), "p "), (dict(p=z(N, 96).cpu()), "p "), (dict(relations=9), "relations must be")):
        args = dict(rec=zi(E, 2), p=z(N, 96), relations=3)
        args.update(bad)
        with pytest.raises(runtime.GnnbError, match=what):
            cm.aggregate_rgcn(args.pop("rec"), args.pop("p"), args.pop("relations"), **args)
    # ... and the C entries themselves
    x, r = z(N, 4 * 260), zi(E + 1, 2)

    def call(rec=q(r), p=q(x), ldp=96, relations=3, root=None, ldr=0, act=4, out=q(x), width=32):
        return lib.gnnb_aggregate_rgcn(cm._ws, rec, p, ldp, relations, root, ldr, None, act, out, width, None)

    for kw in (dict(ldp=771, relations=3, width=257), dict(width=0), dict(relations=0), dict(relations=9, ldp=9 * 32), dict(ldp=95),
               dict(root=q(x), ldr=31), dict(p=None), dict(out=None), dict(rec=None), dict(rec=q(r) + 4), dict(act=5), dict(act=-1)):
        with pytest.raises(runtime.GnnbError, match="bad argument to gnnb_aggregate_rgcn"):
            chk(call(**kw))
    for kw in (dict(relations=0), dict(relations=9), dict(t=None), dict(rec=None), dict(rec=q(r) + 4)):
        a = dict(t=q(td), relations=4, rec=q(r))
        a.update(kw)
        with pytest.raises(runtime.GnnbError, match="bad argument to gnnb_rgcn_slots"):
            chk(lib.gnnb_rgcn_slots(cm._ws, a["t"], a["relations"], a["rec"], None))
    # nothing above left a flag or changed a result
    cm.check()
    assert torch.equal(cm.forward_types(xd, td, cood, nptr, eptr), good)


def C_FLOAT():
    import ctypes as C
    return C.byref(C.c_float())
