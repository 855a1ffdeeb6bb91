"""One workspace across a stream of unlike batches on the MI355X, every conv family (``tests/workspace_life_util.py``).

A ``CompiledModel`` that lives for a whole sequence sees batches whose graph, node and edge counts go up and down, through every
entry point in turn, with the setters called between batches; after every forward one stage entry of the family runs on the
prepared batch into an output pre-filled with NaN.  Every step is held (a) to the bits of a FRESH object of the same capacities,
options and promises that runs the batch through the plain ``forward`` / ``forward_edges`` -- output, ``last_path``, the tables
read back, the stage result, a refusal's text -- and (b) to float64 by ``ref64.budget`` with the project's K = 4, F = 2^-22
(the stage result per in-degree class, ``gine_util.budget_by_degree``).  No tolerance of this file's own; nothing is left out of
a comparison.  References: the family's whole-model ones (the model's torch definition on a ``.double()`` copy; ``base`` the same
in fp32) and its stage restatement.  pna / pnae run on grid features under seeds chosen on the CPU, and the float64 reference
alone is asserted to keep every variance clear of PyG's 1e-5.

Sections: a. sizes up and down, b. routes and promises changing under one workspace, c. two alternating workspaces with
``forward_prepared_prep_next``, d. a captured forward between unlike eager ones, e. setters between ``graph_prep`` and the
prepared forward (they speak of the NEXT prep: ``include/gnnb_hip.h``).  Worst e / e32 per family and sequence go to
GNNB_FP64_REPORT=<file>."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import gatv2_util
import ref64 as R
import workspace_life_util as W
from gnnbuilder_amd import runtime, synthetic
from gnnbuilder_amd.batching import order_large_last
from helpers import batch_vector, edge_batch, to_dev

pytestmark = pytest.mark.gpu

WORST = {}
ORDERED_FAMILIES = ("gcn", "gin", "sage", "pna")  # (the ordered ingest serves the stack kernels' promise; the others refuse it)


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


def _recorder(prefix):
    def record(key, r):
        WORST[f"{prefix}/{key}"] = max(WORST.get(f"{prefix}/{key}", 0.0), r)
    return record


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _host(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())


# ---------------------------------------------------------------------------------------------------- the object under test
def _stage_call(cm, family, c, dev, out):
    """The family's stage entry on the prepared batch, operands ``c`` (``workspace_life_util.stage_operands``)."""
    d = lambda k: None if c[k] is None or (k in ("ea", "edge_attr") and len(c[k]) == 0) else _t(c[k], dev)  # noqa: E731
    if family in ("gcn", "gin", "sage"):
        return cm.aggregate({"gcn": "gcn", "gin": "sum", "sage": "mean"}[family], d("x"), eps=W.STAGE_EPS if family == "gin" else 0.0, out=out)
    if family == "pna":
        return cm.aggregate("pna", d("x"), self_term=d("q"), out=out)
    if family == "gine":
        return cm.aggregate_edges_fused(d("x"), d("ea"), d("we"), d("be"), eps=W.STAGE_EPS, out=out)
    if family == "pnae":
        return cm.aggregate_pna_edges(d("p"), d("q"), d("ea"), d("we"), d("be"), out=out)
    if family == "gatv2":
        return cm.aggregate_gatv2(d("xl"), d("xr"), d("att"), bias=d("bias"), heads=W.HEADS, negative_slope=gatv2_util.SLOPE, out=out)
    if family == "gatv2e":
        return cm.aggregate_gatv2_edges(d("xl"), d("xr"), d("att"), d("edge_attr"), d("w_edge"), bias=d("bias"), heads=W.HEADS,
                                        negative_slope=gatv2_util.SLOPE, out=out)
    if family == "transformer":
        return cm.aggregate_transformer(d("q"), d("k"), d("v"), root=d("root"), heads=W.HEADS, scale=c["scale"], out=out)
    if family == "transformere":
        return cm.aggregate_transformer_edges(d("q"), d("k"), d("v"), d("qe"), d("edge_attr"), d("w_edge"), root=d("root"), heads=W.HEADS,
                                              scale=c["scale"], out=out)
    if family == "resgated":
        return cm.aggregate_resgated(d("k"), d("q"), d("v"), root=d("root"), out=out)
    if family == "resgatede":
        return cm.aggregate_resgated_edges(d("k"), d("q"), d("v"), d("edge_attr"), d("w_gate"), d("w_value"), root=d("root"), out=out)
    if family == "gat":
        return cm.aggregate_gat(d("xl"), d("s_src"), d("s_dst"), bias=d("bias"), heads=W.HEADS, negative_slope=gatv2_util.SLOPE, out=out)
    if family == "gate":
        return cm.aggregate_gat_edges(d("xl"), d("s_src"), d("s_dst"), d("edge_attr"), d("a_edge"), bias=d("bias"), heads=W.HEADS,
                                      negative_slope=gatv2_util.SLOPE, out=out)
    assert family == "ggnn", family
    return cm.aggregate_ggnn(d("p"), d("gh"), d("h"), b_ih=d("b_ih"), out=out)


class Runner:
    """One ``CompiledModel`` and what a step does to it.  ``settings``: the promises and the large segment as the setters leave
    them ({"set_max_graph_nodes": (n,), ...}); ``options``: process-wide options held while this object runs."""

    def __init__(self, family, model, caps, dev, settings=None, addons=True, options=None):
        self.family, self.model, self.caps, self.dev = family, model, caps, dev
        self.edges = family in W.EDGE_FAMILIES
        self.options = dict(options or {})
        self.cm = runtime.CompiledModel.from_model(model, *caps)
        if addons:  # every ingest add-on the family has, right after construction
            if self.edges:
                self.cm.enable_edge_ingest()
            else:
                self.cm.enable_ingest()
                if family in ORDERED_FAMILIES:
                    self.cm.enable_ordered_ingest()
        self.settings = {}
        for name, args in (settings or {}).items():
            self.apply(name, args)

    def apply(self, name, args):
        getattr(self.cm, name)(*args)
        self.settings[name] = tuple(args)

    def _forward(self, step, entry):
        cm, dev, b, ea = self.cm, self.dev, step.batch, step.edge_attr
        x = _t(b.x, dev)
        ead = None if ea is None or len(ea) == 0 else _t(ea, dev)
        idx = (_t(b.coo, dev), _t(b.node_ptr, dev), _t(b.edge_ptr, dev))
        if entry == "forward":
            return cm.forward_edges(x, ead, *idx) if self.edges else cm.forward(x, *idx)
        if entry == "prepared":
            cm.graph_prep(*idx, b.num_nodes)
            return cm.forward_prepared_edges(x, ead) if self.edges else cm.forward_prepared(x)
        if entry == "host":
            return torch.from_numpy(cm.forward_host(b.x, b.coo, b.node_ptr, b.edge_ptr))
        ei, ea_in = step.pyg if step.pyg is not None else W.grouped_mini_batch(b, ea)
        eid = _t(ei, dev)
        kw = dict(batch=_t(batch_vector(b), dev), num_graphs=b.num_graphs) if entry in ("pyg_batch", "ordered") else dict(ptr=_t(b.node_ptr.astype(np.int64), dev))
        if entry == "ordered":
            return cm.forward_pyg_ordered(x, eid, **kw)
        assert entry in ("pyg_batch", "pyg_ptr"), entry
        if self.edges:
            return cm.forward_pyg_edges(x, eid, None if ea_in is None or len(ea_in) == 0 else _t(ea_in, dev), **kw)
        return cm.forward_pyg(x, eid, **kw)

    def run(self, step, entry=None):
        """The step on this object -> its result (``workspace_life_util`` module docstring).  ``entry`` overrides the step's."""
        cm, dev = self.cm, self.dev
        for k, v in self.options.items():
            runtime.set_option(k, v)
        try:
            res = {}
            try:
                res["out"] = _host(self._forward(step, entry or step.entry))
                res["path"] = cm.last_path()
            except runtime.GnnbError as e:
                # an entry that refuses this batch refuses it on every object alike; the batch is prepared for what follows
                res["refused"] = str(e)
                tb = step.tables_batch
                cm.graph_prep(_t(tb.coo, dev), _t(tb.node_ptr, dev), _t(tb.edge_ptr, dev), tb.num_nodes)
            cm.check()
            tb = step.tables_batch
            if step.tables:
                row_ptr, col, in_deg = cm.tables_to_host()
                res["tables"] = (row_ptr.copy(), col.copy(), in_deg.copy(), cm.edge_index_table_to_host().copy())
            if step.stage is not None:
                wide = 4 * W.STAGE_W if self.family in ("pna", "pnae") else W.STAGE_W
                out = torch.full((tb.num_nodes, wide), float("nan"), dtype=torch.float32, device=dev)
                try:
                    got = _stage_call(cm, self.family, step.stage, dev, out)
                    assert got.data_ptr() == out.data_ptr()
                    res["stage"] = _host(got)
                except runtime.GnnbError as e:
                    res["stage_refused"] = str(e)
                cm.check()
            return res
        finally:
            for k in self.options:
                runtime.set_option(k, OPTION_DEFAULTS[k])


OPTION_DEFAULTS = {"pna_classes": 1}  # the process-wide defaults of the options this file sets (gnnb_runtime.hip options())


class Fresh:
    """``run_fresh``: per step a new object of the same capacities, options and promises -- the settings as the long-lived
    object's setters have left them by that step -- that runs the batch through the plain ``forward`` / ``forward_edges``.  The
    ordered entry's host form: ``batching.order_large_last`` at the promise, the segment set to its triple (removed when nothing
    is large), ``forward`` on the ordered batch, the rows put back."""

    def __init__(self, family, model, caps, dev, options=None):
        self.args, self.options, self.settings = (family, model, caps, dev), options, {}

    def __call__(self, step):
        for name, args in step.setters:
            self.settings[name] = tuple(args)
        plain = step
        if step.entry == "ordered":
            ordered, perm, triple = step.ordered
            self.settings["set_large_segment"] = triple if triple[0] < ordered.num_graphs else ()
            plain = dataclasses.replace(step, batch=ordered, ordered=None)
        runner = Runner(*self.args, settings=self.settings, addons=False, options=self.options)
        res = runner.run(plain, entry="forward")
        if step.entry == "ordered" and "out" in res:
            res["out"] = np.ascontiguousarray(res["out"][np.argsort(perm)])
        return res


def _long(runner):
    def run_long(step):
        for name, args in step.setters:
            runner.apply(name, args)
        return runner.run(step)
    return run_long


class References:
    """``reference(step)`` of the driver, each batch's computed once."""

    def __init__(self, family, model):
        self.family, self.model, self.cache = family, model, {}

    def __call__(self, step):
        key = id(step)
        if key not in self.cache:
            refs = {"out": W.model_refs(self.family, self.model, step.batch, step.edge_attr)}
            if step.stage is not None:
                refs["stage"] = W.stage_refs(self.family, step.tables_batch, step.stage)
            self.cache[key] = (step, refs)  # (the step is kept: its id stays its own)
        return self.cache[key][1]


def _assert_everything_ran(steps, results):
    """Only a batch without a node may be refused (its empty ``x`` has no address; on both objects alike, (a)): every other step
    has an output and, where it has a stage entry, a stage result in which no row of the NaN-filled output was skipped."""
    for step, res in zip(steps, results):
        if step.batch.num_nodes > 0:
            assert "out" in res and res["out"].shape == (step.batch.num_graphs, 19), (step.name, sorted(res))
            if step.stage is not None:
                assert not np.isnan(res["stage"]).any(), step.name


def _assert_pna_references_are_clear(family, model, steps):
    if family in ("pna", "pnae"):
        for s in steps:  # on the float64 reference alone, nothing excluded
            assert W.variances_near_the_threshold(model, s.batch, s.batch.x, s.edge_attr) == 0, s.name


# ---------------------------------------------------------------------------------------------------- a. sizes up and down
PLAIN_ENTRIES = ("forward", "prepared", "pyg_batch", "pyg_ptr", "host", "forward", "prepared", "pyg_batch")
EDGE_ENTRIES = ("forward", "prepared", "pyg_batch", "pyg_ptr", "pyg_batch", "forward", "prepared", "pyg_ptr")
SHUFFLED = (2, 4, 6)  # steps whose mini-batch comes with its edges (and attribute rows) under a permutation across graphs


def _sizes_steps(family, hidden=32, layers=2, entries=None, stage=True):
    model, batches, attrs = W.family_sequence(family, hidden, layers)
    entries = entries or (EDGE_ENTRIES if family in W.EDGE_FAMILIES else PLAIN_ENTRIES)
    steps = []
    for i, (name, b, ea, entry) in enumerate(zip(W.SIZES_UP_AND_DOWN, batches, attrs, entries)):
        mini = None
        if i in SHUFFLED and b.num_edges:  # (the tables are then built from the ingest's order: the step's batch is that one)
            b, ea, mini, _ = W.shuffled_mini_batch(b, ea, seed=500 + i)
        steps.append(W.Step(name, b, entry, edge_attr=ea, tables=True, pyg=mini if entry.startswith("pyg") else None,
                            stage=None if not stage else steps[0].stage if i == 7 else W.stage_operands(family, b, 700 + i),
                            same_as=0 if i == 7 else None))
    assert steps[7].batch is steps[0].batch and max(s.batch.num_nodes for s in steps) < 2000
    assert steps[5].batch.num_nodes == 0 and steps[3].batch.num_edges == 0 and steps[1].batch.num_nodes == 1
    hub = steps[2].batch
    assert np.bincount(hub.coo[:, 1]).max() >= 1200 and (hub.coo[:, 0] == hub.coo[:, 1]).any() and (np.diff(hub.node_ptr) == 0).any()
    return model, steps


def _run_sizes(dev, family, hidden, label):
    model, steps = _sizes_steps(family, hidden=hidden)
    _assert_pna_references_are_clear(family, model, steps)
    caps = W.capacities([s.batch for s in steps])
    long = Runner(family, model, caps, dev)
    results = W.run_sequence(steps, _long(long), Fresh(family, model, caps, dev), References(family, model), _recorder(f"workspace_life/sizes/{label}"))
    # what ran: every step but the node-less one has an output, on the route the family has without a promise
    _assert_everything_ran(steps, results)
    assert {r["path"] for r in results if "path" in r} == {"layerwise"}  # (the route every family has without a promise)
    long.cm.check()
    return steps


@pytest.mark.parametrize("family", W.FAMILIES)
def test_sizes_up_and_down(dev, family):
    """Eight batches on one workspace sized for the maxima of the sequence, the entry point rotating with the step; step 8 is step
    1 again and repeats its bits on the same object."""
    _run_sizes(dev, family, 32, family)


def test_sizes_up_and_down_ggnn_state_offset_moves(dev):
    """GatedGraphConv at hidden 9 with three steps per layer: the second state buffer lies ``roundup4(9 N)`` floats into the
    workspace's scratch, so with the sequence's node counts it moves from batch to batch, on and off a 16-byte boundary (which
    form a step's kernel takes follows from it), and both state buffers are written and read in turn in memory that the batch
    before carved differently.  The stage entry is the one of the test above, at width 32."""
    counts = [b.num_nodes for b in W.family_sequence("ggnn", hidden=9)[1]]
    assert len({(9 * n) % 4 for n in counts}) >= 3, counts  # (from the node counts alone, before anything runs)
    steps = _run_sizes(dev, "ggnn", 9, "ggnn-h9")
    assert [s.batch.num_nodes for s in steps] == counts


# ---------------------------------------------------------------------------------------------------- b. routes and promises
def _route_steps(family, model, promise):
    """gcn / gin: the stack kernel's promise on a hub-less batch, promise 0 on the hub batch, promise 29 with the ordered ingest on a
    ``molhiv_tail`` batch that holds graphs beyond 29 nodes, the ordered ingest on a batch with none (the segment is removed),
    plain ``forward`` again."""
    qm9 = W.with_features(synthetic.make_batch("qm9", 96, seed=11), W.IN_DIM, 11)
    hub = edge_batch(8, W.IN_DIM, seed=12)
    tail = W.with_features(synthetic.make_batch("molhiv_tail", 96, seed=13), W.IN_DIM, 13)
    small = W.with_features(synthetic.make_batch("qm9", 40, seed=14), W.IN_DIM, 14)
    sizes = np.diff(tail.node_ptr)
    assert 3 <= (sizes > 29).sum() < 96 and np.diff(qm9.node_ptr).max() <= 29 and np.diff(small.node_ptr).max() <= 29
    st = lambda b, i: W.stage_operands(family, b, 800 + i)  # noqa: E731
    o_tail, o_small = order_large_last(tail, 29), order_large_last(small, 29)
    assert o_tail[2][0] == int((sizes <= 29).sum()) and o_small[2][0] == small.num_graphs
    return [W.Step(f"qm9-96 promise {promise}", qm9, "forward", setters=(("set_max_graph_nodes", (promise,)),), tables=True, stage=st(qm9, 0)),
            W.Step("hub promise 0", hub, "prepared", setters=(("set_max_graph_nodes", (0,)),), tables=True, stage=st(hub, 1)),
            W.Step("molhiv_tail-96 promise 29 ordered", tail, "ordered", setters=(("set_max_graph_nodes", (29,)),), tables=True,
                   stage=st(o_tail[0], 2), ordered=o_tail),
            W.Step("qm9-40 ordered, none large", small, "ordered", tables=True, stage=st(o_small[0], 3), ordered=o_small),
            W.Step("qm9-96 forward", qm9, "forward", tables=True, stage=st(qm9, 4))]


@pytest.mark.parametrize("family,layers,stack,promise", [("gcn", 2, "stack_zf", 64), ("gin", 3, "stack", 61)])
def test_routes_change_under_one_workspace(dev, family, layers, stack, promise):
    """(k_gcn2_fused stages 64 rows, and a tile of at least 4 rows must fit beside the largest graph: 61 is the largest promise the
    GIN stack takes -- under 64 it runs layer by layer; k_gcn2_zf's stages hold 96 rows or more.)"""
    model = W.make_family_model(family, hidden=64, layers=layers, seed=1)
    steps = _route_steps(family, model, promise)
    caps = W.capacities([s.batch for s in steps])
    long = Runner(family, model, caps, dev)
    results = W.run_sequence(steps, _long(long), Fresh(family, model, caps, dev), References(family, model), _recorder(f"workspace_life/routes/{family}"))
    _assert_everything_ran(steps, results)
    paths = [r["path"] for r in results]
    assert paths == [stack, "layerwise", stack + "+large_layerwise", stack, stack], paths
    assert len(set(paths)) == 3
    long.cm.check()


# Seeds of the PNA route sequence (hidden 64: the degree-class form needs an output wider than 32), chosen on the CPU as PNA_SEEDS are
PNA_ROUTE_SEEDS = (2, (224, 217, 250, 231))


def _pna_route_batches():
    _, seeds = PNA_ROUTE_SEEDS
    return [W.with_features(synthetic.make_batch("qm9", 96, seed=seeds[0]), W.IN_DIM, seeds[0], grid=True),
            W.with_features(synthetic.make_batch("qm9", 40, seed=seeds[1]), W.IN_DIM, seeds[1], grid=True),
            W.with_features(synthetic.make_batch("molhiv", 40, seed=seeds[2]), W.IN_DIM, seeds[2], grid=True),
            W.with_features(synthetic.make_batch("qm9", 96, seed=seeds[0]), W.IN_DIM, seeds[3], grid=True)]


def test_pna_degree_promise_comes_and_goes(dev):
    """``set_max_degree(15)``, a batch of another size under it, 0, then 15 again, on batches of in-degree <= 8.  ``last_path`` says
    ``layerwise`` for both PNA forms, so which one ran is read from the bits (as ``test_hip_large_fp64.py`` does): under the
    promise they differ from the same forward with ``pna_classes = 0``, without it they are the same."""
    model = W.make_family_model("pna", hidden=64, layers=2, seed=PNA_ROUTE_SEEDS[0])
    a, b, c, d = _pna_route_batches()
    assert max(np.bincount(x.coo[:, 1]).max() for x in (a, b, c, d)) <= 8
    st = lambda x, i: W.stage_operands("pna", x, 900 + i)  # noqa: E731
    steps = [W.Step("qm9-96 degree 15", a, "forward", setters=(("set_max_degree", (15,)),), tables=True, stage=st(a, 0)),
             W.Step("qm9-40 degree 15", b, "prepared", tables=True, stage=st(b, 1)),
             W.Step("molhiv-40 degree 0", c, "pyg_ptr", setters=(("set_max_degree", (0,)),), tables=True, stage=st(c, 2)),
             W.Step("qm9-96 degree 15 again", d, "forward", setters=(("set_max_degree", (15,)),), tables=True, stage=st(d, 3))]
    _assert_pna_references_are_clear("pna", model, steps)
    caps = W.capacities([s.batch for s in steps])
    long = Runner("pna", model, caps, dev)
    results = W.run_sequence(steps, _long(long), Fresh("pna", model, caps, dev), References("pna", model), _recorder("workspace_life/routes/pna"))
    _assert_everything_ran(steps, results)
    general = Fresh("pna", model, caps, dev, options={"pna_classes": 0})
    for step, res, classes in zip(steps, results, (True, True, False, True)):
        same = np.array_equal(general(step)["out"].view(np.uint32), res["out"].view(np.uint32))
        assert same != classes, (step.name, "the degree-class form" if classes else "the general form", "did not run")
    long.cm.check()


def test_stream_k_tail_between_batches_of_unlike_rows(dev):
    """GraphSAGE at hidden 512: the second layer's GEMM has K = 1024, whose last round of tiles is cut along K (stream-K) on the
    workspace's own scratch.  Two batches of unlike M alternate; the arrival counters are back at zero and the guard region is
    whole after each."""
    model = W.make_family_model("sage", hidden=512, layers=2, seed=2)
    a = W.with_features(synthetic.make_batch("qm9", 96, seed=21), W.IN_DIM, 21)
    b = W.with_features(synthetic.make_batch("molhiv", 40, seed=22), W.IN_DIM, 22)
    assert abs(a.num_nodes - b.num_nodes) > 256
    steps = [W.Step(f"{'qm9-96' if i % 2 == 0 else 'molhiv-40'} #{i}", a if i % 2 == 0 else b, ("forward", "prepared", "pyg_batch", "forward")[i],
                    same_as=i - 2 if i >= 2 else None) for i in range(4)]
    caps = W.capacities([a, b])
    long = Runner("sage", model, caps, dev)
    run_long = _long(long)

    def guarded(step):
        res = run_long(step)
        long.cm.stream_k_guard()
        return res
    results = W.run_sequence(steps, guarded, Fresh("sage", model, caps, dev), References("sage", model), _recorder("workspace_life/stream_k/sage"))
    _assert_everything_ran(steps, results)
    assert all(r["path"] == "layerwise" for r in results)
    long.cm.check()


# ---------------------------------------------------------------------------------------------------- c. two alternating workspaces
class Pipeline:
    """``run_long`` over two alternating objects: step i's forward on one carries step i + 1's graph prep on the other
    (``forward_prepared_prep_next``); the last step is a plain ``forward_prepared``.  A forward that refuses its batch leaves the
    next batch's prep to a ``graph_prep`` call."""

    def __init__(self, family, model, caps, dev, steps, settings):
        self.pair = [Runner(family, model, caps, dev, settings=settings, addons=False) for _ in range(2)]
        self.steps, self.dev, self.i = steps, dev, 0
        b = steps[0].batch
        self.pair[0].cm.graph_prep(*to_dev(b, dev)[1:], b.num_nodes)

    def __call__(self, step):
        i, dev = self.i, self.dev
        assert step is self.steps[i]
        cur, nxt = self.pair[i & 1].cm, self.pair[(i + 1) & 1].cm
        nb = self.steps[i + 1].batch if i + 1 < len(self.steps) else None
        idx = None if nb is None else to_dev(nb, dev)[1:]
        res = {}
        try:
            x = _t(step.batch.x, dev)
            out = cur.forward_prepared(x) if nb is None else cur.forward_prepared_prep_next(x, nxt, *idx, nb.num_nodes)
            res["out"], res["path"] = _host(out), cur.last_path()
        except runtime.GnnbError as e:
            res["refused"] = str(e)
            if nb is not None:
                nxt.graph_prep(*idx, nb.num_nodes)
        cur.check()
        if step.tables:
            row_ptr, col, in_deg = cur.tables_to_host()
            res["tables"] = (row_ptr.copy(), col.copy(), in_deg.copy(), cur.edge_index_table_to_host().copy())
        self.i += 1
        return res


@pytest.mark.parametrize("family,hidden,promise,paths", [("gcn", 64, 64, {"stack_zf"}), ("transformer", 32, 64, {"layerwise"}),
                                                         ("gat", 32, 64, {"layerwise"}), ("ggnn", 32, 64, {"layerwise"})])
def test_two_alternating_workspaces(dev, family, hidden, promise, paths):
    """The sequence of a. through ``forward_prepared_prep_next`` under a promise of 64 nodes per graph -- with the hub batch's
    300-node graph left out (``edge_batch(..., hub=False)``): it would break the promise, and a malformed batch belongs to the
    containment tests.  Every step carries the fresh object's bits and tables."""
    model, steps = _sizes_steps(family, hidden=hidden, entries=("prep_next",) * 8, stage=False)
    no_hub = edge_batch(8, W.IN_DIM, seed=120, hub=False)
    steps[2] = dataclasses.replace(steps[2], name="edge-batch without the hub", batch=no_hub)
    assert max(np.diff(s.batch.node_ptr).max() for s in steps) <= promise
    caps = W.capacities([s.batch for s in steps])
    settings = {"set_max_graph_nodes": (promise,)}
    fresh = Fresh(family, model, caps, dev)
    fresh.settings = dict(settings)
    pipe = Pipeline(family, model, caps, dev, steps, settings)
    results = W.run_sequence(steps, pipe, fresh, References(family, model), _recorder(f"workspace_life/prep_next/{family}"))
    _assert_everything_ran(steps, results)
    assert {r["path"] for r in results if "path" in r} == paths
    for r in pipe.pair:
        r.cm.check()


# ---------------------------------------------------------------------------------------------------- d. a captured forward
def _captured_between_unlike_eager_ones(dev, family, hidden=32):
    """The captured forward on batch A replays with A's eager bits after an eager forward on the hub batch has rewritten the
    workspace's tables, activations and scratch; an eager forward on the reversed batch afterwards carries the fresh object's
    bits.  A single capture stream, no large segment: the graph has no parallel branches."""
    model, batches, attrs = W.family_sequence(family, hidden=hidden)
    edges = family in W.EDGE_FAMILIES
    a, hub, rev = batches[0], batches[2], batches[4]
    caps = W.capacities([a, hub, rev])
    long = Runner(family, model, caps, dev)
    cm = long.cm
    xa, cooa, nptra, eptra = to_dev(a, dev)
    ead = _t(attrs[0], dev) if edges else None  # (held alive beside x: the captured forward reads it at every replay)

    def forward(**kw):
        return cm.forward_edges(xa, ead, cooa, nptra, eptra, **kw) if edges else cm.forward(xa, cooa, nptra, eptra, **kw)
    eager = forward().clone()  # (also the warm-up outside the capture: kernel attributes, caches)
    out = torch.zeros_like(eager)
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):  # (one stream, no parallel branches)
        forward(out=out)
    torch.cuda.synchronize()
    fresh, refs = Fresh(family, model, caps, dev), References(family, model)
    hub_step = W.Step("edge-batch", hub, "forward", edge_attr=attrs[2], tables=True, stage=W.stage_operands(family, hub, 1001))
    rev_step = W.Step("qm9-96-reversed", rev, "forward", edge_attr=attrs[4], tables=True, stage=W.stage_operands(family, rev, 1002))
    W.run_sequence([hub_step], _long(long), fresh, refs, _recorder(f"workspace_life/captured/{family}"))
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)  # (the replay prepares A again: the hub batch's tables are gone, A's bits are back)
    ref, base = W.model_refs(family, model, a, attrs[0])
    R.budget(_host(out), ref, base, what="replay of A")
    W.run_sequence([rev_step], _long(long), fresh, refs, _recorder(f"workspace_life/captured/{family}"))
    cm.check()


def test_a_captured_forward_between_unlike_eager_ones(dev):
    """One layer-wise family (GraphSAGE), a single capture stream, no large segment: the graph has no parallel branches.  The
    captured forward on batch A replays with A's eager bits after an eager forward on the hub batch has rewritten the workspace's
    tables and activations; an eager forward on the reversed batch afterwards carries the fresh object's bits."""
    _captured_between_unlike_eager_ones(dev, "sage")


@pytest.mark.parametrize("family", ["ggnn", "gate"])
def test_a_captured_forward_between_unlike_eager_ones_of(dev, family):
    """The test above (it keeps its name) for two of the newer families.  gate: the capture is of ``forward_edges``.  ggnn: three
    steps per layer at hidden 9, where the captured graph has A's carve of the state buffers baked in -- the second one
    ``roundup4(9 N)`` floats into the scratch -- and the eager forward of the hub batch in between carves the same memory for
    another N, whose ``9 N`` has another remainder by 4."""
    if family == "ggnn":
        batches = W.family_sequence(family, hidden=9)[1]
        assert (9 * batches[0].num_nodes) % 4 != (9 * batches[2].num_nodes) % 4  # (1742 and 489 nodes: 2 and 1)
    _captured_between_unlike_eager_ones(dev, family, hidden=9 if family == "ggnn" else 32)


# ---------------------------------------------------------------------------------------------------- e. setters behind graph_prep
def _prepared_forward(runner, step, between, entry, nxt=None):
    """``graph_prep`` of the step's batch, the setters ``between``, then the prepared entry -> a result as ``Runner.run``'s."""
    cm, dev, b = runner.cm, runner.dev, step.tables_batch
    idx = to_dev(b, dev)[1:]
    cm.graph_prep(*idx, b.num_nodes)
    for name, args in between:
        getattr(cm, name)(*args)
    x = _t(b.x, dev)
    if entry == "forward_prepared":
        out = cm.forward_prepared(x)
    elif entry == "forward_prepared_edges":
        out = cm.forward_prepared_edges(x, _t(step.edge_attr, dev))
    else:
        assert entry == "forward_prepared_prep_next", entry
        out = cm.forward_prepared_prep_next(x, nxt.cm, *idx, b.num_nodes)
    res = {"out": _host(out), "path": cm.last_path()}
    cm.check()
    row_ptr, col, in_deg = cm.tables_to_host()
    res["tables"] = (row_ptr.copy(), col.copy(), in_deg.copy(), cm.edge_index_table_to_host().copy())
    return res


SEGMENT_CASES = [  # (settings at graph prep, setters between prep and forward, the route the PREP's settings give)
    ("segment-cleared", {"set_max_graph_nodes": (29,), "set_large_segment": "tail"}, (("set_large_segment", ()),), "+large_layerwise"),
    ("segment-set", {"set_max_graph_nodes": (29,)}, (("set_large_segment", "half"),), ""),
    ("segment-moved", {"set_max_graph_nodes": (29,), "set_large_segment": "tail"}, (("set_large_segment", "half"),), "+large_layerwise"),
    ("promise-cleared", {"set_max_graph_nodes": (29,)}, (("set_max_graph_nodes", (0,)),), ""),
    ("promise-set", {}, (("set_max_graph_nodes", (29,)),), None),
]


@pytest.mark.parametrize("entry", ["forward_prepared", "forward_prepared_prep_next"])
@pytest.mark.parametrize("family,layers,stack", [("gcn", 2, "stack_zf"), ("gin", 3, "stack")])
@pytest.mark.parametrize("case,at_prep,between,suffix", SEGMENT_CASES)
def test_setters_between_prep_and_forward_speak_of_the_next_prep(dev, case, at_prep, between, suffix, family, layers, stack, entry):
    """``graph_prep`` -> setter -> prepared forward: the forward runs the split, the promise and the tile size its prep validated
    and baked into the tables -- the fresh object's bits for the settings that held AT PREP, its route, a clean ``check()`` -- and
    the setter takes effect at the next prep, where the plain forward carries the bits of a fresh object with the new settings."""
    model = W.make_family_model(family, hidden=64, layers=layers, seed=1)
    tail = W.with_features(synthetic.make_batch("molhiv_tail", 96, seed=13), W.IN_DIM, 13)
    small = W.with_features(synthetic.make_batch("qm9", 96, seed=11), W.IN_DIM, 11)
    ordered, _, triple = order_large_last(tail, 29)
    with_segment = at_prep.get("set_large_segment") == "tail"
    b = ordered if with_segment else small  # (without a segment the promise has to hold for every graph: the hub-less batch)
    assert triple[0] >= tail.num_graphs // 2  # (the graphs in front of "half" keep the promise in the ordered batch too)
    half = (b.num_graphs // 2, int(b.node_ptr[b.num_graphs // 2]), int(b.edge_ptr[b.num_graphs // 2]))  # a triple that fits the batch
    named = {"tail": triple, "half": half}
    at_prep = {k: named.get(v, v) for k, v in at_prep.items()}
    between = tuple((k, named.get(v, v)) for k, v in between)
    caps = W.capacities([tail, small])
    step = W.Step(case, b, entry, tables=True)
    long = Runner(family, model, caps, dev, settings=at_prep, addons=False)
    nxt = Runner(family, model, caps, dev, settings=at_prep, addons=False) if entry.endswith("prep_next") else None
    got = _prepared_forward(long, step, between, entry, nxt)
    want = Runner(family, model, caps, dev, settings=at_prep, addons=False).run(step, entry="forward")
    W.assert_same_bits(got, want, f"{case}: prepared forward against a fresh object with the prep's settings")
    assert got["path"] == ("layerwise" if suffix is None else stack + suffix), got["path"]
    ref, base = W.model_refs(family, model, b, None)
    R.budget(got["out"], ref, base, what=case)
    if nxt is not None:  # the guest's tables are the batch's too
        nxt.cm.check()
        assert all(np.array_equal(p, q) for p, q in zip(nxt.cm.tables_to_host(), got["tables"][:3]))
    # the next prep sees the setter: the plain forward on the same object against a fresh one with the settings as they stand now
    now = dict(at_prep, **dict(between))
    # (a segment names graph B / 2 of the batch it was made for: that batch again; without one the promise covers every graph)
    nstep = W.Step(case + ", next batch", b if now.get("set_large_segment") else small, "forward", tables=True)
    after = long.run(nstep)
    fresh = Runner(family, model, caps, dev, settings=now, addons=False).run(nstep)
    W.assert_same_bits(after, fresh, f"{case}: the next forward against a fresh object with the settings as they stand")
    assert after["path"] == {"segment-cleared": stack, "segment-set": stack + "+large_layerwise", "segment-moved": stack + "+large_layerwise",
                             "promise-cleared": "layerwise", "promise-set": stack}[case], after["path"]


@pytest.mark.parametrize("first,then", [(15, 0), (0, 15)])
def test_degree_promise_between_prep_and_forward(dev, first, then):
    """PNA: the degree-class tables belong to the prepared batch.  ``set_max_degree`` after ``graph_prep`` neither drops tables
    that the prep made nor conjures ones it did not: the prepared forward has the fresh object's bits for the promise that held at
    prep -- the class form's (they differ from ``pna_classes = 0``) or the general form's."""
    model = W.make_family_model("pna", hidden=64, layers=2, seed=PNA_ROUTE_SEEDS[0])
    b = _pna_route_batches()[0]
    caps = W.capacities([b])
    step = W.Step(f"degree {first} -> {then}", b, "forward_prepared", tables=True)
    _assert_pna_references_are_clear("pna", model, [step])
    at_prep = {"set_max_degree": (first,)}
    got = _prepared_forward(Runner("pna", model, caps, dev, settings=at_prep, addons=False), step, (("set_max_degree", (then,)),), "forward_prepared")
    want = Runner("pna", model, caps, dev, settings=at_prep, addons=False).run(step, entry="forward")
    W.assert_same_bits(got, want, "prepared forward against a fresh object with the prep's promise")
    general = Runner("pna", model, caps, dev, settings=at_prep, addons=False, options={"pna_classes": 0}).run(step, entry="forward")
    assert np.array_equal(general["out"].view(np.uint32), got["out"].view(np.uint32)) == (first == 0)
    ref, base = W.model_refs("pna", model, b, None)
    R.budget(got["out"], ref, base, what=step.name)


@pytest.mark.parametrize("family", ["gine", "transformere", "gate", "resgatede"])
def test_setters_between_prep_and_forward_edges(dev, family):
    """``forward_prepared_edges`` goes through the same body: every setter between ``graph_prep`` and it leaves the route
    (``layerwise``) and the bits alone."""
    model, batches, attrs = W.family_sequence(family)
    b, ea = batches[6], attrs[6]
    caps = W.capacities([b])
    step = W.Step("molhiv-40", b, "forward_prepared_edges", edge_attr=ea, tables=True)
    half = (b.num_graphs // 2, int(b.node_ptr[b.num_graphs // 2]), int(b.edge_ptr[b.num_graphs // 2]))
    between = (("set_max_graph_nodes", (64,)), ("set_max_degree", (15,)), ("set_large_segment", half))
    got = _prepared_forward(Runner(family, model, caps, dev, addons=False), step, between, "forward_prepared_edges")
    want = Runner(family, model, caps, dev, addons=False).run(step, entry="forward")
    W.assert_same_bits(got, want, "prepared forward against a fresh object")
    assert got["path"] == "layerwise"
    ref, base = W.model_refs(family, model, b, ea)
    R.budget(got["out"], ref, base, what=family)


@pytest.mark.parametrize("family", ["gat", "ggnn"])
def test_setters_between_prep_and_forward_plain(dev, family):
    """The plain twin: every setter between ``graph_prep`` and ``forward_prepared`` leaves the route (``layerwise``), the tables and
    the bits alone."""
    model, batches, _ = W.family_sequence(family)
    b = batches[6]
    caps = W.capacities([b])
    step = W.Step("molhiv-40", b, "forward_prepared", tables=True)
    half = (b.num_graphs // 2, int(b.node_ptr[b.num_graphs // 2]), int(b.edge_ptr[b.num_graphs // 2]))
    between = (("set_max_graph_nodes", (64,)), ("set_max_degree", (15,)), ("set_large_segment", half))
    got = _prepared_forward(Runner(family, model, caps, dev, addons=False), step, between, "forward_prepared")
    want = Runner(family, model, caps, dev, addons=False).run(step, entry="forward")
    W.assert_same_bits(got, want, "prepared forward against a fresh object")
    assert got["path"] == "layerwise"
    ref, base = W.model_refs(family, model, b, None)
    R.budget(got["out"], ref, base, what=family)
