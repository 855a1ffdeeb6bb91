"""One long-lived object against a stream of unlike batches: the driver, the batch sequences and the CPU stand-ins.

``run_sequence`` walks a list of ``Step``s.  For every step it asks two callables for a result -- ``run_long(step)``, bound to
ONE object that lives for the whole sequence, and ``run_fresh(step)``, which builds a new object of the same capacities, options
and promises and runs the step's batch through the plain ``forward`` / ``forward_edges`` -- and asserts

  (a) the two results are equal BIT FOR BIT, key by key with no key left out: the output, ``last_path``, the tables where the
      step asks for them, the stage entry's result, and a refusal's text where an entry refuses the batch;
  (b) ``ref64.budget(got, ref64, base32)`` with the project's K = 4, F = 2^-22 for the output, and the class-wise
      ``gine_util.budget_by_degree`` for the stage entry's result.

The driver has no tolerance of its own.  A result is a dict: ``out`` [B, mlp_out] float32 and ``path``, or ``refused`` (the
error's text); optionally ``tables`` (a tuple of integer arrays), and ``stage`` [N, w] float32 or ``stage_refused``.

The stand-ins (``TorchDevice``) run the package's torch model in fp32 where a device would be, honestly or with ONE kind of state
left over from the batch before; ``tests/test_workspace_life_driver.py`` shows that the driver passes the honest one and rejects
each of the others."""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

import ref64 as R
from gine_util import budget_by_degree
from gnnbuilder_amd import synthetic
from gnnbuilder_amd.batching import from_pyg_batch, pack_graphs
from helpers import EMPTY, batch_vector, edge_batch, grid_features


@dataclass
class Step:
    name: str
    batch: object  # GraphBatch: x [N, in_dim], coo in the order the tables are built from
    entry: str  # which entry point the long-lived object runs it through (the fresh one: always the plain forward)
    edge_attr: Optional[np.ndarray] = None  # [E, edge_dim] in coo order (edge families; None where E = 0)
    setters: tuple = ()  # ((method name, args), ...): applied to the long-lived object BEFORE the entry, and they persist
    tables: bool = False  # compare the tables read back with tables_to_host as well
    pyg: Optional[tuple] = None  # (edge_index [2, E] int64, edge_attr in ITS column order or None): the mini-batch of the PyG entries
    stage: Optional[dict] = None  # operands of the stage entry that follows the forward
    same_as: Optional[int] = None  # an earlier step of the sequence whose long-lived result this one repeats bit for bit
    ordered: Optional[tuple] = None  # the ordered entry: (batch with the oversized graphs last, perm, triple) of batching.order_large_last

    @property
    def tables_batch(self):
        """The batch in the order the workspace's tables hold it: what a stage entry behind the forward runs on."""
        return self.batch if self.ordered is None else self.ordered[0]


# ---------------------------------------------------------------------------------------------------- the driver
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same_bits(got, want, what):
    """Every key of both results, nothing left out: float32 arrays by their bit patterns (so -0 is not +0 and a NaN must be the
    same NaN), integer arrays by value, strings by equality."""
    assert set(got) == set(want), f"{what}: results hold different things: {sorted(got)} against {sorted(want)}"
    for key in sorted(got):
        g, w = got[key], want[key]
        if isinstance(g, str) or isinstance(w, str):
            assert g == w, f"{what}: {key}: {g!r} against {w!r}"
            continue
        gs, ws = (g, w) if isinstance(g, (tuple, list)) else ((g,), (w,))
        assert len(gs) == len(ws), f"{what}: {key}: {len(gs)} arrays against {len(ws)}"
        for i, (ga, wa) in enumerate(zip(gs, ws)):
            ga, wa = np.asarray(ga), np.asarray(wa)
            assert ga.shape == wa.shape and ga.dtype == wa.dtype, f"{what}: {key}[{i}]: {ga.dtype}{ga.shape} against {wa.dtype}{wa.shape}"
            same = _bits(ga) == _bits(wa)
            if not np.all(same):
                first = tuple(int(v) for v in np.argwhere(~same)[0])
                raise AssertionError(f"{what}: {key}[{i}] differs in {int((~same).sum())} of {same.size} elements, first at {first}: "
                                     f"{ga[first]!r} against {wa[first]!r}")


def run_sequence(steps, run_long, run_fresh, reference, record=None):
    """The driver (module docstring).  ``reference(step)`` -> {"out": (ref64, base32)} and, where the step has a stage entry,
    "stage": (ref64, base32, coo of the tables) -- for every key the long-lived result holds as numbers.  ``record(key,
    e / e32)`` receives every figure.  Returns the long-lived results."""
    longs = []
    for i, step in enumerate(steps):
        what = f"step {i + 1} {step.name} [{step.entry}]"
        long, fresh = run_long(step), run_fresh(step)
        for key in ("refused", "stage_refused"):
            if key in long:
                print(f"{what}: {key}: {long[key]}")
        assert_same_bits(long, fresh, f"(a) {what}: long-lived against fresh")
        if step.same_as is not None:
            assert_same_bits(long, longs[step.same_as], f"(a) {what}: against step {step.same_as + 1} on the same object")
        refs = reference(step)
        need = {k for k in ("out", "stage") if k in long}  # every number the object produced has a reference
        assert need <= set(refs), f"(b) {what}: no reference for {sorted(need - set(refs))}"
        if "out" in need:
            ref, base = refs["out"]
            e, e32, _ = R.errors(long["out"], ref, base)
            print(f"{what}: out e = {e:.3e}, e32 = {e32:.3e}, e / e32 = {R.ratio(e, e32):.2f}")
            if record:
                record("out", R.ratio(e, e32))
            R.budget(long["out"], ref, base, what=f"(b) {what}: out")
        if "stage" in need:
            ref, base, coo = refs["stage"]
            for name, r in budget_by_degree(long["stage"], ref, base, coo, what=f"(b) {what}: stage").items():
                if record:
                    record(f"stage/{name}", r)
        longs.append(long)
    return longs


# ---------------------------------------------------------------------------------------------------- batches
def with_features(batch, width, seed, grid=False):
    """``batch``'s graphs with seeded features of ``width``: uniform(-1, 1), or ``helpers.grid_features`` (PNA)."""
    x = grid_features(batch.num_nodes, width, seed) if grid else \
        np.random.default_rng(seed).uniform(-1, 1, (batch.num_nodes, width)).astype(np.float32)
    return type(batch)(x=x, coo=batch.coo, node_ptr=batch.node_ptr, edge_ptr=batch.edge_ptr)


def reversed_graphs(batch):
    """The graphs of ``batch`` in reversed order."""
    return pack_graphs([batch.graph(g) for g in range(batch.num_graphs)][::-1])


def lone_nodes(count, width, seed):
    """``count`` one-node graphs without an edge."""
    x = np.random.default_rng(seed).uniform(-1, 1, (count, width)).astype(np.float32)
    return pack_graphs([(x[i:i + 1], np.zeros((0, 2), np.int32)) for i in range(count)])


SIZES_UP_AND_DOWN = ("qm9-96", "one-node", "edge-batch", "64-lone-nodes", "qm9-96-reversed", "three-empty", "molhiv-40", "qm9-96-again")


def sizes_up_and_down(in_dim, seeds, grid=False):
    """The eight batches of ``SIZES_UP_AND_DOWN`` with features of ``in_dim``; ``seeds``: one feature seed per batch (the last
    batch is the first).  The largest has under 2,000 nodes; ``edge-batch`` holds explicit self loops, duplicate edges, isolated
    nodes, an empty graph, a one-node graph and a hub of in-degree 1200."""
    first = with_features(synthetic.make_batch("qm9", 96, seed=seeds[0]), in_dim, seeds[0], grid)
    return [first,
            with_features(lone_nodes(1, in_dim, seeds[1]), in_dim, seeds[1], grid),
            with_features(edge_batch(8, in_dim, seeds[2]), in_dim, seeds[2], grid),
            with_features(lone_nodes(64, in_dim, seeds[3]), in_dim, seeds[3], grid),
            with_features(reversed_graphs(first), in_dim, seeds[4], grid),
            pack_graphs([EMPTY(in_dim)] * 3),
            with_features(synthetic.make_batch("molhiv", 40, seed=seeds[6]), in_dim, seeds[6], grid),
            first]


def capacities(batches):
    return tuple(max(max(getattr(b, k) for b in batches), 1) for k in ("num_graphs", "num_nodes", "num_edges"))


def shuffled_mini_batch(batch, edge_attr, seed):
    """``batch`` as a PyG loader could hold it -- the columns of ``edge_index`` (and the rows of ``edge_attr`` with them) under one
    seeded permutation across graphs -- and what the ingest makes of it: returns (batch whose coo is ``from_pyg_batch``'s, its
    edge_attr or None, (edge_index [2, E] int64, edge_attr in edge_index's order or None), the ingest's order)."""
    perm = np.random.default_rng(seed).permutation(batch.num_edges)
    ei = np.ascontiguousarray(batch.coo[perm].T.astype(np.int64)).reshape(2, -1)
    ea = None if edge_attr is None else np.ascontiguousarray(edge_attr[perm])
    made = from_pyg_batch(batch.x, ei, ptr=batch.node_ptr.astype(np.int64), edge_attr=ea, return_edge_order=True)
    gb, ea_ord, order = (made[0], None, made[1]) if ea is None else made
    return gb, ea_ord, (ei, ea), order


def grouped_mini_batch(batch, edge_attr):
    """The PyG form of ``batch`` with its edges in ``coo``'s own order: the ingest returns ``coo`` itself."""
    return np.ascontiguousarray(batch.coo.T.astype(np.int64)).reshape(2, -1), edge_attr


# ---------------------------------------------------------------------------------------------------- PNA: the std's threshold
def pna_layer_variances(model, batch, x, edge_attr=None):
    """Per layer of a float64 copy of a PNA / PNAE ``model``: (var [rows, F] of the messages per (node, column), max_j h_ij^2) on
    the rows that have in-edges (``pnae_util.layer_variances`` for both families)."""
    import copy
    m = copy.deepcopy(model).double()
    ei = R.edge_index(batch.coo)
    h = torch.from_numpy(np.ascontiguousarray(x)).double()
    ea = None if edge_attr is None else torch.from_numpy(np.ascontiguousarray(edge_attr)).double()
    dst = ei[1].numpy()
    out = []
    with torch.no_grad():
        for i, (conv, act) in enumerate(zip(m.gnn_convs, m.gnn_activations)):
            msg = (conv.conv.pre_nns[0](torch.cat([h[ei[1]], h[ei[0]]], -1)) if ea is None else conv.conv.message(h, ei, ea)).numpy()
            n, w = h.shape[0], msg.shape[1]
            deg = np.bincount(dst, minlength=n)[:n]
            s1, s2, hi = np.zeros((n, w)), np.zeros((n, w)), np.zeros((n, w))
            np.add.at(s1, dst, msg)
            np.add.at(s2, dst, msg * msg)
            np.maximum.at(hi, dst, msg * msg)
            has = deg > 0
            d = np.maximum(deg, 1)[:, None]
            out.append(((s2 / d - (s1 / d) ** 2)[has], hi[has]))
            h_in = h
            h = conv(h, ei) if ea is None else conv(h, ei, ea)
            if m.gnn_skip_connection and i != 0 and i != m.gnn_num_layers - 1:
                h = h + h_in
            h = act(h)
    return out


def variances_near_the_threshold(model, batch, x, edge_attr=None):
    """How many (node, column) variances of the float64 reference lie within ``16 * 2^-24 * max_j h_ij^2`` of PyG's 1e-5, over
    all layers (``test_hip_pnae.assert_no_variance_near_the_threshold``'s margin): 0 means fp32 decides every std's clamp and mask
    as float64 does."""
    if batch.num_edges == 0:
        return 0
    return int(sum((np.abs(var - R.PNA_STD_EPS) <= 16 * 2.0 ** -24 * hi).sum() for var, hi in pna_layer_variances(model, batch, x, edge_attr)))


# ---------------------------------------------------------------------------------------------------- one model per family
FAMILIES = ("gcn", "gin", "sage", "pna", "gine", "pnae", "gatv2", "gatv2e", "transformer", "transformere", "resgated", "resgatede", "gat",
            "gate", "ggnn")
EDGE_FAMILIES = ("gine", "pnae", "gatv2e", "transformere", "resgatede", "gate")
GGNN_STEPS, GGNN_H_WIDTH = 3, 12  # three steps: both state buffers are written and read in turn; the stage's h narrower than its width
IN_DIM, EDGE_DIM, HEADS = 9, 3, 4


def make_family_model(family, hidden=32, layers=2, seed=0, out_dim=None):
    """The family's model from its existing maker: ``in_dim`` 9, all three pools, 4 heads where there are heads, ``edge_dim`` 3,
    ``GGNN_STEPS`` steps per GatedGraphConv layer; ``out_dim``: the last layer's width (None: ``hidden``)."""
    import gat_util
    import gate_util
    import gatv2_util
    import gatv2e_util
    import gine_util
    import pnae_util
    import ggnn_util
    import resgated_util
    import resgatede_util
    import transformer_util
    import transformere_util
    from helpers import make_model
    kw = dict(in_dim=IN_DIM, hidden=hidden, layers=layers, seed=seed)
    if out_dim is not None:
        kw["out_dim"] = out_dim
    if family in ("gcn", "gin", "sage", "pna"):
        return make_model(family, **kw)
    if family == "gine":
        return gine_util.make_gine_model(edge_dim=EDGE_DIM, **kw)
    if family == "pnae":
        return pnae_util.make_pnae_model(edge_dim=EDGE_DIM, **kw)
    if family == "gatv2":
        return gatv2_util.make_gatv2_model(heads=HEADS, **kw)
    if family == "gatv2e":
        return gatv2e_util.make_gatv2e_model(edge_dim=EDGE_DIM, heads=HEADS, **kw)
    if family == "transformer":
        return transformer_util.make_transformer_model(heads=HEADS, **kw)
    if family == "transformere":
        return transformere_util.make_transformere_model(edge_dim=EDGE_DIM, heads=HEADS, **kw)
    if family == "resgated":
        return resgated_util.make_resgated_model(**kw)
    if family == "resgatede":
        return resgatede_util.make_resgatede_model(edge_dim=EDGE_DIM, **kw)
    if family == "gat":
        return gat_util.make_gat_model(heads=HEADS, **kw)
    if family == "gate":
        return gate_util.make_gate_model(edge_dim=EDGE_DIM, heads=HEADS, **kw)
    assert family == "ggnn", family
    return ggnn_util.make_ggnn_model(steps=GGNN_STEPS, **kw)


# Seeds of the pna / pnae sequences, chosen on the CPU (tests/test_workspace_life_driver.py asserts them): the model's seed, then
# one feature seed per batch of SIZES_UP_AND_DOWN (the first that leaves no variance of the float64 reference within the margin of
# PyG's 1e-5 -- variances_near_the_threshold -- counted up from 100 + 10 * position); the other families take 100 + 10 * position
PNA_SEEDS = {"pna": (3, (104, 110, 122, 130, 163, 150, 161, 104)), "pnae": (0, (101, 110, 120, 130, 143, 150, 160, 101))}


def family_sequence(family, hidden=32, layers=2):
    """(model, the eight batches of ``SIZES_UP_AND_DOWN``, their edge attributes or Nones) for ``family``; pna and pnae on grid
    features (``helpers.grid_features``) under ``PNA_SEEDS``."""
    import gine_util
    model_seed, seeds = PNA_SEEDS.get(family, (0, tuple(100 + 10 * i for i in range(7)) + (100,)))
    model = make_family_model(family, hidden, layers, model_seed)
    batches = sizes_up_and_down(IN_DIM, seeds, grid=family in PNA_SEEDS)
    attrs = [gine_util.edge_attrs(b.num_edges, EDGE_DIM, seed=s + 1) if family in EDGE_FAMILIES and b.num_edges else None
             for b, s in zip(batches, seeds)]
    attrs[-1] = attrs[0]
    return model, batches, attrs


def model_refs(family, model, batch, edge_attr):
    """(float64 reference, fp32 ``base``) of the whole model on ``batch``: the ones the family's whole-model test uses -- the
    model's own torch definition on a ``.double()`` copy and as it stands, both on the CPU."""
    import gine_util
    if family in EDGE_FAMILIES:
        ea = np.zeros((0, EDGE_DIM), np.float32) if edge_attr is None else edge_attr
        return gine_util.forward64(model, batch, batch.x, ea), gine_util.run(model, batch, batch.x, ea)
    return R.forward64(model, batch, batch.x), R.run(model, batch, batch.x)


# ---------------------------------------------------------------------------------------------------- one stage entry per family
STAGE_W, STAGE_EPS = 32, 0.25
PNA_VAR_WINDOW = (2.5e-6, 4e-5)  # (test_hip_pnae.VAR_WINDOW) around PyG's std threshold 1e-5: no variance of the reference may lie here


def _uniform(seed, shape, span=1.0):
    return np.random.default_rng(seed).uniform(-span, span, shape).astype(np.float32)


def stage_operands(family, batch, seed):
    """Fresh operands of width ``STAGE_W`` for the family's stage entry on ``batch`` (the batch as the tables hold it): uniform
    for the plain aggregates, the family's own dyadic grids (its ``*_util.stage_case`` / ``edge_case``, "flat") for the others --
    an edge family's ``edge_attr`` the one its helper made for this ``coo``."""
    import gat_util
    import gate_util
    import gatv2_util
    import gatv2e_util
    import gine_util
    import ggnn_util
    import pnae_util
    import resgated_util
    import resgatede_util
    import transformer_util
    import transformere_util
    n, e, w = batch.num_nodes, batch.num_edges, STAGE_W
    if family in ("gcn", "gin", "sage"):
        return dict(x=_uniform(seed, (n, w)))
    if family == "pna":
        return dict(x=grid_features(n, w, seed), q=_uniform(seed + 1, (n, w)))
    if family == "gine":
        we, be = gine_util.stage_weights(w, EDGE_DIM, seed + 2)
        return dict(x=_uniform(seed, (n, w)), ea=gine_util.edge_attrs(e, EDGE_DIM, seed + 1), we=we, be=be)
    if family == "pnae":
        return pnae_util.stage_case(batch, w, EDGE_DIM)
    if family == "gatv2":
        return gatv2_util.stage_case(n, w, HEADS, "flat", seed=seed)
    if family == "gatv2e":
        return gatv2e_util.edge_case(batch.coo, n, w, HEADS, EDGE_DIM, "flat", seed=seed)
    if family == "transformer":
        return transformer_util.stage_case(n, w, HEADS, "flat")
    if family == "transformere":
        return transformere_util.edge_case(batch.coo, n, w, HEADS, EDGE_DIM, "flat")
    if family == "resgated":
        return resgated_util.stage_case(n, w, "flat")
    if family == "resgatede":
        return resgatede_util.edge_case(batch.coo, n, w, EDGE_DIM, "flat")
    if family == "gat":
        return gat_util.stage_case(n, w, HEADS, "flat", seed=seed)
    if family == "gate":
        return gate_util.edge_case(batch.coo, n, w, HEADS, EDGE_DIM, "flat", seed=seed)
    assert family == "ggnn", family
    return ggnn_util.stage_case(n, w, GGNN_H_WIDTH, "flat")  # (h narrower than the stage: its zero-padded columns are exercised)


def stage_refs(family, batch, c):
    """(float64 restatement, the same in fp32, the edges of the tables for the in-degree classes) of the family's stage entry on
    operands ``c``.  What a reference needs to hold for the comparison to leave nothing out is asserted here, on the reference
    alone: no PNA variance near PyG's threshold; every non-self GAT score, every ResGated gate argument and gated value and every
    GatedGraphConv neighbour sum and r and z argument exact in fp32."""
    import gat_util
    import gate_util
    import gatv2_util
    import gatv2e_util
    import ggnn_util
    import pnae_util
    import resgated_util
    import resgatede_util
    import transformer_util
    import transformere_util
    coo, n = batch.coo, batch.num_nodes
    f8, f4 = np.float64, np.float32
    if family == "gcn":  # (a GCN workspace's tables hold no explicit self loop)
        tc = R.workspace_edges(coo, True)
        return R.gcn_agg64(c["x"], tc), R.gcn_agg64(c["x"], tc, f4), tc
    if family == "gin":
        return R.sum_agg64(c["x"], coo, STAGE_EPS), R.sum_agg64(c["x"], coo, STAGE_EPS, f4), coo
    if family == "sage":
        return R.mean_agg64(c["x"], coo), R.mean_agg64(c["x"], coo, f4), coo
    if family in ("pna", "pnae"):
        if family == "pna":
            src, dst = coo[:, 0], coo[:, 1]
            h64, h32 = c["x"].astype(f8)[src] + c["q"].astype(f8)[dst], c["x"][src] + c["q"][dst]
        else:
            h64, h32 = pnae_util.stage_messages(coo, c, c["q"], f8), pnae_util.stage_messages(coo, c, c["q"], f4)
            assert np.array_equal(h32.astype(f8), h64)  # every message is exact in fp32
        ref, var, _ = pnae_util.stage_ref(coo, n, h64)
        assert not ((var >= PNA_VAR_WINDOW[0]) & (var <= PNA_VAR_WINDOW[1])).any()
        return ref, pnae_util.stage_ref(coo, n, h32)[0], coo
    if family == "gine":
        ref = R.gine_agg64(c["x"], coo, c["ea"].astype(f8) @ c["we"].astype(f8).T + c["be"].astype(f8), STAGE_EPS)
        return ref, R.gine_agg64(c["x"], coo, (c["ea"] @ c["we"].T + c["be"]).astype(f4), STAGE_EPS, dtype=f4), coo
    if family == "gatv2e" and batch.num_edges == 0:  # (no attribute row: every self loop's mean attribute is 0 -- GATv2 on self loops)
        family = "gatv2"
    if family == "transformere" and batch.num_edges == 0:  # (no edge: nothing to project -- TransformerConv, every row its root)
        family = "transformer"
    if family == "gatv2":  # (a GATv2 workspace is a GCN description: explicit self loops dropped, as gatv2_ref drops them)
        args = (c["xl"], c["xr"], c["att"], c["bias"], None, "none", coo, HEADS, gatv2_util.SLOPE)
        return gatv2_util.gatv2_ref(*args), gatv2_util.gatv2_ref(*args, dtype=f4), R.workspace_edges(coo, True)
    if family == "gatv2e":
        args = (c["xl"], c["xr"], c["att"], c["bias"], None, "none", coo, c["edge_attr"], c["w_edge"], HEADS, gatv2_util.SLOPE)
        return gatv2e_util.gatv2e_ref(*args), gatv2e_util.gatv2e_ref(*args, dtype=f4), R.workspace_edges(coo, True)
    if family == "transformer":
        args = (c["q"], c["k"], c["v"], c["root"], None, "none", coo, HEADS, c["scale"])
        return transformer_util.transformer_ref(*args), transformer_util.transformer_ref(*args, dtype=f4), coo
    if family == "transformere":
        args = (c["q"], c["k"], c["v"], c["qe"], c["root"], None, "none", coo, c["edge_attr"], c["w_edge"], HEADS, c["scale"])
        return transformere_util.transformere_ref(*args), transformere_util.transformere_ref(*args, dtype=f4), coo
    if family == "gate" and batch.num_edges == 0:  # (no attribute row: every self loop's mean attribute is 0 -- GAT on self loops)
        family = "gat"
    if family == "resgatede" and batch.num_edges == 0:  # (no edge: no gate and no value -- ResGatedGraphConv without a neighbour)
        family = "resgated"
    if family == "resgated":
        args = (c["k"], c["q"], c["v"], c["root"], None, "none", coo)
        return resgated_util.resgated_ref(*args), resgated_util.resgated_ref(*args, dtype=f4), coo
    if family == "resgatede":
        resgatede_util.assert_exact_terms(c, coo)
        args = (c["k"], c["q"], c["v"], c["root"], None, "none", coo, c["edge_attr"], c["w_gate"], c["w_value"])
        return resgatede_util.resgatede_ref(*args), resgatede_util.resgatede_ref(*args, dtype=f4), coo
    if family == "gat":  # (a GAT workspace is a GCN description too: explicit self loops dropped, as gat_ref drops them)
        args = (c["xl"], c["s_src"], c["s_dst"], c["bias"], None, "none", coo, HEADS, gat_util.SLOPE)
        return gat_util.gat_ref(*args), gat_util.gat_ref(*args, dtype=f4), R.workspace_edges(coo, True)
    if family == "gate":
        gate_util.assert_exact_scores(c, coo, "flat")
        args = (c["xl"], c["s_src"], c["s_dst"], c["a_edge"], c["bias"], None, "none", coo, c["edge_attr"], HEADS, gate_util.SLOPE)
        return gate_util.gate_ref(*args, fill="mean"), gate_util.gate_ref(*args, dtype=f4, fill="mean"), R.workspace_edges(coo, True)
    assert family == "ggnn", family
    ggnn_util.arguments_are_exact(c, coo)
    args = (c["p"], c["gh"], c["h"], c["b_ih"], None, "none", coo)
    return ggnn_util.ggnn_ref(*args), ggnn_util.ggnn_ref(*args, dtype=f4), coo


# ---------------------------------------------------------------------------------------------------- the CPU stand-ins
def torch_forward(model, batch, x, edge_attr=None, coo=None, pooled_hook=None):
    """The model as it stands (its own dtype), layer by layer as ``ref64.run`` / ``gine_util.run`` walk it; ``pooled_hook`` sees
    the pooled matrix before the head.  Returns (out [B, mlp_out], pooled)."""
    dtype = next(model.parameters()).dtype
    ei = R.edge_index(batch.coo if coo is None else coo)
    h = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)
    ea = None if edge_attr is None else torch.from_numpy(np.ascontiguousarray(edge_attr)).to(dtype)
    with torch.no_grad():
        for i, (conv, act) in enumerate(zip(model.gnn_convs, model.gnn_activations)):
            h_in = h
            h = conv(h, ei) if ea is None else conv(h, ei, ea)
            if model.gnn_skip_connection and i != 0 and i != model.gnn_num_layers - 1:
                h = h + h_in
            h = act(h)
        pooled = model.global_pooling(h, torch.from_numpy(batch_vector(batch)), batch.num_graphs)
        if pooled_hook is not None:
            pooled = pooled_hook(pooled)
        out = model.mlp_head(pooled)
        if model.output_activation_module is not None:
            out = model.output_activation_module(out)
    return out.numpy(), pooled


FAULTS = ("pooled-row-kept", "stale-dinv", "rows-beyond-previous-N-zero", "previous-edges-appended", "previous-edge-order")


class TorchDevice:
    """The torch model in the model's dtype where the device would be.  ``fault`` (one of ``FAULTS``, None: honest) makes it carry
    ONE kind of state from the batch before into the next, as a workspace whose arrays are sized for the capacity could:

    - ``pooled-row-kept``: a graph of at most one node keeps row g of the previous batch's pooled matrix;
    - ``stale-dinv``: the GCN stage entry takes ``dinv`` from the previous batch's in-degrees for the first min(N_prev, N) nodes;
    - ``rows-beyond-previous-N-zero``: rows of ``x`` from N_prev on are read as zero;
    - ``previous-edges-appended``: the previous batch's last E_prev - E edges follow the current edge list (those that lie inside
      the current batch's N nodes -- the others a device would have read out of bounds);
    - ``previous-edge-order``: the mini-batch's ``edge_attr`` rows are put in the previous mini-batch's edge order.

    ``stage`` of a step: {"x": [N, w]} -> the GCN aggregate on a GCN workspace's tables (explicit self loops dropped)."""

    def __init__(self, model, fault=None):
        assert fault is None or fault in FAULTS
        self.model, self.fault = model, fault
        self.dtype = {torch.float32: np.float32, torch.float64: np.float64}[next(model.parameters()).dtype]
        self.prev = None  # dict of the previous batch's leftovers

    def run(self, step):
        b, fault, prev = step.batch, self.fault, self.prev
        x, coo, ea = b.x, b.coo, step.edge_attr
        order = None
        if step.pyg is not None:  # the ingest: edges grouped by graph with a stable sort, the attribute rows behind them
            ei, ea_in = step.pyg
            made = from_pyg_batch(b.x, ei, ptr=b.node_ptr.astype(np.int64), return_edge_order=True)
            coo, order = made[0].coo, made[1]
            use = order
            if fault == "previous-edge-order" and prev is not None and prev["order"] is not None:
                old = prev["order"][prev["order"] < len(order)]
                use = np.concatenate([old, np.arange(len(old), len(order))])
            ea = None if ea_in is None else np.ascontiguousarray(ea_in[use])
        if fault == "rows-beyond-previous-N-zero" and prev is not None:
            x = x.copy()
            x[prev["N"]:] = 0
        if fault == "previous-edges-appended" and prev is not None and len(prev["coo"]) > len(coo):
            tail = prev["coo"][len(coo):]
            coo = np.concatenate([coo, tail[(tail < b.num_nodes).all(1)]])
            assert ea is None  # (the stand-in of a model without edge attributes)
        hook = None
        if fault == "pooled-row-kept" and prev is not None:
            def hook(pooled):
                pooled, old = pooled.clone(), prev["pooled"]
                for g in np.flatnonzero(np.diff(b.node_ptr) <= 1):
                    if g < old.shape[0]:
                        pooled[g] = old[g]
                return pooled
        out, pooled = torch_forward(self.model, b, x, ea, coo=coo, pooled_hook=hook)
        res = {"out": out, "path": "layerwise"}
        tcoo = R.workspace_edges(b.coo, True)
        deg = np.bincount(tcoo[:, 1], minlength=b.num_nodes)[:b.num_nodes]
        if step.stage is not None:
            use_deg = deg.copy()
            if fault == "stale-dinv" and prev is not None:
                k = min(len(prev["deg"]), len(deg))
                use_deg[:k] = prev["deg"][:k]
            res["stage"] = R.gcn_agg64(step.stage["x"], tcoo, self.dtype, deg=use_deg)
        if order is None and prev is not None:  # (the ingest's scratch outlives the batches that come without an ingest)
            order = prev["order"]
        self.prev = dict(N=b.num_nodes, coo=b.coo, pooled=pooled, deg=deg, order=order)
        return res
