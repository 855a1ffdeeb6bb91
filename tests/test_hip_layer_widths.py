"""Whole models whose layers are unlike in width on the MI355X: ``out_dim != hidden`` for the eleven families whose scratch
layout follows the layer's own width -- ``[k | q | v | r]`` [N, 4 fo], ``[xl | s_src | s_dst | pad]`` [N, fo + roundup4(2 heads)],
``[q | k | v | r | qe]`` [N, 4 fo + roundup4(heads * edge_dim)], ``[p | gh]`` [N, 6 fo] with the per-step weight stride -- carved
from scratch that the workspace sizes as a maximum over the layers, before a pooling and a head that read ``out_dim`` columns.  A
stride, a scratch maximum or a derived weight slot taken from the wrong layer gives the right result whenever all layers are
equally wide; here they are not: three layers (in 9 -> hidden -> hidden -> out), the widths the smallest that separate them -- a
multiple of 4 against one that is not (the 16-byte against the scalar row form), 5 columns per head against 8, narrower and wider.

Every case: ``forward`` / ``forward_edges`` against float64 by ``ref64.budget`` with the project's K = 4, F = 2^-22 (no tolerance
of this file's own; the reference is the model's torch definition on a ``.double()`` copy, ``base`` the same in fp32); the same
bits from a second call, from the prepared form, from the PyG entry on a device ``edge_index`` + ``batch``, and from a workspace
of three times the capacities (the summation order is fixed per batch: larger scratch must not move a bit).  Worst e / e32 go to
GNNB_FP64_REPORT=<file> under ``forward/widths/<family>-<hidden>-<out>``."""
import json
import os

import numpy as np
import pytest
import torch

import ggnn_util
import gine_util
import ref64 as R
import workspace_life_util as W
from gnnbuilder_amd import runtime, synthetic
from gnnbuilder_amd.batching import pack_graphs
from helpers import EMPTY, ONE, batch_vector, to_dev

pytestmark = pytest.mark.gpu

WORST = {}
HEADED = ("gatv2", "gatv2e", "transformer", "transformere", "gat", "gate")
GATED = ("resgated", "resgatede", "gine", "pnae")
# (family, hidden, out_dim, layers, GatedGraphConv steps)
CASES = [(f, h, o, 3, 0) for f in HEADED for h, o in ((32, 20), (20, 32))] + \
        [(f, h, o, 3, 0) for f in GATED for h, o in ((32, 21), (12, 40))] + \
        [("ggnn", 12, 40, 3, 3), ("ggnn", 9, 12, 3, 2), ("ggnn", 4, 16, 1, 2)]  # (in <= hidden <= out; one layer: hidden is no layer's width)
# pnae runs on grid features: (model seed, feature seed) per (hidden, out), chosen on the CPU the way PNA_SEEDS were -- the first
# pair, feature seeds counted up from 160, that leaves no variance of the float64 reference within the margin of PyG's 1e-5
# (variances_near_the_threshold, asserted below on the reference alone); the other families: model seed 0, features 160
PNAE_SEEDS = {(32, 21): (0, 162), (12, 40): (0, 160)}
MOLHIV_SEED, ATTR_SEED = 160, 161  # (molhiv-40 of workspace_life_util's sequence)


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


def widths_model(family, hidden, out_dim, layers, steps, seed=0):
    if family == "ggnn":
        return ggnn_util.make_ggnn_model(in_dim=W.IN_DIM, hidden=hidden, layers=layers, out_dim=out_dim, steps=steps, seed=seed)
    return W.make_family_model(family, hidden=hidden, layers=layers, seed=seed, out_dim=out_dim)


BATCHES = {}


def widths_batch(feature_seed=MOLHIV_SEED, grid=False):
    """molhiv-40 of the workspace-life sequence (1051 nodes, 2320 edges), an empty graph and a one-node graph behind it; its edge
    attributes (the edge families')."""
    key = (feature_seed, grid)
    if key not in BATCHES:
        mol = synthetic.make_batch("molhiv", 40, seed=MOLHIV_SEED)
        graphs = [(g[0][:, :1], g[1]) for g in (mol.graph(i) for i in range(mol.num_graphs))] + [EMPTY(1), ONE(1)]
        b = W.with_features(pack_graphs(graphs), W.IN_DIM, feature_seed, grid)
        assert (b.num_graphs, b.num_nodes, b.num_edges) == (42, 1052, 2320) and list(np.diff(b.node_ptr)[-2:]) == [0, 1]
        BATCHES[key] = (b, gine_util.edge_attrs(b.num_edges, W.EDGE_DIM, seed=ATTR_SEED))
    return BATCHES[key]


def widths_case(family, hidden, out_dim, layers, steps):
    """(model, batch, edge attributes or None) of a case."""
    model_seed, feature_seed = PNAE_SEEDS[(hidden, out_dim)] if family == "pnae" else (0, MOLHIV_SEED)
    b, ea = widths_batch(feature_seed, grid=family == "pnae")
    return widths_model(family, hidden, out_dim, layers, steps, model_seed), b, ea if family in W.EDGE_FAMILIES else None


@pytest.mark.parametrize("family,hidden,out_dim,layers,steps", CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in CASES])
def test_unlike_layer_widths(dev, family, hidden, out_dim, layers, steps):
    model, b, ea = widths_case(family, hidden, out_dim, layers, steps)
    edges = family in W.EDGE_FAMILIES
    widths = [(c.in_channels, c.out_channels) for c in model.gnn_convs]
    assert widths == ([(W.IN_DIM, out_dim)] if layers == 1 else [(W.IN_DIM, hidden), (hidden, hidden), (hidden, out_dim)]) and out_dim != hidden
    if family == "pnae":  # on the float64 reference alone, nothing excluded
        assert W.variances_near_the_threshold(model, b, b.x, ea) == 0
    ref, base = W.model_refs(family, model, b, ea)
    xd, cood, nptr, eptr = to_dev(b, dev)
    ead = _t(ea, dev) if edges else None
    eid, batch_dev = _t(W.grouped_mini_batch(b, ea)[0], dev), _t(batch_vector(b), dev)

    def run(scale):
        """forward, forward again, the prepared form and the PyG entry on a workspace of ``scale`` times the batch's size."""
        cm = runtime.CompiledModel.from_model(model, scale * b.num_graphs, scale * b.num_nodes, scale * b.num_edges)
        cm.enable_edge_ingest() if edges else cm.enable_ingest()  # (right after construction)
        forward = (lambda: cm.forward_edges(xd, ead, cood, nptr, eptr)) if edges else (lambda: cm.forward(xd, cood, nptr, eptr))
        out = forward().clone()
        assert cm.last_path() == "layerwise" and out.shape == (b.num_graphs, 19)
        cm.check()
        assert torch.equal(forward(), out), "a second call"
        cm.graph_prep(cood, nptr, eptr, b.num_nodes)
        assert torch.equal(cm.forward_prepared_edges(xd, ead) if edges else cm.forward_prepared(xd), out), "the prepared form"
        pyg = cm.forward_pyg_edges(xd, eid, ead, batch=batch_dev, num_graphs=b.num_graphs) if edges else \
            cm.forward_pyg(xd, eid, batch=batch_dev, num_graphs=b.num_graphs)
        assert torch.equal(pyg, out), "the PyG entry"
        assert cm.last_path() == "layerwise"
        cm.check()
        return out.cpu().numpy()

    got = run(1)
    entry = f"forward/widths/{family}-{hidden}-{out_dim}"
    e, e32, _ = R.errors(got, ref, base)
    print(f"{entry}: e = {e:.3e}, e32 = {e32:.3e}, e / e32 = {R.ratio(e, e32):.2f}")
    WORST[entry] = max(WORST.get(entry, 0.0), R.ratio(e, e32))
    R.budget(got, ref, base, what=entry)
    W.assert_same_bits({"out": run(3)}, {"out": got}, f"{entry}: a workspace of three times the capacities")
