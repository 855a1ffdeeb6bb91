"""Shared builders for the test-suite (models with the reference's default PyTorch init,
as gen_test_data.py:217 does, and seeded synthetic batches)."""
import numpy as np
import torch

import gnnbuilder_amd as gnnb
from gnnbuilder_amd import synthetic
from gnnbuilder_amd.batching import GraphBatch

CONVS = {"gcn": gnnb.GCNConv_GNNB, "gin": gnnb.GINConv_GNNB, "sage": gnnb.SAGEConv_GNNB, "pna": gnnb.PNAConv_GNNB}
ACTS = {"relu": torch.nn.ReLU, "gelu": torch.nn.GELU, "sigmoid": torch.nn.Sigmoid, "tanh": torch.nn.Tanh}


def make_model(conv="gcn", in_dim=11, hidden=128, layers=2, out_dim=None, act="relu", skip=True,
               pools=("add", "mean", "max"), mlp_hidden=64, mlp_layers=2, task_out=19, mlp_act="relu", seed=0):
    torch.manual_seed(seed)
    out_dim = hidden if out_dim is None else out_dim
    gw = in_dim if layers == 0 else out_dim
    model = gnnb.GNNModel(in_dim, None, hidden, layers, out_dim, CONVS[conv], ACTS[act], skip,
                          gnnb.GlobalPooling(list(pools)), gnnb.MLP(len(pools) * gw, task_out, mlp_hidden, mlp_layers,
                                                                   activation=ACTS[mlp_act]), None)
    # PyG initialises GCN's bias to zero; give every bias a value so it is exercised
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("bias"):
                p.uniform_(-0.1, 0.1)
    return model.eval()


def canon(model):
    return [p.numpy() for p in model.canonical_params()]


def to_dev(batch, dev):
    return (torch.from_numpy(batch.x).to(dev), torch.from_numpy(batch.coo).to(dev),
            torch.from_numpy(batch.node_ptr).to(dev), torch.from_numpy(batch.edge_ptr).to(dev))


def batch_vector(batch):
    return np.repeat(np.arange(batch.num_graphs), np.diff(batch.node_ptr)).astype(np.int64)


def hub_graph(n, fin, edges, seed):
    """``n`` nodes, ``edges`` edges into node 0 (duplicates) plus a ring."""
    rng = np.random.default_rng(seed)
    ring = np.stack([np.arange(n), (np.arange(n) + 1) % n], 1)
    hub = np.stack([rng.integers(1, n, edges), np.zeros(edges, np.int64)], 1)
    return rng.uniform(-1, 1, (n, fin)).astype(np.float32), np.concatenate([ring, hub]).astype(np.int32)


EMPTY = lambda fin: (np.zeros((0, fin), np.float32), np.zeros((0, 2), np.int32))  # noqa: E731
ONE = lambda fin: (np.full((1, fin), 0.5, np.float32), np.zeros((0, 2), np.int32))  # noqa: E731


def looped_graph(n, fin, seed):
    """A random graph of ``n`` nodes with explicit self loops (one node has two), duplicate edges and isolated nodes."""
    rng = np.random.default_rng(seed)
    e = rng.integers(0, n - 3, (3 * n, 2))  # (nodes n-3 .. n-1: no edge at all)
    loops = np.stack([np.arange(0, n - 3, 3)] * 2, 1)
    coo = np.concatenate([e, loops, loops[:1], e[:5]])
    return rng.uniform(-1, 1, (n, fin)).astype(np.float32), coo[rng.permutation(len(coo))].astype(np.int32)


def edge_batch(graphs, fin, seed, hub=True):
    """``graphs`` QM9-shaped molecules plus every edge the stage kernels must serve: a graph with explicit self loops,
    duplicate edges and isolated nodes, a 300-node graph with a hub of in-degree 1200 (``hub``), an empty and a one-node
    graph; features uniform(-1, 1) of width ``fin``."""
    from gnnbuilder_amd.batching import pack_graphs
    b = synthetic.make_batch("qm9", graphs, seed=seed)
    rng = np.random.default_rng(seed)
    gs = [(rng.uniform(-1, 1, (b.graph(g)[0].shape[0], fin)).astype(np.float32), b.graph(g)[1]) for g in range(b.num_graphs)]
    extra = [looped_graph(40, fin, seed), EMPTY(fin)] + ([hub_graph(300, fin, 1200, seed)] if hub else []) + [ONE(fin)]
    return pack_graphs(gs[:graphs // 2] + extra + gs[graphs // 2:])


STAR_IN_DEGREES = (0, 1, 3, 4, 5, 8, 9, 63, 64, 65, 66, 127, 128, 129, 257, 300, 1200)


def star_graph(n, fin, in_degrees, seed):
    """``n`` nodes; node ``i`` has exactly ``in_degrees[i]`` in-edges (none behind the list), sources drawn from the whole
    graph (duplicates and self loops occur), the edges shuffled."""
    rng = np.random.default_rng(seed)
    dst = np.repeat(np.arange(len(in_degrees)), in_degrees)
    coo = np.stack([rng.integers(0, n, len(dst)), dst], 1)
    return rng.uniform(-1, 1, (n, fin)).astype(np.float32), coo[rng.permutation(len(coo))].astype(np.int32)


def sweep_batch(graphs, fin, seed):
    """``graphs`` QM9-shaped molecules and three 400-node ``star_graph``s of ``STAR_IN_DEGREES`` -- the first graph, one near
    the middle (its list reversed: the long rows land in other lane groups) and the last graph -- with an empty and a
    one-node graph between the others; features uniform(-1, 1) of width ``fin``.  Returns (batch, the stars' graph ids)."""
    from gnnbuilder_amd.batching import pack_graphs
    b = synthetic.make_batch("qm9", graphs, seed=seed)
    rng = np.random.default_rng(seed + 1)
    gs = [(rng.uniform(-1, 1, (b.graph(g)[0].shape[0], fin)).astype(np.float32), b.graph(g)[1]) for g in range(b.num_graphs)]
    stars = [star_graph(400, fin, STAR_IN_DEGREES[::-1] if k == 1 else STAR_IN_DEGREES, seed + 10 + k) for k in range(3)]
    third, half = graphs // 3, graphs // 2
    parts = [stars[0]] + gs[:third] + [EMPTY(fin)] + gs[third:half] + [stars[1]] + gs[half:2 * third] + [ONE(fin)] + gs[2 * third:] \
        + [stars[2]]
    return pack_graphs(parts), np.array([0, half + 2, len(parts) - 1])


def sub_edge_rows(batch, graph_ids):
    """The edges of graphs ``graph_ids`` (increasing) as rows of ``batch.coo``, in ``sub_batch``'s order: what selects the
    sub-batch's rows of a per-edge array."""
    gids = np.asarray(graph_ids, np.int64)
    e0, esz = batch.edge_ptr[gids].astype(np.int64), np.diff(batch.edge_ptr).astype(np.int64)[gids]
    return np.repeat(e0 - np.concatenate([[0], np.cumsum(esz)[:-1]]), esz) + np.arange(esz.sum())


def grid_features(n, w, seed):
    """uniform(-1, 1) rounded to multiples of 1/4, plus noise below 1e-3: two messages of a column differ by < 2e-3 or by
    > 0.24, so no PNA variance lies near PyG's 1e-5 threshold (the std jumps there; float64 and fp32 could legitimately
    land on its two sides) -- and many lie below it, where the clamp decides."""
    rng = np.random.default_rng(seed)
    return (np.round(rng.uniform(-1, 1, (n, w)) * 4) / 4 + rng.uniform(-1e-3, 1e-3, (n, w))).astype(np.float32)


def _local_coo(batch):
    """The batch's edges with graph-local ids (``batch.coo`` minus each edge's graph start)."""
    return batch.coo.astype(np.int64) - np.repeat(batch.node_ptr[:-1].astype(np.int64), np.diff(batch.edge_ptr))[:, None]


def _assemble(sizes, esizes, lcoo):
    """A GraphBatch from per-graph node / edge counts and the concatenated graph-local edges; ``x`` has width 0 (features
    of huge batches live on the device: ``huge_x``)."""
    node_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    edge_ptr = np.concatenate([[0], np.cumsum(esizes)]).astype(np.int64)
    assert node_ptr[-1] < 2 ** 31 and edge_ptr[-1] < 2 ** 31
    coo = (lcoo + np.repeat(node_ptr[:-1], esizes)[:, None]).astype(np.int32)
    return GraphBatch(x=np.zeros((int(node_ptr[-1]), 0), np.float32), coo=np.ascontiguousarray(coo),
                      node_ptr=node_ptr.astype(np.int32), edge_ptr=edge_ptr.astype(np.int32))


def huge_batch(num_nodes, seed, shape="qm9", base_graphs=4096, place=()):
    """At least ``num_nodes`` nodes of whole graphs: a seeded ``synthetic.make_batch`` of ``base_graphs`` graphs tiled with
    offset arithmetic (no Python loop per graph).  ``place``: (node id, graph-local coo [e, 2], node count) triples in
    increasing node order; each graph is put where it straddles its node id (``id - first node = n // 2``) behind one
    edge-less filler graph that closes the gap.  ``x`` has width 0: ``huge_x`` makes the features."""
    b = synthetic.make_batch(shape, base_graphs, seed=seed)
    sizes0, esz0, lcoo0 = np.diff(b.node_ptr).astype(np.int64), np.diff(b.edge_ptr).astype(np.int64), _local_coo(b)
    reps = num_nodes // b.num_nodes + 2
    sizes, esz = np.tile(sizes0, reps), np.tile(esz0, reps)
    lcoo = np.tile(lcoo0, (reps, 1))
    nptr = np.concatenate([[0], np.cumsum(sizes)])
    eptr = np.concatenate([[0], np.cumsum(esz)])
    ps, pe, pc = [], [], []
    g, shift = 0, 0  # next tiled graph; nodes inserted in front of it so far
    for node, coo, n in place:
        start = int(node) - int(n) // 2
        g1 = int(np.searchsorted(nptr, start - shift, "right")) - 1  # the tiled graphs that end at or before `start`
        assert g1 >= g, "place: node ids too close together"
        ps.append(sizes[g:g1]), pe.append(esz[g:g1]), pc.append(lcoo[eptr[g]:eptr[g1]])
        gap = start - int(nptr[g1]) - shift
        if gap:
            ps.append([gap]), pe.append([0]), pc.append(np.zeros((0, 2), np.int64))
        coo = np.asarray(coo, np.int64).reshape(-1, 2)
        ps.append([n]), pe.append([len(coo)]), pc.append(coo)
        shift += gap + int(n)
        g = g1
    g1 = int(np.searchsorted(nptr, num_nodes - shift, "left"))
    ps.append(sizes[g:g1]), pe.append(esz[g:g1]), pc.append(lcoo[eptr[g]:eptr[g1]])
    out = _assemble(np.concatenate(ps).astype(np.int64), np.concatenate(pe).astype(np.int64), np.concatenate(pc))
    assert out.num_nodes >= num_nodes
    return out


def huge_x(num_nodes, width, seed, device="cpu"):
    """uniform(-1, 1) features [num_nodes, width] from their own seeded generator, made where they are used."""
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    return torch.empty((num_nodes, width), dtype=torch.float32, device=device).uniform_(-1.0, 1.0, generator=gen)


def sub_batch(batch, graph_ids):
    """Graphs ``graph_ids`` (increasing) of ``batch`` as a batch of their own, nodes and edges renumbered; returns
    (sub-batch, the sub-batch's nodes as ids of ``batch``).  ``x`` is taken along where ``batch`` has it."""
    gids = np.asarray(graph_ids, np.int64)
    assert np.all(np.diff(gids) > 0)
    n0, n1 = batch.node_ptr[gids].astype(np.int64), batch.node_ptr[gids + 1].astype(np.int64)
    e0, e1 = batch.edge_ptr[gids].astype(np.int64), batch.edge_ptr[gids + 1].astype(np.int64)
    sizes, esz = n1 - n0, e1 - e0
    ranges = lambda lo, cnt: np.repeat(lo - np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt) + np.arange(cnt.sum())  # noqa: E731
    rows, edges = ranges(n0, sizes), ranges(e0, esz)
    lcoo = batch.coo[edges].astype(np.int64) - np.repeat(n0, esz)[:, None]
    sub = _assemble(sizes, esz, lcoo)
    if batch.x.shape[1]:
        sub.x = np.ascontiguousarray(batch.x[rows])
    return sub, rows


def sample_graphs(batch, seed, count=256, nodes=()):
    """The graphs a test at scale checks: the first, the last, ``count`` seeded random ones and the ones holding node ids
    ``nodes`` and their neighbours on both sides (increasing, unique)."""
    B = batch.num_graphs
    g = [0, B - 1] + list(np.random.default_rng(seed).integers(0, B, count))
    for v in nodes:
        k = int(np.searchsorted(batch.node_ptr, v, "right")) - 1
        g += [max(k - 1, 0), k, min(k + 1, B - 1)]
    return np.unique(np.asarray(g, np.int64))


def oracle_tables_batched(batch: GraphBatch):
    """(row_ptr, col) of the whole batch from the oracle's per-graph tables."""
    from oracle import oracle as O

    row_ptr, cols = [0], []
    for g in range(batch.num_graphs):
        xg, cg = batch.graph(g)
        in_deg, _, offsets, nbrs = O.tables(cg, xg.shape[0])
        n0 = int(batch.node_ptr[g])
        for d in in_deg:
            row_ptr.append(row_ptr[-1] + int(d))
        cols.append(nbrs + n0)
    return np.asarray(row_ptr, np.int32), (np.concatenate(cols) if cols else np.zeros(0, np.int32)).astype(np.int32)
