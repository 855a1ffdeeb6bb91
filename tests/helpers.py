"""Shared builders for the test-suite (models with the reference's default PyTorch init,
as gen_test_data.py:217 does, and seeded synthetic batches)."""
import numpy as np
import torch

import gnnbuilder_amd as gnnb
from gnnbuilder_amd import synthetic

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


def grid_features(n, w, seed):
    """uniform(-1, 1) rounded to multiples of 1/4, plus noise below 1e-3: two messages of a column differ by < 2e-3 or by
    > 0.24, so no PNA variance lies near PyG's 1e-5 threshold (the std jumps there; float64 and fp32 could legitimately
    land on its two sides) -- and many lie below it, where the clamp decides."""
    rng = np.random.default_rng(seed)
    return (np.round(rng.uniform(-1, 1, (n, w)) * 4) / 4 + rng.uniform(-1e-3, 1e-3, (n, w))).astype(np.float32)
