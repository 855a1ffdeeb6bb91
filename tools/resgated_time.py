#!/usr/bin/env python3
"""Time of the ResGatedGraphConv aggregate (csrc/k_resgated.hip) at the C3t batch: the batch of workload c3t (4096
``molhiv_tail`` graphs: heavy-tailed molecule sizes), width ``--width`` (128).  Fails without a GPU.

Five candidates that alternate inside every loop of one call, all on the same batch and the same workspace -- a
ResGatedGraphConv model's (a GIN description: the tables keep explicit self loops):
  resgated     ``aggregate_resgated`` with root: the per-column sigmoid gate and the gated sum of the value rows in one pass over the
               edges, ``k`` / ``q`` / ``v`` / ``root`` the four column blocks of one [N, 4 width] matrix, as a layer's GEMM leaves
               them
  transformer  ``aggregate_transformer`` (heads 1) with root on the same four blocks: the same two gathers per edge, with the score's
               cross-lane sum and the online softmax state on top
  gine         ``aggregate_edges_fused`` (GINE, ``edge_dim`` 4) at the same width: one gather per edge, an elementwise nonlinear
               message formed from the edge's attributes
  sum          ``aggregate("sum", x)`` at the same width: the same rows gathered once, nothing else -- the floor
  torch        the unfused composition in torch on the GPU, what a user would run otherwise: ``index_select`` x 3, add,
               ``sigmoid``, multiply, ``index_add``, add, over the batch's edges
HIP events on the launch stream around ``--launches`` back-to-back launches of one candidate, microseconds per launch; median
over ``--loops`` loops, with the loop-to-loop spread (min, max), after a warm-up of every candidate.  ``*_us`` of the library's
candidates: the launches captured once into a HIP graph and replayed between the events -- the device's own time;
``*_eager_us``: the same launches issued from Python, which the host's enqueue rate can bound.  The torch composition is timed
eagerly only (eight kernels per call, each long enough to keep the queue full at this size).  The fused kernel and the torch
composition are compared (max |difference| relative to max |value|) before anything is timed.  Bytes per launch are this tool's
arithmetic from the shapes -- what the algorithm has to move, not a counter.  The ratios to the floor and to
``aggregate_transformer`` are context; the one condition this tool holds is that the fused stage is faster than the torch
composition of the same run.

``--out FILE`` also writes the JSON line to a file."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import gnnbuilder_amd as gnnb  # noqa: E402
from gnnbuilder_amd import runtime, synthetic  # noqa: E402

EDGE_DIM = 4


def aggregate_bytes(N, E, width):
    """Bytes one launch has to move, from the shapes: the floor reads x_j per edge, the node records (32 B per node) and col
    (4 B per edge), and writes [N, width]; GINE reads x_i per node, the edge's attributes and its row index (4 B) on top; the
    gated and the dot-product forms read TWO rows per edge and two per node (k_i or q_i, and root_i).  The torch composition
    writes and re-reads its [E, width] intermediates: not counted here."""
    tables = 32 * N + 4 * E
    two = 8 * width * E + tables + 12 * width * N
    return {"sum": 4 * width * E + tables + 4 * width * N, "gine": 4 * width * (E + N) + tables + 4 * width * N + (4 * EDGE_DIM + 4) * E,
            "resgated": two, "transformer": two}


def torch_resgated(k, q, v, root, src, dst):
    """The layer behind its GEMM in plain torch ops; ``src`` / ``dst``: the batch's edges as they are."""
    g = torch.sigmoid(k.index_select(0, dst) + q.index_select(0, src))
    return torch.zeros_like(root).index_add(0, dst, g * v.index_select(0, src)) + root


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="c3t", help="the batch's workload in bench.WORKLOADS (its shape and batch size)")
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--loops", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.launches < 50 or args.loops < 5:
        ap.error("at least five loops of at least 50 launches")

    runtime.load_library(require_gpu=True)  # fails loudly: no fallback
    w = bench.WORKLOADS[args.workload]
    dev = torch.device("cuda:0")
    b = synthetic.make_batch(w["shape"], w["batch"], seed=0)
    B, N, E = b.num_graphs, b.num_nodes, b.num_edges
    W = args.width
    rng = np.random.default_rng(0)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    torch.manual_seed(0)
    model = gnnb.GNNModel(b.x.shape[1], None, W, 3, W, gnnb.ResGatedGraphConv_GNNB, torch.nn.ReLU, True,
                          gnnb.GlobalPooling(["add", "mean", "max"]), gnnb.MLP(3 * W, 1, 64, 2), None).eval()
    cm = runtime.CompiledModel.from_model(model, B, N, E)  # (a GIN description: explicit self loops stay)
    cood, nptr, eptr = to(b.coo), to(b.node_ptr), to(b.edge_ptr)
    cm.graph_prep(cood, nptr, eptr, N)
    kqvr = to(rng.uniform(-1, 1, (N, 4 * W)).astype(np.float32))
    k, q, v, root = (kqvr[:, i * W:(i + 1) * W] for i in range(4))
    xs = q.contiguous()
    ea = to(rng.uniform(-1, 1, (E, EDGE_DIM)).astype(np.float32))
    we, be = to(rng.uniform(-0.5, 0.5, (W, EDGE_DIM)).astype(np.float32)), to(rng.uniform(-0.5, 0.5, W).astype(np.float32))
    src, dst = to(b.coo[:, 0].astype(np.int64)), to(b.coo[:, 1].astype(np.int64))
    ours = ("resgated", "transformer", "gine", "sum")
    outs = {name: torch.empty((N, W), device=dev) for name in ours}
    calls = {"resgated": lambda: cm.aggregate_resgated(k, q, v, root=root, out=outs["resgated"]),
             "transformer": lambda: cm.aggregate_transformer(k, q, v, root=root, heads=1, out=outs["transformer"]),
             "gine": lambda: cm.aggregate_edges_fused(xs, ea, we, be, eps=0.1, out=outs["gine"]),
             "sum": lambda: cm.aggregate("sum", xs, out=outs["sum"]),
             "torch": lambda: torch_resgated(k, q, v, root, src, dst)}
    # the fused kernel and the composition compute the same layer
    want = calls["torch"]()
    got = calls["resgated"]()
    diff = float((got - want).abs().max() / want.abs().max())
    assert diff < 1e-5, diff
    cm.check()
    timer = runtime.HipTimer()
    for _ in range(10):  # warm-up of every candidate
        for call in calls.values():
            call()
    torch.cuda.synchronize()

    def captured(call):
        """``--launches`` launches of ``call`` as one HIP graph."""
        side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            for _ in range(args.launches):
                call()
        graph.replay()  # (warm-up of the graph itself)
        torch.cuda.synchronize()
        return graph

    def eagerly(call):
        def run():
            for _ in range(args.launches):
                call()
        return run

    def alternate(runs):
        t = {name: [] for name in runs}
        for _ in range(args.loops):
            for name, run in runs.items():  # (the candidates alternate inside the loop)
                timer.start()
                run()
                timer.stop()
                t[name].append(timer.elapsed_ms() * 1000.0 / args.launches)
        return t

    graphs = {name: captured(calls[name]) for name in ours}
    times = alternate({name: g.replay for name, g in graphs.items()})
    eager = alternate({name: eagerly(call) for name, call in calls.items()})
    nbytes = aggregate_bytes(N, E, W)
    res = {"workload": args.workload, "shape": w["shape"], "graphs": B, "nodes": N, "edges": E,
           "explicit_self_loops": int((b.coo[:, 0] == b.coo[:, 1]).sum()), "max_in_degree": int(np.bincount(b.coo[:, 1]).max()), "width": W,
           "edge_dim_gine": EDGE_DIM, "launches": args.launches, "loops": args.loops, "device": torch.cuda.get_device_name(0),
           "fused_vs_torch_rel_diff": diff, "bytes": nbytes}
    for name in ours:
        t = times[name]
        res[f"{name}_us"] = round(statistics.median(t), 2)
        res[f"{name}_us_min_max"] = [round(min(t), 2), round(max(t), 2)]
        res[f"{name}_GBps"] = round(nbytes[name] / statistics.median(t) / 1e3, 1)
    for name, t in eager.items():
        res[f"{name}_eager_us"] = round(statistics.median(t), 2)
        res[f"{name}_eager_us_min_max"] = [round(min(t), 2), round(max(t), 2)]
    res["resgated_over_sum"] = round(res["resgated_us"] / res["sum_us"], 3)
    res["resgated_over_transformer"] = round(res["resgated_us"] / res["transformer_us"], 3)
    res["resgated_over_gine"] = round(res["resgated_us"] / res["gine_us"], 3)
    res["torch_over_resgated"] = round(res["torch_eager_us"] / res["resgated_us"], 2)
    cm.check()
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    # the one condition: in the same run, eager against eager as well as against the device's own time
    assert res["resgated_eager_us"] < res["torch_eager_us"] and res["resgated_us"] < res["torch_eager_us"], res


if __name__ == "__main__":
    main()
