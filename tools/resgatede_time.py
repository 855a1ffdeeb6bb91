#!/usr/bin/env python3
"""Time of the ResGatedGraphConv aggregate with edge features (csrc/k_resgated_edge.hip) at the C3t batch: the batch of workload
c3t (4096 ``molhiv_tail`` graphs: heavy-tailed molecule sizes), width ``--width`` (128), ``edge_dim`` 4 and 16.  Fails without a GPU.

The candidates alternate inside every loop of one call, all on the same batch and the same workspace -- a ResGatedGraphConv
model's (a GIN description: the tables keep explicit self loops):
  resgatede_d  ``aggregate_resgated_edges`` with root at ``edge_dim`` d: the gate with its edge term and the gated sum of the value
               rows with theirs in one pass over the edges, ``k`` / ``q`` / ``v`` / ``root`` the four column blocks of one
               [N, 4 width] matrix and ``w_gate`` / ``w_value`` the two row blocks of one [2 width, d] matrix, as a layer has them
  resgated     ``aggregate_resgated`` with root on the same four blocks: the same two row gathers per edge without the edge term --
               the floor of this kernel
  gine_d       ``aggregate_edges_fused`` (GINE) at the same width and ``edge_dim``: one row gather per edge, d FMAs per (edge,
               column) from the edge's attributes
  sum          ``aggregate("sum", x)`` at the same width: the same rows gathered once, nothing else
  torch_d      the unfused composition of the same layer behind its GEMM in torch on the GPU, what a user would run otherwise:
               ``index_select`` x 3, two [E, d] x [d, width] products, adds, ``sigmoid``, multiply, ``index_add``, add
HIP events on the launch stream around ``--launches`` back-to-back launches of one candidate, microseconds per launch; median
over ``--loops`` loops, with the loop-to-loop spread (min, max), after a warm-up of every candidate.  ``*_us`` of the library's
candidates: the launches captured once into a HIP graph and replayed between the events -- the device's own time;
``*_eager_us``: the same launches issued from Python, which the host's enqueue rate can bound.  The torch composition is timed
eagerly only.  The fused kernel and the torch composition are compared (max |difference| relative to max |value|) at both
``edge_dim`` before anything is timed.  The distance to the floor is reported, not promised; the one condition this tool holds is
that the fused stage is faster than the torch composition of the same run, at both ``edge_dim``.

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

EDGE_DIMS = (4, 16)


def torch_resgatede(k, q, v, root, ea, wg, wv, src, dst):
    """The layer behind its GEMM in plain torch ops; ``src`` / ``dst``: the batch's edges as they are."""
    g = torch.sigmoid(k.index_select(0, dst) + q.index_select(0, src) + ea @ wg.t())
    return torch.zeros_like(root).index_add(0, dst, g * (v.index_select(0, src) + ea @ wv.t())) + root


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
    src, dst = to(b.coo[:, 0].astype(np.int64)), to(b.coo[:, 1].astype(np.int64))
    ea, gv, be = {}, {}, to(rng.uniform(-0.5, 0.5, W).astype(np.float32))
    for d in EDGE_DIMS:
        ea[d] = to(rng.uniform(-1, 1, (E, d)).astype(np.float32))
        gv[d] = to(rng.uniform(-0.5, 0.5, (2 * W, d)).astype(np.float32))
    ours = tuple(f"resgatede_{d}" for d in EDGE_DIMS) + ("resgated",) + tuple(f"gine_{d}" for d in EDGE_DIMS) + ("sum",)
    outs = {name: torch.empty((N, W), device=dev) for name in ours}
    calls = {"resgated": lambda: cm.aggregate_resgated(k, q, v, root=root, out=outs["resgated"]),
             "sum": lambda: cm.aggregate("sum", xs, out=outs["sum"])}
    for d in EDGE_DIMS:
        calls[f"resgatede_{d}"] = lambda d=d: cm.aggregate_resgated_edges(k, q, v, ea[d], gv[d][:W], gv[d][W:], root=root,
                                                                          out=outs[f"resgatede_{d}"])
        calls[f"gine_{d}"] = lambda d=d: cm.aggregate_edges_fused(xs, ea[d], gv[d][:W], be, eps=0.1, out=outs[f"gine_{d}"])
        calls[f"torch_{d}"] = lambda d=d: torch_resgatede(k, q, v, root, ea[d], gv[d][:W], gv[d][W:], src, dst)
    # the fused kernel and the composition compute the same layer
    diffs = {}
    for d in EDGE_DIMS:
        want, got = calls[f"torch_{d}"](), calls[f"resgatede_{d}"]()
        diffs[d] = float((got - want).abs().max() / want.abs().max())
        assert diffs[d] < 1e-5, (d, diffs[d])
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
    res = {"workload": args.workload, "shape": w["shape"], "graphs": B, "nodes": N, "edges": E,
           "explicit_self_loops": int((b.coo[:, 0] == b.coo[:, 1]).sum()), "max_in_degree": int(np.bincount(b.coo[:, 1]).max()), "width": W,
           "edge_dims": list(EDGE_DIMS), "launches": args.launches, "loops": args.loops, "device": torch.cuda.get_device_name(0),
           "fused_vs_torch_rel_diff": {str(d): diffs[d] for d in EDGE_DIMS}}
    for name in ours:
        t = times[name]
        res[f"{name}_us"] = round(statistics.median(t), 2)
        res[f"{name}_us_min_max"] = [round(min(t), 2), round(max(t), 2)]
    for name, t in eager.items():
        res[f"{name}_eager_us"] = round(statistics.median(t), 2)
        res[f"{name}_eager_us_min_max"] = [round(min(t), 2), round(max(t), 2)]
    for d in EDGE_DIMS:
        res[f"resgatede_{d}_minus_floor_us"] = round(res[f"resgatede_{d}_us"] - res["resgated_us"], 2)
        res[f"resgatede_{d}_over_floor"] = round(res[f"resgatede_{d}_us"] / res["resgated_us"], 3)
        res[f"resgatede_{d}_over_gine"] = round(res[f"resgatede_{d}_us"] / res[f"gine_{d}_us"], 3)
        res[f"torch_{d}_over_resgatede"] = round(res[f"torch_{d}_eager_us"] / res[f"resgatede_{d}_us"], 2)
    cm.check()
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    # the one condition: in the same run, eager against eager as well as against the device's own time, at both edge_dim
    for d in EDGE_DIMS:
        assert res[f"resgatede_{d}_eager_us"] < res[f"torch_{d}_eager_us"] and res[f"resgatede_{d}_us"] < res[f"torch_{d}_eager_us"], (d, res)


if __name__ == "__main__":
    main()
