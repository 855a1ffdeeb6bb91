#!/usr/bin/env python3
"""Time of GINE's edge aggregate and of a whole GINE forward at the heavy-tailed molecule shape (workload c3t: 4096
``molhiv_tail`` graphs), width ``--width`` (128), ``--edge-dim`` (4).  Fails without a GPU.

(a) the aggregate, two candidates that alternate inside every loop of one call:
  fused       ``aggregate_edges_fused`` (csrc/k_gine.hip): the projection W_e e + b_e inside the aggregate kernel
  two_kernel  ``linear`` over the [E, edge_dim] edge features, then ``aggregate_edges`` on the [E, width] matrix it wrote
              (what ``CompiledModel.gine_conv`` runs; not tuned here)
HIP events on the launch stream around ``--launches`` back-to-back launches of one candidate, microseconds per launch; median
over ``--loops`` loops, with the loop-to-loop spread (min, max).  ``*_us``: the launches captured once into a HIP graph and
replayed between the events -- the device's own time; ``*_eager_us``: the same launches issued from Python, which the host's
enqueue rate can bound (one call against two).  The two agree (fp32 budget against float64 on sampled rows
is the tests' business; here: max |difference| relative to max |value|) before anything is timed.  Bytes per launch are this
tool's arithmetic from the shapes -- what the algorithm has to move, not a counter.

(b) the whole forward, wall clock of calls that end in a synchronise: a 3-layer GINE model through ``forward_pyg_edges`` beside
the same model shape as plain GIN through ``forward_pyg`` without a promise (the layer-wise route): what edge features cost.
Context, not an acceptance figure.

``--out FILE`` also writes the JSON line to a file."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import gnnbuilder_amd as gnnb  # noqa: E402
from gnnbuilder_amd import runtime, synthetic  # noqa: E402


def aggregate_bytes(N, E, width, edge_dim):
    """Bytes one launch has to move, from the shapes: every route reads x_j per edge and x_i per node, the CSR tables (node
    records 32 B per node, col and eid 4 B per edge each) and writes [N, width]."""
    common = 4 * width * (E + 2 * N) + 32 * N + 8 * E
    weights = 4 * width * (edge_dim + 1)
    return {"fused": common + 4 * E * edge_dim + weights,
            "two_kernel": common + (4 * E * edge_dim + weights + 4 * E * width) + 4 * E * width,  # (GEMM: read e, write p; aggregate: read p)
            "projected_edge_term": 4 * E * width}


def build(conv, f_in, edge_dim, width, layers, out):
    torch.manual_seed(0)
    return gnnb.GNNModel(f_in, edge_dim, width, layers, width, conv, torch.nn.ReLU, True, gnnb.GlobalPooling(["add"]),
                         gnnb.MLP(width, out, 64, 2), None).eval()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="c3t")
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--edge-dim", type=int, default=4)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--loops", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20, help="calls per loop of the whole-forward leg")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.launches < 50 or args.loops < 5:
        ap.error("at least five loops of at least 50 launches")

    runtime.load_library(require_gpu=True)  # fails loudly: no fallback
    w = bench.WORKLOADS[args.workload]
    dev = torch.device("cuda:0")
    b = synthetic.make_batch(w["shape"], w["batch"], seed=0)
    B, N, E = b.num_graphs, b.num_nodes, b.num_edges
    W, ED, f_in = args.width, args.edge_dim, b.x.shape[1]
    rng = np.random.default_rng(0)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    gine = runtime.CompiledModel.from_model(build(gnnb.GINEConv_GNNB, f_in, ED, W, w["layers"], 1), B, N, E)
    gine.enable_edge_ingest()
    gin = runtime.CompiledModel.from_model(build(gnnb.GINConv_GNNB, f_in, None, W, w["layers"], 1), B, N, E)
    gin.enable_ingest()
    coo, nptr, eptr = to(b.coo), to(b.node_ptr), to(b.edge_ptr)
    ea = to(rng.uniform(-1, 1, (E, ED)).astype(np.float32))

    # ---- (a) the aggregate at [N, width]
    h = to(rng.uniform(-1, 1, (N, W)).astype(np.float32))
    we, be = to(rng.uniform(-0.5, 0.5, (W, ED)).astype(np.float32)), to(rng.uniform(-0.5, 0.5, W).astype(np.float32))
    gine.graph_prep(coo, nptr, eptr, N)
    out_f, out_t = torch.empty_like(h), torch.empty_like(h)
    pe = torch.empty((E, W), dtype=torch.float32, device=dev)

    def fused():
        gine.aggregate_edges_fused(h, ea, we, be, eps=0.1, out=out_f)

    def two_kernel():
        runtime.linear([(ea, None)], we, be, out=pe)
        gine.aggregate_edges(h, pe, eps=0.1, out=out_t)

    fused(), two_kernel()
    gine.check()
    diff = float((out_f - out_t).abs().max() / out_t.abs().max())
    assert diff < 1e-5, diff  # (two fp32 evaluations of the same sums: the projection in another order)
    timer = runtime.HipTimer()
    for _ in range(10):  # warm-up of both
        fused(), two_kernel()
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

    graphs = {"fused": captured(fused), "two_kernel": captured(two_kernel)}
    times = alternate({name: g.replay for name, g in graphs.items()})
    eager = alternate({"fused": eagerly(fused), "two_kernel": eagerly(two_kernel)})
    res = {"workload": args.workload, "shape": w["shape"], "graphs": B, "nodes": N, "edges": E, "max_in_degree": int(np.bincount(b.coo[:, 1]).max()),
           "width": W, "edge_dim": ED, "launches": args.launches, "loops": args.loops, "device": torch.cuda.get_device_name(0),
           "aggregate_rel_diff": diff, "bytes": aggregate_bytes(N, E, W, ED)}
    for name, t in times.items():
        res[f"{name}_us"] = round(statistics.median(t), 2)
        res[f"{name}_us_min_max"] = [round(min(t), 2), round(max(t), 2)]
        res[f"{name}_GBps"] = round(res["bytes"][name] / statistics.median(t) / 1e3, 1)
        res[f"{name}_eager_us"] = round(statistics.median(eager[name]), 2)
    res["fused_over_two_kernel"] = round(res["fused_us"] / res["two_kernel_us"], 3)

    # ---- (b) the whole forward from the loader's tensors
    x = to(b.x)
    ei = to(b.coo.T.astype(np.int64))
    batch = to(np.repeat(np.arange(B), np.diff(b.node_ptr)).astype(np.int64))

    def wall_us(call):
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        per_call = []
        for _ in range(args.loops):
            t0 = time.perf_counter()
            for _ in range(args.calls):
                call()
                torch.cuda.synchronize()
            per_call.append((time.perf_counter() - t0) * 1e6 / args.calls)
        return round(statistics.median(per_call), 1), [round(min(per_call), 1), round(max(per_call), 1)]

    walls = {"forward_pyg_edges_gine": lambda: gine.forward_pyg_edges(x, ei, ea, batch=batch, num_graphs=B),
             "forward_pyg_gin_layerwise": lambda: gin.forward_pyg(x, ei, batch=batch, num_graphs=B)}
    for name, call in walls.items():
        res[f"{name}_us"], res[f"{name}_us_min_max"] = wall_us(call)
    res["gine_path"], res["gin_path"] = gine.last_path(), gin.last_path()
    gine.check(), gin.check()
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
