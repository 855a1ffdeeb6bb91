#!/usr/bin/env python3
"""Time of PNA's edge aggregate (csrc/k_pna_edge.hip) beside the plain PNA aggregate at the C4-tail shape: the batch of workload
c3t (4096 ``molhiv_tail`` graphs: heavy-tailed molecule sizes) at the width of workload c4's PNA layers, ``--width`` (128),
``--edge-dim`` (4).  Fails without a GPU.

Two candidates that alternate inside every loop of one call:
  pna_edge  ``aggregate_pna_edges``: max | min | mean | std of q_i + p_j + (W_e e_ij + b_e), the projection formed in the kernel
  plain     ``aggregate("pna", p, self_term=q)``: the same gather and the same four statistics of q_i + p_j, without the edge
            term -- the floor (k_aggregate.hip's ring form, which stages whole graphs in LDS)
HIP events on the launch stream around ``--launches`` back-to-back launches of one candidate, microseconds per launch; median
over ``--loops`` loops, with the loop-to-loop spread (min, max).  ``*_us``: the launches captured once into a HIP graph and
replayed between the events -- the device's own time; ``*_eager_us``: the same launches issued from Python, which the host's
enqueue rate can bound.  With W_e = 0 and b_e = 0 the two compute the same statistics: max, min and mean are compared (max
|difference| relative to max |value|) before anything is timed.  Bytes per launch are this tool's arithmetic from the shapes -- what the algorithm has to
move, not a counter.  Context, not an acceptance figure.

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


def aggregate_bytes(N, E, width, edge_dim):
    """Bytes one launch has to move, from the shapes: both read p_j per edge and q_i per node, the node records (32 B per node)
    and col (4 B per edge), and write [N, 4 width]; the edge form also reads eid (4 B per edge), the attribute rows and W_e, b_e."""
    plain = 4 * width * (E + N) + 32 * N + 4 * E + 16 * width * N
    return {"plain": plain, "pna_edge": plain + 4 * E + 4 * E * edge_dim + 4 * width * (edge_dim + 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="c3t", help="the batch's workload in bench.WORKLOADS (its shape and batch size)")
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--edge-dim", type=int, default=4)
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
    W, ED = args.width, args.edge_dim
    rng = np.random.default_rng(0)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    torch.manual_seed(0)
    model = gnnb.GNNModel(b.x.shape[1], ED, W, 3, W, gnnb.PNAEConv_GNNB, torch.nn.ReLU, True, gnnb.GlobalPooling(["add", "mean", "max"]),
                          gnnb.MLP(3 * W, 1, 64, 2), None).eval()
    cm = runtime.CompiledModel.from_model(model, B, N, E)
    cm.graph_prep(to(b.coo), to(b.node_ptr), to(b.edge_ptr), N)
    p, q = to(rng.uniform(-1, 1, (N, W)).astype(np.float32)), to(rng.uniform(-1, 1, (N, W)).astype(np.float32))
    ea = to(rng.uniform(-1, 1, (E, ED)).astype(np.float32))
    we, be = to(rng.uniform(-0.5, 0.5, (W, ED)).astype(np.float32)), to(rng.uniform(-0.5, 0.5, W).astype(np.float32))
    out_e, out_p = torch.empty((N, 4 * W), device=dev), torch.empty((N, 4 * W), device=dev)

    def pna_edge():
        cm.aggregate_pna_edges(p, q, ea, we, be, out=out_e)

    def plain():
        cm.aggregate("pna", p, self_term=q, out=out_p)

    # without an edge term the two are the same statistics of the same messages
    cm.aggregate_pna_edges(p, q, ea, torch.zeros_like(we), torch.zeros_like(be), out=out_e)
    plain()
    cm.check()
    # (max | min | mean: PyG's std jumps at a variance of 1e-5, where two fp32 evaluations may land on two sides)
    diff = float((out_e[:, :3 * W] - out_p[:, :3 * W]).abs().max() / out_p[:, :3 * W].abs().max())
    assert diff < 1e-5, diff
    timer = runtime.HipTimer()
    for _ in range(10):  # warm-up of both
        pna_edge(), plain()
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

    graphs = {"pna_edge": captured(pna_edge), "plain": captured(plain)}
    times = alternate({name: g.replay for name, g in graphs.items()})
    eager = alternate({"pna_edge": eagerly(pna_edge), "plain": eagerly(plain)})
    res = {"workload": args.workload, "shape": w["shape"], "graphs": B, "nodes": N, "edges": E, "max_in_degree": int(np.bincount(b.coo[:, 1]).max()),
           "width": W, "edge_dim": ED, "launches": args.launches, "loops": args.loops, "device": torch.cuda.get_device_name(0),
           "aggregate_rel_diff_without_edge_term": diff, "bytes": aggregate_bytes(N, E, W, ED)}
    for name, t in times.items():
        res[f"{name}_us"] = round(statistics.median(t), 2)
        res[f"{name}_us_min_max"] = [round(min(t), 2), round(max(t), 2)]
        res[f"{name}_GBps"] = round(res["bytes"][name] / statistics.median(t) / 1e3, 1)
        res[f"{name}_eager_us"] = round(statistics.median(eager[name]), 2)
    res["pna_edge_over_plain"] = round(res["pna_edge_us"] / res["plain_us"], 3)
    res["bytes_pna_edge_over_plain"] = round(res["bytes"]["pna_edge"] / res["bytes"]["plain"], 3)
    cm.check()
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
