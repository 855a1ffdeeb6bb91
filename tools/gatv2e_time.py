#!/usr/bin/env python3
"""Time of the GATv2 aggregate with edge features (csrc/k_gatv2_edge.hip) at the C3t batch: the batch of workload c3t (4096
``molhiv_tail`` graphs: heavy-tailed molecule sizes), width ``--width`` (128), heads 1 and 4, ``edge_dim`` 4 and 16.  Fails
without a GPU.

Four kinds of candidate that alternate inside every loop of one call:
  gatv2e_h{1,4}_d{4,16}  ``aggregate_gatv2_edges`` with bias: edge projection, scores, softmax and weighted sum in one pass over the
                         edges, ``xl`` / ``xr`` the two halves of one [N, 2 width] matrix, as a layer's GEMM leaves them
  gatv2_h1, gatv2_h4     ``aggregate_gatv2`` on the same operands and the same workspace, measured in the same run: the same gather
                         without the edge term -- the floor of the edge form
  sum                    ``aggregate("sum", xl)`` at the same width: the same rows gathered once, no score and no softmax
  torch_h{1,4}_d{4,16}   the unfused composition in torch on the GPU, what a user would run otherwise: the per-destination mean of
                         the attributes for the self loops, ``lin_edge`` over all E + N attribute rows (the [E + N, width] projected
                         edge term), ``index_select`` of xl_j and xr_i, ``leaky_relu``, the score, a scatter softmax and
                         ``index_add`` of the weighted rows
HIP events on the launch stream around ``--launches`` back-to-back launches of one candidate, microseconds per launch; median
over ``--loops`` loops, with the loop-to-loop spread (min, max), after a warm-up of every candidate.  ``*_us`` of the library's
candidates: the launches captured once into a HIP graph and replayed between the events -- the device's own time;
``*_eager_us``: the same launches issued from Python, which the host's enqueue rate can bound.  The torch composition is timed
eagerly only.  The fused kernel and the torch composition are compared (max |difference| relative to max |value|) before anything
is timed.  Bytes per launch are this tool's arithmetic from the shapes -- what the algorithm has to move, not a counter.  Context,
not an acceptance figure.

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

SLOPE = 0.2
HEADS, EDGE_DIMS = (1, 4), (4, 16)


def aggregate_bytes(N, E, width, edge_dim):
    """Bytes one launch has to move, from the shapes: the floor reads x_j per edge and x_i per node, the node records (32 B per
    node) and col (4 B per edge), and writes [N, width]; the attention form reads xr_i per node, att and bias on top; the edge
    form eid (4 B per edge), the attribute rows and W_e on top of that."""
    floor = 4 * width * (E + N) + 32 * N + 4 * E + 4 * width * N
    gat = floor + 4 * width * N + 8 * width
    return {"sum": floor, "gatv2": gat, "gatv2e": gat + 4 * E + 4 * edge_dim * E + 4 * width * edge_dim}


def torch_gatv2e(xl, xr, att, bias, ea, we, src, dst, edst, heads):
    """The layer behind its GEMM in plain torch ops; ``src`` / ``dst``: the edges without (v, v) rows, then one self loop per node;
    ``ea``: the kept edges' attribute rows, ``edst`` their destinations."""
    n, w = xl.shape
    c = w // heads
    deg = xl.new_zeros(n).index_add(0, edst, xl.new_ones(edst.numel()))
    loop = xl.new_zeros(n, ea.shape[1]).index_add(0, edst, ea) / deg.clamp(min=1).unsqueeze(-1)
    p = (torch.cat([ea, loop]) @ we.t()).view(-1, heads, c)
    xj = xl.index_select(0, src).view(-1, heads, c)
    z = torch.nn.functional.leaky_relu(xj + xr.index_select(0, dst).view(-1, heads, c) + p, SLOPE)
    s = (z * att.view(1, heads, c)).sum(-1)
    idx = dst.unsqueeze(-1).expand(-1, heads)
    smax = s.new_full((n, heads), float("-inf")).scatter_reduce(0, idx, s, reduce="amax", include_self=True)
    e = (s - smax.index_select(0, dst)).exp()
    a = e / (s.new_zeros(n, heads).index_add(0, dst, e).index_select(0, dst) + 1e-16)
    return xl.new_zeros(n, heads, c).index_add(0, dst, a.unsqueeze(-1) * xj).view(n, w) + bias


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
    model = gnnb.GNNModel(b.x.shape[1], 4, W, 3, W, gnnb.GATv2EConv_GNNB, torch.nn.ReLU, True, gnnb.GlobalPooling(["add", "mean", "max"]),
                          gnnb.MLP(3 * W, 1, 64, 2), None, gnn_heads=4).eval()
    cm = runtime.CompiledModel.from_model(model, B, N, E)  # (such a model's workspace is a GCN workspace)
    cm.graph_prep(to(b.coo), to(b.node_ptr), to(b.edge_ptr), N)
    lr = to(rng.uniform(-1, 1, (N, 2 * W)).astype(np.float32))
    xl, xr = lr[:, :W], lr[:, W:]
    att, bias = to(rng.uniform(-0.5, 0.5, W).astype(np.float32)), to(rng.uniform(-0.5, 0.5, W).astype(np.float32))
    ea = {d: to(rng.uniform(-1, 1, (E, d)).astype(np.float32)) for d in EDGE_DIMS}
    we = {d: to(rng.uniform(-0.5, 0.5, (W, d)).astype(np.float32)) for d in EDGE_DIMS}
    xs = xl.contiguous()
    keep = b.coo[:, 0] != b.coo[:, 1]
    kept = b.coo[keep]
    keep_dev = to(np.flatnonzero(keep).astype(np.int64))
    ea_kept = {d: ea[d].index_select(0, keep_dev) for d in EDGE_DIMS}
    loops = np.arange(N)
    src, dst = to(np.concatenate([kept[:, 0], loops]).astype(np.int64)), to(np.concatenate([kept[:, 1], loops]).astype(np.int64))
    edst = to(kept[:, 1].astype(np.int64))
    edge_names = [f"gatv2e_h{h}_d{d}" for h in HEADS for d in EDGE_DIMS]
    ours = edge_names + ["gatv2_h1", "gatv2_h4", "sum"]
    outs = {name: torch.empty((N, W), device=dev) for name in ours}

    def fused_edges(heads, d):
        return lambda: cm.aggregate_gatv2_edges(xl, xr, att, ea[d], we[d], bias=bias, heads=heads, negative_slope=SLOPE, out=outs[f"gatv2e_h{heads}_d{d}"])

    def fused(heads):
        return lambda: cm.aggregate_gatv2(xl, xr, att, bias=bias, heads=heads, negative_slope=SLOPE, out=outs[f"gatv2_h{heads}"])

    def composed(heads, d):
        return lambda: torch_gatv2e(xl, xr, att, bias, ea_kept[d], we[d], src, dst, edst, heads)

    calls = {f"gatv2e_h{h}_d{d}": fused_edges(h, d) for h in HEADS for d in EDGE_DIMS}
    calls.update({"gatv2_h1": fused(1), "gatv2_h4": fused(4), "sum": lambda: cm.aggregate("sum", xs, out=outs["sum"])})
    calls.update({f"torch_h{h}_d{d}": composed(h, d) for h in HEADS for d in EDGE_DIMS})
    # the fused kernel and the composition compute the same layer
    diffs = {}
    for h in HEADS:
        for d in EDGE_DIMS:
            want = calls[f"torch_h{h}_d{d}"]()
            got = calls[f"gatv2e_h{h}_d{d}"]()
            diffs[f"h{h}_d{d}"] = float((got - want).abs().max() / want.abs().max())
            assert diffs[f"h{h}_d{d}"] < 1e-5, diffs
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
    nbytes = {d: aggregate_bytes(N, E, W, d) for d in EDGE_DIMS}
    res = {"workload": args.workload, "shape": w["shape"], "graphs": B, "nodes": N, "edges": E, "edges_without_self_loops": int(len(kept)),
           "max_in_degree": int(np.bincount(kept[:, 1]).max()), "width": W, "negative_slope": SLOPE, "launches": args.launches, "loops": args.loops,
           "device": torch.cuda.get_device_name(0), "fused_vs_torch_rel_diff": diffs, "bytes": {f"d{d}": v for d, v in nbytes.items()}}
    for name in ours:
        t = times[name]
        kind = "sum" if name == "sum" else "gatv2e" if name.startswith("gatv2e") else "gatv2"
        d = int(name.rsplit("_d", 1)[1]) if kind == "gatv2e" else EDGE_DIMS[0]
        res[f"{name}_us"] = round(statistics.median(t), 2)
        res[f"{name}_us_min_max"] = [round(min(t), 2), round(max(t), 2)]
        res[f"{name}_GBps"] = round(nbytes[d][kind] / statistics.median(t) / 1e3, 1)
    for name, t in eager.items():
        res[f"{name}_eager_us"] = round(statistics.median(t), 2)
        res[f"{name}_eager_us_min_max"] = [round(min(t), 2), round(max(t), 2)]
    for h in HEADS:
        for d in EDGE_DIMS:
            res[f"gatv2e_h{h}_d{d}_over_gatv2_h{h}"] = round(res[f"gatv2e_h{h}_d{d}_us"] / res[f"gatv2_h{h}_us"], 3)
            res[f"torch_h{h}_d{d}_over_gatv2e_h{h}_d{d}"] = round(res[f"torch_h{h}_d{d}_eager_us"] / res[f"gatv2e_h{h}_d{d}_us"], 2)
    cm.check()
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
