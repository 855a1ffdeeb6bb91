#!/usr/bin/env python3
"""Time of the TransformerConv aggregate (csrc/k_transformer.hip) at the C3t batch: the batch of workload c3t (4096
``molhiv_tail`` graphs: heavy-tailed molecule sizes), width ``--width`` (128), heads 1 and 4.  Fails without a GPU.

Four kinds of candidate that alternate inside every loop of one call, all on the same batch:
  tf_h1, tf_h4        ``aggregate_transformer`` with root: dot-product scores, softmax and the weighted sum of the value rows in one
                      pass over the edges, ``q`` / ``k`` / ``v`` / ``root`` the four column blocks of one [N, 4 width] matrix, as a
                      layer's GEMM leaves them; on the workspace of a TransformerConv model (a GIN description: the tables keep
                      explicit self loops)
  gatv2_h1, gatv2_h4  ``aggregate_gatv2`` with bias at the same width, ``xl`` / ``xr`` column blocks of the same matrix, on the
                      workspace of a GATv2 model (a GCN description) prepared with the same batch: ONE gather per edge where the
                      dot-product form has two
  sum                 ``aggregate("sum", x)`` at the same width on the TransformerConv workspace: the same rows gathered once, no
                      score and no softmax -- the floor
  torch_h1, torch_h4  the unfused composition in torch on the GPU, what a user would run otherwise: ``index_select`` of q_i, k_j
                      and v_j, the scaled dot product, a scatter softmax (``scatter_reduce`` amax, ``exp``, ``index_add``, a divide)
                      and ``index_add`` of the weighted rows, over the batch's edges
HIP events on the launch stream around ``--launches`` back-to-back launches of one candidate, microseconds per launch; median
over ``--loops`` loops, with the loop-to-loop spread (min, max), after a warm-up of every candidate.  ``*_us`` of the library's
candidates: the launches captured once into a HIP graph and replayed between the events -- the device's own time;
``*_eager_us``: the same launches issued from Python, which the host's enqueue rate can bound.  The torch composition is timed
eagerly only (a dozen kernels per call, each long enough to keep the queue full at this size).  The fused kernel and the torch
composition are compared (max |difference| relative to max |value|) before anything is timed.  Bytes per launch are this tool's
arithmetic from the shapes -- what the algorithm has to move, not a counter.  The ratios to ``aggregate_gatv2`` and to the floor
are context; the one condition this tool holds is that the fused stage is faster than the torch composition of the same run.

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


def aggregate_bytes(N, E, width):
    """Bytes one launch has to move, from the shapes: the floor reads x_j per edge and x_i per node, the node records (32 B per
    node) and col (4 B per edge), and writes [N, width]; GATv2 reads xr_i per node, att and bias on top; the dot-product form
    reads k_j AND v_j per edge, q_i and root_i per node.  The torch composition writes and re-reads its [E, width] and
    [E, heads] intermediates: not counted here."""
    tables = 32 * N + 4 * E
    return {"sum": 4 * width * (E + N) + tables + 4 * width * N, "gatv2": 4 * width * (E + N) + tables + 8 * width * N + 8 * width,
            "tf": 8 * width * E + tables + 12 * width * N}


def torch_transformer(q, k, v, root, src, dst, heads):
    """The layer behind its GEMM in plain torch ops; ``src`` / ``dst``: the batch's edges as they are."""
    n, w = q.shape
    c = w // heads
    s = (q.index_select(0, dst).view(-1, heads, c) * k.index_select(0, src).view(-1, heads, c)).sum(-1) / float(np.sqrt(c))
    idx = dst.unsqueeze(-1).expand(-1, heads)
    smax = s.new_full((n, heads), float("-inf")).scatter_reduce(0, idx, s, reduce="amax", include_self=True)
    e = (s - smax.index_select(0, dst)).exp()
    a = e / (s.new_zeros(n, heads).index_add(0, dst, e).index_select(0, dst) + 1e-16)
    return q.new_zeros(n, heads, c).index_add(0, dst, a.unsqueeze(-1) * v.index_select(0, src).view(-1, heads, c)).view(n, w) + root


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

    def model(conv):
        return gnnb.GNNModel(b.x.shape[1], None, W, 3, W, conv, torch.nn.ReLU, True, gnnb.GlobalPooling(["add", "mean", "max"]),
                             gnnb.MLP(3 * W, 1, 64, 2), None, gnn_heads=4).eval()

    cm = runtime.CompiledModel.from_model(model(gnnb.TransformerConv_GNNB), B, N, E)  # (a GIN description: explicit self loops stay)
    gat = runtime.CompiledModel.from_model(model(gnnb.GATv2Conv_GNNB), B, N, E)       # (a GCN description: they are dropped)
    cood, nptr, eptr = to(b.coo), to(b.node_ptr), to(b.edge_ptr)
    cm.graph_prep(cood, nptr, eptr, N)
    gat.graph_prep(cood, nptr, eptr, N)
    qkvr = to(rng.uniform(-1, 1, (N, 4 * W)).astype(np.float32))
    q, k, v, root = (qkvr[:, i * W:(i + 1) * W] for i in range(4))
    att, bias = to(rng.uniform(-0.5, 0.5, W).astype(np.float32)), to(rng.uniform(-0.5, 0.5, W).astype(np.float32))
    xs = k.contiguous()
    src, dst = to(b.coo[:, 0].astype(np.int64)), to(b.coo[:, 1].astype(np.int64))
    ours = ("tf_h1", "tf_h4", "gatv2_h1", "gatv2_h4", "sum")
    outs = {name: torch.empty((N, W), device=dev) for name in ours}

    def fused(heads):
        return lambda: cm.aggregate_transformer(q, k, v, root=root, heads=heads, out=outs[f"tf_h{heads}"])

    def gatv2(heads):
        return lambda: gat.aggregate_gatv2(q, k, att, bias=bias, heads=heads, negative_slope=SLOPE, out=outs[f"gatv2_h{heads}"])

    calls = {"tf_h1": fused(1), "tf_h4": fused(4), "gatv2_h1": gatv2(1), "gatv2_h4": gatv2(4),
             "sum": lambda: cm.aggregate("sum", xs, out=outs["sum"]),
             "torch_h1": lambda: torch_transformer(q, k, v, root, src, dst, 1), "torch_h4": lambda: torch_transformer(q, k, v, root, src, dst, 4)}
    # the fused kernel and the composition compute the same layer
    diffs = {}
    for heads in (1, 4):
        want = calls[f"torch_h{heads}"]()
        got = calls[f"tf_h{heads}"]()
        diffs[f"h{heads}"] = float((got - want).abs().max() / want.abs().max())
        assert diffs[f"h{heads}"] < 1e-5, diffs
    cm.check(), gat.check()
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
           "launches": args.launches, "loops": args.loops, "device": torch.cuda.get_device_name(0), "fused_vs_torch_rel_diff": diffs,
           "bytes": nbytes}
    for name in ours:
        t = times[name]
        res[f"{name}_us"] = round(statistics.median(t), 2)
        res[f"{name}_us_min_max"] = [round(min(t), 2), round(max(t), 2)]
        res[f"{name}_GBps"] = round(nbytes[name.split("_")[0]] / statistics.median(t) / 1e3, 1)
    for name, t in eager.items():
        res[f"{name}_eager_us"] = round(statistics.median(t), 2)
        res[f"{name}_eager_us_min_max"] = [round(min(t), 2), round(max(t), 2)]
    for heads in (1, 4):
        res[f"tf_h{heads}_over_sum"] = round(res[f"tf_h{heads}_us"] / res["sum_us"], 3)
        res[f"tf_h{heads}_over_gatv2_h{heads}"] = round(res[f"tf_h{heads}_us"] / res[f"gatv2_h{heads}_us"], 3)
        res[f"torch_h{heads}_over_tf_h{heads}"] = round(res[f"torch_h{heads}_eager_us"] / res[f"tf_h{heads}_us"], 2)
    cm.check(), gat.check()
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    for heads in (1, 4):  # the one condition: in the same run, eager against eager as well as against the device's own time
        assert res[f"tf_h{heads}_eager_us"] < res[f"torch_h{heads}_eager_us"] and res[f"tf_h{heads}_us"] < res[f"torch_h{heads}_eager_us"], res


if __name__ == "__main__":
    main()
