#!/usr/bin/env python3
"""Time of the GAT (v1) aggregate (csrc/k_gat.hip) at the C3t batch: the batch of workload c3t (4096 ``molhiv_tail`` graphs:
heavy-tailed molecule sizes), width ``--width`` (128), heads 1 and 4.  Fails without a GPU.

The candidates alternate inside every loop of one call:
  gat_h1, gat_h4      ``aggregate_gat`` with bias: one scalar per (edge, head) in front of the softmax, ``xl``, ``s_src`` and ``s_dst``
                      the column blocks of one [N, width + roundup4(2 heads)] matrix, as a layer's GEMM leaves them
  gatv2_h1, gatv2_h4  ``aggregate_gatv2`` with bias: the same ONE gather per edge, a score per column and a cross-lane sum
  sum                 ``aggregate("sum", xl)`` at the same width on the same (GCN) workspace: the same rows gathered once, no score
                      and no softmax -- the floor
  gemm_h4, gemm_plain the layer's GEMM x -> [N, width + 8] with the folded score rows, and x -> [N, width] without them
                      (``runtime.linear`` at in = width, no bias); gemm_scores: the eight score rows alone, x -> [N, 8]
  torch_h1, torch_h4  the unfused composition in torch on the GPU, what a user would run otherwise: ``index_select`` of the two
                      scores, ``leaky_relu``, a scatter softmax (``scatter_reduce`` amax, ``exp``, ``index_add``, a divide),
                      ``index_select`` of xl_j and ``index_add`` of the weighted rows, over the edges plus one self loop per node
HIP events on the launch stream around ``--launches`` back-to-back launches of one candidate, microseconds per launch; median
over ``--loops`` loops, with the loop-to-loop spread (min, max), after a warm-up of every candidate.  ``*_us`` of the library's
candidates: the launches captured once into a HIP graph and replayed between the events -- the device's own time;
``*_eager_us``: the same launches issued from Python, which the host's enqueue rate can bound.  The torch composition is timed
eagerly only.  The fused kernel and the torch composition are compared (max |difference| relative to max |value|) before anything
is timed.  Bytes per launch are this tool's arithmetic from the shapes -- what the algorithm has to move, not a counter.
Context, not an acceptance figure.

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


def aggregate_bytes(N, E, width, heads):
    """Bytes one launch has to move, from the shapes: the floor reads x_j per edge and x_i per node, the node records (32 B per
    node) and col (4 B per edge), and writes [N, width]; GAT v1 reads 4 heads bytes per edge and 8 heads per node on top, and the
    bias; GATv2 reads xr_i per node, att and bias on top of the floor."""
    floor = 4 * width * (E + N) + 32 * N + 4 * E + 4 * width * N
    return {"sum": floor, "gat": floor + 4 * heads * (E + N) + 4 * heads * N + 4 * width, "gatv2": floor + 4 * width * N + 8 * width}


def torch_gat(xl, s_src, s_dst, bias, src, dst, heads):
    """The layer behind its GEMM in plain torch ops; ``src`` / ``dst``: the edges without (v, v) rows, then one self loop per node."""
    n, w = xl.shape
    c = w // heads
    s = torch.nn.functional.leaky_relu(s_src.index_select(0, src) + s_dst.index_select(0, dst), SLOPE)
    idx = dst.unsqueeze(-1).expand(-1, heads)
    smax = s.new_full((n, heads), float("-inf")).scatter_reduce(0, idx, s, reduce="amax", include_self=True)
    e = (s - smax.index_select(0, dst)).exp()
    a = e / (s.new_zeros(n, heads).index_add(0, dst, e).index_select(0, dst) + 1e-16)
    xj = xl.index_select(0, src).view(-1, heads, c)
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
    model = gnnb.GNNModel(b.x.shape[1], None, W, 3, W, gnnb.GATv1Conv_GNNB, torch.nn.ReLU, True, gnnb.GlobalPooling(["add", "mean", "max"]),
                          gnnb.MLP(3 * W, 1, 64, 2), None, gnn_heads=4).eval()
    cm = runtime.CompiledModel.from_model(model, B, N, E)  # (a GAT model's workspace is a GCN workspace)
    cm.graph_prep(to(b.coo), to(b.node_ptr), to(b.edge_ptr), N)
    # the operands as a layer's GEMM leaves them: [xl | s_src | s_dst | pad] for GAT v1 (per heads), [xl | xr] for GATv2
    blocks = {h: to(rng.uniform(-1, 1, (N, W + (2 * h + 3) // 4 * 4)).astype(np.float32)) for h in (1, 4)}
    lr = to(rng.uniform(-1, 1, (N, 2 * W)).astype(np.float32))
    for h in (1, 4):
        blocks[h][:, :W] = lr[:, :W]  # (every candidate gathers the same rows)
    xl, xr = lr[:, :W], lr[:, W:]
    att, bias = to(rng.uniform(-0.5, 0.5, W).astype(np.float32)), to(rng.uniform(-0.5, 0.5, W).astype(np.float32))
    xs = xl.contiguous()
    kept = b.coo[b.coo[:, 0] != b.coo[:, 1]]
    loops = np.arange(N)
    src, dst = to(np.concatenate([kept[:, 0], loops]).astype(np.int64)), to(np.concatenate([kept[:, 1], loops]).astype(np.int64))
    # the layer's GEMM at in = width: on the folded weight [W ; A_src W ; A_dst W ; 0] of 4 heads, and on W alone
    xin = to(rng.uniform(-1, 1, (N, W)).astype(np.float32))
    w_fold, w_plain = to(rng.uniform(-0.1, 0.1, (W + 8, W)).astype(np.float32)), to(rng.uniform(-0.1, 0.1, (W, W)).astype(np.float32))
    ours = ("gat_h1", "gat_h4", "gatv2_h1", "gatv2_h4", "sum", "gemm_h4", "gemm_plain", "gemm_scores")
    outs = {name: torch.empty((N, {"gemm_h4": W + 8, "gemm_scores": 8}.get(name, W)), device=dev) for name in ours}

    def gat(heads):
        t = blocks[heads]
        return lambda: cm.aggregate_gat(t[:, :W], t[:, W:W + heads], t[:, W + heads:W + 2 * heads], bias=bias, heads=heads, negative_slope=SLOPE,
                                        out=outs[f"gat_h{heads}"])

    def gatv2(heads):
        return lambda: cm.aggregate_gatv2(xl, xr, att, bias=bias, heads=heads, negative_slope=SLOPE, out=outs[f"gatv2_h{heads}"])

    def torch_call(heads):
        t = blocks[heads]
        return lambda: torch_gat(t[:, :W], t[:, W:W + heads], t[:, W + heads:W + 2 * heads], bias, src, dst, heads)

    calls = {"gat_h1": gat(1), "gat_h4": gat(4), "gatv2_h1": gatv2(1), "gatv2_h4": gatv2(4),
             "sum": lambda: cm.aggregate("sum", xs, out=outs["sum"]),
             "gemm_h4": lambda: runtime.linear([(xin, None)], w_fold, out=outs["gemm_h4"]),
             "gemm_plain": lambda: runtime.linear([(xin, None)], w_plain, out=outs["gemm_plain"]),
             "gemm_scores": lambda: runtime.linear([(xin, None)], w_fold[W:], out=outs["gemm_scores"]),
             "torch_h1": torch_call(1), "torch_h4": torch_call(4)}
    # the fused kernel and the composition compute the same layer
    diffs = {}
    for heads in (1, 4):
        want = calls[f"torch_h{heads}"]()
        got = calls[f"gat_h{heads}"]()
        diffs[f"h{heads}"] = float((got - want).abs().max() / want.abs().max())
        assert diffs[f"h{heads}"] < 1e-5, diffs
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
    nbytes = {h: aggregate_bytes(N, E, W, h) for h in (1, 4)}
    res = {"workload": args.workload, "shape": w["shape"], "graphs": B, "nodes": N, "edges": E, "edges_without_self_loops": int(len(kept)),
           "max_in_degree": int(np.bincount(kept[:, 1]).max()), "width": W, "negative_slope": SLOPE, "launches": args.launches, "loops": args.loops,
           "device": torch.cuda.get_device_name(0), "fused_vs_torch_rel_diff": diffs,
           "bytes": {"sum": nbytes[1]["sum"], "gatv2": nbytes[1]["gatv2"], "gat_h1": nbytes[1]["gat"], "gat_h4": nbytes[4]["gat"]}}
    for name in ours:
        t = times[name]
        res[f"{name}_us"] = round(statistics.median(t), 2)
        res[f"{name}_us_min_max"] = [round(min(t), 2), round(max(t), 2)]
        if not name.startswith("gemm"):
            nb = res["bytes"]["sum" if name == "sum" else "gatv2" if name.startswith("gatv2") else name]
            res[f"{name}_GBps"] = round(nb / statistics.median(t) / 1e3, 1)
    for name, t in eager.items():
        res[f"{name}_eager_us"] = round(statistics.median(t), 2)
        res[f"{name}_eager_us_min_max"] = [round(min(t), 2), round(max(t), 2)]
    for heads in (1, 4):
        res[f"gat_h{heads}_over_sum"] = round(res[f"gat_h{heads}_us"] / res["sum_us"], 3)
        res[f"gat_h{heads}_over_gatv2_h{heads}"] = round(res[f"gat_h{heads}_us"] / res[f"gatv2_h{heads}_us"], 3)
        res[f"torch_h{heads}_over_gat_h{heads}"] = round(res[f"torch_h{heads}_eager_us"] / res[f"gat_h{heads}_us"], 2)
    res["gemm_h4_over_gemm_plain"] = round(res["gemm_h4_us"] / res["gemm_plain_us"], 3)
    cm.check()
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
