#!/usr/bin/env python3
"""Time of the GatedGraphConv step (csrc/k_ggnn.hip and its GEMM) at the C3t batch: the batch of workload c3t (4096
``molhiv_tail`` graphs: heavy-tailed molecule sizes), width ``--width`` (128).  Fails without a GPU.

Candidates that alternate inside every loop of one call, all on the same batch and the same workspace -- a GatedGraphConv
model's (a GIN description: the tables keep explicit self loops):
  ggnn         ``aggregate_ggnn`` with ``b_ih``: the sum of the neighbours' folded messages -- THREE row-widths gathered per edge --
               and the whole GRU cell in one pass over the edges, ``p`` / ``gh`` the two halves of one [N, 6 width] matrix, as a
               step's GEMM leaves them
  resgated     ``aggregate_resgated`` with root at the same width: TWO row-widths gathered per edge, two transcendentals per
               (edge, column)
  sum          ``aggregate("sum", x)`` at the same width: ONE row-width gathered per edge, nothing else -- the floor
  gemm         the step's GEMM [N, width] -> [N, 6 width] (``linear`` on a [6 width, width] weight with a bias)
  agg_first    the aggregate-first order composed from existing stage entries, its gate pass LEFT OUT -- a lower bound for that
               order: ``aggregate("sum")`` at the width plus ``linear`` [N, 2 width] -> [N, 4 width] on a prebuilt ``[s | h]``
               (the r and z blocks take s and h together, the n block's two halves stay apart: 8 width^2 flops per row)
  torch        the unfused composition in torch on the GPU, what a user would run otherwise: ``index_select``, ``index_add``,
               two sigmoids, a tanh and the blend behind the same GEMM's output
HIP events on the launch stream around ``--launches`` back-to-back launches of one candidate, microseconds per launch; median
over ``--loops`` loops, with the loop-to-loop spread (min, max), after a warm-up of every candidate.  ``*_us`` of the library's
candidates: the launches captured once into a HIP graph and replayed between the events -- the device's own time;
``*_eager_us``: the same launches issued from Python, which the host's enqueue rate can bound.  The torch composition is timed
eagerly only.  The fused kernel and the torch composition are compared (max |difference| relative to max |value|) before
anything is timed.  Bytes per launch are this tool's arithmetic from the shapes -- what the algorithm has to move, not a counter.
Nothing is promised: the tool holds no timing to a condition.  What the design rests on is REPORTED (``expect_*``), true or
false: the kernel lands between ``aggregate_resgated`` and 1.5 x it, GEMM + kernel is not slower than the aggregate-first lower
bound, and the fused kernel is faster than the torch composition of the same run.

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


def aggregate_bytes(N, E, width):
    """Bytes one launch has to move, from the shapes: the floor reads x_j per edge, the node records (32 B per node) and col
    (4 B per edge), and writes [N, width]; the gated form reads TWO rows per edge and two per node (k_i, root_i); the GRU form
    reads THREE row-widths per edge and four per node (gh_i's three blocks, h_i)."""
    tables = 32 * N + 4 * E
    return {"sum": 4 * width * E + tables + 4 * width * N, "resgated": 8 * width * E + tables + 12 * width * N,
            "ggnn": 12 * width * E + tables + 20 * width * N}


def torch_ggnn(p, gh, h, b_ih, src, dst, W):
    """The step behind its GEMM in plain torch ops; ``src`` / ``dst``: the batch's edges as they are."""
    gi = torch.zeros_like(p).index_add(0, dst, p.index_select(0, src)) + b_ih
    r = torch.sigmoid(gi[:, :W] + gh[:, :W])
    z = torch.sigmoid(gi[:, W:2 * W] + gh[:, W:2 * W])
    n = torch.tanh(gi[:, 2 * W:] + r * gh[:, 2 * W:])
    return n + z * (h - n)


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
    uni = lambda *shape, s=1.0: to(rng.uniform(-s, s, shape).astype(np.float32))  # noqa: E731
    torch.manual_seed(0)
    model = gnnb.GNNModel(b.x.shape[1], None, W, 3, W, gnnb.GatedGraphConv_GNNB, torch.nn.ReLU, True,
                          gnnb.GlobalPooling(["add", "mean", "max"]), gnnb.MLP(3 * W, 1, 64, 2), None, gnn_steps=1).eval()
    cm = runtime.CompiledModel.from_model(model, B, N, E)  # (a GIN description: explicit self loops stay)
    cood, nptr, eptr = to(b.coo), to(b.node_ptr), to(b.edge_ptr)
    cm.graph_prep(cood, nptr, eptr, N)
    h = uni(N, W)
    bound = 1.0 / W ** 0.5
    w6, b6, b_ih = uni(6 * W, W, s=bound), uni(6 * W, s=bound), uni(3 * W, s=bound)
    b6[:3 * W] = 0.0  # (the p block takes no bias)
    w_af, b_af, sh = uni(4 * W, 2 * W, s=bound), uni(4 * W, s=bound), uni(N, 2 * W)
    pg = runtime.linear([(h, None)], w6, bias=b6)  # [p | gh] as the step's GEMM leaves it
    p, gh = pg[:, :3 * W], pg[:, 3 * W:]
    kqvr = uni(N, 4 * W)
    k, q, v, root = (kqvr[:, i * W:(i + 1) * W] for i in range(4))
    src, dst = to(b.coo[:, 0].astype(np.int64)), to(b.coo[:, 1].astype(np.int64))
    ours = ("ggnn", "resgated", "sum", "gemm", "agg_first_gemm")
    outs = {"ggnn": torch.empty((N, W), device=dev), "resgated": torch.empty((N, W), device=dev), "sum": torch.empty((N, W), device=dev),
            "gemm": torch.empty((N, 6 * W), device=dev), "agg_first_gemm": torch.empty((N, 4 * W), device=dev)}
    calls = {"ggnn": lambda: cm.aggregate_ggnn(p, gh, h, b_ih=b_ih, out=outs["ggnn"]),
             "resgated": lambda: cm.aggregate_resgated(k, q, v, root=root, out=outs["resgated"]),
             "sum": lambda: cm.aggregate("sum", h, out=outs["sum"]),
             "gemm": lambda: runtime.linear([(h, None)], w6, bias=b6, out=outs["gemm"]),
             "agg_first_gemm": lambda: runtime.linear([(sh, None)], w_af, bias=b_af, out=outs["agg_first_gemm"]),
             "torch": lambda: torch_ggnn(p, gh, h, b_ih, src, dst, W)}
    # the fused kernel and the composition compute the same step
    want = calls["torch"]()
    got = calls["ggnn"]()
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
           "launches": args.launches, "loops": args.loops, "device": torch.cuda.get_device_name(0), "fused_vs_torch_rel_diff": diff,
           "bytes": nbytes}
    for name in ours:
        t = times[name]
        res[f"{name}_us"] = round(statistics.median(t), 2)
        res[f"{name}_us_min_max"] = [round(min(t), 2), round(max(t), 2)]
        if name in nbytes:
            res[f"{name}_GBps"] = round(nbytes[name] / statistics.median(t) / 1e3, 1)
    for name, t in eager.items():
        res[f"{name}_eager_us"] = round(statistics.median(t), 2)
        res[f"{name}_eager_us_min_max"] = [round(min(t), 2), round(max(t), 2)]
    res["step_us"] = round(res["gemm_us"] + res["ggnn_us"], 2)  # this order: GEMM, then the fused kernel
    res["agg_first_lower_bound_us"] = round(res["sum_us"] + res["agg_first_gemm_us"], 2)  # the other order without its gate pass
    res["ggnn_over_sum"] = round(res["ggnn_us"] / res["sum_us"], 3)
    res["ggnn_over_resgated"] = round(res["ggnn_us"] / res["resgated_us"], 3)
    res["step_over_agg_first_lower_bound"] = round(res["step_us"] / res["agg_first_lower_bound_us"], 3)
    res["torch_over_ggnn"] = round(res["torch_eager_us"] / res["ggnn_us"], 2)
    res["expect_kernel_between_resgated_and_1p5x"] = bool(res["resgated_us"] <= res["ggnn_us"] <= 1.5 * res["resgated_us"])
    res["expect_step_not_slower_than_agg_first_lower_bound"] = bool(res["step_us"] <= res["agg_first_lower_bound_us"])
    # (in the same run, eager against eager as well as against the device's own time)
    res["expect_fused_faster_than_torch"] = bool(res["ggnn_eager_us"] < res["torch_eager_us"] and res["ggnn_us"] < res["torch_eager_us"])
    cm.check()
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
