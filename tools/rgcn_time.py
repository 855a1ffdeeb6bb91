#!/usr/bin/env python3
"""Time of the RGCNConv layer (csrc/k_rgcn.hip and its GEMM) at the C3t batch: the batch of workload c3t (4096 ``molhiv_tail``
graphs: heavy-tailed molecule sizes), width ``--width`` (128), ``--relations`` (4) relations, seeded uniform edge types.  Fails
without a GPU.

Candidates that alternate inside every loop of one call, all on the same batch -- on an RGCNConv model's workspace (a GIN
description: the tables keep explicit self loops), but for ``gat``, whose stage entry takes a GCN description's workspace:
  rgcn         ``aggregate_rgcn`` with root: ONE row-width gathered per edge from the edge's relation block, an 8-byte slot
               record per edge, ``p`` / ``root`` the blocks of one [N, (R + 1) width] matrix, as the layer's GEMM leaves them
  slots        ``rgcn_slots``: the slot records, once per forward for all layers
  gat          ``aggregate_gat`` at heads 1 and the same width: ONE row-width and one score per edge, the online softmax
  sum          ``aggregate("sum", x)`` at the same width: ONE row-width gathered per edge, nothing else -- the floor
  gemm         the layer's GEMM [N, width] -> [N, (R + 1) width] (``linear`` on a [(R + 1) width, width] weight with a bias)
  agg_first    a lower bound for the aggregate-first order (per-relation means at the input width, then one GEMM with
               K = (R + 1) width), composed from existing stage entries with its per-relation aggregate counted as ONE plain
               ``aggregate("sum")`` at the width: that plus ``linear`` [N, (R + 1) width] -> [N, width]
  torch        the unfused composition in torch on the GPU, what a user would run otherwise: per relation ``index_select``,
               ``index_add``, a division by the counts, behind the same GEMM's output
HIP events on the launch stream around ``--launches`` back-to-back launches of one candidate, microseconds per launch; median
over ``--loops`` loops, with the loop-to-loop spread (min, max), after a warm-up of every candidate.  ``*_us`` of the library's
candidates: the launches captured once into a HIP graph and replayed between the events -- the device's own time;
``*_eager_us``: the same launches issued from Python, which the host's enqueue rate can bound.  The torch composition is timed
eagerly only.  The fused kernel and the torch composition are compared (max |difference| relative to max |value|) before
anything is timed.  Bytes per launch are this tool's arithmetic from the shapes -- what the algorithm has to move, not a counter.
Nothing is promised: nobody had measured any of this when the tool was written, and it holds no timing to a condition.  What the
design rests on is REPORTED (``expect_*``), true or false: the kernel lands between ``sum`` and ``aggregate_gat`` of the same
run, GEMM + kernel is not slower than the aggregate-first lower bound, and the fused kernel is faster than the torch composition
of the same run.

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
    (4 B per edge), and writes [N, width]; the RGCN form reads the 8-byte slot record per edge and the root row per node
    besides; the GAT form a score per edge and per node and the row's own xl; the slot pass reads eid and the type per edge
    (twice: count, then write) and writes the record."""
    tables = 32 * N + 4 * E
    return {"sum": 4 * width * E + tables + 4 * width * N, "rgcn": 4 * width * E + 8 * E + tables + 8 * width * N,
            "gat": 4 * width * E + 4 * E + tables + 8 * width * N + 8 * N, "slots": 32 * N + 16 * E + 8 * E}


def torch_rgcn(pr, src, dst, types, R, W):
    """The layer behind its GEMM in plain torch ops; ``src`` / ``dst`` / ``types``: the batch's edges as they are."""
    out = pr[:, R * W:].clone()
    for r in range(R):
        m = types == r
        s, d = src[m], dst[m]
        cnt = torch.zeros(pr.shape[0], device=pr.device).index_add(0, d, torch.ones(d.numel(), device=pr.device))
        acc = torch.zeros((pr.shape[0], W), device=pr.device).index_add(0, d, pr[:, r * W:(r + 1) * W].index_select(0, s))
        out = out + acc / cnt.clamp(min=1).unsqueeze(-1)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="c3t", help="the batch's workload in bench.WORKLOADS (its shape and batch size)")
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--relations", type=int, default=4)
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
    W, R = args.width, args.relations
    rng = np.random.default_rng(0)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    uni = lambda *shape, s=1.0: to(rng.uniform(-s, s, shape).astype(np.float32))  # noqa: E731
    torch.manual_seed(0)
    pools, head = gnnb.GlobalPooling(["add", "mean", "max"]), gnnb.MLP(3 * W, 1, 64, 2)
    model = gnnb.GNNModel(b.x.shape[1], None, W, 3, W, gnnb.RGCNConv_GNNB, torch.nn.ReLU, True, pools, head, None, gnn_relations=R).eval()
    cm = runtime.CompiledModel.from_model(model, B, N, E)  # (a GIN description: explicit self loops stay)
    gcn_model = gnnb.GNNModel(b.x.shape[1], None, W, 3, W, gnnb.GCNConv_GNNB, torch.nn.ReLU, True, pools, head, None).eval()
    cg = runtime.CompiledModel.from_model(gcn_model, B, N, E)  # (a GCN description: what aggregate_gat takes)
    cood, nptr, eptr = to(b.coo), to(b.node_ptr), to(b.edge_ptr)
    cm.graph_prep(cood, nptr, eptr, N)
    cg.graph_prep(cood, nptr, eptr, N)
    types_np = rng.integers(0, R, E).astype(np.int32)
    types = to(types_np)
    h = uni(N, W)
    bound = 1.0 / W ** 0.5
    wr, br = uni((R + 1) * W, W, s=bound), uni((R + 1) * W, s=bound)
    br[:R * W] = 0.0  # (the relation blocks take no bias)
    w_af, b_af, cat = uni(W, (R + 1) * W, s=bound), uni(W, s=bound), uni(N, (R + 1) * W)
    pr = runtime.linear([(h, None)], wr, bias=br)  # [p_0 | .. | p_{R-1} | root] as the layer's GEMM leaves it
    p, root = pr[:, :R * W], pr[:, R * W:]
    rec = cm.rgcn_slots(types, R)
    s_src, s_dst = uni(N, 1), uni(N, 1)
    src, dst = to(b.coo[:, 0].astype(np.int64)), to(b.coo[:, 1].astype(np.int64))
    ours = ("rgcn", "slots", "gat", "sum", "gemm", "agg_first_gemm")
    outs = {"rgcn": torch.empty((N, W), device=dev), "gat": torch.empty((N, W), device=dev), "sum": torch.empty((N, W), device=dev),
            "gemm": torch.empty((N, (R + 1) * W), device=dev), "agg_first_gemm": torch.empty((N, W), device=dev)}
    rec2 = torch.zeros_like(rec)
    calls = {"rgcn": lambda: cm.aggregate_rgcn(rec, p, R, root=root, out=outs["rgcn"]),
             "slots": lambda: runtime._check(cm.lib.gnnb_rgcn_slots(cm._ws, types.data_ptr(), R, rec2.data_ptr(), runtime._stream_ptr())),
             "gat": lambda: cg.aggregate_gat(h, s_src, s_dst, heads=1, out=outs["gat"]),
             "sum": lambda: cm.aggregate("sum", h, out=outs["sum"]),
             "gemm": lambda: runtime.linear([(h, None)], wr, bias=br, out=outs["gemm"]),
             "agg_first_gemm": lambda: runtime.linear([(cat, None)], w_af, bias=b_af, out=outs["agg_first_gemm"]),
             "torch": lambda: torch_rgcn(pr, src, dst, types, R, W)}
    # the fused kernel and the composition compute the same layer
    want = calls["torch"]()
    got = calls["rgcn"]()
    diff = float((got - want).abs().max() / want.abs().max())
    assert diff < 1e-5, diff
    calls["slots"]()
    assert torch.equal(rec2, rec)
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
           "relations": R, "launches": args.launches, "loops": args.loops, "device": torch.cuda.get_device_name(0),
           "fused_vs_torch_rel_diff": diff, "bytes": nbytes}
    for name in ours:
        t = times[name]
        res[f"{name}_us"] = round(statistics.median(t), 2)
        res[f"{name}_us_min_max"] = [round(min(t), 2), round(max(t), 2)]
        if name in nbytes:
            res[f"{name}_GBps"] = round(nbytes[name] / statistics.median(t) / 1e3, 1)
    for name, t in eager.items():
        res[f"{name}_eager_us"] = round(statistics.median(t), 2)
        res[f"{name}_eager_us_min_max"] = [round(min(t), 2), round(max(t), 2)]
    res["layer_us"] = round(res["gemm_us"] + res["rgcn_us"], 2)  # this order: GEMM, then the fused kernel
    res["agg_first_lower_bound_us"] = round(res["sum_us"] + res["agg_first_gemm_us"], 2)  # the other order, its aggregate as ONE plain sum
    res["rgcn_over_sum"] = round(res["rgcn_us"] / res["sum_us"], 3)
    res["rgcn_over_gat"] = round(res["rgcn_us"] / res["gat_us"], 3)
    res["layer_over_agg_first_lower_bound"] = round(res["layer_us"] / res["agg_first_lower_bound_us"], 3)
    res["torch_over_rgcn"] = round(res["torch_eager_us"] / res["rgcn_us"], 2)
    res["expect_kernel_between_sum_and_gat"] = bool(res["sum_us"] <= res["rgcn_us"] <= res["gat_us"])
    res["expect_layer_not_slower_than_agg_first_lower_bound"] = bool(res["layer_us"] <= res["agg_first_lower_bound_us"])
    # (in the same run, eager against eager as well as against the device's own time)
    res["expect_fused_faster_than_torch"] = bool(res["rgcn_eager_us"] < res["torch_eager_us"] and res["rgcn_us"] < res["torch_eager_us"])
    cm.check()
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
