#!/usr/bin/env python3
"""Time of the GENConv aggregate (csrc/k_gen.hip) and its layer's GEMMs at the C3t batch: the batch of workload c3t (4096
``molhiv_tail`` graphs), width ``--width`` (128), temperature ``--t`` (1).  Fails without a GPU.

Candidates that alternate inside every loop of one call, all on the same batch (a GENConv model's workspace -- a GIN description:
the tables keep explicit self loops -- and, for ``aggregate_gat``, a GCN workspace):
  gen_d0, gen_d4, gen_d16    ``aggregate_gen`` without edge features and at edge_dim 4 and 16, s and r the two column blocks of one
                             [N, 2 width] tensor, as in a model
  sum                        ``aggregate("sum", x)`` at the width: the same gather, no state -- the floor
  gine_d4, gine_d16          the GINE aggregate (``aggregate_edges_fused``): the same bytes and the same message, a plain sum
  gat                        ``aggregate_gat`` at heads 1: one gather per edge, one softmax state per row
  gemm_sr, gemm_mlp0, gemm_mlp2   the layer's GEMMs [N, w] -> [N, 2 w], [N, w] -> [N, 2 w] with ReLU, [N, 2 w] -> [N, w]
  torch_d0, torch_d4, torch_d16   the unfused composition in torch on the same GPU (edge term, message, segmented max, exp, two
                             segmented sums), eager
HIP events around ``--launches`` launches captured once into a HIP graph and replayed; median over ``--loops`` loops with the spread.
Nothing is promised and no timing is held to a condition.  What the design expects (written before the first run)
is REPORTED (``expect_*``), true or false:
  (1) at edge_dim 4 and 16 the kernel is within 1.0 .. 1.35 x the GINE aggregate at the same edge_dim
  (2) at edge_dim 0 the kernel is at most ``aggregate_gat`` and at most 2 x the floor

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

EDGE_DIMS = (0, 4, 16)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="c3t")
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--t", type=float, default=1.0)
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
    W, T = args.width, args.t
    rng = np.random.default_rng(0)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    uni = lambda *shape, s=1.0: to(rng.uniform(-s, s, shape).astype(np.float32))  # noqa: E731
    torch.manual_seed(0)
    pools, head = gnnb.GlobalPooling(["add", "mean", "max"]), gnnb.MLP(3 * W, 1, 64, 2)
    model = gnnb.GNNModel(b.x.shape[1], None, W, 3, W, gnnb.GENConv_GNNB, torch.nn.ReLU, True, pools, head, None, gnn_softmax_t=T).eval()
    cm = runtime.CompiledModel.from_model(model, B, N, E)  # (a GIN description: explicit self loops stay)
    gcn_model = gnnb.GNNModel(b.x.shape[1], None, W, 3, W, gnnb.GCNConv_GNNB, torch.nn.ReLU, True, pools, head, None).eval()
    cg = runtime.CompiledModel.from_model(gcn_model, B, N, E)  # (a GCN description: what aggregate_gat takes)
    cood, nptr, eptr = to(b.coo), to(b.node_ptr), to(b.edge_ptr)
    cm.graph_prep(cood, nptr, eptr, N)
    cg.graph_prep(cood, nptr, eptr, N)
    h, sr = uni(N, W), uni(N, 2 * W)
    s, r = sr[:, :W], sr[:, W:]
    src, dst = to(b.coo[:, 0].astype(np.int64)), to(b.coo[:, 1].astype(np.int64))
    s_src, s_dst = uni(N, 1), uni(N, 1)
    bound = 1.0 / W ** 0.5
    w_sr, b_sr, w_m0, b_m0, w_m2, b_m2 = uni(2 * W, W, s=bound), uni(2 * W, s=bound), uni(2 * W, W, s=bound), uni(2 * W, s=bound), uni(
        W, 2 * W, s=bound), uni(W, s=bound)
    hid = uni(N, 2 * W)
    out = lambda *shape: torch.empty(shape, device=dev)  # noqa: E731
    o_sr, o_m0, o_m2, o_sum, o_gat = out(N, 2 * W), out(N, 2 * W), out(N, W), out(N, W), out(N, W)
    calls = {"sum": lambda: cm.aggregate("sum", h, out=o_sum),
             "gat": lambda: cg.aggregate_gat(h, s_src, s_dst, heads=1, out=o_gat),
             "gemm_sr": lambda: runtime.linear([(h, None)], w_sr, bias=b_sr, out=o_sr),
             "gemm_mlp0": lambda: runtime.linear([(h, None)], w_m0, bias=b_m0, act="relu", out=o_m0),
             "gemm_mlp2": lambda: runtime.linear([(hid, None)], w_m2, bias=b_m2, out=o_m2)}
    rel_diff = {}
    for d in EDGE_DIMS:
        ea, we, be = (uni(E, d), uni(W, d, s=1.0 / d), uni(W, s=0.5)) if d else (None, None, None)
        o_gen, o_gine = out(N, W), out(N, W)
        calls[f"gen_d{d}"] = lambda ea=ea, we=we, be=be, o=o_gen: cm.aggregate_gen(s, r, ea, we, be, t=T, out=o)
        if d:
            calls[f"gine_d{d}"] = lambda ea=ea, we=we, be=be, o=o_gine: cm.aggregate_edges_fused(h, ea, we, be, out=o)

        def torch_layer(ea=ea, we=we, be=be):
            m = s.index_select(0, src)
            if ea is not None:
                m = m + (ea @ we.T + be)
            m = torch.relu(m) + 1e-7
            z = T * m
            zmax = torch.full((N, W), float("-inf"), device=dev).scatter_reduce(0, dst.unsqueeze(1).expand_as(z), z, "amax")
            wgt = torch.exp(z - zmax.index_select(0, dst))
            den = torch.zeros((N, W), device=dev).index_add(0, dst, wgt)
            num = torch.zeros((N, W), device=dev).index_add(0, dst, wgt * m)
            return torch.where(den > 0, num / den.clamp(min=1), num) + r
        calls[f"torch_d{d}"] = torch_layer
        want = torch_layer()
        rel_diff[f"d{d}"] = float((calls[f"gen_d{d}"]() - want).abs().max() / want.abs().max())
        assert rel_diff[f"d{d}"] < 1e-5, rel_diff
    cm.check()
    ours = [n for n in calls if not n.startswith("torch")]
    timer = runtime.HipTimer()
    for _ in range(5):  # warm-up of every candidate
        for call in calls.values():
            call()
    torch.cuda.synchronize()

    def captured(call):
        side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            for _ in range(args.launches):
                call()
        graph.replay()  # (warm-up of the graph itself)
        torch.cuda.synchronize()
        return graph

    def eagerly(call, launches):
        def run():
            for _ in range(launches):
                call()
        return run

    def alternate(runs, launches):
        t = {name: [] for name in runs}
        for _ in range(args.loops):
            for name, run in runs.items():  # (the candidates alternate inside the loop)
                timer.start()
                run()
                timer.stop()
                t[name].append(timer.elapsed_ms() * 1000.0 / launches)
        return t

    graphs = {name: captured(calls[name]) for name in ours}
    times = alternate({name: g.replay for name, g in graphs.items()}, args.launches)
    tt = alternate({n: eagerly(c, 5) for n, c in calls.items() if n.startswith("torch")}, 5)
    res = {"workload": args.workload, "shape": w["shape"], "graphs": B, "nodes": N, "edges": E, "width": W, "t": T,
           "launches": args.launches, "loops": args.loops, "device": torch.cuda.get_device_name(0), "kernel_vs_torch_rel_diff": rel_diff}
    for name in ours:
        t = times[name]
        res[f"{name}_us"] = round(statistics.median(t), 2)
        res[f"{name}_us_min_max"] = [round(min(t), 2), round(max(t), 2)]
    for d in EDGE_DIMS:
        res[f"torch_d{d}_eager_us"] = round(statistics.median(tt[f"torch_d{d}"]), 1)
        res[f"gen_d{d}_over_sum"] = round(res[f"gen_d{d}_us"] / res["sum_us"], 3)
        if d:
            res[f"gen_over_gine_d{d}"] = round(res[f"gen_d{d}_us"] / res[f"gine_d{d}_us"], 3)
            res[f"expect_gen_within_1p35x_gine_d{d}"] = bool(res[f"gen_d{d}_us"] <= 1.35 * res[f"gine_d{d}_us"])
    res["gen_d0_over_gat"] = round(res["gen_d0_us"] / res["gat_us"], 3)
    res["expect_gen_d0_at_most_gat_and_2x_sum"] = bool(res["gen_d0_us"] <= res["gat_us"] and res["gen_d0_us"] <= 2.0 * res["sum_us"])
    res["layer_gemms_us"] = round(res["gemm_sr_us"] + res["gemm_mlp0_us"] + res["gemm_mlp2_us"], 2)
    cm.check()
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
