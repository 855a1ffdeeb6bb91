#!/usr/bin/env python3
"""Time of EdgeConv's max aggregate (csrc/k_edgeconv.hip) and its layer's GEMM at the C3t batch: the batch of workload c3t (4096
``molhiv_tail`` graphs), width ``--width`` (128).  Fails without a GPU.

Candidates that alternate inside every loop of one call, all on the same batch (an EdgeConv model's workspace -- a GIN description: the
tables keep explicit self loops; it carries the kernels' scratch):
  edgeconv       ``gnnb_aggregate_edgeconv``: the slot -> row map, k_edgeconv_max and its fix-up pass (a)
  cfconv         ``gnnb_aggregate_cfconv`` at the same width, 50 gaussians: k_schnet_cfconv, the same tiles and second layer (b)
  sum            ``aggregate("sum", x)`` at the width: one gather, no product -- the floor (c)
  gemm_ab        the layer's GEMM x -> [a | b], [N, w] -> [N, 2 w] (d)
  unfused        the composition from this project's own pieces: the two gathers and ReLU in torch, ``linear`` over [E, H], the
                 segmented max in torch (e)
  torch          the same composition in torch alone, eager (f)
HIP events around ``--launches`` launches captured once into a HIP graph and replayed (the two compositions: eager, 5 launches); median
over ``--loops`` loops with the spread.  ``edgeconv_mfma_fraction``: the kernel's 2 E H F flops over the candidate's time as a fraction of
the fp32 MFMA peak (``bench.FP32_MFMA_PEAK_TFLOPS``).  Nothing is promised and no timing is held to a condition.  What the design
expects (written before the first run) is REPORTED (``expect_*``), true or false:
  (a) the stage entry is below the unfused composition (e)
  (b) the stage entry is at or below k_schnet_cfconv at the same width (b)

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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="c3t")
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
    W, G, CUT = args.width, 50, 5.0
    rng = np.random.default_rng(0)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    uni = lambda *shape, s=1.0: to(rng.uniform(-s, s, shape).astype(np.float32))  # noqa: E731
    torch.manual_seed(0)
    pools, head = gnnb.GlobalPooling(["add", "mean", "max"]), gnnb.MLP(3 * W, 1, 64, 2)
    model = gnnb.GNNModel(b.x.shape[1], None, W, 3, W, gnnb.EdgeConv_GNNB, torch.nn.ReLU, True, pools, head, None, gnn_aggr="max").eval()
    cm = runtime.CompiledModel.from_model(model, B, N, E)
    cm.graph_prep(to(b.coo), to(b.node_ptr), to(b.edge_ptr), N)
    h, ab = uni(N, W), uni(N, 2 * W)
    w_ec, b_ec = uni(2 * W, W, s=1.0 / W ** 0.5), uni(2 * W, s=1.0 / W ** 0.5)
    w2, b2 = uni(W, W, s=1.0 / W ** 0.5), uni(W)
    dist, c1, cb1 = to(rng.uniform(0.3, 1.1 * CUT, E).astype(np.float32)), uni(W, G, s=1.0 / G), uni(W)
    src, dst = to(b.coo[:, 0].astype(np.int64)), to(b.coo[:, 1].astype(np.int64))
    idx = dst.unsqueeze(1).expand(E, W)
    has = torch.zeros(N, dtype=torch.bool, device=dev).index_fill(0, dst, True).unsqueeze(1)
    out = lambda *shape: torch.empty(shape, device=dev)  # noqa: E731
    o_ec, o_cf, o_sum, o_g, o_e = out(N, W), out(N, W), out(N, W), out(N, 2 * W), out(E, W)
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731

    def edgeconv():
        runtime._check(cm.lib.gnnb_aggregate_edgeconv(cm._ws, ab.data_ptr(), 2 * W, W, w2.data_ptr(), W, b2.data_ptr(), W, None, runtime.ACT["none"],
                                                      o_ec.data_ptr(), W, stream()))
        return o_ec

    def cfconv():
        runtime._check(cm.lib.gnnb_aggregate_cfconv(cm._ws, h.data_ptr(), W, W, dist.data_ptr(), c1.data_ptr(), G, cb1.data_ptr(), w2.data_ptr(), W,
                                                    b2.data_ptr(), G, CUT, o_cf.data_ptr(), W, stream()))

    def composed(lin):
        m = lin(torch.relu(ab[:, :W].index_select(0, dst) + ab[:, W:].index_select(0, src)))
        r = torch.full((N, W), float("-inf"), device=dev).scatter_reduce(0, idx, m, "amax", include_self=True)
        return torch.where(has, r, torch.zeros_like(r))

    calls = {"edgeconv": edgeconv,
             "cfconv": cfconv,
             "sum": lambda: cm.aggregate("sum", h, out=o_sum),
             "gemm_ab": lambda: runtime.linear([(h, None)], w_ec, bias=b_ec, out=o_g),
             "unfused": lambda: composed(lambda a: runtime.linear([(a, None)], w2, bias=b2, out=o_e)),
             "torch": lambda: composed(lambda a: torch.addmm(b2, a, w2.T))}
    want = calls["torch"]()
    rel_diff = float((edgeconv() - want).abs().max() / want.abs().max())
    assert rel_diff < 1e-5, rel_diff
    cm.check()
    eager = ("unfused", "torch")
    ours = [n for n in calls if n not in eager]
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
    times.update(alternate({n: eagerly(calls[n], 5) for n in eager}, 5))
    res = {"workload": args.workload, "shape": w["shape"], "graphs": B, "nodes": N, "edges": E, "width": W, "launches": args.launches,
           "loops": args.loops, "device": torch.cuda.get_device_name(0), "kernel_vs_torch_rel_diff": rel_diff}
    for name in calls:
        t = times[name]
        res[f"{name}_us"] = round(statistics.median(t), 2)
        res[f"{name}_us_min_max"] = [round(min(t), 2), round(max(t), 2)]
    res["edgeconv_flops"] = 2 * E * W * W
    res["edgeconv_tflops"] = round(res["edgeconv_flops"] / res["edgeconv_us"] * 1e-6, 2)
    res["edgeconv_mfma_fraction"] = round(res["edgeconv_tflops"] / bench.FP32_MFMA_PEAK_TFLOPS, 3)
    res["edgeconv_over_sum"] = round(res["edgeconv_us"] / res["sum_us"], 2)
    res["expect_edgeconv_below_unfused"] = bool(res["edgeconv_us"] < res["unfused_us"])
    res["expect_edgeconv_at_or_below_cfconv"] = bool(res["edgeconv_us"] <= res["cfconv_us"])
    cm.check()
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
