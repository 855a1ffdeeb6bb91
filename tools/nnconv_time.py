#!/usr/bin/env python3
"""Time of the NNConv layer (csrc/k_nnconv.hip and its GEMM) at the C3t batch: the batch of workload c3t (4096 ``molhiv_tail``
graphs), width ``--width`` (128), ``--edge-dim`` (4) edge attributes, the linear edge network (K = 0) and the hidden one
(``--hidden``, 16).  Fails without a GPU.

Candidates that alternate inside every loop of one call, all on the same batch and an NNConv model's workspace (a GIN
description: the tables keep explicit self loops), per variant v in (L, H):
  nnconv_v     ``aggregate_nnconv``: ONE row of the input width gathered per edge, K' + 1 row-widths written per node
  gemm_v       the layer's GEMM [N, (K' + 2) width] -> [N, width] on the two segments [A | x]
  tf_gemm_v    the transform-first order's GEMM [N, width] -> [N, (K' + 1) width]
  sum          ``aggregate("sum", x)`` at the width: the same gather without coefficients or the wide store -- the floor
  gine         the GINE aggregate (``aggregate_edges_fused``) at the same edge_dim
  torch_v      the unfused composition in torch on the GPU, Theta [E, width, width] materialised (a slice of ``--torch-edges``
               edges, scaled to the batch: the whole tensor is 64 KiB per edge)
The transform-first bound is ``tf_gemm_v`` plus (K' + 1) x ``sum``: its aggregate would gather K' + 1 row-widths per edge.
HIP events around ``--launches`` launches captured once into a HIP graph and replayed; median over ``--loops`` loops with the spread.
Nothing is promised and no timing is held to a condition.  What the design expects is REPORTED (``expect_*``), true or false:
the kernel is below the transform-first gather ((K' + 1) x sum), and kernel + GEMM is below the transform-first total.

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
    ap.add_argument("--edge-dim", type=int, default=4)
    ap.add_argument("--hidden", type=int, default=16)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--loops", type=int, default=7)
    ap.add_argument("--torch-edges", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.launches < 50 or args.loops < 5:
        ap.error("at least five loops of at least 50 launches")

    runtime.load_library(require_gpu=True)  # fails loudly: no fallback
    w = bench.WORKLOADS[args.workload]
    dev = torch.device("cuda:0")
    b = synthetic.make_batch(w["shape"], w["batch"], seed=0)
    B, N, E = b.num_graphs, b.num_nodes, b.num_edges
    W, D = args.width, args.edge_dim
    rng = np.random.default_rng(0)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    uni = lambda *shape, s=1.0: to(rng.uniform(-s, s, shape).astype(np.float32))  # noqa: E731
    torch.manual_seed(0)
    pools, head = gnnb.GlobalPooling(["add", "mean", "max"]), gnnb.MLP(3 * W, 1, 64, 2)
    model = gnnb.GNNModel(b.x.shape[1], D, W, 2, W, gnnb.NNConv_GNNB, torch.nn.ReLU, True, pools, head, None).eval()
    cm = runtime.CompiledModel.from_model(model, B, N, E)
    cood, nptr, eptr = to(b.coo), to(b.node_ptr), to(b.edge_ptr)
    cm.graph_prep(cood, nptr, eptr, N)
    h, ea = uni(N, W), uni(E, D)
    bound = 1.0 / W ** 0.5
    we, be = uni(W, D), uni(W)
    src, dst = to(b.coo[:, 0].astype(np.int64)), to(b.coo[:, 1].astype(np.int64))
    calls, outs, variants = {}, {}, {"L": 0, "H": args.hidden}
    res_diff = {}
    for v, K in variants.items():
        kq = K or D
        w1, b1 = (uni(K, D), uni(K)) if K else (None, None)
        A = torch.empty((N, (kq + 1) * W), device=dev)
        wn, bn = uni(W, (kq + 2) * W, s=bound), uni(W, s=bound)
        wt = uni((kq + 1) * W, W, s=bound)
        outs[v] = (torch.empty((N, W), device=dev), torch.empty((N, (kq + 1) * W), device=dev))
        calls[f"nnconv_{v}"] = lambda w1=w1, b1=b1, A=A: cm.aggregate_nnconv(h, ea, w1, b1, out=A)
        calls[f"gemm_{v}"] = lambda A=A, wn=wn, bn=bn, v=v: runtime.linear([(A, None), (h, None)], wn, bias=bn, out=outs[v][0])
        calls[f"tf_gemm_{v}"] = lambda wt=wt, v=v: runtime.linear([(h, None)], wt, out=outs[v][1])

        def torch_layer(w1=w1, b1=b1, wn=wn, kq=kq, n=min(args.torch_edges, E)):  # (the first n edges: Theta [n, W, W])
            c = ea[:n] if w1 is None else torch.relu(ea[:n] @ w1.T + b1)
            w2 = wn[:, :kq * W].reshape(W, kq, W)  # [o, k, col]
            theta = torch.einsum("ek,okc->eco", c, w2) + wn[:, kq * W:(kq + 1) * W].T
            msg = torch.bmm(h.index_select(0, src[:n]).unsqueeze(1), theta).squeeze(1)
            return torch.zeros((N, W), device=dev).index_add(0, dst[:n], msg)
        calls[f"torch_{v}"] = torch_layer
        # the kernel and the plain composition compute the same aggregate (all edges, block by block)
        got = calls[f"nnconv_{v}"]()
        c = torch.cat([ea if w1 is None else torch.relu(ea @ w1.T + b1), torch.ones((E, 1), device=dev)], 1)
        worst = 0.0
        for k in range(kq + 1):
            want = torch.zeros((N, W), device=dev).index_add(0, dst, c[:, k:k + 1] * h.index_select(0, src))
            worst = max(worst, float((got[:, k * W:(k + 1) * W] - want).abs().max() / want.abs().max()))
        assert worst < 1e-5, worst
        res_diff[v] = worst
    gine_out, sum_out = torch.empty((N, W), device=dev), torch.empty((N, W), device=dev)
    calls["sum"] = lambda: cm.aggregate("sum", h, out=sum_out)
    calls["gine"] = lambda: cm.aggregate_edges_fused(h, ea, we, be, out=gine_out)
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
    res = {"workload": args.workload, "shape": w["shape"], "graphs": B, "nodes": N, "edges": E, "width": W, "edge_dim": D,
           "hidden": args.hidden, "launches": args.launches, "loops": args.loops, "device": torch.cuda.get_device_name(0),
           "kernel_vs_torch_rel_diff": res_diff}
    for name in ours:
        t = times[name]
        res[f"{name}_us"] = round(statistics.median(t), 2)
        res[f"{name}_us_min_max"] = [round(min(t), 2), round(max(t), 2)]
    for v, K in variants.items():
        kq = K or D
        scale = E / min(args.torch_edges, E)
        res[f"torch_{v}_eager_us_scaled"] = round(statistics.median(tt[f"torch_{v}"]) * scale, 1)
        res[f"layer_{v}_us"] = round(res[f"nnconv_{v}_us"] + res[f"gemm_{v}_us"], 2)
        res[f"tf_gather_{v}_us"] = round((kq + 1) * res["sum_us"], 2)
        res[f"tf_total_{v}_us"] = round(res[f"tf_gemm_{v}_us"] + res[f"tf_gather_{v}_us"], 2)
        res[f"nnconv_{v}_over_sum"] = round(res[f"nnconv_{v}_us"] / res["sum_us"], 3)
        res[f"expect_kernel_below_transform_first_gather_{v}"] = bool(res[f"nnconv_{v}_us"] < res[f"tf_gather_{v}_us"])
        res[f"expect_layer_below_transform_first_total_{v}"] = bool(res[f"layer_{v}_us"] < res[f"tf_total_{v}_us"])
    cm.check()
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
