#!/usr/bin/env python3
"""Time of SchNet's continuous-filter aggregate (csrc/k_schnet.hip) and its layer's GEMMs at the C3t batch: the batch of workload c3t
(4096 ``molhiv_tail`` graphs), width ``--width`` (128), ``--gaussians`` (50).  Fails without a GPU.

Candidates that alternate inside every loop of one call, all on the same batch (a SchNet model's workspace -- a GIN description: the
tables keep explicit self loops):
  cfconv         ``gnnb_aggregate_cfconv``: the slot -> row map, k_schnet_cfconv and its fix-up pass (a)
  sum            ``aggregate("sum", x)`` at the width: the same gather, no filter -- the floor (b)
  unfused        the composition from this project's own pieces: the basis, two ``linear`` GEMMs over [E, .] with ssp between them, the
                 product with C(d) and the gathered row, a segmented sum (elementwise steps and the sum in torch) (c)
  torch          the same composition in torch alone, eager (d)
  gemm_lin1, gemm_lin2, gemm_lin   the layer's three node GEMMs [N, w] -> [N, w] (e)
HIP events around ``--launches`` launches captured once into a HIP graph and replayed (the two compositions: eager, 5 launches); median
over ``--loops`` loops with the spread.  ``cfconv_mfma_fraction``: the kernel's 2 E (Gp F + F^2) flops over the candidate's time as a
fraction of the fp32 MFMA peak (``bench.FP32_MFMA_PEAK_TFLOPS``), to put beside the 0.61 .. 0.68 ``k_linear_dma`` reaches (README).
Nothing is promised and no timing is held to a condition.  What the design expects (written before the first run) is
REPORTED (``expect_*``), true or false:
  (1) the kernel is below the unfused composition (c)
  (2) its MFMA fraction is at least 0.25 and below ``k_linear_dma``'s 0.61: LDS feeds 1.06 operand registers per MFMA (34 of the CU's
      128 bytes per clock), so LDS is not the limit; what is left are ssp's VALU work on the MFMA's issue port, layer 1's short chains
      (13 k steps) and five barriers per tile with one workgroup per CU

``--out FILE`` also writes the JSON line to a file."""
import argparse
import json
import math
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

LINEAR_DMA_FRACTION = 0.61


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="c3t")
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--gaussians", type=int, default=50)
    ap.add_argument("--cutoff", type=float, default=5.0)
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
    W, G, CUT = args.width, args.gaussians, args.cutoff
    rng = np.random.default_rng(0)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    uni = lambda *shape, s=1.0: to(rng.uniform(-s, s, shape).astype(np.float32))  # noqa: E731
    torch.manual_seed(0)
    pools, head = gnnb.GlobalPooling(["add", "mean", "max"]), gnnb.MLP(3 * W, 1, 64, 2)
    model = gnnb.GNNModel(b.x.shape[1], 1, W, 3, W, gnnb.SchNetConv_GNNB, torch.nn.ReLU, True, pools, head, None, gnn_gaussians=G,
                          gnn_cutoff=CUT).eval()
    cm = runtime.CompiledModel.from_model(model, B, N, E)  # (a GIN description: explicit self loops stay; it carries the kernel's scratch)
    cm.graph_prep(to(b.coo), to(b.node_ptr), to(b.edge_ptr), N)
    x1, h = uni(N, W), uni(N, W)
    dist = to(rng.uniform(0.3, 1.1 * CUT, E).astype(np.float32))
    w1, b1, w2, b2 = uni(W, G, s=1.0 / G), uni(W), uni(W, W, s=1.0 / W), uni(W)
    wl, bl = uni(W, W, s=1.0 / W ** 0.5), uni(W, s=1.0 / W ** 0.5)
    src, dst = to(b.coo[:, 0].astype(np.int64)), to(b.coo[:, 1].astype(np.int64))
    mu = torch.linspace(0.0, CUT, G, device=dev)
    coeff = -0.5 / float(mu[1] - mu[0]) ** 2 if G > 1 else -0.5 / CUT ** 2
    ssp = lambda v: torch.nn.functional.softplus(v) - math.log(2.0)  # noqa: E731
    out = lambda *shape: torch.empty(shape, device=dev)  # noqa: E731
    o_cf, o_sum, o_g, o_e1, o_e2 = out(N, W), out(N, W), out(N, W), out(E, W), out(E, W)

    def cfconv():
        runtime._check(cm.lib.gnnb_aggregate_cfconv(cm._ws, x1.data_ptr(), W, W, dist.data_ptr(), w1.data_ptr(), G, b1.data_ptr(), w2.data_ptr(), W,
                                                    b2.data_ptr(), G, CUT, o_cf.data_ptr(), W, torch.cuda.current_stream().cuda_stream))
        return o_cf

    def composed(lin):
        rbf = torch.exp(coeff * (dist.unsqueeze(1) - mu) ** 2)
        f = lin(ssp(lin(rbf, w1, b1, o_e1)), w2, b2, o_e2) * (0.5 * (torch.cos(dist * (math.pi / CUT)) + 1.0)).unsqueeze(1)
        return torch.zeros((N, W), device=dev).index_add(0, dst, x1.index_select(0, src) * f)

    calls = {"cfconv": cfconv,
             "sum": lambda: cm.aggregate("sum", h, out=o_sum),
             "gemm_lin1": lambda: runtime.linear([(h, None)], wl, out=o_g),
             "gemm_lin2": lambda: runtime.linear([(h, None)], wl, bias=bl, out=o_g),
             "gemm_lin": lambda: runtime.linear([(h, None)], wl, bias=bl, act="relu", out=o_g),
             "unfused": lambda: composed(lambda a, wt, bs, o: runtime.linear([(a, None)], wt, bias=bs, out=o)),
             "torch": lambda: composed(lambda a, wt, bs, o: torch.addmm(bs, a, wt.T))}
    want = calls["torch"]()
    rel_diff = float((cfconv() - want).abs().max() / want.abs().max())
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
    res = {"workload": args.workload, "shape": w["shape"], "graphs": B, "nodes": N, "edges": E, "width": W, "gaussians": G, "cutoff": CUT,
           "launches": args.launches, "loops": args.loops, "device": torch.cuda.get_device_name(0), "kernel_vs_torch_rel_diff": rel_diff}
    for name in calls:
        t = times[name]
        res[f"{name}_us"] = round(statistics.median(t), 2)
        res[f"{name}_us_min_max"] = [round(min(t), 2), round(max(t), 2)]
    gp = (G + 3) // 4 * 4
    res["cfconv_flops"] = 2 * E * (gp * W + W * W)
    res["cfconv_tflops"] = round(res["cfconv_flops"] / res["cfconv_us"] * 1e-6, 2)
    res["cfconv_mfma_fraction"] = round(res["cfconv_tflops"] / bench.FP32_MFMA_PEAK_TFLOPS, 3)
    res["linear_dma_mfma_fraction"] = LINEAR_DMA_FRACTION
    res["cfconv_over_sum"] = round(res["cfconv_us"] / res["sum_us"], 2)
    res["layer_gemms_us"] = round(res["gemm_lin1_us"] + res["gemm_lin2_us"] + res["gemm_lin_us"], 2)
    res["expect_cfconv_below_unfused"] = bool(res["cfconv_us"] < res["unfused_us"])
    res["expect_mfma_fraction_0p25_to_linear_dma"] = bool(0.25 <= res["cfconv_mfma_fraction"] < LINEAR_DMA_FRACTION)
    cm.check()
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
