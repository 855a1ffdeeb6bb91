#!/usr/bin/env python3
"""Time of the TransformerConv aggregate with edge features (csrc/k_transformer_edge.hip) at the C3t batch: the batch of workload
c3t (4096 ``molhiv_tail`` graphs: heavy-tailed molecule sizes), width ``--width`` (128), heads 1 and 4, ``edge_dim`` 4 and 16.
Fails without a GPU.

The candidates alternate inside every loop of one call, all on the same batch:
  tfe_h*_d*      ``aggregate_transformer_edges`` with root: ``q`` / ``k`` / ``v`` / ``root`` / ``qe`` the column blocks of one
                 [N, 4 width + heads edge_dim] matrix, as a layer's GEMM leaves them, ``edge_attr`` [E, edge_dim] and ``w_edge``;
                 on the workspace of a TransformerConv model (a GIN description: the tables keep explicit self loops)
  tf_h*          ``aggregate_transformer`` on the same blocks and workspace: the same two gathers without the edge term -- the floor
  gatv2e_h*_d*   ``aggregate_gatv2_edges`` at the same width and ``edge_dim`` on the workspace of a GATv2 model (a GCN description)
                 prepared with the same batch: the sibling that forms ``W_e e_ij`` per edge and column
  sum            ``aggregate("sum", x)`` at the same width: the rows gathered once, no score and no softmax
  gemm, gemm_qe_h*_d*   the layer's GEMM ``x [N, width] -> [N, 4 width]`` and the same with the ``roundup4(heads edge_dim)`` folded
                 query columns behind it (``runtime.linear``)
  torch_h*_d*    the unfused composition in torch on the GPU, what a user would run otherwise: the projected edge term [E, width]
                 (a GEMM), ``index_select`` of q_i, k_j and v_j, the scaled dot product, a scatter softmax and ``index_add`` of the
                 weighted rows
HIP events on the launch stream around ``--launches`` back-to-back launches of one candidate, microseconds per launch; median
over ``--loops`` loops, with the loop-to-loop spread (min, max), after a warm-up of every candidate.  ``*_us`` of the library's
candidates: the launches captured once into a HIP graph and replayed between the events -- the device's own time;
``*_eager_us``: the same launches issued from Python, which the host's enqueue rate can bound.  The torch composition is timed
eagerly only.  The fused kernel and the torch composition are compared (max |difference| relative to max |value|, ``qe`` formed
as ``W_e^T q`` per head) before anything is timed.  The ratios to the floor and to the sibling are context: no ratio is a
condition.  The one condition this tool holds is that the fused stage is faster than the torch composition of the same run.

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


def torch_transformer_edges(q, k, v, root, ea, we, src, dst, heads):
    """The layer behind its GEMM in plain torch ops, as models.py defines it: project, add to key and value."""
    n, w = q.shape
    c = w // heads
    p = (ea @ we.t()).view(-1, heads, c)
    kj = k.index_select(0, src).view(-1, heads, c) + p
    s = (q.index_select(0, dst).view(-1, heads, c) * kj).sum(-1) / float(np.sqrt(c))
    idx = dst.unsqueeze(-1).expand(-1, heads)
    smax = s.new_full((n, heads), float("-inf")).scatter_reduce(0, idx, s, reduce="amax", include_self=True)
    e = (s - smax.index_select(0, dst)).exp()
    a = e / (s.new_zeros(n, heads).index_add(0, dst, e).index_select(0, dst) + 1e-16)
    return q.new_zeros(n, heads, c).index_add(0, dst, a.unsqueeze(-1) * (v.index_select(0, src).view(-1, heads, c) + p)).view(n, w) + root


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

    def model(conv, edge_dim=None):
        return gnnb.GNNModel(b.x.shape[1], edge_dim, W, 3, W, conv, torch.nn.ReLU, True, gnnb.GlobalPooling(["add", "mean", "max"]),
                             gnnb.MLP(3 * W, 1, 64, 2), None, gnn_heads=4).eval()

    cm = runtime.CompiledModel.from_model(model(gnnb.TransformerConv_GNNB), B, N, E)  # (a GIN description: explicit self loops stay)
    gat = runtime.CompiledModel.from_model(model(gnnb.GATv2Conv_GNNB), B, N, E)       # (a GCN description: they are dropped)
    cood, nptr, eptr = to(b.coo), to(b.node_ptr), to(b.edge_ptr)
    cm.graph_prep(cood, nptr, eptr, N)
    gat.graph_prep(cood, nptr, eptr, N)
    src, dst = to(b.coo[:, 0].astype(np.int64)), to(b.coo[:, 1].astype(np.int64))
    att, bias = to(rng.uniform(-0.5, 0.5, W).astype(np.float32)), to(rng.uniform(-0.5, 0.5, W).astype(np.float32))
    x = to(rng.uniform(-1, 1, (N, W)).astype(np.float32))
    w4, b4 = to(rng.uniform(-0.1, 0.1, (4 * W, W)).astype(np.float32)), to(rng.uniform(-0.1, 0.1, 4 * W).astype(np.float32))

    calls, outs, diffs, cases = {}, {}, {}, {}
    for d in EDGE_DIMS:
        ea = to(rng.uniform(-1, 1, (E, d)).astype(np.float32))
        we = to(rng.uniform(-0.5, 0.5, (W, d)).astype(np.float32))
        for h in HEADS:
            rq = (h * d + 3) // 4 * 4
            big = to(rng.uniform(-1, 1, (N, 4 * W + rq)).astype(np.float32))
            q, k, v, root = (big[:, i * W:(i + 1) * W] for i in range(4))
            qe = big[:, 4 * W:4 * W + h * d]
            qe.copy_(torch.einsum("hcd,nhc->nhd", we.view(h, W // h, d), q.reshape(N, h, W // h)).reshape(N, h * d))  # qe = W_e^T q
            cases[h, d] = dict(q=q, k=k, v=v, root=root, qe=qe, ea=ea, we=we)
            wq, bq = to(rng.uniform(-0.1, 0.1, (4 * W + rq, W)).astype(np.float32)), to(rng.uniform(-0.1, 0.1, 4 * W + rq).astype(np.float32))
            for name, width in ((f"tfe_h{h}_d{d}", W), (f"gatv2e_h{h}_d{d}", W), (f"gemm_qe_h{h}_d{d}", 4 * W + rq)):
                outs[name] = torch.empty((N, width), device=dev)
            calls[f"tfe_h{h}_d{d}"] = (lambda c=cases[h, d], h=h, d=d: cm.aggregate_transformer_edges(
                c["q"], c["k"], c["v"], c["qe"], c["ea"], c["we"], root=c["root"], heads=h, out=outs[f"tfe_h{h}_d{d}"]))
            calls[f"gatv2e_h{h}_d{d}"] = (lambda c=cases[h, d], h=h, d=d: gat.aggregate_gatv2_edges(
                c["q"], c["k"], att, c["ea"], c["we"], bias=bias, heads=h, negative_slope=SLOPE, out=outs[f"gatv2e_h{h}_d{d}"]))
            calls[f"gemm_qe_h{h}_d{d}"] = (lambda wq=wq, bq=bq, h=h, d=d: runtime.linear([(x, None)], wq, bq, out=outs[f"gemm_qe_h{h}_d{d}"]))
            calls[f"torch_h{h}_d{d}"] = (lambda c=cases[h, d], h=h: torch_transformer_edges(c["q"], c["k"], c["v"], c["root"], c["ea"], c["we"],
                                                                                          src, dst, h))
    for h in HEADS:
        outs[f"tf_h{h}"] = torch.empty((N, W), device=dev)
        calls[f"tf_h{h}"] = (lambda c=cases[h, EDGE_DIMS[0]], h=h: cm.aggregate_transformer(c["q"], c["k"], c["v"], root=c["root"], heads=h,
                                                                                           out=outs[f"tf_h{h}"]))
    outs["sum"], outs["gemm"] = torch.empty((N, W), device=dev), torch.empty((N, 4 * W), device=dev)
    xs = x.contiguous()
    calls["sum"] = lambda: cm.aggregate("sum", xs, out=outs["sum"])
    calls["gemm"] = lambda: runtime.linear([(x, None)], w4, b4, out=outs["gemm"])
    ours = [name for name in calls if not name.startswith("torch")]
    # the fused kernel and the composition compute the same layer
    for d in EDGE_DIMS:
        for h in HEADS:
            want, got = calls[f"torch_h{h}_d{d}"](), calls[f"tfe_h{h}_d{d}"]()
            diffs[f"h{h}_d{d}"] = float((got - want).abs().max() / want.abs().max())
            assert diffs[f"h{h}_d{d}"] < 1e-4, diffs
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
    res = {"workload": args.workload, "shape": w["shape"], "graphs": B, "nodes": N, "edges": E,
           "explicit_self_loops": int((b.coo[:, 0] == b.coo[:, 1]).sum()), "max_in_degree": int(np.bincount(b.coo[:, 1]).max()), "width": W,
           "launches": args.launches, "loops": args.loops, "device": torch.cuda.get_device_name(0), "fused_vs_torch_rel_diff": diffs}
    for name in ours:
        t = times[name]
        res[f"{name}_us"] = round(statistics.median(t), 2)
        res[f"{name}_us_min_max"] = [round(min(t), 2), round(max(t), 2)]
    for name, t in eager.items():
        res[f"{name}_eager_us"] = round(statistics.median(t), 2)
        res[f"{name}_eager_us_min_max"] = [round(min(t), 2), round(max(t), 2)]
    for d in EDGE_DIMS:
        for h in HEADS:
            tag = f"h{h}_d{d}"
            res[f"tfe_{tag}_over_tf_h{h}"] = round(res[f"tfe_{tag}_us"] / res[f"tf_h{h}_us"], 3)         # the gap to the floor
            res[f"tfe_{tag}_over_gatv2e_{tag}"] = round(res[f"tfe_{tag}_us"] / res[f"gatv2e_{tag}_us"], 3)  # ... and to the sibling
            res[f"torch_{tag}_over_tfe_{tag}"] = round(res[f"torch_{tag}_eager_us"] / res[f"tfe_{tag}_us"], 2)
            res[f"gemm_qe_{tag}_over_gemm"] = round(res[f"gemm_qe_{tag}_us"] / res["gemm_us"], 3)
    cm.check(), gat.check()
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    for d in EDGE_DIMS:  # the one condition: in the same run, eager against eager as well as against the device's own time
        for h in HEADS:
            tag = f"h{h}_d{d}"
            assert res[f"tfe_{tag}_eager_us"] < res[f"torch_{tag}_eager_us"] and res[f"tfe_{tag}_us"] < res[f"torch_{tag}_eager_us"], res


if __name__ == "__main__":
    main()
