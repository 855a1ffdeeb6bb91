#!/usr/bin/env python3
"""Time of the GAT (v1) aggregate with edge features (csrc/k_gat_edge.hip) at the C3t batch: the batch of workload c3t (4096
``molhiv_tail`` graphs: heavy-tailed molecule sizes), width ``--width`` (128), heads 1 and 4, edge_dim 4 and 16.  Fails without a
GPU.

The candidates alternate inside every loop of one call, all on ONE workspace:
  gate_h{1,4}_d{4,16}    ``aggregate_gat_edges`` with bias: d FMAs per (edge, head) on the folded ``a_edge`` in front of
                         ``aggregate_gat``'s add and leaky_relu; ``xl``, ``s_src`` and ``s_dst`` the column blocks of one
                         [N, width + roundup4(2 heads)] matrix, as a layer's GEMM leaves them
  gat_h{1,4}             ``aggregate_gat`` with bias on the same blocks: the same gather without the edge term -- the floor
  gatv2e_h{1,4}_d{4,16}  ``aggregate_gatv2_edges`` at the same edge_dim: a projected edge term per column and a cross-lane sum
  sum                    ``aggregate("sum", xl)`` at the same width: the same rows gathered once, no score and no softmax
  gemm_h4                the layer's GEMM x -> [N, width + 8] with the folded score rows (``runtime.linear`` at in = width, no
                         bias): GAT v1's, unchanged by the edge form
  torch_h{1,4}_d{4,16}   the unfused composition in torch on the GPU, what a user would run otherwise: the attribute mean per
                         destination (``index_add``, a divide), the edge term as a [E + N, d] x [d, heads] product,
                         ``index_select`` of the two scores, ``leaky_relu``, a scatter softmax, ``index_select`` of xl_j and
                         ``index_add`` of the weighted rows, over the edges plus one self loop per node
HIP events on the launch stream around ``--launches`` back-to-back launches of one candidate, microseconds per launch; median
over ``--loops`` loops, with the loop-to-loop spread (min, max), after a warm-up of every candidate.  The library's candidates: the
launches captured once into a HIP graph and replayed between the events -- the device's own time.  The torch composition is timed
eagerly.  The fused kernel and the torch composition are compared (max |difference| relative to max |value|) before anything is
timed.  Bytes per launch are this tool's arithmetic from the shapes -- what the algorithm has to move, not a counter.  Context, not
an acceptance figure.

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


def aggregate_bytes(N, E, width, heads, d):
    """Bytes one launch has to move, from the shapes: the gather reads x_j per edge and x_i per node, the node records (32 B per
    node) and col (4 B per edge), and writes [N, width]; GAT v1 reads 4 heads bytes per edge and 8 heads per node on top, and the
    bias; the edge form reads eid (4 B) and the attribute row (4 d B) per edge on top of that."""
    floor = 4 * width * (E + N) + 32 * N + 4 * E + 4 * width * N
    gat = floor + 4 * heads * (E + N) + 4 * heads * N + 4 * width
    return {"sum": floor, "gat": gat, "gate": gat + 4 * E + 4 * d * E}


def torch_gate(xl, s_src, s_dst, a_edge, bias, esrc, edst, ea, heads):
    """The layer behind its GEMM in plain torch ops; ``esrc`` / ``edst`` / ``ea``: the edges without (v, v) rows and their
    attribute rows; one self loop per node with the mean attribute is added here."""
    n, w = xl.shape
    c = w // heads
    loops = torch.arange(n, device=xl.device)
    deg = xl.new_zeros(n).index_add(0, edst, xl.new_ones(edst.numel()))
    loop_attr = xl.new_zeros(n, ea.shape[1]).index_add(0, edst, ea) / deg.clamp(min=1).unsqueeze(-1)
    src, dst = torch.cat([esrc, loops]), torch.cat([edst, loops])
    t = torch.cat([ea, loop_attr]) @ a_edge.t()
    s = torch.nn.functional.leaky_relu(s_src.index_select(0, src) + s_dst.index_select(0, dst) + t, SLOPE)
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
    model = gnnb.GNNModel(b.x.shape[1], 4, W, 3, W, gnnb.GATv1EConv_GNNB, torch.nn.ReLU, True, gnnb.GlobalPooling(["add", "mean", "max"]),
                          gnnb.MLP(3 * W, 1, 64, 2), None, gnn_heads=4).eval()
    cm = runtime.CompiledModel.from_model(model, B, N, E)  # (a GAT model's workspace is a GCN workspace)
    cm.graph_prep(to(b.coo), to(b.node_ptr), to(b.edge_ptr), N)
    # the operands as a layer's GEMM leaves them: [xl | s_src | s_dst | pad] for GAT v1 (per heads), [xl | xr] for GATv2
    blocks = {h: to(rng.uniform(-1, 1, (N, W + (2 * h + 3) // 4 * 4)).astype(np.float32)) for h in HEADS}
    lr = to(rng.uniform(-1, 1, (N, 2 * W)).astype(np.float32))
    for h in HEADS:
        blocks[h][:, :W] = lr[:, :W]  # (every candidate gathers the same rows)
    xl, xr = lr[:, :W], lr[:, W:]
    att, bias = to(rng.uniform(-0.5, 0.5, W).astype(np.float32)), to(rng.uniform(-0.5, 0.5, W).astype(np.float32))
    xs = xl.contiguous()
    eas = {d: to(rng.uniform(-1, 1, (E, d)).astype(np.float32)) for d in EDGE_DIMS}
    a_edge = {(h, d): to(rng.uniform(-0.5, 0.5, (h, d)).astype(np.float32)) for h in HEADS for d in EDGE_DIMS}
    w_edge = {d: to(rng.uniform(-0.5, 0.5, (W, d)).astype(np.float32)) for d in EDGE_DIMS}
    keep = b.coo[:, 0] != b.coo[:, 1]
    kept = b.coo[keep]
    esrc, edst = to(kept[:, 0].astype(np.int64)), to(kept[:, 1].astype(np.int64))
    ea_kept = {d: eas[d][to(np.flatnonzero(keep))] for d in EDGE_DIMS}
    xin = to(rng.uniform(-1, 1, (N, W)).astype(np.float32))
    w_fold = to(rng.uniform(-0.1, 0.1, (W + 8, W)).astype(np.float32))
    combos = [(h, d) for h in HEADS for d in EDGE_DIMS]
    ours = ([f"gate_h{h}_d{d}" for h, d in combos] + [f"gat_h{h}" for h in HEADS] + [f"gatv2e_h{h}_d{d}" for h, d in combos] + ["sum", "gemm_h4"])
    outs = {name: torch.empty((N, W + 8 if name == "gemm_h4" else W), device=dev) for name in ours}

    def gate(h, d):
        t = blocks[h]
        return lambda: cm.aggregate_gat_edges(t[:, :W], t[:, W:W + h], t[:, W + h:W + 2 * h], eas[d], a_edge[h, d], bias=bias, heads=h,
                                              negative_slope=SLOPE, out=outs[f"gate_h{h}_d{d}"])

    def gat(h):
        t = blocks[h]
        return lambda: cm.aggregate_gat(t[:, :W], t[:, W:W + h], t[:, W + h:W + 2 * h], bias=bias, heads=h, negative_slope=SLOPE,
                                        out=outs[f"gat_h{h}"])

    def gatv2e(h, d):
        return lambda: cm.aggregate_gatv2_edges(xl, xr, att, eas[d], w_edge[d], bias=bias, heads=h, negative_slope=SLOPE,
                                                out=outs[f"gatv2e_h{h}_d{d}"])

    def torch_call(h, d):
        t = blocks[h]
        return lambda: torch_gate(t[:, :W], t[:, W:W + h], t[:, W + h:W + 2 * h], a_edge[h, d], bias, esrc, edst, ea_kept[d], h)

    calls = {**{f"gate_h{h}_d{d}": gate(h, d) for h, d in combos}, **{f"gat_h{h}": gat(h) for h in HEADS},
             **{f"gatv2e_h{h}_d{d}": gatv2e(h, d) for h, d in combos},
             "sum": lambda: cm.aggregate("sum", xs, out=outs["sum"]),
             "gemm_h4": lambda: runtime.linear([(xin, None)], w_fold, out=outs["gemm_h4"]),
             **{f"torch_h{h}_d{d}": torch_call(h, d) for h, d in combos}}
    # the fused kernel and the composition compute the same layer
    diffs = {}
    for h, d in combos:
        want = calls[f"torch_h{h}_d{d}"]()
        got = calls[f"gate_h{h}_d{d}"]()
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
    eager = alternate({name: eagerly(call) for name, call in calls.items() if name.startswith("torch")})
    res = {"workload": args.workload, "shape": w["shape"], "graphs": B, "nodes": N, "edges": E, "edges_without_self_loops": int(len(kept)),
           "max_in_degree": int(np.bincount(kept[:, 1]).max()), "width": W, "negative_slope": SLOPE, "launches": args.launches, "loops": args.loops,
           "device": torch.cuda.get_device_name(0), "fused_vs_torch_rel_diff": diffs, "bytes": {"sum": aggregate_bytes(N, E, W, 1, 4)["sum"]}}
    for h in HEADS:
        res["bytes"][f"gat_h{h}"] = aggregate_bytes(N, E, W, h, 4)["gat"]
        for d in EDGE_DIMS:
            res["bytes"][f"gate_h{h}_d{d}"] = aggregate_bytes(N, E, W, h, d)["gate"]
    for name in ours:
        t = times[name]
        res[f"{name}_us"] = round(statistics.median(t), 2)
        res[f"{name}_us_min_max"] = [round(min(t), 2), round(max(t), 2)]
        if name in res["bytes"]:
            res[f"{name}_GBps"] = round(res["bytes"][name] / statistics.median(t) / 1e3, 1)
    for name, t in eager.items():
        res[f"{name}_eager_us"] = round(statistics.median(t), 2)
        res[f"{name}_eager_us_min_max"] = [round(min(t), 2), round(max(t), 2)]
    for h, d in combos:
        g = res[f"gate_h{h}_d{d}_us"]
        res[f"gate_h{h}_d{d}_over_gat_h{h}"] = round(g / res[f"gat_h{h}_us"], 3)  # the ratio to the floor: reported, not promised
        res[f"gate_h{h}_d{d}_over_gatv2e"] = round(g / res[f"gatv2e_h{h}_d{d}_us"], 3)
        res[f"gate_h{h}_d{d}_over_sum"] = round(g / res["sum_us"], 3)
        res[f"torch_h{h}_d{d}_over_gate"] = round(res[f"torch_h{h}_d{d}_eager_us"] / g, 2)
    cm.check()
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
