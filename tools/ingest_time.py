#!/usr/bin/env python3
"""Time of the device ingest of a PyG mini-batch (``CompiledModel.ingest_pyg``, csrc/k_ingest.hip) at the BASELINE config 2
batch shape, beside the host route it replaces and the graph prep that follows it.

  grouped    edge_index as ``Batch.from_data_list`` gives it (the fast path)
  shuffled   the same edges under a seeded permutation (the radix grouping)
  graph_prep ``gnnb_graph_prep`` on the ingested arrays, for scale
  host       ``batching.from_pyg_batch`` on tensors brought from the device + the three copies back (wall clock)

Device figures: HIP events around ``--calls`` back-to-back calls on one stream, microseconds per call, median of ``--repeats``
(``*_us``: eager calls, which the host's enqueue rate can bound; ``*_graph_us``: the same calls captured into one HIP graph and
replayed, the device's own time).
``--out FILE`` also writes the JSON line to a file; under ``rocprofv3 --kernel-trace --stats`` use small ``--repeats``.

``--ordered`` times the ordered form instead (``forward_pyg_ordered``, csrc/k_order.hip) on the heavy-tailed molecule shape
(workload c3t unless ``--workload`` names another) under the promise ``--promise`` (57), beside the two routes a caller had before:

  forward_pyg_ordered   ordered ingest (with its one wait), large segment, forward, rows put back
  host_round_trip       tensors to the CPU, ``from_pyg_batch``, ``order_large_last``, upload, ``set_large_segment``, ``forward``
  forward_pyg           no promise: every batch layer by layer
  forward_preordered    for scale: ``forward`` alone on arrays ordered beforehand, segment set (what is left of the first two
                        once the ordering is free)

The ordered form waits inside the call, so all three are wall-clock times of a call that ends in a synchronise, microseconds per
call over ``--calls`` calls, median of ``--repeats``.  ``ordered_ingest_us`` is ``ingest_pyg_ordered`` alone (enqueue and wait: the
time before the host may enqueue the forward); ``wait_us`` is that minus the enqueue-only time of the plain ``ingest_pyg`` -- an
upper bound of the wait, the enqueue of the three ordering kernels is in it -- and ``wait_share`` its share of
``forward_pyg_ordered``."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from gnnbuilder_amd import runtime, synthetic  # noqa: E402
from gnnbuilder_amd.batching import from_pyg_batch, order_large_last  # noqa: E402


def ordered_leg(args):
    w = bench.WORKLOADS[args.workload if args.workload != "c2" else "c3t"]
    dev = torch.device("cuda:0")
    b = synthetic.make_batch(w["shape"], w["batch"], seed=0)
    B, N, E = b.num_graphs, b.num_nodes, b.num_edges
    model = bench.build_model(w)
    cm = runtime.CompiledModel.from_model(model, B, N, E, max_graph_nodes=args.promise)
    cm.enable_ordered_ingest()
    layerwise = runtime.CompiledModel.from_model(model, B, N, E)  # no promise
    layerwise.enable_ingest()
    x = torch.from_numpy(b.x).to(dev)
    ei = torch.from_numpy(np.ascontiguousarray(b.coo.T.astype(np.int64))).to(dev)
    batch = torch.from_numpy(np.repeat(np.arange(B), np.diff(b.node_ptr)).astype(np.int64)).to(dev)

    def ordered():
        return cm.forward_pyg_ordered(x, ei, batch=batch, num_graphs=B)

    def round_trip():
        r = from_pyg_batch(x.cpu().numpy(), ei.cpu().numpy(), batch=batch.cpu().numpy(), num_graphs=B)
        o, perm, seg = order_large_last(r, args.promise)
        if seg[0] == B:
            cm.set_large_segment()
        else:
            cm.set_large_segment(*seg)
        out = cm.forward(*[torch.from_numpy(a).to(dev) for a in (o.x, o.coo, o.node_ptr, o.edge_ptr)])
        return out[torch.from_numpy(np.argsort(perm)).to(dev)]

    def wall_us(call, calls, sync_each=True):
        for _ in range(min(calls, 5)):
            call()
        torch.cuda.synchronize()
        per_call = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            for _ in range(calls):
                call()
                if sync_each:
                    torch.cuda.synchronize()
            t1 = time.perf_counter()  # (sync_each = False: the enqueue alone, the clock stops in front of the synchronise)
            torch.cuda.synchronize()
            per_call.append((t1 - t0) * 1e6 / calls)
        return round(statistics.median(per_call), 1), [round(min(per_call), 1), round(max(per_call), 1)]

    # the three routes agree before anything is timed: ordered == host round trip exactly (the same kernels on the same arrays)
    got, want = ordered().clone(), round_trip()
    cm.check()
    assert torch.equal(got, want)
    path = cm.last_path()
    large = int((np.diff(b.node_ptr) > args.promise).sum())
    res = {"workload": w["shape"], "graphs": B, "nodes": N, "edges": E, "promise": args.promise, "large_graphs": large, "path": path,
           "calls": args.calls, "repeats": args.repeats, "order_bytes": runtime.order_bytes(B, N, E, b.x.shape[1], cm.out_dim)}
    res["forward_pyg_ordered_us"], res["forward_pyg_ordered_us_min_max"] = wall_us(ordered, args.calls)
    res["forward_pyg_no_promise_us"], res["forward_pyg_no_promise_us_min_max"] = wall_us(
        lambda: layerwise.forward_pyg(x, ei, batch=batch, num_graphs=B), args.calls)
    res["host_round_trip_us"], res["host_round_trip_us_min_max"] = wall_us(round_trip, max(args.calls // 20, 3))
    r = from_pyg_batch(b.x, ei.cpu().numpy(), batch=batch.cpu().numpy(), num_graphs=B)
    o, _, seg = order_large_last(r, args.promise)
    pre = [torch.from_numpy(a).to(dev) for a in (o.x, o.coo, o.node_ptr, o.edge_ptr)]
    cm.set_large_segment(*(seg if seg[0] < B else ()))
    res["forward_preordered_us"], res["forward_preordered_us_min_max"] = wall_us(lambda: cm.forward(*pre), args.calls)
    res["ordered_ingest_us"], _ = wall_us(lambda: cm.ingest_pyg_ordered(x, ei, batch=batch, num_graphs=B), args.calls)
    res["ingest_enqueue_us"], _ = wall_us(lambda: cm.ingest_pyg(ei, batch=batch, num_graphs=B), args.calls, sync_each=False)
    res["wait_us"] = round(res["ordered_ingest_us"] - res["ingest_enqueue_us"], 1)
    res["wait_share"] = round(res["wait_us"] / res["forward_pyg_ordered_us"], 3)
    cm.check()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="c2")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ordered", action="store_true", help="time forward_pyg_ordered beside the host round trip and forward_pyg")
    ap.add_argument("--promise", type=int, default=57, help="max_graph_nodes promise of the --ordered leg")
    args = ap.parse_args()
    if args.ordered:
        line = json.dumps(ordered_leg(args))
        print(line)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(line + "\n")
        return

    w = bench.WORKLOADS[args.workload]
    dev = torch.device("cuda:0")
    b = synthetic.make_batch(w["shape"], w["batch"], seed=0)
    B, N, E = b.num_graphs, b.num_nodes, b.num_edges
    cm = runtime.CompiledModel.from_model(bench.build_model(w), B, N, E, max_graph_nodes=int(np.diff(b.node_ptr).max()))
    cm.enable_ingest()
    x = torch.from_numpy(b.x).to(dev)
    ei = np.ascontiguousarray(b.coo.T.astype(np.int64))
    batch = torch.from_numpy(np.repeat(np.arange(B), np.diff(b.node_ptr)).astype(np.int64)).to(dev)
    grouped = torch.from_numpy(ei).to(dev)
    shuffled = torch.from_numpy(np.ascontiguousarray(ei[:, np.random.default_rng(0).permutation(E)])).to(dev)

    timer = runtime.HipTimer()

    def device_us(call, calls=None):
        calls = calls or args.calls
        for _ in range(min(calls, 20)):
            call()
        torch.cuda.synchronize()
        per_call = []
        for _ in range(args.repeats):
            timer.start()
            for _ in range(calls):
                call()
            timer.stop()
            per_call.append(timer.elapsed_ms() * 1000.0 / calls)
        return per_call

    def graph_us(call, per_graph=20):
        """`per_graph` calls captured once, replayed; None where the capture is refused."""
        try:
            side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=side):
                for _ in range(per_graph):
                    call()
        except Exception as exc:  # noqa: BLE001
            print(f"capture refused: {exc}", file=sys.stderr)
            return None
        replays = max(args.calls // per_graph, 1)
        t = [v / per_graph for v in device_us(graph.replay, replays)]
        return round(statistics.median(t), 2)

    def host_route(edges):
        t0 = time.perf_counter()
        r = from_pyg_batch(np.zeros((N, 0), np.float32), edges.cpu().numpy(), batch=batch.cpu().numpy(), num_graphs=B)
        out = [torch.from_numpy(a).to(dev) for a in (r.coo, r.node_ptr, r.edge_ptr)]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6, out

    # both paths give what the host adapter gives (exact), before anything is timed
    for edges in (grouped, shuffled):
        got = cm.ingest_pyg(edges, batch=batch, num_graphs=B)
        cm.check()
        _, ref = host_route(edges)
        assert all(torch.equal(g, r) for g, r in zip(got, ref))

    res = {"workload": args.workload, "graphs": B, "nodes": N, "edges": E, "calls": args.calls, "repeats": args.repeats,
           "sort_passes": -(-max(B - 1, 0).bit_length() // runtime.INGEST_DIGIT_BITS), "ingest_bytes": runtime.ingest_bytes(B, N, E)}
    for name, edges in (("grouped", grouped), ("shuffled", shuffled)):
        t = device_us(lambda: cm.ingest_pyg(edges, batch=batch, num_graphs=B))
        res[f"ingest_{name}_us"] = round(statistics.median(t), 2)
        res[f"ingest_{name}_us_min_max"] = [round(min(t), 2), round(max(t), 2)]
        res[f"ingest_{name}_graph_us"] = graph_us(lambda: cm.ingest_pyg(edges, batch=batch, num_graphs=B))
    coo, nptr, eptr = cm.ingest_pyg(grouped, batch=batch, num_graphs=B)
    t = device_us(lambda: cm.graph_prep(coo, nptr, eptr, N))
    res["graph_prep_us"] = round(statistics.median(t), 2)
    res["graph_prep_graph_us"] = graph_us(lambda: cm.graph_prep(coo, nptr, eptr, N))
    t = device_us(lambda: cm.forward(x, coo, nptr, eptr))
    res["forward_us"] = round(statistics.median(t), 2)
    t = device_us(lambda: cm.forward_pyg(x, grouped, batch=batch, num_graphs=B))
    res["forward_pyg_grouped_us"] = round(statistics.median(t), 2)
    cm.check()
    for name, edges in (("grouped", grouped), ("shuffled", shuffled)):
        t = [host_route(edges)[0] for _ in range(max(args.repeats, 3))]
        res[f"host_route_{name}_us"] = round(statistics.median(t), 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
