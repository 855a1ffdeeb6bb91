"""Every forward route against a float64 evaluation of the same model, with an fp32-class error budget.

The parity tests hold the HIP output within 1e-4 of the fp32 oracle; on outputs of scale 0.1 .. 1 that is several hundred
times the error of a plain fp32 evaluation, so a kernel could lose bits (a dropped partial product, a coarse reciprocal, a
weight operand rounded short) and still pass.  Here each route is forced with the options the suite already uses and its
output must meet ``ref64.budget``: ``e <= K * e32 + F`` relative to the output scale, where ``e32`` is the fp32 oracle's own
error against float64 on the same inputs (K, F and the worst measured ``e / e32`` per route: DESIGN.md section 4).

Math modes: bf16x6 (math 1) is an fp32-equivalent mode and gets the fp32 budget wherever it changes kernels; f16x3 (math 3)
gets it on uniform(-1, 1) inputs, as the README claims; bf16x3 (math 2) is reduced precision by design and has its own
relative bound.  The 2^8 / 2^-8 scaled inputs run in math 0 and 1 only: f16x3's mid piece is an fp16 subnormal once
|x| < 0.25, which leaves an absolute error floor of ~3e-8 per operand element -- outside a relative budget."""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

import bench
import ref64 as R
from gnnbuilder_amd import runtime, synthetic
from gnnbuilder_amd.batching import order_large_last, pack_graphs
from helpers import EMPTY, ONE, canon, hub_graph, make_model, to_dev
from oracle import oracle as O

pytestmark = pytest.mark.gpu

# the process-wide defaults of every option this file sets (gnnb_runtime.hip options())
DEFAULTS = {"math": 0, "fuse_zf": 1, "zf_shape": 2, "zf_head": 0, "fuse_gcn2": 1, "stage_cut": 0, "large_fork": 2, "fuse_narrow": 1,
            "first_ring": 1, "pna_classes": 1, "pna_pagg": 1, "pna_first": 1, "pna_fold_lin": 1, "sage_first_mean": 1,
            "head_small": 1, "head_pairs": 1, "head_split": 0, "fuse_pool": 1, "fold_skip": 1}
# math 2 (bf16x3: hi + mid bf16 pieces of both operands of k_gcn2_zf's wide update, ~16 significant bits per product): max error
# relative to the output scale against float64.  README C2: 6.4e-7 absolute; measured here at C2 shape: 2.76e-6 relative; bound 3x that
BF16X3_BOUND = 8.3e-6
WORST = {}  # route -> worst e / e32 (reported with GNNB_FP64_REPORT=<file>, for the calibration in DESIGN.md section 4)


@pytest.fixture(scope="module", autouse=True)
def _library():
    runtime.load_library(require_gpu=True)  # fails loudly: no fallback
    yield
    report = os.environ.get("GNNB_FP64_REPORT")
    if report:  # (merged with what test_hip_stage_fp64.py wrote there)
        have = {}
        if os.path.exists(report):
            with open(report) as f:
                have = json.load(f)
        have.update(WORST)
        with open(report, "w") as f:
            json.dump(dict(sorted(have.items())), f, indent=1)


@contextlib.contextmanager
def options(**kw):
    try:
        for k, v in kw.items():
            runtime.set_option(k, v)
        yield
    finally:
        for k in kw:
            runtime.set_option(k, DEFAULTS[k])


def references(model, batch, x):
    """(float64 model output, fp32 oracle output) for ``check``: computed once where several cases share a model and a batch."""
    return R.forward64(model, batch, x), O.forward_batched(model.spec(), canon(model), x, batch.coo, batch.node_ptr, batch.edge_ptr)


def check(route, got, model, batch, x, k=R.K, refs=None):
    """``got`` against the float64 model within the fp32 budget; records e / e32 under ``route``."""
    ref, base = refs if refs is not None else references(model, batch, x)
    e, e32 = R.budget(got, ref, base, k=k, what=route)
    WORST[route] = max(WORST.get(route, 0.0), R.ratio(e, e32))
    return ref


def hip(model, batch, x, promise=0, maxdeg=0, **opts):
    """One forward through the C ABI with ``opts`` set; (output, reported path)."""
    with options(**opts):
        cm = runtime.CompiledModel.from_model(model, batch.num_graphs, batch.num_nodes, max(batch.num_edges, 1), max_graph_nodes=promise)
        if maxdeg:
            cm.set_max_degree(maxdeg)
        _, coo, nptr, eptr = to_dev(batch, dev_())
        out = cm.forward(torch.from_numpy(x).to(dev_()), coo, nptr, eptr).cpu().numpy()
        cm.check()
        path = cm.last_path()
        cm.close()
    return out, path


def dev_():
    return torch.device("cuda:0")


def uniform_x(batch, fin, seed, scale=1.0):
    return (scale * np.random.default_rng(seed).uniform(-1, 1, (batch.num_nodes, fin))).astype(np.float32)


def regraphed(batch, fin, seed, extra=()):
    """``batch``'s graphs with uniform(-1, 1) features of width ``fin``, plus ``extra`` graphs."""
    rng = np.random.default_rng(seed)
    graphs = [(rng.uniform(-1, 1, (batch.graph(g)[0].shape[0], fin)).astype(np.float32), batch.graph(g)[1]) for g in range(batch.num_graphs)]
    return pack_graphs(graphs + list(extra))




# --------------------------------------------------------------------------- k_gcn2_zf (the benched 2-layer GCN stack)
@pytest.mark.parametrize("shape,head,fin,act", [(0, 0, 11, "relu"), (1, 1, 20, "tanh"), (2, 0, 32, "gelu"), (2, 1, 16, "sigmoid"),
                                                (2, 0, 11, "relu")], ids=lambda v: str(v))
@pytest.mark.parametrize("math", [0, 1, 3])
def test_stack_zf(shape, head, fin, act, math):
    model = make_model("gcn", in_dim=fin, hidden=128, layers=2, act=act, mlp_act=act, task_out=7, seed=fin + shape)
    batch = regraphed(synthetic.make_batch("qm9", 300, seed=shape), fin, fin, [hub_graph(61, fin, 600, 1), EMPTY(fin), ONE(fin)])
    got, path = hip(model, batch, batch.x, promise=61, math=math, zf_shape=shape, zf_head=head)
    assert path == "stack_zf"
    check(f"stack_zf math{math}", got, model, batch, batch.x)


@pytest.mark.parametrize("scale", [2.0 ** 8, 2.0 ** -8], ids=["x2^8", "x2^-8"])
@pytest.mark.parametrize("math", [0, 1])  # (not 3: the f16x3 mid piece is subnormal below |x| = 0.25 -- module docstring)
def test_stack_zf_scaled_inputs(scale, math):
    model = make_model("gcn", in_dim=11, hidden=128, layers=2, act="tanh", mlp_act="relu", task_out=5, seed=3)
    batch = synthetic.make_batch("qm9", 300, seed=4)
    x = uniform_x(batch, 11, 5, scale)
    got, path = hip(model, batch, x, promise=29, math=math)
    assert path == "stack_zf"
    check(f"stack_zf math{math}", got, model, batch, x)


def test_stack_zf_all_negative_max_pool():
    """tanh with a last bias of -2: every pooled activation is negative, so a max that starts at 0 shows; 1- and 0-node graphs."""
    model = make_model("gcn", in_dim=11, hidden=128, layers=2, act="tanh", pools=("max", "add", "mean"), task_out=5, seed=6)
    with torch.no_grad():
        model.gnn_convs[-1].conv.bias.fill_(-2.0)
    batch = regraphed(synthetic.make_batch("qm9", 300, seed=6), 11, 6, [ONE(11), EMPTY(11), ONE(11)])
    x = 0.25 * batch.x
    for name, opts in (("stack_zf", {}), ("stack", {"fuse_zf": 0}), ("layerwise", {"fuse_gcn2": 0})):
        got, path = hip(model, batch, x, promise=29 if name != "layerwise" else 0, **opts)
        assert path == name
        check(f"{name} math0", got, model, batch, x)


# --------------------------------------------------------------------------- k_gcn2_fused: deep GCN / GIN stacks
@pytest.mark.parametrize("conv,layers,act,cut", [("gcn", 3, "relu", 0), ("gcn", 4, "tanh", 1), ("gcn", 6, "gelu", 0), ("gcn", 5, "sigmoid", 1),
                                                 ("gin", 2, "relu", 1), ("gin", 3, "tanh", 0), ("gin", 4, "gelu", 1), ("gin", 3, "sigmoid", 0)],
                         ids=lambda v: str(v))
@pytest.mark.parametrize("math", [0, 1, 3])
def test_stack(conv, layers, act, cut, math):
    model = make_model(conv, in_dim=9, hidden=128 if layers < 5 else 64, layers=layers, act=act, mlp_act=act, task_out=3, seed=layers)
    if conv == "gin":
        eps = float(np.random.default_rng(layers).uniform(-0.5, 0.5))
        for c in model.gnn_convs:
            c.eps = eps
            c.conv.eps.fill_(eps)
    batch = regraphed(synthetic.make_batch("qm9", 250, seed=layers), 9, layers, [hub_graph(61, 9, 600, 2), EMPTY(9), ONE(9)])
    got, path = hip(model, batch, batch.x, promise=61, math=math, fuse_zf=0, stage_cut=cut)
    assert path == "stack"
    check(f"stack math{math}", got, model, batch, batch.x)


@pytest.mark.parametrize("scale", [2.0 ** 8, 2.0 ** -8], ids=["x2^8", "x2^-8"])
@pytest.mark.parametrize("math", [0, 1])  # (not 3: module docstring)
def test_stack_scaled_inputs_and_saturation(scale, math):
    """x 2^8 through sigmoid drives pre-activations far beyond +-20 (saturation); x 2^-8 keeps them near the biases."""
    model = make_model("gin", in_dim=9, hidden=128, layers=3, act="sigmoid", mlp_act="tanh", task_out=3, seed=8)
    batch = synthetic.make_batch("molhiv", 200, seed=8)
    x = uniform_x(batch, 9, 8, scale)
    got, path = hip(model, batch, x, promise=int(np.diff(batch.node_ptr).max()), math=math)
    assert path == "stack"
    check(f"stack math{math}", got, model, batch, x)


# --------------------------------------------------------------------------- layer by layer
# (math 1 / 3 change the SAGE / PNA kernels of this route, not GCN's or GIN's)
@pytest.mark.parametrize("conv,act,math", [("gcn", "relu", 0), ("gin", "tanh", 0), ("sage", "gelu", 0), ("pna", "sigmoid", 0), ("sage", "relu", 1),
                                           ("pna", "tanh", 1), ("sage", "sigmoid", 3), ("pna", "gelu", 3)], ids=lambda v: str(v))
def test_layerwise(conv, act, math):
    """No promise; a hub of in-degree 1200 (one 300-node graph), empty and one-node graphs."""
    model = make_model(conv, in_dim=11, hidden=128, layers=3, act=act, mlp_act=act, task_out=4, seed=11)
    batch = regraphed(synthetic.make_batch("qm9", 250, seed=12), 11, 12, [hub_graph(300, 11, 1200, 3), EMPTY(11), ONE(11)])
    got, path = hip(model, batch, batch.x, math=math, fuse_gcn2=0)
    assert path == "layerwise"
    check(f"layerwise math{math}", got, model, batch, batch.x)


@pytest.mark.parametrize("conv", ["sage", "pna"])
@pytest.mark.parametrize("scale", [2.0 ** 8, 2.0 ** -8], ids=["x2^8", "x2^-8"])
@pytest.mark.parametrize("math", [0, 1])  # (not 3: module docstring)
def test_layerwise_scaled_inputs(conv, scale, math):
    model = make_model(conv, in_dim=11, hidden=128, layers=2, act="tanh", task_out=4, seed=13)
    batch = synthetic.make_batch("qm9", 250, seed=13)
    x = uniform_x(batch, 11, 13, scale)
    got, path = hip(model, batch, x, math=math)
    assert path == "layerwise"
    # K = 6 for PNA at 2^8: its std is sqrt(E[h^2] - E[h]^2); where a node's messages (nearly) coincide, the rounding of
    # E[h^2] at |h| ~ 2^8 leaves a spurious std of ~2^-12 |h| whose size depends on the summation order, so two honest fp32
    # evaluations differ more there than elsewhere (measured e/e32 4.8 in math 0 and 1, with the oracle's own error 1.9e-5 here, ~100x the other routes')
    check(f"layerwise math{math}" + (" pna x2^8" if conv == "pna" and scale > 1 else ""), got, model, batch, x,
          k=6.0 if conv == "pna" and scale > 1 else R.K)


def _pna_batch(fin):
    """QM9-shaped graphs (max in-degree <= 15 once the stars are in) plus stars whose leaves carry identical features and no
    in-edges: the centre's messages are identical in every layer, its std is exactly 0 -- next to molecules whose std is far
    above PyG's sqrt(1e-5) threshold.  No inputs near the threshold: the std is discontinuous there, and float64 would
    legitimately land on the other side of it."""
    base = synthetic.make_batch("qm9", 250, seed=21)
    rng = np.random.default_rng(fin)
    stars = []
    for k in (3, 9, 15):
        x = np.repeat(rng.uniform(-1, 1, (1, fin)), k + 1, 0).astype(np.float32)
        x[0] = rng.uniform(-1, 1, fin)
        stars.append((x, np.stack([np.arange(1, k + 1), np.zeros(k, np.int64)], 1).astype(np.int32)))
    return regraphed(base, fin, fin, stars + [EMPTY(fin), ONE(fin)])


@pytest.mark.parametrize("classes,pagg,first,fold", [(1, 1, 1, 1), (0, 0, 0, 0), (1, 0, 1, 0), (0, 1, 0, 1)], ids=lambda v: str(v))
@pytest.mark.parametrize("math", [0, 1, 3])
def test_pna_degree_promise(classes, pagg, first, fold, math):
    model = make_model("pna", in_dim=11, hidden=128, layers=3, act="relu", task_out=3, seed=22)
    batch = _pna_batch(11)
    maxdeg = int(np.bincount(batch.coo[:, 1]).max())
    assert maxdeg <= 15
    got, path = hip(model, batch, batch.x, promise=int(np.diff(batch.node_ptr).max()), maxdeg=maxdeg, math=math, pna_classes=classes,
                    pna_pagg=pagg, pna_first=first, pna_fold_lin=fold)
    assert path == "layerwise"
    check(f"pna_promise math{math}", got, model, batch, batch.x)


@pytest.mark.parametrize("on", [1, 0])
@pytest.mark.parametrize("act", ["gelu", "sigmoid"])
def test_sage_first_mean(on, act):
    model = make_model("sage", in_dim=9, hidden=256, layers=3, act=act, task_out=3, seed=23)
    batch = regraphed(synthetic.make_batch("molhiv", 250, seed=23), 9, 23, [hub_graph(40, 9, 300, 4), EMPTY(9), ONE(9)])
    got, path = hip(model, batch, batch.x, promise=int(np.diff(batch.node_ptr).max()), sage_first_mean=on)
    assert path == "layerwise"
    check("sage_first_mean", got, model, batch, batch.x)


@pytest.mark.parametrize("conv,fin", [("gcn", 11), ("gin", 9), ("sage", 16)])
@pytest.mark.parametrize("narrow,ring", [(1, 1), (1, 0), (0, 1)])
def test_narrow_first_layer(conv, fin, narrow, ring):
    model = make_model(conv, in_dim=fin, hidden=128, layers=2, act="tanh", task_out=3, seed=fin)
    batch = regraphed(synthetic.make_batch("molhiv", 250, seed=fin), fin, fin, [hub_graph(300, fin, 1200, 5)])
    got, path = hip(model, batch, batch.x, fuse_gcn2=0, fuse_narrow=narrow, first_ring=ring)
    assert path == "layerwise"
    check("narrow_first", got, model, batch, batch.x)


@pytest.mark.parametrize("fork", [0, 1, 2])
@pytest.mark.parametrize("conv,layers,limit", [("gcn", 2, 40), ("gin", 3, 57)])
def test_large_segment(conv, layers, limit, fork):
    model = make_model(conv, in_dim=9, hidden=128, layers=layers, act="relu", pools=("add", "max", "mean"), task_out=3, seed=5)
    b0 = synthetic.make_batch("molhiv_tail", 300, seed=11)
    batch = pack_graphs([b0.graph(g) for g in range(150)] + [hub_graph(300, 9, 1200, 6), EMPTY(9)] + [b0.graph(g) for g in range(150, 300)])
    ordered, perm, (g0, n0, e0) = order_large_last(batch, limit)
    assert g0 < ordered.num_graphs
    with options(large_fork=fork):
        cm = runtime.CompiledModel.from_model(model, ordered.num_graphs, ordered.num_nodes, ordered.num_edges,
                                              max_graph_nodes=int(np.diff(ordered.node_ptr)[:g0].max()))
        cm.set_large_segment(g0, n0, e0)
        got = cm.forward(*to_dev(ordered, dev_())).cpu().numpy()
        cm.check()
        assert cm.last_path() in ("stack+large_layerwise", "stack_zf+large_layerwise"), cm.last_path()
        cm.close()
    check("large_segment", got, model, ordered, ordered.x)


@pytest.mark.parametrize("small,pairs", [(1, 1), (1, 0), (0, 1)])
@pytest.mark.parametrize("mlp_hidden,mlp_layers,task_out,out_act", [(64, 2, 19, None), (50, 2, 7, torch.nn.Softmax), (128, 3, 33, torch.nn.LogSoftmax)])
def test_readouts(small, pairs, mlp_hidden, mlp_layers, task_out, out_act):
    model = make_model("gcn", in_dim=11, hidden=64, layers=2, pools=("add", "mean", "max"), mlp_hidden=mlp_hidden, mlp_layers=mlp_layers,
                       task_out=task_out, mlp_act="tanh", seed=mlp_hidden)
    if out_act is not None:
        model.output_activation = out_act
        model.output_activation_module = out_act(dim=-1)
    batch = synthetic.make_batch("qm9", 203, seed=task_out)
    got, path = hip(model, batch, batch.x, promise=29, head_small=small, head_pairs=pairs)
    assert path == "stack_zf"
    check("readout", got, model, batch, batch.x)


def test_forward_host():
    for conv, promise in (("gcn", 29), ("sage", 0)):
        model = make_model(conv, in_dim=11, hidden=128, layers=2, act="gelu", task_out=5, seed=31)
        batch = synthetic.make_batch("qm9", 200, seed=31)
        cm = runtime.CompiledModel.from_model(model, batch.num_graphs, batch.num_nodes, batch.num_edges, max_graph_nodes=promise)
        got = cm.forward_host(batch.x, batch.coo, batch.node_ptr, batch.edge_ptr)
        cm.check()
        assert cm.last_path() == ("stack_zf" if promise else "layerwise")
        cm.close()
        check("forward_host", got, model, batch, batch.x)


# --------------------------------------------------------------------------- GINE / Simple / LGConv (no GNNModel form)
def test_weight_free_and_gine_convs():
    """Against a float64 statement of the oracle's formulas, graph by graph; hub of in-degree 1200, isolated nodes."""
    rng = np.random.default_rng(41)
    fin, edim = 32, 5
    b = regraphed(synthetic.make_batch("molhiv", 100, seed=41), fin, 41, [hub_graph(300, fin, 1200, 7), ONE(fin), EMPTY(fin)])
    ea = rng.uniform(-1, 1, (b.num_edges, edim)).astype(np.float32)
    ws = [rng.uniform(-0.5, 0.5, s).astype(np.float32) for s in ((fin, edim), (fin,), (64, fin), (64,), (24, 64), (24,))]
    cm = runtime.CompiledModel.from_model(make_model("gin", in_dim=fin, hidden=8, layers=1, out_dim=8, task_out=3, mlp_layers=0),
                                          b.num_graphs, b.num_nodes, b.num_edges)
    xd, cood, nptr, eptr = to_dev(b, dev_())
    cm.graph_prep(cood, nptr, eptr, b.num_nodes)
    got = {"simple": cm.aggregate("simple", xd).cpu().numpy(), "lg": cm.aggregate("lg", xd).cpu().numpy(),
           "gine": cm.gine_conv(xd, torch.from_numpy(ea).to(dev_()), *[torch.from_numpy(t).to(dev_()) for t in ws], eps=0.3).cpu().numpy()}
    cm.check()
    cm.close()
    for kind, g in got.items():
        ref, base = [], []
        for i in range(b.num_graphs):
            lo, hi = b.node_ptr[i], b.node_ptr[i + 1]
            if hi == lo:
                continue
            xg, cg, eg = b.x[lo:hi], b.coo[b.edge_ptr[i]:b.edge_ptr[i + 1]] - lo, ea[b.edge_ptr[i]:b.edge_ptr[i + 1]]
            if kind == "gine":
                ref.append(R.gine64(xg, cg, eg, ws, eps=0.3))
                base.append(O.gine_conv(xg, cg, eg, ws, eps=0.3))
            else:
                ref.append({"simple": R.simple64, "lg": R.lg64}[kind](xg, cg))
                base.append(O.conv(kind, xg, cg, []))
        e, e32 = R.budget(g, np.concatenate(ref), np.concatenate(base), what=kind)
        WORST[kind] = max(WORST.get(kind, 0.0), R.ratio(e, e32))


# --------------------------------------------------------------------------- the large-K GEMM (SAGE / PNA updates)
@pytest.mark.parametrize("math", [0, 1, 3])
def test_large_k_gemm(math):
    """Four segments (two row-scaled, as PNA's scalers), bias + skip + tanh, a stream-K tail: fp32 budget against float64, with
    an fp32 CPU product as the base."""
    M, N, Fw = 70000, 128, 32
    g = torch.Generator().manual_seed(M + N)
    x, A = torch.rand(M, Fw, generator=g) - 0.5, torch.rand(M, 4 * Fw, generator=g) - 0.5
    amp, att = torch.rand(M, generator=g) + 0.5, torch.rand(M, generator=g) + 0.5
    w = (torch.rand(N, 13 * Fw, generator=g) - 0.5) / (13 * Fw) ** 0.5
    b, skip = torch.rand(N, generator=g), torch.rand(M, N, generator=g) - 0.5
    rows = torch.cat([torch.arange(0, 3000), torch.arange(M - 3000, M)])
    cat = torch.cat([x, A, A * amp[:, None], A * att[:, None]], 1)[rows]
    ref = torch.tanh(cat.double() @ w.double().T + b.double() + skip[rows].double()).numpy()
    base = torch.tanh(cat @ w.T + b + skip[rows]).numpy()
    Ad = A.to(dev_())
    segs = [(x.to(dev_()), None), (Ad, None), (Ad, amp.to(dev_())), (Ad, att.to(dev_()))]
    with options(math=math):
        got = runtime.linear(segs, w.to(dev_()), b.to(dev_()), skip=skip.to(dev_()), act="tanh").cpu()[rows].numpy()
    e, e32 = R.budget(got, ref, base, what=f"large-K GEMM math {math}")
    WORST[f"large_k_gemm math{math}"] = R.ratio(e, e32)


# --------------------------------------------------------------------------- C2 at full size (README accuracy line)
@pytest.mark.parametrize("math", [0, 2, 3])
def test_config2_full_size(math):
    """BASELINE config 2 (4096 QM9-shaped graphs, 2-layer GCN d128, k_gcn2_zf) against float64: math 0 and 3 in the fp32
    budget, math 2 (bf16x3) within its own bound (README: 7.1e-8 / 6.4e-7 / 7.5e-8 relative to the output scale)."""
    w = bench.WORKLOADS["c2"]
    model = bench.build_model(w)
    batch = synthetic.make_batch(w["shape"], w["batch"], seed=3)
    got, path = hip(model, batch, batch.x, promise=int(np.diff(batch.node_ptr).max()), math=math)
    assert path == "stack_zf"
    if math == 2:
        ref = R.forward64(model, batch, batch.x)
        e = R.errors(got, ref, ref)[0]
        WORST["c2 math2 (relative error)"] = e
        assert e < BF16X3_BOUND, e
    else:
        check(f"c2 math{math}", got, model, batch, batch.x)
