"""The C-ABI stage entry points and wide / odd-width models against float64, with the fp32-class budget of ref64.

test_hip_fp64.py holds every forward route to ``ref64.budget`` with the shapes the forward passes.  An outside caller of the
stage entries (``gnnb_linear``, ``gnnb_aggregate``, ``gnnb_global_pool``, ``gnnb_aggregate_edges``,
``gnnb_pna_product_aggregate``: INTEGRATION.md section 3) can pass layouts the forward never makes -- column slices (``lda``,
``ldw`` wider than the operand), base pointers one float past a 16-byte boundary, widths that are not multiples of 4 -- and
each kernel picks its vector or scalar form and its kernel family from exactly those properties.  Here every such form is
reached on purpose and compared with a float64 restatement of the same operation (ref64: ``linear64``, ``gcn_agg64`` ...).
``base`` is an fp32 evaluation of the same formula: the ref64 forms in float32 (neighbours in CSR order, self term last) for
the aggregates and pooling, a float32 torch CPU product for the GEMMs.

Where each form is reached (gnnb_runtime.hip ``build_gemm``, gemm_launch.hip ``launch_linear``, k_aggregate.hip ``launch_aggregate``):
  * scalar GEMM operands (``avec`` / ``wvec`` = 0): the ``a_slice`` / ``w_slice`` / ``offset`` layouts and every odd K;
  * scalar epilogue (``vec`` = 0): odd N, or the ``offset`` layout (bias, skip, out one float in);
  * scalar aggregate / pooling / GINE forms (``v4`` = 0): odd widths and the offset x / self_dev / out views;
  * the ring aggregate's ``big`` direct path (a node tile larger than a stage): widths 1024 and 2048 (PNA: 1024), where
    ``cap = 158 KB / slots / per_row`` is below a node tile's rows for most tiles, and the 300-node graph's hub tile;
  * the GEMM-chain fallback behind ``launch_readout_fused``: every model of ``test_wide_and_odd_models`` (a head of > 158 KB of weights, or
    a pooled width ``d`` that is not a multiple of 4); ``fuse_head = 0`` forces the same chain and must agree.
"""
import contextlib
import json
import os
import zlib

import numpy as np
import pytest
import torch

import ref64 as R
from gnnbuilder_amd import runtime
from helpers import edge_batch, grid_features, make_model, to_dev

pytestmark = pytest.mark.gpu

# the process-wide defaults of every option this file sets (gnnb_runtime.hip options())
DEFAULTS = {"math": 0, "gemm_wlds": 1, "gemm_variant": 0, "gemm_dma": 1, "gemm_tail_split": 2, "agg_form": 0, "agg_balance": 0,
            "fuse_head": 1, "pna_pagg": 1}
WORST = {}  # entry -> worst e / e32 (merged into GNNB_FP64_REPORT=<file> with test_hip_fp64.py's)


@pytest.fixture(scope="module", autouse=True)
def _library():
    runtime.load_library(require_gpu=True)  # fails loudly: no fallback
    yield
    report = os.environ.get("GNNB_FP64_REPORT")
    if report:
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


def dev_():
    return torch.device("cuda:0")


def record(entry, got, ref, base, k=R.K):
    e, e32 = R.budget(got, ref, base, k=k, what=entry)
    WORST[entry] = max(WORST.get(entry, 0.0), R.ratio(e, e32))


def on_device(a, offset=False):
    """``a`` (numpy) as a contiguous CUDA tensor; ``offset``: starting one float past a 16-byte boundary of its buffer."""
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32))
    if not offset:
        return t.to(dev_())
    buf = torch.zeros(t.numel() + 4, dtype=torch.float32, device=dev_())
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


# --------------------------------------------------------------------------- gnnb_linear
# every GEMM family, forced through the options that choose it (gemm_launch.hip launch_linear); the predicates then still pick
# the family's scalar form (or the next family) from the operands' layout
FAMILIES = {"wlds": {}, "reg": {"gemm_wlds": 0}, "dma_tail2": {"gemm_variant": 1}, "dma_tail1": {"gemm_variant": 1, "gemm_tail_split": 1},
            "dma_tail0": {"gemm_variant": 1, "gemm_tail_split": 0}, "generic": {"gemm_variant": 1, "gemm_dma": 0}}
KS, NS, MS = (1, 3, 11, 33, 64, 128, 129, 1056), (1, 3, 31, 32, 33, 63, 64, 65, 129, 257), (0, 1, 127, 128, 129, 3000)
LAYOUTS = ("contiguous", "a_slice", "w_slice", "offset")
ACTS = ("none", "relu", "gelu", "sigmoid", "tanh")


def _gemm_cases():
    """Seeded random selection over (family, layout, K per segment, N, M, segments, row scales, activation, skip), every
    value of each axis at least once; plus the shapes that reach the weights-in-LDS and LDS-DMA kernels' vector forms, and
    a math 1 / math 3 subset (as test_hip_fp64.test_large_k_gemm)."""
    rng = np.random.default_rng(2026)
    cases = []
    for i in range(72):
        nseg = 1 + i % 4 if i % 3 else 1
        ks = tuple(int(KS[(i + 3 * s) % len(KS)] if s == 0 else rng.choice(KS[:6])) for s in range(nseg))
        cases.append(dict(family=list(FAMILIES)[i % len(FAMILIES)], layout=LAYOUTS[(i // 6) % 4], ks=ks, n=NS[i % len(NS)],
                          m=MS[(i // 2) % len(MS)], rowscale=bool(i % 5 == 1 or (nseg > 1 and i % 2)), act=ACTS[i % 5],
                          skip=bool(i % 4 == 3), math=0))
    for fam in FAMILIES:  # the vector forms: K, N in {64, 128}, aligned, no skip (weights in LDS) / K % 32 == 0 (LDS-DMA)
        for k, n in ((64, 64), (128, 128), (128, 257), (1056, 129)):
            cases.append(dict(family=fam, layout="contiguous", ks=(k,), n=n, m=3000, rowscale=False, act="tanh", skip=False, math=0))
    for math in (1, 3):
        for fam, layout, ks, n in (("reg", "contiguous", (128,), 128), ("dma_tail2", "contiguous", (64, 1056), 257),
                                   ("dma_tail1", "offset", (33, 64), 129), ("generic", "a_slice", (129,), 65)):
            cases.append(dict(family=fam, layout=layout, ks=ks, n=n, m=3000, rowscale=True, act="gelu", skip=True, math=math))
    return cases


GEMM_CASES = _gemm_cases()


def _gemm_id(c):
    return f"{c['family']}-{c['layout']}-K{'+'.join(map(str, c['ks']))}-N{c['n']}-M{c['m']}-{c['act']}" + \
           ("-rs" if c["rowscale"] else "") + ("-skip" if c["skip"] else "") + (f"-math{c['math']}" if c["math"] else "")


def _run_gemm(c, seed):
    g = np.random.default_rng(seed)
    M, N, ks, layout = c["m"], c["n"], c["ks"], c["layout"]
    K = sum(ks)
    mrows = max(M, 1)  # (M = 0: views of a one-row buffer, so that no pointer is null)
    segs_h, segs_d = [], []
    for s, k in enumerate(ks):
        if layout == "a_slice":  # lda = k + 5 - (k % 4 == 3): never a multiple of 4, the slice starts 3 floats in
            lda = k + 3 + (2 if (k + 5) % 4 else 3)
            buf = g.uniform(-1, 1, (mrows, lda)).astype(np.float32)
            a_h = buf[:M, 3:3 + k]
            a_d = torch.from_numpy(buf).to(dev_())[:M, 3:3 + k]
            assert a_d.stride(0) == lda and lda % 4
        else:
            a_h = g.uniform(-1, 1, (M, k)).astype(np.float32)
            a_d = on_device(a_h, layout == "offset") if M else on_device(g.uniform(-1, 1, (1, k)), layout == "offset")[:0]
        rs_h = (g.uniform(0.5, 1.5, M).astype(np.float32) if c["rowscale"] else None)
        rs_d = None if rs_h is None else (on_device(rs_h) if M else on_device(np.ones(1))[:0])
        segs_h.append((a_h, rs_h))
        segs_d.append((a_d, rs_d))
    scale = 1.0 / np.sqrt(K)
    if layout == "w_slice":  # ldw = K + 5, the slice starts one float in: koff of every segment after an odd K is odd too
        wbuf = (g.uniform(-1, 1, (N, K + 5)) * scale).astype(np.float32)
        w_h = wbuf[:, 1:1 + K]
        w_d = torch.from_numpy(wbuf).to(dev_())[:, 1:1 + K]
    else:
        w_h = (g.uniform(-1, 1, (N, K)) * scale).astype(np.float32)
        w_d = on_device(w_h, layout == "offset")
    b_h = g.uniform(-0.5, 0.5, N).astype(np.float32)
    sk_h = g.uniform(-0.5, 0.5, (M, N)).astype(np.float32) if c["skip"] else None
    off = layout == "offset"
    b_d = on_device(b_h, off)
    sk_d = None if sk_h is None else (on_device(sk_h, off) if M else on_device(np.zeros((1, N)), off)[:0])
    out_buf = torch.full((mrows * N + 4,), 7.0, dtype=torch.float32, device=dev_())
    out_d = out_buf[1:1 + M * N].view(M, N) if off else out_buf[:M * N].view(M, N)
    with options(math=c["math"], **FAMILIES[c["family"]]):
        runtime.linear(segs_d, w_d, b_d, skip=sk_d, act=c["act"], out=out_d)
    torch.cuda.synchronize()
    return segs_h, w_h, b_h, sk_h, out_d.cpu().numpy(), out_buf


@pytest.mark.parametrize("case", GEMM_CASES, ids=_gemm_id)
def test_linear(case):
    segs, w, b, sk, got, out_buf = _run_gemm(case, zlib.crc32(_gemm_id(case).encode()))
    if case["m"] == 0:  # OK, and nothing written
        assert bool((out_buf == 7.0).all())
        return
    ref = R.linear64(segs, w, b, sk, case["act"])
    base = R.linear64(segs, w, b, sk, case["act"], dtype=torch.float32)
    record(f"linear {case['family']} math{case['math']}", got, ref, base)


def test_linear_axes_are_covered():
    for axis, values in (("ks", KS), ("n", NS), ("m", MS), ("layout", LAYOUTS), ("act", ACTS), ("family", tuple(FAMILIES))):
        seen = {v for c in GEMM_CASES for v in (c[axis] if axis == "ks" else (c[axis],))}
        assert set(values) <= seen, (axis, set(values) - seen)
    assert {len(c["ks"]) for c in GEMM_CASES} == {1, 2, 3, 4}


# --------------------------------------------------------------------------- gnnb_aggregate
AGG_WIDTHS = (1, 3, 5, 33, 64, 100, 128, 130, 256, 257, 1024, 2048)
# (kind, eps, PNA destination term): every gnnb_agg kind but COPY
AGG_KINDS = (("gcn", 0.0, False), ("sum", 0.25, False), ("sum", -0.5, False), ("mean", 0.0, False), ("pna", 0.0, False),
             ("pna", 0.0, True), ("lg", 0.0, False), ("simple", 0.0, False))
# (agg_form, agg_balance, offset operands): a half fraction of the 2^3 -- every pair of the three appears
VARIANTS = ((0, 0, False), (1, 0, True), (0, 1, True), (1, 1, False))


def _ref_agg(kind, x, coo, eps, q, dtype):
    if kind == "gcn":
        return R.gcn_agg64(x, coo, dtype=dtype)
    if kind == "sum":
        return R.sum_agg64(x, coo, eps, dtype=dtype)
    if kind == "mean":
        return R.mean_agg64(x, coo, dtype=dtype)
    if kind == "pna":
        return R.pna_agg64(x, coo, q, dtype=dtype)
    return {"lg": R.lg64, "simple": R.simple64}[kind](x, coo, dtype=dtype)


@pytest.fixture(scope="module")
def agg_batch():
    """300 molecules (>= 256 node tiles: the row-balanced ranges of agg_balance = 1 exist for the ring's grid), a graph with
    explicit self loops, duplicate edges and isolated nodes, a 300-node graph with a hub of in-degree 1200, an empty and
    a one-node graph."""
    b = edge_batch(300, 1, 31)
    assert int(np.bincount(b.coo[:, 1]).max()) >= 1200 and (b.coo[:, 0] == b.coo[:, 1]).any()
    return b


@pytest.fixture(scope="module")
def workspaces(agg_batch):
    """(gcn workspace?, agg_balance) -> a CompiledModel with the batch prepared (the balance is read at graph prep)."""
    b = agg_batch
    out = {}
    for conv in ("gcn", "gin"):
        for bal in (0, 1):
            cm = runtime.CompiledModel.from_model(make_model(conv, in_dim=4, hidden=8, layers=1, out_dim=8, task_out=2, mlp_layers=1),
                                                  b.num_graphs, b.num_nodes, b.num_edges)
            _, coo, nptr, eptr = to_dev(b, dev_())
            with options(agg_balance=bal):
                cm.graph_prep(coo, nptr, eptr, b.num_nodes)
            out[(conv == "gcn", bal)] = cm
    yield out
    for cm in out.values():
        cm.close()


# every kind at every width on a workspace of another model; on a GCN workspace (explicit self loops absent from its tables for
# every kind) a subset of the widths; PNA up to width 1024
AGG_CASES = [(gcn_ws, w, *k) for gcn_ws in (False, True) for w in AGG_WIDTHS for k in AGG_KINDS
             if not (k[0] == "pna" and w > 1024) and not (gcn_ws and w not in (1, 3, 33, 128, 130, 1024))]


@pytest.mark.parametrize("gcn_ws,width,kind,eps,self_term", AGG_CASES,
                         ids=[f"{'gcn_ws' if c[0] else 'other_ws'}-w{c[1]}-{c[2]}{c[3]:g}{'-q' if c[4] else ''}" for c in AGG_CASES])
def test_aggregate(gcn_ws, width, kind, eps, self_term, agg_batch, workspaces):
    """Widths 1024 and 2048 (PNA: 1024) reach the ring's ``big`` direct path; odd widths and the offset views its scalar form;
    agg_form 1 the register-gather kernel at widths 64 / 128 / 256 (aligned operands)."""
    b = agg_batch
    x = grid_features(b.num_nodes, width, width) if kind == "pna" else \
        np.random.default_rng(width).uniform(-1, 1, (b.num_nodes, width)).astype(np.float32)
    q = np.random.default_rng(width + 1).uniform(-1, 1, x.shape).astype(np.float32) if self_term else None
    coo = R.workspace_edges(b.coo, gcn_ws)
    ref, base = _ref_agg(kind, x, coo, eps, q, np.float64), _ref_agg(kind, x, coo, eps, q, np.float32)
    for form, bal, off in VARIANTS:
        cm = workspaces[(gcn_ws, bal)]
        xd, qd = on_device(x, off), (on_device(q, off) if q is not None else None)
        out = on_device(np.full_like(ref, np.nan), off)  # (NaN: a row the kernel skips fails the budget)
        with options(agg_form=form, agg_balance=bal):  # (read at graph prep for the cut table AND at launch, which uses it)
            cm.aggregate(kind, xd, self_term=qd, eps=eps, out=out)
        cm.check()
        record(f"aggregate {kind}{' q' if self_term else ''} form{form}", out.cpu().numpy(), ref, base)


# --------------------------------------------------------------------------- gnnb_global_pool
@pytest.mark.parametrize("d", [1, 3, 7, 33, 130, 1024])
def test_global_pool(d):
    """Every order of 1 to 3 pools; all-negative inputs (a max that starts at 0 shows); empty and one-node graphs; a
    2000-node graph; an offset x (scalar form)."""
    from gnnbuilder_amd.batching import pack_graphs
    from helpers import EMPTY, ONE
    rng = np.random.default_rng(d)
    graphs = [(rng.uniform(-1, 1, (int(n), d)).astype(np.float32), np.zeros((0, 2), np.int32)) for n in rng.integers(1, 30, 60)]
    batch = pack_graphs(graphs[:30] + [EMPTY(d), ONE(d), (rng.uniform(-1, 1, (2000, d)).astype(np.float32), np.zeros((0, 2), np.int32))] +
                        graphs[30:] + [EMPTY(d)])
    cm = runtime.CompiledModel.from_model(make_model("gin", in_dim=4, hidden=8, layers=1, out_dim=8, task_out=2, mlp_layers=1),
                                          batch.num_graphs, batch.num_nodes, 1)
    _, coo, nptr, eptr = to_dev(batch, dev_())
    cm.graph_prep(coo, nptr, eptr, batch.num_nodes)
    import itertools
    orders = [p for r in (1, 2, 3) for p in itertools.permutations(("add", "mean", "max"), r)]
    for i, pools in enumerate(orders):
        x = batch.x - 1.5 if i % 2 else batch.x  # (uniform(-2.5, -0.5): every max negative)
        ref = R.pool64(x, batch, pools)
        base = np.concatenate([_pool32(x, batch, p) for p in pools], 1)
        xd = on_device(x, offset=i % 3 == 0)
        got = cm.global_pool(xd, list(pools)).cpu().numpy()
        record("global_pool", got, ref, base)
    cm.close()


def _pool32(x, batch, p):
    """fp32 pooling, rows summed in order."""
    out = np.zeros((batch.num_graphs, x.shape[1]), np.float32)
    for g in range(batch.num_graphs):
        rows = x[batch.node_ptr[g]:batch.node_ptr[g + 1]]
        if len(rows):
            s = np.cumsum(rows, 0, dtype=np.float32)[-1]  # (sequential: np.add.reduce would sum pairwise)
            out[g] = {"add": s, "max": rows.max(0), "mean": s / np.float32(len(rows))}[p]
    return out


# --------------------------------------------------------------------------- gnnb_aggregate_edges
@pytest.mark.parametrize("width", [1, 3, 64, 130])
@pytest.mark.parametrize("eps", [0.0, -0.3])
def test_aggregate_edges(width, eps, agg_batch, workspaces):
    b = agg_batch
    rng = np.random.default_rng(width)
    x = rng.uniform(-1, 1, (b.num_nodes, width)).astype(np.float32)
    et = rng.uniform(-1, 1, (b.num_edges, width)).astype(np.float32)
    ref, base = R.gine_agg64(x, b.coo, et, eps), R.gine_agg64(x, b.coo, et, eps, dtype=np.float32)
    cm = workspaces[(False, 0)]
    for off in (False, True):
        out = on_device(np.full_like(x, np.nan), off)
        cm.aggregate_edges(on_device(x, off), on_device(et, off), eps=eps, out=out)
        record("aggregate_edges", out.cpu().numpy(), ref, base)


# --------------------------------------------------------------------------- gnnb_pna_product_aggregate
@pytest.mark.parametrize("width", [32, 64, 128])
@pytest.mark.parametrize("ldw", ["2w", "2w+1"])
def test_pna_product_aggregate(width, ldw):
    """``wb`` = the strided ``W_pre[:, w:]`` view (ldw = 2w), and one whose row stride is not a multiple of 4: the kernel
    takes 16-byte aligned operands only, so that one must be refused (GNNB_ERR_INVALID), never read wrong."""
    from helpers import EMPTY, ONE
    from gnnbuilder_amd import synthetic
    from gnnbuilder_amd.batching import pack_graphs
    b0 = synthetic.make_batch("qm9", 200, seed=width)
    graphs = [b0.graph(g) for g in range(b0.num_graphs)] + [EMPTY(width), ONE(width)]
    # x on a 1/4 grid and W_b on a 1/64 grid: every p_j = W_b x_j is exact in fp32 and float64 alike, a non-zero variance of a
    # node's messages is >= 1.5e-5, and the std threshold (1e-5) lies between the two sides
    rng = np.random.default_rng(width)
    b = pack_graphs([(np.round(rng.uniform(-1, 1, (gx.shape[0], width)) * 4).astype(np.float32) / 4, c) for gx, c in graphs])
    promise = int(np.diff(b.node_ptr).max())
    cm = runtime.CompiledModel.from_model(make_model("pna", in_dim=width, hidden=width, layers=1, out_dim=width, task_out=2, mlp_layers=1),
                                          b.num_graphs, b.num_nodes, b.num_edges, max_graph_nodes=promise)
    _, coo, nptr, eptr = to_dev(b, dev_())
    cm.graph_prep(coo, nptr, eptr, b.num_nodes)
    rng = np.random.default_rng(width)
    ld = 2 * width + (ldw == "2w+1")
    wpre = (np.round(rng.uniform(-1, 1, (width, ld)) * 16) / 64).astype(np.float32)
    wb_h = wpre[:, width:2 * width]
    wb = torch.from_numpy(wpre).to(dev_())[:, width:2 * width]
    assert wb.stride(0) == ld
    p64 = b.x.astype(np.float64) @ wb_h.T.astype(np.float64)
    ref = R.pna_agg64(p64, b.coo)
    base = R.pna_agg64((torch.from_numpy(b.x) @ torch.from_numpy(wb_h).T).numpy(), b.coo, dtype=np.float32)
    if ld % 4:
        with pytest.raises(runtime.GnnbError, match=r"error -1: .*ldw that is a multiple of 4"):  # GNNB_ERR_INVALID
            cm.pna_product_aggregate(on_device(b.x), wb)
    else:
        got = cm.pna_product_aggregate(on_device(b.x), wb).cpu().numpy()
        cm.check()
        record("pna_product_aggregate", got, ref, base)
    cm.close()


# --------------------------------------------------------------------------- whole models at the edges
# (conv, hidden, in_dim, out_dim, layers, mlp_hidden): hidden 512 / 1024, in_dim 33 / 100 / 300, out_dim 30 / 130 -- every
# head here is beyond the fused readout (> 158 KB of weights, or a pooled width that is not a multiple of 4): the GEMM chain
WIDE = (("gcn", 512, 33, None, 3, 256), ("gcn", 1024, 300, 130, 2, 64), ("gin", 512, 300, 30, 2, 128), ("gin", 1024, 100, None, 2, 64),
        ("sage", 512, 100, 130, 2, 512), ("sage", 1024, 33, None, 2, 64), ("pna", 512, 33, 30, 2, 64), ("pna", 1024, 100, None, 2, 32))


def _wide_batch(fin, seed, graphs=80, hub=True):
    from helpers import EMPTY, ONE, hub_graph
    from gnnbuilder_amd import synthetic
    from gnnbuilder_amd.batching import pack_graphs
    b = synthetic.make_batch("qm9", graphs, seed=seed)
    rng = np.random.default_rng(seed)
    graphs = [(rng.uniform(-1, 1, (b.graph(g)[0].shape[0], fin)).astype(np.float32), b.graph(g)[1]) for g in range(b.num_graphs)]
    return pack_graphs(graphs + ([hub_graph(300, fin, 1200, seed)] if hub else []) + [EMPTY(fin), ONE(fin)])


def _forward(model, batch, promise=0, **opts):
    with options(**opts):
        cm = runtime.CompiledModel.from_model(model, batch.num_graphs, batch.num_nodes, batch.num_edges, max_graph_nodes=promise)
        got = cm.forward(*to_dev(batch, dev_())).cpu().numpy()
        cm.check()
        path = cm.last_path()
        cm.close()
    return got, path


@pytest.mark.parametrize("conv,hidden,fin,out_dim,layers,mlp_hidden", WIDE, ids=lambda v: str(v))
def test_wide_and_odd_models(conv, hidden, fin, out_dim, layers, mlp_hidden):
    """Layer by layer (no promise), odd-width aggregates and GEMMs, the readout's GEMM chain; ``fuse_head = 0`` forces the
    same chain through the option and must agree within the budget.  Base: the fp32 oracle, as in test_hip_fp64 (the model in
    fp32 torch is no fair base here: its BLAS sums K = 13 * 1024 in blocks, more accurately than any K-ordered sum)."""
    model = make_model(conv, in_dim=fin, hidden=hidden, layers=layers, out_dim=out_dim, act="tanh", mlp_hidden=mlp_hidden,
                       mlp_layers=3, task_out=7, mlp_act="gelu", seed=hidden + fin)
    # (the oracle's scalar loops set the batch size: PNA at 1024 -- 13F-wide post-NN products -- on 10 graphs and no hub)
    batch = _wide_batch(fin, hidden + fin, *((10, False) if (conv, hidden) == ("pna", 1024) else (30, True)))
    ref = R.forward64(model, batch, batch.x)
    from oracle import oracle as O
    from helpers import canon
    base = O.forward_batched(model.spec(), canon(model), batch.x, batch.coo, batch.node_ptr, batch.edge_ptr)
    got, path = _forward(model, batch)
    assert path == "layerwise"
    record(f"wide {conv}", got, ref, base)
    got0, path0 = _forward(model, batch, fuse_head=0)
    assert path0 == "layerwise"
    record(f"wide {conv}", got0, ref, base)


@pytest.mark.parametrize("out_dim,want", [(32, "stack_zf"), (30, "layerwise")])
def test_stack_promise_with_odd_out_dim_falls_back(out_dim, want):
    """A 2-layer GCN with a promise that fits the stack kernels' stages (molecules only: no hub graph): out_dim 32 takes
    ``stack_zf`` (the control), out_dim 30 -- which the stack kernels refuse (h1 & 3) -- must run layer by layer."""
    from oracle import oracle as O
    from helpers import canon
    model = make_model("gcn", in_dim=11, hidden=128, layers=2, out_dim=out_dim, act="relu", task_out=5, seed=3)
    batch = _wide_batch(11, 3, hub=False)
    promise = int(np.diff(batch.node_ptr).max())
    assert promise <= 29
    got, path = _forward(model, batch, promise=promise)
    assert path == want
    base = O.forward_batched(model.spec(), canon(model), batch.x, batch.coo, batch.node_ptr, batch.edge_ptr)
    record(f"stack promise out_dim {out_dim}", got, R.forward64(model, batch, batch.x), base)


def test_linear_empty_operands_without_address():
    """M = 0 with operands that have no address (torch gives an empty tensor none; the header allows NULL): GNNB_OK, an empty
    result -- both through the C entry with NULL pointers and through ``runtime.linear`` on empty torch tensors."""
    import ctypes as C
    lib = runtime.load_library(require_gpu=True)
    w = on_device(np.ones((5, 7)))
    segs = (runtime.GemmSeg * 2)()
    for i, (k, rs) in enumerate(((3, None), (4, None))):
        segs[i].a_dev, segs[i].rowscale_dev, segs[i].lda, segs[i].k = None, rs, k, k
    assert lib.gnnb_linear(segs, 2, C.c_void_p(w.data_ptr()), 7, None, None, None, 0, 5, runtime.ACT["tanh"],
                           C.c_void_p(runtime._stream_ptr())) == runtime.GNNB_OK
    a = torch.empty((0, 7), dtype=torch.float32, device=dev_())
    rs, skip = torch.empty((0,), dtype=torch.float32, device=dev_()), torch.empty((0, 5), dtype=torch.float32, device=dev_())
    out = runtime.linear([(a, rs)], w, on_device(np.ones(5)), skip=skip, act="relu")
    torch.cuda.synchronize()
    assert tuple(out.shape) == (0, 5)
