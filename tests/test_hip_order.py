"""PyG mini-batches ordered on the device so that the graphs beyond the ``max_graph_nodes`` promise come last
(csrc/k_order.hip; ``CompiledModel.ingest_pyg_ordered`` / ``forward_pyg_ordered``).

The reference of the arrays is always ``batching.order_large_last(batching.from_pyg_batch(...), limit)`` on the CPU: exact
integer equality of ``coo``, ``node_ptr``, ``edge_ptr``, ``perm`` and the triple, ``x_ord`` bit for bit -- no tolerance.  The
reference of the forward is the host route ON THE SAME WORKSPACE (``set_large_segment`` + ``forward`` on the host-ordered batch,
rows put back): the same kernels on the same arrays, so ``torch.equal``; in the caller's order it also meets the float64 budget
of tests/test_hip_fp64.py (``ref64.budget`` with its own K and F against the fp32 oracle's error)."""
import re

import numpy as np
import pytest
import torch

import ref64 as R
from gnnbuilder_amd import runtime, synthetic
from gnnbuilder_amd.batching import from_pyg_batch, order_large_last
from helpers import batch_vector, canon, make_model
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    runtime.load_library(require_gpu=True)  # fails loudly: no fallback
    return torch.device("cuda:0")


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _pyg(b, shuffle_seed=None):
    """(edge_index [2, E] int64, batch [N] int64) of a GraphBatch, the edges under a seeded permutation if asked."""
    ei = np.ascontiguousarray(b.coo.T.astype(np.int64)).reshape(2, -1)
    if shuffle_seed is not None:
        ei = np.ascontiguousarray(ei[:, np.random.default_rng(shuffle_seed).permutation(ei.shape[1])])
    return ei, batch_vector(b)


def _gin(in_dim):
    return make_model("gin", in_dim=in_dim, hidden=8, layers=1, out_dim=8, task_out=3, mlp_layers=0)


_MODELS = {}


def _arrays_model(in_dim, caps=(512, 16384, 32768)):
    """One-layer GIN workspaces for the array tests, one per input width (the promise is set per case)."""
    key = (in_dim, caps)
    if key not in _MODELS:
        m = runtime.CompiledModel.from_model(_gin(in_dim), *caps)
        m.enable_ordered_ingest()
        _MODELS[key] = m
    return _MODELS[key]


def _host(x, ei, limit, batch=None, ptr=None, B=None):
    r = from_pyg_batch(x, ei, batch=batch, ptr=ptr, num_graphs=B)
    o, perm, seg = order_large_last(r, limit)
    return r, o, perm, seg


def _device_arrays(m, dev, x, ei, batch=None, ptr=None, B=None, x_dev=None):
    got = m.ingest_pyg_ordered(_t(x, dev) if x_dev is None else x_dev, _t(ei, dev), batch=_t(batch, dev), ptr=_t(ptr, dev), num_graphs=B)
    x_ord, coo, nptr, eptr, perm, seg = got
    assert x_ord.dtype == torch.float32 and all(t.dtype == torch.int32 for t in (coo, nptr, eptr, perm))
    assert all(t.is_cuda for t in got[:5]) and all(isinstance(v, int) for v in seg)
    return tuple(t.cpu().numpy() for t in got[:5]) + (seg,)


def _same_arrays(got, o, perm, seg):
    x_ord, coo, nptr, eptr, gperm, gseg = got
    assert gseg == tuple(int(v) for v in seg), (gseg, seg)
    for g, r, what in ((coo, o.coo, "coo"), (nptr, o.node_ptr, "node_ptr"), (eptr, o.edge_ptr, "edge_ptr"), (gperm, perm, "perm")):
        assert g.shape == r.shape, (what, g.shape, r.shape)
        assert np.array_equal(g.astype(np.int64), r.astype(np.int64)), what
    assert x_ord.shape == o.x.shape and x_ord.dtype == np.float32
    assert np.array_equal(x_ord.view(np.uint32), np.ascontiguousarray(o.x).view(np.uint32)), "x_ord"


def _check_arrays(m, dev, x, ei, limit, batch=None, ptr=None, B=None, x_dev=None):
    m.set_max_graph_nodes(limit)
    got = _device_arrays(m, dev, x, ei, batch=batch, ptr=ptr, B=B, x_dev=x_dev)
    m.check()
    r, o, perm, seg = _host(x, ei, limit, batch=batch, ptr=ptr, B=B)
    _same_arrays(got, o, perm, seg)
    return r, perm, seg


# ---------------------------------------------------------------------------------------------------- 1. arrays against the host
CASES = {  # name: (shape, graphs, seed, limit, large graphs, triple or None)
    "qm9 some": ("qm9", 12, 5, 20, 3, None),
    "molhiv 24": ("molhiv_tail", 300, 11, 40, 24, (276, 6445, 14008)),
    "molhiv 1": ("molhiv_tail", 300, 11, 57, 1, None),
    "molhiv none": ("molhiv_tail", 300, 11, 1000, 0, None),
    "qm9 all": ("qm9", 12, 5, 5, 12, None),
}


@pytest.mark.parametrize("form", ["batch", "ptr"])
@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_arrays_equal_the_host_order(dev, case, shuffled, form):
    shape, graphs, seed, limit, n_large, triple = CASES[case]
    b = synthetic.make_batch(shape, graphs, seed=seed)
    ei, batch = _pyg(b, 7 if shuffled else None)
    m = _arrays_model(b.x.shape[1])
    if form == "batch":
        r, perm, seg = _check_arrays(m, dev, b.x, ei, limit, batch=batch, B=graphs)
    else:
        r, perm, seg = _check_arrays(m, dev, b.x, ei, limit, ptr=b.node_ptr.astype(np.int64))
    assert graphs - seg[0] == n_large == int((np.diff(b.node_ptr) > limit).sum())
    if triple is not None:
        assert seg == triple
    if n_large == 0:
        assert np.array_equal(perm, np.arange(graphs)) and seg == (graphs, r.num_nodes, r.num_edges)
    if n_large == graphs:
        assert seg == (0, 0, 0)


# ---------------------------------------------------------------------------------------------------- 2. graph counts
COUNTS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]


def _chains(B):
    """B graphs of 0 .. 5 nodes (empty ones included); a chain, both directions, on every graph of >= 2 nodes whose index is
    no multiple of 3; edges shuffled; features of width 3."""
    rng = np.random.default_rng(B)
    sizes = rng.integers(0, 6, B)
    nptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    src, dst = [], []
    for g in range(B):
        if sizes[g] >= 2 and g % 3 != 0:
            a = nptr[g] + np.arange(sizes[g] - 1)
            src += [a, a + 1]
            dst += [a + 1, a]
    ei = np.stack([np.concatenate(src), np.concatenate(dst)]).astype(np.int64) if src else np.zeros((2, 0), np.int64)
    ei = np.ascontiguousarray(ei[:, rng.permutation(ei.shape[1])])
    x = rng.uniform(-1, 1, (int(nptr[-1]), 3)).astype(np.float32)
    return x, ei, nptr, np.repeat(np.arange(B), sizes).astype(np.int64)


@pytest.mark.parametrize("B", COUNTS)
def test_graph_counts_around_wave_workgroup_and_scan_chunk(dev, B):
    """64 lanes, 16 waves = 1024 graphs per chunk of the carried scan: B = 1025 and 2049 carry into a second / third chunk."""
    x, ei, nptr, batch = _chains(B)
    m = _arrays_model(3, (max(COUNTS), 5 * max(COUNTS), 8 * max(COUNTS)))
    _, _, seg = _check_arrays(m, dev, x, ei, 3, batch=batch, B=B)
    n_large = B - seg[0]
    assert n_large == int((np.diff(nptr) > 3).sum())
    assert n_large == 0 if B == 1 else 16 <= n_large <= 710  # (what the host reference gives over these B)
    _check_arrays(m, dev, x, ei, 3, ptr=nptr)


# ---------------------------------------------------------------------------------------------------- 3. row widths
@pytest.mark.parametrize("in_dim,unaligned", [(1, False), (3, False), (4, False), (4, True), (11, False), (130, False)])
def test_row_widths_of_the_gather(dev, in_dim, unaligned):
    """Width 1, odd, a multiple of 4 (the 16-byte path), 4 from a pointer that is only 4-byte aligned (the scalar path at the
    same width), 11, and 130 = 2 mod 4 beyond one wave's 64 lanes."""
    b = synthetic.make_batch("qm9", 12, seed=5)
    ei, batch = _pyg(b, 3)
    x = np.random.default_rng(in_dim).uniform(-1, 1, (b.num_nodes, in_dim)).astype(np.float32)
    x_dev = None
    if unaligned:
        buf = torch.zeros(b.num_nodes * in_dim + 8, dtype=torch.float32, device=dev)
        x_dev = buf[1:1 + b.num_nodes * in_dim].view(b.num_nodes, in_dim)
        x_dev.copy_(torch.from_numpy(x))
        assert x_dev.data_ptr() % 16 == 4 and x_dev.is_contiguous()
    _check_arrays(_arrays_model(in_dim), dev, x, ei, 20, batch=batch, B=12, x_dev=x_dev)


# ---------------------------------------------------------------------------------------------------- 4. / 5. forward
_REFS = {}


def _references(key, model, r):
    """(float64 model output, fp32 oracle output) on the batch in the caller's order, computed once per (model, batch)."""
    if key not in _REFS:
        _REFS[key] = (R.forward64(model, r, r.x), O.forward_batched(model.spec(), canon(model), r.x, r.coo, r.node_ptr, r.edge_ptr))
    return _REFS[key]


def _host_route(m, dev, r, limit):
    """The same batch through the host: ordered there, uploaded, large segment set by hand, rows put back."""
    o, perm, seg = order_large_last(r, limit)
    if seg[0] == r.num_graphs:
        m.set_large_segment()
    else:
        m.set_large_segment(*seg)
    out = m.forward(_t(o.x, dev), _t(o.coo, dev), _t(o.node_ptr, dev), _t(o.edge_ptr, dev))
    return out[torch.from_numpy(np.argsort(perm)).to(dev)]


def _molhiv():
    b = synthetic.make_batch("molhiv_tail", 300, seed=11)
    ei, batch = _pyg(b, 7)
    return b, ei, batch


def _forward_case(dev, model, b, ei, batch, promise, key=None, paths=None):
    B = b.num_graphs
    m = runtime.CompiledModel.from_model(model, B, b.num_nodes, max(b.num_edges, 1), max_graph_nodes=promise)
    m.enable_ordered_ingest()
    got = m.forward_pyg_ordered(_t(b.x, dev), _t(ei, dev), batch=_t(batch, dev), num_graphs=B).clone()
    m.check()
    path = m.last_path()
    if paths is not None:
        assert path in paths, path
    r = from_pyg_batch(b.x, ei, batch=batch, num_graphs=B)
    want = _host_route(m, dev, r, promise)
    m.check()
    assert m.last_path() == path
    assert torch.equal(got, want)
    if key is not None:
        ref, base = _references(key, model, r)
        e, e32 = R.budget(got.cpu().numpy(), ref, base, what=key)
        print(f"{key}: e = {e:.3e}, e32 = {e32:.3e}")
    m.close()


@pytest.mark.parametrize("conv,layers,promise", [("gcn", 2, 40), ("gin", 3, 57)])
def test_forward_stack_route(dev, conv, layers, promise):
    model = make_model(conv, in_dim=9, hidden=128, layers=layers, act="relu", pools=("add", "max", "mean"), task_out=3, seed=5)
    b, ei, batch = _molhiv()
    _forward_case(dev, model, b, ei, batch, promise, key=f"ordered {conv}{layers}", paths=("stack+large_layerwise", "stack_zf+large_layerwise"))


def test_forward_sage(dev):
    model = make_model("sage", in_dim=9, hidden=16, layers=2, task_out=3, seed=5)
    b, ei, batch = _molhiv()
    _forward_case(dev, model, b, ei, batch, 40, key="ordered sage2")


def test_forward_all_large(dev):
    b = synthetic.make_batch("qm9", 12, seed=5)
    ei, batch = _pyg(b, 7)
    _forward_case(dev, make_model("gcn", in_dim=11, hidden=32, layers=2, task_out=5), b, ei, batch, 5)


def test_forward_without_a_promise_is_forward_pyg(dev):
    b = synthetic.make_batch("qm9", 12, seed=5)
    ei, batch = _pyg(b, 7)
    m = runtime.CompiledModel.from_model(make_model("gcn", in_dim=11, hidden=32, layers=2, task_out=5), 12, b.num_nodes, b.num_edges)
    m.enable_ordered_ingest()
    args = (_t(b.x, dev), _t(ei, dev))
    got = m.forward_pyg_ordered(*args, batch=_t(batch, dev), num_graphs=12).clone()
    path = m.last_path()
    want = m.forward_pyg(*args, batch=_t(batch, dev), num_graphs=12)
    m.check()
    assert torch.equal(got, want) and m.last_path() == path != "none"


# ---------------------------------------------------------------------------------------------------- 6. state between batches
def test_state_between_batches_on_one_workspace(dev):
    """Large graphs, none, large graphs again: the large segment follows each batch, and is gone after the one without."""
    promise = 40
    model = make_model("gcn", in_dim=9, hidden=32, layers=2, task_out=3, seed=2)
    a = synthetic.make_batch("molhiv_tail", 300, seed=11)
    c = synthetic.make_batch("molhiv_tail", 200, seed=12)
    oa, _, (g0, _, _) = order_large_last(a, promise)
    none = oa.slice(0, g0)  # a's small graphs: nothing large
    assert 0 < g0 < 300 and int((np.diff(c.node_ptr) > promise).sum()) > 0 and int(np.diff(none.node_ptr).max()) <= promise
    m = runtime.CompiledModel.from_model(model, 300, a.num_nodes, a.num_edges, max_graph_nodes=promise)
    m.enable_ordered_ingest()
    dv = {}
    for name, b in (("a", a), ("none", none), ("c", c)):
        ei, batch = _pyg(b, 5)
        dv[name] = (b, ei, batch, (_t(b.x, dev), _t(ei, dev)), _t(batch, dev))

    def ordered(name, **kw):
        b, _, _, args, batch = dv[name]
        return m.forward_pyg_ordered(*args, batch=batch, num_graphs=b.num_graphs, **kw)

    b, _, _, args, batch = dv["none"]
    before = m.forward_pyg(*args, batch=batch, num_graphs=b.num_graphs).clone()
    got = {"a": ordered("a").clone(), "none": ordered("none").clone()}
    plain = m.forward_pyg(*args, batch=batch, num_graphs=b.num_graphs).clone()  # (the segment of "a" is gone)
    side = torch.cuda.Stream()
    out = torch.empty((c.num_graphs, m.out_dim), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert ordered("c", out=out, stream=side) is out
    side.synchronize()
    got["c"] = out.clone()
    m.check()
    assert torch.equal(plain, before) and torch.equal(got["none"], before)
    for name in ("a", "none", "c"):
        b, ei, batch = dv[name][:3]
        want = _host_route(m, dev, from_pyg_batch(b.x, ei, batch=batch, num_graphs=b.num_graphs), promise)
        assert torch.equal(got[name], want), name
    m.check()


# ---------------------------------------------------------------------------------------------------- 7. a flagged batch
def test_flagged_batch_stays_contained(dev):
    """The malformed input of tests/test_hip_ingest.py: an endpoint = N.  The ordered ingest returns, every array it returns is
    in range and monotone, check() raises flag 0x80; a good batch runs clean afterwards."""
    b = synthetic.make_batch("qm9", 12, seed=9)
    ei, batch = _pyg(b)
    N, E, B = b.num_nodes, b.num_edges, 12
    bad = ei.copy()
    bad[1, int(b.edge_ptr[4]) + 1] = N
    m = _arrays_model(11)
    m.set_max_graph_nodes(20)
    assert int((np.diff(b.node_ptr) > 20).sum()) > 0
    x_ord, coo, nptr, eptr, perm, seg = _device_arrays(m, dev, b.x, bad, batch=batch, B=B)
    with pytest.raises(runtime.GnnbError) as err:
        m.check()
    flags = re.search(r"flags 0x([0-9a-f]+)", str(err.value))
    assert flags and int(flags.group(1), 16) & 0x80, str(err.value)
    assert x_ord.shape == (N, 11) and coo.shape == (E, 2) and nptr.shape == eptr.shape == (B + 1,) and perm.shape == (B,)
    assert nptr[0] == 0 and nptr[-1] == N and np.all(np.diff(nptr) >= 0)
    assert eptr[0] == 0 and eptr[-1] == E and np.all(np.diff(eptr) >= 0)
    assert coo.min() >= 0 and coo.max() < N
    assert np.array_equal(np.sort(perm), np.arange(B))
    assert 0 <= seg[0] <= B and seg[1] == nptr[seg[0]] and seg[2] == eptr[seg[0]]
    _check_arrays(m, dev, b.x, ei, 20, batch=batch, B=B)  # a well-formed batch on the same workspace is not blamed for it


def test_flagged_batch_is_reported_by_the_next_forward(dev):
    """tests/test_hip_ingest.py's test of this name for ``forward_pyg_ordered``: what the ingest kernels of a call flag is
    reported by the NEXT call on the workspace -- not by the call's own graph prep -- and once."""
    b = synthetic.make_batch("qm9", 12, seed=9)
    ei, batch = _pyg(b)
    N = b.num_nodes
    bad = ei.copy()
    bad[1, int(b.edge_ptr[4]) + 1] = N
    model = make_model("gcn", in_dim=4, hidden=16, layers=2, out_dim=16, task_out=3, mlp_layers=0)
    m = runtime.CompiledModel.from_model(model, 16, 512, 1024)
    m.enable_ordered_ingest()
    x, batch_dev = torch.zeros((N, 4), device=dev), _t(batch, dev)
    m.forward_pyg_ordered(x, _t(bad, dev), batch=batch_dev, num_graphs=12)  # flagged on the device; no check()
    torch.cuda.synchronize()
    with pytest.raises(runtime.GnnbError, match="earlier batch"):
        m.forward_pyg_ordered(x, _t(ei, dev), batch=batch_dev, num_graphs=12)
    m.forward_pyg_ordered(x, _t(ei, dev), batch=batch_dev, num_graphs=12)  # reported once
    m.check()


# ---------------------------------------------------------------------------------------------------- 8. API errors, no device work
def test_api_errors(dev):
    b = synthetic.make_batch("qm9", 12, seed=9)
    ei, batch = _pyg(b)
    x, ei_dev, batch_dev = _t(b.x, dev), _t(ei, dev), _t(batch, dev)
    plain = runtime.CompiledModel.from_model(_gin(11), 16, 512, 1024)
    plain.enable_ingest()  # (the plain ingest alone does not enable the ordered form)
    for call in (plain.ingest_pyg_ordered, plain.forward_pyg_ordered):
        with pytest.raises(runtime.GnnbError, match="enable_ordered_ingest"):
            call(x, ei_dev, batch=batch_dev, num_graphs=12)
    m = _arrays_model(11)
    for call in (m.ingest_pyg_ordered, m.forward_pyg_ordered):
        with pytest.raises(runtime.GnnbError, match="float32"):
            call(x.double(), ei_dev, batch=batch_dev, num_graphs=12)
        with pytest.raises(runtime.GnnbError, match="last dimension 11"):
            call(x[:, :9].contiguous(), ei_dev, batch=batch_dev, num_graphs=12)
        with pytest.raises(runtime.GnnbError, match="contiguous"):
            call(x.t().contiguous().t(), ei_dev, batch=batch_dev, num_graphs=12)
        with pytest.raises(runtime.GnnbError, match="int64"):
            call(x, ei_dev.to(torch.int32), batch=batch_dev, num_graphs=12)
        with pytest.raises(runtime.GnnbError, match=r"\[2, E\].*contiguous\(\)"):
            call(x, ei_dev.t().contiguous(), batch=batch_dev, num_graphs=12)
        with pytest.raises(runtime.GnnbError, match="num_graphs is required"):
            call(x, ei_dev, batch=batch_dev)
        with pytest.raises(runtime.GnnbError, match="one per node"):
            call(x[:-1], ei_dev, batch=batch_dev, num_graphs=12)
    small = runtime.CompiledModel.from_model(_gin(11), 4, 512, 1024)
    small.enable_ordered_ingest()  # (enables the plain ingest as well)
    small.enable_ordered_ingest()  # (a second call is a no-op)
    with pytest.raises(runtime.GnnbError, match="error -2.*exceeds workspace"):
        small.ingest_pyg_ordered(x, ei_dev, batch=batch_dev, num_graphs=12)
    with pytest.raises(runtime.GnnbError, match="error -2.*exceeds workspace"):
        small.forward_pyg_ordered(x, ei_dev, batch=batch_dev, num_graphs=12)
    # in use: a batch has been prepared on the workspace
    plain.forward(x, _t(b.coo, dev), _t(b.node_ptr, dev), _t(b.edge_ptr, dev))
    with pytest.raises(runtime.GnnbError, match="in use"):
        plain.enable_ordered_ingest()
    plain.check()
