"""k_gcn2_zf's aggregate-and-pool phase (P1) and the next stage's narrow aggregate (P0') against float64, batch shapes chosen
for what those two phases do with a stage: the row walk's full passes and its tail pass, tasks that wrap on a wave, stages
around the number of idle waves at which P0' is dealt over the idle waves only, rows of degree > 4 (from the stage's LDS slice
of `col` and from global memory), empty graphs, and a batch of one stage (no P0' at all).

A workgroup walks an equal share of the batch's node tiles and the grid is one workgroup per resident slot (256 on the wide
shape), so a stage only fills -- and a workgroup only has a second stage, i.e. a P0' -- when the batch holds a few hundred rows
per workgroup: the batches repeat their pattern 256 times.  Every case runs the whole model through the C ABI in both shapes
(``zf_shape`` 2 = 16 waves and 176-row stages, 0 = 8 waves and 96-row stages), twice (same bits), and holds the output to
``ref64.budget`` with the project's own K and F.  The references are computed once per (model, batch) and shared by the two
shapes and by the CPU test, which holds the fp32 oracle itself to the float64 model on the same batches: a failure on the GPU
then points at the kernel."""
import functools

import numpy as np
import pytest
import torch

import ref64 as R
from gnnbuilder_amd import runtime
from gnnbuilder_amd.batching import pack_graphs
from helpers import EMPTY, ONE, canon, hub_graph, make_model, to_dev
from oracle import oracle as O

REPS = 256  # workgroups of the wide shape's grid on one MI355X: every workgroup gets the pattern once
PROMISE = 29

# (f0, h0, h1, activation, pools): the C2 instantiation; a narrower last layer (the lane geometry is not a literal, a row takes
# fewer lanes); a narrow first layer under a full-width last one
MODELS = {
    "c2": dict(in_dim=11, hidden=128, out_dim=128, act="relu", pools=("add", "mean", "max")),
    "h64x32": dict(in_dim=9, hidden=64, out_dim=32, act="tanh", pools=("max",)),
    "h32x128": dict(in_dim=16, hidden=32, out_dim=128, act="sigmoid", pools=("add", "mean", "max")),
}


def mol(n, fin, rng):
    """``n`` nodes on an undirected path plus n // 3 undirected chords: degrees mostly <= 4, as QM9's."""
    x = rng.uniform(-1, 1, (n, fin)).astype(np.float32)
    if n < 2:
        return x, np.zeros((0, 2), np.int32)
    e = [np.stack([np.arange(n - 1), np.arange(1, n)], 1)]
    if n >= 4:
        a = rng.integers(0, n, n // 3)
        e.append(np.stack([a, (a + 2 + rng.integers(0, n - 3, n // 3)) % n], 1))
    e = np.concatenate(e)
    return x, np.concatenate([e, e[:, ::-1]]).astype(np.int32)


def sized(sizes, fin, seed, reps=REPS):
    rng = np.random.default_rng(seed)
    return [mol(int(n), fin, rng) for _ in range(reps) for n in sizes]


def _tail_edges(fin):
    # tail pass only (1, 2, 3 nodes at two rows per pass and at four), no tail (4), one full pass plus a tail (5), the longest walk
    return sized((1, 2, 3, 4, 5, 28, 29) * 4, fin, 1)


def _tasks_wrap(fin):
    # 40 small graphs fill a stage: more tasks than waves, no idle wave, P0' dealt over all waves; then a stage of ten tasks
    rng = np.random.default_rng(2)
    return sized(tuple(rng.integers(3, 5, 40)) + tuple(rng.integers(17, 20, 10)), fin, 2)


def _idle_13(fin):
    return sized((13,) * 26, fin, 3)  # 13 tasks per 176-row stage: three idle waves, one short of the condition


def _idle_16(fin):
    return sized((11,) * 32, fin, 4)  # 16 tasks per 176-row stage: no idle wave


def _idle_most(fin):
    return sized((29,) * 12, fin, 5)  # six tasks per stage, ten idle waves take all of P0'


def _hubs(fin):
    # degree > 4 inside the row walk: a hub as the first graph, directly behind a one-node graph, as the last graph;
    # and one whose stage holds more edges than the stage's LDS slice of `col` (1024 wide / 512 narrow; hub_graph gives any
    # number of edges at 29 nodes, as duplicates), so that the rest of the row comes from global memory
    g = sized((5, 17, 9, 29, 12, 2) * 5, fin, 6)
    k = len(g) // 2
    return ([hub_graph(29, fin, 300, 61)] + g[:k] + [ONE(fin), hub_graph(23, fin, 200, 62)] + g[k:k + 700] +
            [hub_graph(29, fin, 1100, 63)] + g[k + 700:] + [hub_graph(29, fin, 300, 64)])


def _empties(fin):
    g = sized((7, 18, 3, 29, 11, 1, 22) * 3, fin, 7)
    k = len(g) // 2
    return ([EMPTY(fin)] * 3 + g[:k] + [EMPTY(fin)] * 2 + g[k:k + 1] + [EMPTY(fin)] + g[k + 1:k + 9] + [EMPTY(fin)] + g[k + 9:] +
            [EMPTY(fin)] * 5)


def _single_17(fin):
    return sized((17,), fin, 8, reps=1)  # one stage, no next stage: no P0'


BATCHES = {"tail_edges": _tail_edges, "tasks_wrap": _tasks_wrap, "idle_13": _idle_13, "idle_16": _idle_16, "idle_most": _idle_most,
           "hubs": _hubs, "empties": _empties, "single_17": _single_17}
CASES = [(m, b) for m in MODELS for b in BATCHES]


@functools.lru_cache(maxsize=None)
def case(mname, bname):
    """(model, batch, float64 output, fp32 oracle output): computed once, never written to."""
    kw = MODELS[mname]
    model = make_model("gcn", layers=2, task_out=7, mlp_act=kw["act"], seed=len(mname) + len(bname), **kw)
    batch = pack_graphs(BATCHES[bname](kw["in_dim"]))
    assert int(np.diff(batch.node_ptr).max()) <= PROMISE
    ref = R.forward64(model, batch, batch.x)
    base = O.forward_batched(model.spec(), canon(model), batch.x, batch.coo, batch.node_ptr, batch.edge_ptr)
    for a in (ref, base):
        a.setflags(write=False)
    return model, batch, ref, base


@pytest.mark.parametrize("mname,bname", CASES)
def test_fp32_oracle_meets_float64_on_these_batches(mname, bname):
    """No GPU: the budget's base is itself an fp32-class evaluation of the float64 model here (the bound of test_ref64.py)."""
    _, _, ref, base = case(mname, bname)
    assert np.isfinite(ref).all() and ref.shape[0] == case(mname, bname)[1].num_graphs
    assert np.abs(base - ref).max() <= 4e-6 * np.abs(ref).max()


def forward_twice(model, batch, shape):
    dev = torch.device("cuda:0")
    try:
        runtime.set_option("zf_shape", shape)
        cm = runtime.CompiledModel.from_model(model, batch.num_graphs, batch.num_nodes, max(batch.num_edges, 1), max_graph_nodes=PROMISE)
        x, coo, nptr, eptr = to_dev(batch, dev)
        outs = []
        for _ in range(2):
            outs.append(cm.forward(x, coo, nptr, eptr).cpu().numpy().copy())
            cm.check()
            assert cm.last_path() == "stack_zf"
        cm.close()
    finally:
        runtime.set_option("zf_shape", 2)
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [2, 0], ids=["wide", "narrow"])
@pytest.mark.parametrize("mname,bname", CASES)
def test_zf_p1(mname, bname, shape):
    runtime.load_library(require_gpu=True)  # fails loudly: no fallback
    model, batch, ref, base = case(mname, bname)
    first, second = forward_twice(model, batch, shape)
    assert np.array_equal(first, second)
    R.budget(first, ref, base, what=f"stack_zf {mname} {bname} zf_shape {shape}")
