"""The rungs of the forward's sequencing that no other test reaches, against float64 with the fp32-class budget of ref64.

gnnb_forward.hip decides which kernels a forward runs: per conv layer a ladder of forms (``gcn_layer`` ... ``pna_layer``), then
the readout ladder (``readout_layerwise``).  test_hip_fp64.py forces every kernel route; here every DECISION of the two ladders
that it leaves out is forced with the options that steer it -- ``head_split``, ``head_small``, ``fuse_pool``, ``fold_skip``, a
head of more than eight linears, a large segment the small per-layer kernel declines -- and the output must meet
``ref64.budget`` with the project's K and F.  Every case is 200 QM9-shaped graphs plus an empty and a
one-node graph; width 256 only where a rung needs it."""
import functools

import numpy as np
import pytest
import torch

from gnnbuilder_amd import runtime, synthetic
from gnnbuilder_amd.batching import order_large_last, pack_graphs
from helpers import EMPTY, ONE, hub_graph, make_model
from test_hip_fp64 import _library, check, dev_, hip, options, references, regraphed  # noqa: F401  (_library: module fixture)

pytestmark = pytest.mark.gpu

POOLS = ("add", "mean", "max")


@functools.lru_cache(maxsize=None)
def case(conv, hidden, layers=2, mlp_layers=2, fin=11):
    """(model, batch, (float64 reference, fp32 oracle output)): once per model, shared by the option settings run on it."""
    model = make_model(conv, in_dim=fin, hidden=hidden, layers=layers, pools=POOLS, mlp_hidden=64, mlp_layers=mlp_layers, task_out=5,
                       seed=hidden + layers)
    batch = regraphed(synthetic.make_batch("qm9", 200, seed=hidden + mlp_layers), fin, layers, [EMPTY(fin), ONE(fin)])
    return model, batch, references(model, batch, batch.x)


# --------------------------------------------------------------------------- the readout ladder behind a node matrix
@pytest.mark.parametrize("split,small", [(0, 1), (0, 0), (1, 1), (1, 0)])
@pytest.mark.parametrize("hidden", [256, 64])
def test_readout_rungs(hidden, split, small):
    """A GCN layer never pools in a GEMM epilogue, so the ladder starts from the node matrix.  hidden 256: the head's first
    matrix (768 x 64 floats) does not fit k_pool_mlp's LDS -- one-launch form declined, then k_head_small on the pooled matrix
    (``small``) or the GEMM chain; ``split`` pools first.  hidden 64: the head fits k_pool_mlp."""
    model, batch, refs = case("gcn", hidden)
    got, path = hip(model, batch, batch.x, fuse_gcn2=0, head_split=split, head_small=small)
    assert path == "layerwise"
    check("rungs readout", got, model, batch, batch.x, refs=refs)


@pytest.mark.parametrize("fuse_pool", [1, 0])
@pytest.mark.parametrize("small", [1, 0])
def test_epilogue_pooled_readout(fuse_pool, small):
    """GraphSAGE's last layer pools in its GEMM's epilogue (``fuse_pool``): the ladder starts from a complete pooled matrix."""
    model, batch, refs = case("sage", 256)
    got, path = hip(model, batch, batch.x, fuse_pool=fuse_pool, head_small=small)
    assert path == "layerwise"
    check("rungs epilogue_pool", got, model, batch, batch.x, refs=refs)


@pytest.mark.parametrize("conv,promise", [("gcn", 29), ("sage", 0)])
def test_head_of_nine_linears(conv, promise):
    """``mlp_layers = 8`` hidden layers are nine linears, one more than a HeadArgs holds: pooling pass + GEMM chain.  The GCN
    stack is gated on a head of <= 8 as well, so the promised GCN model runs layer by layer."""
    model, batch, refs = case(conv, 64, mlp_layers=8)
    assert model.spec()["mlp_hidden_layers"] + 1 == 9
    got, path = hip(model, batch, batch.x, promise=promise)
    assert path == "layerwise"
    check("rungs head9", got, model, batch, batch.x, refs=refs)


# --------------------------------------------------------------------------- the middle layer's skip connection
@pytest.mark.parametrize("fold", [1, 0])
@pytest.mark.parametrize("conv", ["sage", "pna"])
def test_fold_skip(conv, fold):
    """Three layers with skip: the middle one takes its skip as + I on x's own weights (``fold_skip``, GraphSAGE slot 2; PNA's
    derived slots always carry it) or as the GEMM's skip operand.  PNA under a degree promise: the degree-class GEMM."""
    model, batch, refs = case(conv, 128, layers=3)
    maxdeg = int(np.bincount(batch.coo[:, 1]).max()) if conv == "pna" else 0
    assert maxdeg <= 15
    got, path = hip(model, batch, batch.x, maxdeg=maxdeg, fold_skip=fold, pna_fold_lin=1)
    assert path == "layerwise"
    check("rungs fold_skip", got, model, batch, batch.x, refs=refs)


# --------------------------------------------------------------------------- large segment, general layer-by-layer form
def test_large_segment_general_form():
    """The large segment through ``run_conv_layers(row_lo > 0)`` + ``pool_large_segment`` with ``large_fork = 2``.

    The issue's model (gcn, 3 layers, hidden 256) is not taken by the stack kernel: k_gcn2_fused takes hidden 32 / 64 / 128
    only, and every width it takes suits k_conv_rows (<= 128) too.  What is left is ``large_segment_small``'s alignment
    condition: an ``in_dim`` that is a multiple of 4 with ``x`` not on a 16-byte boundary.  The stack kernel asks ``x`` for
    4-byte alignment only, so gcn, in_dim 8, hidden 128, 3 layers with ``x`` one float past a 16-byte boundary is the smallest
    model whose small segment the stack takes while k_conv_rows declines the large one."""
    fin = 8
    model = make_model("gcn", in_dim=fin, hidden=128, layers=3, act="relu", pools=POOLS, task_out=5, seed=57)
    b0 = regraphed(synthetic.make_batch("molhiv_tail", 200, seed=57), fin, 57)
    batch = pack_graphs([b0.graph(g) for g in range(100)] + [hub_graph(300, fin, 1200, 6), EMPTY(fin), ONE(fin)] +
                        [b0.graph(g) for g in range(100, 200)])
    ordered, _, (g0, n0, e0) = order_large_last(batch, 57)
    assert 0 < g0 < ordered.num_graphs
    buf = torch.zeros(ordered.x.size + 4, dtype=torch.float32, device=dev_())
    x = buf[1:1 + ordered.x.size].view(ordered.x.shape)
    x.copy_(torch.from_numpy(ordered.x))
    assert x.data_ptr() % 16 == 4
    with options(large_fork=2):
        cm = runtime.CompiledModel.from_model(model, ordered.num_graphs, ordered.num_nodes, ordered.num_edges,
                                              max_graph_nodes=int(np.diff(ordered.node_ptr)[:g0].max()))
        cm.set_large_segment(g0, n0, e0)
        got = cm.forward(x, *[torch.from_numpy(a).to(dev_()) for a in (ordered.coo, ordered.node_ptr, ordered.edge_ptr)]).cpu().numpy()
        cm.check()
        assert cm.last_path() == "stack+large_layerwise", cm.last_path()
        cm.close()
    check("rungs large_general", got, model, ordered, ordered.x)
