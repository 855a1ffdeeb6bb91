"""NNConv on the CPU: the plain-torch ``_NNConv`` against the explicit-``Theta`` float64 reference, and the fold identity
``A W_fold == sum_j x_j Theta(e_ij)`` that the aggregate-first order rests on (include/gnnb_nnconv.h)."""
import numpy as np
import pytest
import torch

import nnconv_util as U
from gnnbuilder_amd.models import _NNConv
from helpers import edge_batch, looped_graph


def _case(fi, d, seed):
    x, coo = looped_graph(40, fi, seed)
    return x, coo, np.random.default_rng(seed).uniform(-1, 1, (len(coo), d)).astype(np.float32)


@pytest.mark.parametrize("hidden,aggr", [(0, "add"), (5, "mean")])
def test_the_torch_definition_equals_the_explicit_theta_reference(hidden, aggr):
    fi, fo, d = 7, 5, 3
    x, coo, e = _case(fi, d, seed=3)
    torch.manual_seed(1)
    conv = _NNConv(fi, fo, d, hidden, aggr).double()
    p = {k: v.detach().numpy() for k, v in conv.state_dict().items()}
    assert set(p) == {"bias", "lin.weight", "nn.0.weight", "nn.0.bias"} | ({"nn.2.weight", "nn.2.bias"} if hidden else set())
    last = "nn.2" if hidden else "nn.0"
    w1, b1 = (p["nn.0.weight"], p["nn.0.bias"]) if hidden else (None, None)
    ref = U.theta_sum(x, coo, e, p[last + ".weight"], p[last + ".bias"], fo, w1, b1)
    if aggr == "mean":
        ref /= np.maximum(np.bincount(coo[:, 1], minlength=len(x)), 1)[:, None]
    ref += x.astype(np.float64) @ p["lin.weight"].T + p["bias"]
    with torch.no_grad():
        got = conv(torch.from_numpy(x).double(), torch.from_numpy(coo.T.astype(np.int64)), torch.from_numpy(e).double()).numpy()
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("hidden,aggr", [(0, "add"), (5, "mean")])
def test_the_block_wise_aggregate_has_the_bits_of_the_definition(hidden, aggr, dtype):
    """``aggregate_ref_blocks`` (what the many-sweep GPU tests are held to) on a batch with a hub of 1200 in-edges, rows without
    in-edges, self loops and duplicate edges."""
    b = edge_batch(4, 7, seed=2)
    rng = np.random.default_rng(5)
    e = rng.uniform(-1, 1, (b.num_edges, 3)).astype(np.float32)
    w1, b1 = (rng.uniform(-1, 1, (hidden, 3)).astype(np.float32), rng.uniform(-0.3, 0.3, hidden).astype(np.float32)) if hidden else (None, None)
    want, got = U.aggregate_ref(b.x, b.coo, e, w1, b1, aggr, dtype), U.aggregate_ref_blocks(b.x, b.coo, e, w1, b1, aggr, dtype)
    assert got.dtype == want.dtype == dtype and got.shape == want.shape and np.array_equal(got, want)
    empty = np.zeros((0, 2), np.int32)
    assert not U.aggregate_ref_blocks(b.x[:3], empty, e[:0], w1, b1, aggr, dtype).any()


def test_the_forward_by_graphs_is_the_forward_in_one_piece():
    """``forward_by_graphs`` against ``forward64`` / ``run`` on a batch with an empty and a one-node graph at a chunk's end.  The two
    are the same definition on the same rows; torch's GEMMs choose their blocking by the row count, so a chunk may round another
    way.  Either run is a plain evaluation in its dtype, some ten ulps of the output's scale from the exact value (e32 of the
    whole-model GPU tests is 4 ... 11 ulps), so two of them lie within 32 ulps of each other: 2^-48 and 2^-19 of the scale."""
    b = edge_batch(6, 9, seed=3)
    ea = np.random.default_rng(4).uniform(-1, 1, (b.num_edges, 4)).astype(np.float32)
    model = U.make_model(9, 12, 2, 4, 5, "mean", seed=1)
    assert (np.diff(b.node_ptr)[[4, 6]] == [0, 1]).all()
    for graphs in (1, 5, 7, 64):
        got = U.forward_by_graphs(model, b, b.x, ea, graphs=graphs)
        want = U.forward64(model, b, b.x, ea)
        assert got.dtype == np.float64 and got.shape == want.shape and np.abs(got - want).max() <= 2.0 ** -48 * np.abs(want).max()
        got32, want32 = U.forward_by_graphs(model, b, b.x, ea, graphs=graphs, double=False), U.run(model, b, b.x, ea)
        assert got32.dtype == np.float32 and np.abs(got32 - want32).max() <= 2.0 ** -19 * np.abs(want32).max()


@pytest.mark.parametrize("hidden", [0, 4])
def test_the_fold_identity_holds_in_float64(hidden):
    fi, fo, d = 6, 5, 3
    x, coo, e = _case(fi, d, seed=4)
    rng = np.random.default_rng(9)
    kq = hidden or d
    w2, b2 = rng.uniform(-1, 1, (fi * fo, kq)), rng.uniform(-1, 1, fi * fo)
    w1, b1 = (rng.uniform(-1, 1, (hidden, d)), rng.uniform(-1, 1, hidden)) if hidden else (None, None)
    a = U.aggregate_ref(x, coo, e, w1, b1)
    ref = U.theta_sum(x, coo, e, w2, b2, fo, w1, b1)
    assert np.abs(a @ U.fold(w2, b2, fi, fo) - ref).max() <= 1e-12 * np.abs(ref).max()
