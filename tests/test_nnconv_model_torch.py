"""NNConv on the CPU: the plain-torch ``_NNConv`` against the explicit-``Theta`` float64 reference, and the fold identity
``A W_fold == sum_j x_j Theta(e_ij)`` that the aggregate-first order rests on (include/gnnb_nnconv.h)."""
import numpy as np
import pytest
import torch

import nnconv_util as U
from gnnbuilder_amd.models import _NNConv
from helpers import looped_graph


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
