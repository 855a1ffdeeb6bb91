"""``ggnn_util.ggnn_ref`` -- the float64 restatement tests/test_hip_ggnn.py holds the kernel against -- and the inputs of that
file, checked on references alone: the helper batches hold the rows the long-row path needs, the dyadic grids make every sum of
``p_j`` and every r and z argument exact in fp32, the steep set saturates the reference, and the budget (``ref64.budget``, K = 4,
F = 2^-22, per in-degree class) REJECTS each of four wrong kernels restated in fp32 on the stage test's own inputs.  No GPU."""
import numpy as np
import pytest

from ggnn_util import FAULTS, arguments_are_exact, ggnn_ref, sigmoid, stage_case
from gine_util import budget_by_degree
from helpers import edge_batch, sweep_batch

BATCHES = {}


def _batch(kind):
    """The two batches of tests/test_hip_ggnn.py's stage test."""
    if kind not in BATCHES:
        BATCHES[kind] = edge_batch(8, 4, seed=21) if kind == "edge" else sweep_batch(24, 4, seed=5)[0]
    return BATCHES[kind]


def test_the_helper_batches_hold_rows_of_two_pieces_and_of_many():
    """The long-row path at two pieces (65 .. 128 in-edges) and at many, and rows without in-edges: the two batches hold all."""
    deg = [np.bincount(_batch(k).coo[:, 1], minlength=_batch(k).num_nodes) for k in ("edge", "sweep")]
    both = np.concatenate(deg)
    assert (both > 128).any() and ((both > 64) & (both <= 128)).any()
    assert all(d.max() >= 1200 and (d == 0).sum() >= 5 for d in deg)


@pytest.mark.parametrize("kind", ["edge", "sweep"])
@pytest.mark.parametrize("width,h_width", [(32, 32), (9, 7), (1, 1)])
def test_the_grids_are_exact_and_the_steep_set_saturates(kind, width, h_width):
    b = _batch(kind)
    for operands in ("flat", "steep"):
        c = stage_case(b.num_nodes, width, h_width, operands)
        r32, z32 = arguments_are_exact(c, b.coo)  # (asserts: sums of p_j and both gate arguments are exact in fp32)
        base = ggnn_ref(c["p"], c["gh"], c["h"], c["b_ih"], None, "none", b.coo, dtype=np.float32)
        assert base.dtype == np.float32 and np.isfinite(base).all()
        if operands == "steep":
            g = np.concatenate([sigmoid(r32), sigmoid(z32)])
            assert np.abs(r32).max() >= 200.0 and (g == 0.0).any() and (g == 1.0).any() and not np.isnan(g).any()
            assert (np.abs(base) == 1.0).any()  # a shut update gate leaves the tanh: exactly +-1


def test_the_reference_is_within_its_own_budget():
    """``base`` against ``ref`` passes trivially (e = e32): the rejections below are the faults', not the rule's."""
    b = _batch("edge")
    c = stage_case(b.num_nodes, 32, 12, "flat")
    args = (c["p"], c["gh"], c["h"], c["b_ih"], None, "none", b.coo)
    ref, base = ggnn_ref(*args), ggnn_ref(*args, dtype=np.float32)
    budget_by_degree(base, ref, base, b.coo, what="base")


@pytest.mark.parametrize("fault", FAULTS)
def test_the_budget_rejects_a_wrong_kernel(fault):
    """On the inputs of the stage test (edge batch, width 32, ``h_width`` 12, flat): a kernel with ``fault`` -- ``bias_ih`` added
    per edge, r and z swapped, ``h`` not zero-padded with its columns shifted, ``r`` applied to ``gi_n`` -- restated in fp32 is
    outside the budget."""
    b = _batch("edge")
    c = stage_case(b.num_nodes, 32, 12, "flat")
    args = (c["p"], c["gh"], c["h"], c["b_ih"], None, "none", b.coo)
    ref, base = ggnn_ref(*args), ggnn_ref(*args, dtype=np.float32)
    wrong = ggnn_ref(*args, dtype=np.float32, fault=fault)
    with pytest.raises(AssertionError, match="e ="):
        budget_by_degree(wrong, ref, base, b.coo, what=fault)
