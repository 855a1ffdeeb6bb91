"""The rule ``tests/test_hip_gine_sweeps.py`` applies -- ``ref64.budget`` per in-degree class (``gine_util.budget_by_degree``) --
has power against what ``k_gine_aggregate`` could get wrong: on a smaller copy of that file's batch, each fault is injected
into the fp32 ``base`` of the stage entry (an honest result), shown to move the float64 value by more than 1e-3 of its
class's scale, and must be rejected; the unfaulted ``base`` passes.  CPU only."""
import numpy as np
import pytest

import ref64 as R
from gine_util import budget_by_degree, degree_classes, edge_attrs, stage_weights
from helpers import STAR_IN_DEGREES, sweep_batch
from test_hip_gine import _stage_refs

WIDTH, EDGE_DIM, EPS = 130, 5, 0.3  # scalar form, three column passes of 64 columns
PASS = 64


@pytest.fixture(scope="module")
def case():
    b, stars = sweep_batch(480, 9, seed=51)
    assert b.num_nodes > 4 * 2048 + 2
    x = np.random.default_rng(1).uniform(-1, 1, (b.num_nodes, WIDTH)).astype(np.float32)
    ea = edge_attrs(b.num_edges, EDGE_DIM, seed=2)
    we, be = stage_weights(WIDTH, EDGE_DIM, seed=3)
    ref, base = _stage_refs(x, b.coo, ea, we, be, EPS)
    deg = np.bincount(b.coo[:, 1], minlength=b.num_nodes)
    assert set(STAR_IN_DEGREES) <= set(deg.tolist())
    return dict(b=b, x=x, ea=ea, we=we, be=be, ref=ref, base=base, deg=deg, classes=degree_classes(b.coo, b.num_nodes))


def _slots(case, node):
    """The COO rows of ``node``'s in-edges in COO order: its CSR slots."""
    return np.flatnonzero(case["b"].coo[:, 1] == node)


def _rejected(case, got, ref_faulted, cls):
    """``got`` = ``base`` with a fault; ``ref_faulted`` = the float64 value of the same fault: it differs from the reference
    by more than 1e-3 of the class's scale (the fault is no rounding matter), and the class-wise budget raises."""
    m = case["classes"][cls]
    moved = np.abs(ref_faulted[m] - case["ref"][m]).max() / np.abs(case["ref"][m]).max()
    assert moved > 1e-3, moved
    with pytest.raises(AssertionError, match="e = "):
        R.budget(got[m], case["ref"][m], case["base"][m])
    with pytest.raises(AssertionError, match="e = "):
        budget_by_degree(got, case["ref"], case["base"], case["b"].coo, what="fault")


def _refaulted(case, coo=None, ea=None, be=None):
    """(float64, fp32) stage results on inputs with a fault."""
    return _stage_refs(case["x"], case["b"].coo if coo is None else coo, case["ea"] if ea is None else ea, case["we"],
                       case["be"] if be is None else be, EPS)


def test_unfaulted_base_passes(case):
    out = budget_by_degree(case["base"], case["ref"], case["base"], case["b"].coo)
    assert set(out) == {"deg<=4", "deg5-64", "deg>64", "all"}
    # the classes' scales are what makes the rule per class: a hub's sum is ~100 times a molecule's row
    s = {k: np.abs(case["ref"][m]).max() for k, m in case["classes"].items()}
    assert s["deg>64"] > 50 * s["deg<=4"] and s["deg5-64"] > 3 * s["deg<=4"]


def test_last_slot_of_a_65_row_dropped(case):
    node = int(np.flatnonzero(case["deg"] == 65)[0])
    keep = np.ones(case["b"].num_edges, bool)
    keep[_slots(case, node)[-1]] = False
    ref_f, got = _refaulted(case, coo=case["b"].coo[keep], ea=case["ea"][keep])
    assert np.array_equal(np.flatnonzero((got != case["base"]).any(1)), [node])
    _rejected(case, got, ref_f, "deg>64")


def test_messages_behind_the_preloaded_four_dropped(case):
    node = int(np.flatnonzero(case["deg"] == 5)[0])
    keep = np.ones(case["b"].num_edges, bool)
    keep[_slots(case, node)[4:]] = False
    ref_f, got = _refaulted(case, coo=case["b"].coo[keep], ea=case["ea"][keep])
    assert np.array_equal(np.flatnonzero((got != case["base"]).any(1)), [node])
    _rejected(case, got, ref_f, "deg5-64")


def test_two_adjacent_rows_of_a_later_sweep_exchanged(case):
    low = case["classes"]["deg<=4"]
    r = 4 * 2048 + int(np.flatnonzero(low[4 * 2048:-1] & low[4 * 2048 + 1:])[0])
    swap = np.arange(case["b"].num_nodes)
    swap[[r, r + 1]] = [r + 1, r]
    _rejected(case, case["base"][swap], case["ref"][swap], "deg<=4")


def test_bias_missing_in_the_second_column_pass(case):
    be = case["be"].copy()
    be[PASS:2 * PASS] = 0.0
    ref_f, got = _refaulted(case, be=be)
    assert not (got[:, :PASS] != case["base"][:, :PASS]).any() and not (got[:, 2 * PASS:] != case["base"][:, 2 * PASS:]).any()
    for cls in case["classes"]:
        _rejected(case, got, ref_f, cls)


def test_an_edge_with_the_attributes_of_an_edge_into_another_row(case):
    coo = case["b"].coo
    node = int(np.flatnonzero(case["deg"] == 3)[0])
    e1 = int(_slots(case, node)[1])
    e2 = int(np.flatnonzero(coo[:, 1] != node)[0])
    ea = case["ea"].copy()
    ea[e1] = case["ea"][e2]
    ref_f, got = _refaulted(case, ea=ea)
    assert np.array_equal(np.flatnonzero((got != case["base"]).any(1)), [node])
    _rejected(case, got, ref_f, "deg<=4")
