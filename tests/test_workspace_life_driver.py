"""The long-lived-workspace driver on the CPU (``tests/workspace_life_util.py``): with the fp32 torch model standing in for the
device it passes; with a stand-in that carries ONE kind of stale state from the batch before -- each first shown to move the
float64 value by more than 1e-3 of the output's scale -- it fails, by the bit comparison with a fresh object (a) and, on its
own, by the float64 budget (b).  No GPU."""
import copy
import dataclasses

import numpy as np
import pytest
import torch

import ggnn_util
import gine_util
import pnae_util
import ref64 as R
import workspace_life_util as W
from gnnbuilder_amd import synthetic
from gnnbuilder_amd.batching import pack_graphs
from helpers import EMPTY, ONE, edge_batch, make_model

IN_DIM, EDGE_DIM, STAGE_W = 9, 3, 32


def _models(edges):
    model = gine_util.make_gine_model(in_dim=IN_DIM, edge_dim=EDGE_DIM, hidden=32, layers=2, seed=3) if edges else \
        make_model("gin", in_dim=IN_DIM, hidden=32, layers=2, seed=3)
    return model, copy.deepcopy(model).double()


def _steps(edges):
    """Four unlike batches: the hub batch, a smaller molecule batch as a shuffled mini-batch, a few graphs of at most one node
    among two molecules, and a larger molecule batch as a shuffled mini-batch."""
    mols = synthetic.make_batch("qm9", 2, seed=8)
    small = pack_graphs([ONE(IN_DIM), EMPTY(IN_DIM), (mols.graph(0)[0][:, :IN_DIM], mols.graph(0)[1]), (np.full((1, IN_DIM), -0.25, np.float32), ONE(IN_DIM)[1]),
                         (mols.graph(1)[0][:, :IN_DIM], mols.graph(1)[1]), EMPTY(IN_DIM)])
    raw = [("hub", edge_batch(8, IN_DIM, seed=21), False), ("qm9-16", W.with_features(synthetic.make_batch("qm9", 16, seed=5), IN_DIM, 5), True),
           ("lone", small, False), ("qm9-24", W.with_features(synthetic.make_batch("qm9", 24, seed=6), IN_DIM, 6), True)]
    steps = []
    for i, (name, b, pyg) in enumerate(raw):
        ea = gine_util.edge_attrs(b.num_edges, EDGE_DIM, seed=40 + i) if edges else None
        mini = None
        if pyg:
            b, ea, mini, _ = W.shuffled_mini_batch(b, ea, seed=50 + i)
        stage = dict(x=np.random.default_rng(60 + i).uniform(-1, 1, (b.num_nodes, STAGE_W)).astype(np.float32))
        steps.append(W.Step(name, b, "pyg" if pyg else "forward", edge_attr=ea, pyg=mini, stage=stage))
    assert steps[1].batch.num_nodes < steps[0].batch.num_nodes and steps[1].batch.num_edges < steps[0].batch.num_edges
    assert steps[3].batch.num_nodes > steps[2].batch.num_nodes and steps[3].batch.num_edges > steps[1].batch.num_edges
    assert (np.diff(steps[2].batch.node_ptr) <= 1).sum() == 4
    return steps


def _plain(step):
    """The step as a fresh object takes it: the plain forward on the batch's own arrays."""
    return dataclasses.replace(step, entry="forward", pyg=None)


def _fresh(model):
    return lambda step: W.TorchDevice(model).run(_plain(step))


def _reference(model, model64):
    def reference(step):
        ref, base = W.TorchDevice(model64).run(_plain(step)), W.TorchDevice(model).run(_plain(step))
        return {"out": (ref["out"], base["out"]), "stage": (ref["stage"], base["stage"], R.workspace_edges(step.batch.coo, True))}
    return reference


@pytest.mark.parametrize("edges", [False, True])
def test_the_honest_stand_in_passes(edges):
    model, model64 = _models(edges)
    steps = _steps(edges)
    seen = {}
    longs = W.run_sequence(steps, W.TorchDevice(model).run, _fresh(model), _reference(model, model64),
                           record=lambda k, r: seen.__setitem__(k, max(seen.get(k, 0.0), r)))
    assert len(longs) == len(steps) and all(set(r) == {"out", "path", "stage"} for r in longs)
    assert seen["out"] == pytest.approx(1.0) and seen["stage/all"] == pytest.approx(1.0)  # (the stand-in IS base: e = e32)


@pytest.mark.parametrize("edges", [False, True])
def test_the_stand_in_is_the_reference_walk(edges):
    """``torch_forward`` is ``ref64.run`` / ``gine_util.run`` with a hook: the same bits."""
    model, model64 = _models(edges)
    for step in _steps(edges):
        b = step.batch
        for m in (model, model64):
            want = gine_util.run(m, b, b.x, step.edge_attr) if edges else R.run(m, b, b.x)
            got = W.torch_forward(m, b, b.x, step.edge_attr)[0]
            assert got.dtype == want.dtype and np.array_equal(got, want)


def _moves_float64(fault, edges):
    """The largest change the fault makes to a float64 result over the sequence, relative to that result's scale."""
    _, model64 = _models(edges)
    honest, stale = W.TorchDevice(model64), W.TorchDevice(model64, fault)
    worst = 0.0
    for step in _steps(edges):
        want, got = honest.run(step), stale.run(step)
        for key in ("out", "stage"):
            worst = max(worst, float(np.abs(got[key] - want[key]).max() / np.abs(want[key]).max()))
    return worst


@pytest.mark.parametrize("check", ["a", "b"])
@pytest.mark.parametrize("fault", W.FAULTS)
def test_each_kind_of_stale_state_is_rejected(fault, check):
    edges = fault == "previous-edge-order"
    assert _moves_float64(fault, edges) > 1e-3
    model, model64 = _models(edges)
    steps = _steps(edges)
    stale = W.TorchDevice(model, fault)
    if check == "a":  # against a fresh object's bits
        run_long, run_fresh = stale.run, _fresh(model)
    else:  # the fresh object echoes the long-lived one, so that (a) holds and the float64 budget has to speak
        last = {}
        run_long = lambda step: last.setdefault(id(step), stale.run(step))  # noqa: E731
        run_fresh = lambda step: copy.deepcopy(last[id(step)])  # noqa: E731
    with pytest.raises(AssertionError, match=rf"^\({check}\) step"):
        W.run_sequence(steps, run_long, run_fresh, _reference(model, model64))


def test_the_bit_comparison_leaves_nothing_out():
    a = np.linspace(-1, 1, 12, dtype=np.float32).reshape(3, 4)
    good = dict(out=a, path="layerwise", tables=(np.arange(5, dtype=np.int32), np.arange(3, dtype=np.int32)), stage=a * 2)
    W.assert_same_bits(good, copy.deepcopy(good), "same")
    ulp = a.copy()
    ulp[2, 1] = np.nextafter(ulp[2, 1], np.float32(2))
    zero, negzero = a.copy(), a.copy()
    zero[0, 0], negzero[0, 0] = 0.0, -0.0
    nan1, nan2 = a.copy(), a.copy()
    nan1.view(np.uint32)[1, 1], nan2.view(np.uint32)[1, 1] = 0x7fc00000, 0x7fc00001
    tables = (good["tables"][0], np.array([0, 2, 1], np.int32))
    for left, right, where in ((good, dict(good, out=ulp), r"out\[0\] differs in 1 of 12 elements, first at \(2, 1\)"),
                               (good, dict(good, stage=ulp * 2), "stage"), (good, dict(good, path="stack_zf"), "path"),
                               (good, dict(good, tables=tables), r"tables\[1\]"), (good, dict(good, tables=good["tables"][:1]), "2 arrays against 1"),
                               (good, dict(good, out=a.astype(np.float64)), "float32"), (good, dict(good, out=a[:2]), r"\(3, 4\) against"),
                               (good, {k: v for k, v in good.items() if k != "stage"}, "different things"),
                               (good, dict(out=a, path="layerwise", tables=good["tables"], stage_refused="bad argument"), "different things"),
                               (dict(good, out=nan1), dict(good, out=nan2), r"first at \(1, 1\)"),  # two NaNs of other payloads
                               (dict(good, out=zero), dict(good, out=negzero), r"first at \(0, 0\)")):  # 0 and -0
        with pytest.raises(AssertionError, match=where):
            W.assert_same_bits(left, right, "x")
    W.assert_same_bits(dict(good, out=nan1), dict(good, out=nan1.copy()), "the same NaN")
    W.assert_same_bits(dict(refused="null argument"), dict(refused="null argument"), "refusals")
    with pytest.raises(AssertionError, match="refused"):
        W.assert_same_bits(dict(refused="null argument"), dict(refused="bad argument"), "refusals")


def test_the_driver_compares_a_repeat_and_wants_every_reference():
    model, model64 = _models(False)
    steps = _steps(False)[:2]
    steps.append(dataclasses.replace(steps[0], name="hub-again", same_as=0))
    W.run_sequence(steps, W.TorchDevice(model).run, _fresh(model), _reference(model, model64))
    drift = [0]

    def drifting(step):  # the third step's repeat of the first differs in one bit, on both objects alike
        res = W.TorchDevice(model).run(_plain(step))
        drift[0] += step.same_as is not None
        if step.same_as is not None:
            res["out"] = res["out"].copy()
            res["out"].view(np.uint32)[0, 0] ^= 1
        return res
    with pytest.raises(AssertionError, match=r"^\(a\) step 3 hub-again \[forward\]: against step 1 on the same object"):
        W.run_sequence(steps, drifting, drifting, _reference(model, model64))
    assert drift[0] == 2
    no_stage = lambda step: {"out": _reference(model, model64)(step)["out"]}  # noqa: E731
    with pytest.raises(AssertionError, match=r"^\(b\) step 1 .*no reference for \['stage'\]"):
        W.run_sequence(steps, W.TorchDevice(model).run, _fresh(model), no_stage)


def test_pna_variances_are_pnae_utils():
    """``pna_layer_variances`` on a PNAE model is ``pnae_util.layer_variances``; on a PNA model it sees the pre-NN's messages."""
    b = W.with_features(synthetic.make_batch("qm9", 6, seed=2), IN_DIM, 2, grid=True)
    ea = gine_util.edge_attrs(b.num_edges, EDGE_DIM, seed=3)
    pnae = pnae_util.make_pnae_model(in_dim=IN_DIM, edge_dim=EDGE_DIM, hidden=32, layers=2, seed=1)
    for (v0, h0), (v1, h1) in zip(W.pna_layer_variances(pnae, b, b.x, ea), pnae_util.layer_variances(pnae, b, b.x, ea)):
        assert np.array_equal(v0, v1) and np.array_equal(h0, h1)
    pna = make_model("pna", in_dim=IN_DIM, hidden=32, layers=2, seed=1)
    (v, hi), _ = W.pna_layer_variances(pna, b, b.x)
    conv = copy.deepcopy(pna).double().gnn_convs[0].conv
    x = torch.from_numpy(b.x).double()
    src, dst = b.coo[:, 0].astype(np.int64), b.coo[:, 1].astype(np.int64)
    with torch.no_grad():
        msg = conv.pre_nns[0](torch.cat([x[dst], x[src]], -1)).numpy()
    i = int(np.flatnonzero(np.bincount(dst, minlength=b.num_nodes) > 0)[0])
    assert np.allclose(v[0], msg[dst == i].var(0), rtol=0, atol=1e-12) and np.array_equal(hi[0], (msg[dst == i] ** 2).max(0))
    assert W.variances_near_the_threshold(pna, pack_graphs([EMPTY(IN_DIM)] * 2), np.zeros((0, IN_DIM), np.float32)) == 0


@pytest.mark.parametrize("family", sorted(W.PNA_SEEDS))
def test_the_pna_sequences_stay_clear_of_the_std_threshold(family):
    """The seeds the GPU file uses for pna / pnae were chosen here, on the float64 reference alone: no variance of any layer on
    any batch of the sequence within the margin of PyG's 1e-5, nothing excluded."""
    model, batches, attrs = W.family_sequence(family)
    for b, ea in zip(batches, attrs):
        assert W.variances_near_the_threshold(model, b, b.x, ea) == 0


# ---------------------------------------------------------------------------------------------------- the four newer families
NEWER = ("resgatede", "gat", "gate", "ggnn")


@pytest.fixture(scope="module")
def newer_sequences():
    return {f: W.family_sequence(f) for f in NEWER}


@pytest.mark.parametrize("family", NEWER)
def test_the_newer_families_sequences_build(newer_sequences, family):
    assert family in W.FAMILIES and (family in W.EDGE_FAMILIES) == (family in ("resgatede", "gate"))
    model, batches, attrs = newer_sequences[family]
    assert len(batches) == len(attrs) == len(W.SIZES_UP_AND_DOWN) and batches[7] is batches[0]
    for b, ea in zip(batches, attrs):
        if family in W.EDGE_FAMILIES and b.num_edges:
            assert ea.shape == (b.num_edges, W.EDGE_DIM) and ea.dtype == np.float32
        else:
            assert ea is None
    if family == "ggnn":  # (three steps per layer: both state buffers are written and read in turn)
        assert W.GGNN_STEPS == 3 and all(c.conv.num_layers == 3 for c in model.gnn_convs)


@pytest.mark.parametrize("family", NEWER)
def test_the_newer_families_stage_cases_hold_on_every_batch(newer_sequences, family):
    """``stage_operands`` and ``stage_refs`` on all eight batches, the hub's 1200 in-edges among them: the reference-only asserts
    of ``stage_refs`` hold (exact scores, gate arguments, gated values, neighbour sums), and the fp32 restatement stays within
    the budget of the float64 one in every in-degree class -- a condition on the inputs fails here, long before a GPU run."""
    _, batches, _ = newer_sequences[family]
    for i, b in enumerate(batches):
        c = W.stage_operands(family, b, 700 + i)
        if family in W.EDGE_FAMILIES:
            assert c["edge_attr"].shape == (b.num_edges, W.EDGE_DIM)
        if family == "ggnn":
            assert c["h"].shape == (b.num_nodes, W.GGNN_H_WIDTH) and W.GGNN_H_WIDTH < W.STAGE_W
        ref, base, coo = W.stage_refs(family, b, c)
        assert ref.shape == base.shape == (b.num_nodes, W.STAGE_W) and ref.dtype == np.float64 and base.dtype == np.float32
        if b.num_nodes:
            gine_util.budget_by_degree(base, ref, base, coo, what=f"{family} {W.SIZES_UP_AND_DOWN[i]}")


@pytest.mark.parametrize("family", NEWER)
def test_the_newer_families_model_references_pair_up(newer_sequences, family):
    model, batches, attrs = newer_sequences[family]
    for i in (0, 1, 2, 3, 6):  # (one of each kind of batch: molecules, one node, the hub batch, lone nodes, larger molecules)
        ref, base = W.model_refs(family, model, batches[i], attrs[i])
        assert ref.dtype == np.float64 and base.dtype == np.float32 and ref.shape == base.shape == (batches[i].num_graphs, 19)
        R.budget(base, ref, base, what=f"{family} {W.SIZES_UP_AND_DOWN[i]}")


def test_the_ggnn_state_offset_moves_along_the_sequence():
    """At hidden 9 the second state buffer lies ``roundup4(9 N)`` floats into the scratch: over the sequence ``9 N mod 4`` takes at
    least three values, and the captured batch's differs from the hub batch's."""
    counts = [b.num_nodes for b in W.family_sequence("ggnn", hidden=9)[1]]
    assert counts == [1742, 1, 489, 64, 1742, 0, 1051, 1742]
    assert len({(9 * n) % 4 for n in counts}) >= 3
    assert ((9 * counts[0]) % 4, (9 * counts[2]) % 4) == (2, 1)


@pytest.mark.parametrize("fault", ggnn_util.FAULTS)
def test_the_stage_comparison_rejects_a_wrong_gru(newer_sequences, fault):
    """A wrong kernel restated in fp32 (``ggnn_util.FAULTS``) in the place of ``got`` on the ``edge-batch`` step, at ``h_width`` 12:
    ``stage_refs``' comparison rejects it in at least one in-degree class, and takes the right one."""
    b = newer_sequences["ggnn"][1][2]
    c = W.stage_operands("ggnn", b, 702)
    ref, base, coo = W.stage_refs("ggnn", b, c)
    gine_util.budget_by_degree(base, ref, base, coo, what="the right GRU")
    wrong = ggnn_util.ggnn_ref(c["p"], c["gh"], c["h"], c["b_ih"], None, "none", b.coo, dtype=np.float32, fault=fault)
    assert wrong.dtype == np.float32 and wrong.shape == base.shape
    with pytest.raises(AssertionError):
        gine_util.budget_by_degree(wrong, ref, base, coo, what=fault)
