"""What every stage entry point of ``CompiledModel`` hands to the C ABI: which pointer, which row stride, which scalar, in which
place -- and what it refuses before anything crosses.  No kernel runs: the library is a recorder, the model a bare shell with the
sizes of a prepared batch.  (CUDA tensors all the same: the operand checks refuse CPU ones.)

Every strided operand is a column slice of a buffer ``ROW`` floats wide.  At (N, E) = (3, 4) its row stride crosses as it is; at
(1, 0) a node matrix has one row, for which the entries pass its own column count (any stride describes one row, and the C side
requires ld >= columns), and the edge operands of a batch without edges cross as NULL."""
import pytest
import torch

from gnnbuilder_amd import runtime
from gnnbuilder_amd.runtime import ACT, AGG, NN_AGGR, GnnbError

pytestmark = pytest.mark.gpu

W, H, ED, R, ROW = 8, 2, 3, 2, 40
SIZES = ((3, 4), (1, 0))


class Recorder:
    """Stands in for the loaded library: every symbol is a function that stores its arguments and reports GNNB_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, symbol):
        def entry(*args):
            self.calls.append((symbol, args))
            return 0
        return entry


def shell(N, E):
    cm = object.__new__(runtime.CompiledModel)
    cm._N, cm._E, cm._ws, cm.edge_dim = N, E, None, ED
    cm.lib = Recorder()
    return cm


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


class Operands:
    """Tensors of one (N, E) and the expectations that go with them."""

    def __init__(self, N, E, dev):
        self.N, self.E, self.dev = N, E, dev
        self.stream = int(torch.cuda.current_stream().cuda_stream)

    def cut(self, rows, cols):  # a column slice: row stride ROW, its pointer 3 floats into the buffer
        return torch.zeros((rows, ROW), device=self.dev)[:, 3:3 + cols]

    def full(self, *shape, dtype=torch.float32):
        return torch.zeros(shape, dtype=dtype, device=self.dev)

    def nld(self, cols):  # the ld of a node matrix [N, cols] cut from a buffer
        return ROW if self.N > 1 else cols

    def eptr(self, t):  # an operand with one row per edge
        return t.data_ptr() if self.E else None


def p(t):
    return t.data_ptr()


# one function per entry: (the C symbol, the call's result or None, the argument tuple the symbol must receive)
def case_aggregate(cm, o):
    x, out = o.full(o.N, W), o.full(o.N, W)
    cm.aggregate("sum", x, eps=0.25, out=out)
    return "gnnb_aggregate", (None, AGG["sum"], p(x), None, p(out), W, 0.25, o.stream)


def case_pna_product_aggregate(cm, o):
    x, wb, out = o.full(o.N, W), o.cut(W, W), o.full(o.N, 4 * W)
    cm.pna_product_aggregate(x, wb, out=out)
    return "gnnb_pna_product_aggregate", (None, p(x), p(wb), ROW, p(out), W, o.stream)


def case_aggregate_edges(cm, o):
    x, term, out = o.full(o.N, W), o.full(o.E, W), o.full(o.N, W)
    cm.aggregate_edges(x, term, eps=0.5, out=out)
    return "gnnb_aggregate_edges", (None, p(x), p(term), p(out), W, 0.5, o.stream)


def case_aggregate_edges_fused(cm, o):
    x, ea, we, be, out = o.full(o.N, W), o.full(o.E, ED), o.cut(W, ED), o.full(W), o.full(o.N, W)
    cm.aggregate_edges_fused(x, ea, we, be, eps=0.5, out=out)
    return "gnnb_aggregate_edges_fused", (None, p(x), o.eptr(ea), ED, p(we), ROW, p(be), p(out), W, 0.5, o.stream)


def case_aggregate_pna_edges(cm, o):
    x, ea, we, be, out = o.full(o.N, W), o.full(o.E, ED), o.cut(W, ED), o.full(W), o.full(o.N, 4 * W)
    cm.aggregate_pna_edges(x, None, ea, we, be, out=out)
    return "gnnb_aggregate_pna_edges", (None, p(x), None, o.eptr(ea), ED, p(we), ROW, p(be), p(out), W, o.stream)


def case_aggregate_gatv2(cm, o):
    xl, xr, att, out = o.cut(o.N, W), o.cut(o.N, W), o.full(W), o.full(o.N, W)
    cm.aggregate_gatv2(xl, xr, att, act="relu", heads=H, negative_slope=0.125, out=out)
    return "gnnb_aggregate_gatv2", (None, p(xl), o.nld(W), p(xr), o.nld(W), p(att), None, None, ACT["relu"], H, 0.125, p(out), W, o.stream)


def case_aggregate_gatv2_edges(cm, o):
    xl, xr, att, ea, we, out = o.cut(o.N, W), o.cut(o.N, W), o.full(W), o.full(o.E, ED), o.cut(W, ED), o.full(o.N, W)
    cm.aggregate_gatv2_edges(xl, xr, att, ea, we, act="relu", heads=H, negative_slope=0.125, out=out)
    return "gnnb_aggregate_gatv2_edges", (None, p(xl), o.nld(W), p(xr), o.nld(W), p(att), None, None, ACT["relu"], H, 0.125, o.eptr(ea), ED,
                                          p(we), ROW, p(out), W, o.stream)


def case_aggregate_gat(cm, o):
    xl, ss, sd, bias, out = o.cut(o.N, W), o.cut(o.N, H), o.cut(o.N, H), o.full(W), o.full(o.N, W)
    cm.aggregate_gat(xl, ss, sd, bias=bias, act="tanh", heads=H, negative_slope=0.125, out=out)
    return "gnnb_aggregate_gat", (None, p(xl), o.nld(W), p(ss), o.nld(H), p(sd), o.nld(H), p(bias), None, ACT["tanh"], H, 0.125, p(out), W,
                                  o.stream)


def case_aggregate_gat_edges(cm, o):
    xl, ss, sd, ea, ae, out = o.cut(o.N, W), o.cut(o.N, H), o.cut(o.N, H), o.full(o.E, ED), o.cut(H, ED), o.full(o.N, W)
    cm.aggregate_gat_edges(xl, ss, sd, ea, ae, act="tanh", heads=H, negative_slope=0.125, out=out)
    return "gnnb_aggregate_gat_edges", (None, p(xl), o.nld(W), p(ss), o.nld(H), p(sd), o.nld(H), None, None, ACT["tanh"], H, 0.125,
                                        o.eptr(ea), ED, p(ae), ROW, p(out), W, o.stream)


def case_aggregate_transformer(cm, o):
    q, k, v, root, skip, out = o.cut(o.N, W), o.cut(o.N, W), o.cut(o.N, W), o.cut(o.N, W), o.full(o.N, W), o.full(o.N, W)
    cm.aggregate_transformer(q, k, v, root=root, skip=skip, act="gelu", heads=H, scale=0.5, out=out)
    return "gnnb_aggregate_transformer", (None, p(q), o.nld(W), p(k), o.nld(W), p(v), o.nld(W), p(root), o.nld(W), p(skip), ACT["gelu"], H, 0.5,
                                          p(out), W, o.stream)


def case_aggregate_transformer_edges(cm, o):
    q, k, v, qe, root, out = o.cut(o.N, W), o.cut(o.N, W), o.cut(o.N, W), o.cut(o.N, H * ED), o.cut(o.N, W), o.full(o.N, W)
    ea, we = o.full(o.E, ED), o.cut(W, ED)
    cm.aggregate_transformer_edges(q, k, v, qe, ea, we, root=root, act="gelu", heads=H, scale=0.5, out=out)
    return "gnnb_aggregate_transformer_edges", (None, p(q), o.nld(W), p(k), o.nld(W), p(v), o.nld(W), p(qe), o.nld(H * ED), p(root), o.nld(W),
                                                None, ACT["gelu"], H, 0.5, o.eptr(ea), ED, p(we), ROW, p(out), W, o.stream)


def case_aggregate_resgated(cm, o):
    k, q, v, out = o.cut(o.N, W), o.cut(o.N, W), o.cut(o.N, W), o.full(o.N, W)
    cm.aggregate_resgated(k, q, v, act="sigmoid", out=out)
    # (no root: NULL, and the width where its ld would stand)
    return "gnnb_aggregate_resgated", (None, p(k), o.nld(W), p(q), o.nld(W), p(v), o.nld(W), None, W, None, ACT["sigmoid"], p(out), W, o.stream)


def case_aggregate_resgated_edges(cm, o):
    k, q, v, out = o.cut(o.N, W), o.cut(o.N, W), o.cut(o.N, W), o.full(o.N, W)
    ea, wg, wv = o.full(o.E, ED), o.cut(W, ED), o.cut(W, ED)
    cm.aggregate_resgated_edges(k, q, v, ea, wg, wv, act="sigmoid", out=out)
    return "gnnb_aggregate_resgated_edges", (None, p(k), o.nld(W), p(q), o.nld(W), p(v), o.nld(W), None, W, None, ACT["sigmoid"], o.eptr(ea),
                                             ED, p(wg), ROW, p(wv), ROW, p(out), W, o.stream)


def case_aggregate_ggnn(cm, o):
    pm, gh, h, out = o.cut(o.N, 3 * W), o.cut(o.N, 3 * W), o.cut(o.N, 5), o.full(o.N, W)
    cm.aggregate_ggnn(pm, gh, h, act="none", out=out)
    return "gnnb_aggregate_ggnn", (None, p(pm), o.nld(3 * W), p(gh), o.nld(3 * W), p(h), o.nld(5), 5, None, None, ACT["none"], p(out), W,
                                   o.stream)


def case_aggregate_nnconv(cm, o):
    x, ea, out = o.full(o.N, W), o.full(o.E, ED), o.cut(o.N, (ED + 1) * W)
    cm.aggregate_nnconv(x, ea, aggr="mean", out=out)
    return "gnnb_aggregate_nnconv", (None, p(x), W, o.eptr(ea), ED, None, None, 0, NN_AGGR["mean"], p(out), o.nld((ED + 1) * W), o.stream)


def case_aggregate_gen(cm, o):
    s, r, out = o.cut(o.N, W), o.cut(o.N, W), o.cut(o.N, W)
    ea, we, be = o.full(o.E, ED), o.full(W, ED), o.full(W)
    cm.aggregate_gen(s, r, ea, we, be, t=0.5, eps=0.25, out=out)
    return "gnnb_aggregate_gen", (None, p(s), o.nld(W), p(r), o.nld(W), W, o.eptr(ea), ED, p(we), ED, p(be), 0.5, 0.25, p(out), o.nld(W),
                                  o.stream)


def case_rgcn_slots(cm, o):
    et = o.full(o.E, dtype=torch.int32)
    rec = cm.rgcn_slots(et, R)
    assert tuple(rec.shape) == (o.E, 2) and rec.dtype == torch.int32
    return "gnnb_rgcn_slots", (None, o.eptr(et), R, o.eptr(rec), o.stream)


def case_aggregate_rgcn(cm, o):
    rec, pm, root, out = o.full(o.E, 2, dtype=torch.int32), o.cut(o.N, R * W), o.cut(o.N, W), o.full(o.N, W)
    cm.aggregate_rgcn(rec, pm, R, root=root, act="relu", out=out)
    return "gnnb_aggregate_rgcn", (None, o.eptr(rec), p(pm), o.nld(R * W), R, p(root), o.nld(W), None, ACT["relu"], p(out), W, o.stream)


CASES = [f for name, f in sorted(globals().items()) if name.startswith("case_")]


@pytest.mark.parametrize("sizes", SIZES, ids=lambda s: f"N{s[0]}E{s[1]}")
@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__[5:])
def test_arguments(dev, case, sizes):
    cm = shell(*sizes)
    symbol, args = case(cm, Operands(*sizes, dev))
    assert cm.lib.calls == [(symbol, args)]


def test_every_stage_method_has_a_case():
    methods = {m for m in vars(runtime.CompiledModel) if m.startswith("aggregate") and m != "aggregate_timed"}
    assert methods | {"pna_product_aggregate", "rgcn_slots"} == {f.__name__[5:] for f in CASES}


def refused(dev, message, call):
    cm, o = shell(3, 4), Operands(3, 4, dev)
    with pytest.raises(GnnbError) as info:
        call(cm, o)
    assert str(info.value) == message
    assert cm.lib.calls == []


def test_refuses_heads_that_do_not_divide_the_width(dev):
    refused(dev, "width 8: a GATv2 layer is at most 256 wide and divisible by heads (3)",
            lambda cm, o: cm.aggregate_gatv2(o.cut(3, W), o.cut(3, W), o.full(W), heads=3))
    refused(dev, "width 8: a GAT layer is at most 256 wide and divisible by heads (3)",
            lambda cm, o: cm.aggregate_gat_edges(o.cut(3, W), o.cut(3, 3), o.cut(3, 3), o.full(4, ED), o.cut(3, ED), heads=3))
    refused(dev, "heads must be an int in 1 .. 8, got 9",
            lambda cm, o: cm.aggregate_transformer(o.cut(3, W), o.cut(3, W), o.cut(3, W), heads=9))


def test_refuses_an_unknown_act(dev):
    message = "act must be one of ['gelu', 'none', 'relu', 'sigmoid', 'tanh'], got 'swish'"
    refused(dev, message, lambda cm, o: cm.aggregate_resgated(o.cut(3, W), o.cut(3, W), o.cut(3, W), act="swish"))
    refused(dev, message, lambda cm, o: cm.aggregate_rgcn(o.full(4, 2, dtype=torch.int32), o.cut(3, R * W), R, act="swish"))


def test_refuses_a_block_of_another_width(dev):
    refused(dev, f"k must be [3, 8] on {dev}, got (3, 9) on {dev}",
            lambda cm, o: cm.aggregate_transformer(o.cut(3, W), o.cut(3, W + 1), o.cut(3, W)))
    refused(dev, "k has shape (3, 7); expected 3 rows",
            lambda cm, o: cm.aggregate_transformer_edges(o.cut(3, W), o.cut(3, W - 1), o.cut(3, W), o.cut(3, ED), o.full(4, ED), o.cut(W, ED)))


def test_refuses_an_edge_weight_too_wide(dev):
    message = f"w_edge must be [8, 1 .. 16] on {dev}, got (8, 17) on {dev}"
    refused(dev, message, lambda cm, o: cm.aggregate_edges_fused(o.full(3, W), o.full(4, 17), o.cut(W, 17), o.full(W)))
    refused(dev, message, lambda cm, o: cm.aggregate_gatv2_edges(o.cut(3, W), o.cut(3, W), o.full(W), o.full(4, 17), o.cut(W, 17)))


def test_refuses_a_bias_of_another_dtype(dev):
    refused(dev, "bias must be torch.float32, got torch.float64",
            lambda cm, o: cm.aggregate_gat(o.cut(3, W), o.cut(3, H), o.cut(3, H), bias=o.full(W, dtype=torch.float64), heads=H))
    refused(dev, "b_edge must be torch.float32, got torch.float64",
            lambda cm, o: cm.aggregate_pna_edges(o.full(3, W), None, o.full(4, ED), o.cut(W, ED), o.full(W, dtype=torch.float64)))


def test_refuses_relations_out_of_range(dev):
    refused(dev, "relations must be an int in 1 .. 8, got 9", lambda cm, o: cm.rgcn_slots(o.full(4, dtype=torch.int32), 9))
