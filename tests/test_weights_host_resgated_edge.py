"""The weight image of a ResGatedGraphConv model with edge features (csrc/gnnb_weights.h: ``build_weight_image`` with a GIN
description, ``gated`` and ``edge_dim``), checked without a GPU by a stand-alone program of its own
(tests/weights_host_resgated_edge_main.cpp, with its own ``main``, built with ``g++`` under the address and undefined-behaviour
sanitizers and run as a child process on files -- never loaded into Python): eight tensors per layer, key / query / value weights
[out, in + edge_dim] with the x columns first; ``w_kqvr`` holds exactly the x column blocks, ``b_kqvr = [b_k | b_q | b_v | bias]``
as for the plain model, and the new slot ``w_gv_edge = [W_g ; W_v]``: ``W_g = W_ke + W_qe`` formed in double and rounded once,
``W_v`` the copy.  And a plain ResGatedGraphConv model's image through this program is byte for byte what
tests/weights_host_resgated_main.cpp gives.  Everything bit for bit."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from resgatede_util import make_resgatede_model
from test_weights_host import GIN, layer_widths, uniform
from test_weights_host_gat import run_gat
from test_weights_host_resgated import MLP_HIDDEN, MLP_N, MLP_OUT, _head, _job, rg_prog, rg_tensors  # noqa: F401  (rg_prog: the fixture)

ROOT = Path(__file__).resolve().parent.parent

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def rge_prog(tmp_path_factory):
    exe = tmp_path_factory.mktemp("weights_host_resgated_edge") / "weights_host_resgated_edge_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I", str(ROOT / "include"),
                    "-I", str(ROOT / "gnn-builder_amd" / "csrc"), str(ROOT / "tests" / "weights_host_resgated_edge_main.cpp"), "-o", str(exe)],
                   check=True)
    return exe


def rge_tensors(rng, fi, fo, d):
    """A layer's eight tensors in canonical order: key, query, value [fo, fi + d] with their biases, lin_skip's weight [fo, fi], the
    conv's bias."""
    return [uniform(rng, fo, fi + d), uniform(rng, fo), uniform(rng, fo, fi + d), uniform(rng, fo), uniform(rng, fo, fi + d), uniform(rng, fo),
            uniform(rng, fo, fi), uniform(rng, fo)]


# (L, in, hidden, out): odd widths, a one-layer model, and the shape at which a GIN model gets the stack kernel's execution-order
# copy -- such a model does not
CASES = [(3, 3, 6, 6), (2, 5, 9, 15), (3, 9, 32, 32), (1, 7, 0, 16), (1, 7, 0, 9)]


def _check_layer(img, layout, l, fi, fo, d, tensors):
    wk, bk, wq, bq, wv, bv, ws, bias = tensors
    off = layout[f"conv{l}.w_kqvr"]
    stacked = img[off:off + 4 * fo * fi].reshape(4 * fo, fi)
    for blk, w in enumerate((wk[:, :fi], wq[:, :fi], wv[:, :fi], ws)):  # exactly the x column blocks, as the layer's GEMM reads them
        assert np.array_equal(stacked[blk * fo:(blk + 1) * fo].view(np.uint32), np.ascontiguousarray(w).view(np.uint32)), (l, blk)
    off = layout[f"conv{l}.b_kqvr"]
    got = img[off:off + 4 * fo].reshape(4, fo)
    assert np.array_equal(got.view(np.uint32), np.stack([bk, bq, bv, bias]).view(np.uint32))  # (b_q is b_q: nothing folded)
    off = layout[f"conv{l}.w_gv_edge"]
    gv = img[off:off + 2 * fo * d].reshape(2, fo, d)
    w_g = (wk[:, fi:].astype(np.float64) + wq[:, fi:].astype(np.float64)).astype(np.float32)  # in double, rounded once
    assert np.array_equal(gv[0].view(np.uint32), w_g.view(np.uint32))
    assert np.array_equal(gv[1].view(np.uint32), np.ascontiguousarray(wv[:, fi:]).view(np.uint32))  # W_v: the copy


@pytest.mark.parametrize("d", [1, 3, 4, 16])
@pytest.mark.parametrize("L,fin,hid,out", CASES)
def test_image_of_a_resgated_edge_model(rge_prog, tmp_path, L, fin, hid, out, d):
    rng = np.random.default_rng(100 * fin + d)
    widths = layer_widths(L, fin, hid, out)
    layers = [rge_tensors(rng, a, b, d) for a, b in widths]
    head = _head(rng, out)
    img, layout = run_gat(rge_prog, tmp_path, _job(GIN, L, fin, hid, out, 1, edge_dim=d, gated=1), [a for t in layers for a in t] + head)
    # blob order: w_kqvr, b_kqvr, w_gv_edge per layer, then the head; every tensor padded to 4 floats; nothing else (no gin_w / gin_b)
    at, want = 0, {}
    for l, (a, b) in enumerate(widths):
        for name, n in (("w_kqvr", 4 * b * a), ("b_kqvr", 4 * b), ("w_gv_edge", 2 * b * d)):
            want[f"conv{l}.{name}"] = at
            at += -(-n // 4) * 4
    for i, t in enumerate(head):
        want[f"head{i // 2}.{'wb'[i % 2]}"] = at
        at += -(-t.size // 4) * 4
    assert layout == want and img.size == at
    for l, (a, b) in enumerate(widths):
        _check_layer(img, layout, l, a, b, d, layers[l])
    for i, t in enumerate(head):
        off = layout[f"head{i // 2}.{'wb'[i % 2]}"]
        assert np.array_equal(img[off:off + t.size], t.ravel())


def test_the_gate_fold_is_rounded_once(rge_prog, tmp_path):
    """Where the fp32 sum and the once-rounded double sum could differ they do not: the sum of two floats is exact in double, so
    the fold IS the correctly rounded fp32 sum -- checked on values whose fp32 sum rounds (1 + 2^-24 ties, a cancelling pair)."""
    fi, fo, d = 3, 4, 3
    rng = np.random.default_rng(5)
    t = rge_tensors(rng, fi, fo, d)
    t[0][:, fi:] = np.float32(1.0)
    t[2][:, fi:] = np.array([2.0 ** -24, 3 * 2.0 ** -25, -1.0 + 2.0 ** -23], np.float32)
    img, layout = run_gat(rge_prog, tmp_path, _job(GIN, 1, fi, 0, fo, 0, edge_dim=d, gated=1), t + _head(rng, fo))
    _check_layer(img, layout, 0, fi, fo, d, t)
    off = layout["conv0.w_gv_edge"]
    assert np.array_equal(img[off:off + d], np.array([1.0, 1.0 + 2.0 ** -23, 2.0 ** -23], np.float32))


def test_image_of_a_model_from_models_py(rge_prog, tmp_path):
    """``GNNModel.canonical_params()`` of a seeded model through the builder: the blocks are the model's own tensors, split."""
    d = 3
    model = make_resgatede_model(in_dim=9, edge_dim=d, hidden=12, layers=2, out_dim=8, pools=("add", "max"), mlp_hidden=MLP_HIDDEN,
                                 mlp_layers=1, task_out=MLP_OUT)
    params = [p.numpy() for p in model.canonical_params()]
    assert len(params) == 2 * 8 + 2 * MLP_N
    img, layout = run_gat(rge_prog, tmp_path, _job(GIN, 2, 9, 12, 8, 1, edge_dim=d, gated=1), params)
    for l, conv in enumerate(model.gnn_convs):
        c = conv.conv
        fo, fi = c.lin_skip.weight.shape
        assert c.lin_key.weight.shape == (fo, fi + d)
        g = lambda p: p.detach().numpy()  # noqa: E731
        _check_layer(img, layout, l, fi, fo, d, [g(c.lin_key.weight), g(c.lin_key.bias), g(c.lin_query.weight), g(c.lin_query.bias),
                                                 g(c.lin_value.weight), g(c.lin_value.bias), g(c.lin_skip.weight), g(c.bias)])


@pytest.mark.parametrize("L,fin,hid,out,skip", [(3, 9, 32, 32, 1), (2, 5, 9, 15, 0), (1, 7, 0, 9, 1)])
def test_plain_resgated_blob_is_what_it_was(rg_prog, rge_prog, tmp_path, L, fin, hid, out, skip):  # noqa: F811
    rng = np.random.default_rng(fin + 2)
    flat = [a for fi, fo in layer_widths(L, fin, hid, out) for a in rg_tensors(rng, fi, fo)] + _head(rng, out)
    job = _job(GIN, L, fin, hid, out, skip, gated=1)
    img, layout = run_gat(rg_prog, tmp_path, job, flat)
    img2, layout2 = run_gat(rge_prog, tmp_path, job, flat)
    assert img2.tobytes() == img.tobytes() and layout2 == layout and "conv0.w_gv_edge" not in layout2
