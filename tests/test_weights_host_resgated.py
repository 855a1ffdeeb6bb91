"""The weight image of a ResGatedGraphConv model (csrc/gnnb_weights.h: ``build_weight_image`` with a GIN description and
``gated``), checked without a GPU by a stand-alone program of its own (tests/weights_host_resgated_main.cpp, with its own
``main``, built with ``g++`` under the address and undefined-behaviour sanitizers and run as a child process on files -- never
loaded into Python): eight tensors per layer; ``w_kqvr = [W_k ; W_q ; W_v ; W_skip]`` and ``b_kqvr = [b_k | b_q | b_v | bias]``
-- the conv's own bias rides as the skip block's, ``b_q`` is not folded into ``b_k`` --, compared block by block with the
model's tensors; no execution-order copy; the head last.  And the images of a GIN and a plain TransformerConv model through this
program are byte for byte what the existing host programs give.  Everything bit for bit."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from resgated_util import make_resgated_model
from test_weights_host import GIN, build_image, layer_widths, prog, uniform  # noqa: F401  (prog: the fixture)
from test_weights_host_gat import run_gat
from test_weights_host_transformer import tf_prog, tf_tensors  # noqa: F401  (tf_prog: the fixture)

ROOT = Path(__file__).resolve().parent.parent

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def rg_prog(tmp_path_factory):
    exe = tmp_path_factory.mktemp("weights_host_resgated") / "weights_host_resgated_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I", str(ROOT / "include"),
                    "-I", str(ROOT / "gnn-builder_amd" / "csrc"), str(ROOT / "tests" / "weights_host_resgated_main.cpp"), "-o", str(exe)],
                   check=True)
    return exe


POOLS, MLP_N, MLP_HIDDEN, MLP_OUT = 2, 2, 6, 3


def _head(rng, out):
    return [uniform(rng, MLP_HIDDEN, POOLS * out), uniform(rng, MLP_HIDDEN), uniform(rng, MLP_OUT, MLP_HIDDEN), uniform(rng, MLP_OUT)]


def _job(conv, L, fin, hid, out, skip, edge_dim=0, gat_heads=0, tf_heads=0, gated=0):
    return [conv, L, fin, hid, out, skip, edge_dim, gat_heads, tf_heads, gated, MLP_N, MLP_HIDDEN, MLP_OUT, POOLS]


def rg_tensors(rng, fi, fo):
    """A layer's eight tensors in canonical order: key, query, value with their biases, lin_skip's weight, the conv's bias."""
    return [uniform(rng, fo, fi), uniform(rng, fo), uniform(rng, fo, fi), uniform(rng, fo), uniform(rng, fo, fi), uniform(rng, fo),
            uniform(rng, fo, fi), uniform(rng, fo)]


# (L, in, hidden, out): odd widths, a one-layer model, and the shape at which a GIN model gets the stack kernel's execution-order
# copy -- such a model does not
CASES = [(3, 3, 6, 6), (2, 5, 9, 15), (3, 9, 32, 32), (1, 7, 0, 16), (1, 7, 0, 9)]


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("L,fin,hid,out", CASES)
def test_image_of_a_resgated_model(rg_prog, tmp_path, L, fin, hid, out, skip):
    rng = np.random.default_rng(100 * fin + skip)
    widths = layer_widths(L, fin, hid, out)
    layers = [rg_tensors(rng, a, b) for a, b in widths]
    head = _head(rng, out)
    img, layout = run_gat(rg_prog, tmp_path, _job(GIN, L, fin, hid, out, skip, gated=1), [a for t in layers for a in t] + head)
    # blob order: w_kqvr, b_kqvr per layer, then the head; every tensor padded to 4 floats; nothing else (no gin_w / gin_b)
    at, want = 0, {}
    for l, (a, b) in enumerate(widths):
        for name, n in (("w_kqvr", 4 * b * a), ("b_kqvr", 4 * b)):
            want[f"conv{l}.{name}"] = at
            at += -(-n // 4) * 4
    for i, t in enumerate(head):
        want[f"head{i // 2}.{'wb'[i % 2]}"] = at
        at += -(-t.size // 4) * 4
    assert layout == want and img.size == at
    for l, (a, b) in enumerate(widths):
        wk, bk, wq, bq, wv, bv, ws, bias = layers[l]
        off = layout[f"conv{l}.w_kqvr"]
        stacked = img[off:off + 4 * b * a].reshape(4 * b, a)
        for blk, w in enumerate((wk, wq, wv, ws)):  # block by block, row for row, as the layer's GEMM reads it
            assert np.array_equal(stacked[blk * b:(blk + 1) * b].view(np.uint32), w.view(np.uint32)), (l, blk)
        off = layout[f"conv{l}.b_kqvr"]
        got = img[off:off + 4 * b].reshape(4, b)
        assert np.array_equal(got.view(np.uint32), np.stack([bk, bq, bv, bias]).view(np.uint32))  # (b_q is b_q: nothing folded)
    for i, t in enumerate(head):
        off = layout[f"head{i // 2}.{'wb'[i % 2]}"]
        assert np.array_equal(img[off:off + t.size], t.ravel())


def test_image_of_a_model_from_models_py(rg_prog, tmp_path):
    """``GNNModel.canonical_params()`` of a seeded model through the builder: the stacked blocks are the model's own tensors."""
    model = make_resgated_model(in_dim=9, hidden=12, layers=2, out_dim=8, pools=("add", "max"), mlp_hidden=MLP_HIDDEN, mlp_layers=1,
                                task_out=MLP_OUT)
    params = [p.numpy() for p in model.canonical_params()]
    assert len(params) == 2 * 8 + 2 * MLP_N
    img, layout = run_gat(rg_prog, tmp_path, _job(GIN, 2, 9, 12, 8, 1, gated=1), params)
    for l, conv in enumerate(model.gnn_convs):
        c = conv.conv
        fo, fi = c.lin_key.weight.shape
        off = layout[f"conv{l}.w_kqvr"]
        stacked = img[off:off + 4 * fo * fi].reshape(4, fo, fi)
        for blk, lin in enumerate((c.lin_key, c.lin_query, c.lin_value, c.lin_skip)):
            assert np.array_equal(stacked[blk], lin.weight.detach().numpy()), (l, blk)
        off = layout[f"conv{l}.b_kqvr"]
        want = np.stack([c.lin_key.bias.detach().numpy(), c.lin_query.bias.detach().numpy(), c.lin_value.bias.detach().numpy(),
                         c.bias.detach().numpy()])
        assert np.array_equal(img[off:off + 4 * fo].reshape(4, fo), want) and np.abs(want[3]).max() > 0


@pytest.mark.parametrize("L,fin,hid,out,skip", [(3, 9, 32, 32, 1), (2, 7, 6, 5, 0)])
def test_gin_blobs_are_what_they_were(prog, rg_prog, tmp_path, L, fin, hid, out, skip):  # noqa: F811
    img, layout, layers, head = build_image(prog, tmp_path, "gin", L, fin, hid, out, skip=skip, seed=7)
    flat = [v for t in layers for v in t.values()] + head
    img2, layout2 = run_gat(rg_prog, tmp_path, _job(GIN, L, fin, hid, out, skip), flat)
    assert img2.tobytes() == img.tobytes() and layout2 == layout


@pytest.mark.parametrize("L,fin,hid,out,heads", [(3, 3, 6, 6, 3), (2, 9, 32, 32, 4)])
def test_plain_transformer_blob_is_what_it_was(tf_prog, rg_prog, tmp_path, L, fin, hid, out, heads):  # noqa: F811
    rng = np.random.default_rng(fin + 1)
    flat = [a for fi, fo in layer_widths(L, fin, hid, out) for a in tf_tensors(rng, fi, fo)] + _head(rng, out)
    tf_job = [GIN, L, fin, hid, out, 1, 0, 0, heads, MLP_N, MLP_HIDDEN, MLP_OUT, POOLS]
    img, layout = run_gat(tf_prog, tmp_path, tf_job, flat)
    img2, layout2 = run_gat(rg_prog, tmp_path, _job(GIN, L, fin, hid, out, 1, tf_heads=heads), flat)
    assert img2.tobytes() == img.tobytes() and layout2 == layout and "conv0.w_kqvr" not in layout
