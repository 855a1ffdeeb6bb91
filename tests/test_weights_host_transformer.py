"""The weight image of a TransformerConv model (csrc/gnnb_weights.h: ``build_weight_image`` with a GIN description and
``tf_heads > 0``), checked without a GPU by a stand-alone program of its own (tests/weights_host_transformer_main.cpp, with its
own ``main``, built with ``g++`` under the address and undefined-behaviour sanitizers and run as a child process on files -- never
loaded into Python): eight tensors per layer in PyG's order (key, query, value, skip); ``w_qkvr = [W_q ; W_k ; W_v ; W_skip]``
[4 out, in] and ``b_qkvr`` stacked row for row; none of GIN's slots and no execution-order copy for the stack kernel, whatever the
widths; the head last.  And the images of a GIN, a GINE and a GATv2 model through the builder's full argument list are byte for
byte what the existing host programs (which do not name the new argument) give, which the existing tests hold to their layouts.
Everything bit for bit."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_weights_host import GCN, GIN, build_image, layer_widths, prog, uniform  # noqa: F401  (prog: the fixture)
from test_weights_host_gat import gat_prog, gat_tensors, run_gat  # noqa: F401  (gat_prog: the fixture)

ROOT = Path(__file__).resolve().parent.parent

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def tf_prog(tmp_path_factory):
    exe = tmp_path_factory.mktemp("weights_host_transformer") / "weights_host_transformer_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I", str(ROOT / "include"),
                    "-I", str(ROOT / "gnn-builder_amd" / "csrc"), str(ROOT / "tests" / "weights_host_transformer_main.cpp"), "-o", str(exe)],
                   check=True)
    return exe


def tf_tensors(rng, fi, fo):
    """A layer's eight tensors in canonical order (include/gnnb_transformer.h): key, query, value, skip -- weight, bias each."""
    return [t for _ in range(4) for t in (uniform(rng, fo, fi), uniform(rng, fo))]


POOLS, MLP_N, MLP_HIDDEN, MLP_OUT = 2, 2, 6, 3


def _head(rng, out):
    return [uniform(rng, MLP_HIDDEN, POOLS * out), uniform(rng, MLP_HIDDEN), uniform(rng, MLP_OUT, MLP_HIDDEN), uniform(rng, MLP_OUT)]


def _job(conv, L, fin, hid, out, skip, edge_dim=0, gat_heads=0, tf_heads=0):
    return [conv, L, fin, hid, out, skip, edge_dim, gat_heads, tf_heads, MLP_N, MLP_HIDDEN, MLP_OUT, POOLS]


# (L, in, hidden, out, heads): odd widths (sizes that are no multiple of 4 floats are padded), a one-layer model, and the shapes at
# which a GIN model gets the stack kernel's execution-order copy (hidden 32 / 128, out % 4 == 0) -- a TransformerConv model does not
CASES = [(3, 3, 6, 6, 3), (1, 7, 0, 9, 1), (2, 9, 32, 32, 4), (3, 11, 128, 24, 2)]


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("L,fin,hid,out,heads", CASES)
def test_image_of_a_transformer_model(tf_prog, tmp_path, L, fin, hid, out, heads, skip):
    rng = np.random.default_rng(100 * fin + skip)
    widths = layer_widths(L, fin, hid, out)
    layers = [tf_tensors(rng, a, b) for a, b in widths]
    head = _head(rng, out)
    img, layout = run_gat(tf_prog, tmp_path, _job(GIN, L, fin, hid, out, skip, tf_heads=heads), [a for t in layers for a in t] + head)
    # blob order: w_qkvr, b_qkvr per layer, then the head; every tensor padded to 4 floats; nothing else (no gin_w / gin_b)
    at, want = 0, {}
    for l, (a, b) in enumerate(widths):
        for name, n in (("w_qkvr", 4 * b * a), ("b_qkvr", 4 * b)):
            want[f"conv{l}.{name}"] = at
            at += -(-n // 4) * 4
    for i, t in enumerate(head):
        want[f"head{i // 2}.{'wb'[i % 2]}"] = at
        at += -(-t.size // 4) * 4
    assert layout == want and img.size == at
    for l, (a, b) in enumerate(widths):
        wk, bk, wq, bq, wv, bv, ws, bs = layers[l]
        for name, ref in (("w_qkvr", np.concatenate([wq, wk, wv, ws], 0)), ("b_qkvr", np.concatenate([bq, bk, bv, bs]))):
            off = layout[f"conv{l}.{name}"]
            assert np.array_equal(img[off:off + ref.size], ref.ravel()), (l, name)
            pad = -ref.size % 4
            assert not img[off + ref.size:off + ref.size + pad].any()
        # the stacked matrix as the layer's GEMM reads it, row for row: block 0 is W_q, 1 W_k, 2 W_v, 3 W_skip -- and the bias
        off = layout[f"conv{l}.w_qkvr"]
        stacked = img[off:off + 4 * b * a].reshape(4 * b, a)
        for blk, w in enumerate((wq, wk, wv, ws)):
            for o in range(b):
                assert np.array_equal(stacked[blk * b + o], w[o]), (l, blk, o)
        off = layout[f"conv{l}.b_qkvr"]
        assert np.array_equal(img[off:off + 4 * b].reshape(4, b), np.stack([bq, bk, bv, bs]))
    for i, t in enumerate(head):
        off = layout[f"head{i // 2}.{'wb'[i % 2]}"]
        assert np.array_equal(img[off:off + t.size], t.ravel())


# (conv, L, in, hidden, out, skip): a GIN model with the execution-order copy (gin_w, gin_b in its layout) and without, a GINE model
OTHERS = [("gin", 3, 9, 32, 32, 1), ("gin", 2, 7, 6, 5, 0), ("gine", 3, 9, 32, 32, 1), ("gine", 2, 5, 12, 7, 0)]


@pytest.mark.parametrize("conv,L,fin,hid,out,skip", OTHERS)
def test_gin_and_gine_blobs_are_what_they_were(prog, tf_prog, tmp_path, conv, L, fin, hid, out, skip):  # noqa: F811
    """The same tensors through the existing host program (``build_weight_image(d, edge_dim, params)``: the call of every model
    that existed) and through this file's with ``gat_heads = tf_heads = 0`` spelled out: byte-identical images, equal layouts."""
    img, layout, layers, head = build_image(prog, tmp_path, conv, L, fin, hid, out, skip=skip, seed=7)
    assert ("gin_w" in layout) == (conv == "gin" and hid == 32)
    flat = [v for t in layers for v in t.values()] + head
    img2, layout2 = run_gat(tf_prog, tmp_path, _job(GIN, L, fin, hid, out, skip, edge_dim=3 if conv == "gine" else 0), flat)
    assert img2.tobytes() == img.tobytes() and layout2 == layout
    # canonical tensors at their offsets, back to back from the blob's start, padded to 4 floats: the parent's layout
    at = 0
    for l, t in enumerate(layers):
        for name, v in t.items():
            assert layout[f"conv{l}.{name}"] == at and np.array_equal(img[at:at + v.size], v.ravel())
            at += -(-v.size // 4) * 4


@pytest.mark.parametrize("L,fin,hid,out,heads", [(3, 3, 6, 6, 3), (2, 9, 32, 32, 4)])
def test_gatv2_blob_is_what_it_was(gat_prog, tf_prog, tmp_path, L, fin, hid, out, heads):  # noqa: F811
    rng = np.random.default_rng(fin)
    layers = [gat_tensors(rng, a, b, heads) for a, b in layer_widths(L, fin, hid, out)]
    flat = [a for t in layers for a in t] + _head(rng, out)
    img, layout = run_gat(gat_prog, tmp_path, [L, fin, hid, out, 1, heads, MLP_N, MLP_HIDDEN, MLP_OUT, POOLS], flat)
    img2, layout2 = run_gat(tf_prog, tmp_path, _job(GCN, L, fin, hid, out, 1, gat_heads=heads), flat)
    assert img2.tobytes() == img.tobytes() and layout2 == layout
    assert layout["conv0.w_lr"] == 0 and "conv0.w_qkvr" not in layout
