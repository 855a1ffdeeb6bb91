"""The weight image of a TransformerConv model with edge features (csrc/gnnb_weights.h: ``build_weight_image`` with a GIN
description, ``tf_heads > 0`` and ``edge_dim > 0``), checked without a GPU by a stand-alone program of its own
(tests/weights_host_transformer_edge_main.cpp, with its own ``main``, built with ``g++`` under the address and undefined-behaviour
sanitizers and run as a child process on files -- never loaded into Python): nine tensors per layer; ``w_qkvre = [W_q ; W_k ; W_v ;
W_skip ; W_qe ; 0]`` with ``W_qe[h d + t] = sum_c W_e[h C + c][t] W_q[h C + c]`` and ``b_qkvre`` likewise, the folded block held bit
for bit to a float64 evaluation written here (``c`` increasing, rounded once), zero rows up to a multiple of 4; ``w_edge`` raw
behind them; the head last.  And the images of a GIN, GINE, GATv2, GATv2E and plain TransformerConv model through this program are
byte for byte what the existing host programs give.  Everything bit for bit."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_weights_host import GCN, GIN, build_image, layer_widths, prog, uniform  # noqa: F401  (prog: the fixture)
from test_weights_host_gat import gat_prog, gat_tensors, run_gat  # noqa: F401  (gat_prog: the fixture)
from test_weights_host_gat_edge import gat_edge_prog  # noqa: F401  (the fixture)
from test_weights_host_transformer import tf_prog, tf_tensors  # noqa: F401  (tf_prog: the fixture)

ROOT = Path(__file__).resolve().parent.parent

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def tfe_prog(tmp_path_factory):
    exe = tmp_path_factory.mktemp("weights_host_transformer_edge") / "weights_host_transformer_edge_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I", str(ROOT / "include"),
                    "-I", str(ROOT / "gnn-builder_amd" / "csrc"), str(ROOT / "tests" / "weights_host_transformer_edge_main.cpp"), "-o", str(exe)],
                   check=True)
    return exe


POOLS, MLP_N, MLP_HIDDEN, MLP_OUT = 2, 2, 6, 3


def _head(rng, out):
    return [uniform(rng, MLP_HIDDEN, POOLS * out), uniform(rng, MLP_HIDDEN), uniform(rng, MLP_OUT, MLP_HIDDEN), uniform(rng, MLP_OUT)]


def _job(conv, L, fin, hid, out, skip, edge_dim=0, gat_heads=0, tf_heads=0):
    return [conv, L, fin, hid, out, skip, edge_dim, gat_heads, tf_heads, MLP_N, MLP_HIDDEN, MLP_OUT, POOLS]


def fold64(wq, bq, we, heads):
    """(W_qe [heads d, in], b_qe [heads d]): per head and attribute the sum over the head's columns, ``c`` increasing, of
    ``W_e[h C + c][t] * W_q[h C + c][:]`` accumulated in float64 (a product of two floats is exact there) and rounded to fp32 once."""
    fo, fi = wq.shape
    d, C = we.shape[1], fo // heads
    w, b = np.zeros((heads * d, fi), np.float32), np.zeros(heads * d, np.float32)
    for h in range(heads):
        for t in range(d):
            acc, ab = np.zeros(fi, np.float64), np.float64(0.0)
            for c in range(C):
                e = np.float64(we[h * C + c, t])
                acc = acc + e * wq[h * C + c].astype(np.float64)
                ab = ab + e * np.float64(bq[h * C + c])
            w[h * d + t], b[h * d + t] = acc.astype(np.float32), np.float32(ab)
    return w, b


# (L, in, hidden, out, heads, edge_dim): heads * edge_dim = 3, 9, 16, 48 and 128 (one, three and no padding rows), odd widths, a
# one-layer model, and the shape at which a GIN model gets the stack kernel's execution-order copy -- such a model does not
CASES = [(3, 3, 6, 6, 3, 1), (2, 5, 9, 15, 3, 3), (2, 9, 32, 32, 4, 4), (3, 11, 24, 12, 3, 16), (1, 7, 0, 16, 8, 16), (1, 7, 0, 9, 1, 3)]


def test_the_cases_cover_the_padding():
    assert {h * d for *_, h, d in CASES} == {3, 9, 16, 48, 128}


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("L,fin,hid,out,heads,ed", CASES)
def test_image_of_a_transformer_model_with_edge_features(tfe_prog, tmp_path, L, fin, hid, out, heads, ed, skip):
    rng = np.random.default_rng(100 * fin + skip)
    widths = layer_widths(L, fin, hid, out)
    layers = [tf_tensors(rng, a, b) + [uniform(rng, b, ed)] for a, b in widths]
    head = _head(rng, out)
    img, layout = run_gat(tfe_prog, tmp_path, _job(GIN, L, fin, hid, out, skip, edge_dim=ed, tf_heads=heads), [a for t in layers for a in t] + head)
    rq = -(-heads * ed // 4) * 4  # the folded block's rows, padded to whole 16-byte pieces of the GEMM's output row
    # blob order: w_qkvre, b_qkvre, w_edge per layer, then the head; every tensor padded to 4 floats; nothing else
    at, want = 0, {}
    for l, (a, b) in enumerate(widths):
        for name, n in (("w_qkvre", (4 * b + rq) * a), ("b_qkvre", 4 * b + rq), ("w_edge", b * ed)):
            want[f"conv{l}.{name}"] = at
            at += -(-n // 4) * 4
    for i, t in enumerate(head):
        want[f"head{i // 2}.{'wb'[i % 2]}"] = at
        at += -(-t.size // 4) * 4
    assert layout == want and img.size == at
    for l, (a, b) in enumerate(widths):
        wk, bk, wq, bq, wv, bv, ws, bs, we = layers[l]
        off = layout[f"conv{l}.w_qkvre"]
        stacked = img[off:off + (4 * b + rq) * a].reshape(4 * b + rq, a)
        for blk, w in enumerate((wq, wk, wv, ws)):  # row for row, as the layer's GEMM reads it
            for o in range(b):
                assert np.array_equal(stacked[blk * b + o], w[o]), (l, blk, o)
        wqe, bqe = fold64(wq, bq, we, heads)
        assert np.array_equal(stacked[4 * b:4 * b + heads * ed].view(np.uint32), wqe.view(np.uint32)), l  # bit for bit
        assert not stacked[4 * b + heads * ed:].any() and stacked[4 * b + heads * ed:].shape[0] == rq - heads * ed
        off = layout[f"conv{l}.b_qkvre"]
        bias = img[off:off + 4 * b + rq]
        assert np.array_equal(bias[:4 * b].reshape(4, b), np.stack([bq, bk, bv, bs]))
        assert np.array_equal(bias[4 * b:4 * b + heads * ed].view(np.uint32), bqe.view(np.uint32)) and not bias[4 * b + heads * ed:].any()
        # the fold is what it claims: x -> qe equals W_e[h]^T q[h] (float64, to rounding of the fp32 fold)
        x = rng.uniform(-1, 1, (5, a))
        q3 = (x @ wq.astype(np.float64).T + bq).reshape(5, heads, b // heads)
        direct = np.einsum("hcd,nhc->nhd", we.astype(np.float64).reshape(heads, b // heads, ed), q3).reshape(5, heads * ed)
        assert np.abs(x @ wqe.astype(np.float64).T + bqe - direct).max() <= 1e-5 * max(1.0, np.abs(direct).max())
        # w_edge raw, as the kernel's epilogue reads it: row c of [out, edge_dim] at row stride edge_dim
        off = layout[f"conv{l}.w_edge"]
        assert np.array_equal(img[off:off + b * ed].reshape(b, ed), we)
        assert not img[off + b * ed:off + b * ed + (-b * ed % 4)].any()
    for i, t in enumerate(head):
        off = layout[f"head{i // 2}.{'wb'[i % 2]}"]
        assert np.array_equal(img[off:off + t.size], t.ravel())


# (conv, L, in, hidden, out, skip): a GIN model with the execution-order copy (gin_w, gin_b in its layout) and without, a GINE model
OTHERS = [("gin", 3, 9, 32, 32, 1), ("gin", 2, 7, 6, 5, 0), ("gine", 3, 9, 32, 32, 1), ("gine", 2, 5, 12, 7, 0)]


@pytest.mark.parametrize("conv,L,fin,hid,out,skip", OTHERS)
def test_gin_and_gine_blobs_are_what_they_were(prog, tfe_prog, tmp_path, conv, L, fin, hid, out, skip):  # noqa: F811
    img, layout, layers, head = build_image(prog, tmp_path, conv, L, fin, hid, out, skip=skip, seed=7)
    flat = [v for t in layers for v in t.values()] + head
    img2, layout2 = run_gat(tfe_prog, tmp_path, _job(GIN, L, fin, hid, out, skip, edge_dim=3 if conv == "gine" else 0), flat)
    assert img2.tobytes() == img.tobytes() and layout2 == layout


@pytest.mark.parametrize("L,fin,hid,out,heads", [(3, 3, 6, 6, 3), (2, 9, 32, 32, 4)])
def test_gatv2_and_gatv2e_blobs_are_what_they_were(gat_prog, gat_edge_prog, tfe_prog, tmp_path, L, fin, hid, out, heads):  # noqa: F811
    rng = np.random.default_rng(fin)
    layers = [gat_tensors(rng, a, b, heads) + [uniform(rng, b, 3)] for a, b in layer_widths(L, fin, hid, out)]
    head = _head(rng, out)
    flat = [a for t in layers for a in t[:6]] + head
    img, layout = run_gat(gat_prog, tmp_path, [L, fin, hid, out, 1, heads, MLP_N, MLP_HIDDEN, MLP_OUT, POOLS], flat)
    img2, layout2 = run_gat(tfe_prog, tmp_path, _job(GCN, L, fin, hid, out, 1, gat_heads=heads), flat)
    assert img2.tobytes() == img.tobytes() and layout2 == layout
    flat = [a for t in layers for a in t] + head
    img, layout = run_gat(gat_edge_prog, tmp_path, [L, fin, hid, out, 1, heads, 3, MLP_N, MLP_HIDDEN, MLP_OUT, POOLS], flat)
    img2, layout2 = run_gat(tfe_prog, tmp_path, _job(GCN, L, fin, hid, out, 1, edge_dim=3, gat_heads=heads), flat)
    assert img2.tobytes() == img.tobytes() and layout2 == layout and "conv0.w_edge" in layout and "conv0.w_qkvre" not in layout


@pytest.mark.parametrize("L,fin,hid,out,heads", [(3, 3, 6, 6, 3), (2, 9, 32, 32, 4)])
def test_plain_transformer_blob_is_what_it_was(tf_prog, tfe_prog, tmp_path, L, fin, hid, out, heads):  # noqa: F811
    rng = np.random.default_rng(fin + 1)
    flat = [a for fi, fo in layer_widths(L, fin, hid, out) for a in tf_tensors(rng, fi, fo)] + _head(rng, out)
    img, layout = run_gat(tf_prog, tmp_path, _job(GIN, L, fin, hid, out, 1, tf_heads=heads), flat)
    img2, layout2 = run_gat(tfe_prog, tmp_path, _job(GIN, L, fin, hid, out, 1, tf_heads=heads), flat)
    assert img2.tobytes() == img.tobytes() and layout2 == layout
    assert "conv0.w_qkvr" in layout and "conv0.w_qkvre" not in layout and "conv0.w_edge" not in layout
