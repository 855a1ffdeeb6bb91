"""The weight image of a GatedGraphConv model (csrc/gnnb_weights.h: ``build_weight_image`` with a GIN description and
``ggnn_steps``), checked without a GPU by a stand-alone program of its own (tests/weights_host_ggnn_main.cpp, with its own
``main``, built with ``g++`` under the address and undefined-behaviour sanitizers and run as a child process on files -- never
loaded into Python): five tensors per layer; per (layer, step) ``[W_p[t] ; weight_hh]`` with ``W_p[t] = weight_ih @ weight[t]^T``
compared bit for bit with a double-precision fold computed here and rounded once; the step-0 slot holds only the first ``in``
input columns; ``b_ggc = [0 | bias_hh]``, its ``p`` half zeros; ``bias_ih`` raw; no execution-order copy; the head last.  And the
images of a GIN and of a ResGatedGraphConv model through this program are byte for byte what the existing host programs give."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from ggnn_util import make_ggnn_model
from test_weights_host import GIN, build_image, layer_widths, prog, uniform  # noqa: F401  (prog: the fixture)
from test_weights_host_gat import run_gat
from test_weights_host_resgated import rg_prog, rg_tensors  # noqa: F401  (rg_prog: the fixture)

ROOT = Path(__file__).resolve().parent.parent

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def gg_prog(tmp_path_factory):
    exe = tmp_path_factory.mktemp("weights_host_ggnn") / "weights_host_ggnn_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I", str(ROOT / "include"),
                    "-I", str(ROOT / "gnn-builder_amd" / "csrc"), str(ROOT / "tests" / "weights_host_ggnn_main.cpp"), "-o", str(exe)],
                   check=True)
    return exe


POOLS, MLP_N, MLP_HIDDEN, MLP_OUT = 2, 2, 6, 3


def _head(rng, out):
    return [uniform(rng, MLP_HIDDEN, POOLS * out), uniform(rng, MLP_HIDDEN), uniform(rng, MLP_OUT, MLP_HIDDEN), uniform(rng, MLP_OUT)]


def _job(conv, L, fin, hid, out, skip, edge_dim=0, gat_heads=0, tf_heads=0, gated=0, steps=0):
    return [conv, L, fin, hid, out, skip, edge_dim, gat_heads, tf_heads, gated, steps, MLP_N, MLP_HIDDEN, MLP_OUT, POOLS]


def gg_tensors(rng, fo, steps):
    """A layer's five tensors in canonical order: weight [steps, out, out], rnn.weight_ih, rnn.weight_hh, rnn.bias_ih, rnn.bias_hh."""
    return [uniform(rng, steps, fo, fo), uniform(rng, 3 * fo, fo), uniform(rng, 3 * fo, fo), uniform(rng, 3 * fo), uniform(rng, 3 * fo)]


def fold(weight_t, w_ih, w_hh, cols):
    """``[W_p ; weight_hh][:, :cols]`` with ``W_p = weight_ih @ weight_t^T`` accumulated in double, c increasing, rounded once."""
    fo = weight_t.shape[0]
    acc = np.zeros((3 * fo, fo), np.float64)
    for c in range(fo):  # (sequential in c: the order the builder adds in)
        acc += w_ih[:, c].astype(np.float64)[:, None] * weight_t[:, c].astype(np.float64)[None, :]
    return np.concatenate([acc.astype(np.float32)[:, :cols], w_hh[:, :cols]], 0)


def _pad4(n):
    return -(-n // 4) * 4


# (L, in, hidden, out): in < out and in == out, odd widths (sizes that are no multiple of 4 floats are padded), a one-layer model,
# and the shape at which a GIN model gets the stack kernel's execution-order copy -- such a model does not
CASES = [(3, 3, 6, 6), (2, 5, 9, 15), (3, 9, 32, 32), (1, 7, 0, 16), (1, 9, 0, 9), (2, 1, 1, 3)]


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("L,fin,hid,out", CASES)
def test_image_of_a_ggnn_model(gg_prog, tmp_path, L, fin, hid, out, steps):
    rng = np.random.default_rng(100 * fin + steps)
    widths = layer_widths(L, fin, hid, out)
    layers = [gg_tensors(rng, b, steps) for _, b in widths]
    head = _head(rng, out)
    img, layout = run_gat(gg_prog, tmp_path, _job(GIN, L, fin, hid, out, 1, steps=steps), [a for t in layers for a in t] + head)
    # blob order: w_ggc, w_ggc_next (steps > 1), b_ggc, b_ih per layer, then the head; every tensor padded to 4 floats; nothing
    # else (no gin_w / gin_b)
    at, want = 0, {}
    for l, (a, b) in enumerate(widths):
        sizes = [("w_ggc", 6 * b * a)] + ([("w_ggc_next", (steps - 1) * _pad4(6 * b * b))] if steps > 1 else []) + [("b_ggc", 6 * b), ("b_ih", 3 * b)]
        for name, n in sizes:
            want[f"conv{l}.{name}"] = at
            at += _pad4(n)
    for i, t in enumerate(head):
        want[f"head{i // 2}.{'wb'[i % 2]}"] = at
        at += _pad4(t.size)
    assert layout == want and img.size == at
    for l, (a, b) in enumerate(widths):
        weight, w_ih, w_hh, b_ih, b_hh = layers[l]
        off = layout[f"conv{l}.w_ggc"]
        got = img[off:off + 6 * b * a].reshape(6 * b, a)  # step 0: K = the layer's input width, the first `in` columns only
        assert np.array_equal(got.view(np.uint32), fold(weight[0], w_ih, w_hh, a).view(np.uint32)), l
        for t in range(1, steps):
            off = layout[f"conv{l}.w_ggc_next"] + (t - 1) * _pad4(6 * b * b)
            got = img[off:off + 6 * b * b].reshape(6 * b, b)
            assert np.array_equal(got.view(np.uint32), fold(weight[t], w_ih, w_hh, b).view(np.uint32)), (l, t)
            assert not img[off + 6 * b * b:off + _pad4(6 * b * b)].any()
        off = layout[f"conv{l}.b_ggc"]
        assert not img[off:off + 3 * b].any()  # the p block takes no bias: it would be counted once per edge
        assert np.array_equal(img[off + 3 * b:off + 6 * b].view(np.uint32), b_hh.view(np.uint32))
        off = layout[f"conv{l}.b_ih"]
        assert np.array_equal(img[off:off + 3 * b].view(np.uint32), b_ih.view(np.uint32))
    for i, t in enumerate(head):
        off = layout[f"head{i // 2}.{'wb'[i % 2]}"]
        assert np.array_equal(img[off:off + t.size], t.ravel())


def test_the_fold_is_not_the_fp32_product():
    """The comparison above would not see a fold in fp32: on these tensors an fp32 matmul differs from the double fold."""
    rng = np.random.default_rng(5)
    weight, w_ih, w_hh, _, _ = gg_tensors(rng, 32, 1)
    assert not np.array_equal(fold(weight[0], w_ih, w_hh, 32)[:96], w_ih @ weight[0].T)


def test_image_of_a_model_from_models_py(gg_prog, tmp_path):
    """``GNNModel.canonical_params()`` of a seeded model through the builder: the folded blocks are the model's own tensors'."""
    model = make_ggnn_model(in_dim=9, hidden=12, layers=2, out_dim=16, steps=3, pools=("add", "max"), mlp_hidden=MLP_HIDDEN, mlp_layers=1,
                            task_out=MLP_OUT)
    params = [p.numpy() for p in model.canonical_params()]
    assert len(params) == 2 * 5 + 2 * MLP_N
    img, layout = run_gat(gg_prog, tmp_path, _job(GIN, 2, 9, 12, 16, 1, steps=3), params)
    for l, conv in enumerate(model.gnn_convs):
        c = conv.conv
        fo, fi = c.out_channels, c.in_channels
        sd = {k: v.numpy() for k, v in c.state_dict().items()}
        off = layout[f"conv{l}.w_ggc"]
        assert np.array_equal(img[off:off + 6 * fo * fi].reshape(6 * fo, fi), fold(sd["weight"][0], sd["rnn.weight_ih"], sd["rnn.weight_hh"], fi))
        off = layout[f"conv{l}.w_ggc_next"] + _pad4(6 * fo * fo)
        assert np.array_equal(img[off:off + 6 * fo * fo].reshape(6 * fo, fo), fold(sd["weight"][2], sd["rnn.weight_ih"], sd["rnn.weight_hh"], fo))
        off = layout[f"conv{l}.b_ih"]
        assert np.array_equal(img[off:off + 3 * fo], sd["rnn.bias_ih"]) and np.abs(sd["rnn.bias_ih"]).max() > 0


@pytest.mark.parametrize("L,fin,hid,out,skip", [(3, 9, 32, 32, 1), (2, 7, 6, 5, 0)])
def test_gin_blobs_are_what_they_were(prog, gg_prog, tmp_path, L, fin, hid, out, skip):  # noqa: F811
    img, layout, layers, head = build_image(prog, tmp_path, "gin", L, fin, hid, out, skip=skip, seed=7)
    flat = [v for t in layers for v in t.values()] + head
    img2, layout2 = run_gat(gg_prog, tmp_path, _job(GIN, L, fin, hid, out, skip), flat)
    assert img2.tobytes() == img.tobytes() and layout2 == layout


@pytest.mark.parametrize("L,fin,hid,out", [(3, 3, 6, 6), (2, 9, 32, 32)])
def test_resgated_blob_is_what_it_was(rg_prog, gg_prog, tmp_path, L, fin, hid, out):  # noqa: F811
    rng = np.random.default_rng(fin + 1)
    flat = [a for fi, fo in layer_widths(L, fin, hid, out) for a in rg_tensors(rng, fi, fo)] + _head(rng, out)
    rg_job = [GIN, L, fin, hid, out, 1, 0, 0, 0, 1, MLP_N, MLP_HIDDEN, MLP_OUT, POOLS]
    img, layout = run_gat(rg_prog, tmp_path, rg_job, flat)
    img2, layout2 = run_gat(gg_prog, tmp_path, _job(GIN, L, fin, hid, out, 1, gated=1), flat)
    assert img2.tobytes() == img.tobytes() and layout2 == layout and "conv0.w_ggc" not in layout
