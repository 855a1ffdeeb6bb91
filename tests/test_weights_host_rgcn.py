"""The weight image of an RGCNConv model (csrc/gnnb_weights.h: ``build_weight_image`` with a GIN description and
``rgcn_relations``), checked without a GPU by a stand-alone program of its own (tests/weights_host_rgcn_main.cpp, with its own
``main``, built with ``g++`` under the address and undefined-behaviour sanitizers and run as a child process on files -- never
loaded into Python): three tensors per layer; ``w_rgcn = [weight[0]^T ; .. ; weight[R-1]^T ; root^T]`` compared bit for bit with
the transposes (no arithmetic); ``b_rgcn``'s relation blocks zeros, its last block ``bias``; odd widths padded to 4 floats; no
execution-order copy; the head last.  And the images of a GIN and of a GatedGraphConv model through this program are byte for
byte what the existing host programs give."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rgcn_util import make_rgcn_model
from test_weights_host import GIN, build_image, layer_widths, prog, uniform  # noqa: F401  (prog: the fixture)
from test_weights_host_gat import run_gat
from test_weights_host_ggnn import gg_prog, gg_tensors  # noqa: F401  (gg_prog: the fixture)
from test_weights_host_ggnn import _job as gg_job

ROOT = Path(__file__).resolve().parent.parent

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def rgcn_prog(tmp_path_factory):
    exe = tmp_path_factory.mktemp("weights_host_rgcn") / "weights_host_rgcn_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I", str(ROOT / "include"),
                    "-I", str(ROOT / "gnn-builder_amd" / "csrc"), str(ROOT / "tests" / "weights_host_rgcn_main.cpp"), "-o", str(exe)],
                   check=True)
    return exe


POOLS, MLP_N, MLP_HIDDEN, MLP_OUT = 2, 2, 6, 3


def _head(rng, out):
    return [uniform(rng, MLP_HIDDEN, POOLS * out), uniform(rng, MLP_HIDDEN), uniform(rng, MLP_OUT, MLP_HIDDEN), uniform(rng, MLP_OUT)]


def _job(conv, L, fin, hid, out, skip, edge_dim=0, gat_heads=0, tf_heads=0, gated=0, steps=0, relations=0):
    return [conv, L, fin, hid, out, skip, edge_dim, gat_heads, tf_heads, gated, steps, relations, MLP_N, MLP_HIDDEN, MLP_OUT, POOLS]


def rgcn_tensors(rng, fi, fo, relations):
    """A layer's three tensors in canonical order: weight [R, in, out], root [in, out], bias [out]."""
    return [uniform(rng, relations, fi, fo), uniform(rng, fi, fo), uniform(rng, fo)]


def stacked(weight, root):
    """``[weight[0]^T ; .. ; weight[R-1]^T ; root^T]`` [(R + 1) out, in]: transposes, no arithmetic."""
    return np.concatenate([w.T for w in weight] + [root.T], 0)


def _pad4(n):
    return -(-n // 4) * 4


# (L, in, hidden, out): in < out, in > out, odd widths (sizes that are no multiple of 4 floats are padded), a one-layer model, and
# the shape at which a GIN model gets the stack kernel's execution-order copy -- such a model does not
CASES = [(3, 3, 6, 6), (2, 5, 9, 15), (3, 9, 32, 32), (1, 7, 0, 16), (2, 9, 5, 3), (2, 1, 1, 3)]


@pytest.mark.parametrize("relations", [1, 3, 8])
@pytest.mark.parametrize("L,fin,hid,out", CASES)
def test_image_of_an_rgcn_model(rgcn_prog, tmp_path, L, fin, hid, out, relations):
    rng = np.random.default_rng(100 * fin + relations)
    widths = layer_widths(L, fin, hid, out)
    layers = [rgcn_tensors(rng, a, b, relations) for a, b in widths]
    head = _head(rng, out)
    img, layout = run_gat(rgcn_prog, tmp_path, _job(GIN, L, fin, hid, out, 1, relations=relations), [a for t in layers for a in t] + head)
    # blob order: w_rgcn, b_rgcn per layer, then the head; every tensor padded to 4 floats; nothing else (no gin_w / gin_b)
    at, want = 0, {}
    for l, (a, b) in enumerate(widths):
        for name, n in (("w_rgcn", (relations + 1) * b * a), ("b_rgcn", (relations + 1) * b)):
            want[f"conv{l}.{name}"] = at
            at += _pad4(n)
    for i, t in enumerate(head):
        want[f"head{i // 2}.{'wb'[i % 2]}"] = at
        at += _pad4(t.size)
    assert layout == want and img.size == at
    for l, (a, b) in enumerate(widths):
        weight, root, bias = layers[l]
        off, n = layout[f"conv{l}.w_rgcn"], (relations + 1) * b * a
        got = img[off:off + n].reshape((relations + 1) * b, a)
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(stacked(weight, root)).view(np.uint32)), l
        assert not img[off + n:off + _pad4(n)].any()  # the padding
        off, n = layout[f"conv{l}.b_rgcn"], (relations + 1) * b
        assert not img[off:off + relations * b].any()  # the relation blocks take no bias: it would be counted once per edge
        assert np.array_equal(img[off + relations * b:off + n].view(np.uint32), bias.view(np.uint32))
        assert not img[off + n:off + _pad4(n)].any()
    for i, t in enumerate(head):
        off = layout[f"head{i // 2}.{'wb'[i % 2]}"]
        assert np.array_equal(img[off:off + t.size], t.ravel())


def test_image_of_a_model_from_models_py(rgcn_prog, tmp_path):
    """``GNNModel.canonical_params()`` of a seeded model through the builder: the stacked blocks are the model's own tensors',
    and block ``r`` applied as ``nn.Linear`` does is ``x @ weight[r]``."""
    model = make_rgcn_model(in_dim=9, hidden=12, layers=2, out_dim=15, relations=3, pools=("add", "max"), mlp_hidden=MLP_HIDDEN, mlp_layers=1,
                            task_out=MLP_OUT)
    params = [p.numpy() for p in model.canonical_params()]
    assert len(params) == 2 * 3 + 2 * MLP_N
    img, layout = run_gat(rgcn_prog, tmp_path, _job(GIN, 2, 9, 12, 15, 1, relations=3), params)
    x = np.random.default_rng(0).uniform(-1, 1, (5, 12)).astype(np.float32)
    for l, conv in enumerate(model.gnn_convs):
        c = conv.conv
        fo, fi = c.out_channels, c.in_channels
        sd = {k: v.numpy() for k, v in c.state_dict().items()}
        off = layout[f"conv{l}.w_rgcn"]
        w = img[off:off + 4 * fo * fi].reshape(4 * fo, fi)
        assert np.array_equal(w, stacked(sd["weight"], sd["root"]))
        assert np.array_equal(x[:, :fi] @ w[2 * fo:3 * fo].T, x[:, :fi] @ sd["weight"][2])
        off = layout[f"conv{l}.b_rgcn"]
        assert np.array_equal(img[off + 3 * fo:off + 4 * fo], sd["bias"]) and np.abs(sd["bias"]).max() > 0


@pytest.mark.parametrize("L,fin,hid,out,skip", [(3, 9, 32, 32, 1), (2, 7, 6, 5, 0)])
def test_gin_blobs_are_what_they_were(prog, rgcn_prog, tmp_path, L, fin, hid, out, skip):  # noqa: F811
    img, layout, layers, head = build_image(prog, tmp_path, "gin", L, fin, hid, out, skip=skip, seed=7)
    flat = [v for t in layers for v in t.values()] + head
    img2, layout2 = run_gat(rgcn_prog, tmp_path, _job(GIN, L, fin, hid, out, skip), flat)
    assert img2.tobytes() == img.tobytes() and layout2 == layout


@pytest.mark.parametrize("L,fin,hid,out,steps", [(3, 3, 6, 6, 1), (2, 9, 32, 32, 3)])
def test_ggnn_blob_is_what_it_was(gg_prog, rgcn_prog, tmp_path, L, fin, hid, out, steps):  # noqa: F811
    rng = np.random.default_rng(fin + 1)
    flat = [a for _, fo in layer_widths(L, fin, hid, out) for a in gg_tensors(rng, fo, steps)] + _head(rng, out)
    img, layout = run_gat(gg_prog, tmp_path, gg_job(GIN, L, fin, hid, out, 1, steps=steps), flat)
    img2, layout2 = run_gat(rgcn_prog, tmp_path, _job(GIN, L, fin, hid, out, 1, steps=steps), flat)
    assert img2.tobytes() == img.tobytes() and layout2 == layout and "conv0.w_rgcn" not in layout
