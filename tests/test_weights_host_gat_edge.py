"""The weight image of a GATv2 model with edge features (csrc/gnnb_weights.h: ``build_weight_image`` with a GCN description,
``gat_heads > 0`` and ``edge_dim > 0``), checked without a GPU by a stand-alone program of its own
(tests/weights_host_gat_edge_main.cpp, with its own ``main``, built with ``g++`` under the address and undefined-behaviour
sanitizers and run as a child process on files -- never loaded into Python): seven tensors per layer; ``w_edge`` [out, edge_dim]
sits at its slot behind ``gat_bias``, raw and padded like the others; the other slots and the head are what the model without edge
features has; with ``edge_dim = 0`` the program gives that model's blob, bit for bit.  Everything bit for bit."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_weights_host import layer_widths, uniform
from test_weights_host_gat import gat_tensors, run_gat

ROOT = Path(__file__).resolve().parent.parent

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def gat_edge_prog(tmp_path_factory):
    exe = tmp_path_factory.mktemp("weights_host_gat_edge") / "weights_host_gat_edge_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I", str(ROOT / "include"),
                    "-I", str(ROOT / "gnn-builder_amd" / "csrc"), str(ROOT / "tests" / "weights_host_gat_edge_main.cpp"), "-o", str(exe)], check=True)
    return exe


# (L, in, hidden, out, heads, edge_dim): odd widths (sizes that are no multiple of 4 floats are padded) at every edge_dim of the
# kernel tests, a one-layer model, and the 2-layer shape with hidden % 16 == 0 at which a GCN model gets the stack kernel's
# fragment copy -- such a model does not
CASES = [(3, 3, 6, 6, 3, 1), (1, 7, 0, 9, 1, 3), (2, 9, 32, 32, 4, 4), (3, 11, 130, 24, 2, 16), (2, 5, 9, 15, 3, 3)]


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("L,fin,hid,out,heads,ed", CASES)
def test_image_of_a_gatv2_model_with_edge_features(gat_edge_prog, tmp_path, L, fin, hid, out, heads, ed, skip):
    rng = np.random.default_rng(100 * fin + skip)
    widths = layer_widths(L, fin, hid, out)
    layers = [gat_tensors(rng, a, b, heads) + [uniform(rng, b, ed)] for a, b in widths]
    pools, mlp_n, mlp_hidden, mlp_out = 2, 2, 6, 3
    head = [uniform(rng, mlp_hidden, pools * out), uniform(rng, mlp_hidden), uniform(rng, mlp_out, mlp_hidden), uniform(rng, mlp_out)]
    job = [L, fin, hid, out, skip, heads, ed, mlp_n, mlp_hidden, mlp_out, pools]
    img, layout = run_gat(gat_edge_prog, tmp_path, job, [a for t in layers for a in t] + head)
    # blob order: w_lr, b_lr, att, gat_bias, w_edge per layer, then the head; every tensor padded to 4 floats; nothing else
    at, want = 0, {}
    for l, (a, b) in enumerate(widths):
        for name, n in (("w_lr", 2 * b * a), ("b_lr", 2 * b), ("att", b), ("gat_bias", b), ("w_edge", b * ed)):
            want[f"conv{l}.{name}"] = at
            at += -(-n // 4) * 4
    for i, t in enumerate(head):
        want[f"head{i // 2}.{'wb'[i % 2]}"] = at
        at += -(-t.size // 4) * 4
    assert layout == want and img.size == at
    for l, (a, b) in enumerate(widths):
        wl, bl, wr, br, att, bias, we = layers[l]
        for name, ref in (("w_lr", np.concatenate([wl, wr], 0)), ("b_lr", np.concatenate([bl, br])), ("att", att.reshape(-1)), ("gat_bias", bias),
                          ("w_edge", we)):
            off = layout[f"conv{l}.{name}"]
            assert np.array_equal(img[off:off + ref.size], ref.ravel()), (l, name)
            pad = -ref.size % 4
            assert not img[off + ref.size:off + ref.size + pad].any()
        # w_edge as the kernel reads it: row c of [out, edge_dim] at row stride edge_dim
        off = layout[f"conv{l}.w_edge"]
        assert np.array_equal(img[off:off + b * ed].reshape(b, ed), we)
    for i, t in enumerate(head):
        off = layout[f"head{i // 2}.{'wb'[i % 2]}"]
        assert np.array_equal(img[off:off + t.size], t.ravel())
    # the same model without its lin_edge tensors (edge_dim 0): every other slot holds the same floats, and the blob is the one
    # tests/weights_host_gat_main.cpp's program gives (tests/test_weights_host_gat.py holds that one to its layout)
    plain_dir = tmp_path / "plain"
    plain_dir.mkdir()
    job0 = [L, fin, hid, out, skip, heads, 0, mlp_n, mlp_hidden, mlp_out, pools]
    img0, layout0 = run_gat(gat_edge_prog, plain_dir, job0, [a for t in layers for a in t[:6]] + head)
    assert not [k for k in layout0 if k.endswith("w_edge")] and set(layout0) == {k for k in layout if not k.endswith("w_edge")}
    for name, off0 in layout0.items():
        ends = sorted(v for v in list(layout0.values()) + [img0.size] if v > off0)[0]
        off = layout[name]
        assert np.array_equal(img0[off0:ends], img[off:off + ends - off0]), name
