"""The weight image of a GAT (v1) model with edge features (csrc/gnnb_weights.h: ``build_weight_image`` with a GCN description,
``gat1_heads > 0`` and ``edge_dim > 0``), checked without a GPU by a stand-alone program of its own
(tests/weights_host_gatconv_edge_main.cpp, with its own ``main``, built with ``g++`` under the address and undefined-behaviour
sanitizers and run as a child process on files -- never loaded into Python): six tensors per layer; ``w_gat`` and ``gat_bias``
exactly the plain GAT model's of the same tensors; one more derived slot ``a_edge`` [heads, roundup4(edge_dim)] whose rows are
summed in double and rounded once, its pad columns zero; the head last.  Everything bit for bit."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_weights_host import layer_widths, uniform

ROOT = Path(__file__).resolve().parent.parent

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = tmp_path_factory.mktemp("weights_host_gatconv_edge") / "weights_host_gatconv_edge_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I", str(ROOT / "include"),
                    "-I", str(ROOT / "gnn-builder_amd" / "csrc"), str(ROOT / "tests" / "weights_host_gatconv_edge_main.cpp"), "-o", str(exe)],
                   check=True)
    return exe


def run(prog, tmp_path, job, tensors):
    """One child process -> (the image's floats, the layout dict)."""
    tensors = [np.ascontiguousarray(t, dtype=np.float32) for t in tensors]
    (tmp_path / "job.txt").write_text(" ".join(str(v) for v in list(job) + [len(tensors)] + [t.size for t in tensors]))
    (tmp_path / "in.bin").write_bytes(b"".join(t.tobytes() for t in tensors))
    r = subprocess.run([str(prog), str(tmp_path / "job.txt"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(tmp_path / "out.txt")],
                       capture_output=True, text=True)
    report = r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in report and "runtime error" not in report and r.returncode == 0, (job, r.returncode, report)
    layout = {name: int(off) for name, off in (line.split() for line in (tmp_path / "out.txt").read_text().splitlines())}
    return np.fromfile(tmp_path / "out.bin", dtype=np.float32), layout


def layer_tensors(rng, fi, fo, heads, d):
    """A layer's six tensors in canonical order (include/gnnb_gatconv_edge.h): GAT v1's four, att_edge, lin_edge.weight."""
    c = fo // heads
    return [uniform(rng, fo, fi), uniform(rng, 1, heads, c), uniform(rng, 1, heads, c), uniform(rng, fo), uniform(rng, 1, heads, c),
            uniform(rng, fo, d)]


def fold_edge(w_edge, att_edge, heads):
    """[heads, d]: row h = sum_c att_edge[h, c] * W_e[h C + c, :] in float64, c increasing, rounded to fp32 once."""
    fo, d = w_edge.shape
    c = fo // heads
    att = att_edge.reshape(heads, c).astype(np.float64)
    w64 = w_edge.astype(np.float64)
    rows = np.zeros((heads, d), np.float64)
    for h in range(heads):
        for k in range(c):
            rows[h] += att[h, k] * w64[h * c + k]  # (a product of two fp32 values is exact in float64: only the sum's order matters)
    return rows.astype(np.float32)


# (L, in, hidden, out, heads): odd widths, a one-layer model, the 2-layer shape at which a GCN model gets the stack kernel's
# fragment copy -- this model does not --, three strides, and C = 3 with 8 heads
CASES = [(3, 3, 6, 6, 3), (1, 7, 0, 9, 1), (2, 9, 32, 32, 4), (3, 11, 130, 24, 2), (2, 5, 24, 24, 8)]


@pytest.mark.parametrize("d", [1, 3, 4, 16])
@pytest.mark.parametrize("L,fin,hid,out,heads", CASES)
def test_image_of_a_gat_model_with_edge_features(prog, tmp_path, L, fin, hid, out, heads, d):
    rng = np.random.default_rng(100 * fin + d)
    widths = layer_widths(L, fin, hid, out)
    layers = [layer_tensors(rng, a, b, heads, d) for a, b in widths]
    pools, mlp_n, mlp_hidden, mlp_out = 2, 2, 6, 3
    head = [uniform(rng, mlp_hidden, pools * out), uniform(rng, mlp_hidden), uniform(rng, mlp_out, mlp_hidden), uniform(rng, mlp_out)]
    img, layout = run(prog, tmp_path, [L, fin, hid, out, 1, heads, d, mlp_n, mlp_hidden, mlp_out, pools], [a for t in layers for a in t] + head)
    srows, ecols = layout.pop("score_rows"), layout.pop("edge_cols")
    assert ecols == -(-d // 4) * 4
    # blob order: w_gat, gat_bias, a_edge per layer, then the head LAST; every tensor padded to 4 floats; nothing else
    at, want = 0, {}
    for l, (a, b) in enumerate(widths):
        for name, n in (("w_gat", (b + srows) * a), ("gat_bias", b), ("a_edge", heads * ecols)):
            want[f"conv{l}.{name}"] = at
            at += -(-n // 4) * 4
    for i, t in enumerate(head):
        want[f"head{i // 2}.{'wb'[i % 2]}"] = at
        at += -(-t.size // 4) * 4
    assert layout == want and img.size == at
    # the plain GAT model of the same tensors: w_gat and gat_bias are bit-identical (the GEMM is unchanged)
    (tmp_path / "plain").mkdir()
    pimg, playout = run(prog, tmp_path / "plain", [L, fin, hid, out, 1, heads, 0, mlp_n, mlp_hidden, mlp_out, pools],
                        [a for t in layers for a in t[:4]] + head)
    assert playout.pop("edge_cols") == 0 and playout.pop("score_rows") == srows and not [k for k in playout if "a_edge" in k]
    for l, (a, b) in enumerate(widths):
        w, att_src, att_dst, bias, att_edge, w_edge = layers[l]
        for name, n in (("w_gat", (b + srows) * a), ("gat_bias", b)):
            off, poff = layout[f"conv{l}.{name}"], playout[f"conv{l}.{name}"]
            assert np.array_equal(img[off:off + n].view(np.uint32), pimg[poff:poff + n].view(np.uint32)), (l, name)
        off = layout[f"conv{l}.a_edge"]
        g = img[off:off + heads * ecols].reshape(heads, ecols)  # the table as the kernel reads it, row stride roundup4(d)
        assert np.array_equal(g[:, :d].view(np.uint32), fold_edge(w_edge, att_edge, heads).view(np.uint32)), l
        assert not g[:, d:].any()  # the pad columns are zeros
    for i, t in enumerate(head):
        off = layout[f"head{i // 2}.{'wb'[i % 2]}"]
        assert np.array_equal(img[off:off + t.size], t.ravel())


def test_the_fold_is_rounded_once(prog, tmp_path):
    """Operands at which an fp32 running sum differs from the float64 sum rounded once: the image holds the latter."""
    fin, out, heads, d = 5, 24, 2, 5
    rng = np.random.default_rng(7)
    layer = layer_tensors(rng, fin, out, heads, d)
    layer[5] = (layer[5] * np.float32(1 + 2.0 ** -12)).astype(np.float32)
    head = [uniform(rng, 3, out), uniform(rng, 3)]
    img, layout = run(prog, tmp_path, [1, fin, 0, out, 0, heads, d, 1, 6, 3, 1], layer + head)
    g = img[layout["conv0.a_edge"]:][:heads * 8].reshape(heads, 8)
    c = out // heads
    naive = np.zeros((heads, d), np.float32)
    for h in range(heads):
        for k in range(c):
            naive[h] = naive[h] + layer[4].reshape(heads, c)[h, k] * layer[5][h * c + k]  # fp32 all the way
    once = fold_edge(layer[5], layer[4], heads)
    assert not np.array_equal(naive, once)  # (the case tells the two apart)
    assert np.array_equal(g[:, :d], once) and not g[:, d:].any()
