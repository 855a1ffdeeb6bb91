"""The weight image of a GAT (v1) model (csrc/gnnb_weights.h: ``build_weight_image`` with a GCN description and ``gat1_heads > 0``),
checked without a GPU by a stand-alone program of its own (tests/weights_host_gatconv_main.cpp, with its own ``main``, built with
``g++`` under the address and undefined-behaviour sanitizers and run as a child process on files -- never loaded into Python): four
tensors per layer; one derived slot ``w_gat = [W ; A_src W ; A_dst W ; 0]`` [out + roundup4(2 heads), in] whose folded rows are
summed in double and rounded once, ``gat_bias`` raw; none of GCN's or GATv2's slots and no fragment copy for the stack kernel,
whatever the widths; the head last.  Everything bit for bit."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_weights_host import layer_widths, uniform

ROOT = Path(__file__).resolve().parent.parent

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def gatconv_prog(tmp_path_factory):
    exe = tmp_path_factory.mktemp("weights_host_gatconv") / "weights_host_gatconv_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I", str(ROOT / "include"),
                    "-I", str(ROOT / "gnn-builder_amd" / "csrc"), str(ROOT / "tests" / "weights_host_gatconv_main.cpp"), "-o", str(exe)], check=True)
    return exe


def run_gatconv(prog, tmp_path, job, tensors):
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


def gatconv_tensors(rng, fi, fo, heads):
    """A layer's four tensors in canonical order (include/gnnb_gatconv.h)."""
    return [uniform(rng, fo, fi), uniform(rng, 1, heads, fo // heads), uniform(rng, 1, heads, fo // heads), uniform(rng, fo)]


def fold(w, att, heads):
    """[heads, in]: row h = sum_c att[h, c] * W[h C + c, :] in float64, c increasing, rounded to fp32 once."""
    fo, fi = w.shape
    c = fo // heads
    att = att.reshape(heads, c).astype(np.float64)
    w64 = w.astype(np.float64)
    rows = np.zeros((heads, fi), np.float64)
    for h in range(heads):
        for k in range(c):
            rows[h] += att[h, k] * w64[h * c + k]  # (a product of two fp32 values is exact in float64: only the sum's order matters)
    return rows.astype(np.float32)


# (L, in, hidden, out, heads): odd widths (sizes that are no multiple of 4 floats are padded), a one-layer model, the 2-layer shape
# with hidden % 16 == 0 at which a GCN model gets the stack kernel's fragment copy -- a GAT model does not --, three strides, and
# 2 heads = 16 score rows with C = 3
CASES = [(3, 3, 6, 6, 3), (1, 7, 0, 9, 1), (2, 9, 32, 32, 4), (3, 11, 130, 24, 2), (2, 5, 24, 24, 8)]


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("L,fin,hid,out,heads", CASES)
def test_image_of_a_gat_model(gatconv_prog, tmp_path, L, fin, hid, out, heads, skip):
    rng = np.random.default_rng(100 * fin + skip)
    widths = layer_widths(L, fin, hid, out)
    layers = [gatconv_tensors(rng, a, b, heads) for a, b in widths]
    pools, mlp_n, mlp_hidden, mlp_out = 2, 2, 6, 3
    head = [uniform(rng, mlp_hidden, pools * out), uniform(rng, mlp_hidden), uniform(rng, mlp_out, mlp_hidden), uniform(rng, mlp_out)]
    job = [L, fin, hid, out, skip, heads, mlp_n, mlp_hidden, mlp_out, pools]
    img, layout = run_gatconv(gatconv_prog, tmp_path, job, [a for t in layers for a in t] + head)
    srows = layout.pop("score_rows")
    assert srows == -(-2 * heads // 4) * 4 and srows >= 2 * heads and srows % 4 == 0
    # blob order: w_gat, gat_bias per layer, then the head; every tensor padded to 4 floats; nothing else -- none of GCN's slots
    # (w0, b0), none of GATv2's (w_lr, b_lr, att), no fragment copy (zf_w1f)
    at, want = 0, {}
    for l, (a, b) in enumerate(widths):
        for name, n in (("w_gat", (b + srows) * a), ("gat_bias", b)):
            want[f"conv{l}.{name}"] = at
            at += -(-n // 4) * 4
    for i, t in enumerate(head):
        want[f"head{i // 2}.{'wb'[i % 2]}"] = at
        at += -(-t.size // 4) * 4
    assert layout == want and img.size == at
    for l, (a, b) in enumerate(widths):
        w, att_src, att_dst, bias = layers[l]
        off = layout[f"conv{l}.w_gat"]
        g = img[off:off + (b + srows) * a].reshape(b + srows, a)  # the matrix as the layer's GEMM reads it
        assert np.array_equal(g[:b], w)  # W's own rows, copied
        assert np.array_equal(g[b:b + heads].view(np.uint32), fold(w, att_src, heads).view(np.uint32)), (l, "src")
        assert np.array_equal(g[b + heads:b + 2 * heads].view(np.uint32), fold(w, att_dst, heads).view(np.uint32)), (l, "dst")
        assert g[b + 2 * heads:].shape[0] == srows - 2 * heads and not g[b + 2 * heads:].any()  # the pad rows are zeros
        assert not img[off + g.size:off + g.size + (-g.size % 4)].any()
        off = layout[f"conv{l}.gat_bias"]
        assert np.array_equal(img[off:off + b], bias)
        assert not img[off + b:off + b + (-b % 4)].any()
    for i, t in enumerate(head):
        off = layout[f"head{i // 2}.{'wb'[i % 2]}"]
        assert np.array_equal(img[off:off + t.size], t.ravel())


def test_the_fold_is_rounded_once(gatconv_prog, tmp_path):
    """Operands at which an fp32 running sum differs from the float64 sum rounded once: the image holds the latter."""
    fin, out, heads = 5, 24, 2
    rng = np.random.default_rng(7)
    w = (uniform(rng, out, fin) * np.float32(1 + 2.0 ** -12)).astype(np.float32)
    att_src, att_dst = uniform(rng, 1, heads, out // heads), uniform(rng, 1, heads, out // heads)
    head = [uniform(rng, 3, out), uniform(rng, 3)]
    img, layout = run_gatconv(gatconv_prog, tmp_path, [1, fin, 0, out, 0, heads, 1, 6, 3, 1], [w, att_src, att_dst, uniform(rng, out)] + head)
    g = img[layout["conv0.w_gat"]:][:(out + 4) * fin].reshape(out + 4, fin)
    c = out // heads
    naive = np.zeros((heads, fin), np.float32)
    for h in range(heads):
        for k in range(c):
            naive[h] = naive[h] + att_src.reshape(heads, c)[h, k] * w[h * c + k]  # fp32 all the way
    once = fold(w, att_src, heads)
    assert not np.array_equal(naive, once)  # (the case tells the two apart)
    assert np.array_equal(g[out:out + heads], once)
