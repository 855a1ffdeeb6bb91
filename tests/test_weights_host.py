"""The weight image of ``gnnb_model_create`` is pure host arithmetic (csrc/gnnb_weights.h): where every named tensor of a conv
layer sits in the blob, which derived forms a model has, the two permuted copies the stack kernels read, and the folded PNA
matrices.  Checked here without a GPU: tests/weights_host_main.cpp includes the header, is built with a plain ``g++`` under the
address and undefined-behaviour sanitizers and run as a child process on files; every reference is a numpy float64 restatement
written below, none is read from the C++.  Inputs are uniform(-1, 1), seeded."""
import itertools
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
GCN, GIN, SAGE, PNA = 0, 1, 2, 3  # gnnb_conv (include/gnnb_hip.h)
DEG_CLASSES = 16
SHAPES = [(3, 5), (7, 7), (12, 36), (33, 33)]  # (fi, fo): fo > 32 in the last two, where PNA's class weights exist
U24 = 2.0 ** -24  # half an fp32 ulp, relative

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = tmp_path_factory.mktemp("weights_host") / "weights_host_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I", str(ROOT / "include"),
                    "-I", str(ROOT / "gnn-builder_amd" / "csrc"), str(ROOT / "tests" / "weights_host_main.cpp"), "-o", str(exe)], check=True)
    return exe


def run(prog, tmp_path, job, tensors):
    """One child process: job = the mode and its numbers; tensors = the fp32 inputs.  -> (the output floats, the layout dict)."""
    tensors = [np.ascontiguousarray(t, dtype=np.float32) for t in tensors]
    (tmp_path / "job.txt").write_text(" ".join(str(v) for v in list(job) + [len(tensors)] + [t.size for t in tensors]))
    (tmp_path / "in.bin").write_bytes(b"".join(t.tobytes() for t in tensors))
    r = subprocess.run([str(prog), str(tmp_path / "job.txt"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(tmp_path / "out.txt")],
                       capture_output=True, text=True)
    report = r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in report and "runtime error" not in report and r.returncode == 0, (job, r.returncode, report)
    layout = {}
    if job[0] == "image":
        layout = {name: int(off) for name, off in (line.split() for line in (tmp_path / "out.txt").read_text().splitlines())}
    return np.fromfile(tmp_path / "out.bin", dtype=np.float32), layout


def uniform(rng, *shape):
    return rng.uniform(-1.0, 1.0, shape).astype(np.float32)


def layer_widths(L, fin, hid, out):
    """models.py:519-549"""
    if L == 1:
        return [(fin, out)]
    return [(fin, hid)] + [(hid, hid)] * (L - 2) + [(hid, out)]


CANONICAL = {  # per conv layer: (member the tensor is found under, shape), in the order of include/gnnb_hip.h; SAGE's Wl, Wr: in w_cat
    "gcn": lambda fi, fo, ed: [("w0", (fo, fi)), ("b0", (fo,))],
    "gin": lambda fi, fo, ed: [("w0", (fo, fi)), ("b0", (fo,)), ("w1", (fo, fo)), ("b1", (fo,))],
    "gine": lambda fi, fo, ed: [("w0", (fo, fi)), ("b0", (fo,)), ("w1", (fo, fo)), ("b1", (fo,)), ("edge_w", (fi, ed)), ("edge_b", (fi,))],
    "sage": lambda fi, fo, ed: [("wl", (fo, fi)), ("b_cat", (fo,)), ("wr", (fo, fi))],
    "pna": lambda fi, fo, ed: [("w_pre", (fi, 2 * fi)), ("b_pre", (fi,)), ("w_post", (fo, 13 * fi)), ("b_post", (fo,)), ("w_lin", (fo, fo)),
                               ("b_lin", (fo,))],
}
CONV_TYPE = {"gcn": GCN, "gin": GIN, "gine": GIN, "sage": SAGE, "pna": PNA}


def build_image(prog, tmp_path, conv, L, fin, hid, out, skip=0, fpx=(0, 0), delta=1.0, seed=0):
    """A model's image from seeded tensors -> (image, layout, per-layer dict of the canonical tensors, head tensors)."""
    rng = np.random.default_rng(seed)
    ed = 3 if conv == "gine" else 0
    layers, flat = [], []
    for fi, fo in layer_widths(L, fin, hid, out):
        t = {name: uniform(rng, *shape) for name, shape in CANONICAL[conv](fi, fo, ed)}
        layers.append(t)
        flat += list(t.values())
    pools, mlp_n, mlp_hidden, mlp_out = 2, 2, 6, 3
    head = [uniform(rng, mlp_hidden, pools * out), uniform(rng, mlp_hidden), uniform(rng, mlp_out, mlp_hidden), uniform(rng, mlp_out)]
    job = ["image", CONV_TYPE[conv], L, fin, hid, out, skip, fpx[0], fpx[1], delta, ed, mlp_n, mlp_hidden, mlp_out, pools]
    img, layout = run(prog, tmp_path, job, flat + head)
    return img, layout, layers, head


def on_grid(v, W, I):
    """q(v) of gnnb_model_desc::fpx_w (exact in float64: a floor at 2^-(W-I), a wrap into [-2^(I-1), 2^(I-1)))"""
    v = np.floor(v.astype(np.float64) * 2.0 ** (W - I)) / 2.0 ** (W - I)
    return v - 2.0 ** I * np.floor((v + 2.0 ** (I - 1)) / 2.0 ** I)


def expected_slots(conv, l, L, fi, fo, skip, fpx):
    """The members a layer has, in blob order, with their sizes: the canonical tensors, then the derived forms under the conditions
    gnnb_model_create builds them."""
    skip_fold = bool(skip) and l != 0 and l != L - 1 and fi == fo and not fpx
    if conv == "sage":
        return [("w_cat", fo * 2 * fi), ("b_cat", fo)] + ([("w_cat_skip", fo * 2 * fi)] if skip_fold else [])
    slots = [(name, int(np.prod(shape))) for name, shape in CANONICAL[conv](fi, fo, 3)]
    if conv == "pna" and not fpx:
        slots += [("w_fold", fo * 13 * fi), ("b_fold", fo)]
        if fo > 32:
            slots += [("w_class", DEG_CLASSES * fo * 5 * fi), ("b_class", DEG_CLASSES * fo)]
    return slots


def check_layout(conv, L, fin, hid, out, skip, fpx, img, layout, layers, head, zf=False, gin=False):
    """Every offset: a multiple of 4 floats, and exactly where the blob order puts it (conv layers, zf_w1f, gin_w, gin_b, head);
    the layout names exactly the members the model has; canonical tensors bit-exact at their offsets (on the grid under fpx)."""
    order = []
    for l, (fi, fo) in enumerate(layer_widths(L, fin, hid, out)):
        order += [(f"conv{l}.{name}", n) for name, n in expected_slots(conv, l, L, fi, fo, skip, fpx[0])]
    if zf:
        order.append(("zf_w1f", 16 * -(-out // 16) * hid))
    if gin:
        order += [("gin_w", (2 * L - 1) * hid * hid), ("gin_b", (2 * L - 1) * hid)]
    order += [(f"head{i // 2}.{'wb'[i % 2]}", t.size) for i, t in enumerate(head)]
    at, want = 0, {}
    for name, n in order:
        want[name] = at
        at += -(-n // 4) * 4
    assert layout == want  # (a member the model should not have, e.g. w_class at fo <= 32, would be an extra key)
    assert img.size == at and all(off % 4 == 0 for off in layout.values())
    put = (lambda t: on_grid(t, *fpx).astype(np.float32)) if fpx[0] else (lambda t: t)
    for l, t in enumerate(layers):
        for name, a in t.items():
            if name in ("wl", "wr"):
                continue
            off = layout[f"conv{l}.{name}"]
            assert np.array_equal(img[off:off + a.size], put(a).ravel()), (l, name)
        if conv == "sage":
            off = layout[f"conv{l}.w_cat"]
            cat = np.concatenate([put(t["wl"]), put(t["wr"])], 1)
            assert np.array_equal(img[off:off + cat.size], cat.ravel()), l
    for i, a in enumerate(head):
        off = layout[f"head{i // 2}.{'wb'[i % 2]}"]
        assert np.array_equal(img[off:off + a.size], put(a).ravel()), i
    if fpx[0]:
        W, I = fpx
        scaled = img.astype(np.float64) * 2.0 ** (W - I)
        assert np.array_equal(scaled, np.floor(scaled)) and img.min() >= -2.0 ** (I - 1) and img.max() < 2.0 ** (I - 1)


@pytest.mark.parametrize("conv", ["gcn", "gin", "gine", "sage", "pna"])
@pytest.mark.parametrize("fi,fo", SHAPES)
def test_layout_of_every_conv_type(prog, tmp_path, conv, fi, fo):
    """Three layers fi -> fo -> fo -> fo: the middle one has fi == fo, so with skip connections it is the layer whose derived
    forms carry + I.  Derived members exactly under gnnb_model_create's conditions: w_cat_skip iff such a layer and no fpx; w_fold
    iff no fpx, w_class iff also fo > 32; edge_w / edge_b iff a GINE model.  No width here has a stack kernel: no zf_w1f, no gin_w."""
    for skip, fpx in itertools.product((0, 1), ((0, 0), (16, 8))):
        if conv == "gine" and fpx[0]:
            continue  # (gnnb_edge_model_create refuses the combination)
        img, layout, layers, head = build_image(prog, tmp_path, conv, 3, fi, fo, fo, skip, fpx, delta=0.7, seed=fi + skip)
        check_layout(conv, 3, fi, fo, fo, skip, fpx, img, layout, layers, head)
        assert ("conv1.w_cat_skip" in layout) == (conv == "sage" and skip == 1 and not fpx[0])
        assert "conv0.w_cat_skip" not in layout and "conv2.w_cat_skip" not in layout
        for l in range(3):
            assert (f"conv{l}.w_fold" in layout) == (f"conv{l}.b_fold" in layout) == (conv == "pna" and not fpx[0])
            assert (f"conv{l}.w_class" in layout) == (f"conv{l}.b_class" in layout) == (conv == "pna" and not fpx[0] and fo > 32)
            assert (f"conv{l}.edge_w" in layout) == (f"conv{l}.edge_b" in layout) == (conv == "gine")
        if conv == "sage" and "conv1.w_cat_skip" in layout:
            off = layout["conv1.w_cat_skip"]
            want = np.concatenate([layers[1]["wl"], layers[1]["wr"] + np.eye(fo, dtype=np.float32)], 1)
            assert np.array_equal(img[off:off + want.size], want.ravel())


def test_layout_with_the_stack_kernels_copies(prog, tmp_path):
    """A 2-layer GCN of hidden % 16 == 0 has zf_w1f behind its conv layers; a GIN stack of hidden 32 / 64 / 128 has gin_w, gin_b
    there; the head comes last.  A GINE model of the same widths has no execution-order copy."""
    for fpx in ((0, 0), (16, 8)):
        img, layout, layers, head = build_image(prog, tmp_path, "gcn", 2, 11, 32, 20, 0, fpx)
        check_layout("gcn", 2, 11, 32, 20, 0, fpx, img, layout, layers, head, zf=True)
        img, layout, layers, head = build_image(prog, tmp_path, "gin", 3, 9, 32, 16, 1, fpx)
        check_layout("gin", 3, 9, 32, 16, 1, fpx, img, layout, layers, head, gin=True)
    img, layout, layers, head = build_image(prog, tmp_path, "gine", 3, 9, 32, 16, 1)
    check_layout("gine", 3, 9, 32, 16, 1, (0, 0), img, layout, layers, head)
    img, layout, layers, head = build_image(prog, tmp_path, "gcn", 3, 11, 32, 20)  # (three layers: k_gcn2_zf does not take it)
    check_layout("gcn", 3, 11, 32, 20, 0, (0, 0), img, layout, layers, head)


@pytest.mark.parametrize("fi,fo", SHAPES)
def test_sage_cat_weights(prog, tmp_path, fi, fo):
    rng = np.random.default_rng(fi)
    wl, wr = uniform(rng, fo, fi), uniform(rng, fo, fi)
    got, _ = run(prog, tmp_path, ["sage_cat", fo, fi, 0], [wl, wr])
    assert np.array_equal(got.reshape(fo, 2 * fi), np.concatenate([wl, wr], 1))
    if fi == fo:
        got, _ = run(prog, tmp_path, ["sage_cat", fo, fi, 1], [wl, wr])
        assert np.array_equal(got.reshape(fo, 2 * fi), np.concatenate([wl, wr + np.eye(fo, dtype=np.float32)], 1))


def fragment_order(w, K, out):
    """W zero-padded to whole 16-row slices, [NS, li, KQ, lg, e] -> [NS, KQ, lg, li, e]"""
    NS, KQ = -(-out // 16), K // 16
    padded = np.zeros((NS * 16, K), dtype=np.float32)
    padded[:out] = w
    return padded.reshape(NS, 16, KQ, 4, 4).transpose(0, 2, 3, 1, 4)


@pytest.mark.parametrize("K,out", [(32, 20), (64, 64), (128, 36)])
def test_zf_fragment_order(prog, tmp_path, K, out):
    w = uniform(np.random.default_rng(K), out, K)
    got, _ = run(prog, tmp_path, ["zf", K, out], [w])
    want = fragment_order(w, K, out)
    assert np.array_equal(got, want.ravel())
    rows_past_out = want.transpose(0, 3, 1, 2, 4).reshape(-1, K)[out:]  # (back in row order)
    assert rows_past_out.size == (16 * -(-out // 16) - out) * K and not rows_past_out.any()
    # and as the model's image holds it: the copy is made from layer 1's weight in the image
    img, layout, layers, _ = build_image(prog, tmp_path, "gcn", 2, 11, K, out, seed=K)
    off = layout["zf_w1f"]
    assert np.array_equal(img[off:off + want.size], fragment_order(layers[1]["w0"], K, out).ravel())


@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("half", [False, True])
def test_gin_execution_order(prog, tmp_path, L, half):
    """Wb0 | Wa1 Wb1 | ... at one hidden x hidden stride, each matrix at the top-left of its slot, zero elsewhere; biases likewise."""
    hid, fin = 32, 9
    out = hid // 2 if half else hid
    rng = np.random.default_rng(10 * L + half)
    layers = [{name: uniform(rng, *shape) for name, shape in CANONICAL["gin"](fi, fo, 0)} for fi, fo in layer_widths(L, fin, hid, out)]
    job = ["gin_exec", GIN, L, fin, hid, out, 0, 0, 0, 1.0, 0, 1, 4, 2, 1]
    got, _ = run(prog, tmp_path, job, [a for t in layers for a in t.values()])
    nm = 2 * L - 1
    w, b = got[:nm * hid * hid].reshape(nm, hid, hid), got[nm * hid * hid:].reshape(nm, hid)
    assert got.size == nm * hid * (hid + 1)
    mats = [(layers[0]["w1"], layers[0]["b1"])]
    for l in range(1, L):
        mats += [(layers[l]["w0"], layers[l]["b0"]), (layers[l]["w1"], layers[l]["b1"])]
    assert len(mats) == nm
    for i, (m, bias) in enumerate(mats):
        want_w, want_b = np.zeros((hid, hid), dtype=np.float32), np.zeros(hid, dtype=np.float32)
        want_w[:m.shape[0], :m.shape[1]] = m
        want_b[:bias.size] = bias
        assert np.array_equal(w[i], want_w) and np.array_equal(b[i], want_b), i
    if L >= 2:  # as the model's image holds it (a one-layer model has no stack kernel, and no copy)
        img, layout, ilayers, _ = build_image(prog, tmp_path, "gin", L, fin, hid, out, seed=L)
        off = layout["gin_w"]
        assert np.array_equal(img[off:off + hid * hid].reshape(hid, hid), ilayers[0]["w1"])


def fold64(w_post, b_post, w_lin, b_lin, fi, skip):
    """W' = W_lin W_post (+ I on the x block), b' = W_lin b_post + b_lin in float64, and the same expressions on absolute values"""
    w64 = lambda a: a.astype(np.float64)
    ref_w, ref_b = w64(w_lin) @ w64(w_post), w64(w_lin) @ w64(b_post) + w64(b_lin)
    abs_w, abs_b = np.abs(w64(w_lin)) @ np.abs(w64(w_post)), np.abs(w64(w_lin)) @ np.abs(w64(b_post)) + np.abs(w64(b_lin))
    if skip:
        ref_w[:, :fi] += np.eye(fi)
        abs_w[:, :fi] += np.eye(fi)
    return ref_w, ref_b, abs_w, abs_b


def pna_tensors(fi, fo, seed):
    rng = np.random.default_rng(seed)
    return {name: uniform(rng, *shape) for name, shape in CANONICAL["pna"](fi, fo, 0)}


def folded(prog, tmp_path, t, fi, fo, skip):
    got, _ = run(prog, tmp_path, ["pna_fold", fi, fo, skip], [t["w_post"], t["b_post"], t["w_lin"], t["b_lin"]])
    return got[:fo * 13 * fi].reshape(fo, 13 * fi), got[fo * 13 * fi:]


@pytest.mark.parametrize("fi,fo", SHAPES)
def test_pna_fold_lin(prog, tmp_path, fi, fo):
    """The code sums in double and rounds once to fp32: the error is half an fp32 ulp of a value no larger than A, the expression
    on absolute values; (1 + 1e-6) covers the double sums' own noise.  Measured: 0.93 x 2^-24 A."""
    t = pna_tensors(fi, fo, fi)
    for skip in ((0, 1) if fi == fo else (0,)):  # (+ I is folded only into a layer with fi == fo)
        w, b = folded(prog, tmp_path, t, fi, fo, skip)
        ref_w, ref_b, abs_w, abs_b = fold64(t["w_post"], t["b_post"], t["w_lin"], t["b_lin"], fi, skip)
        worst = max(np.max(np.abs(w - ref_w) / abs_w), np.max(np.abs(b - ref_b) / abs_b)) / U24
        print(f"pna_fold_lin ({fi}, {fo}) skip {skip}: worst error {worst:.3f} x 2^-24 A")
        assert np.all(np.abs(w - ref_w) <= U24 * abs_w * (1 + 1e-6)) and np.all(np.abs(b - ref_b) <= U24 * abs_b * (1 + 1e-6))


@pytest.mark.parametrize("delta", [1.0, 0.7])
@pytest.mark.parametrize("fi,fo", SHAPES)
def test_pna_degree_class_weights(prog, tmp_path, fi, fo, delta):
    """( W'_x + S_c Wq | W'_1 + amp W'_2 + att W'_3 ) and b' + S_c bq of the fp32 folded matrix, S_c = the max + min + mean blocks
    of the right half; amp and att in float32 with the code's two operations.  One rounding to fp32 gives 2^-24 A; libm's logf and
    numpy's may differ by one fp32 ulp, up to 2^-23 A each on the amp and att terms: 5 x 2^-24 A.  Measured: 2.32 x 2^-24 A."""
    t = pna_tensors(fi, fo, 100 + fi)
    w, b = folded(prog, tmp_path, t, fi, fo, int(fi == fo))
    got, _ = run(prog, tmp_path, ["pna_class", fi, fo, delta], [w, b, t["w_pre"], t["b_pre"]])
    n = DEG_CLASSES * fo * 5 * fi
    cw, cb = got[:n].reshape(DEG_CLASSES, fo, 5 * fi), got[n:].reshape(DEG_CLASSES, fo)
    assert got.size == n + DEG_CLASSES * fo
    w64, b64 = w.astype(np.float64), b.astype(np.float64)
    wq, bq = t["w_pre"][:, :fi].astype(np.float64), t["b_pre"].astype(np.float64)  # columns [0, F) act on the destination
    worst = 0.0
    for c in range(DEG_CLASSES):
        lg = np.log(np.float32(max(c, 1)) + np.float32(1.0))
        assert lg.dtype == np.float32
        amp, att = np.float64(lg / np.float32(delta)), np.float64(np.float32(delta) / lg)
        ref_a = w64[:, fi:5 * fi] + amp * w64[:, 5 * fi:9 * fi] + att * w64[:, 9 * fi:]
        abs_a = np.abs(w64[:, fi:5 * fi]) + amp * np.abs(w64[:, 5 * fi:9 * fi]) + att * np.abs(w64[:, 9 * fi:])
        ref_x, abs_x, ref_b, abs_b = w64[:, :fi], np.abs(w64[:, :fi]), b64, np.abs(b64)
        if c > 0:
            s = ref_a[:, :fi] + ref_a[:, fi:2 * fi] + ref_a[:, 2 * fi:3 * fi]
            abs_s = abs_a[:, :fi] + abs_a[:, fi:2 * fi] + abs_a[:, 2 * fi:3 * fi]
            ref_x, abs_x = ref_x + s @ wq, abs_x + abs_s @ np.abs(wq)
            ref_b, abs_b = ref_b + s @ bq, abs_b + abs_s @ np.abs(bq)
        else:  # class 0 carries no S term: the folded x block and bias, bit for bit
            assert np.array_equal(cw[0][:, :fi], w[:, :fi]) and np.array_equal(cb[0], b)
        ref, bound = np.concatenate([ref_x, ref_a], 1), np.concatenate([abs_x, abs_a], 1)
        worst = max(worst, np.max(np.abs(cw[c] - ref) / bound), np.max(np.abs(cb[c] - ref_b) / abs_b))
        assert np.all(np.abs(cw[c] - ref) <= 5 * U24 * bound * (1 + 1e-6)), c
        assert np.all(np.abs(cb[c] - ref_b) <= 5 * U24 * abs_b * (1 + 1e-6)), c
    print(f"pna_degree_class_weights ({fi}, {fo}) delta {delta}: worst error {worst / U24:.3f} x 2^-24 A")
