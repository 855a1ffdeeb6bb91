"""The weight image of a PNA model with edge features (csrc/gnnb_weights.h: ``build_weight_image`` with a PNA description and
``edge_dim > 0``), checked without a GPU by the stand-alone program of tests/test_weights_host.py (tests/weights_host_main.cpp
built with ``g++`` under the address and undefined-behaviour sanitizers): eight tensors per layer; the six of PNA stored raw with a
three-block pre-NN; ``edge_w = W_pre[:, 2F:3F] W_enc`` and ``edge_b = W_pre[:, 2F:3F] b_enc`` derived; ``w_fold`` as for PNA; no
degree-class form."""
import shutil

import numpy as np
import pytest

from test_weights_host import PNA, SHAPES, fold64, layer_widths, prog, run, uniform  # noqa: F401  (prog: the fixture)

ED = 3
U23 = 2.0 ** -23  # one fp32 ulp, relative

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def pnae_tensors(rng, fi, fo):
    """A layer's eight tensors in canonical order: (member the raw tensor is found under, or None for the edge encoder's; array)."""
    return [("w_pre", uniform(rng, fi, 3 * fi)), ("b_pre", uniform(rng, fi)), ("w_post", uniform(rng, fo, 13 * fi)), ("b_post", uniform(rng, fo)),
            ("w_lin", uniform(rng, fo, fo)), ("b_lin", uniform(rng, fo)), (None, uniform(rng, fi, ED)), (None, uniform(rng, fi))]


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("fi,fo", SHAPES)
def test_image_of_a_pna_model_with_edge_features(prog, tmp_path, fi, fo, skip):
    """Three layers fi -> fo -> fo -> fo (the middle one carries + I in w_fold when skip is set)."""
    rng = np.random.default_rng(10 * fi + skip)
    L, delta = 3, 0.7
    layers = [pnae_tensors(rng, a, b) for a, b in layer_widths(L, fi, fo, fo)]
    pools, mlp_n, mlp_hidden, mlp_out = 2, 2, 6, 3
    head = [uniform(rng, mlp_hidden, pools * fo), uniform(rng, mlp_hidden), uniform(rng, mlp_out, mlp_hidden), uniform(rng, mlp_out)]
    job = ["image", PNA, L, fi, fo, fo, skip, 0, 0, delta, ED, mlp_n, mlp_hidden, mlp_out, pools]
    img, layout = run(prog, tmp_path, job, [a for t in layers for _, a in t] + head)
    # blob order: the raw six, w_fold, b_fold, edge_w, edge_b per layer, then the head; every tensor padded to 4 floats
    at, want = 0, {}
    for l, (a, b) in enumerate(layer_widths(L, fi, fo, fo)):
        sizes = [(n, t.size) for n, t in layers[l] if n] + [("w_fold", b * 13 * a), ("b_fold", b), ("edge_w", a * ED), ("edge_b", a)]
        for name, n in sizes:
            want[f"conv{l}.{name}"] = at
            at += -(-n // 4) * 4
    for i, t in enumerate(head):
        want[f"head{i // 2}.{'wb'[i % 2]}"] = at
        at += -(-t.size // 4) * 4
    assert layout == want and img.size == at  # (no w_class / b_class at any width, fo > 32 included)
    w64 = lambda a: a.astype(np.float64)  # noqa: E731
    for l, (a, b) in enumerate(layer_widths(L, fi, fo, fo)):
        t = dict((n, v) for n, v in layers[l] if n)
        w_enc, b_enc = layers[l][6][1], layers[l][7][1]
        for name, v in t.items():  # the raw tensors in place, w_pre with its row stride of 3 fi
            off = layout[f"conv{l}.{name}"]
            assert np.array_equal(img[off:off + v.size], v.ravel()), (l, name)
        wc = w64(t["w_pre"][:, 2 * a:])
        for name, ref in (("edge_w", wc @ w64(w_enc)), ("edge_b", wc @ w64(b_enc))):
            off = layout[f"conv{l}.{name}"]
            got = img[off:off + ref.size].reshape(ref.shape)
            worst = np.max(np.abs(got - ref) / np.abs(ref))
            print(f"layer {l} {name} ({a}, {b}): worst error {worst / U23:.3f} ulp")
            assert np.all(np.abs(got - ref) <= U23 * np.abs(ref)), (l, name)
        # w_fold as for PNA (test_weights_host.test_pna_fold_lin's bound), + I on the skip middle layer
        ref_w, ref_b, abs_w, abs_b = fold64(t["w_post"], t["b_post"], t["w_lin"], t["b_lin"], a, bool(skip) and l == 1)
        off_w, off_b = layout[f"conv{l}.w_fold"], layout[f"conv{l}.b_fold"]
        assert np.all(np.abs(img[off_w:off_w + ref_w.size].reshape(ref_w.shape) - ref_w) <= 2.0 ** -24 * abs_w * (1 + 1e-6))
        assert np.all(np.abs(img[off_b:off_b + b] - ref_b) <= 2.0 ** -24 * abs_b * (1 + 1e-6))
    for i, t in enumerate(head):
        off = layout[f"head{i // 2}.{'wb'[i % 2]}"]
        assert np.array_equal(img[off:off + t.size], t.ravel())
