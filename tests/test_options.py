"""gnnb_set_option against the table of options as the project documents it: every name, and for every name which values
are taken and which are refused.  The library loads without a GPU; no compute calls here.

The options are process-wide, so every call is made in a child process that reports what happened; the expectations
below are written out by hand (they are NOT read from csrc/gnnb_internal.h: that is the code under test)."""
import json
import os
import subprocess
import sys
import textwrap
from pathlib import Path

import pytest

from gnnbuilder_amd import runtime

ROOT = Path(__file__).resolve().parent.parent
GNNB_ERR_INVALID = -1  # include/gnnb_hip.h


def between(lo, hi):
    return lambda v: lo <= v <= hi


def one_of(*vals):
    return lambda v: v in vals


FLAG = between(0, 1)

# name -> (default, the values gnnb_set_option takes).  The default is what the environment variable GNNB_<NAME> replaces;
# it is listed for the record -- without a getter only the GPU tests can observe it (tests/test_hip_parity.py).
OPTIONS = {
    "tile_rows": (8, lambda v: v >= 4),  # (no upper bound)
    "agg_lds_kb": (0, between(0, 160)),
    "agg_ring_waves": (0, one_of(0, 1, 2, 4, 8, 16)),
    "agg_ring_slots": (2, between(1, 4)),
    "agg_ring_wg_per_cu": (1, between(1, 4)),
    "agg_nt_store": (1, FLAG),
    "agg_balance": (0, FLAG),
    "gemm_variant": (0, FLAG),
    "gemm_max_wg_per_cu": (2, between(1, 8)),
    "gemm_dma": (1, FLAG),
    "gemm_wlds": (1, FLAG),
    "gemm_wlds_slots": (2, between(1, 4)),
    "fuse_narrow": (1, FLAG),
    "first_ring": (1, FLAG),
    "fuse_zf": (1, FLAG),
    "large_fork": (2, between(0, 2)),
    "zf_shape": (2, between(0, 2)),
    "fuse_gcn2": (1, FLAG),
    "fuse_head": (1, FLAG),
    "fuse_pool": (1, FLAG),
    "head_small": (1, FLAG),
    "head_split": (0, FLAG),
    "math": (0, between(0, 3)),
    "gemm_tail_split": (2, between(0, 2)),
    "pna_fold_lin": (1, FLAG),
    "pna_classes": (1, FLAG),
    "fold_skip": (1, FLAG),
    "sage_first_mean": (1, FLAG),
    "pna_first": (1, FLAG),
    "pna_pagg": (1, FLAG),
    "stage_cut": (0, FLAG),
    "zf_head": (0, FLAG),
    "agg_form": (0, between(0, 2)),
    "agg_rg_r": (0, between(0, 4)),
    "agg_rg_wgs": (0, between(0, 64)),
    "agg_rg_flags": (1, between(0, 15)),
    "prep_group": (4, one_of(1, 4)),
    "head_pairs": (1, FLAG),
    "guest_prep": (1, FLAG),
}
VALUES = list(range(-2, 171)) + [100000]

# what the child does: every call, nothing judged -- {"name": {"value": [return code, last error]}}; names[-1] = None is the NULL name
DRIVER = textwrap.dedent('''
    import json, sys
    sys.path.insert(0, %(root)r)
    from gnnbuilder_amd import runtime
    lib = runtime.load_library(require_gpu=False)
    names, values = json.loads(sys.argv[1])
    out = {}
    for name in names:
        res = {}
        for v in values:
            rc = lib.gnnb_set_option(None if name is None else name.encode(), v)
            res[str(v)] = [rc, lib.gnnb_last_error().decode() if rc != 0 else ""]
        out["<NULL>" if name is None else name] = res
    print(json.dumps(out))
''')


@pytest.fixture(scope="module")
def calls():
    if not runtime.LIB_PATH.exists():
        runtime.build_library()
    names = list(OPTIONS) + ["no_such_option", "", "TILE_ROWS", "tile_rows ", None]
    run = subprocess.run([sys.executable, "-c", DRIVER % {"root": str(ROOT)}, json.dumps([names, VALUES])], capture_output=True, text=True,
                         env=dict(os.environ), timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    return json.loads(run.stdout.strip().splitlines()[-1])


def test_the_table_has_every_option_once():
    assert len(OPTIONS) == 39
    assert all(accepts(default) for default, accepts in OPTIONS.values())  # (every default is a value the setter takes)


@pytest.mark.parametrize("name", list(OPTIONS))
def test_set_option_takes_exactly_the_documented_values(calls, name):
    accepts = OPTIONS[name][1]
    wrong = []
    for v in VALUES:
        rc, msg = calls[name][str(v)]
        if (rc == 0) != bool(accepts(v)):
            wrong.append((v, rc))
        elif rc != 0 and (rc != GNNB_ERR_INVALID or f"unknown option or bad value: {name}={v}" not in msg):
            wrong.append((v, rc, msg))
    assert not wrong, (name, wrong[:8])


@pytest.mark.parametrize("name", ["no_such_option", "", "TILE_ROWS", "tile_rows "])
def test_unknown_names_are_refused(calls, name):
    for v in VALUES:
        rc, msg = calls[name][str(v)]
        assert rc == GNNB_ERR_INVALID and f"{name}={v}" in msg, (name, v, rc, msg)


def test_null_name_is_refused(calls):
    for v in VALUES:
        rc, msg = calls["<NULL>"][str(v)]
        assert rc == GNNB_ERR_INVALID and msg, (v, rc, msg)
