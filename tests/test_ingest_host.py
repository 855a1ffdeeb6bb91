"""The size of the ingest allocation (``gnnb_ingest_bytes``, behind ``CompiledModel.enable_ingest``) is pure host arithmetic:
monotone in each capacity, and large enough for every array the kernels of csrc/k_ingest.hip index.  No GPU needed."""
import itertools

import pytest

from gnnbuilder_amd import runtime


@pytest.fixture(scope="module")
def size():
    if not runtime.LIB_PATH.exists():
        runtime.build_library()  # hipcc cross-compiles gfx950 without a GPU
    return runtime.ingest_bytes


def needed(B, N, E):
    """Bytes the kernels index at capacity (B, N, E): node_ptr and edge_ptr [B+1], coo [E, 2], two halves of (key, edge index)
    [E] each, digit counts [2^bits x tiles], the state words -- all int32."""
    tiles = -(-E // runtime.INGEST_TILE)
    return 4 * (2 * (B + 1) + 2 * E + 4 * E + (1 << runtime.INGEST_DIGIT_BITS) * tiles + 4)


def exact(B, N, E):
    """The allocation's closed form: every array's bytes rounded up to 256 -- the state words, the two ptr arrays, coo, two
    halves of keys and edge indices, the digit counts; sized for at least one edge."""
    up = lambda b: -(-b // 256) * 256
    E = max(E, 1)
    tiles = -(-E // runtime.INGEST_TILE)
    return up(16) + 2 * up(4 * (B + 1)) + up(8 * E) + 4 * up(4 * E) + up(4 * (1 << runtime.INGEST_DIGIT_BITS) * tiles)


def test_size_is_a_monotone_function_of_the_capacities(size):
    grid = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2048, 2049, 65536, 70_000, 140_000, 1 << 20]
    for axis in range(3):
        for other in [(1, 1), (300, 5000), (70_000, 140_000)]:
            sizes = []
            for v in grid:
                caps = list(other)
                caps.insert(axis, v)
                sizes.append(size(*caps))
                assert sizes[-1] == size(*caps) > 0  # (a function of the three numbers alone)
                assert sizes[-1] == exact(*caps), caps
            assert sizes == sorted(sizes), (axis, other, sizes)


def test_size_covers_what_the_kernels_index(size):
    # the shapes of tests/test_hip_ingest.py: 70 000 two-node graphs, and the edge counts around wave / workgroup / tile
    shapes = [(70_000, 140_000, 140_000), (512, 16384, 32768)]
    shapes += [(5, 40, E) for E in (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)]
    shapes += list(itertools.product([1, 12, 300], [1, 5000], [0, 1024, 1025, 11000]))
    for B, N, E in shapes:
        assert size(B, N, E) >= needed(B, N, E), (B, N, E)
        assert size(B, N, E) <= needed(B, N, max(E, 1)) + 16 * 256  # (no more than the arrays and their 256-byte alignment)
        assert size(B, N, E) == exact(B, N, E), (B, N, E)
