"""The size of the ordered ingest's allocation (``gnnb_order_bytes``, behind ``CompiledModel.enable_ordered_ingest``) is pure host
arithmetic: positive, monotone in each of its five arguments, large enough for every array the kernels of csrc/k_order.hip
index, and its own -- the plain ingest's allocation (``gnnb_ingest_bytes``) keeps the sizes it had.  No GPU needed."""
import pytest

from gnnbuilder_amd import runtime


@pytest.fixture(scope="module")
def lib():
    if not runtime.LIB_PATH.exists():
        runtime.build_library()  # hipcc cross-compiles gfx950 without a GPU
    return runtime


def needed(B, N, E, in_dim, mlp_out):
    """Bytes the kernels index at these capacities: x_ord [N, in_dim] and the staged outputs [B, mlp_out] fp32; coo [E, 2], the
    two ptr arrays [B+1], perm and the two shifts [B], int32."""
    return 4 * (N * in_dim + B * mlp_out + 2 * E + 2 * (B + 1) + 3 * B)


def exact(B, N, E, in_dim, mlp_out):
    """The allocation's closed form: every array's bytes rounded up to 256 -- x_ord, coo (sized for at least one edge), the two
    ptr arrays, perm and the two shifts, the staged outputs."""
    up = lambda b: -(-b // 256) * 256
    return up(4 * N * in_dim) + up(8 * max(E, 1)) + 2 * up(4 * (B + 1)) + 3 * up(4 * B) + up(4 * B * mlp_out)


def test_size_is_positive_and_monotone_in_every_argument(lib):
    assert lib.order_bytes(0, 0, 0, 0, 0) > 0
    grid = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 70_000, 1 << 20]
    for axis in range(5):
        for other in [(0, 0, 0, 0), (1, 1, 1, 1), (300, 5000, 9, 3), (4096, 110_000, 130, 19)]:
            sizes = []
            for v in grid:
                args = list(other)
                args.insert(axis, v)
                sizes.append(lib.order_bytes(*args))
                assert sizes[-1] == lib.order_bytes(*args) > 0  # (a function of the five numbers alone)
                assert sizes[-1] == exact(*args), args
            assert sizes == sorted(sizes), (axis, other, sizes)


def test_size_covers_what_the_kernels_index(lib):
    # the shapes of tests/test_hip_order.py among them
    for args in [(512, 16384, 32768, 11, 3), (2049, 10245, 16392, 3, 3), (300, 7596, 16600, 9, 3), (12, 214, 460, 130, 3), (1, 1, 0, 1, 1),
                 (4096, 110_000, 240_000, 9, 1), (1 << 20, 1 << 24, 1 << 25, 256, 64)]:
        assert lib.order_bytes(*args) >= needed(*args), args
        assert lib.order_bytes(*args) <= needed(*args) + 8 + 8 * 256, args  # (no more than the arrays and their 256-byte alignment)
        assert lib.order_bytes(*args) == exact(*args), args


def test_size_does_not_depend_on_another_model(lib):
    """A function of its arguments, not of any model or workspace the process holds: the same capacities at another model's
    widths give that model's size, and asking does not change the answer for the first."""
    caps = (300, 5000, 11000)
    first = lib.order_bytes(*caps, 9, 3)
    other = lib.order_bytes(*caps, 130, 19)
    assert other > first
    assert lib.order_bytes(*caps, 9, 3) == first and lib.order_bytes(*caps, 130, 19) == other
    assert other - first >= 4 * (5000 * (130 - 9) + 300 * (19 - 3)) - 2 * 256


def test_the_plain_ingest_keeps_its_allocation_size(lib):
    """``gnnb_ingest_bytes`` as it was before the ordered form existed (the ordered arrays have an allocation of their own)."""
    before = {(1, 1, 0): 3072, (12, 300, 700): 18688, (300, 5000, 11000): 278272, (4096, 110_000, 240_000): 6034176,
              (70_000, 140_000, 140_000): 4061184}
    for caps, size in before.items():
        assert lib.ingest_bytes(*caps) == size, caps


def test_negative_capacities_have_no_size(lib):
    assert lib.order_bytes(-1, 1, 1, 1, 1) == 0 and lib.order_bytes(1, 1, 1, -1, 1) == 0
