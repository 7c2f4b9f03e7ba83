"""The tile sort (zsc_amd/csrc/hash_sort.h) alone on the lane emulation, against a plain stable sort.

tests/emu_sort builds the kernel source with -DZSC_WAVE_EMU at 64 and at 16 lanes per wave and runs every
tile of a buffer the way k_hash_sort does.  A wave takes HS_SCATTER_BATCH steps of its slice through a
scatter as one unit (all loads, the multi-splits in step order, all stores), so the sizes are those at which
that can go wrong: slices with fewer steps than a batch, a ragged last batch or last step, the tile's edges,
and a second tile.  The kinds: one bucket with every lane on the same digit (zero), about one position per
bucket (random), and text.
"""
import bisect
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from zsc_amd import corpus

HERE = os.path.dirname(os.path.abspath(__file__))
TILE, DIR_STRIDE, HASH_MASK = 32768, 32776, 0x7FFF

KINDS = ("zero", "random", "text")
SIZES = (3, 66, 1027, 2049, 16 * 64 * 3 + 5, 32767, 32768, 32769, 32770, 2 * 32768 + 7)


@pytest.fixture(scope="module", params=["libsort_emu64.so", "libsort_emu16.so"], ids=["wave64", "wave16"])
def emu(request):
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_sort")], check=True)
    L = C.CDLL(os.path.join(HERE, "emu_sort", request.param))
    L.emu_sort_tiles.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def expected(data):
    """sorted / rank / dir of every tile by a plain stable sort on (hash, position)."""
    n = len(data)
    owners = max(n - 2, 0)
    ntiles = max(1, (n + TILE - 1) // TILE)
    sorted_ = np.full(ntiles * TILE, 0xDEADBEEF, dtype=np.uint32)
    rank = np.full(n, 0xDEAD, dtype=np.uint16)
    dir_ = np.full(ntiles * DIR_STRIDE, 0xDEAD, dtype=np.uint16)
    for t in range(ntiles):
        start = t * TILE
        m = min(max(owners - start, 0), TILE)
        h = [((data[start + p] << 10) ^ (data[start + p + 1] << 5) ^ data[start + p + 2]) & HASH_MASK for p in range(m)]
        order = sorted(range(m), key=lambda p: (h[p], p))
        keys = [h[p] for p in order]
        for idx, p in enumerate(order):
            sorted_[t * TILE + idx] = p | (h[p] << 16)
            rank[start + p] = idx
        for hh in range(32769):  # dir[h] = first sorted index whose hash is >= h; dir[32768] = m
            dir_[t * DIR_STRIDE + hh] = bisect.bisect_left(keys, hh)
    return ntiles, sorted_, rank, dir_


@pytest.fixture(scope="module")
def cases():
    """Every (kind, size) buffer with its expected arrays, computed once for both emulation builds."""
    out = {}
    for kind in KINDS:
        for n in SIZES:
            data = corpus.make_buffer(kind, n, 100 + n)
            out[kind, n] = (data, expected(data))
    return out


def test_constants(emu):
    assert emu.emu_sort_waves() == 16 and emu.emu_sort_batch() >= 1
    per_slice = 64 // emu.emu_sort_wave() * 32  # steps of a wave's slice in a full tile
    assert per_slice % emu.emu_sort_batch() == 0, "a full tile's slice is a whole number of batches (the fast path)"


@pytest.mark.parametrize("kind", KINDS)
def test_tile_sort_equals_a_stable_sort(emu, cases, kind):
    for n in SIZES:
        data, (ntiles, want_sorted, want_rank, want_dir) = cases[kind, n]
        got_sorted = np.zeros(ntiles * TILE, dtype=np.uint32)
        got_rank = np.zeros(max(n, 1), dtype=np.uint16)
        got_dir = np.zeros(ntiles * DIR_STRIDE, dtype=np.uint16)
        assert emu.emu_sort_tiles(data, n, got_sorted.ctypes.data, got_rank.ctypes.data, got_dir.ctypes.data) == ntiles
        # (what the sort does not write keeps the driver's fill pattern on both sides)
        assert np.array_equal(got_sorted, want_sorted), (kind, n, "sorted")
        assert np.array_equal(got_rank[:n], want_rank), (kind, n, "rank")
        assert np.array_equal(got_dir, want_dir), (kind, n, "dir")
