"""The packing kernels (zsc_amd/csrc/pack.h) on the lane emulation, against a numpy restatement.

tests/emu_pack builds pack.h with -DZSC_WAVE_EMU at 64 and at 16 lanes per wave and runs the launches that
zsc_hip_*_plan_pack and zsc_hip_unpack enqueue -- the scan's reduce / scan-of-sums / apply passes, then the
move, a wave per tile -- on item lengths, statuses and slot offsets this file supplies.  No deflate is needed:
the kernels move bytes whatever they are.  The contract held here (include/zsc_hip.h):

  * offsets[i] is the sum of the lengths before i, each rounded up to align; a failed item has length 0
  * pack writes every byte of [0, total): the items' bytes, zeros between them, and nothing at or behind total
  * with total > cap nothing is written
  * unpack writes [dst_off[i], + len[i]) and no other byte
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CANARY, MARGIN = 0xC7, 256
u8p, u32p, i32p, u64p = (C.POINTER(t) for t in (C.c_uint8, C.c_uint32, C.c_int32, C.c_uint64))


def load(name):
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_pack")], check=True)
    L = C.CDLL(os.path.join(HERE, "emu_pack", name))
    L.emu_pack_scan.argtypes = [u32p, i32p, C.c_uint64, C.c_uint32, u64p]
    L.emu_pack_move.argtypes = [C.c_int, C.c_uint64, u64p, u32p, i32p, u64p, C.c_void_p, C.c_void_p, C.c_uint64,
                                C.c_uint64]
    L.emu_pack_move.restype = None
    L.emu_pack_tile.restype = C.c_uint64
    L.B, L.TILE = L.emu_pack_scan_b(), L.emu_pack_tile()
    return L


@pytest.fixture(scope="module", params=["libpack_emu64.so", "libpack_emu16.so"])
def pk(request):
    L = load(request.param)
    assert L.emu_pack_wave() == (64 if "64" in request.param else 16)
    return L


def ptr(a, t):
    return a.ctypes.data_as(t)


def aligned(n):
    """n bytes of canary behind a 16-byte aligned start, with MARGIN bytes of canary on either side"""
    raw = np.full(n + 2 * MARGIN + 16, CANARY, dtype=np.uint8)
    skip = (-raw.ctypes.data) % 16
    whole = raw[skip:skip + n + 2 * MARGIN]
    return whole, whole[MARGIN:MARGIN + n]


def want_offsets(lens, status, align):
    eff = np.where(np.asarray(status) == 0, np.asarray(lens, dtype=np.uint64), np.uint64(0))
    a = np.uint64(align)
    return np.concatenate([[np.uint64(0)], np.cumsum((eff + a - np.uint64(1)) // a * a, dtype=np.uint64)]), eff


def scan(L, lens, status, align):
    n = len(lens)
    lens32 = np.ascontiguousarray(lens, dtype=np.uint32)
    st = np.ascontiguousarray(status, dtype=np.int32)
    off = np.full(n + 1, 0xEEEEEEEE, dtype=np.uint64)
    launches = L.emu_pack_scan(ptr(lens32, u32p), ptr(st, i32p), n, align, ptr(off, u64p))
    return off, launches


def round_trip(L, lens, align, status=None, seed=1, cap_short=0):
    """pack the items from slots with canaries around them, check the image byte by byte, unpack it into
    fresh slots and check those; returns the offsets"""
    n = len(lens)
    rng = np.random.default_rng(seed)
    status = [0] * n if status is None else status
    lens32 = np.ascontiguousarray(lens, dtype=np.uint32)
    st = np.ascontiguousarray(status, dtype=np.int32)
    want_off, eff = want_offsets(lens, status, align)
    total = int(want_off[-1])
    # slots: multiples of 16, 16 to 48 bytes of canary between an item's last granule and the next slot
    soff = np.zeros(max(n, 1), dtype=np.uint64)
    at = 0
    for i in range(n):
        soff[i] = at
        at += (int(lens[i]) + 15) // 16 * 16 + 16 * int(rng.integers(1, 4))
    swhole, sparse = aligned(at)
    data = []
    for i in range(n):
        d = rng.integers(1, 256, int(lens[i]), dtype=np.uint8)  # (no zeros: a missing byte shows against the padding)
        data.append(d)
        sparse[int(soff[i]):int(soff[i]) + len(d)] = d
    sparse_before = swhole.copy()

    off, _ = scan(L, lens, status, align)
    assert np.array_equal(off, want_off)

    image = np.zeros(total, dtype=np.uint8)
    for i in range(n):
        if status[i] == 0:
            image[int(off[i]):int(off[i]) + len(data[i])] = data[i]
    tiles = (total + L.TILE - 1) // L.TILE + 2  # (the grid comes from the capacity: tiles behind the end return)
    dwhole, dense = aligned(total + 64)
    cap = total - cap_short
    L.emu_pack_move(0, n, ptr(off, u64p), ptr(lens32, u32p), ptr(st, i32p), ptr(soff, u64p), dense.ctypes.data,
                    sparse.ctypes.data, cap, tiles)
    assert np.array_equal(swhole, sparse_before), "the pack wrote to its source"
    if cap_short:
        assert (dwhole == CANARY).all(), "total > cap, yet something was written"
        return off
    assert np.array_equal(dense[:total], image)
    assert (dwhole[:MARGIN] == CANARY).all() and (dwhole[MARGIN + total:] == CANARY).all(), "written outside [0, total)"

    # and back: only the items' own bytes may change
    bwhole, back = aligned(at)
    want_back = bwhole.copy()
    for i in range(n):
        if status[i] == 0:
            want_back[MARGIN + int(soff[i]):MARGIN + int(soff[i]) + len(data[i])] = data[i]
    exact = np.ascontiguousarray(dense[:total])  # (a copy: nothing behind total to read by accident)
    epad = np.zeros(total + 16, dtype=np.uint8)
    base = (-epad.ctypes.data) % 16
    epad[base:base + total] = exact
    L.emu_pack_move(1, n, ptr(off, u64p), ptr(eff.astype(np.uint32), u32p), None, ptr(soff, u64p),
                    epad[base:].ctypes.data, back.ctypes.data, 2 ** 64 - 1, tiles)
    assert np.array_equal(bwhole, want_back)
    return off


def special_lens(L):
    T = L.TILE
    return [0, 1, 2, 8, 15, 16, 17, 20, 31, 33, T - 1, T, T + 1, 3 * T + 5]


# ---- offsets ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["0", "1", "B-1", "B", "B+1", "B*B", "B*B+3"])
def test_offsets_at_the_scan_boundaries(pk, which):
    B = pk.B
    n = {"0": 0, "1": 1, "B-1": B - 1, "B": B, "B+1": B + 1, "B*B": B * B, "B*B+3": B * B + 3}[which]
    rng = np.random.default_rng(n + 7)
    lens = rng.integers(0, 70000, n, dtype=np.uint32)
    status = np.where(rng.integers(0, 9, n) == 0, -5, 0).astype(np.int32)
    for align in (1, 16, 4096):
        off, launches = scan(pk, lens, status, align)
        want, _ = want_offsets(lens, status, align)
        assert np.array_equal(off, want), (which, align)
        assert launches == (1 if n <= B else 3 if n <= B * B else 5)


def test_total_beyond_4_gib(pk):
    """no memory behind the items: the scan alone, in 64 bits"""
    n = 3 * pk.B + 5
    lens = np.full(n, 0xFFFFFFF1, dtype=np.uint32)
    lens[::7] = 3
    status = np.zeros(n, dtype=np.int32)
    off, _ = scan(pk, lens, status, 16)
    want, _ = want_offsets(lens, status, 16)
    assert int(want[-1]) > 2 ** 43 and np.array_equal(off, want)


# ---- moves -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shift", range(16))
def test_every_length_at_every_misalignment(pk, shift):
    """align 1 with `shift` one-byte items in front: source and destination are `shift` bytes apart"""
    for n in special_lens(pk):
        off = round_trip(pk, [1] * shift + [n, 5], 1, seed=shift * 100 + n % 97)
        assert int(off[shift]) == shift


@pytest.mark.parametrize("align", [16, 256])
def test_every_length_aligned(pk, align):
    for n in special_lens(pk):
        round_trip(pk, [1, n, 3, n], align, seed=n % 89)


@pytest.mark.parametrize("align", [1, 16, 256])
def test_sixty_four_two_byte_items(pk, align):
    """an empty raw stream is two bytes: eight of them share a granule"""
    round_trip(pk, [2] * 64, align)
    round_trip(pk, [8] * 33 + [20] * 31, align)


@pytest.mark.parametrize("align", [1, 16, 256])
def test_zero_length_items(pk, align):
    round_trip(pk, [0, 17, 33], align)
    round_trip(pk, [17, 33, 0], align)
    round_trip(pk, [17, 0, 33], align)
    round_trip(pk, [0, 0, 0], align)
    round_trip(pk, [0] * 70 + [pk.TILE + 1] + [0] * 70 + [1], align)
    round_trip(pk, [], align)


@pytest.mark.parametrize("align", [1, 16, 256])
def test_failed_items_take_no_room(pk, align):
    round_trip(pk, [100, 5000, 33, 7], align, status=[0, -5, 0, -5])
    round_trip(pk, [100, 5000], align, status=[-5, -5])


@pytest.mark.parametrize("align", [1, 16, 256])
def test_seeded_mix(pk, align):
    rng = np.random.default_rng(300 + align)
    sp = special_lens(pk)
    lens = [sp[int(rng.integers(0, 10))] if rng.integers(0, 4) else sp[int(rng.integers(0, 14))] for _ in range(300)]
    status = [0 if rng.integers(0, 16) else -5 for _ in range(300)]
    round_trip(pk, lens, align, status=status, seed=align)


@pytest.mark.parametrize("align", [1, 16])
def test_nothing_moves_into_a_short_image(pk, align):
    round_trip(pk, [17, pk.TILE + 1, 2, 2, 300], align, cap_short=1)
    round_trip(pk, [1], align, cap_short=1)


# ---- the sanitizer build ---------------------------------------------------------------------------------

def test_seeded_mix_under_address_sanitizer():
    """`make asan`: the harness as a program of its own with AddressSanitizer and UBSan; the sparse image ends
    at the last item's end rounded up to 16 and the dense one exactly at total"""
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_pack"), "asan"], check=True)
    r = subprocess.run([os.path.join(HERE, "emu_pack", "pack_asan")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(" 0 mismatches") == 3, r.stdout
