"""The seek-point index a deflate plan writes with its streams (zsc_amd/csrc/deflate_index.h) on the lane
emulation, against the oracle and the indexed inflate path.

tests/emu_dindex builds the deflate pipeline's kernel sources and deflate_index.h with -DZSC_WAVE_EMU and
runs what zsc_hip_deflate_plan_run enqueues for one buffer with the index on, then the export.  Every
stream must be the oracle's; every blob is taken apart here from the layout documented in
include/zsc_hip.h and must name exactly the points the rule of DESIGN.md section 11 gives for the stream's
blocks, with the check values and windows of the input; and the emulated indexed plan of tests/emu_index
must accept every piece -- it accepts a piece only if its window length and check value are exact.
"""
import ctypes as C
import os
import random
import struct
import subprocess
import sys
import zlib

import pytest

from zsc_amd import corpus
import test_inflate_index_emu as tix
from test_inflate_index_emu import HEADER, H_FIELDS, POINT, covering_run, indexed, points, reseal, windows

HERE = os.path.dirname(os.path.abspath(__file__))
Z_BUF_ERROR = -5
Z_DEFAULT_STRATEGY, Z_HUFFMAN_ONLY, Z_RLE, Z_FIXED = 0, 2, 3, 4
BT_STORED = 0
BIG = 300000
MAX_DIST = 32768 - 262  # w_size - MIN_LOOKAHEAD: deflate emits no distance beyond it, so no window is longer
PERIOD = MAX_DIST - 1    # the longest period at which the parser still finds the repeat (at MAX_DIST it finds none)


def load(name):
    L = C.CDLL(os.path.join(HERE, "emu_dindex", name))
    L.emu_dindex_compress.argtypes = [C.c_char_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32,
                                      C.c_uint32, C.c_char_p, C.POINTER(C.c_uint32), C.c_char_p, C.c_uint64,
                                      C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_uint32,
                                      C.POINTER(C.c_uint32)]
    return L


@pytest.fixture(scope="module")
def dix():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_dindex")], check=True)
    return load("libdix_emu64.so")


@pytest.fixture(scope="module")
def idx():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_index")], check=True)
    return tix.load("libidx_emu16.so")


def compress(L, data, level, wbits, mem_level, strategy, chunk, out_cap):
    """(status, stream, blob or None, [(bit_off, in_begin, in_len, type)])"""
    out = C.create_string_buffer(max(out_cap, 1) + 64)
    blob = C.create_string_buffer(HEADER + (out_cap // max(chunk, 256) + 2) * (POINT + 32768))
    max_blocks = len(data) // ((1 << (mem_level + 6)) - 1) + 2
    blocks = (C.c_uint32 * (4 * max_blocks))()
    ol, bl, nb = C.c_uint32(), C.c_uint64(), C.c_uint32()
    rc = L.emu_dindex_compress(data, len(data), level, wbits, mem_level, strategy, chunk, out_cap, out, C.byref(ol),
                               blob, len(blob), C.byref(bl), blocks, max_blocks, C.byref(nb))
    assert bl.value <= len(blob) and nb.value <= max_blocks
    blist = [tuple(blocks[4 * i:4 * i + 4]) for i in range(nb.value)]
    return rc, out.raw[:ol.value] if rc == 0 else b"", (blob.raw[:bl.value] if bl.value else None), blist


_BUFFERS = {}


def buffer(kind, size, seed):
    key = (kind, size, seed)
    if key not in _BUFFERS:
        if kind == "mix":
            third = size // 3
            _BUFFERS[key] = (corpus.make_buffer("text", third, seed) + corpus.make_buffer("random", third, seed + 1) +
                             corpus.make_buffer("zero", size - 2 * third, seed + 2))
        elif kind == "period":  # random bytes repeated: every match lies one period back
            _BUFFERS[key] = (corpus.make_buffer("random", PERIOD, seed) * (size // PERIOD + 1))[:size]
        else:
            _BUFFERS[key] = corpus.make_buffer(kind, size, seed)
    return _BUFFERS[key]


# (kind, size, seed, level, window_bits, mem_level, strategy, chunk_bytes)
CASES = [
    ("text", BIG, 11, 6, 15, 8, Z_DEFAULT_STRATEGY, 256),
    ("random", BIG, 12, 6, 15, 8, Z_DEFAULT_STRATEGY, 256),
    ("zero", BIG, 13, 6, 15, 8, Z_DEFAULT_STRATEGY, 256),
    ("zero", BIG, 13, 6, 15, 1, Z_DEFAULT_STRATEGY, 256),
    ("period", BIG, 17, 6, 15, 1, Z_DEFAULT_STRATEGY, 256),
    ("mix", BIG, 14, 6, 31, 8, Z_DEFAULT_STRATEGY, 1024),
    ("text", BIG, 11, 1, -15, 8, Z_DEFAULT_STRATEGY, 8192),
    ("text", BIG, 11, 9, 31, 8, Z_DEFAULT_STRATEGY, 1024),
    ("mix", BIG, 14, 9, 9, 8, Z_DEFAULT_STRATEGY, 256),
    ("text", BIG, 11, 6, 9, 8, Z_DEFAULT_STRATEGY, 1024),
    ("text", BIG, 11, 6, 15, 8, Z_RLE, 1024),
    ("mix", BIG, 14, 9, 31, 8, Z_RLE, 256),
    ("text", BIG, 11, 6, -15, 8, Z_HUFFMAN_ONLY, 8192),
    ("mix", BIG, 14, 1, 31, 8, Z_FIXED, 256),
    ("text", BIG, 11, 6, 15, 1, Z_DEFAULT_STRATEGY, 256),  # mem_level 1: blocks of 127 symbols
    ("mix", BIG, 14, 1, -15, 1, Z_DEFAULT_STRATEGY, 1024),
    ("random", BIG, 12, 9, -15, 8, Z_DEFAULT_STRATEGY, 8192),
    ("zero", BIG, 13, 1, 31, 8, Z_DEFAULT_STRATEGY, 1024),
] + [(kind, size, 20 + size % 7, level, wbits, 8, Z_DEFAULT_STRATEGY, 256)
     for size in (0, 1, 3072)
     for kind, level, wbits in (("text", 6, 15), ("random", 1, 31), ("zero", 9, -15), ("mix", 6, 9))]


def case_id(c):
    return "-".join(str(x) for x in c)


def expected_bits(blocks, chunk):
    """bit 0, plus the first block with input in every later chunk"""
    first = {}
    for bit, _, in_len, _ in blocks[1:]:
        if in_len > 0:
            first.setdefault(bit // (8 * chunk), bit)
    return [0] + [bit for ch, bit in sorted(first.items()) if ch > 0]


def check_case(dix, idx, oracle, case):
    """assertions 1-4 and 6 of one case; returns (stream, blob, points, blocks)"""
    kind, size, seed, level, wbits, mem_level, strategy, chunk = case
    data = buffer(kind, size, seed)
    orc, want, _ = oracle.compress(data, level, window_bits=wbits, mem_level=mem_level, strategy=strategy)
    assert orc == 0
    cap = oracle.max_output(len(data), max(len(data), 1), level, wbits, mem_level)[1]
    rc, stream, blob, blocks = compress(dix, data, level, wbits, mem_level, strategy, chunk, cap)
    # 1. the oracle's stream
    assert rc == 0 and stream == want
    # 2. a valid blob with the specified header
    assert blob is not None and idx.emu_idx_validate(blob, len(blob)) == 1
    assert reseal(blob) == blob
    h = {f: struct.unpack_from("<I", blob, at)[0] for f, at in H_FIELDS.items()}
    kind_of = 0 if wbits < 0 else 2 if wbits > 15 else 1
    assert (h["total"], h["consumed"], h["chunk_bytes"]) == (len(data), len(stream), chunk)
    assert h["trailer"] == len(stream) - (0, 4, 8)[kind_of] and h["kind"] == kind_of
    assert C.c_int32(h["window_bits"]).value == wbits
    assert h["head"] == ((1 | 15 << 8) if kind_of == 2 else (wbits << 8) if kind_of == 1 else 15 << 8)
    # 3. the points, from the documented layout
    pts = points(blob)
    assert h["npoints"] == len(pts) and HEADER + POINT * len(pts) + sum(p["wlen"] for p in pts) == len(blob)
    off = 0
    for p, w in zip(pts, windows(blob, pts)):
        assert p["off"] == off
        piece = data[off:off + p["len"]]
        assert p["check"] == (zlib.crc32(piece) if kind_of == 2 else zlib.adler32(piece))
        assert p["wlen"] <= min(off, 32768) and w == data[off - p["wlen"]:off]
        off += p["len"]
    assert off == len(data)
    assert [p["bit"] for p in pts] == expected_bits(blocks, chunk)
    begins = {bit: in_begin for bit, in_begin, _, _ in blocks}
    assert all(p["off"] == begins[p["bit"]] for p in pts[1:])
    # 4. every piece accepted by the indexed plan
    assert indexed(idx, stream, len(data), wbits, blob) == (0, data, len(stream), len(pts))
    # 6. the short buffers: one point
    if size <= 3072:
        assert len(pts) == 1
    return stream, blob, pts, blocks


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_round_trip(dix, idx, oracle, case):
    stream, blob, pts, blocks = check_case(dix, idx, oracle, case)
    kind, size, _, level, wbits, mem_level, strategy, chunk = case
    # 5. what the kinds of data must show at the finest chunk size.  The longest window: a window is as
    # long as the piece's farthest distance, and deflate emits none beyond MAX_DIST = 32 506 (a window of
    # 32 768 bytes, the format's limit, cannot come from this encoder); text comes close to it, the
    # periodic buffer has pieces that start with the farthest match the parser finds.  300 KB of zeros are one block unless the blocks are short (mem_level 1).
    if (size, level, wbits, strategy, chunk) == (BIG, 6, 15, Z_DEFAULT_STRATEGY, 256):
        types = {bit: t for bit, _, _, t in blocks}
        assert all(p["wlen"] <= MAX_DIST for p in pts)
        if kind == "text" and mem_level == 8:
            assert len(pts) >= 4 and all(30000 < p["wlen"] for p in pts[1:-1])
        elif kind == "period":
            assert len(pts) >= 4 and any(p["wlen"] == PERIOD for p in pts)
        elif kind == "random":
            at_stored = [p for p in pts[1:] if types[p["bit"]] == BT_STORED]
            assert at_stored and all(p["wlen"] == 0 for p in at_stored)
        elif kind == "zero" and mem_level == 1:
            assert any(p["wlen"] == 1 for p in pts[1:])


def test_short_out_cap(dix, oracle):
    """7. one byte short: Z_BUF_ERROR and no blob"""
    for kind, size in (("text", BIG), ("random", 3072), ("text", 0)):
        data = buffer(kind, size, 11)
        want = oracle.compress(data, 6)[1]
        rc, stream, blob, _ = compress(dix, data, 6, 15, 8, 0, 256, len(want) - 1)
        assert (rc, stream, blob) == (Z_BUF_ERROR, b"", None)
        rc, stream, blob, _ = compress(dix, data, 6, 15, 8, 0, 256, len(want))
        assert (rc, stream) == (0, want) and blob is not None


def test_ranges(dix, idx, oracle):
    """ranges out of the middle of a stream, from a deflate plan's blob"""
    text = buffer("text", BIG, 11)
    for wbits in (15, 31, -15):
        cap = oracle.max_output(len(text), len(text), 6, wbits, 8)[1]
        rc, s, blob, _ = compress(dix, text, 6, wbits, 8, 0, 8192, cap)
        assert rc == 0
        pts = points(blob)
        assert len(pts) >= 4
        rnd = random.Random(78)
        ranges = []
        for _ in range(20):
            b = rnd.randrange(len(text))
            ranges.append((b, rnd.randrange(1, min(len(text) - b, 120000) + 1)))
        edge = pts[len(pts) // 2]["off"]
        ranges += [(edge - 1, 1), (edge, 1), (edge - 1, 2)]
        for b, n in ranges:
            want = covering_run(pts, b, n)
            got = (C.c_uint32 * 4)()
            assert idx.emu_idx_range(blob, len(blob), b, n, got) == 1
            assert tuple(got) == want, (b, n)
            first, count, pbegin, plen = want
            rc, data, used, np_ = indexed(idx, s, plen, wbits, blob, (b, n))
            assert (rc, np_) == (0, count), (b, n)
            assert data == text[pbegin:pbegin + plen], (b, n)
            last = first + count
            end_bit = pts[last]["bit"] if last < len(pts) else 8 * struct.unpack_from("<I", blob, H_FIELDS["trailer"])[0]
            assert used == (end_bit + 7) // 8, (b, n)


ASAN_CASES = [c for c in CASES if c[1] <= 3072] + [CASES[0], CASES[3], CASES[6], CASES[12]]

ASAN_CHILD = """
import sys
sys.path[:0] = {paths!r}
import test_deflate_index_emu as t
import test_inflate_index_emu as tix
from oracle.oracle_py import Oracle
dix, idx, oracle = t.load("libdix_emu64_asan.so"), tix.load("libidx_emu16_asan.so"), Oracle()
for case in t.ASAN_CASES:
    t.check_case(dix, idx, oracle, case)
t.test_short_out_cap(dix, oracle)
print("deflate index round trip under AddressSanitizer: ok")
"""


def test_round_trip_under_address_sanitizer():
    """The round trip once more on builds of both emulations with AddressSanitizer (host code only), in a
    child process with the sanitizer's runtime preloaded: an access outside the drivers' allocations ends it."""
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_dindex"), "asan"], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_index"), "asan"], check=True)
    rt = subprocess.run(["g++", "-print-file-name=libasan.so"], check=True, capture_output=True, text=True).stdout.strip()
    assert os.path.isabs(rt), "no AddressSanitizer runtime beside the compiler"
    env = dict(os.environ)
    env["LD_PRELOAD"] = " ".join(filter(None, [rt, env.get("LD_PRELOAD", "")]))
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=0:exitcode=66:verify_asan_link_order=0"
    code = ASAN_CHILD.format(paths=[os.path.dirname(HERE), HERE])
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0 and "ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
