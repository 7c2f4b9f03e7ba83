"""The indexed inflate path (zsc_amd/csrc/inflate_index.h) on the lane emulation, against the oracle.

tests/emu_index builds the path's kernel sources with -DZSC_WAVE_EMU at 16 and at 64 lanes.  Its driver
runs the chunks path with the index enabled and exports the blob, then the indexed path: the write
worker, finish and the serial decoder for what is left, as the runtime enqueues them.  Every whole-stream
decode must give the oracle's (status, bytes, consumed) whatever the blob holds; a damaged blob must
leave the stream to the serial decoder (0 pieces).  The blobs are taken apart and put together here from
the layout documented in include/zsc_hip.h, not with the library's own routines.
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
from test_inflate_chunks_emu import CHUNK, make_cases, zlib_stream

HERE = os.path.dirname(os.path.abspath(__file__))
Z_DATA_ERROR = -3
REFUSED = -100  # the driver's answer where create refuses the plan

# the documented layout
HEADER, POINT = 48, 32
H_FIELDS = {"magic": 0, "version": 4, "crc": 8, "window_bits": 12, "kind": 16, "head": 20, "chunk_bytes": 24,
            "consumed": 28, "total": 32, "trailer": 36, "npoints": 40, "reserved": 44}
P_FIELDS = {"bit": (0, 8), "woff": (8, 8), "off": (16, 4), "len": (20, 4), "check": (24, 4), "wlen": (28, 4)}


def load(name):
    L = C.CDLL(os.path.join(HERE, "emu_index", name))
    L.emu_idx_validate.argtypes = [C.c_char_p, C.c_uint64]
    L.emu_idx_info.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(C.c_uint32)]
    L.emu_idx_range.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32)]
    L.emu_idx_build.argtypes = [C.c_char_p, C.c_uint32, C.c_int, C.c_char_p, C.c_uint32, C.c_uint32,
                                C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_char_p,
                                C.c_uint64, C.POINTER(C.c_uint64)]
    L.emu_idx_uncompress.argtypes = [C.c_char_p, C.c_uint32, C.c_int, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint64,
                                     C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                     C.POINTER(C.c_uint32)]
    return L


@pytest.fixture(scope="module", params=["libidx_emu16.so", "libidx_emu64.so"], ids=["group16", "wave64"])
def idx(request):
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_index")], check=True)
    return load(request.param)


def build(L, data, cap, wbits, chunk=CHUNK):
    """the chunks plan with the index enabled: (rc, out, used, pieces, blob or None)"""
    out = C.create_string_buffer(max(cap, 1))
    blob = C.create_string_buffer(HEADER + (len(data) // chunk + 2) * (POINT + 32768))
    ol, used, npieces, bl = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
    rc = L.emu_idx_build(data, len(data), wbits, out, cap, chunk, C.byref(ol), C.byref(used), C.byref(npieces), blob,
                         len(blob), C.byref(bl))
    assert bl.value <= len(blob)
    return rc, out.raw[:ol.value], used.value, npieces.value, (blob.raw[:bl.value] if bl.value else None)


def indexed(L, data, cap, wbits, blob, rng=None):
    out = C.create_string_buffer(max(cap, 1))
    ol, used, npieces = C.c_uint32(), C.c_uint32(), C.c_uint32()
    rc = L.emu_idx_uncompress(data, len(data), wbits, out, cap, blob, len(blob) if blob else 0, rng is not None,
                              rng[0] if rng else 0, rng[1] if rng else 0, C.byref(ol), C.byref(used), C.byref(npieces))
    return rc, out.raw[:ol.value], used.value, npieces.value


def info(L, blob):
    v = (C.c_uint32 * 8)()
    if not L.emu_idx_info(blob, len(blob), v):
        return None
    return dict(zip(("window_bits", "kind", "head", "chunk_bytes", "consumed", "total", "trailer", "npoints"), v))


# ---- blobs by the documented format ----

def reseal(blob):
    return blob[:8] + struct.pack("<I", zlib.crc32(blob[12:])) + blob[12:]


def flip(blob, at, bit):
    b = bytearray(blob)
    b[at + bit // 8] ^= 1 << (bit % 8)
    return bytes(b)


def points(blob):
    n = struct.unpack_from("<I", blob, H_FIELDS["npoints"])[0]
    return [dict(zip(("bit", "woff", "off", "len", "check", "wlen"),
                     struct.unpack_from("<QQIIII", blob, HEADER + POINT * i))) for i in range(n)]


def assemble(blob, pts, wins):
    """the header of `blob` with these points and windows, laid out as documented, sealed"""
    out = bytearray(blob[:HEADER])
    struct.pack_into("<I", out, H_FIELDS["npoints"], len(pts))
    at = HEADER + POINT * len(pts)
    for p, w in zip(pts, wins):
        out += struct.pack("<QQIIII", p["bit"], at, p["off"], p["len"], p["check"], len(w))
        at += len(w)
    return reseal(bytes(out) + b"".join(wins))


def windows(blob, pts):
    return [blob[p["woff"]:p["woff"] + p["wlen"]] for p in pts]


def test_round_trip(idx, oracle):
    took = 0
    for name, stream, cap, wbits, _ in make_cases(oracle):
        want = oracle.uncompress(stream, cap, window_bits=wbits)
        rc, out, used, npieces, blob = build(idx, stream, cap, wbits)
        assert (rc, out, used) == want, name
        if npieces == 0:
            assert blob is None, name  # "no index"
            assert indexed(idx, stream, cap, wbits, None) == want + (0,), name
            continue
        assert npieces > 1 and blob is not None, name
        assert idx.emu_idx_validate(blob, len(blob)) == 1, name
        h = info(idx, blob)
        assert (h["total"], h["consumed"], h["npoints"]) == (len(out), used, npieces), name
        assert h["chunk_bytes"] == CHUNK and C.c_int32(h["window_bits"]).value == wbits, name
        # the documented layout: a stale CRC is found, a recomputed one is the library's
        assert reseal(blob) == blob, name
        pts = points(blob)
        assert all(p["wlen"] <= min(p["off"], 32768) for p in pts) and pts[0]["wlen"] == 0, name
        assert indexed(idx, stream, cap, wbits, blob) == want + (npieces,), name
        took += 1
    assert took > 25


def many_piece_streams(oracle):
    text = corpus.make_buffer("text", 300000, 11)
    other = corpus.make_buffer("text", 300000, 12)
    return [(f"w{wbits}", zlib_stream(text, 6, wbits), zlib_stream(other, 6, wbits), len(text), wbits)
            for wbits in (15, 31, -15)]


def damaged_blobs(blob):
    """[(what, blob)] -- every one must leave the stream to the serial decoder"""
    out = []
    for n in (0, 1, 11, HEADER - 1, HEADER, HEADER + POINT - 1, HEADER + POINT, len(blob) // 2, len(blob) - 1):
        out.append((f"truncated-{n}", blob[:n]))
    pts = points(blob)
    n = len(pts)
    assert n >= 4
    # One bit in each header field; the bit is the field's lowest, except where that would give another
    # true index of the same stream: chunk_bytes only says how the points are told apart (its top set bit
    # is flipped: 0 is no chunk size), and the reserved word has no meaning at all (any bit must fail).
    hbit = {f: 0 for f in H_FIELDS}
    hbit["chunk_bytes"] = struct.unpack_from("<I", blob, H_FIELDS["chunk_bytes"])[0].bit_length() - 1
    for f, at in H_FIELDS.items():
        out.append((f"header-{f}-stale", flip(blob, at, hbit[f])))
        if f != "crc":  # (a recomputed CRC would undo the flip)
            out.append((f"header-{f}-sealed", reseal(flip(blob, at, hbit[f]))))
    for which, i in (("first", 0), ("middle", n // 2), ("last", n - 1)):
        for f, (at, _) in P_FIELDS.items():
            d = flip(blob, HEADER + POINT * i + at, 0)
            out.append((f"point-{which}-{f}-stale", d))
            out.append((f"point-{which}-{f}-sealed", reseal(d)))
    wins = windows(blob, pts)
    k = next(i for i in range(1, n) if pts[i]["wlen"] > 8)
    out.append(("window-byte", reseal(flip(blob, pts[k]["woff"] + pts[k]["wlen"] - 1, 0))))
    out.append(("window-first-byte", reseal(flip(blob, pts[k]["woff"], 3))))
    # a window length changed alone, and changed with the layout kept consistent
    for delta in (-1, 1):
        d = bytearray(blob)
        struct.pack_into("<I", d, HEADER + POINT * k + P_FIELDS["wlen"][0], pts[k]["wlen"] + delta)
        out.append((f"wlen{delta:+d}-field", reseal(bytes(d))))
    w2 = list(wins)
    w2[k] = wins[k][1:]
    out.append(("wlen-shortened", assemble(blob, pts, w2)))
    if pts[k]["wlen"] < min(pts[k]["off"], 32768):
        w2[k] = b"\x00" + wins[k]
        out.append(("wlen-lengthened", assemble(blob, pts, w2)))
    p2, w2 = list(pts), list(wins)
    p2[k], p2[k + 1], w2[k], w2[k + 1] = p2[k + 1], p2[k], w2[k + 1], w2[k]
    out.append(("points-swapped", assemble(blob, p2, w2)))
    for delta in (-1, 1):
        p2 = [dict(p) for p in pts]
        p2[k]["bit"] += delta
        out.append((f"bit{delta:+d}", assemble(blob, p2, wins)))
    return out


def test_untrusted_blobs(idx, oracle):
    run_untrusted(idx, oracle)


def run_untrusted(L, oracle):
    for name, stream, sibling, cap, wbits in many_piece_streams(oracle):
        want = oracle.uncompress(stream, cap, window_bits=wbits)
        rc, out, used, npieces, blob = build(L, stream, cap, wbits)
        assert (rc, out, used) == want and npieces >= 4, name
        assert indexed(L, stream, cap, wbits, blob) == want + (npieces,), name
        for what, bad in damaged_blobs(blob):
            got = indexed(L, stream, cap, wbits, bad)
            assert got == want + (0,), (name, what, got[0], len(got[1]), got[2], got[3])
        # the blob of another stream of equal length
        n = max(len(stream), len(sibling))
        a, b = stream + bytes(n - len(stream)), sibling + bytes(n - len(sibling))
        other = build(L, b, cap, wbits)[4]
        assert other is not None
        assert indexed(L, a, cap, wbits, other) == oracle.uncompress(a, cap, window_bits=wbits) + (0,), name
        # another window_bits, a short dest_cap
        w2 = {15: 31, 31: 15, -15: 15}[wbits]
        assert indexed(L, stream, cap, w2, blob) == oracle.uncompress(stream, cap, window_bits=w2) + (0,), name
        assert indexed(L, stream, cap - 1, wbits, blob) == oracle.uncompress(stream, cap - 1, window_bits=wbits) + (0,), name
        # a valid blob, the stream truncated; then junk appended (parallel: consumed is the trailer's end)
        for cut in (1, 5, len(stream) // 3):
            t = stream[:-cut]
            assert indexed(L, t, cap, wbits, blob) == oracle.uncompress(t, cap, window_bits=wbits) + (0,), (name, cut)
        j = stream + b"\x01\x02junk after the trailer"
        assert indexed(L, j, cap, wbits, blob) == (0, out, len(stream), npieces), name
        assert oracle.uncompress(j, cap, window_bits=wbits) == (0, out, len(stream)), name


def covering_run(pts, begin, n):
    """the minimal run of whole pieces that covers [begin, begin + n), from the points alone"""
    hit = [i for i, p in enumerate(pts) if p["len"] and p["off"] < begin + n and p["off"] + p["len"] > begin]
    return hit[0], hit[-1] - hit[0] + 1, pts[hit[0]]["off"], pts[hit[-1]]["off"] + pts[hit[-1]]["len"] - pts[hit[0]]["off"]


def test_ranges(idx, oracle):
    text = corpus.make_buffer("text", 400000, 21)
    for wbits in (15, 31, -15):
        s = zlib_stream(text, 6, wbits)
        rc, out, used, npieces, blob = build(idx, s, len(text), wbits)
        assert (rc, out) == (0, text) and npieces >= 4
        pts = points(blob)
        rnd = random.Random(77)
        ranges = []
        for _ in range(50):
            b = rnd.randrange(len(text))
            ranges.append((b, rnd.randrange(1, min(len(text) - b, 120000) + 1)))
        ranges += [(0, 1), (len(text) - 1, 1), (0, len(text))]
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
        # a damaged window, the CRC recomputed: Z_DATA_ERROR and nothing
        k = len(pts) // 2
        assert pts[k]["wlen"] > 0
        bad = reseal(flip(blob, pts[k]["woff"] + pts[k]["wlen"] - 1, 0))
        assert indexed(idx, s, pts[k]["len"], wbits, bad, (pts[k]["off"], 1)) == (Z_DATA_ERROR, b"", 0, 0)
        # ... as a range item on a stream without a valid index
        assert indexed(idx, s, 100, wbits, blob[:-1], (0, 1)) == (Z_DATA_ERROR, b"", 0, 0)
        assert indexed(idx, s, 100, wbits, None, (0, 1)) == (Z_DATA_ERROR, b"", 0, 0)
        # past the end, or empty: refused at create
        got = (C.c_uint32 * 4)()
        for b, n in ((len(text), 1), (len(text) - 1, 2), (0, len(text) + 1), (5, 0)):
            assert idx.emu_idx_range(blob, len(blob), b, n, got) == 0
            assert indexed(idx, s, len(text), wbits, blob, (b, n))[0] == REFUSED


ASAN_CHILD = """
import sys
sys.path[:0] = {paths!r}
import test_inflate_index_emu as t
from oracle.oracle_py import Oracle
t.run_untrusted(t.load("libidx_emu16_asan.so"), Oracle())
print("untrusted blobs under AddressSanitizer: ok")
"""


def test_untrusted_blobs_under_address_sanitizer():
    """The untrusted-blob cases once more on a build of the emulation with AddressSanitizer, in a child
    process with the sanitizer's runtime preloaded: an access outside the driver's allocations ends it."""
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_index"), "asan"], check=True)
    rt = subprocess.run(["g++", "-print-file-name=libasan.so"], check=True, capture_output=True, text=True).stdout.strip()
    assert os.path.isabs(rt), "no AddressSanitizer runtime beside the compiler"
    env = dict(os.environ)
    env["LD_PRELOAD"] = " ".join(filter(None, [rt, env.get("LD_PRELOAD", "")]))
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=0:exitcode=66:verify_asan_link_order=0"
    code = ASAN_CHILD.format(paths=[os.path.dirname(HERE), HERE])
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0 and "ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
