"""The sections inflate path (zsc_amd/csrc/inflate_sections.h) on the lane emulation, against the oracle.

tests/emu_sections builds the path's kernel sources with -DZSC_WAVE_EMU at 16 lanes (the decoder's
group width on the GPU) and 64 lanes; its driver runs scan -> setup -> scan -> count -> resolve -> write
-> finish and then the serial decoder for a stream that did not finish, as the runtime enqueues them.
Every case must give the oracle's (status, bytes, consumed), and the number of sections decoded in
parallel must be the expected one.  make_cases() is shared with tests/test_gpu_inflate_sections.py.
"""
import ctypes as C
import os
import random
import struct
import subprocess
import zlib

import pytest

from zsc_amd import corpus

HERE = os.path.dirname(os.path.abspath(__file__))
MARK = b"\x00\x00\xff\xff"
ANY = None  # section count not predicted: only the results are checked


@pytest.fixture(scope="module", params=["libsec_emu16.so", "libsec_emu64.so"], ids=["group16", "wave64"])
def sec(request):
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_sections")], check=True)
    L = C.CDLL(os.path.join(HERE, "emu_sections", request.param))
    L.emu_sec_crc32_combine.restype = C.c_uint32
    L.emu_sec_crc32_combine.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    L.emu_sec_adler32_combine.restype = C.c_uint32
    L.emu_sec_adler32_combine.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    L.emu_sec_set_work_bound.argtypes = [C.c_uint32, C.c_uint32]
    L.emu_sec_set_pool.argtypes = [C.c_uint32]
    return L


def emu_uncompress(L, data, cap, window_bits):
    out = C.create_string_buffer(max(cap, 1))
    ol, used, nsec, ncand = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    rc = L.emu_sec_uncompress(data, len(data), window_bits, out, cap, C.byref(ol), C.byref(used),
                              C.byref(nsec), C.byref(ncand))
    return rc, out.raw[:ol.value], used.value, nsec.value


def zlib_flushed(data, pieces, level, wbits, flush):
    """a stock-zlib stream with `flush` after each of `pieces` (byte counts); the rest with Z_FINISH"""
    co = zlib.compressobj(level, zlib.DEFLATED, wbits)
    out, at = [], 0
    for p in pieces:
        out.append(co.compress(data[at:at + p]) + co.flush(flush))
        at += p
    out.append(co.compress(data[at:]) + co.flush())
    return b"".join(out)


def markers_plus_one(stream):
    k = stream.count(MARK)
    return k + 1 if k else 0


def make_cases(oracle, seed=1, n_oracle=150, max_len=24000):
    """[(name, stream, dest_cap, window_bits, expected sections or ANY)]"""
    rnd = random.Random(seed)
    cases = []
    kinds = ("text", "table", "token", "bitmap", "object")
    # oracle-made streams: levels 0-9, zlib / gzip / raw, window_bits 9-15, max_block_len from 1 KiB up
    for i in range(n_oracle):
        kind = kinds[i % len(kinds)]
        n = rnd.randrange(1, max_len)
        data = corpus.make_buffer(kind, n, 100 + i)
        level = i % 10
        wb = rnd.choice(list(range(9, 16)))
        wrap = i % 3
        wbits = wb if wrap == 0 else (wb + 16 if wrap == 1 else -wb)
        mbl = rnd.choice([1024, 2048, 4096, 10000, 65536, n + 1])
        rc, comp, _ = oracle.compress(data, level, window_bits=wbits, max_block_len=mbl)
        assert rc == 0, (i, rc)
        # (stored data may hold the pattern; compressed data at these sizes does not)
        want = ANY if level == 0 or kind == "bitmap" else markers_plus_one(comp)
        cases.append((f"oracle-{kind}-l{level}-w{wbits}-m{mbl}", comp, n, wbits, want))
    text = corpus.make_buffer("text", 60000, 7)
    # stock zlib, Z_FULL_FLUSH: sections = flushes + 1
    for wbits in (15, 31, -15):
        for level in (1, 6, 9):
            pieces = [rnd.randrange(500, 9000) for _ in range(rnd.randrange(1, 9))]
            s = zlib_flushed(text, pieces, level, wbits, zlib.Z_FULL_FLUSH)
            cases.append((f"zlib-full-l{level}-w{wbits}", s, len(text), wbits, len(pieces) + 1))
    # Z_SYNC_FLUSH on repetitive text: the sections need each other's history, all serial
    rep = (b"the quick brown fox jumps over the lazy dog; " * 1500)[:60000]
    for wbits in (15, 31):
        s = zlib_flushed(rep, [4000] * 10, 6, wbits, zlib.Z_SYNC_FLUSH)
        cases.append((f"zlib-sync-w{wbits}", s, len(rep), wbits, 0))
    # stored data dense with the pattern: the candidate list overflows
    dense = MARK * 5000
    rc, s, _ = oracle.compress(dense, 0, max_block_len=4096)
    cases.append(("stored-dense", s, len(dense), 15, 0))
    # stored data with the pattern every 97 bytes (false candidates that decode as something)
    sparse = bytearray(corpus.make_buffer("text", 30000, 9))
    for p in range(50, len(sparse) - 8, 97):
        sparse[p:p + 5] = MARK + b"\x00"
    rc, s, _ = oracle.compress(bytes(sparse), 0, max_block_len=4096)
    cases.append(("stored-sparse", s, len(sparse), 15, ANY))
    rc, s, _ = oracle.compress(bytes(sparse), 6, max_block_len=4096)
    cases.append(("deflated-sparse", s, len(sparse), 15, ANY))
    # gzip header with the pattern in FEXTRA and across FEXTRA / FNAME (a NUL ends FNAME and FCOMMENT)
    body = zlib_flushed(text, [7000, 7000, 7000], 6, -15, zlib.Z_FULL_FLUSH)
    extra = b"AB" + struct.pack("<H", 10) + MARK * 2 + b"\0\0"
    hdr = b"\x1f\x8b\x08" + bytes([0x04 | 0x08 | 0x10]) + b"\0\0\0\0\0\x03" + struct.pack("<H", len(extra)) + extra
    hdr += b"\xff\xffname\0" + b"comment\0"
    trailer = struct.pack("<II", zlib.crc32(text), len(text))
    cases.append(("gzip-fields", hdr + body + trailer, len(text), 31, 4))
    hcrc = hdr[:3] + bytes([hdr[3] | 0x02]) + hdr[4:]
    hcrc += struct.pack("<H", zlib.crc32(hcrc) & 0xffff)
    cases.append(("gzip-fhcrc", hcrc + body + trailer, len(text), 31, 4))
    zs = zlib_flushed(text, [10000, 10000], 6, 15, zlib.Z_FULL_FLUSH)
    # FDICT
    cz = zlib.compressobj(6, zlib.DEFLATED, 15, zdict=b"the dictionary")
    fd = cz.compress(text[:20000]) + cz.flush(zlib.Z_FULL_FLUSH) + cz.compress(text[20000:]) + cz.flush()
    cases.append(("fdict", fd, len(text), 15, 0))
    # junk after the trailer (parallel; consumed ends at the trailer)
    cases.append(("junk-after", zs + b"\x01\x02junk" + MARK + b"junk", len(text), 15, 3))
    # truncation: in the last section, in the trailer
    cases.append(("truncated-body", zs[:len(zs) - 200], len(text), 15, 0))
    cases.append(("truncated-trailer", zs[:-2], len(text), 15, 0))
    # short dest_cap
    cases.append(("short-cap", zs, len(text) - 1, 15, 0))
    cases.append(("tiny-cap", zs, 100, 15, 0))
    # a wrong trailer
    cases.append(("bad-adler", zs[:-1] + bytes([zs[-1] ^ 1]), len(text), 15, 0))
    gz = zlib_flushed(text, [10000, 10000], 6, 31, zlib.Z_FULL_FLUSH)
    cases.append(("bad-isize", gz[:-4] + struct.pack("<I", len(text) + 1), len(text), 31, 0))
    # a corrupted middle section: Z_DATA_ERROR and resynchronisation, by the serial decoder
    marks = [i for i in range(len(zs)) if zs.startswith(MARK, i)]
    mid = (marks[0] + marks[1]) // 2
    bad = bytearray(zs)
    for j in range(mid, mid + 6):
        bad[j] ^= 0x5a
    cases.append(("corrupt-middle", bytes(bad), len(text), 15, 0))
    # the header's window (1 KiB) is smaller than a later section's distances: serial (a data error)
    small = text[:300]
    s = zlib_flushed(small + text, [300], 6, 15, zlib.Z_FULL_FLUSH)
    cmf = 0x28
    flg = (31 - (cmf * 256) % 31) % 31
    cases.append(("dmax-later-section", bytes([cmf, flg]) + s[2:], len(small) + len(text), 15, 0))
    # empty input, empty output
    cases.append(("empty-input", b"", 10, 15, 0))
    e = zlib_flushed(b"", [], 6, 15, zlib.Z_FULL_FLUSH)
    cases.append(("empty-output", e, 0, 15, 0))
    e2 = zlib_flushed(b"abc", [3], 6, 15, zlib.Z_FULL_FLUSH)
    cases.append(("flush-then-empty-final", e2, 3, 15, 2))
    return cases


def test_crc32_and_adler32_combine(sec, oracle):
    rnd = random.Random(5)
    for la, lb in [(0, 0), (0, 7), (9, 0), (1, 1), (5551, 1), (5552, 0), (5552, 5552), (5553, 5551),
                   (3, 5552), (11104, 5553), (40000, 70000), (65536, 65536), (100, 1 << 20)]:
        a = bytes(rnd.randrange(256) for _ in range(min(la, 5000))) * (la // 5000 + 1)
        b = bytes(rnd.randrange(256) for _ in range(min(lb, 5000))) * (lb // 5000 + 1)
        a, b = a[:la], b[:lb]
        assert sec.emu_sec_crc32_combine(oracle.crc32(a), oracle.crc32(b), lb) == oracle.crc32(a + b), (la, lb)
        assert sec.emu_sec_adler32_combine(oracle.adler32(a), oracle.adler32(b), lb) == oracle.adler32(a + b), (la, lb)
    # all-0xff bytes: the Adler sums at their largest
    ff = b"\xff" * 5552
    assert sec.emu_sec_adler32_combine(oracle.adler32(ff), oracle.adler32(ff), 5552) == oracle.adler32(ff * 2)


def test_sections_equal_the_oracle(sec, oracle):
    cases = make_cases(oracle)
    assert len(cases) > 150
    parallel = 0
    for name, stream, cap, wbits, want in cases:
        rc, out, used, nsec = emu_uncompress(sec, stream, cap, wbits)
        orc, oout, oused = oracle.uncompress(stream, cap, window_bits=wbits)
        assert (rc, out, used) == (orc, oout, oused), (name, rc, orc, len(out), len(oout), used, oused)
        if want is not ANY:
            assert nsec == want, (name, nsec, want)
        if nsec:
            assert rc == 0, name
            parallel += 1
    assert parallel > 60


def test_work_bound_sends_the_stream_serial(sec, oracle):
    text = corpus.make_buffer("text", 60000, 3)
    s = zlib_flushed(text, [8000] * 5, 6, 15, zlib.Z_FULL_FLUSH)
    assert emu_uncompress(sec, s, len(text), 15)[3] == 6
    try:
        sec.emu_sec_set_work_bound(0, 64)
        rc, out, used, nsec = emu_uncompress(sec, s, len(text), 15)
        assert nsec == 0
        assert (rc, out, used) == oracle.uncompress(s, len(text))
    finally:
        sec.emu_sec_set_work_bound(4, 65536)


def test_candidate_pool_used_up_sends_the_stream_serial(sec, oracle):
    text = corpus.make_buffer("text", 60000, 4)
    s = zlib_flushed(text, [6000] * 7, 6, 31, zlib.Z_FULL_FLUSH)
    assert emu_uncompress(sec, s, len(text), 31)[3] == 8
    try:
        for slots in (1, 7, 8):  # the stream needs 8 (7 markers and its start)
            sec.emu_sec_set_pool(slots)
            rc, out, used, nsec = emu_uncompress(sec, s, len(text), 31)
            assert nsec == (8 if slots == 8 else 0), slots
            assert (rc, out, used) == oracle.uncompress(s, len(text), window_bits=31)
    finally:
        sec.emu_sec_set_pool(0)
