"""The chunks inflate path (zsc_amd/csrc/inflate_chunks.h) on the lane emulation, against the oracle.

tests/emu_chunks builds the path's kernel sources with -DZSC_WAVE_EMU at 16 lanes (the decoder's group
width on the GPU) and 64 lanes; its driver runs setup -> scan -> count -> want -> retry -> resolve ->
window -> write -> finish and then the serial decoder for a stream that did not finish, as the runtime
enqueues them.  Every case must give the oracle's (status, bytes, consumed); where the number of pieces
decoded in parallel is predictable it must be the expected one (MANY: more than one).  make_cases() is
shared with tests/test_gpu_inflate_chunks.py.
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
ANY = None     # piece count not predicted: only the results are checked
MANY = "many"  # more than one piece
CHUNK = 8192   # chunk_bytes of the emulated plans (small, so that small streams have many chunks)


@pytest.fixture(scope="module", params=["libchk_emu16.so", "libchk_emu64.so"], ids=["group16", "wave64"])
def chk(request):
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_chunks")], check=True)
    L = C.CDLL(os.path.join(HERE, "emu_chunks", request.param))
    L.emu_chk_set_work_bound.argtypes = [C.c_uint32, C.c_uint32]
    L.emu_chk_set_retry.argtypes = [C.c_int]
    L.emu_chk_header_ok.argtypes = [C.c_char_p, C.c_uint32, C.c_uint64]
    L.emu_chk_decoder_header_ok.argtypes = [C.c_char_p, C.c_uint32, C.c_uint64]
    return L


def emu_uncompress(L, data, cap, window_bits, chunk=CHUNK):
    out = C.create_string_buffer(max(cap, 1))
    ol, used, npieces, ncand = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    rc = L.emu_chk_uncompress(data, len(data), window_bits, out, cap, chunk, C.byref(ol), C.byref(used),
                              C.byref(npieces), C.byref(ncand))
    return rc, out.raw[:ol.value], used.value, npieces.value


def zlib_stream(data, level, wbits, flush=None, every=None):
    co = zlib.compressobj(level, zlib.DEFLATED, wbits)
    if flush is None:
        return co.compress(data) + co.flush()
    out = []
    for at in range(0, len(data), every):
        out.append(co.compress(data[at:at + every]) + co.flush(flush))
    out.append(co.flush())
    return b"".join(out)


def make_cases(oracle, seed=3, n_oracle=40):
    """[(name, stream, dest_cap, window_bits, expected pieces: an int, MANY or ANY)]"""
    rnd = random.Random(seed)
    cases = []
    text = corpus.make_buffer("text", 300000, 11)
    # marker-free stock zlib / gzip / raw at levels 1, 6, 9
    for level in (1, 6, 9):
        for wbits in (15, 31, -15):
            s = zlib_stream(text, level, wbits)
            cases.append((f"zlib-l{level}-w{wbits}", s, len(text), wbits, MANY))
    # the oracle's own zsc_compress2 output, window_bits 9-15, raw / zlib / gzip, no markers
    kinds = ("text", "table", "token", "bitmap", "object")
    for i in range(n_oracle):
        kind = kinds[i % len(kinds)]
        n = rnd.randrange(1000, 120000)
        data = corpus.make_buffer(kind, n, 300 + i)
        level = 1 + i % 9
        wb = 9 + i % 7
        wrap = i % 3
        wbits = wb if wrap == 0 else (wb + 16 if wrap == 1 else -wb)
        rc, comp, _ = oracle.compress(data, level, window_bits=wbits, max_block_len=n + 1)
        assert rc == 0, (i, rc)
        cases.append((f"oracle-{kind}-l{level}-w{wbits}", comp, n, wbits, ANY))
    # Z_SYNC_FLUSH: the pieces share history; decoded in parallel all the same
    rep = (b"the quick brown fox jumps over the lazy dog; " * 7000)[:300000]
    for wbits in (15, 31):
        s = zlib_stream(text, 6, wbits, zlib.Z_SYNC_FLUSH, 16384)
        cases.append((f"zlib-sync-text-w{wbits}", s, len(text), wbits, MANY))
    s = zlib_stream(rep + text, 6, 15, zlib.Z_SYNC_FLUSH, 4096)
    cases.append(("zlib-sync-rep", s, len(rep) + len(text), 15, ANY))
    # stored only: level 0, and random data at level 6 (stored blocks the encoder chose)
    s = zlib_stream(text[:100000], 0, 15)
    cases.append(("stored-level0", s, 100000, 15, MANY))
    rnd_data = random.Random(5).randbytes(90000)
    s = zlib_stream(rnd_data, 6, 31)
    cases.append(("stored-random-gzip", s, len(rnd_data), 31, MANY))
    # fixed-block heavy: runs of zeros (fixed blocks are not searched for: few pieces, or one)
    zeros = bytearray(200000)
    for p in range(0, len(zeros), 997):
        zeros[p] = p & 0xff
    s = zlib_stream(bytes(zeros), 6, 15)
    cases.append(("fixed-zeros", s, len(zeros), 15, ANY))
    s = zlib_stream(bytes(zeros), 1, -15)
    cases.append(("fixed-zeros-raw", s, len(zeros), -15, ANY))
    # a misleading stored payload: real dynamic-block streams and LEN / ~LEN patterns inside stored data
    mis = bytearray()
    while len(mis) < 120000:
        mis += zlib_stream(text[len(mis) % 50000:len(mis) % 50000 + 3000], 9, -15)
        ln = rnd.randrange(0, 3000)
        mis += struct.pack("<HH", ln, ln ^ 0xffff) + b"\x00\x00\xff\xff"
    s = zlib_stream(bytes(mis), 0, 15)
    cases.append(("misleading-stored", s, len(mis), 15, ANY))
    s = zlib_stream(bytes(mis), 6, 31)
    cases.append(("misleading-deflated", s, len(mis), 31, ANY))
    zs = zlib_stream(text, 6, 15)
    # FDICT
    cz = zlib.compressobj(6, zlib.DEFLATED, 15, zdict=b"the dictionary")
    fd = cz.compress(text) + cz.flush()
    cases.append(("fdict", fd, len(text), 15, 0))
    # a raw stream made with a preset dictionary: its first piece reaches before the output (a data
    # error that only resolve's reach check finds; without it the pieces would chain to a Z_OK)
    cz = zlib.compressobj(6, zlib.DEFLATED, -15, zdict=text[:30000])
    cases.append(("raw-zdict", cz.compress(text) + cz.flush(), len(text), -15, 0))
    # truncation: in the body, in the trailer
    cases.append(("truncated-body", zs[:len(zs) - 3000], len(text), 15, 0))
    cases.append(("truncated-trailer", zs[:-2], len(text), 15, 0))
    # short dest_cap
    cases.append(("short-cap", zs, len(text) - 1, 15, 0))
    cases.append(("tiny-cap", zs, 100, 15, 0))
    # bad trailers
    cases.append(("bad-adler", zs[:-1] + bytes([zs[-1] ^ 1]), len(text), 15, 0))
    gz = zlib_stream(text, 6, 31)
    cases.append(("bad-crc", gz[:-5] + bytes([gz[-5] ^ 1]) + gz[-4:], len(text), 31, 0))
    cases.append(("bad-isize", gz[:-4] + struct.pack("<I", len(text) + 1), len(text), 31, 0))
    # junk after the trailer (parallel; consumed ends at the trailer)
    cases.append(("junk-after", zs + b"\x01\x02junk", len(text), 15, MANY))
    # a corrupted middle: a data error, decoded by the serial decoder
    bad = bytearray(zs)
    for j in range(len(zs) // 2, len(zs) // 2 + 6):
        bad[j] ^= 0x5a
    cases.append(("corrupt-middle", bytes(bad), len(text), 15, 0))
    # a zlib header whose window (1 KiB) is smaller than the distances used later: a data error
    s = zlib_stream(text, 6, 15)
    cmf = 0x28
    flg = (31 - (cmf * 256) % 31) % 31
    cases.append(("dmax-smaller", bytes([cmf, flg]) + s[2:], len(text), 15, 0))
    # small streams (one chunk: serial), empty input, empty output
    cases.append(("one-chunk", zlib_stream(text[:5000], 6, 15), 5000, 15, 0))
    cases.append(("empty-input", b"", 10, 15, 0))
    cases.append(("empty-output", zlib_stream(b"", 6, 15), 0, 15, 0))
    return cases


def check_pieces(name, got, want):
    if want is ANY:
        return
    if want is MANY:
        assert got > 1, (name, got)
    else:
        assert got == want, (name, got, want)


def test_chunks_equal_the_oracle(chk, oracle):
    cases = make_cases(oracle)
    parallel = 0
    for name, stream, cap, wbits, want in cases:
        rc, out, used, npieces = emu_uncompress(chk, stream, cap, wbits)
        orc, oout, oused = oracle.uncompress(stream, cap, window_bits=wbits)
        assert (rc, out, used) == (orc, oout, oused), (name, rc, orc, len(out), len(oout), used, oused)
        check_pieces(name, npieces, want)
        if npieces:
            assert rc == 0, name
            parallel += 1
    assert parallel > 25


def test_chunk_sizes(chk, oracle):
    text = corpus.make_buffer("text", 200000, 12)
    s = zlib_stream(text, 1, 15)
    want = oracle.uncompress(s, len(text))
    for chunk in (1024, 4096, 20000, 100000, len(s) - 1, len(s)):
        rc, out, used, npieces = emu_uncompress(chk, s, len(text), 15, chunk)
        assert (rc, out, used) == want, chunk
        assert (npieces > 1) == (chunk < len(s) // 2), (chunk, npieces)


def test_work_bound_sends_the_stream_serial(chk, oracle):
    text = corpus.make_buffer("text", 200000, 13)
    s = zlib_stream(text, 6, 15)
    assert emu_uncompress(chk, s, len(text), 15)[3] > 1
    try:
        chk.emu_chk_set_work_bound(0, 64)
        rc, out, used, npieces = emu_uncompress(chk, s, len(text), 15)
        assert npieces == 0
        assert (rc, out, used) == oracle.uncompress(s, len(text))
    finally:
        chk.emu_chk_set_work_bound(4, 65536)


def test_header_validator_agrees_with_the_decoder(chk, oracle):
    """inf_dyn_header_ok (the scan) against the decoder's own verdict on the first block's header, at
    every bit offset of a few streams"""
    text = corpus.make_buffer("text", 40000, 14)
    streams = [zlib_stream(text, 6, -15)[:2500], zlib_stream(text, 1, -15)[-2000:],
               oracle.compress(corpus.make_buffer("table", 20000, 15), 9, window_bits=-15)[1][:1500],
               random.Random(16).randbytes(1500)]
    hits = 0
    for s in streams:
        for bit in range(len(s) * 8):
            v = chk.emu_chk_header_ok(s, len(s), bit)
            d = chk.emu_chk_decoder_header_ok(s, len(s), bit)
            assert bool(v) == bool(d), (bit, v, d)
            hits += bool(v)
    assert hits >= 2  # (the true block starts at least)


def false_clean_stream(chunk, nblocks=12):
    """A raw stream of stored blocks whose ends fall 2005 bytes into every third chunk, with a complete
    raw deflate stream (a dynamic block with BFINAL set) stored 100 bytes into every chunk: in those
    chunks the first candidate is false and decodes cleanly to a final block, ahead of the true one,
    chunk after chunk."""
    text = corpus.make_buffer("text", 40000, 22)
    co = zlib.compressobj(9, zlib.DEFLATED, -15)
    mini = co.compress(text[:2000]) + co.flush()
    sizes = [2000] + [3 * chunk - 5] * nblocks
    total = sum(sz + 5 for sz in sizes)
    body = bytearray(corpus.make_buffer("text", total, 23))
    for c in range(total // chunk):
        p = c * chunk + 100
        if p + len(mini) <= total:
            body[p:p + len(mini)] = mini
    out, payload, at = bytearray(), bytearray(), 0
    for i, sz in enumerate(sizes):
        data = bytes(body[at + 5:at + 5 + sz])
        out += bytes([1 if i == len(sizes) - 1 else 0]) + struct.pack("<HH", sz, sz ^ 0xffff) + data
        payload += data
        at += sz + 5
    return bytes(out), bytes(payload)


@pytest.mark.parametrize("retry", [1, 0], ids=["retry", "no-retry"])
def test_adjacent_false_clean_candidates_keep_the_chain(chk, oracle, retry):
    s, payload = false_clean_stream(4096)
    want = oracle.uncompress(s, len(payload), window_bits=-15)
    assert want == (0, payload, len(s))
    try:
        chk.emu_chk_set_retry(retry)
        rc, out, used, npieces = emu_uncompress(chk, s, len(payload), -15, 4096)
    finally:
        chk.emu_chk_set_retry(1)
    assert (rc, out, used) == want
    assert npieces == 12  # (one piece per stored block after the first, which shares chunk 0)
