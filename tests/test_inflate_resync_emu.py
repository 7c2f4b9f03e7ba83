"""The resync inflate path (zsc_amd/csrc/inflate_resync.h) on the lane emulation, against the recorded
reference results and the oracle.

tests/emu_resync builds the path's kernel sources with -DZSC_WAVE_EMU at 16 lanes (the decoder's group
width on the GPU) and 64 lanes; its driver runs scan -> setup -> scan -> count -> resolve -> write ->
finish and then the serial decoder for a stream that did not finish, as the runtime enqueues them.  It
also runs the serial decoder on its own and returns both error counts: the resync path's (or, for a
stream that went serial, the serial decoder's) and the serial decoder's.  The helpers that build cases
are shared with tests/test_gpu_inflate_resync.py.
"""
import ctypes as C
import hashlib
import json
import os
import random
import subprocess
import zlib

import pytest

from zsc_amd import corpus

HERE = os.path.dirname(os.path.abspath(__file__))
MARK = b"\x00\x00\xff\xff"
# a stored block with LEN != ~NLEN: a data error at the first block of the section it starts
BAD_BLOCK = b"\x00\x34\x12\x55\x55"
HEADER_LEN = {15: 2, 31: 10, -15: 0}


@pytest.fixture(scope="module", params=["librsy_emu16.so", "librsy_emu64.so"], ids=["group16", "wave64"])
def rsy(request):
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_resync")], check=True)
    L = C.CDLL(os.path.join(HERE, "emu_resync", request.param))
    L.emu_rsy_set_work_bound.argtypes = [C.c_uint32, C.c_uint32]
    return L


def emu_uncompress(L, data, cap, window_bits):
    """(status, bytes, consumed, sections decoded in parallel, error count, the serial decoder's count)"""
    out = C.create_string_buffer(max(cap, 1))
    v = [C.c_uint32() for _ in range(5)]
    rc = L.emu_rsy_uncompress(data, len(data), window_bits, out, cap, *[C.byref(x) for x in v])
    ol, used, nsec, errors, serial_errors = (x.value for x in v)
    return rc, out.raw[:ol], used, nsec, errors, serial_errors


def full_flush_stream(data, section, level=6, wbits=15):
    """a stock-zlib stream with Z_FULL_FLUSH after every `section` input bytes; returns (stream, the
    input of each section, the offset where each section's compressed data starts)"""
    co = zlib.compressobj(level, zlib.DEFLATED, wbits)
    pieces = [data[i:i + section] for i in range(0, len(data), section)] or [b""]
    parts = [co.compress(p) + (co.flush(zlib.Z_FULL_FLUSH) if i < len(pieces) - 1 else co.flush())
             for i, p in enumerate(pieces)]
    stream = b"".join(parts)
    starts, at = [], 0
    for i, part in enumerate(parts):
        starts.append(HEADER_LEN[wbits] if i == 0 else at)
        at += len(part)
    return stream, pieces, starts


def damage_sections(stream, pieces, starts, damaged, wbits):
    """the first 5 bytes of each damaged section overwritten with BAD_BLOCK.  Returns the stream and
    what the reference gives for it: (status, output, consumed, data errors, sections() of a resync
    plan).  The trailer fails as well unless the last section is damaged (its search finds no
    pattern) or there is none (raw)."""
    b = bytearray(stream)
    for i in damaged:
        b[starts[i]:starts[i] + len(BAD_BLOCK)] = BAD_BLOCK
    out = b"".join(p for i, p in enumerate(pieces) if i not in damaged)
    errors = len(damaged) + (0 if not damaged or wbits < 0 or len(pieces) - 1 in damaged else 1)
    return bytes(b), (-3 if damaged else 0, out, len(b), errors, len(pieces))


def constructed_cases():
    """[(name, stream, cap, window_bits, (status, output, consumed, errors, sections))]"""
    cases = []
    data = corpus.make_buffer("text", 80000, 21)
    for wbits in (15, 31, -15):
        stream, pieces, starts = full_flush_stream(data, 4096, 6, wbits)
        assert stream.count(MARK) == len(pieces) - 1
        last = len(pieces) - 1
        for damaged in ([], [0], [3], [last], [0, last], [1, 2, 3], [2, 7, 11, 19], list(range(0, last + 1, 2))):
            s, want = damage_sections(stream, pieces, starts, damaged, wbits)
            cases.append((f"w{wbits}-damaged{damaged}", s, len(data), wbits, want))
    return cases


def serial_cases():
    """damage the resync path leaves to the serial decoder: [(name, stream, cap, window_bits)]"""
    data = corpus.make_buffer("text", 40000, 22)
    cases = []
    for wbits in (15, 31):
        stream, pieces, starts = full_flush_stream(data, 4096, 6, wbits)
        s, _ = damage_sections(stream, pieces, starts, [4], wbits)
        cases.append((f"w{wbits}-header", bytes([stream[0] ^ 0x20]) + stream[1:], len(data), wbits))
        cases.append((f"w{wbits}-header-and-section", bytes([s[0] ^ 0x20]) + s[1:], len(data), wbits))
        cases.append((f"w{wbits}-damaged-truncated-trailer", s[:-2], len(data), wbits))
        cases.append((f"w{wbits}-damaged-truncated-tail", s[:len(s) - 300], len(data), wbits))
        cases.append((f"w{wbits}-damaged-short-cap", s, len(data) - 4096 - 1000, wbits))
        cases.append((f"w{wbits}-damaged-tiny-cap", s, 9, wbits))
        # a pattern inside a failing trailer resumes decoding there: serial
        cases.append((f"w{wbits}-pattern-in-trailer", s[:len(s) - (8 if wbits == 31 else 4)] + MARK +
                      (b"\0\0\0\0" if wbits == 31 else b""), len(data), wbits))
    # Z_SYNC_FLUSH: sections need each other's history; a damaged one resumes into such a section
    rep = (b"the quick brown fox jumps over the lazy dog; " * 1500)[:60000]
    for wbits in (15, 31, -15):
        co = zlib.compressobj(6, zlib.DEFLATED, wbits)
        s = b"".join(co.compress(rep[i:i + 4000]) + co.flush(zlib.Z_SYNC_FLUSH) for i in range(0, 56000, 4000))
        s += co.compress(rep[56000:]) + co.flush()
        cases.append((f"w{wbits}-sync-flush", s, len(rep), wbits))
        marks = [i for i in range(len(s)) if s.startswith(MARK, i)]
        b = bytearray(s)
        b[marks[3] + 4:marks[3] + 9] = BAD_BLOCK
        cases.append((f"w{wbits}-sync-flush-damaged", bytes(b), len(rep), wbits))
    return cases


def semantics_cases():
    """cases that pin what the resynchronised state is: [(name, stream, cap, window_bits, (status, output,
    consumed, errors, sections), parallel)]"""
    import struct
    data = corpus.make_buffer("text", 40000, 25)
    cases = []
    # gzip: ISIZE counts the output since the last resume; the CRC covers all of it
    stream, pieces, starts = full_flush_stream(data, 4096, 6, 31)
    s, (st, out, used, errors, nsec) = damage_sections(stream, pieces, starts, [3], 31)
    since = sum(len(p) for p in pieces[4:])
    good = s[:-8] + struct.pack("<II", zlib.crc32(out), since)
    cases.append(("gzip-isize-since-resume", good, len(data), 31, (-3, out, len(good), 1, nsec), True))
    whole = s[:-8] + struct.pack("<II", zlib.crc32(out), len(out))
    cases.append(("gzip-isize-whole-output", whole, len(data), 31, (-3, out, len(whole), 2, nsec), True))
    # the output salvaged fills dest_len exactly
    cases.append(("salvaged-size-cap", s, len(out), 31, (st, out, used, errors, nsec), True))
    # a zlib header whose window (1 KiB) is smaller than the distances of later sections: before the
    # first resume that is the reference's data error (serial); after one, the limit is 32 KiB
    small = data[:300]
    co = zlib.compressobj(6, zlib.DEFLATED, 15)
    z = co.compress(small) + co.flush(zlib.Z_FULL_FLUSH)
    pieces = [small] + [data[i:i + 4096] for i in range(0, len(data), 4096)]
    parts = [z[2:]] + [co.compress(p) + (co.flush(zlib.Z_FULL_FLUSH) if i < len(pieces) - 2 else co.flush())
                       for i, p in enumerate(pieces[1:])]
    cmf = 0x28
    hdr = bytes([cmf, (31 - (cmf * 256) % 31) % 31])
    raw = hdr + b"".join(parts)
    starts, at = [], 2
    for part in parts:
        starts.append(at)
        at += len(part)
    cases.append(("zlib-small-window", raw, len(small) + len(data), 15, None, False))
    s, want = damage_sections(raw, pieces, starts, [1], 15)
    cases.append(("zlib-small-window-resumed", s, len(small) + len(data), 15, want, True))
    return cases


def golden_cases():
    """the recorded reference results: [(name, stream, cap, window_bits, (rc, out_len, consumed, sha256))]"""
    from test_oracle import apply_edits
    g = json.load(open(os.path.join(HERE, "golden", "inflate_golden.json")))
    cases = []
    for r in g["resync"]:
        stream = bytes.fromhex(r["stream_hex"])
        for j, c in enumerate(r["cases"]):
            cases.append((f"{r['kind']}-{r['seed']}-{j}", apply_edits(stream, c["edits"]), c["dest_cap"],
                          r["window_bits"], (c["rc"], c["out_len"], c["consumed"], c["out_sha256"])))
    return cases


def damaged_sweep(oracle, seed, count):
    """seeded damage to multi-section streams: [(name, stream, cap, window_bits)]"""
    rnd = random.Random(seed)
    kinds = ("text", "table", "token", "object", "bitmap")
    cases = []
    for i in range(count):
        wbits = (15, 31, -15)[i % 3]
        level = (0, 1, 6, 9)[(i // 3) % 4]
        n = rnd.randrange(1500, 14000)
        data = corpus.make_buffer(kinds[i % len(kinds)], n, 3000 + i)
        mbl = rnd.choice([512, 1024, 2048, 3000])
        if i % 2:
            rc, comp, _ = oracle.compress(data, level, window_bits=wbits, max_block_len=mbl)
            assert rc == 0
        else:
            comp, _, _ = full_flush_stream(data, mbl, level, wbits)
        b = bytearray(comp)
        for _ in range(rnd.randrange(1, 4)):
            op = rnd.randrange(4)
            at = rnd.randrange(len(b))
            if op == 0:
                b[at] ^= 1 << rnd.randrange(8)
            elif op == 1:
                b[at:at + 5] = BAD_BLOCK
            elif op == 2:
                del b[at:at + rnd.randrange(1, 40)]
            else:
                b[at:at + 3] = bytes(rnd.randrange(256) for _ in range(3))
        if i % 11 == 0:
            del b[rnd.randrange(len(b) // 2, len(b)):]
        cap = rnd.choice([n, n, n + 100, max(1, n - rnd.randrange(1, 3000))])
        cases.append((f"sweep{i}-l{level}-w{wbits}-m{mbl}", bytes(b), cap, wbits))
    return cases


def test_recorded_reference_cases(rsy):
    cases = golden_cases()
    assert len(cases) == 168
    parallel = 0
    for name, stream, cap, wbits, want in cases:
        rc, out, used, nsec, errors, serial_errors = emu_uncompress(rsy, stream, cap, wbits)
        assert (rc, len(out), used, hashlib.sha256(out).hexdigest()) == want, name
        assert errors == serial_errors, (name, errors, serial_errors)
        parallel += nsec > 0
    assert parallel >= 40


def test_constructed_damage_exact(rsy, oracle):
    """the construction's expectations, which are also the oracle's"""
    for name, stream, cap, wbits, (status, out, consumed, errors, nsec) in constructed_cases():
        assert oracle.uncompress(stream, cap, window_bits=wbits) == (status, out, consumed), name
        got = emu_uncompress(rsy, stream, cap, wbits)
        assert got == (status, out, consumed, nsec, errors, errors), (name, got[0], len(got[1]), got[2:])


def test_isize_window_and_cap_semantics(rsy, oracle):
    for name, stream, cap, wbits, want, parallel in semantics_cases():
        got = emu_uncompress(rsy, stream, cap, wbits)
        assert got[:3] == oracle.uncompress(stream, cap, window_bits=wbits), name
        assert got[4] == got[5], (name, got[4], got[5])
        if want is not None:
            assert got[:3] == want[:3] and (got[3], got[4]) == (want[4], want[3]), (name, got[0], got[2:])
        assert (got[3] > 0) == parallel, (name, got[3])


def test_damaged_sweep_equals_the_oracle(rsy, oracle):
    cases = damaged_sweep(oracle, 11, 1050)
    parallel = damaged_parallel = 0
    for name, stream, cap, wbits in cases:
        rc, out, used, nsec, errors, serial_errors = emu_uncompress(rsy, stream, cap, wbits)
        assert (rc, out, used) == oracle.uncompress(stream, cap, window_bits=wbits), name
        assert errors == serial_errors, (name, errors, serial_errors)
        parallel += nsec > 0
        damaged_parallel += nsec > 0 and rc == -3
    assert parallel >= 300 and damaged_parallel >= 200, (parallel, damaged_parallel)


def test_serial_cases_go_serial_and_equal_the_oracle(rsy, oracle):
    for name, stream, cap, wbits in serial_cases():
        rc, out, used, nsec, errors, serial_errors = emu_uncompress(rsy, stream, cap, wbits)
        assert (rc, out, used) == oracle.uncompress(stream, cap, window_bits=wbits), name
        assert errors == serial_errors, (name, errors, serial_errors)
        assert nsec == 0, name


def test_failing_trailer_alone_is_one_data_error(rsy, oracle):
    """a sound body under a wrong check value or ISIZE: the trailer's data error, and no pattern behind it"""
    data = corpus.make_buffer("text", 40000, 24)
    for wbits, at in ((15, -1), (31, -5), (31, -1)):
        stream, pieces, _ = full_flush_stream(data, 4096, 6, wbits)
        b = bytearray(stream)
        b[at] ^= 1
        want = oracle.uncompress(bytes(b), len(data), window_bits=wbits)
        assert want == (-3, data, len(b))
        assert emu_uncompress(rsy, bytes(b), len(data), wbits) == want + (len(pieces), 1, 1), (wbits, at)


def test_work_bound_sends_a_damaged_stream_serial(rsy, oracle):
    data = corpus.make_buffer("text", 60000, 23)
    stream, pieces, starts = full_flush_stream(data, 6000, 6, 15)
    s, want = damage_sections(stream, pieces, starts, [2, 5], 15)
    assert emu_uncompress(rsy, s, len(data), 15)[3] == len(pieces)
    try:
        rsy.emu_rsy_set_work_bound(0, 64)
        rc, out, used, nsec, errors, serial_errors = emu_uncompress(rsy, s, len(data), 15)
        assert nsec == 0
        assert (rc, out, used, errors) == want[:4]
    finally:
        rsy.emu_rsy_set_work_bound(4, 65536)
