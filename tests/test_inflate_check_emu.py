"""The check path (zsc_amd/csrc/inflate_check.h) on the lane emulation, against the oracle.

tests/emu_check builds the path's kernel sources with -DZSC_WAVE_EMU into a stand-alone program at 64, 16
(the decoder's group width on the GPU) and 8 lanes; it runs setup -> scan -> count -> want -> retry ->
resolve -> window -> check-write -> finish for a stream longer than a chunk and then the whole-stream ring
decode (relaunched through the size decode after a data error) for a stream that did not finish, as the
runtime enqueues them.  The program keeps a shadow of every ring and aborts when a slot read does not hold
the position asked for or a position is overwritten before it was folded; every whole-stream decode of a
run shares one ring, so the ring is reused from stream to stream all through a test.

For every case and every limit, (status, size, consumed) must be the oracle's (rc, len(out), used) at
dest_cap = limit, with no exception, and the check value handed out must be zlib's over the oracle's
output wherever the status is 0 (Adler-32 for zlib and raw streams, CRC-32 for gzip ones).  The limits:
unlimited, the exact size, the size minus 1, and 0.  Every case is checked with chunk_bytes 4096 and with
"never cut".  The same cases go through the program built with -fsanitize=address,undefined (a stand-alone
program on the CPU) at 16 lanes, the ring boundary and trailer cases at 8 lanes too, which must print the same
lines.
"""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from zsc_amd import corpus

from test_inflate_size_emu import CHUNK, LANES, NEVER_CUT, UNLIMITED, limits_of, oracle_unlimited

HERE = os.path.dirname(os.path.abspath(__file__))
RING, FOLD = 65536, 16384  # CHK_RING, CHK_FOLD of inflate_check.h: the lengths below move with them
BOUNDARY_LENGTHS = [L + d for L in (FOLD, 2 * FOLD, 3 * FOLD, RING, RING + FOLD, 2 * RING) for d in (-1, 0, 1)]
WRAPPERS = (15, -15, 31)
# the sanitizer build is four times slower: every case goes through it at the GPU's group width, and the ring
# boundary and trailer cases also at 8 lanes, where a lane decodes with two slots (lfc2 / lof2)
SAN_LANES = (16,)
SAN_LANES_RING = (16, 8)


def is_gzip(s, wbits):
    return wbits >= 16 and s[:2] == b"\x1f\x8b"


def answer(oracle, s, limit, wbits, hint):
    """(status, size, consumed, check value) of the contract: the oracle at dest_cap = limit, and zlib's
    check value of its output where the status is 0"""
    if limit == UNLIMITED:
        rc, size, used = oracle_unlimited(oracle, s, wbits, hint)
        out = oracle.uncompress(s, size + 1, window_bits=wbits)[1] if rc == 0 else b""
        assert rc != 0 or len(out) == size
    else:
        rc, out, used = oracle.uncompress(s, limit, window_bits=wbits)
        size = len(out)
    value = 0
    if rc == 0:
        value = zlib.crc32(out) if is_gzip(s, wbits) else zlib.adler32(out)
    return rc, size, used, value


def run_emu(tmp_path, lanes, jobs, san=False):
    """jobs: [(stream, window_bits, limit, chunk_bytes)] -> [(status, size, consumed, pieces, errors, value)]"""
    path = os.path.join(str(tmp_path), f"check{lanes}.bin")
    with open(path, "wb") as f:
        for s, wbits, limit, chunk in jobs:
            f.write(struct.pack("<iIII", wbits, limit, chunk, len(s)) + s)
    r = subprocess.run([os.path.join(HERE, "emu_check", f"emu_check{lanes}" + ("_san" if san else "")), path],
                       check=True, stdout=subprocess.PIPE)
    rows = [tuple(int(x) for x in line.split()) for line in r.stdout.decode().splitlines()]
    assert len(rows) == len(jobs)
    return rows


@pytest.fixture(scope="module")
def emu_built():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_check")], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_check"), "san"], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_size")], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_chunks")], check=True)


def chunks_emu_pieces(s, cap, wbits):
    """the pieces the chunks emulation decodes the stream in, at 16 lanes and chunk_bytes 4096"""
    L = C.CDLL(os.path.join(HERE, "emu_chunks", "libchk_emu16.so"))
    out = C.create_string_buffer(max(cap, 1))
    v = [C.c_uint32() for _ in range(4)]
    rc = L.emu_chk_uncompress(s, len(s), wbits, out, cap, CHUNK, *[C.byref(x) for x in v])
    assert rc == 0
    return v[2].value


def check_cases(tmp_path, oracle, cases, pieces_as_chunks=False, san_lanes=SAN_LANES):
    """cases: [(name, stream, window_bits, size hint)].  Returns the number of (case, limit) pairs the
    chunked path finished at 16 lanes."""
    jobs, wants, names = [], [], []
    for name, s, wbits, hint in cases:
        for limit in limits_of(oracle, s, wbits, hint):
            want = answer(oracle, s, limit, wbits, hint)
            for chunk in (CHUNK, NEVER_CUT):
                jobs.append((s, wbits, limit, chunk))
                wants.append(want)
                names.append((name, wbits, limit, chunk))
    chunked = 0
    for lanes in LANES:
        rows = run_emu(tmp_path, lanes, jobs)
        if lanes in san_lanes:
            assert run_emu(tmp_path, lanes, jobs, san=True) == rows
        for row, want, name, job in zip(rows, wants, names, jobs):
            assert (row[0], row[1], row[2], row[5]) == want, (lanes, name, row, want)
            if job[3] == NEVER_CUT:
                assert row[3] == 0, (lanes, name, row)
            elif row[3]:
                assert row[0] == 0 and row[3] > 1, (lanes, name, row)
                chunked += lanes == 16
            # a sound stream longer than two chunks, at a limit it fits: finished by the chunked path, in
            # the pieces the chunks emulation decodes it in
            if (pieces_as_chunks and lanes == 16 and job[3] == CHUNK and len(job[0]) > 2 * CHUNK and want[0] == 0):
                assert row[3] == chunks_emu_pieces(job[0], want[1], job[1]), (name, row)
    return chunked


def chunks_cases(oracle):
    from test_inflate_size_emu import chunks_cases as cases
    return cases(oracle)


def shape_cases():
    from test_gpu_inflate_size import shape_cases as cases
    return [(name, s, wbits, hint) for wbits, group in cases().items() for name, s, hint in group]


def _deflate(data, wbits, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    return co.compress(data) + co.flush()


def boundary_makers():
    """{name: output length -> (data, level, strategy)}: what meets the ring's wrap and the fold boundaries"""
    rnd = np.random.default_rng(71).integers(0, 256, 32768, dtype=np.uint8).tobytes()
    noise = np.random.default_rng(72).integers(0, 256, 2 * RING + 1, dtype=np.uint8).tobytes()
    text = corpus.make_buffer("text", 2 * RING + 1, 73)
    return {
        "zeros": lambda n: (bytes(n), 6, zlib.Z_DEFAULT_STRATEGY),              # distance 1, length 258
        "dist32768": lambda n: ((rnd * 7)[:n], 6, zlib.Z_DEFAULT_STRATEGY),     # every match at distance 32 768
        "huffman-only": lambda n: (text[:n], 6, zlib.Z_HUFFMAN_ONLY),           # literals only
        "stored": lambda n: (noise[:n], 0, zlib.Z_DEFAULT_STRATEGY),            # stored blocks of 65 535
        "fixed": lambda n: (text[:n], 6, zlib.Z_FIXED),
        "rle": lambda n: (text[:n], 6, zlib.Z_RLE),
    }


def boundary_cases(wrappers=WRAPPERS, lengths=BOUNDARY_LENGTHS):
    cases = []
    for name, make in boundary_makers().items():
        for n in lengths:
            data, level, strategy = make(n)
            assert len(data) == n
            for wbits in wrappers:
                cases.append((f"{name}-{n}", _deflate(data, wbits, level, strategy), wbits, n))
    return cases


def trailer_flips():
    """{window_bits: (the sound stream, its output, [(name, damaged stream, is a check-value flip)])}: each
    byte of the check value and of ISIZE flipped in turn"""
    text = corpus.make_buffer("text", 70000, 74)
    flips = {}
    for wbits in (15, 31):
        s = _deflate(text, wbits)
        fields = [("check", len(s) - (8 if wbits == 31 else 4))] + ([("isize", len(s) - 4)] if wbits == 31 else [])
        flips[wbits] = (s, text, [(f"{field}{j}", s[:at + j] + bytes([s[at + j] ^ 0x40]) + s[at + j + 1:],
                                   field == "check") for field, at in fields for j in range(4)])
    return flips


def damaged_flush_cases():
    """three damaged full-flush streams per wrapper: one error, two errors, an error in the last section;
    [(name, stream, window_bits, size hint, the reference's data-error count)]"""
    from test_inflate_resync_emu import damage_sections, full_flush_stream
    data = corpus.make_buffer("text", 80000, 21)
    cases = []
    for wbits in (15, 31):
        stream, pieces, starts = full_flush_stream(data, 4096, 6, wbits)
        for damaged in ([3], [2, 7], [len(pieces) - 1]):
            s, want = damage_sections(stream, pieces, starts, damaged, wbits)
            cases.append((f"w{wbits}-damaged{damaged}", s, wbits, len(data), want[3]))
    return cases


def test_chunks_and_shape_cases_equal_the_oracle(emu_built, tmp_path, oracle):
    chunked = check_cases(tmp_path, oracle, chunks_cases(oracle) + shape_cases(), pieces_as_chunks=True)
    assert chunked > 60  # (most streams of make_cases, at two of their limits)


@pytest.mark.parametrize("maker", list(boundary_makers()))
def test_ring_and_fold_boundaries(emu_built, tmp_path, oracle, maker):
    cases = [c for c in boundary_cases() if c[0].startswith(maker + "-")]
    assert len(cases) == len(BOUNDARY_LENGTHS) * len(WRAPPERS)
    chunked = check_cases(tmp_path, oracle, cases, pieces_as_chunks=True, san_lanes=SAN_LANES_RING)
    if maker in ("huffman-only", "stored"):
        assert chunked > 0  # (streams longer than two chunks, cut at dynamic headers / stored blocks)


def test_trailer_damage_is_found(emu_built, tmp_path, oracle):
    """what the feature adds to a size plan: a flipped check-value byte is Z_DATA_ERROR with the full
    length, as the oracle has it, where the size emulation says Z_OK; and it ends in the whole-stream decode"""
    from test_inflate_size_emu import run_emu as run_size_emu
    for wbits, (sound, text, flips) in trailer_flips().items():
        assert len(sound) > 2 * CHUNK
        jobs, wants, size_wants = [], [], []
        for name, s, is_check in flips:
            for limit in (UNLIMITED, len(text)):
                want = answer(oracle, s, limit, wbits, len(text))
                assert want[:2] == (-3, len(text)), (wbits, name)
                for chunk in (CHUNK, NEVER_CUT):
                    jobs.append((s, wbits, limit, chunk))
                    wants.append(want)
                    size_wants.append((0, len(text), len(s)) if is_check else want[:3])
        for lanes in LANES:
            rows = run_emu(tmp_path, lanes, jobs)
            if lanes in SAN_LANES_RING:
                assert run_emu(tmp_path, lanes, jobs, san=True) == rows
            for row, want in zip(rows, wants):
                assert (row[0], row[1], row[2], row[5]) == want and row[3] == 0, (lanes, wbits, row, want)
            size_rows = run_size_emu(tmp_path, lanes, jobs)
            assert [r[:3] for r in size_rows] == size_wants, (lanes, wbits)
        # the sound stream itself is finished by the chunked path
        row = run_emu(tmp_path, 16, [(sound, wbits, UNLIMITED, CHUNK)])[0]
        assert row[0] == 0 and row[3] > 1 and row[5] == (zlib.crc32(text) if wbits == 31 else zlib.adler32(text))


def test_damaged_flush_streams_equal_the_oracle(emu_built, tmp_path, oracle):
    cases = damaged_flush_cases()
    check_cases(tmp_path, oracle, [c[:4] for c in cases])
    jobs = [(s, wbits, UNLIMITED, chunk) for _, s, wbits, _, _ in cases for chunk in (CHUNK, NEVER_CUT)]
    errors = [e for c in cases for e in (c[4], c[4])]
    for lanes in LANES:
        rows = run_emu(tmp_path, lanes, jobs)
        assert [r[4] for r in rows] == errors and all(r[0] == -3 and r[3] == 0 for r in rows), lanes
