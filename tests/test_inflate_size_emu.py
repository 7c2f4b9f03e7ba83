"""The size path (zsc_amd/csrc/inflate_size.h) on the lane emulation, against the oracle.

tests/emu_size builds the path's kernel sources with -DZSC_WAVE_EMU into a stand-alone program at 64, 16
(the decoder's group width on the GPU) and 8 lanes; it runs setup -> scan -> count -> want -> retry ->
resolve -> finish for a stream longer than a chunk and then the whole-stream size decode for a stream
that did not finish, as the runtime enqueues them.

For every case and every limit, (status, size, consumed) must be the oracle's (rc, len(out), used) at
dest_cap = limit.  The limits: unlimited, the exact size, the size minus 1, and 0.  Every case is sized
with chunk_bytes 4096 and with "never cut".

The one exception of the contract (include/zsc_hip.h) is built into the expectation, not left out of it:
where a stream's deflate data is sound and its check value all there, the expectation is the oracle's answer for
the same stream with the right check value in the trailer (expect()).  Which cases that touches is
asserted.  The helpers are shared with tests/test_gpu_inflate_size.py.
"""
import json
import os
import struct
import subprocess
import zlib

import pytest

from zsc_amd import corpus

HERE = os.path.dirname(os.path.abspath(__file__))
UNLIMITED = 0xFFFFFFFF
NEVER_CUT = 0xFFFFFFFF
CHUNK = 4096
LANES = (64, 16, 8)


def with_right_check(s, wbits):
    """s with the check value of its zlib / gzip trailer made right, where its deflate data is sound and
    the four bytes of the check value are there; None otherwise (raw, a damaged or truncated stream, a
    preset dictionary).  ISIZE is left as it is."""
    if wbits < 0 or len(s) < 2:
        return None
    gzip = wbits >= 16 and s[:2] == b"\x1f\x8b"
    if gzip:
        if len(s) < 10:
            return None
        flags, h = s[3], 10
        if flags & 4:
            if len(s) < h + 2:
                return None
            h += 2 + struct.unpack_from("<H", s, h)[0]
        for bit in (8, 16):
            if flags & bit:
                z = s.find(b"\0", h)
                if z < 0:
                    return None
                h = z + 1
        if flags & 2:
            h += 2
    else:
        if 16 <= wbits < 32 or (s[1] & 0x20):
            return None  # (a gzip-only decoder, or FDICT)
        h = 2
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(s[h:])
    except zlib.error:
        return None
    if not d.eof:
        return None
    t = len(s) - len(d.unused_data)
    if len(s) - t < 4:
        return None  # (both decoders run out of input before the check value is whole)
    chk = struct.pack("<I", zlib.crc32(out)) if gzip else struct.pack(">I", zlib.adler32(out))
    return s[:t] + chk + s[t + 4:]


def oracle_unlimited(oracle, s, wbits, hint):
    """the oracle with no limit: a capacity the output does not fill (a decode that never meets the end
    of its buffer is the decode without one)"""
    cap = 2 * hint + 65536
    while True:
        rc, out, used = oracle.uncompress(s, cap, window_bits=wbits)
        if len(out) < cap:
            return rc, len(out), used
        cap *= 4


def expect(oracle, s, limit, wbits, hint=0):
    """(status, size, consumed) of the contract, and whether the exception applied"""
    fixed = with_right_check(s, wbits)
    excepted = fixed is not None and fixed != s
    src = fixed if excepted else s
    if limit == UNLIMITED:
        return oracle_unlimited(oracle, src, wbits, hint), excepted
    rc, out, used = oracle.uncompress(src, limit, window_bits=wbits)
    return (rc, len(out), used), excepted


def limits_of(oracle, s, wbits, hint):
    """the four limits of a case (three where the size is 0)"""
    (_, size, _), _ = expect(oracle, s, UNLIMITED, wbits, hint)
    return [UNLIMITED] + sorted({size, max(size, 1) - 1, 0}, reverse=True)


def run_emu(tmp_path, lanes, jobs):
    """jobs: [(stream, window_bits, limit, chunk_bytes)] -> [(status, size, consumed, pieces)]"""
    path = os.path.join(str(tmp_path), f"cases{lanes}.bin")
    with open(path, "wb") as f:
        for s, wbits, limit, chunk in jobs:
            f.write(struct.pack("<iIII", wbits, limit, chunk, len(s)) + s)
    r = subprocess.run([os.path.join(HERE, "emu_size", f"emu_size{lanes}"), path], check=True,
                       stdout=subprocess.PIPE)
    rows = [tuple(int(x) for x in line.split()) for line in r.stdout.decode().splitlines()]
    assert len(rows) == len(jobs)
    return rows


@pytest.fixture(scope="module")
def emu_built():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_size")], check=True)


def check_cases(tmp_path, oracle, cases):
    """cases: [(name, stream, window_bits, size hint)].  Returns the names the exception applied to and
    the number of (case, limit) pairs the chunked path finished."""
    jobs, wants, names, excepted = [], [], [], set()
    for name, s, wbits, hint in cases:
        for limit in limits_of(oracle, s, wbits, hint):
            want, ex = expect(oracle, s, limit, wbits, hint)
            if ex:
                excepted.add(name)
            for chunk in (CHUNK, NEVER_CUT):
                jobs.append((s, wbits, limit, chunk))
                wants.append(want)
                names.append((name, limit, chunk))
    chunked = 0
    for lanes in LANES:
        rows = run_emu(tmp_path, lanes, jobs)
        for row, want, name, job in zip(rows, wants, names, jobs):
            assert row[:3] == want, (lanes, name, row, want)
            if job[3] == NEVER_CUT:
                assert row[3] == 0, (lanes, name, row)
            elif row[3]:
                assert row[0] == 0 and row[3] > 1, (lanes, name, row)
                chunked += lanes == 16
    return excepted, chunked


def chunks_cases(oracle):
    from test_inflate_chunks_emu import make_cases
    return [(name, s, wbits, cap) for name, s, cap, wbits, _ in make_cases(oracle)]


def golden_cases(oracle):
    from test_oracle import apply_edits
    g = json.load(open(os.path.join(HERE, "golden", "inflate_golden.json")))
    cases = []
    for i, c in enumerate(g["inflate_kat"]):
        raw = bytes(int(x, 16) for x in c["hex"].split())
        cases.append((f"kat{i}", raw, c["window_bits"], c["dest_cap"]))
    src = corpus.make_buffer(g["corrupt_source"]["kind"], g["corrupt_source"]["size"], g["corrupt_source"]["seed"])
    rc, good, _ = oracle.compress(src, g["corrupt_source"]["level"])
    assert rc == 0
    for i, c in enumerate(g["corrupt"]):
        if "flip" in c:
            bad = bytearray(good)
            bad[c["flip"]] = (bad[c["flip"]] + 1) & 0xff
            cases.append((f"corrupt{i}", bytes(bad), 15, len(src)))
        else:
            cases.append((f"corrupt{i}", good[:c["cut"]], 15, len(src)))
    for r in g["resync"]:
        stream = bytes.fromhex(r["stream_hex"])
        for j, c in enumerate(r["cases"]):
            cases.append((f"resync-{r['kind']}-{r['seed']}-{j}", apply_edits(stream, c["edits"]), r["window_bits"],
                          c["dest_cap"]))
    return cases


def damaged_cases(oracle, count=150):
    """seeded damage to streams written with full flushes, bytes overwritten, as the resync tests make them"""
    from test_inflate_resync_emu import constructed_cases, damaged_sweep, serial_cases
    cases = [(name, s, wbits, cap) for name, s, cap, wbits, _ in constructed_cases()]
    cases += [(name, s, wbits, cap) for name, s, cap, wbits in serial_cases()]
    cases += [(name, s, wbits, cap) for name, s, cap, wbits in damaged_sweep(oracle, 17, count)]
    return cases


def test_chunks_cases_equal_the_oracle(emu_built, tmp_path, oracle):
    excepted, chunked = check_cases(tmp_path, oracle, chunks_cases(oracle))
    # (corrupt-middle: six bytes overwritten inside a block that still decode as codes of the block, to
    # the end of the stream: all the decoder could find wrong with it is the check value)
    assert excepted == {"bad-adler", "bad-crc", "corrupt-middle"}
    assert chunked > 60  # (most streams of make_cases, at two or three of their limits)


def test_recorded_goldens_equal_the_oracle(emu_built, tmp_path, oracle):
    cases = golden_cases(oracle)
    assert len(cases) == 46 + 13 + 168
    check_cases(tmp_path, oracle, cases)


def test_damaged_streams_equal_the_oracle(emu_built, tmp_path, oracle):
    cases = damaged_cases(oracle)
    assert len(cases) >= 150
    statuses = {expect(oracle, s, UNLIMITED, wbits, hint)[0][0] for _, s, wbits, hint in cases}
    assert {0, -3, -5} <= statuses
    check_cases(tmp_path, oracle, cases)


def test_check_value_is_the_one_exception(emu_built, tmp_path, oracle):
    """a flipped Adler-32 / CRC-32 byte: Z_OK with the full length, consumed to the trailer's end; a
    flipped ISIZE byte: what the oracle gives"""
    text = corpus.make_buffer("text", 50000, 31)
    zs = zlib.compress(text, 6)
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    gz = co.compress(text) + co.flush()
    bad_adler = zs[:-2] + bytes([zs[-2] ^ 0x10]) + zs[-1:]
    bad_crc = gz[:-7] + bytes([gz[-7] ^ 0x10]) + gz[-6:]
    bad_isize = gz[:-3] + bytes([gz[-3] ^ 0x10]) + gz[-2:]
    assert oracle.uncompress(bad_adler, len(text))[0] == -3 and oracle.uncompress(bad_crc, len(text), 31)[0] == -3
    want_isize = oracle.uncompress(bad_isize, len(text), window_bits=31)
    assert want_isize[0] == -3
    jobs, wants = [], []
    for chunk in (CHUNK, NEVER_CUT):
        for limit in (UNLIMITED, len(text)):
            jobs += [(bad_adler, 15, limit, chunk), (bad_crc, 31, limit, chunk), (bad_isize, 31, limit, chunk)]
            wants += [(0, len(text), len(zs)), (0, len(text), len(gz)),
                      (want_isize[0], len(want_isize[1]), want_isize[2])]
    for lanes in LANES:
        rows = run_emu(tmp_path, lanes, jobs)
        assert [r[:3] for r in rows] == wants, lanes
