"""Hand-built DEFLATE streams at the format's limits (tests/deflate_builder.py) on the CPU.

Three things are checked here, none of them on a GPU:
  * the builder against itself: play() of every legal case equals what stock zlib makes of the stream (zlib
    cross-checks the builder only; it is never the checker of a kernel);
  * the oracle, and the compiled reference where it is built, against every record of
    tests/golden/handbuilt_golden.json (recorded from the compiled reference by
    tests/golden/make_handbuilt_golden.py);
  * the kernels in the lane emulations: every record through emu_uncompress of the four tests/emu builds, and
    the records of the composed streams and `deep` through the drivers of the chunks, sections, resync, size,
    check and indexed paths, with the Python wrappers of those paths' own test modules.
"""
import ctypes as C
import os
import subprocess
import zlib

import pytest

import deflate_builder as B

HERE = os.path.dirname(os.path.abspath(__file__))
PATH_DIRS = ("emu_chunks", "emu_sections", "emu_resync", "emu_size", "emu_check", "emu_index")


@pytest.fixture(scope="module")
def golden():
    """(records, streams by case name, the golden file, expected output by case name)"""
    recs, streams, g = B.records()
    wants = {name: want for name, _, _, _, want in B.cases()}
    return recs, streams, g, wants


@pytest.fixture(scope="module")
def paths_built():
    for d in PATH_DIRS:
        subprocess.run(["make", "-s", "-C", os.path.join(HERE, d)], check=True)


def path_records(recs):
    """the records that go through every path's driver: the composed streams and `deep`"""
    names = set(B.composed_names()) | {"deep"}
    return [r for r in recs if r.name in names]


# ---- the builder against itself ----

def test_complete_lengths_are_complete():
    for n in range(1, 289):
        for deep in (False, True):
            lens = B.complete_lengths(n, deep=deep)
            assert len(lens) == n and all(1 <= x <= 15 for x in lens), (n, deep)
            assert B.kraft(lens) == (32768 if n > 1 else 16384), (n, deep)
            if deep and n >= 16:
                assert max(lens) == 15, n
            codes = B.canonical(lens)
            words = sorted(format(c, "0%db" % k) for c, k in codes.values())
            assert len(set(words)) == n and not any(b.startswith(a) for a, b in zip(words, words[1:])), (n, deep)
    order = [7, 3, 5]
    lens = B.complete_lengths(30, order, deep=True)
    assert [lens[x] for x in order] == sorted(lens)[:3]
    for keep in range(1, 7):
        lens = B.complete_lengths(286, [256], deep=True, keep=keep)
        assert set(range(1, keep + 1)) <= set(lens) and B.kraft(lens) == 32768 and max(lens) == 15


def test_check_values_in_plain_python(oracle):
    rnd = B.Lcg(9)
    for n in (0, 1, 5551, 5552, 5553, 70000):
        data = rnd.bytes(n)
        assert B.adler32(data) == oracle.adler32(data) == zlib.adler32(data)
        assert B.crc32(data) == oracle.crc32(data) == zlib.crc32(data)
    assert B.adler32(b"\xff" * 100000) == zlib.adler32(b"\xff" * 100000)


def test_play_equals_stock_zlib():
    """every legal case, and every case there must be"""
    cases = B.cases()
    names = [c[0] for c in cases]
    for must in ("deep", "ring-edge", "tiny-blocks", "stored-phases", "stored-65535", "one-dist-code") + \
            tuple(B.composed_names()):
        assert must in names
    assert {c[3] for c in cases if c[0].startswith("composed-")} == {15, 31, -15}
    legal = 0
    for name, stream, cap, wbits, want in cases:
        d = zlib.decompressobj(wbits)
        if want is None:
            continue
        assert d.decompress(stream) == want and d.eof, name
        assert cap >= len(want), name
        legal += 1
    assert legal >= 20
    for name in ("deep", "ring-edge"):
        out, owner = B.play_slow(B.tokens_of(name))
        assert out == dict((c[0], c[4]) for c in cases)[name] and len(owner) == len(out)


def test_first_difference_names_the_token():
    tokens = [1, 2, 3, (5, 2), 9]
    want = B.play(tokens)
    got = want[:6] + b"\xee" + want[7:]
    msg = B.first_difference(got, want, tokens)
    assert "offset 6" in msg and "(5, 2)" in msg and "byte 3 of it" in msg


# ---- the oracle and the reference against the golden file ----

def _against_records(golden, uncompress, what):
    recs, streams, g, wants = golden
    outs = []
    for r in recs:
        rc, out, used = uncompress(streams[r.name][:r.cut], r.cap, r.window_bits)
        assert (rc, len(out), used) == (r.rc, r.out_len, r.consumed), (what, r.name, r.cut, r.cap, rc, len(out), used, r)
        want = wants[r.name]
        if want is not None:
            assert out == want[:len(out)], (what, r.name, r.cut, r.cap)
        outs.append(out)
    B.check_outputs(recs, g, outs, what)


def test_records_are_what_the_issue_lists(golden):
    recs, streams, g, wants = golden
    assert len(recs) > 8000
    for name, stream in streams.items():
        mine = [r for r in recs if r.name == name]
        full = [r for r in mine if r.cut == len(stream) and r.cap == g["cases"][name]["cap"]]
        assert len(full) == 1
        if len(stream) < B.SHORT:
            assert {r.cut for r in mine} == set(range(len(stream) + 1))
            assert {r.cap for r in mine} == {g["cases"][name]["cap"], 1, 2, 3}
        else:
            assert len({r.cut for r in mine}) >= 12 and len({r.cap for r in mine}) >= 3
    # a legal case decodes to play() at its full record; every record that is Z_OK is a whole legal output,
    # so play() gives its check value
    for r in recs:
        want = wants[r.name]
        if r.rc == 0:
            assert want is not None and r.out_len == len(want), (r.name, r.cut, r.cap)
        if want is not None and r.cut == len(streams[r.name]) and r.cap >= len(want):
            assert (r.rc, r.out_len) == (0, len(want)) and r.out_sha in (None, B.sha(want)), r.name
    # the erroneous ones are data errors at full length, not exhaustion
    for name, want in wants.items():
        if want is None and not name.startswith("fixed-258-d1-cap"):
            assert g["cases"][name]["full"][0] == -3, name
    assert {r.rc for r in recs} == {0, -3, -5}


def test_oracle_equals_the_records(golden, oracle):
    _against_records(golden, lambda s, cap, wbits: oracle.uncompress(s, cap, window_bits=wbits), "oracle")


def test_reference_equals_the_records(golden, live_reference):
    if live_reference is None:
        return  # (recorded from it; where it is not built the oracle stands for it, above)
    _against_records(golden, lambda s, cap, wbits: live_reference.uncompress(s, cap, window_bits=wbits), "reference")


# ---- the kernels in the lane emulations ----

@pytest.mark.parametrize("lib", ["libzsc_emu.so", "libzsc_emu16.so", "libzsc_emu8.so", "libzsc_emu16s.so"],
                         ids=["wave64", "group16", "group8", "group16-stage1024"])
def test_serial_decoder_equals_the_records(golden, lib):
    L = C.CDLL(os.path.join(HERE, "emu", lib))
    buf = C.create_string_buffer(max(r.cap for r in golden[0]) + 1)

    def uncompress(s, cap, wbits):
        ol, used = C.c_uint32(), C.c_uint32()
        rc = L.emu_uncompress(s, len(s), wbits, buf, cap, C.byref(ol), C.byref(used))
        return rc, C.string_at(buf, ol.value), used.value

    _against_records(golden, uncompress, lib)
    if lib == "libzsc_emu16.so":
        # the copy quotient and the ring, byte for byte, with the token named
        recs, streams, g, wants = golden
        for name in ("deep", "ring-edge"):
            rc, out, used = uncompress(streams[name], len(wants[name]), -15)
            assert out == wants[name], B.first_difference(out, wants[name], B.tokens_of(name))


@pytest.mark.parametrize("lib", ["libchk_emu16.so", "libchk_emu64.so"], ids=["group16", "wave64"])
def test_chunks_path_equals_the_records(golden, paths_built, lib):
    from test_inflate_chunks_emu import CHUNK, emu_uncompress
    assert CHUNK == 8192
    recs, streams, g, wants = golden
    L = C.CDLL(os.path.join(HERE, "emu_chunks", lib))
    pieces = {}

    def uncompress(s, cap, wbits):
        rc, out, used, npieces = emu_uncompress(L, s, cap, wbits)
        pieces[(len(s), cap)] = npieces
        return rc, out, used

    part = path_records(recs)
    _against_records((part, streams, g, wants), uncompress, lib)
    # the condition: at full cap every composed stream comes out in more than one piece
    for name in B.composed_names():
        assert pieces[(len(streams[name]), len(wants[name]))] > 1, name


@pytest.mark.parametrize("width", ["16", "64"], ids=["group16", "wave64"])
def test_sections_and_resync_paths_equal_the_records(golden, paths_built, width):
    from test_inflate_resync_emu import emu_uncompress as rsy_uncompress
    from test_inflate_sections_emu import emu_uncompress as sec_uncompress
    recs, streams, g, wants = golden
    part = path_records(recs)
    sec = C.CDLL(os.path.join(HERE, "emu_sections", f"libsec_emu{width}.so"))
    _against_records((part, streams, g, wants), lambda s, cap, wbits: sec_uncompress(sec, s, cap, wbits)[:3], "sections")
    rsy = C.CDLL(os.path.join(HERE, "emu_resync", f"librsy_emu{width}.so"))
    _against_records((part, streams, g, wants), lambda s, cap, wbits: rsy_uncompress(rsy, s, cap, wbits)[:3], "resync")


@pytest.mark.parametrize("width", ["16", "64"], ids=["group16", "wave64"])
def test_indexed_path_equals_the_records(golden, paths_built, width):
    from test_inflate_chunks_emu import CHUNK
    from test_inflate_index_emu import build, indexed, load
    recs, streams, g, wants = golden
    L = load(f"libidx_emu{width}.so")
    took = []

    def uncompress(s, cap, wbits):
        rc, out, used, npieces, blob = build(L, s, cap, wbits, CHUNK)
        assert (blob is not None) == (npieces > 1)
        again = indexed(L, s, cap, wbits, blob)
        assert again == (rc, out, used, npieces if blob is not None else 0), (len(s), cap)
        took.append(npieces)
        return rc, out, used

    _against_records((path_records(recs), streams, g, wants), uncompress, "indexed")
    assert sum(1 for n in took if n > 1) >= len(B.composed_names())


def test_size_and_check_paths_equal_the_records(golden, paths_built, tmp_path):
    from test_inflate_check_emu import run_emu as run_check
    from test_inflate_size_emu import CHUNK, LANES, NEVER_CUT, run_emu as run_size, with_right_check
    recs, streams, g, wants = golden
    part = path_records(recs)
    jobs, rows_of = [], []
    for r in part:
        s = streams[r.name][:r.cut]
        # the size path's documented exception (the trailer's check value is not compared) changes nothing
        # here: no hand-built stream carries a wrong check value
        assert with_right_check(s, r.window_bits) in (None, s), (r.name, r.cut)
        for chunk in (CHUNK, NEVER_CUT):
            jobs.append((s, r.window_bits, r.cap, chunk))
            rows_of.append(r)
    chunked = 0
    for lanes in LANES:
        for row, r, job in zip(run_size(tmp_path, lanes, jobs), rows_of, jobs):
            assert row[:3] == (r.rc, r.out_len, r.consumed), ("size", lanes, r.name, r.cut, r.cap, row)
            assert row[3] == 0 or (job[3] == CHUNK and row[3] > 1), ("size", lanes, r.name, row)
        for row, r, job in zip(run_check(tmp_path, lanes, jobs), rows_of, jobs):
            value = B.check_value(wants[r.name], r.window_bits) if r.rc == 0 else 0
            assert (row[0], row[1], row[2], row[5]) == (r.rc, r.out_len, r.consumed, value), \
                ("check", lanes, r.name, r.cut, r.cap, row)
            chunked += row[3] > 1
    assert chunked >= len(LANES) * len(B.composed_names())
