"""The match search and the parsers (lz_parse_seg.h, lz_parse.h, lz_parse_pipe.h, lz_parse_simple.h) on inputs
built for their edges (tests/parser_cases.py), on the CPU.

For every case: the oracle's stream is the compiled reference's (live where it is built, and its record in
tests/golden/parser_edges_golden.json), stock zlib inflates it back to the input, and the walker finds in it the
tokens the case was built to show.  The 64-lane emulation gives that stream through every parser that can take
the case, the 16-lane build gives the oracle's stage P, and with the product's defaults every case reaches the
path hooks (SG_PATH) it was built for; together the cases reach every hook there is.
tests/test_gpu_parser_edges.py runs the same cases through the GPU build.
"""
import ctypes as C
import os
import subprocess
import zlib

import pytest

import parser_cases as P
from zsc_amd import corpus

HERE = os.path.dirname(os.path.abspath(__file__))
NPATH = 128
PIPE_PATHS = {56, 57, 58, 59}   # the pipeline's resolver: counted where the pipeline schedule is run (emu_pipe)


class Rec(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("sym_begin", "sym_count", "in_begin", "in_len", "stored_ok", "last", "cut", "wend", "at")]


def load(path):
    L = C.CDLL(path)
    L.emu_set_stair_min.argtypes = [C.c_uint32]
    L.emu_parse.argtypes = [C.c_char_p, C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                            C.POINTER(Rec), C.POINTER(C.c_uint32)]
    return L


def defaults(L):
    """the state tests/test_emu_kernels.py expects of the library it shares with this module"""
    L.emu_set_params(15, 8)
    L.emu_set_seg_mode(0)
    L.emu_set_table(1)
    L.emu_set_stair_min(0)
    L.emu_set_one(1)
    L.emu_set_fast_global(1)


def product(L, case):
    """the product's defaults: no match table, the staircase from 256 entries on, the lane-parallel search, the
    greedy parser without an LDS window, and the parser the runtime sends a buffer of this length to"""
    configure(L, case, 2 if case.segmented else 1, 0, 256, 1, 1)


def configure(L, case, seg_mode, table, stair_min, one, fast_global):
    L.emu_set_params(abs(case.window_bits), case.mem_level)
    L.emu_set_seg_mode(seg_mode)
    L.emu_set_table(table)
    L.emu_set_stair_min(stair_min)
    L.emu_set_one(one)
    L.emu_set_fast_global(fast_global)


def compress(L, case):
    n = len(case.data)
    cap = n + (n >> 3) + 256
    out, ol = C.create_string_buffer(cap), C.c_uint32()
    rc = L.emu_compress(case.data, n, case.level, 0 if case.window_bits < 0 else 1, case.strategy, out, cap, C.byref(ol))
    return rc, out.raw[:ol.value]


def paths(L):
    return list((C.c_ulonglong * NPATH).in_dll(L, "g_sg_path"))


def configs(case):
    """(seg_mode, table, stair_min, one, fast_global) for every parser that can take the case"""
    if case.strategy in (P.RLE, P.HUFFMAN_ONLY):
        return [(0, 0, 256, 1, 1)]
    if not P.levels()[case.level]["slow"]:
        return [(0, 0, 256, 1, 1), (0, 0, 256, 1, 0)]
    out = [(2, 0, 256, 1, 1), (3, 0, 256, 1, 1), (1, 0, 256, 1, 1), (2, 0, 0, 1, 1), (2, 0, 256, 0, 1), (3, 0, 0, 0, 1)]
    if abs(case.window_bits) == 15 and case.mem_level == 8:
        out += [(2, 1, 256, 1, 1), (3, 1, 0, 1, 1)]
    return out


@pytest.fixture(scope="module")
def emu64():
    L = load(os.path.join(HERE, "emu", "libzsc_emu.so"))
    yield L
    defaults(L)


@pytest.fixture(scope="module")
def emu16():
    L = load(os.path.join(HERE, "emu", "libzsc_emu16.so"))
    yield L
    defaults(L)


@pytest.fixture(scope="module")
def streams(oracle):
    """{case name: (rc, the oracle's stream)}"""
    out = {}
    for c in P.cases():
        rc, s, _ = oracle.compress(c.data, c.level, window_bits=c.window_bits, mem_level=c.mem_level,
                                   strategy=c.strategy, work_len=1 << 20)
        out[c.name] = (rc, s)
    return out


def test_the_cases_keep_the_fixed_conditions():
    cases = P.cases()
    assert {c.family for c in cases} == set("ABCDEFGHIJK")
    assert len({c.params for c in cases}) <= 40
    assert sum(len(c.data) for c in cases) <= 6 << 20
    assert all(c.features for c in cases)
    # every hook has a case built for it, and every id a case names is a hook
    built_for = set().union(*(c.paths | c.ring_paths for c in cases))
    assert built_for == set(P.PATHS) - PIPE_PATHS, sorted(set(P.PATHS) - built_for)
    # twins for the wave-per-buffer parser, and the sizes its ring classes are chosen by
    slow = [len(c.data) for c in cases if P.levels()[c.level]["slow"] and c.strategy in (P.DEFAULT, P.FILTERED, P.FIXED)]
    assert any(n <= P.SEG_MIN for n in slow) and any(P.SEG_MIN < n <= 6144 for n in slow)
    assert any(6144 < n <= 10240 for n in slow) and any(10240 < n <= 18432 for n in slow) and any(n > 18432 for n in slow)


def test_walker_reads_the_tokens_of_a_stream():
    """the token list is the walker's own: it covers the output without a gap, every copy replays, literals and a
    copy that overlaps itself are where they are in a stream of stock zlib's, a stored block is one entry"""
    data = b"abcabcabcabcabcabcX" + bytes(range(40))
    raw = zlib.compressobj(9, zlib.DEFLATED, -15)
    ps = P.Parse(raw.compress(data) + raw.flush(), -15)
    assert ps.data == data
    at = 0
    for pos, n, dist in ps.tokens:
        assert pos == at and (n == 1) == (dist == 0)
        assert dist == 0 or all(data[pos + i] == data[pos + i - dist] for i in range(n))
        at += n
    assert at == len(data)
    copies = [t for t in ps.tokens if t[2]]
    assert len(copies) == 1 and copies[0][2] == 3 and copies[0][0] + copies[0][1] == 18   # (it overlaps itself)
    pos, n, dist = copies[0]
    assert ps.holds(("copy", pos, n, 3)) is None and ps.holds(("lits", 0, 3)) is None
    assert ps.holds(("copy", pos, n, 4)) is not None and ps.holds(("copy", pos, n - 1, 3)) is not None
    assert ps.holds(("lits", pos - 1, 2)) is not None and ps.holds(("copy_end", 18, 3)) is None
    assert ps.holds(("copy_end", 18, 2)) is not None and ps.holds(("lits", 18, 41)) is None
    stored = zlib.compressobj(0, zlib.DEFLATED, -15)
    ps = P.Parse(stored.compress(b"hello") + stored.flush(), -15)
    assert ps.tokens == [(0, 5, -1)] and ps.holds(("lits", 0, 1)) == "stored block"
    assert ps.holds(("stored", (True,))) is None and ps.holds(("stored", (False,))) is not None


def test_reference_streams_show_every_feature(streams, live_reference):
    golden = P.load_golden()["cases"]
    cases = P.cases()
    assert set(golden) == {c.name for c in cases}
    for c in cases:
        rc, s = streams[c.name]
        assert rc == 0, c.name
        d = zlib.decompressobj(c.window_bits)
        assert d.decompress(s) == c.data and d.eof and not d.unused_data, c.name
        ps = P.Parse(s, c.window_bits)
        assert ps.data == c.data, c.name
        # the oracle's stream is the reference's: its record, and the reference itself where it is built
        assert [rc, len(s), P.sha(s), ps.summary(c.features)] == golden[c.name], c.name
        if live_reference is not None:
            got = live_reference.compress(c.data, c.level, window_bits=c.window_bits, mem_level=c.mem_level,
                                          strategy=c.strategy, work_len=1 << 20)
            assert (got[0], got[1]) == (rc, s), c.name
        assert not ps.missing(c.features), (c.name, ps.missing(c.features))


def test_lane_emulation_gives_the_oracle_stream_through_every_parser(emu64, streams):
    for c in P.cases():
        for cfg in configs(c):
            configure(emu64, c, *cfg)
            assert compress(emu64, c) == streams[c.name], (c.name, cfg)


def test_sixteen_lane_groups_give_the_oracle_stage_p(emu16, oracle):
    """the segmented parser at the width its group code has on the GPU: symbols and block records"""
    for c in P.cases():
        if not c.segmented:
            continue
        n = len(c.data)
        osy, ons, obl, onb = oracle.parse(c.data, c.level, abs(c.window_bits), c.mem_level, c.strategy)
        want = ([(osy[i].dist << 16) | osy[i].lc for i in range(ons)],
                [(b.sym_begin, b.sym_count, b.in_begin, b.in_len, b.stored_ok, b.last) for b in (obl[i] for i in range(onb))])
        for cfg in ((2, 0, 256, 1, 1), (3, 0, 0, 0, 1)):
            configure(emu16, c, *cfg)
            syms = (C.c_uint32 * (n + 64))()
            blocks = (Rec * (n // ((1 << (c.mem_level + 6)) - 1) + 4))()
            ns, nb = C.c_uint32(), C.c_uint32()
            assert emu16.emu_parse(c.data, n, c.level, c.strategy, syms, C.byref(ns), blocks, C.byref(nb)) == 0, c.name
            got = (list(syms[:ns.value]),
                   [(b.sym_begin, b.sym_count, b.in_begin, b.in_len, b.stored_ok, b.last) for b in blocks[:nb.value]])
            assert got == want, (c.name, cfg)


def corpus_inputs():
    """the buffers the older emulation tests feed the parsers (tests/test_lazy_search_emu.py and the search modes
    of tests/test_emu_kernels.py), as cases with the product's defaults"""
    out = []
    for kind in ("text", "table", "bitmap", "random", "zero", "runs"):
        for n in (3073, 4099, 32769, 70001):
            for level in (4, 6, 9, 1):
                out.append(P.Case("corpus", corpus.make_buffer(kind, n, n + 5), level, 15, 8, P.DEFAULT, ()))
    return out


def test_every_case_reaches_the_paths_it_was_built_for(emu64, streams, capsys):
    total = [0] * NPATH
    for c in P.cases():
        product(emu64, c)
        before = paths(emu64)
        assert compress(emu64, c) == streams[c.name], c.name
        hit = [a - b for a, b in zip(paths(emu64), before)]
        missed = sorted(i for i in c.paths if not hit[i])
        assert not missed, (c.name, [(i, P.PATHS[i]) for i in missed])
        assert not [i for i in c.avoid if hit[i]], (c.name, [(i, P.PATHS[i]) for i in c.avoid if hit[i]])
        total = [a + b for a, b in zip(total, hit)]
        if c.ring_paths:   # the same buffer through the wave-per-buffer parser, as the runtime can be told to send it
            configure(emu64, c, 1, 0, 256, 1, 1)
            before = paths(emu64)
            assert compress(emu64, c) == streams[c.name], c.name
            hit = [a - b for a, b in zip(paths(emu64), before)]
            missed = sorted(i for i in c.ring_paths if not hit[i])
            assert not missed, (c.name, "wave-per-buffer", [(i, P.PATHS[i]) for i in missed])
            total = [a + b for a, b in zip(total, hit)]
    old = [0] * NPATH
    for c in corpus_inputs():
        product(emu64, c)
        before = paths(emu64)
        assert compress(emu64, c)[0] == 0
        old = [a + b - x for a, b, x in zip(old, paths(emu64), before)]
    with capsys.disabled():
        print("\npath hooks: id, corpus inputs, new cases, meaning")
        for i in sorted(set(P.PATHS) - PIPE_PATHS):
            print("  %3d %9d %9d  %s" % (i, old[i], total[i], P.PATHS[i]))
    assert all(total[i] for i in set(P.PATHS) - PIPE_PATHS), [i for i in P.PATHS if not total[i]]
    assert not any(total[i] or old[i] for i in range(NPATH) if i not in P.PATHS)


@pytest.fixture(scope="module")
def pipe():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_pipe")], check=True)
    L = load(os.path.join(HERE, "emu_pipe", "libpipe_emu64.so"))
    L.emu_pipe_open.restype = C.c_void_p
    L.emu_pipe_open.argtypes = [C.c_char_p, C.c_uint32, C.c_int, C.c_int]
    L.emu_pipe_run.argtypes = [C.c_void_p, C.c_int, C.c_uint32]
    L.emu_pipe_stream.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.emu_pipe_close.argtypes = [C.c_void_p]
    return L


def test_pipeline_schedules_give_the_oracle_stream(pipe, streams):
    """families A, C, F and G through the pipeline of segments: round robin, reverse (the parses run as far ahead
    of the resolver as the slots allow), wave 0 alone, two seeded orders"""
    before = paths(pipe)
    for c in P.cases():
        if c.family not in "ACFG" or not c.segmented:
            continue
        pipe.emu_set_params(abs(c.window_bits), c.mem_level)
        pipe.emu_set_table(0)
        pipe.emu_set_stair_min(256)
        n = len(c.data)
        for mode, seed in ((0, 0), (1, 0), (2, 0), (4, 1), (4, 2)):
            ctx = pipe.emu_pipe_open(c.data, n, c.level, c.strategy)
            try:
                assert pipe.emu_pipe_run(ctx, mode, seed) == 0, (c.name, mode, seed)
                cap = n + (n >> 3) + 256
                out, ol = C.create_string_buffer(cap), C.c_uint32()
                assert pipe.emu_pipe_stream(ctx, 0 if c.window_bits < 0 else 1, out, cap, C.byref(ol)) == 0, c.name
                assert (0, out.raw[:ol.value]) == streams[c.name], (c.name, mode, seed)
            finally:
                pipe.emu_pipe_close(ctx)
    pipe.emu_set_params(15, 8)
    hit = [a - b for a, b in zip(paths(pipe), before)]
    # the resolver's branches: hand-overs followed, redos after a give-up and at the edge of the slots, the end
    print("pipeline resolver hooks:", {i: hit[i] for i in sorted(PIPE_PATHS)})
    assert all(hit[i] for i in PIPE_PATHS), {i: hit[i] for i in sorted(PIPE_PATHS)}
