"""The block planner (zsc_amd/csrc/huff_plan.h: packed heap, lane-parallel code assignment) on inputs built for
what it does with a block (tests/huff_plan_cases.py), on the CPU.

For every case: the walker of deflate_cases finds in the oracle's stream the features the case was built for;
the 64-lane emulation of the whole pipeline gives the oracle's stream byte for byte; and the planner alone
(tests/emu_huff), fed the oracle's symbols and block cuts, writes the same plans at 64, 16 and 8 lanes per
wave -- at the narrow widths every lane-parallel part takes several steps per tree -- whatever was left in its
LDS image.  tests/test_gpu_huff_plan.py runs the same cases through the GPU build.
"""
import ctypes as C
import os
import zlib

import pytest

import deflate_cases as D
import huff_plan_cases as H
from test_emu_kernels import emu_compress

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def streams(oracle):
    """{case name: (rc, the oracle's stream)}"""
    return {c.name: oracle.compress(c.data, c.level, window_bits=c.window_bits, mem_level=c.mem_level,
                                    strategy=c.strategy, work_len=1 << 20)[:2] for c in H.cases()}


@pytest.fixture(scope="module")
def parses(oracle):
    """{case name: (symbols as the kernels hold them, block records as nine words each, block count)}"""
    out = {}
    for c in H.cases():
        syms, ns, blocks, nb = oracle.parse(c.data, c.level, c.window_bits, c.mem_level, c.strategy)
        words = (C.c_uint32 * (ns + 64))(*[(syms[i].dist << 16) | syms[i].lc for i in range(ns)])
        recs = (C.c_uint32 * (9 * max(nb, 1)))()
        for b in range(nb):
            recs[9 * b:9 * b + 6] = [blocks[b].sym_begin, blocks[b].sym_count, blocks[b].in_begin, blocks[b].in_len,
                                     blocks[b].stored_ok, blocks[b].last]
        out[c.name] = (words, recs, nb)
    return out


def planner(lanes):
    L = C.CDLL(os.path.join(HERE, "emu_huff", "libhuff_emu%d.so" % lanes))
    assert L.emu_huff_lanes() == lanes
    return L


def plans_of(L, parse, strategy, fill):
    words, recs, nb = parse
    size = L.emu_huff_plan(None, None, 0, 0, None, 0)
    out = C.create_string_buffer(size * max(nb, 1))
    L.emu_huff_plan(words, recs, nb, strategy, out, fill)
    return out.raw[:size * nb]


def paths_of(L, clear=True):
    p = (C.c_ulonglong * 16)()
    L.emu_huff_paths(p, 1 if clear else 0)
    return list(p)


def test_every_case_reaches_its_path(streams):
    """with the oracle alone: the stream decodes to the input, and the walker finds what the case was built for"""
    for c in H.cases():
        rc, s = streams[c.name]
        assert rc == 0, c.name
        d = zlib.decompressobj(c.window_bits)
        assert d.decompress(s) == c.data and d.eof, c.name
        blocks, data, end = D.walk(s, c.window_bits)
        assert data == c.data, c.name
        got = D.features(blocks)
        assert c.require <= got, (c.name, sorted(map(str, c.require - got)))
    by = {c.name: D.walk(streams[c.name][1], c.window_bits)[0] for c in H.cases()}
    # one block each, but for the cases that are about several
    assert len(by["blocks-mem1-text"]) > 8 and len(by["blocks-mem1-skewed"]) > 20
    assert [b.out_len for b in by["fib18-full-block"]] == [16383, 0]
    assert [b.out_len for b in by["fib20-full-block-mem9"]] == [32767, 0]
    # the Fibonacci counts make trees far deeper than the limit of 15, and deeper with the block's size
    assert D.huffman_depth(by["fib18"][0].lit_hist)[0] == 18
    assert D.huffman_depth(by["fib20-full-block-mem9"][0].lit_hist)[0] == 20
    blk = by["all-codes"][0]
    assert all(blk.lit_hist) and all(blk.dist_hist) and len(blk.lit_hist) == 286 and len(blk.dist_hist) == 30
    assert len(set(blk.dist_hist)) <= 3 and len(by["all-codes"]) == 1     # (many equal counts)
    assert set(by["flat-128"][0].lit_hist[:128]) == {100} and set(by["flat-256-copies"][0].lit_hist[:256]) <= {1, 2}
    assert sum(1 for x in by["one-distance"][0].dist_hist if x) == 1


def test_whole_streams_of_the_64_lane_emulation_equal_the_oracle(streams):
    """checksum + parse + huffman plan + layout + emit of the kernel sources, 64 lanes, byte for byte"""
    L = C.CDLL(os.path.join(HERE, "emu", "libzsc_emu.so"))
    try:
        for c in H.cases():
            L.emu_set_params(c.window_bits, c.mem_level)
            rc, got = emu_compress(L, c.data, c.level, 1, c.strategy)
            assert (rc, got) == streams[c.name], c.name
    finally:
        L.emu_set_params(15, 8)


def test_plans_are_the_same_at_every_wave_width_and_lds_state(parses):
    """the planner alone on the oracle's parse: 64 lanes (the width whose streams the test above pins to the
    oracle) against 16 and 8 lanes, and against another fill of the LDS image"""
    L64, L16, L8 = planner(64), planner(16), planner(8)
    for c in H.cases():
        want = plans_of(L64, parses[c.name], c.strategy, 0x5A)
        assert len(want) > 0 or not c.data or parses[c.name][2] == 0, c.name
        assert plans_of(L64, parses[c.name], c.strategy, 0xFF) == want, c.name
        assert plans_of(L64, parses[c.name], c.strategy, 0x00) == want, c.name
        assert plans_of(L16, parses[c.name], c.strategy, 0x5A) == want, c.name
        assert plans_of(L8, parses[c.name], c.strategy, 0xA5) == want, c.name


def test_the_planner_takes_the_rare_paths_the_cases_are_for(parses):
    """the planner's own hooks: forced nodes, the overflow repair per tree, the block types"""
    L = planner(64)
    paths_of(L)
    hit = {}
    for c in H.cases():
        plans_of(L, parses[c.name], c.strategy, 0x5A)
        hit[c.name] = paths_of(L)
    FORCED, OVER_LIT, OVER_DIST, OVER_BL, STORED, STATIC, DYNAMIC = range(7)
    assert hit["empty"][FORCED] == 3            # one literal/length node, two distance nodes
    assert hit["one-literal"][FORCED] == 2 and hit["one-distance"][FORCED] == 1
    assert hit["one-distance-29"][FORCED] >= 1 and hit["all-codes"][FORCED] == 0
    for name in ("fib18", "fib18-full-block", "fib20-full-block-mem9"):
        assert hit[name][OVER_LIT] == 1, name
    assert hit["bl-over"][OVER_BL] >= 1 and hit["bl-over-twice"][OVER_BL] >= 1
    assert hit["flat-128"][OVER_LIT] == 0 and hit["flat-128"][DYNAMIC] == 1 and hit["flat-256"][STORED] == 1
    assert hit["stored-wins"][STORED] == 1 and hit["static-wins"][STATIC] == 1
    assert hit["fixed"][STATIC] >= 1 and hit["fixed"][DYNAMIC] == 0
    assert hit["blocks-mem1-text"][DYNAMIC] > 8


def test_lds_per_wave():
    """32 waves per CU need 5 120 bytes or less of the CU's 160 KiB each"""
    assert planner(64).emu_huff_lds_bytes() <= 5120
