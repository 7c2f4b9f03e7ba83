"""The deflate block coder (huff_plan.h, bit_emit.h) on inputs built to reach its edge paths
(tests/deflate_cases.py), on the CPU.

For every case: the oracle's stream decodes to the input with stock zlib; the walker of deflate_cases finds in
it the features the case was built for (a fixture that stops reaching its path fails here, not silently);
the oracle equals the record of tests/golden/deflate_edges_golden.json (made from the compiled reference) and
the compiled reference itself where it is built; and the 64-lane emulation of the kernels equals the oracle
byte for byte.  tests/test_gpu_deflate_edges.py runs the same cases through the GPU build.
"""
import ctypes as C
import os
import zlib

import pytest

import deflate_cases as D
from test_emu_kernels import emu_compress

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def streams(oracle):
    """{case name: (rc, the oracle's stream)}"""
    out = {}
    for c in D.cases():
        rc, s, _ = oracle.compress(c.data, c.level, window_bits=c.window_bits, mem_level=c.mem_level,
                                   strategy=c.strategy, work_len=1 << 20)
        out[c.name] = (rc, s)
    return out


@pytest.fixture(scope="module")
def walked(streams):
    """{case name: blocks}; the walker's output is checked against the input on the way"""
    out = {}
    for c in D.cases():
        rc, s = streams[c.name]
        assert rc == 0, c.name
        blocks, data, end = D.walk(s, c.window_bits)
        trailer = 0 if c.window_bits < 0 else 8 if c.window_bits > 15 else 4
        assert data == c.data and (end + 7) // 8 + trailer == len(s), c.name
        out[c.name] = blocks
    return out


def by_family(letter):
    return [c for c in D.cases() if c.family == letter]


def test_the_cases_are_what_the_families_list():
    cases = D.cases()
    assert {c.family for c in cases} == set("ABCDEFGH")
    assert all(len(c.data) <= 120000 for c in cases)
    assert len(by_family("F")) == 4 * 4 * 301 and len(D.f_groups(cases)) == 16
    assert {(c.mem_level, len(c.data)) for c in by_family("E") if c.strategy == D.HUFFMAN_ONLY} == \
        {(8, n) for n in (16382, 16383, 16384, 32766, 32767)} | {(1, n) for n in (126, 127, 128, 254, 255)} | \
        {(9, 32767), (9, 32768)}
    assert {(c.mem_level, len(c.data)) for c in by_family("E") if c.strategy == D.FIXED} == \
        {(c.mem_level, len(c.data)) for c in by_family("E") if c.strategy == D.HUFFMAN_ONLY}
    assert {c.window_bits for c in by_family("A")} == {15, -15, 31}
    assert {c.strategy for c in by_family("A")} == {D.HUFFMAN_ONLY, D.DEFAULT, D.FILTERED}
    assert len(by_family("C")) >= 3


def test_walker_and_classifier_on_a_stream_made_by_hand():
    """the walker reads what deflate_builder wrote, and the classifier's tree depths are the textbook's"""
    import deflate_builder as B
    for name, stream, cap, wbits, want in B.cases():
        if want is None or name.startswith("composed-"):
            continue
        blocks, out, end = D.walk(stream, wbits)
        assert out == want, name
    assert D.huffman_depth([1, 1, 2, 3, 5, 8])[0] == 5 and D.huffman_depth([5])[0] == 1
    assert D.huffman_depth([1] * 8)[0] == 3 and D.huffman_cost([1] * 8) == 24
    assert D.nodes_over([1, 1, 2, 3, 5, 8], 3) == 4   # two leaves and an internal node at depth 4 and 5 ...
    assert D.repaired([1, 1, 2, 4], [3, 3, 2, 1]) is False and D.repaired([1, 1, 2, 4], [2, 2, 2, 2]) is True


def test_streams_decode_with_stock_zlib(streams):
    for c in D.cases():
        rc, s = streams[c.name]
        d = zlib.decompressobj(c.window_bits)
        assert rc == 0 and d.decompress(s) == c.data and d.eof and not d.unused_data, c.name


def test_every_case_reaches_its_path(walked):
    for c in D.cases():
        got = D.features(walked[c.name])
        assert c.require <= got, (c.name, sorted(map(str, c.require - got)))
    # what no compressor can write (deflate_cases.family_d says why)
    assert not any("hclen4" in D.features(walked[c.name]) for c in D.cases())


def test_family_features(walked):
    feats = {c.name: D.features(walked[c.name]) for c in D.cases()}

    def union(cases):
        out = set()
        for c in cases:
            out |= feats[c.name]
        return out

    a, b, c_, d = union(by_family("A")), union(by_family("B")), union(by_family("C")), union(by_family("D"))
    assert {"lit_over", "lit_repaired", "lit_over_twice", "hlit257", "hclen19"} <= a
    assert {"dist1", "hlit286", "lit_over", "lit_repaired"} <= b
    # a 15-bit length code with five extra bits and the one-bit distance code
    assert max(max(blk.sym_bits) for blk in walked["B-rle-fib17"]) == 21
    assert {"bl_over", "bl_repaired", "bl_over_twice"} <= c_
    assert sum("bl_over" in feats[c.name] for c in by_family("C")) >= 3
    assert {(17, 3), (17, 10), (18, 11), (18, 138), (16, 3), (16, 6), ("split", 139), ("split", 140), "hclen19",
            ("hclen", 12)} <= d
    assert {("zeros", n) for n in (2, 3, 10, 11, 138, 139, 140)} <= d
    assert {("same", n) for n in (3, 4, 6, 7, 8, 9)} <= d
    # a run of 139 zeros goes out as 138 and a single zero, never as 11 + 128 or the like
    blk = walked["D-zero-139"][0]
    at = blk.header_syms.index((18, 138))
    assert blk.header_syms[at + 1] == (0, 1) and blk.header_syms[at + 2][0] != 0
    blk = walked["D-zero-140"][0]
    at = blk.header_syms.index((18, 138))
    assert blk.header_syms[at + 1:at + 3] == [(0, 1), (0, 1)] and blk.header_syms[at + 3][0] != 0
    # E: an input that ends on the cut leaves an empty static block of 10 bits behind full blocks
    for c in by_family("E"):
        if "tiny_block" in c.require:
            blocks = walked[c.name]
            assert (blocks[-1].type, blocks[-1].bits, blocks[-1].out_len) == (1, 10, 0), c.name
            cap = (1 << (c.mem_level + 6)) - 1
            assert [blk.out_len for blk in blocks[:-1]] == [cap] * (len(c.data) // cap), c.name
    blocks = walked["E-huff-mem8-16384"]
    assert (blocks[-1].type, blocks[-1].bits, blocks[-1].out_len) == (1, 18, 1)
    # F: all three block types, per parameter set with a free choice; stored and static under Z_FIXED
    for level, strat in D.F_PARAMS:
        got = union(c for c in by_family("F") if (c.level, c.strategy) == (level, strat))
        want = {"stored", "static"} | ({"dynamic"} if strat == D.DEFAULT else set())
        assert got & {"stored", "static", "dynamic"} == want, (level, strat)
    # G and H: the parse is the planned one, symbol for symbol
    for name, plan, depth, step in (("G-long-symbols", D.long_symbol_plan(23), 14, 1195),
                                    ("H-dist-fib17", D.long_symbol_plan(29, chain=17, flat=False), 16, 1250)):
        blocks = walked[name]
        assert [blk.type for blk in blocks] == [0, 0, 2], name
        blk = blocks[2]
        hist = [0] * 30
        for code, length, sep in plan:
            hist[code] += 1
        assert blk.dist_hist == hist, name
        assert D.huffman_depth(blk.dist_hist)[0] == depth and max(blk.sym_bits) >= 45, name
        # the rare long matches head the block: its first step carries the most bits
        assert D.step_bits(blk) == sum(blk.sym_bits[:64]) == step, name
    assert "dist_over" not in feats["G-long-symbols"] and max(walked["H-dist-fib17"][2].dist_lens) == 15


def test_oracle_equals_the_golden_records(streams):
    D.check_against_golden(D.load_golden(), D.cases(), streams, "oracle")


def test_reference_equals_the_oracle(streams, live_reference):
    if live_reference is None:
        return  # (the golden records were made from it; where it is not built they stand for it, above)
    for c in D.cases():
        rc, out = live_reference.compress(c.data, c.level, window_bits=c.window_bits, mem_level=c.mem_level,
                                          strategy=c.strategy, work_len=1 << 20)
        assert (rc, out) == streams[c.name], c.name


def test_lane_emulation_equals_the_oracle(streams):
    """checksum + parse + huffman plan + layout + emit of the kernel sources, 64 lanes, byte for byte"""
    L = C.CDLL(os.path.join(HERE, "emu", "libzsc_emu.so"))
    try:
        for c in D.cases():
            wrap, wbits = (0, -c.window_bits) if c.window_bits < 0 else (2, c.window_bits - 16) \
                if c.window_bits > 15 else (1, c.window_bits)
            L.emu_set_params(wbits, c.mem_level)
            rc, got = emu_compress(L, c.data, c.level, wrap, c.strategy)
            assert (rc, got) == streams[c.name], c.name
    finally:
        L.emu_set_params(15, 8)
