"""Inputs of at most 64 KiB built to reach what the block planner (zsc_amd/csrc/huff_plan.h) does with a block:
the packed heap's ties and depth field, forced nodes, the overflow repair of each tree, the run-length coding
of the header, the three block types, and consecutive blocks in one wave's LDS image.

Shared by tests/test_huff_plan_emu.py (CPU, lane emulation) and tests/test_gpu_huff_plan.py.  The builders are
those of tests/deflate_cases.py; `require` names features its walker must find in the oracle's stream.
"""
import deflate_cases as D

HUFFMAN_ONLY, FIXED, DEFAULT = D.HUFFMAN_ONLY, D.FIXED, D.DEFAULT

# (code length, how many neighbouring byte values get it): runs of one length of exactly 138, 2, 3, 6, 7, 10, 11
SAME_GROUPS = [(8, 138), (9, 2), (10, 3), (9, 6), (10, 7), (9, 10), (10, 11), (11, 1)]
SAME_RUNS = (2, 3, 6, 7, 10, 11, 138)


def _fib_block(terms, symbols):
    """`terms` byte values in the Fibonacci counts 1, 2, 3, 5, ... (END_BLOCK is the other 1), the most frequent
    one padded so that the input has `symbols` bytes (0: as they are)"""
    counts = D.fib(terms)
    if symbols:
        assert sum(counts) <= symbols
        counts[-1] += symbols - sum(counts)
    return D.shuffled(counts, range(65, 65 + terms), terms)


def _all_codes():
    """every literal, every length code and every distance code in one block (mem_level 9: 32 767 symbols), the
    length and distance codes four times each"""
    plan, slot = [], 0
    for dc in range(30):
        for k in range(4):
            # copies of 3 to 10 bytes from the near distances (ten per length code); the 21 longer length codes,
            # once or twice each, from 1 025 bytes back and more, where the source lies in the matchless prefix
            plan.append((dc, D.LEN_BASE[slot % 8 if dc < 20 else 8 + (slot - 80) % 21], True))
            slot += 1
    r = D.B.Lcg(5)
    r.shuffle(plan)
    return D.copies_input(37, plan, prefix=26000)


_CASES = []


def cases():
    if _CASES:
        return _CASES
    C = D.Case
    flat = bytes(range(256)) * 63
    over = {"lit_over", "lit_repaired", "dynamic", "dist0"}
    from zsc_amd import corpus
    text = corpus.make_buffer("text", 5000, 3)
    out = [
        # ---- literal/length and distance trees
        C("empty", b"", strategy=HUFFMAN_ONLY, require={"static", "dist0"}),
        C("one-literal", b"a" * 5000, strategy=HUFFMAN_ONLY, require={"dynamic", "dist0"}),
        C("one-literal-short", b"a", strategy=HUFFMAN_ONLY, require={"static", "dist0"}),
        C("two-literals", b"ab" * 2500, strategy=HUFFMAN_ONLY, require={"dynamic", "dist0"}),
        C("one-distance", b"a" * 5000, require={"dist1"}),
        # (stored in the end: the planner builds its trees before it knows; the emulation test counts the forced node)
        C("one-distance-29", D.copies_input(41, [(29, 5, True)] * 3, prefix=26000), mem_level=9, require={"stored"}),
        # all 256 literals equally frequent: as literals alone the block goes out stored, so also once each in
        # front of copies of themselves, and 128 of them (seven bits each: dynamic wins)
        C("flat-256", D.shuffled([63] * 256, range(256), 1), strategy=HUFFMAN_ONLY, require={"stored"}),
        C("flat-256-copies", flat, require={"dynamic", "dist1"}),
        C("flat-128", D.shuffled([100] * 128, range(128), 2), strategy=HUFFMAN_ONLY, require={"dynamic", "dist0"}),
        C("all-codes", _all_codes(), mem_level=9, require={"hlit286", "hdist30", "dynamic"}),
        C("fib18", _fib_block(18, 0), strategy=HUFFMAN_ONLY, require=over | {"lit_over_twice"}),
        C("fib18-full-block", _fib_block(18, 16383), strategy=HUFFMAN_ONLY, require=over | {"tiny_block"}),
        C("fib20-full-block-mem9", _fib_block(20, 32767), mem_level=9, strategy=HUFFMAN_ONLY,
          require=over | {"tiny_block"}),
        # ---- the bit-length tree and the header's run lengths
        C("bl-over", D.profile_input(D.BL_OVER_SEEDS[0]), strategy=HUFFMAN_ONLY, require={"bl_over", "bl_repaired"}),
        C("bl-over-twice", D.profile_input(D.BL_OVER_TWICE_SEEDS[0]), strategy=HUFFMAN_ONLY,
          require={"bl_over", "bl_repaired", "bl_over_twice"}),
        C("same-runs", D.header_edges_input([], SAME_GROUPS), strategy=HUFFMAN_ONLY,
          require={("same", n) for n in SAME_RUNS} | {"dynamic"}),
        C("zero-runs", D.header_edges_input([2, 3, 10, 11, 138], [(7, 3), (8, 4), (7, 6), (8, 7), (7, 8), (8, 9), (9, 1)]),
          strategy=HUFFMAN_ONLY,
          require={("zeros", n) for n in (2, 3, 10, 11, 138)} | {(17, 3), (17, 10), (18, 11), (18, 138), "dynamic"}),
        # the literal/length lengths end with END_BLOCK behind a run of zeros, and the distance lengths begin anew
        C("zeros-to-max-code", D.shuffled(D.fib(12), range(20, 32), 4), strategy=HUFFMAN_ONLY,
          require={("zeros", 20), ("zeros", 224), ("split", 224), "hlit257", "dynamic"}),
        # ---- block types
        C("static-wins", text[:40], require={"static"}),
        C("stored-wins", D.B.Lcg(9).bytes(1000), require={"stored"}),
        C("fixed", text[:3000], strategy=FIXED, require={"static"}),
        # ---- many blocks per buffer: 127 symbols each
        C("blocks-mem1-text", text, mem_level=1, require={"dynamic"}),
        C("blocks-mem1-skewed", D.skewed(3000, 8), mem_level=1, strategy=HUFFMAN_ONLY, require={"dynamic"}),
    ]
    assert all(len(c.data) <= 65536 for c in out)
    _CASES.extend(out)
    return _CASES


def groups():
    """{(level, window_bits, mem_level, strategy): cases}"""
    out = {}
    for c in cases():
        out.setdefault(c.params, []).append(c)
    return out
