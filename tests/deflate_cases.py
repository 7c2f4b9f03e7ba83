"""Inputs built to reach the edge paths of the deflate block coder (huff_plan.h, bit_emit.h), a plain-Python
walker of DEFLATE streams, and a classifier that says which of those paths a walked block went through.

No tests live here: tests/test_deflate_edges_emu.py (CPU) and tests/test_gpu_deflate_edges.py (GPU) use it,
tests/golden/make_deflate_edges_golden.py records the compiled reference's answers for the same cases.

The walker is written from RFC 1951 alone.  It shares nothing with the kernels or the oracle, so that a
feature it reports ("this block's literal tree needed the overflow repair") is an independent statement
about the bytes of a stream.

Largest totals of one 64-symbol step of the bit packer that the walker sees: 1 195 bits in G-long-symbols and
1 250 bits in H-dist-fib17 (19 matches of 38 to 46 bits at the head of the block, then copies and literals);
the staging area of bit_emit.h holds 4 096.
"""
import hashlib
import heapq
import json
import os

import deflate_builder as B

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "deflate_edges_golden.json")

HUFFMAN_ONLY, RLE, FIXED, FILTERED, DEFAULT = 2, 3, 4, 1, 0


def sha(b):
    return hashlib.sha256(b).hexdigest()


# ---- the walker ---------------------------------------------------------------------------------------------

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227,
            258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 30


class Block:
    """one walked block; positions are bit offsets from the first byte of the stream, wrapper included"""
    __slots__ = ("type", "last", "first_bit", "end_bit", "hlit", "hdist", "hclen", "lit_lens", "dist_lens", "bl_lens",
                 "header_syms", "lit_hist", "dist_hist", "bl_hist", "sym_pos", "sym_bits", "stored_len", "out_len")

    @property
    def bits(self):
        return self.end_bit - self.first_bit


class _Bits:
    def __init__(self, data, pos):
        self.data = data + b"\0" * 8
        self.pos = pos
        self.limit = 8 * len(data)

    def take(self, n):
        p = self.pos
        v = (int.from_bytes(self.data[p >> 3:(p >> 3) + 4], "little") >> (p & 7)) & ((1 << n) - 1)
        self.pos = p + n
        if self.pos > self.limit:
            raise ValueError("stream ends inside a block")
        return v


def _table(lens):
    """(lookup table over the next `width` bits, width): entry = (symbol, code length)"""
    used = [(l, s) for s, l in enumerate(lens) if l]
    if not used:
        return None, 0
    width = max(l for l, _ in used)
    table = [None] * (1 << width)
    code, prev = 0, 0
    for l, s in sorted(used):
        code <<= l - prev
        prev = l
        rev = int(format(code, "0%db" % l)[::-1], 2)   # codes are packed starting at their most significant bit
        table[rev::1 << l] = [(s, l)] * (1 << (width - l))
        code += 1
    if code > 1 << prev:
        raise ValueError("over-subscribed code")
    return table, width


def _decode(r, table, width):
    p = r.pos
    v = (int.from_bytes(r.data[p >> 3:(p >> 3) + 4], "little") >> (p & 7)) & ((1 << width) - 1)
    e = table[v]
    if e is None:
        raise ValueError("unused code")
    r.pos = p + e[1]
    if r.pos > r.limit:
        raise ValueError("stream ends inside a block")
    return e[0]


def body_offset(stream, window_bits):
    """bytes of wrapper in front of the first block"""
    if window_bits < 0:
        return 0
    if window_bits > 15:
        assert stream[:3] == b"\x1f\x8b\x08" and stream[3] == 0
        return 10
    assert (stream[0] * 256 + stream[1]) % 31 == 0 and stream[0] & 15 == 8
    return 2


def walk(stream, window_bits=15, tokens=None):
    """-> (blocks, output bytes, bit position after the last block).  A list given as `tokens` receives the
    parse the stream states: (input position, length, distance) per copy, (position, 1, 0) per literal and
    (position, length, -1) for the bytes of a stored block, which says nothing about its parse."""
    r = _Bits(stream, 8 * body_offset(stream, window_bits))
    out = bytearray()
    blocks = []
    while True:
        b = Block()
        b.first_bit = r.pos
        b.last = r.take(1)
        b.type = r.take(2)
        b.hlit = b.hdist = b.hclen = 0
        b.lit_lens, b.dist_lens, b.bl_lens, b.header_syms = [], [], [], []
        b.lit_hist, b.dist_hist, b.bl_hist = [0] * 286, [0] * 30, [0] * 19
        b.sym_pos, b.sym_bits = [], []
        b.stored_len = 0
        start = len(out)
        if b.type == 0:
            r.pos = (r.pos + 7) & ~7
            n, c = r.take(16), r.take(16)
            if n ^ c != 0xffff:
                raise ValueError("stored length check")
            at = r.pos >> 3
            if at + n > len(stream):
                raise ValueError("stored block runs past the end")
            if tokens is not None and n:
                tokens.append((len(out), n, -1))
            out += stream[at:at + n]
            r.pos += 8 * n
            b.stored_len = n
        elif b.type == 3:
            raise ValueError("block type 3")
        else:
            if b.type == 1:
                b.lit_lens, b.dist_lens = FIXED_LIT[:], FIXED_DIST[:]
            else:
                b.hlit, b.hdist, b.hclen = r.take(5) + 257, r.take(5) + 1, r.take(4) + 4
                b.bl_lens = [0] * 19
                for k in range(b.hclen):
                    b.bl_lens[CL_ORDER[k]] = r.take(3)
                table, width = _table(b.bl_lens)
                lens = []
                while len(lens) < b.hlit + b.hdist:
                    s = _decode(r, table, width)
                    b.bl_hist[s] += 1
                    if s < 16:
                        lens.append(s)
                        b.header_syms.append((s, 1))
                        continue
                    if s == 16:
                        if not lens:
                            raise ValueError("repeat with nothing before it")
                        n = 3 + r.take(2)
                        lens += [lens[-1]] * n
                    else:
                        n = 3 + r.take(3) if s == 17 else 11 + r.take(7)
                        lens += [0] * n
                    b.header_syms.append((s, n))
                if len(lens) != b.hlit + b.hdist:
                    raise ValueError("code lengths overrun")
                b.lit_lens, b.dist_lens = lens[:b.hlit], lens[b.hlit:]
            lt, lw = _table(b.lit_lens)
            dt, dw = _table(b.dist_lens)
            while True:
                p = r.pos
                s = _decode(r, lt, lw)
                b.lit_hist[s] += 1
                if s < 256:
                    if tokens is not None:
                        tokens.append((len(out), 1, 0))
                    out.append(s)
                elif s == 256:
                    b.sym_pos.append(p)
                    b.sym_bits.append(r.pos - p)
                    break
                else:
                    if s > 285:
                        raise ValueError("length symbol out of range")
                    n = LEN_BASE[s - 257] + r.take(LEN_EXTRA[s - 257])
                    if dt is None:
                        raise ValueError("a match with no distance code")
                    d = _decode(r, dt, dw)
                    if d > 29:
                        raise ValueError("distance symbol out of range")
                    b.dist_hist[d] += 1
                    dist = DIST_BASE[d] + r.take(DIST_EXTRA[d])
                    if dist > len(out):
                        raise ValueError("distance too far back")
                    if tokens is not None:
                        tokens.append((len(out), n, dist))
                    if dist >= n:
                        out += out[-dist:len(out) - dist + n]
                    else:
                        for _ in range(n):
                            out.append(out[-dist])
                b.sym_pos.append(p)
                b.sym_bits.append(r.pos - p)
        b.end_bit = r.pos
        b.out_len = len(out) - start
        blocks.append(b)
        if b.last:
            break
    return blocks, bytes(out), r.pos


# ---- the classifier -----------------------------------------------------------------------------------------

def huffman_depth(hist):
    """(depth, nodes deeper than `limit` for limit in 0..depth) of the plain, unbounded Huffman tree of a
    histogram.  Ties in frequency go to the shallower subtree, as in zlib; one or no symbol makes depth 1."""
    heap = [(f, 0, k, (k,)) for k, f in enumerate(hist) if f]
    if len(heap) < 2:
        return 1, {k: 1 for k, f in enumerate(hist) if f}
    heapq.heapify(heap)
    depth_of = {}
    serial = len(hist)
    while len(heap) > 1:
        a = heapq.heappop(heap)
        b = heapq.heappop(heap)
        node = (a[0] + b[0], max(a[1], b[1]) + 1, serial, (a, b))
        serial += 1
        heapq.heappush(heap, node)
    # depths of all nodes, leaves and internal ones (the root has depth 0)
    stack = [(heap[0], 0)]
    while stack:
        node, d = stack.pop()
        depth_of[node[2]] = d
        if len(node[3]) == 2:
            stack += [(node[3][0], d + 1), (node[3][1], d + 1)]
    return max(depth_of.values()), depth_of


def nodes_over(hist, limit):
    """how many nodes of the plain Huffman tree lie deeper than `limit`: the count that gen_bitlen calls
    overflow (it counts internal nodes too); its first repair loop takes two off per turn"""
    depth, depth_of = huffman_depth(hist)
    return sum(1 for d in depth_of.values() if d > limit) if depth > limit else 0


def huffman_cost(hist):
    """the bits that an unbounded Huffman code spends on a histogram (the same for every way of breaking ties)"""
    heap = [f for f in hist if f]
    heapq.heapify(heap)
    total = 0
    while len(heap) > 1:
        a = heapq.heappop(heap) + heapq.heappop(heap)
        total += a
        heapq.heappush(heap, a)
    return total


def repaired(hist, lens):
    """the code spends more than a Huffman code would: its lengths were cut down to the limit.  Unlike the
    depth of one Huffman tree among several equally good ones, this is a property of the stream."""
    return sum(f * l for f, l in zip(hist, lens)) > huffman_cost(hist)


def classify(b):
    """named features of one walked block:
      stored / static / dynamic, tiny_block (32 bits or fewer);
      sym>=34, sym>=44 (a symbol of that many bits), spill3 (one that reaches into a third 32-bit word);
      dist0, dist1 (no or one distance code in use: the tree gets forced nodes);
      lit_over, dist_over, bl_over (the plain Huffman tree of the histogram is deeper than 15 / 15 / 7),
      *_over_twice (more than two of its nodes are: the repair's first loop turns more than once),
      *_repaired (the code in the stream spends more bits than a Huffman code: it was cut to the limit);
      hclen4, hclen19, hlit257, hlit286, hdist30, ("hclen", n);
      (16, n), (17, n), (18, n): a repeat symbol of the header with its count;
      ("zeros", n), ("split", n), ("same", n): see below"""
    f = set()
    f.add(("stored", "static", "dynamic")[b.type])
    if b.bits <= 32:
        f.add("tiny_block")
    if b.type == 0:
        return f
    big = [(p, n) for p, n in zip(b.sym_pos, b.sym_bits) if n >= 34]
    if big:
        f.add("sym>=34")
    if any(n >= 44 for _, n in big):
        f.add("sym>=44")
    if any((p & 31) + n > 64 for p, n in big):
        f.add("spill3")
    used_d = sum(1 for x in b.dist_hist if x)
    if used_d == 0:
        f.add("dist0")
    if used_d == 1:
        f.add("dist1")
    if huffman_depth(b.lit_hist)[0] > 15:
        f.add("lit_over")
    if huffman_depth(b.dist_hist)[0] > 15:
        f.add("dist_over")
    if b.type != 2:
        return f
    for name, hist, lens in (("lit_repaired", b.lit_hist, b.lit_lens), ("dist_repaired", b.dist_hist, b.dist_lens),
                             ("bl_repaired", b.bl_hist, b.bl_lens)):
        if repaired(hist, lens):
            f.add(name)
    if huffman_depth(b.bl_hist)[0] > 7:
        f.add("bl_over")
        if nodes_over(b.bl_hist, 7) > 2:
            f.add("bl_over_twice")
    if nodes_over(b.lit_hist, 15) > 2:
        f.add("lit_over_twice")
    for name, ok in (("hclen4", b.hclen == 4), ("hclen19", b.hclen == 19), ("hlit257", b.hlit == 257),
                     ("hlit286", b.hlit == 286), ("hdist30", b.hdist == 30)):
        if ok:
            f.add(name)
    f.add(("hclen", b.hclen))
    f |= {p for p in b.header_syms if p[0] >= 16}
    # ("zeros", n): a run of n unused codes; ("split", n): it took more than one header symbol
    for lens, syms in ((b.lit_lens, _header_part(b, 0)), (b.dist_lens, _header_part(b, 1))):
        at = 0
        for s, n in syms:
            if lens[at] == 0 and (at == 0 or lens[at - 1] != 0):
                run = 0
                while at + run < len(lens) and lens[at + run] == 0:
                    run += 1
                f.add(("zeros", run))
                if run > n:
                    f.add(("split", run))
            at += n
    # runs of one non-zero length
    for lens in (b.lit_lens, b.dist_lens):
        k = 0
        while k < len(lens):
            j = k
            while j < len(lens) and lens[j] == lens[k]:
                j += 1
            if lens[k]:
                f.add(("same", j - k))
            k = j
    return f


def _header_part(b, which):
    """the header's symbols that describe the literal/length tree (0) or the distance tree (1)"""
    at, cut = 0, None
    for k, (s, n) in enumerate(b.header_syms):
        if at == b.hlit:
            cut = k
            break
        at += n
    if cut is None:
        cut = len(b.header_syms)
    return b.header_syms[:cut] if which == 0 else b.header_syms[cut:]


def features(blocks):
    f = set()
    for b in blocks:
        f |= classify(b)
    return f


def step_bits(b):
    """the largest number of bits that one 64-symbol step of the bit packer carries in this block"""
    n = b.sym_bits[:-1]  # (END_BLOCK goes out in a step of its own)
    return max((sum(n[i:i + 64]) for i in range(0, len(n), 64)), default=0)


# ---- the cases ----------------------------------------------------------------------------------------------

class Case:
    """an input, the parameters it is compressed with, and the features its stream must show"""

    def __init__(self, name, data, level=6, window_bits=15, mem_level=8, strategy=DEFAULT, require=()):
        self.name, self.data = name, bytes(data)
        self.level, self.window_bits, self.mem_level, self.strategy = level, window_bits, mem_level, strategy
        self.require = frozenset(require)

    @property
    def family(self):
        return self.name[0]

    @property
    def params(self):
        return self.level, self.window_bits, self.mem_level, self.strategy


def fib(k, a=1, b=2):
    out = []
    for _ in range(k):
        out.append(a)
        a, b = b, a + b
    return out


def shuffled(counts, values, seed):
    """counts[i] copies of values[i], in a seeded order"""
    data = []
    for v, n in zip(values, counts):
        data += [v] * n
    B.Lcg(seed).shuffle(data)
    return bytes(data)


def spread(items, key=lambda x: x):
    """the items in an order in which no two neighbours have the same key (the most frequent key may take up
    to half of the places): by falling frequency into the even places, then the odd ones"""
    groups = {}
    for it in items:
        groups.setdefault(key(it), []).append(it)
    flat = [it for g in sorted(groups.values(), key=lambda g: -len(g)) for it in g]
    assert 2 * max(len(g) for g in groups.values()) <= len(flat) + 1
    out = [None] * len(flat)
    out[0::2] = flat[:(len(flat) + 1) // 2]
    out[1::2] = flat[(len(flat) + 1) // 2:]
    assert all(key(a) != key(b) for a, b in zip(out, out[1:]))
    return out


def skewed(n, seed):
    """bytes that a dynamic block codes well: the smaller of two draws below 64, so no two lengths tie often"""
    r = B.Lcg(seed)
    return bytes(32 + min(r.below(64), r.below(64)) for _ in range(n))


def family_a():
    """A: a literal/length tree whose plain Huffman tree is deeper than 15"""
    f17 = shuffled(fib(17), range(65, 82), 17)
    f18 = shuffled(fib(18), range(65, 83), 18)
    assert (len(f17), len(f18)) == (6763, 10944)
    # every byte value present: 239 values 36 times each under the 17-value Fibonacci tail
    rest = [v for v in range(256) if not 65 <= v < 82]
    full = shuffled(fib(17) + [36] * len(rest), list(range(65, 82)) + rest, 19)
    over = {"lit_over", "lit_repaired", "hclen19", "hlit257", "dist0", "dynamic"}
    return [
        Case("A-fib17", f17, strategy=HUFFMAN_ONLY, require=over | {"lit_over_twice"}),
        Case("A-fib18", f18, strategy=HUFFMAN_ONLY, require=over | {"lit_over_twice"}),
        Case("A-fib17-all256", full, strategy=HUFFMAN_ONLY, require=over),
        Case("A-fib17-default", f17, strategy=DEFAULT, require={"dynamic"}),
        Case("A-fib17-filtered", f17, strategy=FILTERED, require={"dynamic"}),
        Case("A-fib18-mem9", f18, mem_level=9, strategy=HUFFMAN_ONLY, require=over),
        Case("A-fib17-raw", f17, window_bits=-15, strategy=HUFFMAN_ONLY, require=over),
        Case("A-fib17-gzip", f17, window_bits=31, strategy=HUFFMAN_ONLY, require=over),
    ]


def rle_input(symbols, seed=0):
    """Z_RLE parses a run of R equal bytes behind another value as one literal and, for 4 <= R <= 259, one
    match of length R - 1 at distance 1.  `symbols` lists (byte value, run length); the runs are put in an
    order in which no two neighbours share a value, so that every run stands as written."""
    out = bytearray()
    for v, n in spread(symbols, key=lambda s: s[0]):
        out += bytes([v]) * n
    return bytes(out)


def family_b():
    """B: deep length codes through Z_RLE.  The rarest literal/length symbols are the length codes 281-285
    (matches of 131 to 258 bytes, five extra bits but for 285); above them literals in Fibonacci counts."""
    def build(k):
        counts = fib(k)
        runs = []
        # one match per run; run lengths are match length + 1
        for code_len, n in zip((140, 170, 200, 240, 258), counts[:5]):
            runs += [(88, code_len + 1)] * n
        nruns = len(runs)
        items = runs
        for i, n in enumerate(counts[5:]):
            v = 97 + i
            if i == 1:
                # the value that starts the runs: their literals count for it
                v, n = 88, n - nruns
            items = items + [(v, 1)] * n
        return rle_input(items)
    need = {"dist1", "hlit286", "dynamic"}
    return [
        Case("B-rle-fib17", build(17), strategy=RLE, require=need | {"lit_over", "lit_repaired", "hclen19"}),
        Case("B-rle-fib18-raw", build(18), window_bits=-15, strategy=RLE, require=need | {"lit_over", "lit_repaired", "hclen19"}),
        Case("B-rle-fib12", build(12), strategy=RLE, require=need),
    ]


def profile_input(seed, depth=13):
    """a Z_HUFFMAN_ONLY input with a seeded frequency profile: a random binary tree of at most `depth` levels
    is grown leaf by leaf (mostly at its deepest leaf, which makes many code lengths with few symbols each),
    its leaves are dealt to byte values in a seeded order, and a leaf at level d gets 2^(depth-d) bytes"""
    r = B.Lcg(seed)
    leaves = [1, 1]
    want = r.between(12, 200)
    while len(leaves) < want:
        deep = max(leaves)
        if r.chance(60) and deep < depth:
            k = leaves.index(deep)
        else:
            k = r.below(len(leaves))
            if leaves[k] >= depth:
                continue
        leaves[k] += 1
        leaves.append(leaves[k])
    r.shuffle(leaves)
    values = list(range(256))
    if r.chance(50):
        r.shuffle(values)
        values = sorted(values[:len(leaves)]) if r.chance(50) else values[:len(leaves)]
    else:
        at = r.below(256 - len(leaves) + 1)
        values = values[at:at + len(leaves)]
    return shuffled([1 << (depth - d) for d in leaves], values, seed)


# 3 000 seeds of profile_input (0..2999) were searched on the CPU with the oracle and the walker: 201 of them
# give a block whose bit-length tree (the code of the header's code lengths, at most 7 bits) needs the
# overflow repair, 27 of those with more than two nodes too deep, so that the repair's first loop turns twice.
BL_OVER_SEEDS = (1, 2, 52)
BL_OVER_TWICE_SEEDS = (150, 287)


def family_c():
    """C: a bit-length tree whose plain Huffman tree is deeper than 7"""
    need = {"bl_over", "bl_repaired", "dynamic", "dist0"}
    return [Case("C-profile-%d" % s, profile_input(s), strategy=HUFFMAN_ONLY, require=need) for s in BL_OVER_SEEDS] + \
           [Case("C-profile-%d-twice" % s, profile_input(s), strategy=HUFFMAN_ONLY, require=need | {"bl_over_twice"})
            for s in BL_OVER_TWICE_SEEDS]


def lengths_input(lens_of, depth, seed):
    """a Z_HUFFMAN_ONLY input whose byte value v gets a code of lens_of[v] bits: 2^(depth - length) bytes of
    it, shuffled.  With END_BLOCK (once per block: `depth` bits) the lengths must fill the code space."""
    assert sum(1 << (depth - l) for l in lens_of.values()) + 1 == 1 << depth
    values = sorted(lens_of)
    return shuffled([1 << (depth - lens_of[v]) for v in values], values, seed)


def header_edges_input(gaps, groups, depth=12, seed=5):
    """byte values in rising order: single values with `gaps` unused values after each, then `groups`
    (code length, how many neighbouring values get it), then single values of distinct lengths that fill what
    is left of the code space"""
    used = sum(1 << (depth - l) for l, n in groups for _ in range(n)) + 1
    rest = (1 << depth) - used
    assert rest > 0
    fill = [depth - k for k in range(depth) if rest >> k & 1]   # distinct lengths, longest first
    assert len(fill) >= len(gaps), (fill, gaps)
    lens_of, v = {}, 0
    for g in gaps:
        lens_of[v] = fill.pop()
        v += 1 + g
    for l, n in groups:
        for _ in range(n):
            lens_of[v] = l
            v += 1
    for l in fill:
        lens_of[v] = l
        v += 1
    assert v <= 256
    return lengths_input(lens_of, depth, seed)


def family_d():
    """D: the repeat thresholds of the dynamic header (3/4, 6/7, 10/11, 138/139), written once in the scan that
    counts the header's symbols and once in the loop that sends them"""
    # equal lengths 3, 4, 6, 7, 8 and 9 times in a row, told apart by a neighbour of another length
    groups = [(7, 3), (8, 4), (7, 6), (8, 7), (7, 8), (8, 9), (9, 1)]
    same = {("same", n) for n in (3, 4, 6, 7, 8, 9)}
    edges = header_edges_input([2, 3, 10, 11, 138], groups)
    e139 = header_edges_input([139, 2], groups, seed=6)
    e140 = header_edges_input([140, 3], groups, seed=7)
    # the Fibonacci counts of family A around a gap of 139: code lengths up to 15, all 19 bit-length codes sent
    deep = shuffled(fib(17), list(range(8)) + list(range(147, 156)), 8)
    # HCLEN.  Four bit-length codes (16, 17, 18, 0) cannot come out of any compressor: END_BLOCK alone has a
    # code of non-zero length, which takes one of the codes 1-15.  Nor can fewer than 12: the distance tree is
    # complete, with at most 30 codes, so some distance code is at most 4 bits long, and of the lengths 1-4 the
    # header's order (16 17 18 0 8 7 9 6 10 5 11 4 ...) lists 4 first, in twelfth place.  Exactly 12 takes 16
    # equally frequent distance codes and literal/length codes of 5 to 11 bits: copies of 4 to 11 bytes from
    # the distance codes 6-21, 16 of each, behind 2 048 bytes without a match.
    r = B.Lcg(3)
    plan = [(code, 4 + r.below(8), True) for code in range(6, 22) for _ in range(16)]
    r.shuffle(plan)
    low = copies_input(31, plan, prefix=2048)
    return [
        Case("D-zero-runs", edges, strategy=HUFFMAN_ONLY,
             require=same | {("zeros", 2), ("zeros", 3), ("zeros", 10), ("zeros", 11), ("zeros", 138), (17, 3), (17, 10),
                             (18, 11), (18, 138), (16, 3), (16, 6), "dynamic"}),
        Case("D-zero-139", e139, strategy=HUFFMAN_ONLY,
             require=same | {("zeros", 139), ("split", 139), (18, 138), (16, 3), (16, 6), "dynamic"}),
        Case("D-zero-140", e140, strategy=HUFFMAN_ONLY,
             require=same | {("zeros", 140), ("split", 140), (18, 138), (17, 3), "dynamic"}),
        Case("D-zero-139-hclen19", deep, strategy=HUFFMAN_ONLY,
             require={("zeros", 139), ("split", 139), (18, 138), "hclen19", "lit_over", "dynamic"}),
        Case("D-hclen12", low, level=6, require={("hclen", 12), "dynamic"}),
    ]


def family_e():
    """E: inputs that end exactly where a block fills up (2^(mem_level+6) - 1 symbols), one byte before and
    one after.  Ending on the cut leaves an empty last block: 10 bits of a static block."""
    cases = []
    for ml, sizes, tiny in ((8, (16382, 16383, 16384, 32766, 32767), (16383, 32766)),
                            (1, (126, 127, 128, 254, 255), (127, 254)),
                            (9, (32767, 32768), (32767,))):
        for n in sizes:
            data = skewed(n, n)
            cases.append(Case("E-huff-mem%d-%d" % (ml, n), data, mem_level=ml, strategy=HUFFMAN_ONLY,
                              require={"tiny_block", "static"} if n in tiny else ()))
            cases.append(Case("E-fixed-mem%d-%d" % (ml, n), data, mem_level=ml, strategy=FIXED, require={"static"}))
    return cases


F_KINDS = ("random", "two", "text", "one")
F_PARAMS = ((1, DEFAULT), (6, DEFAULT), (1, FIXED), (6, FIXED))


def family_f():
    """F: every length 0..300 of four kinds of data, where the sizes of the stored, the static and the dynamic
    form of a block lie within a byte of each other"""
    from zsc_amd import corpus
    text = corpus.make_buffer("text", 300, 7)
    rnd = B.Lcg(11).bytes(300)
    two = bytes(b"ab"[B.Lcg(12 + n).below(2)] for n in range(300))
    src = {"random": rnd, "two": two, "text": text, "one": b"z" * 300}
    return [Case("F-%s-%d-l%ds%d" % (kind, n, level, strat), src[kind][:n], level=level, strategy=strat)
            for level, strat in F_PARAMS for kind in F_KINDS for n in range(301)]


def distinct_trigram_bytes(r, n):
    """n seeded bytes among which no three in a row occur twice: a parser finds no match in them"""
    out, seen = bytearray(), set()
    while len(out) < n:
        b = r.below(256)
        if len(out) >= 2:
            t = (out[-2], out[-1], b)
            if t in seen:
                continue
            seen.add(t)
        out.append(b)
    return out


def copies_input(seed, plan, prefix=32766):
    """`prefix` bytes without a match (two full blocks of literals at mem_level 8), then for every (distance
    code, length, literal behind it?) of `plan` a copy of `length` bytes from a seeded distance in that code's
    range and, if asked for, one more byte.  Sources and bytes are drawn again until the parse is forced:
    the three bytes a copy begins with occur nowhere nearer than its source, the byte behind a copy ends the
    match, and the three bytes that begin at a literal occur nowhere before.  The longest-match search then
    finds each copy where it was taken from (a farther, longer candidate takes a 1-in-256 coincidence)."""
    r = B.Lcg(seed)
    out = distinct_trigram_bytes(r, prefix)
    last = {}

    def note(upto):
        for q in range(max(note.done, 0), upto - 2):
            last[(out[q], out[q + 1], out[q + 2])] = q
        note.done = max(note.done, upto - 2)
    note.done = 0
    note(len(out))
    pending_stop = None   # the byte that would lengthen the copy before, where no literal follows it
    def literal(stop):
        while True:
            b = r.below(256)
            if b != stop and (out[-2], out[-1], b) not in last:
                out.append(b)
                note(len(out))
                return

    def source(code, length):
        lo = DIST_BASE[code]
        p = len(out)
        hi = min(lo + (1 << DIST_EXTRA[code]) - 1, 32000, p)
        assert lo <= hi
        for attempt in range(200):
            dist = r.between(lo, hi + 1)
            at = p - dist
            c = bytearray()
            for k in range(length + 1):
                c.append(out[at + k] if at + k < p else c[at + k - p])
            stop, c = c[length], c[:length]
            if pending_stop is not None and c[0] == pending_stop:
                continue
            # the nearest earlier place where the copy's first three bytes stand is its source
            t = (c[0], c[1], c[2])
            near = last.get(t, -1)
            for q in (p - 2, p - 1):
                if tuple((list(out[q:p]) + list(c))[:3]) == t:
                    near = q
            if near != at:
                continue
            # no match begins at the literal in front of the copy
            if pending_stop is None and (out[p - 1], c[0], c[1]) in last:
                continue
            return c, stop
        return None

    for code, length, sep in plan:
        for _ in range(64):
            found = source(code, length)
            if found:
                break
            # the few distances of a small code all point at unsuitable places: one more literal moves them
            literal(pending_stop)
            pending_stop = None
        c, stop = found
        out += c
        pending_stop = stop
        note(len(out))
        if sep:
            literal(stop)
            pending_stop = None
    return bytes(out)


def long_symbol_plan(seed, chain=14, flat=True):
    """The rarest distance codes are the ones with 13 and 12 extra bits, in Fibonacci counts 1, 2, 3, 5, ...
    from code 29 down to code 16; codes 0-15 share the rest (distance 1 less than the
    others: each of its copies needs a byte value of its own in front).  The matches of the five rarest codes
    are 67 to 257 bytes long, in length codes that occur once or twice in the block (4 or 5 extra bits), and
    stand at the head of the block without a literal between them: one step of the bit packer takes them all."""
    r = B.Lcg(seed)
    counts = {29 - k: n for k, n in enumerate(fib(chain))}
    rare, rest = [], []
    long_lengths = [230, 200, 170, 140, 240, 205, 175, 145, 120, 100, 90, 70, 125, 105, 95, 75, 115, 99, 83]
    for code in range(29, 29 - chain, -1):
        for _ in range(counts[code]):
            if code >= 25:
                rare.append((code, long_lengths[len(rare)], False))
            else:
                rest.append((code, 4 + r.below(2), True))
    for code in range(16 if flat else 0):
        rest += [(code, 4 + r.below(2), True) for _ in range(200 if code == 0 else 328)]
    r.shuffle(rest)
    return rare + rest


def family_g():
    """G: symbols of 44 bits and more (a 15-bit length code is not needed for that: 13 or 14 bits, 5 extra,
    a 13-bit distance code and 13 extra bits), which spill into a third 32-bit word of the staging area"""
    data = copies_input(23, long_symbol_plan(23))
    return [Case("G-long-symbols", data, level=6, require={"sym>=34", "sym>=44", "spill3", "hdist30", "dynamic"})]


def family_h():
    """H: a distance tree whose plain Huffman tree is deeper than 15: the Fibonacci counts 1, 2, 3, ..., 2584
    on the distance codes 29 down to 13 and no other distance in the block"""
    data = copies_input(29, long_symbol_plan(29, chain=17, flat=False))
    return [Case("H-dist-fib17", data, level=6,
                 require={"dist_over", "dist_repaired", "sym>=44", "spill3", "hdist30", "dynamic"})]


FAMILIES = (family_a, family_b, family_c, family_d, family_e, family_f, family_g, family_h)
_CASES = []


def cases():
    """every case, built once"""
    if not _CASES:
        for fam in FAMILIES:
            _CASES.extend(fam())
        assert len({c.name for c in _CASES}) == len(_CASES)
    return _CASES


def f_groups(all_cases):
    """family F's cases by (kind, level, strategy), lengths rising: the golden file keeps one record per group"""
    groups = {}
    for c in all_cases:
        if c.family == "F":
            kind, n, tail = c.name.split("-")[1:]
            groups.setdefault("F-%s-%s" % (kind, tail), []).append(c)
    for g in groups.values():
        assert [len(c.data) for c in g] == list(range(301))
    return groups


def group_digest(outs):
    """one SHA-256 over the SHA-256s of a group's streams"""
    h = hashlib.sha256()
    for o in outs:
        h.update(hashlib.sha256(o).digest())
    return h.hexdigest()


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def check_against_golden(golden, all_cases, results, what):
    """results: {case name: (rc, stream)}; every case has a record, every record a case"""
    groups = f_groups(all_cases)
    single = [c for c in all_cases if c.family != "F"]
    assert set(golden["cases"]) == {c.name for c in single} and set(golden["groups"]) == set(groups)
    for c in single:
        rc, out = results[c.name]
        assert [rc, len(out), sha(out)] == golden["cases"][c.name], (what, c.name, rc, len(out))
    for name, g in groups.items():
        rec = golden["groups"][name]
        got = [results[c.name] for c in g]
        assert [r[0] for r in got] == rec["rc"], (what, name)
        assert [len(r[1]) for r in got] == rec["out_len"], (what, name)
        assert group_digest([r[1] for r in got]) == rec["sha256"], (what, name)
