"""DEFLATE streams built bit by bit, for what no encoder writes (RFC 1951 at its limits).

A plain helper module: tests/test_handbuilt_streams_emu.py, tests/test_gpu_handbuilt_streams.py and
tests/golden/make_handbuilt_golden.py import it.  Nothing here calls a decoder.

  Stream            a bit writer with stored(), fixed() and dynamic() blocks at any bit phase
  canonical()       the canonical Huffman codes of a list of code lengths
  complete_lengths  a complete set of code lengths for n symbols, shallow or with 15-bit codes
  play()            what a list of tokens inflates to, in plain Python: the reference of the operation
  wrap()            raw / zlib / gzip framing, check values in plain Python
  cases()           the named hand-built cases [(name, stream, dest_cap, window_bits, expected or None)]
  records()         every (case, truncation, cap) the golden file holds, with the recorded result

A token is a literal byte (int), a match (length, distance), or Raw(value, nbits, huffman): bits that are
no token (a code the format reserves, the unused bit of a one-code distance code).  Every seeded choice
comes from Lcg below, so the streams do not depend on the Python version; the golden file pins each
stream's SHA-256.
"""
import functools
import hashlib
import json
import os
import struct
from collections import namedtuple

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "handbuilt_golden.json")

STAGE = 512        # INF_STAGE of the product build (zsc_amd/csrc/inflate.h): the decoder's output ring
STAGE_BIG = 1024   # and of the group16-stage1024 emulation
SHORT = 2000       # a case whose stream is shorter is recorded at every truncation

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [x for e in range(1, 14) for x in (e, e)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
CL_PLAIN = [4] * 16 + [0, 0, 0]    # a complete code-length code over the plain lengths 0..15
CL_REPEATS = [5] * 16 + [2, 3, 3]  # a complete one with 16, 17 and 18

Raw = namedtuple("Raw", "value nbits huffman")  # huffman: written MSB first, as a code; else LSB first


class Lcg:
    """Knuth's MMIX generator; the high bits are handed out"""

    def __init__(self, seed):
        self.x = (seed * 0x9E3779B97F4A7C15 + 0x1234567) & 0xFFFFFFFFFFFFFFFF
        for _ in range(4):
            self.next()

    def next(self):
        self.x = (self.x * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        return self.x >> 33

    def below(self, n):
        return self.next() % n

    def between(self, lo, hi):
        """lo <= value < hi"""
        return lo + self.next() % (hi - lo)

    def chance(self, percent):
        return self.next() % 100 < percent

    def choice(self, seq):
        return seq[self.next() % len(seq)]

    def shuffle(self, seq):
        for i in range(len(seq) - 1, 0, -1):
            j = self.next() % (i + 1)
            seq[i], seq[j] = seq[j], seq[i]

    def bytes(self, n):
        return bytes(self.next() & 255 for _ in range(n))


def canonical(lens):
    """{symbol: (code, length)} of RFC 1951 3.2.2 for these code lengths (0: no code)"""
    count = [0] * 17
    for n in lens:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for n in range(1, 17):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    codes = {}
    for sym, n in enumerate(lens):
        if n:
            codes[sym] = (nxt[n], n)
            nxt[n] += 1
    return codes


def kraft(lens):
    """the sum of 2^-length in units of 2^-15: 32768 for a complete set"""
    return sum(1 << (15 - n) for n in lens if n)


def complete_lengths(n, first=(), deep=False, keep=0):
    """A complete set of code lengths for n symbols, 1 <= n <= 288 (n == 1: one code of 1 bit, as complete as
    one code gets).  The symbols of `first`, in that order, and then the others in rising order get the
    lengths from the shortest up.  deep: the longest codes have 15 bits -- the chain 1, 2, ..., 14, 15, 15
    (for n < 16 the chain of n leaves), and the shallowest leaf deeper than `keep` split until there are n,
    so lengths 1..keep stay in the set."""
    assert 1 <= n <= 288
    if n == 1:
        leaves = [1]
    else:
        k = min(n, 16) if deep else 2
        count = [0] * 16
        for x in list(range(1, k)) + [k - 1]:
            count[x] += 1
        for _ in range(n - k):
            x = next(d for d in range(keep + 1, 15) if count[d])
            count[x] -= 1
            count[x + 1] += 2
        leaves = [d for d in range(1, 16) for _ in range(count[d])]
        assert len(leaves) == n and kraft(leaves) == 32768
    leaves.sort()
    lens = [0] * n
    first = list(first)
    seen = set(first)
    for sym, x in zip(first + [i for i in range(n) if i not in seen], leaves):
        lens[sym] = x
    return lens


def length_symbol(n):
    """(symbol, extra value, extra bits)"""
    if n == 258:
        return 285, 0, 0
    for i in range(27, -1, -1):
        if n >= LEN_BASE[i]:
            return 257 + i, n - LEN_BASE[i], LEN_EXTRA[i]
    raise ValueError(n)


def distance_symbol(d):
    for i in range(29, -1, -1):
        if d >= DIST_BASE[i]:
            return i, d - DIST_BASE[i], DIST_EXTRA[i]
    raise ValueError(d)


def literal_length_symbols(tokens):
    return {t if isinstance(t, int) else length_symbol(t[0])[0] for t in tokens if not isinstance(t, Raw)} | {256}


def distance_symbols(tokens):
    return {distance_symbol(t[1])[0] for t in tokens if isinstance(t, tuple) and not isinstance(t, Raw)}


class Stream:
    """LSB-first bit fields, Huffman codes MSB first, and the three block types on top"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value, nbits):
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        if self.n >= 8:
            k = self.n >> 3
            self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def code(self, code, nbits):
        self.bits(int(format(code, "0%db" % nbits)[::-1], 2), nbits)

    def raw(self, r):
        (self.code if r.huffman else self.bits)(r.value, r.nbits)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def phase(self):
        return self.n

    def bytes(self):
        """the stream so far, padded with zero bits to a whole byte"""
        s = Stream()
        s.acc, s.n, s.out = self.acc, self.n, bytearray(self.out)
        s.align()
        return bytes(s.out)

    def tokens(self, lit_codes, dist_codes, tokens):
        for t in tokens:
            if isinstance(t, Raw):
                self.raw(t)
            elif isinstance(t, int):
                self.code(*lit_codes[t])
            else:
                sym, extra, xb = length_symbol(t[0])
                self.code(*lit_codes[sym])
                self.bits(extra, xb)
                sym, extra, xb = distance_symbol(t[1])
                self.code(*dist_codes[sym])
                self.bits(extra, xb)

    def stored(self, data, last, nlen=None):
        """at any bit phase; nlen: what to write for NLEN instead of the complement"""
        self.bits(last, 1)
        self.bits(0, 2)
        self.align()
        self.bits(len(data), 16)
        self.bits(len(data) ^ 0xFFFF if nlen is None else nlen, 16)
        self.out += data

    def fixed(self, tokens, last, eob=True):
        self.bits(last, 1)
        self.bits(1, 2)
        lit = canonical(FIXED_LIT)
        self.tokens(lit, canonical(FIXED_DIST), tokens)
        if eob:
            self.code(*lit[256])

    def dynamic(self, lit_lens, dist_lens, tokens, last, cl_lens=None, hclen=19, header_syms=None, eob=True):
        """header_syms: the (symbol, extra) pairs of the code-length sequence, written as they are; without
        it every length is written as its own symbol"""
        cl_lens = CL_PLAIN if cl_lens is None else cl_lens
        self.bits(last, 1)
        self.bits(2, 2)
        self.bits(len(lit_lens) - 257, 5)
        self.bits(len(dist_lens) - 1, 5)
        self.bits(hclen - 4, 4)
        for sym in CL_ORDER[:hclen]:
            self.bits(cl_lens[sym], 3)
        cl = canonical(cl_lens)
        if header_syms is None:
            header_syms = [(n, 0) for n in list(lit_lens) + list(dist_lens)]
        for sym, extra in header_syms:
            self.code(*cl[sym])
            self.bits(extra, {16: 2, 17: 3, 18: 7}.get(sym, 0))
        lit = canonical(lit_lens)
        self.tokens(lit, canonical(dist_lens), tokens)
        if eob:
            self.code(*lit[256])


def play(tokens, history=b""):
    """what the tokens inflate to behind `history`, in plain Python"""
    out = bytearray(history)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            n, d = t
            assert 3 <= n <= 258 and 1 <= d <= len(out) and d <= 32768, t
            if d >= n:
                out += out[len(out) - d:len(out) - d + n]
            else:
                seg = bytes(out[len(out) - d:])
                out += (seg * (n // d + 1))[:n]
    return bytes(out[len(history):])


def play_slow(tokens):
    """play() byte by byte, and for every output offset the index of the token that made it"""
    out, owner = bytearray(), []
    for k, t in enumerate(tokens):
        if isinstance(t, int):
            out.append(t)
            owner.append(k)
        else:
            for _ in range(t[0]):
                out.append(out[-t[1]])
                owner.append(k)
    return bytes(out), owner


def adler32(data):
    a, b = 1, 0
    for at in range(0, len(data), 5552):
        for x in data[at:at + 5552]:
            a += x
            b += a
        a %= 65521
        b %= 65521
    return (b << 16) | a


@functools.lru_cache(maxsize=None)
def _crc_table():
    table = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ (0xEDB88320 if c & 1 else 0)
        table.append(c)
    return table


def crc32(data):
    table, c = _crc_table(), 0xFFFFFFFF
    for x in data:
        c = table[(c ^ x) & 255] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def wrap(raw, out, window_bits):
    """raw deflate data framed for window_bits: < 0 raw, 8..15 zlib (78 9c, Adler-32), > 15 gzip (a 10-byte
    header, CRC-32, ISIZE)"""
    if window_bits < 0:
        return raw
    if window_bits > 15:
        return b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + raw + struct.pack("<II", crc32(out), len(out) & 0xFFFFFFFF)
    return b"\x78\x9c" + raw + struct.pack(">I", adler32(out))


def check_value(out, window_bits):
    """the value a check plan hands out for this output: CRC-32 for gzip, Adler-32 for zlib and raw"""
    return crc32(out) if window_bits > 15 else adler32(out)


# ---- the cases ----

TAIL = b"\x00" * 8  # behind every erroneous stream, so that running out of input is not what ends it


def _deep_tokens(rnd):
    """the main block of `deep`: a few thousand literals; for every d in 1..770 a fresh literal, (258, d) and a
    seeded length at d; distance 32768 on the first byte that allows it; every far distance code; 13 extra bits
    all zero and all one behind lengths with 5 extra bits"""
    tokens = [rnd.below(256) for _ in range(3000)]
    pos = len(tokens)
    far_done = False
    for d in range(1, 771):
        step = [rnd.below(256), (258, d), (rnd.between(3, 259), d)]
        need = 1 + 258 + step[2][0]
        if not far_done and pos + need > 32768:
            # distance 32768 on the first byte that allows it
            tokens += [rnd.below(256) for _ in range(32768 - pos)]
            tokens += [(258, 32768), (3, 32768)]
            pos = 32768 + 261
            far_done = True
        tokens += step
        pos += need
    assert far_done
    # every distance code from 1025 up, at its nearest and at a seeded distance
    for dsym in range(20, 30):
        tokens += [rnd.below(256), (rnd.between(3, 259), DIST_BASE[dsym]),
                   (rnd.between(3, 259), DIST_BASE[dsym] + rnd.below(1 << DIST_EXTRA[dsym]))]
    # 13 extra bits all zero, 13 extra bits all one; a length with 5 extra bits before each
    tokens += [(258, 24577), (258, 32768), (257, 32768), (131, 24577), (257, 32767), (163, 32768)]
    return tokens


def _deep_case():
    rnd = Lcg(101)
    s = Stream()
    out = bytearray()
    # block 0: 286 literal/length symbols and 30 distance symbols, both deep; length symbols 284 and 285
    # and distance symbols 28 and 29 last in the order, so they get 15-bit codes
    order = [256] + list(range(256)) + list(range(257, 286))
    lit = complete_lengths(286, order, deep=True)
    dist = complete_lengths(30, list(range(30)), deep=True)
    assert lit[284] == lit[285] == 15 and dist[28] == dist[29] == 15
    tokens = _deep_tokens(rnd)
    s.dynamic(lit, dist, tokens, 0)
    out += play(tokens)
    all_tokens = list(tokens)
    def decoded(lens, syms):
        return {lens[x] for x in syms}

    lit_seen = decoded(lit, literal_length_symbols(tokens))
    dist_seen = decoded(dist, distance_symbols(tokens))
    # further blocks: literal/length codes that keep lengths 1..keep, and the distance code 1..14, 15, 15 over 16
    # symbols; the tokens use the shortest and the longest codes of both
    for keep in (1, 2, 3, 4, 5, 6):
        short = list(dict.fromkeys(rnd.below(256) for _ in range(7)))
        lit = complete_lengths(286, [256] + short, deep=True, keep=keep)
        dist_order = list(range(16))
        rnd.shuffle(dist_order)
        dist = complete_lengths(16, dist_order, deep=True)
        assert sorted(dist) == list(range(1, 15)) + [15, 15] and lit[285] == 15
        tokens = []
        for i in range(400):
            tokens.append(rnd.choice(short) if rnd.chance(60) else rnd.below(256))
            if i % 5 == 4:
                dsym = dist_order[i // 5 % 16]
                d = DIST_BASE[dsym] + rnd.below(1 << DIST_EXTRA[dsym])
                tokens.append((rnd.choice([258, 257, 3, rnd.between(3, 259)]), d))
        s.dynamic(lit, dist, tokens, 0)
        out += play(tokens, bytes(out[-32768:]))
        all_tokens += tokens
        lit_seen |= decoded(lit, literal_length_symbols(tokens))
        dist_seen |= decoded(dist, distance_symbols(tokens))
    # a literal/length code with 7-bit codes next to 1..6 has room for 257 symbols only: literals, no distance code
    short = [10, 20, 30, 40, 50, 60, 70]
    lit = complete_lengths(257, [256] + short, deep=True, keep=7)
    assert [lit[x] for x in short[:6]] == [2, 3, 4, 5, 6, 7]
    tokens = [rnd.choice(short + [rnd.below(256)]) for _ in range(300)]
    s.dynamic(lit, [0], tokens, 0)
    out += bytes(tokens)
    all_tokens += tokens
    lit_seen |= decoded(lit, literal_length_symbols(tokens))
    assert lit_seen >= set(range(1, 16)) and dist_seen >= set(range(1, 16)), (lit_seen, dist_seen)
    s.fixed([], 1)
    return s.bytes(), bytes(out), all_tokens


def _ring_edge_case():
    """literals, then matches whose source lies around pos - STAGE and pos - STAGE_BIG: first source byte
    STAGE - 1, STAGE and STAGE + 1 behind the copy's end, and sources that straddle pos - STAGE"""
    rnd = Lcg(202)
    tokens = [rnd.below(256) for _ in range(2100)]
    for stage in (STAGE, STAGE_BIG):
        for n in (3, 16, 17, 257, 258):
            dists = [stage - n + e for e in (-1, 0, 1)]             # the source starts stage + e behind the copy's end
            dists += [stage - 1, stage, stage + 1, stage + n // 2, stage + n - 1, stage + n]  # it straddles pos - stage
            for d in dists:
                tokens += [rnd.below(256) for _ in range(rnd.between(1, 4))]
                tokens.append((n, d))
    used = sorted(literal_length_symbols(tokens))
    dused = sorted(distance_symbols(tokens))
    s = Stream()
    s.dynamic(complete_lengths(286, used, deep=True), complete_lengths(30, dused, deep=True), tokens, 1)
    return s.bytes(), play(tokens), tokens


def _header_syms_plain(lens):
    return [(n, 0) for n in lens]


def _oddities():
    """legal headers nobody writes: [(name, stream, cap, expected)]"""
    cases = []
    lit258 = complete_lengths(258, [256, 65, 66, 67, 257], deep=True)
    # a lone 1-bit distance code, a match through it
    tokens = [65, 66, 67, (3, 1), 66, (3, 1)]
    s = Stream()
    s.dynamic(lit258, [1], tokens, 1)
    cases.append(("one-dist-code", s.bytes(), 100, play(tokens)))
    # an empty distance code, literals only
    tokens = [65, 66, 67, 65]
    s = Stream()
    s.dynamic(lit258, [0], tokens, 1)
    cases.append(("empty-dist-code-literals", s.bytes(), 100, play(tokens)))
    # HLIT 257, HDIST 1, and the fewest code-length codes that can describe a block at all: HCLEN 5 reaches
    # 16, 17, 18, 0 and 8 -- 256 codes of 8 bits (HCLEN 4 reaches no length but 0: among the errors)
    lens = [8] * 255 + [0, 8]
    cl = [0] * 19
    cl[0], cl[8] = 1, 1
    tokens = [0, 1, 254, 128, 7]
    s = Stream()
    s.dynamic(lens, [0], tokens, 1, cl_lens=cl, hclen=5)
    cases.append(("hclen5-hlit257-hdist1", s.bytes(), 100, play(tokens)))
    # the same lengths through 16 (repeat 8) with HCLEN 5: 8, then 16s
    cl = [0] * 19
    cl[16], cl[0], cl[8] = 1, 2, 2
    syms = [(8, 0)] + [(16, 3)] * 42 + [(8, 0), (8, 0), (0, 0), (8, 0), (0, 0)]
    # (1 + 42 * 6 + 2 = 255 lengths of 8, then 0 for literal 255, 8 for the end-of-block code, 0 for the distance)
    s = Stream()
    s.dynamic(lens, [0], tokens, 1, cl_lens=cl, hclen=5, header_syms=syms)
    cases.append(("hclen5-repeat16", s.bytes(), 100, play(tokens)))
    # 16 crossing from the literal lengths into the distance lengths: the 2 bits of symbol 285, the last
    # literal/length length, four times more -- a complete distance code
    lit = complete_lengths(286, [10, 285, 256, 20], deep=True, keep=2)
    assert lit[285] == 2
    tokens = [10, 20, 10, (258, 2), (258, 3), 20, (258, 4), (258, 1)]
    s = Stream()
    s.dynamic(lit, [2, 2, 2, 2], tokens, 1, cl_lens=CL_REPEATS, header_syms=_header_syms_plain(lit) + [(16, 1)])
    cases.append(("repeat16-into-dist", s.bytes(), 1100, play(tokens)))
    # 17 and 18 (runs of zeros) crossing: the unused tail of the literal lengths and the head of the distances
    for name, nlit, zeros_in_dist, sym in (("repeat17-into-dist", 262, 5, 17), ("repeat18-into-dist", 272, 6, 18)):
        lit = complete_lengths(259, [256, 10, 20], deep=True) + [0] * (nlit - 259)
        dist = [0] * zeros_in_dist + complete_lengths(5, [0, 4], deep=True)
        run = nlit - 259 + zeros_in_dist
        extra = run - (3 if sym == 17 else 11)
        assert 0 <= extra < (8 if sym == 17 else 128)
        tokens = [10, 20, 30, 40, 50, 60, 70, 80, 90, 100, 110, 120, 130] * 3
        tokens += [(3, DIST_BASE[zeros_in_dist]), (4, DIST_BASE[zeros_in_dist + 4]), 5]
        syms = _header_syms_plain(lit[:259]) + [(sym, extra)] + _header_syms_plain(dist[zeros_in_dist:])
        s = Stream()
        s.dynamic(lit, dist, tokens, 1, cl_lens=CL_REPEATS, header_syms=syms)
        cases.append((name, s.bytes(), 100, play(tokens)))
    # a literal/length code that is the end-of-block code alone, 1 bit
    s = Stream()
    s.dynamic([0] * 256 + [1], [0], [], 1, cl_lens=CL_REPEATS,
              header_syms=[(18, 127), (18, 256 - 138 - 11), (1, 0), (0, 0)])
    cases.append(("lone-end-of-block-code", s.bytes(), 100, b""))
    return cases


def _header_errors():
    """[(name, stream, cap)]: each one a data error, each followed by TAIL"""
    cases = []
    lit258 = complete_lengths(258, [256, 65, 66, 257], deep=True)
    lit = canonical(lit258)

    def with_match(dist_lens, bit):
        s = Stream()
        s.dynamic(lit258, dist_lens, [65, Raw(lit[257][0], lit[257][1], True), Raw(bit, 1, False), 66], 1)
        return s.bytes() + TAIL

    cases.append(("one-dist-unused-bit", with_match([1], 1), 100))
    cases.append(("empty-dist-match-bit0", with_match([0], 0), 100))
    cases.append(("empty-dist-match-bit1", with_match([0], 1), 100))

    def header(lit_lens, dist_lens, **kw):
        s = Stream()
        s.dynamic(lit_lens, dist_lens, [], 1, eob=False, **kw)
        return s.bytes() + TAIL

    cases.append(("hlit-287", header(FIXED_LIT[:287], [1]), 100))
    cases.append(("hlit-288", header(FIXED_LIT, [1]), 100))
    lit257 = complete_lengths(257, [256], deep=False)
    cases.append(("hdist-31", header(lit257, [5] * 31), 100))
    cases.append(("hdist-32", header(lit257, [5] * 32), 100))
    cases.append(("repeat16-first", header(lit257, [1], cl_lens=CL_REPEATS, header_syms=[(16, 0), (8, 0)]), 100))
    cases.append(("repeat17-past-end", header(lit257, [1], cl_lens=CL_REPEATS,
                                              header_syms=_header_syms_plain(lit257[:256]) + [(17, 0)]), 100))
    cases.append(("repeat18-past-end", header(lit257, [1], cl_lens=CL_REPEATS,
                                              header_syms=[(8, 0), (18, 127), (18, 127)]), 100))
    cases.append(("no-end-of-block-code", header([8] * 256 + [0], [1]), 100))
    cases.append(("lit-oversubscribed", header([7] * 257, [1]), 100))
    cases.append(("lit-incomplete", header([9] * 257, [1]), 100))
    cases.append(("dist-oversubscribed", header(lit257, [1, 1, 1]), 100))
    cases.append(("dist-incomplete", header(lit257, [2, 2]), 100))
    over = [0] * 19
    over[16] = over[17] = over[18] = 1
    cases.append(("codelen-oversubscribed", header(lit257, [1], cl_lens=over, header_syms=[(18, 0)]), 100))
    cases.append(("codelen-incomplete", header(lit257, [1], cl_lens=[4] * 15 + [0] * 4,
                                               header_syms=_header_syms_plain([8] * 10)), 100))
    # HCLEN 4 reaches 16, 17, 18 and 0: every length is 0, the end-of-block code among them
    only0 = [0] * 19
    only0[18], only0[0] = 1, 1
    cases.append(("hclen4-all-lengths-zero", header(lit257, [1], cl_lens=only0, hclen=4,
                                                    header_syms=[(18, 127), (18, 258 - 138 - 11)]), 100))
    for name, fill in (("codelen-all-zero-ff", b"\xff"), ("codelen-all-zero-00", b"\x00")):
        s = Stream()
        s.dynamic(lit257, [1], [], 1, cl_lens=[0] * 19, header_syms=[], eob=False)
        cases.append((name, s.bytes() + fill * 64, 100))
    return cases


def _fixed_cases():
    """[(name, stream, cap, expected or None)]"""
    cases = []

    def one(tokens, eob=True):
        s = Stream()
        s.fixed([65] + tokens, 1, eob=eob)
        return s.bytes() + TAIL

    cases.append(("fixed-symbol-286", one([Raw(0xC6, 8, True)], False), 100, None))
    cases.append(("fixed-symbol-287", one([Raw(0xC7, 8, True)], False), 100, None))
    cases.append(("fixed-dist-code-30", one([Raw(1, 7, True), Raw(30, 5, True)], False), 100, None))
    cases.append(("fixed-dist-code-31", one([Raw(1, 7, True), Raw(31, 5, True)], False), 100, None))
    cases.append(("fixed-dist-beyond-output", one([Raw(1, 7, True), Raw(1, 5, True)], False), 100, None))
    cases.append(("fixed-258-d1", one([(258, 1)]), 300, play([65, (258, 1)])))
    cases.append(("fixed-258-d1-cap-inside", one([(258, 1)]), 200, None))
    cases.append(("fixed-258-d1-cap-before", one([(258, 1)]), 1, None))
    return cases


def _tiny_blocks_case():
    """about 3 000 blocks: stored (0, 1, 5, 300 bytes), fixed (one literal) and dynamic (two literals; HLIT and
    HDIST over their whole ranges, fresh codes every time), so the tables are rebuilt every few bytes"""
    rnd = Lcg(303)
    s, out = Stream(), bytearray()
    for i in range(3000):
        kind = i % 3
        if kind == 0:
            data = bytes([i & 255]) * (0, 1, 5, 300)[(i // 3) % 4]
            s.stored(data, 0)
            out += data
        elif kind == 1:
            s.fixed([i & 255], 0)
            out.append(i & 255)
        else:
            nlit, ndist = 257 + (i // 3) % 30, 1 + (i // 3 + i // 90) % 30
            a, b = rnd.below(256), rnd.below(256)
            first = [256, a, b] if a != b else [256, a]
            rest = list(range(nlit))
            rnd.shuffle(rest)
            lit = complete_lengths(nlit, first + [x for x in rest if x not in first], deep=rnd.chance(50))
            order = list(range(ndist))
            rnd.shuffle(order)
            dist = complete_lengths(ndist, order, deep=rnd.chance(50)) if rnd.chance(80) else [0] * ndist
            s.dynamic(lit, dist, [a, b], 0)
            out += bytes([a, b])
    s.fixed([], 1)
    return s.bytes(), bytes(out)


def _stored_phases_case():
    """stored blocks of 0, 1 and 65535 bytes whose headers start at every bit phase"""
    rnd = Lcg(404)
    s, out = Stream(), bytearray()
    big = rnd.bytes(4096)
    for phase in range(8):
        for n in (0, 1, 65535):
            s.align()
            while s.phase() != phase:
                if (phase - s.phase()) % 2:
                    s.fixed([200], 0)  # 3 + 9 + 7 = 19 bits
                    out.append(200)
                else:
                    s.fixed([], 0)     # 3 + 7 = 10 bits
            assert s.phase() == phase
            data = (big * 17)[phase:phase + n]
            s.stored(data, 0)
            out += data
    s.stored(b"", 1)
    return s.bytes(), bytes(out)


def _stored_cases():
    rnd = Lcg(505)
    cases = []
    big = rnd.bytes(65535)
    s = Stream()
    s.stored(big, 0)
    s.stored(b"", 1)
    cases.append(("stored-65535", s.bytes(), 70000, big))
    s = Stream()
    s.stored(b"abcde", 1, nlen=0xFEFA)
    cases.append(("stored-bad-nlen", s.bytes() + TAIL, 100, None))
    s = Stream()
    s.fixed([97, 98, 99], 0)
    s.stored(b"", 0)
    s.fixed([100, (3, 4)], 1)
    cases.append(("stored-empty-in-the-middle", s.bytes(), 100, play([97, 98, 99, 100, (3, 4)])))
    return cases


def _composed(seed, window_bits, nblocks=60):
    """about 60 blocks of seeded type, 1 to 2 500 tokens each, about 40 % matches at the distances and lengths
    where the copy changes its path"""
    rnd = Lcg(seed)
    s, out = Stream(), bytearray()
    for _ in range(nblocks):
        kind = rnd.below(10)
        if kind == 0:
            data = rnd.bytes(rnd.choice([0, 1, 700, 9000]))
            s.stored(data, 0)
            out += data
            continue
        tokens, cur = [], len(out)
        for _ in range(rnd.between(1, 2501)):
            if cur and rnd.chance(40):
                d = rnd.choice([1, 2, 3, 511, 512, 513, 32768, rnd.between(1, 600), rnd.between(1, 32769)])
                n = rnd.choice([3, 4, 257, 258, rnd.between(3, 259)])
                tokens.append((n, min(d, cur)))
                cur += n
            else:
                tokens.append(rnd.below(256))
                cur += 1
        if kind == 1:
            s.fixed(tokens, 0)
        else:
            used = sorted(literal_length_symbols(tokens))
            rnd.shuffle(used)
            nlit = rnd.choice([286, max(max(used) + 1, 257)])
            lit = complete_lengths(nlit, used, deep=rnd.chance(70))
            dused = sorted(distance_symbols(tokens))
            rnd.shuffle(dused)
            if dused:
                ndist = rnd.choice([30, max(dused) + 1])
                dist = complete_lengths(ndist, dused, deep=rnd.chance(70))
            else:
                ndist = rnd.choice([1, 30])
                dist = complete_lengths(ndist, [], deep=rnd.chance(70)) if rnd.chance(50) else [0] * ndist
            s.dynamic(lit, dist, tokens, 0)
        out += play(tokens, bytes(out[-32768:]))
    s.fixed([], 1)
    out = bytes(out)
    return wrap(s.bytes(), out, window_bits), out


COMPOSED = ((0, 15), (1, 31), (2, -15))  # (seed, window_bits): each decodes in more than one piece at chunk_bytes 8192


@functools.lru_cache(maxsize=None)
def _built():
    cases, tokens_of = [], {}
    stream, out, tokens = _deep_case()
    cases.append(("deep", stream, len(out), -15, out))
    tokens_of["deep"] = tokens
    stream, out, tokens = _ring_edge_case()
    cases.append(("ring-edge", stream, len(out), -15, out))
    tokens_of["ring-edge"] = tokens
    cases += [(name, s, cap, -15, want) for name, s, cap, want in _oddities()]
    cases += [(name, s, cap, -15, None) for name, s, cap in _header_errors()]
    cases += [(name, s, cap, -15, want) for name, s, cap, want in _fixed_cases()]
    # a zlib and a gzip frame round two of the errors and two of the oddities: the error leaves before the trailer
    by_name = {c[0]: c for c in cases}
    for name in ("one-dist-code", "repeat18-into-dist", "one-dist-unused-bit", "fixed-dist-code-31"):
        _, s, cap, _, want = by_name[name]
        for wbits in (15, 31):
            cases.append((f"{name}-w{wbits}", wrap(s, want if want is not None else b"", wbits), cap, wbits, want))
    stream, out = _tiny_blocks_case()
    cases.append(("tiny-blocks", stream, len(out), -15, out))
    stream, out = _stored_phases_case()
    cases.append(("stored-phases", stream, len(out), -15, out))
    cases += [(name, s, cap, -15, want) for name, s, cap, want in _stored_cases()]
    for seed, wbits in COMPOSED:
        stream, out = _composed(seed, wbits)
        cases.append((f"composed-{seed}", stream, len(out), wbits, out))
    assert len({c[0] for c in cases}) == len(cases)
    return tuple(cases), tokens_of


def cases():
    """[(name, stream, dest_cap, window_bits, expected bytes at that cap, or None for a stream that is in
    error or whose cap cuts it short)]"""
    return list(_built()[0])


def tokens_of(name):
    """the tokens of `deep` or `ring-edge`, for a failure message that names the token"""
    return _built()[1][name]


def composed_names():
    return [f"composed-{seed}" for seed, _ in COMPOSED]


# ---- what is recorded ----

def sweep_of(name, stream, cap, expected_len):
    """[(cut, cap)] recorded for a case besides (len(stream), cap): a short case at every truncation and at
    caps {cap, 1, 2, 3}; a long one at a seeded dozen of truncations and at caps len, len - 1, len // 2"""
    if len(stream) < SHORT:
        return [(cut, c) for c in dict.fromkeys([cap, 1, 2, 3]) for cut in range(len(stream) + 1)
                if (cut, c) != (len(stream), cap)]
    rnd = Lcg(len(stream) * 31 + len(name))
    cuts = sorted({rnd.below(len(stream)) for _ in range(12)})
    n = cap if expected_len is None else expected_len
    return [(cut, cap) for cut in cuts] + [(len(stream), c) for c in dict.fromkeys([n, n - 1, n // 2]) if c != cap]


def rle(values):
    runs = []
    for v in values:
        if runs and runs[-1][0] == v:
            runs[-1][1] += 1
        else:
            runs.append([v, 1])
    return runs


def unrle(runs):
    return [v for v, k in runs for _ in range(k)]


def sha(data):
    return hashlib.sha256(data).hexdigest()


Record = namedtuple("Record", "name cut cap window_bits rc out_len consumed out_sha group")


def records(golden=None):
    """Every recorded (case, truncation, cap) with the reference's answer, and the streams by case name.  A
    long case's records and every case's full record carry the SHA-256 of the output; the records of a short
    case's sweep carry None and a group key instead: golden["cases"][name]["sweep_sha256"][cap] is the
    SHA-256 over the outputs' SHA-256 digests at that cap, in truncation order (group_digest())."""
    if golden is None:
        with open(GOLDEN) as f:
            golden = json.load(f)
    streams, recs = {}, []
    for name, stream, cap, wbits, want in cases():
        g = golden["cases"][name]
        assert g["stream_sha256"] == sha(stream), f"the builder no longer makes the recorded stream {name}"
        assert (g["cap"], g["window_bits"]) == (cap, wbits), name
        streams[name] = stream
        rc, out_len, consumed, out_sha = g["full"]
        recs.append(Record(name, len(stream), cap, wbits, rc, out_len, consumed, out_sha, None))
        if "points" in g:
            for cut, c, rc, out_len, consumed, out_sha in g["points"]:
                recs.append(Record(name, cut, c, wbits, rc, out_len, consumed, out_sha, None))
        else:
            for c, sw in g["sweep"].items():
                c = int(c)
                cuts = [cut for cut in range(len(stream) + 1) if (cut, c) != (len(stream), cap)]
                rcs, lens, used = unrle(sw["rc"]), unrle(sw["out_len"]), unrle(sw["consumed_minus_cut"])
                assert len(cuts) == len(rcs) == len(lens) == len(used), name
                for cut, a, b, u in zip(cuts, rcs, lens, used):
                    recs.append(Record(name, cut, c, wbits, a, b, u + cut, None, (name, c)))
    assert set(golden["cases"]) == set(streams), "the golden file holds cases the builder does not make"
    return recs, streams, golden


def group_digest(outputs):
    """the SHA-256 over the SHA-256 digests of a short case's outputs at one cap, in truncation order"""
    h = hashlib.sha256()
    for out in outputs:
        h.update(hashlib.sha256(out).digest())
    return h.hexdigest()


def check_outputs(recs, golden, outputs, what):
    """outputs[i]: the bytes a decoder gave for recs[i] -> the SHA-256 of each against the records"""
    groups = {}
    for r, out in zip(recs, outputs):
        if r.group is None:
            assert sha(out) == r.out_sha, (what, r.name, r.cut, r.cap, "output differs")
        else:
            groups.setdefault(r.group, []).append((r.cut, out))
    for (name, cap), outs in groups.items():
        assert group_digest([out for _, out in sorted(outs)]) == golden["cases"][name]["sweep_sha256"][str(cap)], (what, name, cap, "output differs")


def first_difference(got, want, tokens):
    """a failure message: the first differing offset and the token that produced it"""
    n = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    _, owner = play_slow(tokens)
    if n >= len(owner):
        return f"lengths differ: {len(got)} bytes, {len(want)} expected"
    k = owner[n]
    t = tokens[k]
    start = owner.index(k)
    return (f"first difference at offset {n}: token {k} = {t!r} (its output starts at {start}, byte {n - start} of it); "
            f"got {got[n]:#04x}, expected {want[n]:#04x}")
