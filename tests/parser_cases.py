"""Inputs built for the edges of the match search and the parsers (lz_parse_seg.h, lz_parse.h, lz_parse_pipe.h,
lz_parse_simple.h), and an independent reading of the parse a stream states.

No tests live here: tests/test_parser_edges_emu.py (CPU) and tests/test_gpu_parser_edges.py (GPU) use it,
tests/golden/make_parser_edges_golden.py records the compiled reference's answers for the same cases.

How a case is made visible.  The RFC 1951 walker of deflate_cases.py returns the token list of a stream:
(input position, length, distance) per copy, (position, 1, 0) per literal.  Every case names the FEATURES its
stream must show -- a token at a place, or the absence of one -- and they are asserted on the compiled
reference's stream, so "a copy of 20 bytes at distance exactly 250 starts at position 612" is a statement
about bytes that shares nothing with the kernels or the oracle.  A feature inside a stored block does not
hold (the block says nothing about its parse), so:

  - fillers are seeded bytes of a 16-value alphabet (FILL): dynamic blocks win;
  - planted strings are made of 5-bit byte values (PLANT).  The 15-bit hash of a trigram of such values is
    injective, and no trigram is used twice by a builder unless asked for, so nothing joins a planted chain by
    accident; chains whose length matters are checked position by position (Builder.chain);
  - every planted string stands between two separator bytes that occur once in the whole input (SEPS): no
    match runs into or out of it, and the parser arrives at its first byte with no match pending.

The level constants are read from the oracle's configuration table (levels()), not retyped.
"""
import hashlib
import json
import os
import re

import deflate_builder as B
import deflate_cases as D

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "parser_edges_golden.json")

HUFFMAN_ONLY, RLE, FIXED, FILTERED, DEFAULT = D.HUFFMAN_ONLY, D.RLE, D.FIXED, D.FILTERED, D.DEFAULT
MIN_LOOKAHEAD, TOO_FAR, MAX_MATCH = 262, 4096, 258
SEG_MIN = 3072          # longer buffers of levels 4-9 go to the segmented parser
SG_G, SG_OV = 256, 512  # its segment, and how far past one a parser looks for a hand-over

FILL = bytes(range(97, 113))
PLANT = bytes(range(32))
SEPS = tuple(range(128, 256))

# ---- the path hooks (SG_PATH in zsc_amd/csrc/lz_parse*.h, counted by tests/emu) ------------------------------
PATHS = {
    # the segmented parser: the lane-parallel search of chains below the budget (SG_EVAL_ONE)
    0: "SG_EVAL_ONE: first load reached", 1: "SG_EVAL_ONE: second load reached",
    2: "SG_EVAL_ONE: third load reached", 3: "SG_EVAL_ONE: fourth load reached",
    4: "SG_EVAL_ONE: ended by nice_length in the first load", 5: "... in the second load",
    6: "... in the third load", 7: "... in the fourth load",
    8: "SG_EVAL_ONE: bail (two candidates agree with p beyond 4 GRP bytes), the walk takes over",
    9: "SG_EVAL_ONE: pass skipped, best >= cap",
    10: "SG_EVAL_ONE: the chain head at exactly MAX_DIST accepted",
    11: "SG_EVAL_ONE: a link at exactly MAX_DIST rejected",
    12: "SG_EVAL_ONE: the chain head is outside the window",
    13: "SG_EVAL_ONE: pass ended behind its first compare (no lane can beat best)",
    # the 64-candidate walk (SG_EVAL) and what surrounds it
    14: "walk: the chain head at exactly MAX_DIST accepted", 15: "walk: a link at exactly MAX_DIST rejected",
    16: "SG_HEAD_BLOCKED yes, asked for the chain head", 17: "SG_HEAD_BLOCKED no, asked for the chain head",
    18: "SG_HEAD_BLOCKED yes, asked inside SG_EVAL (_edge)", 19: "SG_HEAD_BLOCKED no, asked inside SG_EVAL (_edge)",
    20: "SG_HEAD_BLOCKED yes, asked by the sweep", 21: "SG_HEAD_BLOCKED no, asked by the sweep",
    22: "walk: the budget runs out on candidates that change nothing (_nb >= budget)",
    23: "walk: the budget reaches zero on a compared candidate", 24: "walk: ended by nice_length",
    25: "walk: the chain leaves the window", 26: "head_ok false: longest_match is not called",
    # the staircase
    27: "staircase of three steps or more", 28: "staircase: the SG_FAR_OVER trip to memory taken",
    29: "staircase: a far chain chosen by that trip", 30: "staircase fallback check: first step to a level >= 5 at p itself",
    31: "staircase fallback check: ... at a later step", 32: "staircase fallback check: last step's candidate in p's tile",
    33: "staircase fallback check: ... in the previous tile", 38: "staircase: a step found on the chain of p + j, j > 0",
    47: "staircase fallback taken: the budget could have ended the walk",
    # the sweep
    34: "sweep chosen", 35: "sweep ended at the window's floor", 36: "sweep ended by nice_length",
    # around the search
    39: "no search: the pending match has max_lazy bytes or more", 40: "budget quartered (pending >= good_length)",
    48: "TOO_FAR: a match of three bytes dropped", 49: "Z_FILTERED: a match of five bytes or fewer dropped",
    # how a segment's parser ends
    41: "exit SYNCED on a fresh position", 42: "exit SYNCED on a neutral position", 43: "exit UNSYNCED (SG_OV passed)",
    44: "exit LAST (end of the super-step, or of the slots a pipeline parser may look into)", 45: "exit END",
    # the pipeline's resolver
    56: "pipeline resolver: follows a hand-over", 57: "pipeline resolver: asks for a redo after UNSYNCED",
    58: "pipeline resolver: asks for a redo after LAST", 59: "pipeline resolver: end of the input",
    # the wave-per-buffer parsers (LZ_EVAL_BATCH, lz_parse_lazy, lz_parse_greedy)
    64: "ring: the chain head at exactly MAX_DIST accepted", 65: "ring: a candidate at exactly MAX_DIST rejected",
    66: "ring: LZ_HEAD_BLOCKED yes", 67: "ring: LZ_HEAD_BLOCKED no",
    68: "greedy: a candidate in reach skipped as never inserted (counted under the greedy parser's test alone)",
    69: "ring: no live chain head, longest_match is not called", 70: "ring: ended by nice_length",
    71: "ring: the budget reaches zero", 72: "ring: the chain leaves the window",
    73: "ring: no search because of max_lazy", 74: "ring: budget quartered", 75: "ring: TOO_FAR drop",
    76: "ring: Z_FILTERED drop", 77: "greedy: a match longer than max_insert, its body is not inserted",
    # Z_RLE (lz_parse_rle)
    80: "rle: a step of 256 positions without a run", 81: "rle: a run shorter than 258 that ends inside the data",
    82: "rle: a run of 258", 83: "rle: a run that ends with the data",
}


def levels():
    """the reference's configuration table as the oracle states it: [{good, lazy, nice, chain, slow}] by level"""
    if not levels.cache:
        with open(os.path.join(ROOT, "oracle", "zsc_oracle.c")) as f:
            body = re.search(r"zo_levels\[10\]\s*=\s*\{(.*?)\};", f.read(), re.S).group(1)
        rows = re.findall(r"\{\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+)\s*\}", body)
        assert len(rows) == 10
        levels.cache = [dict(zip(("good", "lazy", "nice", "chain", "slow"), map(int, r))) for r in rows]
    return levels.cache


levels.cache = None


def sha(b):
    return hashlib.sha256(b).hexdigest()


# ---- the reading of a stream ---------------------------------------------------------------------------------

class Parse:
    """the token list of a stream, by input position"""

    def __init__(self, stream, window_bits):
        self.tokens = []
        self.blocks, self.data, _ = D.walk(stream, window_bits, self.tokens)
        self.at = {t[0]: t for t in self.tokens if t[2] >= 0}
        self.stored = [(t[0], t[0] + t[1]) for t in self.tokens if t[2] < 0]
        self.ends = {t[0] + t[1]: t for t in self.tokens if t[2] > 0}

    def in_stored(self, pos):
        return any(a <= pos < b for a, b in self.stored)

    def holds(self, f):
        """None if the feature holds, else why not"""
        kind = f[0]
        if kind == "stored":    # ("stored", (bool per block)): the one feature that is about stored blocks; a block
            # that is not stored must be larger than its stored form (five bytes of header at most)
            got = tuple(b.type == 0 for b in self.blocks)
            if got != tuple(f[1]):
                return "stored blocks %r" % (got,)
            small = [b.bits for b in self.blocks if b.type and b.bits <= 8 * (b.out_len + 5)]
            return None if not small else "a coded block smaller than its stored form"
        pos = f[1]
        span = f[2] if kind in ("copy", "lits") else 1
        if kind == "copy_end":  # ("copy_end", end, distance): a copy at that distance ends just before `end`
            t = self.ends.get(pos)
            if self.in_stored(pos - 1):
                return "stored block"
            return None if t is not None and t[2] == f[2] else "token ending there: %r" % (t,)
        if any(self.in_stored(x) for x in range(pos, pos + span)):
            return "stored block"
        if kind == "copy":      # ("copy", position, length, distance)
            t = self.at.get(pos)
            return None if t == (pos, f[2], f[3]) else "token there: %r" % (t,)
        if kind == "lits":      # ("lits", position, count): that many literals in a row
            bad = [self.at.get(x) for x in range(pos, pos + span) if self.at.get(x) != (x, 1, 0)]
            return None if not bad else "not a literal: %r" % (bad[0],)
        raise ValueError(f)

    def missing(self, features):
        return ["%r: %s" % (f, why) for f in features for why in [self.holds(f)] if why is not None]

    def summary(self, features):
        """what the golden file keeps per feature: the tokens the walker reads at the feature's place"""
        out = []
        for f in features:
            if f[0] == "stored":
                out.append([b.type for b in self.blocks])
            elif f[0] == "copy_end":
                out.append(list(self.ends.get(f[1], ())))
            else:
                out.append(list(self.at.get(f[1], ())))
        return out


# ---- building ------------------------------------------------------------------------------------------------

def hash15(d, q):
    return ((d[q] << 10) ^ (d[q + 1] << 5) ^ d[q + 2]) & 0x7fff


def ref_hash(d, q, mem_level):
    """the reference's hash of the trigram at q for a mem_level (hash_bits = mem_level + 7)"""
    bits = mem_level + 7
    shift = (bits + 2) // 3
    return ((d[q] << (2 * shift)) ^ (d[q + 1] << shift) ^ d[q + 2]) & ((1 << bits) - 1)


# the 15-bit hashes that trigrams of the filler's alphabet can have: planted trigrams keep away from them
FILL_HASHES = frozenset(((a << 10) ^ (b << 5) ^ c) & 0x7fff for a in FILL for b in FILL for c in FILL)
_attempt = [0]


def draw(make, *args, **kw):
    """make(*args): a case whose chains are what it planned.  A trigram next to a separator can still land on a
    planted chain by its hash; the builder then draws again with the next seed, as copies_input does."""
    for _attempt[0] in range(200):
        try:
            return make(*args, **kw)
        except Redraw:
            continue
        finally:
            _attempt[0] = 0
    raise AssertionError("no seed gives the planned chains: %r %r" % (make.__name__, args))


class Redraw(Exception):
    pass


def planned(ok):
    if not ok:
        raise Redraw()


class Builder:
    def __init__(self, seed):
        self.r = B.Lcg(seed)
        self.out = bytearray()
        self.seen = set()              # trigrams of planted strings handed out so far
        seps = list(SEPS)
        self.r.shuffle(seps)
        self.seps = seps
        self.features = []
        self.paths = set()
        self.ring_paths = set()
        self.avoid = set()
        self.edge = None               # the position the case is about, where it has one

    @property
    def pos(self):
        return len(self.out)

    def fill(self, n, adjacent_differ=False):
        for _ in range(n):
            b = self.r.choice(FILL)
            while adjacent_differ and self.out and self.out[-1] == b:
                b = self.r.choice(FILL)
            self.out.append(b)

    def fill_to(self, pos, **kw):
        assert pos >= self.pos, (pos, self.pos)
        self.fill(pos - self.pos, **kw)

    def sep(self):
        """one byte that occurs nowhere else in the input"""
        self.out.append(self.seps.pop())

    def put(self, s):
        at = self.pos
        self.out += s
        return at

    def fresh(self, n, alphabet=PLANT, first_not=None):
        """n bytes of 5-bit values none of whose trigrams this builder has handed out before"""
        s = bytearray()
        while len(s) < n:
            b = self.r.choice(alphabet)
            if not s and first_not is not None and b == first_not:
                continue
            if len(s) >= 2:
                t = (s[-2], s[-1], b)
                if t in self.seen or ((t[0] << 10) ^ (t[1] << 5) ^ t[2]) & 0x7fff in FILL_HASHES:
                    continue
                self.seen.add(t)
            s.append(b)
        return bytes(s)

    def other(self, b):
        """a 5-bit value that is not b"""
        while True:
            x = self.r.choice(PLANT)
            if x != b:
                return x

    def chain(self, p):
        """the positions before p that share p's 15-bit hash, newest first, as far as the tile of p and the one
        before it reach: this project's chain of p"""
        d, h = self.out, hash15(self.out, p)
        lo = max(((p >> 15) - 1) << 15, 0)
        return [q for q in range(p - 1, lo - 1, -1) if hash15(d, q) == h]

    def want(self, *features):
        self.features += features

    def reach(self, *ids):
        self.paths |= set(ids)

    def never(self, *ids):
        """hooks the case must not reach with the product's defaults"""
        self.avoid |= set(ids)

    def reach_ring(self, *ids):
        """... when the buffer is sent to the wave-per-buffer parser whatever its length (ZSC_HIP_NO_SEG)"""
        self.ring_paths |= set(ids)

    def case(self, name, size, level=6, window_bits=15, mem_level=8, strategy=DEFAULT):
        if size is not None:
            self.fill_to(size)
        c = Case(name, bytes(self.out), level, window_bits, mem_level, strategy, self.features, self.paths,
                 self.ring_paths)
        c.edge = self.edge
        c.avoid = frozenset(self.avoid)
        return c


class Case:
    def __init__(self, name, data, level, window_bits, mem_level, strategy, features, paths=(), ring_paths=()):
        self.name, self.data = name, data
        self.level, self.window_bits, self.mem_level, self.strategy = level, window_bits, mem_level, strategy
        self.features = tuple(features)
        self.paths = frozenset(paths)     # SG_PATH ids the case was built to reach (64 lanes, product defaults)
        self.ring_paths = frozenset(ring_paths)   # ... and when forced through the wave-per-buffer parser
        assert all(i in PATHS for i in self.paths | self.ring_paths), name
        self.edge = None
        self.avoid = frozenset()          # ... and ids it must not reach

    @property
    def family(self):
        return self.name[0]

    @property
    def params(self):
        return self.level, self.window_bits, self.mem_level, self.strategy

    @property
    def segmented(self):
        """does the runtime send it to the segmented parser?"""
        return levels()[self.level]["slow"] and len(self.data) > SEG_MIN and self.strategy not in (RLE, HUFFMAN_ONLY)


def run_features(s, r):
    """what every parser makes of r equal bytes from s on behind another byte: a literal, copies of at most 258
    from distance 1 while three bytes are left, literals"""
    f = [("lits", s, 1)]
    q, rem = s + 1, r - 1
    while rem >= 3:
        n = min(rem, MAX_MATCH)
        f.append(("copy", q, n, 1))
        q, rem = q + n, rem - n
    if rem:
        f.append(("lits", q, rem))
    return f


# ---- family A: window edges ----------------------------------------------------------------------------------

def a_edge(name, wbits, level, variant, dist_minus_max, slides, size, decoys=0, plant_len=20, p=None):
    """A planted string at p whose earlier occurrence lies `dist_minus_max` bytes beyond MAX_DIST.
    variant "head": the only earlier occurrence -- found at MAX_DIST, not beyond.
    variant "link": behind a nearer occurrence of its first five bytes -- found below MAX_DIST only; at MAX_DIST
    the rest of the string (whose chain the far occurrence heads) is found from there once the five are out.
    `slides`: window slides before p, which lies 100 bytes into a window unless `p` says where.  `decoys`: that many older entries on p's chain beyond the far occurrence,
    outside the window, which make the chain too long for the lane-parallel search of level 4 (budget 16)."""
    w = 1 << abs(wbits)
    md = w - MIN_LOOKAHEAD
    dist = md + dist_minus_max
    if p is None:
        p = w + 100 if slides == 0 else (slides + 2) * w + 100
    q = p - dist
    b = Builder(B.Lcg(hash_name(name)).next())
    s = b.fresh(plant_len)
    if decoys:
        assert q > 5 * decoys + 8
        for _ in range(decoys):
            b.put(s[:3] + bytes([b.other(s[3])]))
            b.sep()
    b.fill_to(q - 1)
    b.sep()
    assert b.put(s) == q
    b.sep()
    near = None
    if variant == "link":
        b.fill_to(p - 60 - 1)
        b.sep()
        near = b.put(s[:5])
        b.sep()
    b.fill_to(p - 1)
    b.sep()
    assert b.put(s) == p
    b.edge = p
    b.sep()
    want = [q] if near is None else [near, q]
    planned(b.chain(p)[:len(want)] == want and len(b.chain(p)) == len(want) + decoys)
    lane = level >= 4 and size > SEG_MIN and not decoys
    if variant == "head":
        if dist <= md:
            b.want(("copy", p, plant_len, dist))
            if level >= 4 and plant_len >= levels()[level]["lazy"]:
                b.reach(39 if size > SEG_MIN else 73)   # the position behind p is not searched
            if dist == md:
                b.reach(10 if lane else 14 if size > SEG_MIN and level >= 4 else 64)
        else:
            b.want(("lits", p, plant_len))
            if size > SEG_MIN and level >= 4:
                b.reach(12 if lane else 26)
            else:
                b.reach(69)
            b.reach_ring(69)
    else:
        if dist < md:
            b.want(("copy", p, plant_len, dist))
        elif dist == md:
            b.want(("copy", p, 5, 60), ("copy", p + 5, plant_len - 5, md))
            b.reach(11 if lane else 15 if size > SEG_MIN and level >= 4 else 65)
            b.reach_ring(65, 64)
        else:
            b.want(("copy", p, 5, 60), ("lits", p + 5, plant_len - 5))
            if decoys:
                b.reach(25)
            if size <= SEG_MIN:
                b.reach(72)
    return b.case(name, size, level, wbits)


def hash_name(name):
    return int(hashlib.sha256(("%s/%d" % (name, _attempt[0])).encode()).hexdigest()[:8], 16)


def a_base(name, wbits, level, slides, offset, size, plant_len=20):
    """The earlier occurrence starts at the window's base (`offset` 0: position 0, or the position the first or
    second slide makes the base) or one byte behind it, and p is the first position with that base (with no
    slide: the last one from which MAX_DIST reaches position 0).  At position 0 it is never a candidate -- the
    reference keeps 0 for "no position" -- and the copy starts one byte later; behind a slide the base is
    MAX_DIST + 1 away from the first position that has it, so nothing of the string is found; at base + 1 it is
    found, at exactly MAX_DIST then."""
    w = 1 << abs(wbits)
    md = w - MIN_LOOKAHEAD
    base = slides * w
    # the first position at which the window has slid `slides` times (none: the last one MAX_DIST reaches from 0)
    p = md if slides == 0 else (slides + 1) * w - MIN_LOOKAHEAD + 1
    q = base + offset
    b = Builder(B.Lcg(hash_name(name)).next())
    s = b.fresh(plant_len)
    if q:
        b.fill_to(q - 1)
        b.sep()
    assert b.put(s) == q
    b.sep()
    b.fill_to(p - 1)
    b.sep()
    assert b.put(s) == p
    b.edge = p
    b.sep()
    if offset == 0 and slides == 0:
        b.want(("lits", p, 1), ("copy", p + 1, plant_len - 1, p - q))
    elif offset == 0:
        # (behind a slide the base lies MAX_DIST + 1 or more back from every position: the distance alone decides)
        assert p - q == md + 1
        b.want(("lits", p, plant_len))
    else:
        b.want(("copy", p, plant_len, p - q))
    return b.case(name, size, level, wbits)


def family_a():
    out = []
    for wbits, size, lv in ((9, 3400, 6), (12, 13000, 6), (10, 4500, 9), (-15, 99000, 6)):
        for slides in (0, 1):
            for variant in ("head", "link"):
                for dm in (-1, 0, 1):
                    if abs(wbits) == 15 and (dm == -1 or (variant, slides) == ("link", 0)):
                        continue
                    out.append(draw(a_edge, "A-%s-w%d-s%d-md%+d" % (variant, wbits, slides, dm), wbits, lv, variant, dm, slides, size))
            for dm in (MIN_LOOKAHEAD - 1, MIN_LOOKAHEAD):   # wsize - 1 and wsize
                if abs(wbits) != 15:
                    out.append(draw(a_edge, "A-head-w%d-s%d-wsize%+d" % (wbits, slides, dm - MIN_LOOKAHEAD), wbits, lv, "head", dm,
                                      slides, size))
    # the wrapped 15-bit window (the raw one is above): the head and a link at MAX_DIST and one beyond, behind a slide
    for variant in ("head", "link"):
        for dm in (0, 1):
            out.append(draw(a_edge, "A-%s-w15-s1-md%+d" % (variant, dm), 15, 6, variant, dm, 1, 99000))
    # p the last position before a slide and the first behind it, the string MAX_DIST back both times.  The k-th
    # slide makes k wsize the base; the first position that has it is (k + 1) wsize - MIN_LOOKAHEAD + 1.  One
    # byte earlier the string starts at k wsize exactly and is found, since the base is still (k - 1) wsize; a
    # base that moved one position early would hide it.  Behind the slide it starts at the new base + 1.
    for wbits, size, lv in ((9, 3400, 6), (12, 13000, 6), (10, 4500, 9), (9, 2400, 6)):
        w = 1 << wbits
        for k in (1, 2):
            for when, p in (("last", (k + 1) * w - MIN_LOOKAHEAD), ("first", (k + 1) * w - MIN_LOOKAHEAD + 1)):
                out.append(draw(a_edge, "A-slide%d-%s-w%d-%d" % (k, when, wbits, size), wbits, lv, "head", 0, k, size, p=p))
    # the chain too long for the lane-parallel search: the walk's own tests of the head and of a link (level 4)
    for variant in ("head", "link"):
        for dm in (0, 1):
            out.append(draw(a_edge, "A-%s-walk-w12-md%+d" % (variant, dm), 12, 4, variant, dm, 1, 13000, decoys=20))
    # twins for the wave-per-buffer parser (at most 3 072 bytes)
    for variant in ("head", "link"):
        for dm in (0, 1):
            out.append(draw(a_edge, "A-%s-ring-w9-md%+d" % (variant, dm), 9, 6, variant, dm, 1, 2400))
    # the window's base
    for wbits, size, lv in ((9, 3400, 6), (12, 13000, 6)):
        for slides in (0, 1, 2):
            for offset in (0, 1):
                out.append(draw(a_base, "A-base-w%d-s%d+%d" % (wbits, slides, offset), wbits, lv, slides, offset, size))
    out.append(draw(a_base, "A-base-ring-w9-s1+0", 9, 6, 1, 0, 2400))
    return out


# ---- family B: short and far -----------------------------------------------------------------------------------

def b_input(strategy, level=6, size=9000):
    """Strings of 3, 4 and 5 bytes whose only earlier occurrence lies 4096 or 4097 bytes back, and strings of
    3 to 6 bytes 50 bytes back.  Z_DEFAULT and Z_FIXED drop three bytes beyond 4096, Z_FILTERED everything of five
    bytes or fewer."""
    name = "B-short-far-l%d-s%d-%d" % (level, strategy, size)
    b = Builder(B.Lcg(hash_name("B-short-far")).next())
    far = [(3, 4096), (3, 4097), (4, 4097), (5, 4097)] if size > 4600 else []
    strings = [b.fresh(n) for n, _ in far]
    at = 100
    first = []
    for s in strings:
        b.fill_to(at - 1)
        b.sep()
        first.append(b.put(s))
        b.sep()
        at += 40
    seg = level >= 4 and size > SEG_MIN
    for (n, dist), s, q in zip(far, strings, first):
        p = q + dist
        b.fill_to(p - 1)
        b.sep()
        assert b.put(s) == p
        b.sep()
        kept = not (strategy == FILTERED or (n == 3 and dist > TOO_FAR))
        b.want(("copy", p, n, dist) if kept else ("lits", p, n))
    if far:
        b.reach(49 if strategy == FILTERED else 48)
        b.reach_ring(76 if strategy == FILTERED else 75)
    b.fill(30)
    for n in (3, 4, 5, 6):
        s = b.fresh(n)
        b.sep()
        b.put(s)
        b.sep()
        b.fill(50 - n - 2)
        b.sep()
        p = b.put(s)
        b.sep()
        b.fill(20)
        b.want(("copy", p, n, 50) if strategy != FILTERED or n == 6 else ("lits", p, n))
    if not far and strategy == FILTERED:
        b.reach(76)
    return b.case(name, size, level, 15, 8, strategy)


def family_b():
    return [b_input(DEFAULT), b_input(FILTERED), b_input(FIXED), b_input(FILTERED, size=2000), b_input(DEFAULT, level=9)]


# ---- family C: chain length against the dispatch and the budget ----------------------------------------------

def c_chain(level, total, index, size=None):
    """p's chain has `total` entries that start with p's three bytes; entry `index` (0 the nearest) is the only
    one that goes on, for 12 bytes.  The others differ at the fourth byte: after the first of them they fail
    the pre-check and cost nothing."""
    name = "C-chain-l%d-%d-at%d" % (level, total, index)
    b = Builder(B.Lcg(hash_name(name)).next())
    s = b.fresh(12)
    b.fill(40)
    b.sep()
    entries = []
    for k in range(total - 1, -1, -1):   # the farthest first
        if k == index:
            entries.append(b.put(s))
            b.sep()
        else:
            entries.append(b.put(s[:3] + bytes([b.other(s[3])])))
    b.sep()
    b.fill_to(max(b.pos + 30, SEG_MIN + 40))
    b.sep()
    p = b.put(s)
    b.sep()
    planned(b.chain(p) == entries[::-1])
    b.want(("copy", p, 12, p - entries[total - 1 - index]))
    cfg = levels()[level]
    one_lim = min(cfg["chain"], 257)
    if total < one_lim:
        b.reach(index // 64)        # the load that holds the candidate is reached
    elif total >= 256:
        b.reach(38)                 # a staircase: the second step on the chain of a later, rarer trigram
    return b.case(name, b.pos + 200, level)


def c_budget(level, k, pending=None, tile=False):
    """The nearest candidate gives m bytes, then k decoys that pass the pre-check without improving on it (right
    at every byte but the fourth, so at bytes 0-2, m - 1 and m), then a candidate of m + 10.  Every compared
    candidate costs one unit of the level's chain budget: the long one is reached while 1 + k < budget.
    m is max_lazy or more, so that the position behind p is not searched (it would find the long candidate by a
    chain without decoys): the copy of m bytes stands, and the other ten follow as a copy of their own.
    `pending`: a match of that length is pending at p (it starts at p - 1, from a source of its own, which
    fails p's pre-check and is free); from good_length on it quarters the budget."""
    cfg = levels()[level]
    name = "C-budget-l%d-k%d" % (level, k) + ("-pending%d" % pending if pending else "") + ("-tile" if tile else "")
    b = Builder(B.Lcg(hash_name(name)).next())
    m = max(6, cfg["lazy"], (pending or 0) + 2)
    s = b.fresh(m + 10)
    lead = b.fresh(1)
    b.fill(40 if not tile else 32768 - 300 - (k + 3) * (m + 2))   # `tile`: every candidate in the tile before p's
    b.sep()
    far = b.put(s)
    b.sep()
    decoys = []
    for _ in range(k):
        decoys.append(b.put(s[:3] + bytes([b.other(s[3])]) + s[4:m + 1]))
        b.put(bytes([b.other(s[m + 1])]))
    near = b.put(s[:m])
    b.sep()
    src = None
    if pending:
        src = b.put(lead + s[:pending - 1])
        b.sep()
    b.fill_to(max(b.pos + 30, SEG_MIN + 40) if not tile else 32768 + 200)
    b.sep()
    if pending:
        b.put(lead)
    p = b.put(s)
    b.sep()
    planned(b.chain(p) == ([src + 1] if pending else []) + [near] + decoys[::-1] + [far])
    budget = cfg["chain"] >> 2 if pending and pending >= cfg["good"] else cfg["chain"]
    if pending:
        b.want(("lits", p - 1, 1))
    if 1 + k < budget:
        b.want(("copy", p, m + 10, p - far))
        if 2 + k == budget and k + 2 < 256:
            b.reach(23 if m + 10 < cfg["nice"] else 24)      # the long candidate takes the last unit, or is nice
    else:
        b.want(("copy", p, m, p - near), ("copy", p + m, 10, p - far))
        b.reach(22)          # (the decoys are counted together: they outnumber what is left of the budget)
        b.reach_ring(71)
    if pending and pending >= cfg["good"]:
        b.reach(40)
        b.reach_ring(74)
    if k + 2 >= 256 and not (pending and pending >= cfg["good"]):
        # a staircase: the steps are the near and the far candidate, the decoys lie between them on p's chain
        b.reach(47, 33 if tile else 32, 30 if pending else 31)
    return b.case(name, b.pos + 200, level)


def family_c():
    out = []
    for total in (63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257):
        out.append(draw(c_chain, 9, total, total - 1))
    for index in (0, 63, 64, 127, 128, 191, 192):   # (255 is the last entry, above)
        out.append(draw(c_chain, 9, 256, index))
    for total in (63, 127, 128, 129, 255, 256, 257):
        out.append(draw(c_chain, 6, total, total - 1))
    for level in (4, 5, 6, 7):
        budget = levels()[level]["chain"]
        for k in (budget - 3, budget - 2, budget - 1, budget, budget + 1):
            out.append(draw(c_budget, level, k))
    budget = levels()[7]["chain"]
    for k in (budget - 2, budget - 1):
        out.append(draw(c_budget, 7, k, tile=True))
    for level in (5, 6, 7):    # (level 4: good_length == max_lazy, a pending match of good_length is not searched on)
        cfg = levels()[level]
        for pending in (cfg["good"] - 1, cfg["good"]):
            budget = cfg["chain"] >> 2 if pending >= cfg["good"] else cfg["chain"]
            for k in (budget - 3, budget - 2, budget - 1):
                out.append(draw(c_budget, level, k, pending))
    return out


# ---- family D: ties, nice_length, the end of the data --------------------------------------------------------

def d_tie(level, length, i, j, total):
    """Two candidates of `length` bytes at chain indices i < j among `total`: the nearest wins."""
    name = "D-tie-l%d-len%d-%d-%d" % (level, length, i, j)
    b = Builder(B.Lcg(hash_name(name)).next())
    s = b.fresh(length + 1)
    b.fill(40)
    b.sep()
    entries = []
    for k in range(total - 1, -1, -1):
        if k in (i, j):
            entries.append(b.put(s[:length]))
            b.sep()
        else:
            entries.append(b.put(s[:3] + bytes([b.other(s[3])])))
    b.sep()
    b.fill_to(max(b.pos + 30, SEG_MIN + 40))
    b.sep()
    p = b.put(s[:length])
    b.sep()
    planned(b.chain(p) == entries[::-1])
    # (three bytes: every entry ties, the chain's first wins)
    b.want(("copy", p, length, p - entries[total - 1 - (i if length > 3 else 0)]))
    if length > 256 and i // 64 == j // 64 and total < min(levels()[level]["chain"], 257):
        b.reach(8, 24)
    return b.case(name, b.pos + 200, level)


def d_nice(level, near_len, index, total):
    """A nearer candidate of near_len bytes at chain index `index` in front of a farther one of 258: the walk
    stops at the first candidate that reaches nice_length."""
    cfg = levels()[level]
    name = "D-nice-l%d-%d-at%d-of%d" % (level, near_len, index, total)
    b = Builder(B.Lcg(hash_name(name)).next())
    s = b.fresh(MAX_MATCH)
    b.fill(40)
    b.sep()
    entries = []
    for k in range(total - 1, -1, -1):
        if k == total - 1:
            entries.append(b.put(s))
            b.sep()
        elif k == index:
            entries.append(b.put(s[:near_len]))
            b.sep()
        else:
            entries.append(b.put(s[:3] + bytes([b.other(s[3])])))
    b.sep()
    b.fill_to(max(b.pos + 30, SEG_MIN + 40))
    b.sep()
    p = b.put(s)
    b.sep()
    planned(b.chain(p) == entries[::-1])
    if near_len >= cfg["nice"]:
        b.want(("copy", p, near_len, p - entries[total - 1 - index]))
        if total < min(cfg["chain"], 257):
            b.reach(4 + index // 64)
        elif total < 256:
            b.reach(24)
    else:
        b.want(("copy", p, MAX_MATCH, p - entries[0]))
    return b.case(name, b.pos + 200, level)


def d_end(level, k, size=SEG_MIN + 300):
    """The data ends k bytes behind p, inside a repeat: the match reaches exactly the last byte.  nice_length and
    the match are cut to the lookahead; the last two positions own no trigram."""
    name = "D-end-l%d-k%d-%d" % (level, k, size)
    b = Builder(B.Lcg(hash_name(name)).next())
    s = b.fresh(MAX_MATCH + 4)
    b.fill(40)
    b.sep()
    q = b.put(s)
    b.sep()
    b.fill_to(size - k - 1)
    b.sep()
    p = b.put(s[:k])
    n = min(k, MAX_MATCH)
    b.want(("copy", p, n, p - q))
    if 3 <= k < levels()[level]["lazy"] and levels()[level]["slow"] and size > SEG_MIN and k > 3:
        b.reach(9)      # the next position is searched with as many bytes pending as are left
    if levels()[level]["slow"] and size > SEG_MIN and k < levels()[level]["nice"]:
        b.reach(4)      # nice_length is cut to the lookahead: the one candidate reaches it
    if levels()[level]["slow"] and size <= SEG_MIN:
        b.reach(70)     # ... and in the wave-per-buffer parser
    if k > n:
        b.want(("lits", p + n, k - n))
    return b.case(name, None, level)


def family_d():
    out = []
    for length in (3, 4, 8, 9, 32, 33, 258):
        out.append(draw(d_tie, 9, length, 10, 20, 80))     # the same load
        out.append(draw(d_tie, 9, length, 10, 70, 80))     # neighbouring loads
    out.append(draw(d_tie, 9, 8, 130, 200, 210))
    out.append(draw(d_tie, 9, 33, 70, 200, 210))
    out.append(draw(d_tie, 6, 8, 10, 70, 80))
    out.append(draw(d_tie, 6, 9, 130, 200, 210))           # level 6 walks a chain of 128 entries or more
    nice = levels()[7]["nice"]
    for index in (5, 70, 135, 200):                  # level 7: budget 256, every load of the lane-parallel search
        for near_len in (nice - 1, nice, nice + 1):
            out.append(draw(d_nice, 7, near_len, index, 210))
    nice = levels()[6]["nice"]
    for near_len in (nice - 1, nice, nice + 1):      # level 6, 140 entries: the walk
        out.append(draw(d_nice, 6, near_len, 70, 140))
    for level in (6, 9):
        nice = levels()[level]["nice"]
        for k in sorted({3, 4, 5, nice - 1, nice, 257, 258, 259}):
            out.append(draw(d_end, level, k))
    for k in (3, 4, 258):
        out.append(draw(d_end, 6, k, size=1500))
    return out


# ---- family E: lazy boundaries -------------------------------------------------------------------------------

def e_lazy(level, pending, next_len):
    """A match of `pending` bytes at p and one of `next_len` at p + 1, from sources of their own."""
    cfg = levels()[level]
    name = "E-lazy-l%d-%d-then-%d" % (level, pending, next_len)
    b = Builder(B.Lcg(hash_name(name)).next())
    z = b.fresh(max(pending, next_len + 1) + 1)
    b.fill(40)
    b.sep()
    c1 = b.put(z[:pending])
    b.sep()
    b.fill(30)
    b.sep()
    c2 = b.put(z[1:1 + next_len])
    b.sep()
    b.fill_to(SEG_MIN + 40)
    b.sep()
    p = b.put(z[:max(pending, next_len + 1)])
    b.sep()
    if pending < cfg["lazy"] and next_len > pending:
        b.want(("lits", p, 1), ("copy", p + 1, next_len, p + 1 - c2))
    else:
        b.want(("copy", p, pending, p - c1))
        if pending >= cfg["lazy"]:
            b.reach(39)
        else:
            b.reach(13)
    return b.case(name, b.pos + 200, level)


def e_ladder(level, m=4, steps=11):
    """`steps` positions in a row, each with a match one byte longer than the one before: a literal for each but
    the last, then its copy"""
    name = "E-ladder-l%d" % level
    b = Builder(B.Lcg(hash_name(name)).next())
    z = b.fresh(m + 2 * steps)
    b.fill(40)
    src = []
    for i in range(steps):
        b.sep()
        src.append(b.put(z[i:i + m + i]))
        b.sep()
        b.fill(20)
    b.fill_to(SEG_MIN + 40)
    b.sep()
    p = b.put(z[:m + 2 * steps - 2])
    b.sep()
    last = steps - 1
    b.want(("lits", p, last), ("copy", p + last, m + last, p + last - src[last]))
    return b.case(name, b.pos + 200, level)


def family_e():
    out = []
    for level in (4, 6, 8):
        lazy = levels()[level]["lazy"]
        out += [draw(e_lazy, level, lazy - 1, lazy), draw(e_lazy, level, lazy, lazy + 1), draw(e_lazy, level, lazy - 1, lazy - 1)]
    out += [draw(e_lazy, 9, 257, 258), draw(e_ladder, 6), draw(e_ladder, 9)]
    return out


# ---- family F: runs and periods ------------------------------------------------------------------------------

def f_runs(level, strategy=DEFAULT, size=SEG_MIN + 3000, name=None):
    """runs of one byte value, each of a value of its own, between separators"""
    name = name or "F-runs-l%d-s%d" % (level, strategy)
    b = Builder(B.Lcg(hash_name("F-runs")).next())
    values = list(range(32))
    b.fill(50, adjacent_differ=True)
    for r in (3, 4, 5, 6, 259, 260, 261, 262) + ((517, 518, 519, 520) if size > SEG_MIN else ()):
        v = values.pop()
        b.sep()
        s = b.put(bytes([v]) * r)
        b.sep()
        b.fill(23, adjacent_differ=True)
        b.want(*run_features(s, r))
    b.fill_to(size - 301, adjacent_differ=True)
    b.sep()
    s = b.put(bytes([values.pop()]) * 300)      # a run that ends with the data
    b.want(*run_features(s, 300))
    if strategy == RLE:
        b.reach(81, 82, 83)
    elif size > SEG_MIN and level == 6:
        b.reach(28, 29)     # near a long run's end the chains in reach are its own: the trip to the far ones
    return b.case(name, None, level, 15, 8, strategy)


def f_period(level, period, total, size=SEG_MIN + 200):
    name = "F-period-l%d-%d" % (level, period)
    b = Builder(B.Lcg(hash_name(name)).next())
    unit = b.fresh(period) if period >= 3 else bytes(PLANT[5:5 + period])
    if period >= 3:   # (the trigrams across the joint must be new as well)
        while len({(unit * 2)[i:i + 3] for i in range(period)}) < period:
            unit = b.fresh(period)
    b.fill(60)
    b.sep()
    s = b.put((unit * (total // period + 1))[:total])
    b.sep()
    b.want(("lits", s, period), ("copy", s + period, min(MAX_MATCH, total - period), period))
    return b.case(name, max(size, b.pos + 100), level)


def f_run_tail(level, run, times=2):
    """a run and a tail of eight bytes, all of it repeated: near the run's end the chains in reach are the
    run's own, and the repeat is found through the chains of the tail's trigrams"""
    name = "F-run-tail-l%d-%d-x%d" % (level, run, times)
    b = Builder(B.Lcg(hash_name(name)).next())
    tail = b.fresh(8, alphabet=PLANT[1:])
    unit = bytes([0]) * run + tail
    b.fill(60)
    at = []
    for _ in range(times):
        b.sep()
        at.append(b.put(unit))
        b.sep()
        b.fill(150)
    dist = at[-1] - at[-2]
    b.want(("copy_end", at[-1] + len(unit), dist))
    if run >= 300 and level == 6:
        b.reach(27, 28, 47, 34, 36)
    return b.case(name, max(SEG_MIN + 200, b.pos + 100), level)


def family_f():
    out = [f_runs(6), f_runs(9), f_runs(4), f_runs(6, size=2900, name="F-runs-ring-l6")]
    for period in (2, 3, 4, 257, 258, 259, 260):
        out.append(draw(f_period, 6, period, 3 * max(period, 200)))
    out.append(draw(f_period, 9, 258, 800))
    for run in (70, 130, 300, 5000):
        out.append(draw(f_run_tail, 6, run))
    out.append(draw(f_run_tail, 9, 300, times=3))
    return out


# ---- family G: segment, super-step, tile and ring boundaries -------------------------------------------------

def g_copies(name, level, boundaries, size):
    """a copy of 258 bytes that starts `back` bytes in front of a boundary, for each (boundary, back); its source
    lies 400 bytes before it"""
    b = Builder(B.Lcg(hash_name(name)).next())
    for boundary, back in boundaries:
        p = boundary - back
        s = b.fresh(MAX_MATCH)
        b.fill_to(p - 400 - 1)
        b.sep()
        b.put(s)
        b.sep()
        b.fill_to(p - 1)
        b.sep()
        assert b.put(s) == p
        b.edge = b.edge or p
        b.sep()
        b.want(("copy", p, MAX_MATCH, 400))
    if size > 8192:
        b.reach(44)
    return b.case(name, size, level)


def g_run(name, level, start, length, size, reach=(), random_before=False, never=()):
    """one run of `length` equal bytes from `start` on, literals around it"""
    b = Builder(B.Lcg(hash_name(name)).next())
    if random_before:
        b.put(D.distinct_trigram_bytes(b.r, start - 1))
    else:
        b.fill_to(start - 1)
    b.sep()
    assert b.put(bytes([7]) * length) == start
    b.edge = start
    b.sep()
    b.want(*run_features(start, length))
    b.reach(*reach)
    b.never(*never)
    if random_before:
        b.put(D.distinct_trigram_bytes(b.r, size - b.pos))
    return b.case(name, size, level)


def family_g():
    out = []
    backs = (258, 257, 3, 2, 1, 0)
    out.append(draw(g_copies, "G-copies-256", 6, [(2048 + 768 * i, k) for i, k in enumerate(backs)], 7000))
    out.append(draw(g_copies, "G-copies-8192", 6, [(8192 * (1 + i), k) for i, k in enumerate(backs)], 8192 * 6 + 400))
    out.append(draw(g_copies, "G-copies-tile-ring", 6, [(32768, 257), (32768 + 8192, 0), (45056, 1), (45056 + 2048, 258),
                                                   (90112, 2), (90112 + 768, 3)], 92000))
    out.append(draw(g_copies, "G-copies-256-l9", 9, [(2048 + 768 * i, k) for i, k in enumerate(backs)], 7000))
    # a run from r0 through a segment start S: the parser of the segment before is fresh at r0 + 1 + 258 i, the one
    # that starts at S at S + 258 i (S + 1 + 258 i with its literal owed): they meet at once or not inside the run
    S = 4096
    out.append(draw(g_run, "G-run-meets", 6, S - 1 - 258, 258 + 400, 6000, reach=(41, 45)))
    out.append(draw(g_run, "G-run-misses", 6, S - 100, 100 + 400, 6000, reach=(42,)))
    # the run ends d bytes past the end e_s of the segment it starts in.  That segment's parser is fresh behind
    # every copy of the run and meets no other parser inside it; behind the run's end, at e_s + d, the literals
    # hand it over.  Up to d = 512 it never gives up (hook 43 is not reached by the whole buffer), from 513 on it
    # does and the segments behind are parsed again.  d = 512 is the edge of `p >= e_s + SG_OV`: the parser is
    # fresh at exactly e_s + SG_OV, where the parser of the segment that starts there was fresh too, and the
    # hand-over is tested before the give-up.  A parser that is not handed over at that position and gives up
    # one token later (`>` for `>=`) ends with the same tokens, the redo starts where it ended: no stream and
    # no hook tells the two apart.
    for d in (1, 255, 256, 257, 511, 512, 513, 1100):
        out.append(draw(g_run, "G-run-past-%d" % d, 6, S - 200, 200 + d, 6500, reach=(41, 42) + ((43,) if d >= 513 else ()),
                        never=() if d >= 513 else (43,)))
    # behind incompressible bytes every hand-over is on a neutral position (a literal owed)
    out.append(draw(g_run, "G-run-random-past-255", 6, S - 200, 200 + 255, 6500, random_before=True, reach=(42,), never=(43,)))
    out.append(draw(g_run, "G-run-random-past-513", 6, S - 200, 200 + 513, 6500, random_before=True, reach=(42, 43)))
    return out


# ---- family H: the greedy parser ------------------------------------------------------------------------------

def h_insert(level, extra):
    """A copy of max_insert + extra bytes, then a string whose only earlier occurrence starts two bytes before
    that copy's end.  The greedy parser inserts the body of a copy of at most max_insert bytes: found with
    extra == 0; with extra == 1 the first two positions of the string's source were never inserted and the match
    starts two bytes later, at the first position behind the copy."""
    mi = levels()[level]["lazy"]      # (max_insert_length shares the field)
    m = mi + extra
    name = "H-insert-l%d-%+d" % (level, extra)
    b = Builder(B.Lcg(hash_name(name)).next())
    x = b.fresh(m)
    t = b.fresh(5)
    b.fill(40)
    b.sep()
    b.put(x)
    b.sep()
    b.fill(30)
    b.sep()
    c = b.put(x)          # the copy
    b.put(t)              # ... and what follows it
    b.sep()
    b.fill(30)
    b.sep()
    r = b.put(x[-2:] + t)
    b.sep()
    b.want(("copy", c, m, c - (40 + 1)))
    if extra == 0:
        b.want(("copy", r, 7, r - (c + m - 2)))
    else:
        b.want(("lits", r, 2), ("copy", r + 2, 5, r - (c + m - 2)))
        b.reach(77, 68)
    return b.case(name, 1200, level)


def family_h():
    out = []
    for level in (1, 2, 3):
        out += [draw(h_insert, level, 0), draw(h_insert, level, 1)]
    for level, wbits, size in ((1, 12, 13000), (2, 9, 3400), (3, -15, 99000)):
        for variant in ("head", "link"):
            for dm in (0, 1):
                out.append(draw(a_edge, "H-%s-l%d-w%d-md%+d" % (variant, level, wbits, dm), wbits, level, variant, dm, 1, size))
        if abs(wbits) != 15:
            for offset in (0, 1):
                out.append(draw(a_base, "H-base-l%d-w%d+%d" % (level, wbits, offset), wbits, level, 1, offset, size))
        for k in (3, 4, 5, 258, 259):
            c = draw(d_end, level, k, size=1500)
            c.name = "H-end-l%d-k%d" % (level, k)
            out.append(c)
    # family I's blocker inside the body of a copy: inserted (it blocks) and never inserted (it blocks nothing)
    for level, ml in ((1, 1), (2, 4), (3, 9)):
        for body in ("inserted", "skipped"):
            out.append(draw(i_case, "H-blocker-%s-l%d-m%d" % (body, level, ml), ml, 9, "blocked", 2400, level=level, body=body))
    return out


# ---- family I: hash sizes other than 15 bits ------------------------------------------------------------------

def same_hash_trigram(b, target, mem_level, same15, same_ref):
    """three bytes that are not `target` and whose 15-bit hash and reference hash for mem_level equal target's or
    not, as asked; byte values between the planted alphabet and the filler's, or just above the filler's"""
    pool = list(range(32, 97)) + list(range(113, 128))
    b.r.shuffle(pool)
    t15, tref = hash15(target, 0), ref_hash(target, 0, mem_level)
    bits = mem_level + 7
    shift = (bits + 2) // 3
    for x in pool:
        for y in pool:
            # the third byte that makes the hash asked for equal, if one does
            if same_ref:
                z = (tref ^ (x << (2 * shift)) ^ (y << shift)) & 0xff
            elif same15:
                z = (t15 ^ (x << 10) ^ (y << 5)) & 0xff
            else:
                z = b.r.choice(pool)
            t = bytes((x, y, z))
            if z in pool and t != target[:3] and (hash15(t, 0) == t15) == same15 and (ref_hash(t, 0, mem_level) == tref) == same_ref:
                return t
    raise Redraw()


def i_case(name, mem_level, wbits, kind, size, plant_len=20, dense=0, level=6, body=None):
    """A candidate at exactly MAX_DIST heads the REFERENCE's chain, whose hash has mem_level + 7 bits, only if no
    position between it and p has p's hash under that function.
    kind "free": none has -- found.  "blocked": a different trigram with that hash stands in between (but not on
    this project's 15-bit chain, where the candidate is first) -- a link, dead; the rest of the string is found
    from the next position on.  "edge": a trigram in between shares the 15-bit hash and not the reference's: the
    candidate is second in this project's chain and still the reference's head -- found.  "edge-blocked"
    (hash sizes below 15 bits, where sharing the 15-bit hash implies sharing the reference's): second here, dead.
    `dense`: that many more entries on p's chain, older than the window: a chain of more than 256 entries in a
    window this small is searched by the sweep, which asks the same question for the position at its floor.
    `body` (kind "blocked", levels 1-3): the blocking trigram is the second to fourth byte of a string y that the
    greedy parser copies from an occurrence in front of the candidate.  "inserted": y has max_insert bytes, the
    copy's body enters the chains and the blocker blocks.  "skipped": y has max_insert + 1 bytes, its body is
    never inserted, the blocker is on no chain and the candidate is found -- by the hash alone it would be dead."""
    w = 1 << wbits
    md = w - MIN_LOOKAHEAD
    p = 3 * w + 100
    q = p - md
    b = Builder(B.Lcg(hash_name(name)).next())
    s = b.fresh(plant_len)
    far = [b.put(s[:3] + bytes([b.other(s[3])])) for _ in range(dense)]
    y = y_first = y_copy = None
    if body:
        assert kind == "blocked" and not levels()[level]["slow"]
        m = levels()[level]["lazy"] + (body == "skipped")      # (max_insert_length shares the field)
        y = b.fresh(1) + same_hash_trigram(b, s, mem_level, False, True) + b.fresh(m - 4)
        b.fill_to(q - 30)
        b.sep()
        y_first = b.put(y)
        b.sep()
    b.fill_to(q - 1)
    b.sep()
    assert b.put(s) == q
    b.sep()
    x = None
    if body:
        b.fill_to(p - 80)
        b.sep()
        y_copy = b.put(y)
        x = y_copy + 1
        b.sep()
    elif kind != "free":
        b.fill_to(p - 80)
        b.sep()
        x = b.put(same_hash_trigram(b, s, mem_level, kind != "blocked", kind != "edge"))
        b.sep()
    b.fill_to(p - 1)
    b.sep()
    assert b.put(s) == p
    b.sep()
    b.fill_to(size)
    d = b.out
    between = [y for y in range(q + 1, p) if ref_hash(d, y, mem_level) == ref_hash(d, p, mem_level)]
    planned(b.chain(p) == ([q] if kind in ("free", "blocked") else [x, q]) + far[::-1])
    planned(between == ([] if kind in ("free", "edge") else [x]))
    # (the string's second trigram must head its reference chain too, for the copy that starts one byte later)
    planned(not [y for y in range(q + 2, p + 1) if ref_hash(d, y, mem_level) == ref_hash(d, p + 1, mem_level)])
    seg = size > SEG_MIN and levels()[level]["slow"]
    if body:
        b.want(("copy", y_copy, len(y), y_copy - y_first))
    if kind in ("free", "edge") or body == "skipped":
        b.want(("copy", p, plant_len, md))
        b.reach((17 if kind == "free" else 19 if not dense else 21) if seg else 67)
    else:
        b.want(("lits", p, 1), ("copy", p + 1, plant_len - 1, md))
        b.reach((16 if kind == "blocked" else 18 if not dense else 20) if seg else 66)
    if dense:
        b.reach(34)
        if kind == "edge-blocked":
            b.reach(35)
    return b.case(name, size, level, wbits, mem_level)


def family_i():
    out = []
    for ml in (1, 4, 7, 9):
        for wbits, size in ((9, 3400), (12, 13000), (9, 2400)):
            if ml == 1 and wbits == 12:
                # (an 8-bit hash: some position among MAX_DIST = 3 834 has p's hash, whatever is planted)
                continue
            for kind in ("free", "blocked", "edge" if ml in (1, 4, 9) else "edge-blocked"):
                if size <= SEG_MIN and kind.startswith("edge"):
                    continue
                out.append(draw(i_case, "I-%s-m%d-w%d-%d" % (kind, ml, wbits, size), ml, wbits, kind, size))
    out.append(draw(i_case, "I-edge-m9-w9-sweep", 9, 9, "edge", 3400, dense=300))
    out.append(draw(i_case, "I-edge-blocked-m7-w9-sweep", 7, 9, "edge-blocked", 3400, dense=300))
    return out


# ---- family J: stored blocks across window slides -------------------------------------------------------------

def family_j():
    """Incompressible bytes.  A block may be stored only while its first byte is still in the window when it is
    flushed.  The k-th slide (at (k + 1) wsize - MIN_LOOKAHEAD bytes of input) makes k wsize the base; a block
    that began below it goes out coded although a stored block would be smaller.  Sizes one byte before a slide
    and at it; blocks of 2^(mem_level + 6) - 1 literals.  The feature lists, block by block, whether it is stored.
    A full block that ends at e is flushed with e the next position, behind every slide whose first position
    (k + 1) wsize - MIN_LOOKAHEAD + 1 is at most e; the last block is flushed behind every slide the size reaches.

    What the sets can show.  mem_level 9 (blocks of 32 767): at the first slide the one block, or the second of
    two, starts below wsize; at the second slide of the 15-bit window the second block, which starts one byte
    below wsize, has already gone out coded and the third starts two bytes below 2 wsize.  In the 9- and 12-bit
    windows the one block starts at 0, and the second slide changes nothing that the first has not.
    (9, 1) and (15, 8), blocks of 127 and 16 383: a block is flushed at most that many bytes behind its start,
    and the base lies wsize - MIN_LOOKAHEAD or more behind the position that meets it, so no block ever starts
    below the base: every block is stored on both sides of the slide.  These four state that the slide alone
    forbids nothing."""
    out = []
    for wbits, ml in ((9, 9), (9, 1), (12, 9), (15, 9), (15, 8)):
        w = 1 << wbits
        cap = (1 << (ml + 6)) - 1
        for k in (1, 2) if ml == 9 else (1,):
            slide = (k + 1) * w - MIN_LOOKAHEAD
            for n in (slide - 1, slide):
                data = D.distinct_trigram_bytes(B.Lcg(1000 * wbits + ml), n)
                flags = []
                for start in range(0, n, cap):
                    end = start + cap
                    slides = max(0, (end + MIN_LOOKAHEAD - 1) // w - 1) if end < n else max(0, (n + MIN_LOOKAHEAD) // w - 1)
                    flags.append(start >= slides * w)
                out.append(Case("J-stored-w%d-m%d-%d" % (wbits, ml, n), bytes(data), 6, wbits, ml, DEFAULT,
                                [("stored", tuple(flags))]))
                out[-1].edge = slide
    return out


# ---- family K: Z_RLE and Z_HUFFMAN_ONLY ----------------------------------------------------------------------

def k_rle(level, phase):
    """runs of 2, 3, 4, 258, 259, 260 and 261 equal bytes, the first of them `phase` bytes into the input: the
    kernel looks at 256 positions a step, and the runs begin at every place of a step as `phase` goes round"""
    name = "K-rle-l%d-phase%d" % (level, phase)
    b = Builder(B.Lcg(hash_name(name)).next())
    b.fill(phase, adjacent_differ=True)
    for i, r in enumerate((2, 3, 4, 258, 259, 260, 261, 262)):
        b.sep()
        s = b.put(bytes([i]) * r)
        b.sep()
        b.fill(251 + i, adjacent_differ=True)
        b.want(*run_features(s, r))
    b.reach(80, 81, 82)
    return b.case(name, b.pos + 300, level, 15, 8, RLE)


def family_k():
    out = [draw(k_rle, 6, ph) for ph in (5, 69, 133, 197, 250, 253, 254, 255, 256)]
    out.append(f_runs(1, RLE, name="K-rle-runs-l1"))
    b = Builder(7)
    b.fill(3500)
    b.want(("lits", 0, 3500))
    out.append(b.case("K-huffman-only", None, 6, 15, 8, HUFFMAN_ONLY))
    return out


FAMILIES = (family_a, family_b, family_c, family_d, family_e, family_f, family_g, family_h, family_i, family_j,
            family_k)
_CASES = []


def cases():
    """every case, built once"""
    if not _CASES:
        for fam in FAMILIES:
            _CASES.extend(fam())
        assert len({c.name for c in _CASES}) == len(_CASES)
    return _CASES


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)
