"""Streams that use zlib preset dictionaries, with what inflating them must give.

A plain helper module: tests/test_inflate_dict_emu.py, tests/test_gpu_inflate_dict.py and
tests/golden/make_inflate_dict_golden.py import it.  Nothing here calls the code under test.

Two sources of streams:

  recorded()   streams CPython's zlib wrote with zlib.compressobj(..., zdict=D), kept as hex in
               tests/golden/inflate_dict_golden.json so that another zlib build cannot change them.  The
               expected output is what CPython's zlib.decompressobj(wbits, zdict=D) gives now; the golden
               file pins its SHA-256.
  handbuilt()  streams built bit by bit with tests/deflate_builder.py for the places where a copy out of the
               dictionary can go wrong.  The expected output is deflate_builder.play(tokens, history=T), T the
               part of the dictionary the window holds.

A Case is (name, stream, window_bits, dest_cap, dict, status, out, consumed): dict is the stream's
dictionary (bytes) or None for no dictionary (ZSC_HIP_NO_DICT), and (status, out, consumed) is the
contract's answer (include/zsc_hip.h).  How the expectation of an erroneous hand-built stream comes about:
the stream is cut off by the data error, the bytes made so far stay, and zsc_uncompress's inflateSync finds no
flush marker in the rest of the input (eight zero bytes are appended so that it has something to search), which
makes the status Z_DATA_ERROR and consumed the whole input (reference src/zsc_uncompr.c:109-125,
src/inflate.c:1585-1593).  A dictionary that inflateSetDictionary refuses is Z_DATA_ERROR with nothing out and
nothing consumed; FDICT without a dictionary is Z_NEED_DICT, the same.
"""
import hashlib
import json
import os
import struct
import zlib
from collections import namedtuple

import deflate_builder as db
from zsc_amd import corpus

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "inflate_dict_golden.json")

Z_OK, Z_NEED_DICT, Z_DATA_ERROR = 0, 2, -3
TAIL = b"\x00" * 8

Case = namedtuple("Case", "name stream wbits cap dict status out consumed")


def make_dict(kind, seed, length):
    return corpus.make_buffer(kind, length, seed)


def window_part(d, wbits):
    """the bytes of dictionary d a window of |wbits| bits holds: what lies before byte 0 of the output"""
    return d[max(0, len(d) - (1 << abs(wbits))):]


def zlib_header(cinfo, fdict):
    cmf = 0x08 | (cinfo << 4)
    flg = 0x20 if fdict else 0
    flg += 31 - ((cmf << 8) + flg) % 31
    return bytes([cmf, flg])


def zlib_dict_wrap(raw, out, dict_id, cinfo=7, adler=None):
    """raw deflate data in a zlib wrapper with FDICT: header, DICTID, data, Adler-32 of the output alone"""
    return (zlib_header(cinfo, True) + struct.pack(">I", dict_id) + raw +
            struct.pack(">I", db.adler32(out) if adler is None else adler))


# ---- recorded streams ----

def recorded_specs():
    """what tests/golden/make_inflate_dict_golden.py records: every window size, zlib and raw, at levels 1, 6
    and 9, two dictionary lengths each.  A raw stream is only recorded where it needs its dictionary, which a
    dictionary of one byte cannot bring about (no three-byte match fits in it): that length goes to zlib
    streams, where FDICT and the id are what is checked."""
    lens = [1, 511, 512, 513, 32767, 32768, 32769, 51200]
    specs, k = [], 0
    for raw in (False, True):
        pool = [n for n in lens if not (raw and n == 1)]
        for bits in range(9, 16):
            for level in (1, 6, 9):
                for _ in range(2):
                    n = pool[k % len(pool)]
                    size = [64, 300, 1000, 2500, 5000, 8192][k % 6]
                    specs.append({"name": "rec%03d" % len(specs), "wbits": -bits if raw else bits, "level": level,
                                  "dict": {"kind": "text", "seed": 900 + k % 5, "length": n}, "size": size,
                                  "seed": 40 + k})
                    k += 1
    return specs


def record_of(spec, d):
    """a record that shares vocabulary with its dictionary: it opens with the dictionary's last bytes (so that a
    raw stream cannot do without them), then text of the dictionary's generator interleaved with pieces of it"""
    rnd = db.Lcg(spec["seed"])
    fresh = corpus.make_buffer(spec["dict"]["kind"], spec["size"], spec["seed"])
    out = bytearray(d[-min(len(d), 40):])
    at = 0
    while len(out) < spec["size"]:
        if len(d) >= 16 and rnd.chance(50):
            n = rnd.between(8, min(len(d), 120) + 1)
            a = rnd.below(len(d) - n + 1)
            out += d[a:a + n]
        else:
            n = rnd.between(8, 200)
            out += fresh[at:at + n]
            at += n
    return bytes(out[:max(spec["size"], 1)])


def recorded():
    g = json.load(open(GOLDEN))
    cases = []
    for k, c in enumerate(g["streams"]):
        d = make_dict(c["dict"]["kind"], c["dict"]["seed"], c["dict"]["length"])
        s = bytes.fromhex(c["hex"])
        o = zlib.decompressobj(c["wbits"], zdict=d)
        out = o.decompress(s)
        assert o.eof and not o.unused_data and hashlib.sha256(out).hexdigest() == c["sha256"], c["name"]
        cases.append(Case(c["name"], s, c["wbits"], len(out) + 7 * (k % 3), d, Z_OK, out, len(s)))
    return cases


# ---- hand-built streams ----

def _lits(rnd, n):
    return [rnd.between(97, 123) for _ in range(n)]


def _fixed(tokens, good=None):
    """one final fixed block; good: the number of leading tokens that decode (the next one is the error)"""
    s = db.Stream()
    s.fixed(tokens, 1)
    return s.bytes(), (tokens if good is None else tokens[:good])


def _dynamic_block(s, tokens, last):
    lit = db.complete_lengths(286, first=sorted(db.literal_length_symbols(tokens)))
    dist = db.complete_lengths(30, first=sorted(db.distance_symbols(tokens)))
    s.dynamic(lit, dist, tokens, last)


def handbuilt():
    rnd = db.Lcg(2024)
    d1000 = make_dict("text", 77, 1000)
    d32k = make_dict("text", 78, 32768)
    d512 = make_dict("text", 79, 512)
    d513 = make_dict("text", 80, 513)
    d40000 = make_dict("text", 81, 40000)
    d2000 = make_dict("text", 82, 2000)
    d51200 = make_dict("text", 83, 51200)
    cases = []

    def add(name, raw, tokens_done, wbits, d, bad=False, blocks_out=None, form="raw", cinfo=7, cap=None,
            status=None, adler=None, dict_id=None, assigned="own"):
        """raw: the deflate data; tokens_done: the tokens that decode (for play()), or blocks_out: the output
        itself; form: raw, zlib (with FDICT), zlib-plain (no FDICT) or gzip; assigned: own, none (ZSC_HIP_NO_DICT)
        or another dictionary (bytes)"""
        applies = form in ("raw", "zlib")
        bits = -wbits if wbits < 0 else (wbits & 15) or 8 + cinfo  # (the plan's, or the header's where it has none)
        hist = window_part(d, bits) if applies else b""
        out = db.play(tokens_done, history=hist) if blocks_out is None else blocks_out
        if form == "raw":
            s = raw
        elif form == "zlib":
            s = zlib_dict_wrap(raw, out, db.adler32(d) if dict_id is None else dict_id, cinfo, adler)
        elif form == "zlib-plain":
            s = zlib_header(cinfo, False) + raw + struct.pack(">I", db.adler32(out))
        else:
            s = db.wrap(raw, out, 31)
        if bad:
            s += TAIL
        given = d if assigned == "own" else None if assigned == "none" else assigned
        if status is None:
            status = Z_DATA_ERROR if bad else Z_OK
        if status == Z_NEED_DICT or (status == Z_DATA_ERROR and not bad):
            want = (status, b"", 0)  # (no dictionary, or one that is refused)
        else:
            want = (status, out, len(s))
        cases.append(Case(name, s, wbits, (len(out) if cap is None else cap) + (300 if bad else 0), given, *want))

    # a match as the very first token: distance 1, have, and have + 1
    for wrapname, form, wb in (("raw", "raw", -15), ("zlib", "zlib", 15)):
        for dname, d in (("d1000", d1000), ("d32k", d32k)):
            have = len(d)
            raw, done = _fixed([(5, 1), 120, (258, have), 121])
            add(f"first-{wrapname}-{dname}", raw, done, wb, d, form=form)
            if have < 32768:
                raw, done = _fixed([(5, 1), (7, have + 6)], good=1)
                add(f"first-toofar-{wrapname}-{dname}", raw, done, wb, d, bad=True, form=form)
        raw, done = _fixed([(4, 1001)], good=0)
        add(f"first-only-toofar-{wrapname}", raw, done, wb, d1000, bad=True, form=form)
    # the source runs out of the dictionary into the output, and wraps back into the dictionary
    raw, done = _fixed(_lits(rnd, 100) + [(50, 110), 65])
    add("runs-into-output", raw, done, -15, d1000)
    raw, done = _fixed([97, 98, 99, (258, 5), 100, (258, 5), (3, 300)])
    add("wraps-into-dict", raw, done, -15, d1000)
    raw, done = _fixed([97, (258, 2), (258, 3), (17, 260)])
    add("wraps-into-dict-z", raw, done, 15, d32k, form="zlib")
    # reaches from behind the LDS ring, and the longest distance from position 1
    raw, done = _fixed(_lits(rnd, 600) + [(258, 900), (100, 32768), 66] + _lits(rnd, 30) + [(258, 1200)])
    add("reach-past-ring", raw, done, -15, d32k)
    raw, done = _fixed([97, (258, 32768), (258, 32768), 98])
    add("pos1-dist32768", raw, done, -15, d32k)
    raw, done = _fixed([97, (258, 32768), 98])
    add("pos1-dist32768-z", raw, done, 15, d51200, form="zlib")
    raw, done = _fixed([97, 98, (4, 32769 - 30000)] + [(258, 32768)] * 3 + [(3, 32768), (9, 4000)])
    add("far-sources-only", raw, done, -15, d51200)
    # a dictionary longer than the window: byte 513 back is no longer there
    for dname, d in (("d513", d513), ("d40000", d40000)):
        raw, done = _fixed([(258, 512), 97, (258, 513), (30, 1)])
        add(f"window9-{dname}", raw, done, -9, d)
        raw, done = _fixed([(5, 513)], good=0)
        add(f"window9-toofar-{dname}", raw, done, -9, d, bad=True)
        raw, done = _fixed([98, (5, 513), (5, 519)], good=2)
        add(f"window9-toofar1-{dname}", raw, done, -9, d, bad=True)
    raw, done = _fixed([(258, 512), 97, (258, 512)])
    add("window9-zlib-d40000", raw, done, 9, d40000, form="zlib", cinfo=1)
    # a distance beyond the header's window (DISTEXT), in a plan that allows the largest
    raw, done = _fixed([(5, 512), (5, 512), 97])
    add("dmax-header9-ok", raw, done, 15, d2000, form="zlib", cinfo=1)
    raw, done = _fixed([(5, 512), (5, 513), 97], good=1)
    add("dmax-header9", raw, done, 15, d2000, bad=True, form="zlib", cinfo=1)
    raw, done = _fixed([(5, 600)], good=0)
    add("dmax-header9-first", raw, done, 0, d2000, bad=True, form="zlib", cinfo=1)
    # raw: the limit is 32768 whatever the window: 600 back from 100 is 500 bytes into a 512-byte dictionary
    raw, done = _fixed(_lits(rnd, 100) + [(20, 600), (258, 612 + 20)])
    add("raw9-dist600", raw, done, -9, d512)
    raw, done = _fixed(_lits(rnd, 100) + [(20, 613)], good=100)
    add("raw9-dist613", raw, done, -9, d512, bad=True)
    # FDICT with an empty dictionary (id 00000001)
    raw, done = _fixed([104, 105, (40, 2)])
    add("empty-dict", raw, done, 15, b"", form="zlib")
    raw, done = _fixed([(3, 1)], good=0)
    add("empty-dict-reach", raw, done, 15, b"", bad=True, form="zlib")
    raw, done = _fixed([104, 105, (40, 2)])
    add("empty-dict-raw", raw, done, -15, b"")
    # the check value covers the output alone
    raw, done = _fixed([(100, 1000), 97])
    out = db.play(done, history=d1000)
    add("adler-with-dict", raw, done, 15, d1000, bad=True, form="zlib", adler=db.adler32(d1000 + out))
    add("adler-alone", raw, done, 15, d1000, form="zlib")
    # identification: no dictionary, another one, the whole of a long one
    raw, done = _fixed([(100, 1000), 97])
    add("need-dict", raw, done, 15, d1000, form="zlib", status=Z_NEED_DICT, assigned="none")
    add("need-dict-auto", raw, done, 47, d1000, form="zlib", status=Z_NEED_DICT, assigned="none")
    add("wrong-dict", raw, done, 15, d1000, form="zlib", status=Z_DATA_ERROR, assigned=d2000)
    add("wrong-dict-part", raw, done, 15, d1000, form="zlib", status=Z_DATA_ERROR, assigned=d1000[1:])
    add("auto-zlib", raw, done, 47, d1000, form="zlib")
    raw, done = _fixed([(100, 32768), 97])
    add("id-of-the-whole", raw, done, 15, d51200, form="zlib")
    add("id-of-the-window-only", raw, done, 15, d51200, form="zlib", status=Z_DATA_ERROR,
        dict_id=db.adler32(d51200[-32768:]))
    # streams that never look at their dictionary: zlib without FDICT, gzip, and a reach past the start there
    raw, done = _fixed([104, 105, (40, 2)])
    add("nofdict-ignored", raw, done, 15, d1000, form="zlib-plain")
    add("gzip-ignored", raw, done, 31, d1000, form="gzip")
    add("auto-gzip-ignored", raw, done, 47, d1000, form="gzip")
    raw, done = _fixed([104, (3, 2)], good=1)
    add("nofdict-reach", raw, done, 15, d1000, bad=True, form="zlib-plain")
    add("gzip-reach", raw, done, 31, d1000, bad=True, form="gzip")
    add("raw-nodict-reach", raw, done, -15, d1000, bad=True, assigned="none")
    # stored, fixed and dynamic blocks each carrying a reach
    s = db.Stream()
    s.stored(b"abc", 0)
    t1 = [(10, 3 + 7), 120]
    s.fixed(t1, 0)
    t2 = _lits(rnd, 40) + [(258, 54 + 500), (33, 1000 + 54 + 258 + 33 - 1 - 33), 121, (3, 1)]
    _dynamic_block(s, t2, 0)
    s.stored(b"xyz" * 50, 0)
    t3 = [(100, 1000 + 54 + 258 + 33 + 2 + 3 + 150 - 700)]
    s.fixed(t3, 1)
    out = db.play(t1, history=d1000 + b"abc")
    out = b"abc" + out
    out += db.play(t2, history=d1000 + out)
    out += b"xyz" * 50
    out += db.play(t3, history=d1000 + out)
    add("all-block-types", s.bytes(), None, -15, d1000, blocks_out=out)
    add("all-block-types-z", s.bytes(), None, 15, d1000, blocks_out=out, form="zlib")
    s = db.Stream()
    t4 = [(258, 1000), 97, (258, 1000), (4, 1000 + 517)]
    _dynamic_block(s, t4, 1)
    add("dynamic-first", s.bytes(), t4, -15, d1000)
    s = db.Stream()
    s.stored(b"", 0)
    s.stored(b"q" * 700, 0)
    s.fixed([(258, 1700)], 1)
    add("stored-then-reach", s.bytes(), None, -15, d1000,
        blocks_out=b"q" * 700 + db.play([(258, 1700)], history=d1000 + b"q" * 700))
    names = [c.name for c in cases]
    assert len(names) == len(set(names))
    return cases


def all_cases():
    return recorded() + handbuilt()


# ---- the stored-prefix equivalence ----

def stored_prefix(t):
    """a non-final stored block holding t (at most 65535 bytes): five bytes of header, then t"""
    assert len(t) <= 65535
    return b"\x00" + struct.pack("<HH", len(t), len(t) ^ 0xFFFF) + t
