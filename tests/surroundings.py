"""Helpers of the surroundings tests (no tests here): a plan's results depend only on its own bytes.

The contract (include/zsc_hip.h, "What a run reads, writes and remembers"): a run reads an item's bytes and,
behind them, at the most the 64 readable bytes every device input has; it writes nothing outside the items'
slots [offset, + capacity); and it does not depend on earlier runs of the plan.  The other GPU tests put
zeros around every item, decode into fresh or cleared memory and run a plan again only on what it has just
seen, so none of that could fail there.  Here

* place() builds a device input with a chosen FILLER in every byte that belongs to no item: "zeros" (the
  control), "ones" (0xFF), "noise" (seeded) and "continuation" (noise, and per item the bytes its case supplies
  to lie directly behind it and, where wanted, before it -- the truth a truncated stream was cut from, the
  next piece of a buffer that was cut into pieces);
* canary_image() fills an output with a canary and assert_outside_untouched() asserts that no byte outside
  the union of the slots changed -- every gap, and the 64 bytes behind the last slot.  Nothing is ever
  asserted about the bytes in [offset + out_len, offset + capacity): the serial fallbacks may have written
  there before the parallel path's result was taken or given up, and the contract leaves those bytes open;
* under_fillers() runs one case list under the control and under the hostile fillers and compares every
  result with the oracle's.  A case that fails under the control too is a wrong case (or a plain bug);
  a case that fails under a hostile filler only was reached by its surroundings.  The message says which.

Expected values never come from the code under test: oracle.uncompress() on exactly the item's bytes,
oracle.compress() on exactly the piece, and for a members plan the walk of tests/test_inflate_members_emu.py.
The case lists are built here as well, so that tests/test_surroundings_cases.py can check them against the
oracle alone, with no GPU.
"""
import collections
import zlib

import numpy as np

import deflate_cases as dc
from zsc_amd import corpus

FILLERS = ("zeros", "ones", "noise", "continuation")
HOSTILE = FILLERS[1:]
CANARY = 0xEE
CHUNK = 4096  # the least chunk_bytes of a chunks, size or check plan
GZ = 31
WRAPPERS = (15, 31, -15)
INFLATE_KINDS = ("plain", "sections", "chunks", "resync", "indexed", "size", "check")
Z_OK, Z_DATA_ERROR, Z_BUF_ERROR = 0, -3, -5
TAIL = 64  # readable bytes behind the last item of an input, and the bytes looked at behind the last slot

# one item of an inflate batch: the plan is told len(data); `behind` lies directly behind the data (and
# `before` directly before it) under the "continuation" filler; what names the class of the case
Item = collections.namedtuple("Item", "name data cap behind before what")
Item.__new__.__defaults__ = (b"", b"", "clean")


def round16(n):
    return (n + 15) & ~15


# ---- images ------------------------------------------------------------------------------------------------

def spread_offsets(items, room=TAIL):
    """offsets (multiples of 16) that leave every item at least `room` bytes, and room for what it wants
    behind and before it; -> (offsets, image bytes)"""
    offs, at = [], 0
    for it in items:
        at += round16(len(it.before))
        offs.append(at)
        at += round16(len(it.data) + max(room, len(it.behind) + 16))
    return offs, at + TAIL


def place(items, offsets, nbytes, filler, seed=1):
    """the host image (numpy uint8) of a batch: every item's data at its offset, `filler` everywhere else"""
    assert filler in FILLERS, filler
    if filler == "zeros":
        img = np.zeros(nbytes, dtype=np.uint8)
    elif filler == "ones":
        img = np.full(nbytes, 0xFF, dtype=np.uint8)
    else:
        img = np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)
    ends = [o + len(it.data) for it, o in zip(items, offsets)]
    order = sorted(range(len(items)), key=lambda i: offsets[i])
    for a, b in zip(order, order[1:]):
        assert ends[a] <= offsets[b], "items overlap"
    assert not items or max(ends) + TAIL <= nbytes, "64 readable bytes must follow the last item"
    if filler == "continuation":
        for pos, i in enumerate(order):  # what lies before an item ends at its offset
            lo = ends[order[pos - 1]] if pos else 0
            b = items[i].before[-(offsets[i] - lo):] if offsets[i] > lo else b""
            img[offsets[i] - len(b):offsets[i]] = np.frombuffer(b, dtype=np.uint8)
        for pos, i in enumerate(order):  # what lies behind it starts at its end (and wins over a `before`)
            hi = offsets[order[pos + 1]] if pos + 1 < len(order) else nbytes
            b = items[i].behind[:hi - ends[i]]
            img[ends[i]:ends[i] + len(b)] = np.frombuffer(b, dtype=np.uint8)
    for it, o in zip(items, offsets):
        img[o:o + len(it.data)] = np.frombuffer(it.data, dtype=np.uint8)
    return img


def canary_image(torch, nbytes, canary=CANARY):
    """a device output full of the canary (an output an earlier run left is used as it is, with its host
    copy as the `canary` of assert_outside_untouched)"""
    return torch.full((nbytes,), canary, dtype=torch.uint8, device="cuda")


def outside_changed(image, offsets, caps, canary):
    """None, or a sentence about the first byte outside the union of [off, off + cap) that differs from the
    canary (an int, or an array: the image as it was before the run)"""
    image = np.asarray(image)
    outside = np.ones(len(image), dtype=bool)
    for off, cap in zip(offsets, caps):
        outside[off:off + cap] = False
    was = np.full(len(image), canary, dtype=np.uint8) if np.isscalar(canary) else np.asarray(canary)
    bad = np.flatnonzero(outside & (image != was))
    if not len(bad):
        return None
    at = int(bad[0])
    owner = max([i for i, off in enumerate(offsets) if off <= at], key=lambda i: offsets[i], default=None)
    where = "in front of the first slot" if owner is None else \
        f"{at - offsets[owner] - caps[owner]} bytes behind the end of slot {owner} (cap {caps[owner]})"
    return f"{len(bad)} bytes outside the slots were written, the first at {at}, {where}: {int(image[at]):#x}"


def assert_outside_untouched(image, offsets, caps, canary=CANARY):
    """no byte outside the union of the slots changed: every gap, and the bytes behind the last slot (the
    image is laid out with at least 64 of them).  Bytes in [off + out_len, off + cap) are not looked at."""
    assert len(image) >= max([o + c for o, c in zip(offsets, caps)], default=0) + TAIL
    msg = outside_changed(image, offsets, caps, canary)
    assert msg is None, msg


def under_fillers(names, wants, run, fillers=FILLERS):
    """run(filler) -> one result per case, comparable with wants, and after them any number of sentences
    about bytes written outside the slots.  Runs the control first and then the hostile fillers; asserts
    that everything equals the oracle's, and says whether a case is wrong or its surroundings leaked in."""
    assert fillers[0] == "zeros"
    failed = {}
    for filler in fillers:
        got = run(filler)
        assert len(got) >= len(wants)
        for name, g, w in zip(names, got, wants):
            if g != w:
                failed.setdefault(name, []).append((filler, brief(g), brief(w)))
        for extra in got[len(wants):]:
            if extra is not None:
                failed.setdefault("<outside the slots>", []).append((filler, extra, None))
    lines = []
    for name, fails in failed.items():
        if fails[0][0] == "zeros":
            lines.append(f"{name}: wrong with zeros around it as well (the case or the code, not the "
                         f"surroundings): got {fails[0][1]}, the oracle {fails[0][2]}")
        else:
            lines.append(f"{name}: right with zeros around it, wrong under {[f[0] for f in fails]}: the "
                         f"surroundings leaked in: got {fails[0][1]}, the oracle {fails[0][2]}")
    assert not lines, "\n".join(lines)


def brief(r):
    if isinstance(r, (bytes, bytearray)):
        return f"<{len(r)} bytes, adler {zlib.adler32(r):#x}>"
    if isinstance(r, (tuple, list)):
        return tuple(brief(x) for x in r)
    return r


# ---- inflate: plans and results ----------------------------------------------------------------------------

def make_inflate_plan(kind, lens, caps, wbits, src_offsets, blobs=None):
    import zsc_amd
    kw = dict(window_bits=wbits, src_offsets=src_offsets)
    if kind == "plain":
        return zsc_amd.InflatePlan(lens, caps, **kw)
    if kind == "sections":
        return zsc_amd.InflatePlan(lens, caps, sections=True, **kw)
    if kind == "resync":
        return zsc_amd.InflatePlan(lens, caps, resync=True, **kw)
    if kind == "chunks":
        return zsc_amd.InflatePlan(lens, caps, chunks=True, chunk_bytes=CHUNK, **kw)
    if kind == "indexed":
        return zsc_amd.InflatePlan(lens, caps, indexes=blobs, **kw)
    if kind == "members":
        return zsc_amd.InflatePlan(lens, caps, members=True, **kw)
    assert kind in ("size", "check"), kind
    return zsc_amd.InflatePlan(lens, caps, size_only=kind == "size", check_only=kind == "check", chunk_bytes=CHUNK, **kw)


def writes(kind):
    return kind not in ("size", "check")


def build_blobs(torch, items, wbits):
    """the seek-point indexes of the items' exact bytes, from a chunks plan that keeps them (None for a
    stream the serial decoder produced).  They are an input of the indexed plan, not an expectation."""
    import zsc_amd
    offs, nbytes = spread_offsets(items)
    plan = zsc_amd.InflatePlan([len(it.data) for it in items], [it.cap for it in items], window_bits=wbits, chunks=True,
                               chunk_bytes=CHUNK, keep_index=True, src_offsets=offs)
    try:
        src = torch.from_numpy(place(items, offs, nbytes, "zeros")).cuda()
        dst = torch.zeros(plan.dst_bytes, dtype=torch.uint8, device="cuda")
        plan.run(src.data_ptr(), dst.data_ptr())
        plan.results()
        return [plan.export_index(i) for i in range(len(items))]
    finally:
        plan.close()


def read_inflate(plan, kind, host):
    """[(status, output bytes -- their count for a plan that writes none --, consumed)] after a run"""
    lens, used, stat, _ = plan.results()
    if not writes(kind):
        return [(st, n, u) for st, n, u in zip(stat, lens, used)]
    out = []
    for off, n, cap, u, st in zip(plan.dst_offsets, lens, plan_caps(plan), used, stat):
        assert n <= cap, "more bytes reported than the slot has"
        out.append((st, host[off:off + n].tobytes(), u))
    return out


def plan_caps(plan):
    return plan._surroundings_caps


def run_inflate(torch, kind, items, wbits, filler, blobs=None, seed=1):
    """one plan of `kind` over the items, the input under `filler`, the output full of the canary:
    -> per item (status, bytes or count, consumed) (+ (members,) for a members plan), then the check
    values where the plan has any, then what outside_changed() says"""
    offs, nbytes = spread_offsets(items)
    caps = [it.cap for it in items]
    plan = make_inflate_plan(kind, [len(it.data) for it in items], caps, wbits, offs, blobs)
    plan._surroundings_caps = caps
    try:
        src = torch.from_numpy(place(items, offs, nbytes, filler, seed)).cuda()
        dst = canary_image(torch, plan.dst_bytes) if writes(kind) else None
        torch.cuda.synchronize()
        plan.run(src.data_ptr(), dst.data_ptr() if dst is not None else 0)
        host = dst.cpu().numpy() if dst is not None else None
        res = read_inflate(plan, kind, host)
        if kind == "members":
            res = [r + (m,) for r, m in zip(res, plan.members()[0])]
        extra = []
        if kind == "check":
            res = [r + (v,) for r, v in zip(res, plan.check_values())]
        if host is not None:
            extra.append(outside_changed(host, plan.dst_offsets, caps, CANARY))
        return res + extra
    finally:
        plan.close()


def want_inflate(oracle, kind, item, wbits):
    """what the oracle says about exactly the item's bytes, in the shape run_inflate() reports"""
    if kind == "members":
        from test_inflate_members_emu import walk
        rc, out, used, members = walk(oracle, item.data, item.cap)
        return rc, out, used, members
    if kind == "size":
        # the oracle's, with the one exception of a size plan's contract built in: it does not compare the
        # check value, so a stream whose deflate data is sound is judged with the right value in its trailer
        from test_inflate_size_emu import expect
        return expect(oracle, item.data, item.cap, wbits)[0]
    rc, out, used = oracle.uncompress(item.data, item.cap, window_bits=wbits)
    if kind == "check":
        value = 0 if rc != Z_OK else oracle.crc32(out) if wbits > 15 else oracle.adler32(out)
        return rc, len(out), used, value
    return rc, out, used


# ---- inflate: the cases ------------------------------------------------------------------------------------

_memo = {}


def _comp(oracle, data, level, wbits, **kw):
    rc, s, _ = oracle.compress(data, level, window_bits=wbits, **kw)
    assert rc == 0
    return s


def _length_symbol(n):
    return 285 if n == 258 else max(s for s in range(257, 285) if dc.LEN_BASE[s - 257] <= n)


def code_cuts(stream, wbits):
    """the places of a one-block stream where a byte boundary falls inside a literal's code ({k % 4: k})
    and exactly between a length code (with its extra bits) and its distance code ([k])"""
    tokens = []
    blocks, _, _ = dc.walk(stream, wbits, tokens)
    assert len(blocks) == 1 and blocks[0].type == 2
    b = blocks[0]
    inside, between = {}, []
    for (_, n, dist), p, nb in zip(tokens, b.sym_pos, b.sym_bits):
        if dist == 0:
            k = (p >> 3) + 1
            if 8 * k < p + nb:  # the code goes on behind byte k - 1
                inside.setdefault(k % 4, k)
        else:
            s = _length_symbol(n)
            q = p + b.lit_lens[s] + dc.LEN_EXTRA[s - 257]
            if q % 8 == 0 and q < p + nb:
                between.append(q >> 3)
    return inside, between


def truncated(name, stream, k, cap, what):
    """the first k bytes of the stream, with what they were cut from directly behind them"""
    assert 0 < k < len(stream)
    return Item(name, stream[:k], cap, stream[k:k + 4096], b"", what)


def inflate_cases(oracle, wbits):
    """[Item] of one wrapper; built once and not changed by anyone"""
    key = ("inflate", id(oracle), wbits)
    if key in _memo:
        return _memo[key]
    items = []
    hdr = dc.body_offset(_comp(oracle, b"x", 6, wbits), wbits)
    trl = {15: 4, GZ: 8, -15: 0}[wbits]

    # ---- clean streams: outputs of 0, 1, 300 and a few thousand bytes; len(stream) % 4 takes every value
    for n, data in ((0, b""), (1, b"z"), (300, bytes(range(100)) * 3)):
        items.append(Item(f"clean-{n}", _comp(oracle, data, 6, wbits), n))
    seen, n = set(), 3000
    while len(seen) < 4:
        data = corpus.make_buffer("text", n, 11)
        s = _comp(oracle, data, 6, wbits)
        if len(s) % 4 not in seen:
            seen.add(len(s) % 4)
            items.append(Item(f"clean-text-{n}-mod{len(s) % 4}", s, n))
        n += 7
        assert n < 4000
    # incompressible bytes with a full flush in their middle: a little more than three chunks
    noise = np.random.default_rng(77).integers(0, 256, 12400, dtype=np.uint8).tobytes()
    co = zlib.compressobj(6, zlib.DEFLATED, wbits)
    big = co.compress(noise[:6200]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(noise[6200:]) + co.flush()
    assert 3 * CHUNK < len(big) < 3 * CHUNK + 256 and big.count(b"\x00\x00\xff\xff") >= 1
    items.append(Item("clean-noise-three-chunks", big, len(noise)))

    # ---- truncated streams with the truth behind them
    text = corpus.make_buffer("text", 3000, 5)
    t = _comp(oracle, text, 6, wbits)
    if hdr:
        items.append(truncated("cut-in-header", t, hdr // 2, len(text), "header"))
    inside, between = code_cuts(t, wbits)
    for r in sorted(inside):
        items.append(truncated(f"cut-inside-literal-code-mod{r}", t, inside[r], len(text), "inside-code"))
    assert between, "no length code ends on a byte boundary"
    items.append(truncated("cut-between-length-and-distance", t, between[len(between) // 2], len(text), "length-distance"))
    stored = _comp(oracle, bytes(range(256)) + text[:44], 0, wbits)
    items.append(truncated("cut-in-stored-data", stored, hdr + 5 + 100, 300, "stored"))
    for short in range(1, 4) if trl else ():
        items.append(truncated(f"cut-trailer-{short}-short", t, len(t) - short, len(text), f"trailer-{short}"))

    damaged = bytearray(t)
    damaged[len(t) // 2] ^= 0x40
    items.append(Item("damaged-in-the-middle", bytes(damaged), len(text), what="damaged"))

    # ---- markers, headers and members behind the cut
    flushed_text = corpus.make_buffer("text", 9000, 6)
    f = _comp(oracle, flushed_text, 6, wbits, max_block_len=1024)
    marks = [i for i in range(len(f) - 4) if f[i:i + 4] == b"\x00\x00\xff\xff"]
    assert len(marks) >= 3
    items.append(truncated("cut-before-flush-marker", f, marks[1], len(flushed_text), "marker"))
    if wbits == GZ:
        m0, m1 = _comp(oracle, text[:700], 6, GZ), _comp(oracle, text[700:], 9, GZ)
        for into in range(4):
            items.append(truncated(f"cut-{into}-into-next-member", m0 + m1, len(m0) + into, len(text), f"member-{into}"))
    # more than three chunks of many small dynamic blocks (mem_level 3), cut in the last chunk with a
    # block header right behind the cut
    for n in range(18000, 60000, 500):
        long_text = corpus.make_buffer("text", n, 8)
        s = _comp(oracle, long_text, 6, wbits, mem_level=3)
        if len(s) > 3 * CHUNK + 300:
            break
    assert 3 * CHUNK + 300 < len(s) < 3 * CHUNK + 1024, len(s)
    blocks, _, _ = dc.walk(s, wbits)
    last = [b for b in blocks if b.type == 2 and (b.first_bit >> 3) > 3 * CHUNK + 16]
    assert last, "no dynamic block starts in the last chunk"
    items.append(Item("clean-many-blocks-three-chunks", s, n))
    items.append(truncated("cut-before-dynamic-header-in-last-chunk", s, last[0].first_bit >> 3, n, "block-header"))

    # ---- short destination capacities
    items.append(Item("cap-one-short", t, len(text) - 1, what="cap"))
    items.append(Item("cap-half", t, len(text) // 2, what="cap"))
    items.append(Item("cap-half-noise", big, len(noise) // 2, what="cap"))
    _memo[key] = items
    return items


def member_cases(oracle):
    """[Item] for a members plan: gzip files of its own case set, and files cut with the truth behind the cut"""
    key = ("members", id(oracle))
    if key in _memo:
        return _memo[key]
    from test_inflate_members_emu import make_member_cases
    by = {c.name: c for c in make_member_cases(oracle)}
    items = [Item(n, by[n].data, by[n].cap) for n in
             ("clean-5-l6", "clean-2-l0", "clean-300-empty", "bgzf-3", "clean-flushed-middle", "zero-pad-7", "trailing-1f",
              "flip-crc", "damaged-flushed-then-more", "cap-inside-member-2", "cap-one-short", "lie-bsize-small")]
    text = corpus.make_buffer("text", 5000, 9)
    ms = [_comp(oracle, text[a:b], lv, GZ) for a, b, lv in ((0, 700, 6), (700, 701, 1), (701, 3000, 9), (3000, 5000, 6))]
    f = b"".join(ms)
    first = len(ms[0])
    for into in range(4):
        items.append(truncated(f"cut-{into}-into-member-1", f, first + into, len(text), f"member-{into}"))
    third = first + len(ms[1])
    items.append(truncated("cut-in-member-2-header", f, third + 5, len(text), "header"))
    items.append(truncated("cut-in-member-2-body", f, third + len(ms[2]) // 2, len(text), "body"))
    for short in (1, 2, 3, 5):
        items.append(truncated(f"cut-last-trailer-{short}-short", f, len(f) - short, len(text), f"trailer-{short}"))
    items.append(Item("cap-half", f, len(text) // 2, what="cap"))
    _memo[key] = items
    return items


# ---- deflate: one long buffer cut into pieces ---------------------------------------------------------------

LONG = 120000
PIECES_16 = (16, 48, 272, 3072, 3088, 32768 + 16, 40000)      # and the rest; all multiples of 16
PIECES_ODD = (17, 47, 271, 3071, 3073, 32768 + 13, 40002, 5)  # and the rest
DEFLATE_PLANS = [(1, 15, 0), (3, 15, 0), (4, 15, 0), (6, 15, 0), (9, 15, 0), (6, -15, 0), (6, 31, 0), (6, 9, 0),
                 (6, 15, 2), (6, 15, 3)]  # (level, window_bits, strategy): 2 Z_HUFFMAN_ONLY, 3 Z_RLE


def long_buffer():
    """about 120 KB: text, a period-7 run, zeros, text again -- and the 64 bytes that lie behind it"""
    if "long" not in _memo:
        a = corpus.make_buffer("text", 50000, 21)
        run = (b"abcdefg" * 1500)[:10000]
        b = corpus.make_buffer("text", 40000 + TAIL, 22)
        _memo["long"] = a + run + bytes(20000) + b
        assert len(_memo["long"]) == LONG + TAIL
    return _memo["long"]


def pieces(lengths):
    """consecutive pieces of the long buffer as Items: each with its true continuation behind it and its
    true past before it.  -> the items; the last one ends where the long buffer's 120 000 bytes end"""
    buf = long_buffer()
    lens = list(lengths) + [LONG - sum(lengths)]
    assert lens[-1] > 0
    items, at = [], 0
    for n in lens:
        items.append(Item(f"piece-{n}-at-{at}", buf[at:at + n], 0, buf[at + n:at + n + TAIL], buf[max(0, at - TAIL):at],
                          "piece"))
        at += n
    return items


def want_deflate(oracle, items, level, wbits, strategy, **kw):
    key = ("deflate", id(oracle), tuple(it.name for it in items), level, wbits, strategy, tuple(sorted(kw.items())))
    if key not in _memo:
        got = [oracle.compress(it.data, level, window_bits=wbits, strategy=strategy, **kw) for it in items]
        assert all(rc == 0 and not unsupported for rc, _, unsupported in got)
        _memo[key] = [s for _, s, _ in got]
    return _memo[key]


def make_deflate_plan(lens, level, wbits, strategy, in_offsets=None, out_caps=None):
    """a zsc_amd.DeflatePlan; with in_offsets, one whose buffers lie where the caller says (the C interface
    takes any multiples of 16; the class itself only offers the layout's own)"""
    import ctypes as C
    import zsc_amd
    plan = zsc_amd.DeflatePlan(lens, level, wbits, 8, strategy, out_caps=out_caps)
    if in_offsets is None:
        return plan
    n = len(lens)
    caps, out_off = plan.out_caps, plan.out_offsets
    plan.close()
    rc = zsc_amd.lib.zsc_hip_deflate_plan_create(C.byref(plan._h), n, (C.c_uint32 * n)(*lens), (C.c_uint64 * n)(*in_offsets),
                                                 (C.c_uint64 * n)(*out_off), (C.c_uint32 * n)(*caps), level, wbits, 8, strategy)
    assert rc == 0, rc
    plan.in_offsets = list(in_offsets)
    plan.in_bytes = max(o + l for o, l in zip(in_offsets, lens)) + TAIL
    return plan


def run_deflate(torch, plan, image, canary=0xFF, verify=False):
    """one run of the plan on the host image, the output full of the canary: -> per buffer (status, stream
    -- b"" where the status is not Z_OK: nothing is said about the inside of such a slot), then what
    outside_changed() says, then (verify=True) the verdicts of verify() that are not VERIFY_OK"""
    import zsc_amd
    if verify:
        plan.verify_enable()
    src = torch.from_numpy(image).cuda()
    dst = canary_image(torch, plan.out_bytes, canary)
    torch.cuda.synchronize()
    plan.run(src.data_ptr(), dst.data_ptr())
    lens, stat = plan.results()
    host = dst.cpu().numpy()
    res = []
    for off, n, cap, st in zip(plan.out_offsets, lens, plan.out_caps, stat):
        assert st != Z_OK or n <= cap
        res.append((st, host[off:off + n].tobytes() if st == Z_OK else b""))
    extra = [outside_changed(host, plan.out_offsets, plan.out_caps, canary)]
    if verify:
        assert plan.verify(src.data_ptr(), dst.data_ptr()) == 0
        bad = [(i, v) for i, v in enumerate(plan.verify_results()) if v["verdict"] != zsc_amd.VERIFY_OK]
        extra.append(f"verify() does not call every stream intact: {bad}" if bad else None)
    return res + extra
