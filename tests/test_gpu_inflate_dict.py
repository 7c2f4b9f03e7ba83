"""Plans with zlib preset dictionaries on the GPU (zsc_hip_inflate_plan_dict_enable, k_inflate_dict), through
the C ABI as zsc_amd binds it.

  1. every recorded and hand-built case of tests/inflate_dict_cases.py, each stream with its own dictionary, in
     one plan per window_bits (a plan has one): in the library's order, and in a decode_order that puts four
     different dictionaries, and a mix of dictionary and ZSC_HIP_NO_DICT, into the first wavefronts;
  2. the statuses of identification: no dictionary, a wrong one, one that is ignored, the id of a long one;
  3. the stored-prefix equivalence: for a raw stream S and the part T of its dictionary that the window holds,
     the dictionary plan on S and the PLAIN plan on stored_block(T) + S (dest_cap raised by len(T)) give the same
     status, out_len - len(T), consumed - 5 - len(T) and bytes behind T -- for every truncation, for dest_cap at
     the size, one less and 0, and for single byte flips in front of a full-flush marker.  Nothing in this
     comparison knows what the right answer is: the plain decoder's handling of earlier output is the reference
     for the dictionary decoder's handling of the dictionary, errors and resynchronisation included;
  4. dict_enable a second time replaces the set; other device buffers give the same results; pack_enable works;
  5. dict_enable is Z_STREAM_ERROR for every other plan kind and for an index out of range, and the plan runs on
     as before;
  6. zsc_hip_uncompress_dict_batch and zsc_amd.uncompress_dict_batch.
"""
import ctypes as C
import zlib

import numpy as np
import pytest

import deflate_builder as db
import inflate_dict_cases as idc

pytestmark = pytest.mark.gpu

NO_DICT = 0xFFFFFFFF
Z_STREAM_ERROR = -2
FILL = 0xA5


def run_plan(plan, streams, want_errors=False):
    """one run of `plan` on these streams, in fresh device buffers: [(status, out, consumed)]; every byte of
    the output image outside the outputs must be untouched"""
    import torch
    src = np.zeros(plan.src_bytes, np.uint8)
    for s, off in zip(streams, plan.src_offsets):
        src[off:off + len(s)] = np.frombuffer(s, np.uint8)
    d_src = torch.from_numpy(src).cuda()
    d_dst = torch.full((plan.dst_bytes,), FILL, dtype=torch.uint8, device="cuda")
    plan.run(d_src.data_ptr(), d_dst.data_ptr())
    lens, used, stat, _ = plan.results()
    host = d_dst.cpu().numpy()
    res, mask = [], np.ones(len(host), bool)
    for off, n, u, st in zip(plan.dst_offsets, lens, used, stat):
        res.append((st, host[off:off + n].tobytes(), u))
        mask[off:off + n] = False
    assert (host[mask] == FILL).all(), "a byte outside the outputs was written"
    if want_errors:
        return res, plan.data_errors(), d_dst
    return res


def dict_table(cases):
    """the distinct dictionaries of the cases and every case's index"""
    dicts, index, of = [], {}, []
    for c in cases:
        if c.dict is None:
            of.append(NO_DICT)
            continue
        if c.dict not in index:
            index[c.dict] = len(dicts)
            dicts.append(c.dict)
        of.append(index[c.dict])
    return dicts, of


def mixed_order(of):
    """a decode_order whose first four streams have four different dictionaries and whose next four mix streams
    with and without one, as far as the batch has them; the others follow from the back"""
    first, seen = [], set()
    for i, d in enumerate(of):
        if d != NO_DICT and d not in seen and len(first) < 4:
            first.append(i)
            seen.add(d)
    none = [i for i, d in enumerate(of) if d == NO_DICT and i not in first][:2]
    some = [i for i, d in enumerate(of) if d != NO_DICT and i not in first][:4 - len(none)]
    second = [x for pair in zip(some, none) for x in pair] + some[len(none):] + none[len(some):]
    rest = [i for i in reversed(range(len(of))) if i not in first and i not in second]
    return first + second + rest


@pytest.fixture(scope="module")
def cases():
    return idc.all_cases()


def check(cases, res, what):
    for c, (st, out, used) in zip(cases, res):
        assert (st, len(out), used) == (c.status, len(c.out), c.consumed), (what, c.name)
        assert out == c.out, (what, c.name)


def test_every_case_with_its_own_dictionary(cases):
    import zsc_amd
    assert len(cases) % 4 != 0
    quads, mixes = 0, 0
    for wbits in sorted({c.wbits for c in cases}):
        group = [c for c in cases if c.wbits == wbits]
        dicts, of = dict_table(group)
        streams = [c.stream for c in group]
        order = mixed_order(of)
        quads += len({of[i] for i in order[:4]} - {NO_DICT}) == 4
        mixes += len(order) >= 8 and 0 < sum(of[i] == NO_DICT for i in order[4:8]) < 4
        for decode_order in (None, order):
            plan = zsc_amd.InflatePlan([len(s) for s in streams], [c.cap for c in group], wbits,
                                       decode_order=decode_order, dicts=dicts, stream_dict=of)
            try:
                assert plan.dict_ids() == [zlib.adler32(d) for d in dicts]
                check(group, run_plan(plan, streams), (wbits, decode_order is not None))
            finally:
                plan.close()
    assert quads >= 2 and mixes >= 2


def test_identification_statuses(cases):
    import zsc_amd
    by = {c.name: c for c in cases}
    # no dictionary assigned: Z_NEED_DICT, 0, 0 -- what a plain plan gives for the stream
    c = by["need-dict"]
    plain = zsc_amd.InflatePlan([len(c.stream)], [c.cap], 15)
    withd = zsc_amd.InflatePlan([len(c.stream)], [c.cap], 15, dicts=[b"unused"], stream_dict=[NO_DICT])
    try:
        a, b = run_plan(plain, [c.stream]), run_plan(withd, [c.stream])
        assert a == b == [(idc.Z_NEED_DICT, b"", 0)]
    finally:
        plain.close()
        withd.close()
    names = ["wrong-dict", "wrong-dict-part", "id-of-the-window-only", "id-of-the-whole", "nofdict-ignored",
             "nofdict-reach", "adler-alone", "adler-with-dict", "empty-dict"]
    group = [by[n] for n in names]
    assert all(c.wbits == 15 for c in group)
    assert [c.status for c in group] == [-3, -3, -3, 0, 0, -3, 0, -3, 0]
    assert [c.consumed for c in group[:3]] == [0, 0, 0] and len(by["id-of-the-whole"].dict) == 51200
    dicts, of = dict_table(group)
    plan = zsc_amd.InflatePlan([len(c.stream) for c in group], [c.cap for c in group], 15, dicts=dicts, stream_dict=of)
    try:
        check(group, run_plan(plan, [c.stream for c in group]), "identification")
        assert plan.dict_ids()[of[3]] == zlib.adler32(by["id-of-the-whole"].dict)
    finally:
        plan.close()
    for name, wbits in (("gzip-ignored", 31), ("gzip-reach", 31), ("auto-gzip-ignored", 47)):
        c = by[name]
        plan = zsc_amd.InflatePlan([len(c.stream)], [c.cap], wbits, dicts=[c.dict])
        try:
            check([c], run_plan(plan, [c.stream]), name)
        finally:
            plan.close()


# ---- 3: the stored-prefix equivalence ----

def equivalence_streams():
    """[(name, S, dictionary, size of S's output, position of the flush marker in S, the first bytes that come
    out behind the marker)]: about 50 small raw streams with a full-flush marker in the middle -- written by
    CPython's zlib with the dictionary, or built by hand with a reach before the marker from behind it"""
    rnd = db.Lcg(77)
    dicts = [idc.make_dict("text", 300 + k, n) for k, n in enumerate((40, 300, 700, 1000, 1000, 2000))]
    out = []
    for k in range(40):
        d = dicts[k % len(dicts)]
        a = bytearray(d[-20:])
        for _ in range(rnd.between(1, 4)):
            n = rnd.between(4, min(30, len(d)))
            at = rnd.below(len(d) - n + 1)
            a += d[at:at + n] + bytes(rnd.between(97, 123) for _ in range(rnd.between(1, 6)))
        b = bytes(rnd.between(65, 91) for _ in range(rnd.between(3, 12)))
        co = zlib.compressobj([1, 6, 9][k % 3], zlib.DEFLATED, -15, zdict=d)
        s = co.compress(bytes(a)) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(b) + co.flush()
        out.append((f"cpython{k}", s, d, len(a) + len(b), s.index(b"\x00\x00\xff\xff"), b))
    for k in range(10):
        d = dicts[1 + k % 5]
        have = len(d)
        head = [rnd.between(97, 123) for _ in range(rnd.between(1, 8))]
        ta = head + [(rnd.between(3, 40), have + len(head) - rnd.below(20)), 65 + k, (rnd.between(3, 259), rnd.between(1, 6))]
        s = db.Stream()
        s.fixed(ta, 0)
        s.stored(b"", 0)
        marker = len(s.bytes()) - 4
        n_a = len(db.play(ta, history=d))
        mark = b"MARK%d" % k
        tb = list(mark) + [(10, len(mark) + rnd.between(1, n_a + 1) + (have if k % 2 else 0))]
        s.fixed(tb, 1)
        raw = s.bytes()
        assert raw[marker:marker + 4] == b"\x00\x00\xff\xff"
        out.append((f"built{k}", raw, d, n_a + len(mark) + 10, marker, mark))
    # one stream whose window holds 32 KiB of a longer dictionary (short, so that its variants stay few)
    d = idc.make_dict("text", 399, 40000)
    s, tokens = idc._fixed([(20, 32768), 97, (258, 32768)])
    out.append(("far", s, d, 279, 0, b""))  # (no marker: no flips)
    return out


def equivalence_variants(s, size, marker):
    """(stream, dest_cap) of every truncation, the three capacities and the byte flips in front of the marker"""
    v = [(s[:n], size) for n in range(len(s))]
    v += [(s, size), (s, max(size, 1) - 1), (s, 0)]
    for at in range(0, marker, 3):
        v.append((s[:at] + bytes([s[at] ^ (1 << (at % 8))]) + s[at + 1:], size))
    return v


def test_stored_prefix_equivalence():
    import zsc_amd
    base = equivalence_streams()
    assert len(base) >= 50
    names, streams, caps, dicts, of, prefixed, haves, flipped, tails = [], [], [], [], [], [], [], [], []
    for name, s, d, size, marker, tail in base:
        t = idc.window_part(d, -15)
        assert len(t) <= 65535
        dicts.append(d)
        first = len(streams)
        for v, cap in equivalence_variants(s, size, marker):
            names.append(name)
            streams.append(v)
            caps.append(cap)
            of.append(len(dicts) - 1)
            prefixed.append(idc.stored_prefix(t) + v)
            haves.append(len(t))
            flipped.append(len(streams) - first > len(s) + 3)
            tails.append(tail)
    dplan = zsc_amd.InflatePlan([len(s) for s in streams], caps, -15, dicts=dicts, stream_dict=of)
    pplan = zsc_amd.InflatePlan([len(s) for s in prefixed], [c + h for c, h in zip(caps, haves)], -15)
    try:
        got, errors, _ = run_plan(dplan, streams, want_errors=True)
        ref, ref_errors, _ = run_plan(pplan, prefixed, want_errors=True)
    finally:
        dplan.close()
        pplan.close()
    resynced, refused = 0, 0
    for k, ((st, out, used), (rst, rout, rused), have) in enumerate(zip(got, ref, haves)):
        what = (names[k], k, len(streams[k]), caps[k])
        assert (st, len(out), used) == (rst, len(rout) - have, rused - 5 - have), what
        assert out == rout[have:], what
        assert errors[k] == ref_errors[k], what
        if flipped[k] and errors[k] and tails[k]:
            # (the bytes behind the marker came out: decoding went on there after the data error)
            resynced += tails[k] in out
            refused += names[k].startswith("built") and errors[k] == 2 and out.endswith(tails[k]) and st == -3
    assert {r[0] for r in got} >= {0, -3, -5}
    assert resynced >= 1, "no case resynchronised"
    assert refused >= 1, "no case reached before out_base after a resynchronisation"


# ---- 4, 5, 6 ----

def test_replacing_the_set_other_buffers_and_packing(cases):
    import torch
    import zsc_amd
    group = [c for c in cases if c.wbits == -15]
    dicts, of = dict_table(group)
    streams = [c.stream for c in group]
    plan = zsc_amd.InflatePlan([len(s) for s in streams], [c.cap for c in group], -15, dicts=[b"another dictionary"])
    try:
        assert plan.scratch_bytes() == 32768 + 8 + 4 * len(group)
        wrong = run_plan(plan, streams)
        assert [r[:1] + (len(r[1]),) for r in wrong] != [(c.status, len(c.out)) for c in group]
        assert plan.dict_enable(dicts, of) == 0
        assert plan.scratch_bytes() == (32768 + 8) * len(dicts) + 4 * len(group)
        assert plan.dict_ids() == [zlib.adler32(d) for d in dicts]
        check(group, run_plan(plan, streams), "the replaced set")
        check(group, run_plan(plan, streams), "other device buffers")
        plan.pack_enable(16)
        res, _, d_dst = run_plan(plan, streams, want_errors=True)
        check(group, res, "with packing enabled")
        cap = sum((len(c.out) + 15) & ~15 for c in group) + 64
        d_packed = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        assert plan.pack(d_dst.data_ptr(), d_packed.data_ptr(), cap) == 0
        offsets, total = plan.pack_results()
        image = d_packed.cpu().numpy().tobytes()
        assert total <= cap
        for c, off in zip(group, offsets):
            assert image[off:off + len(c.out)] == c.out, c.name
    finally:
        plan.close()


def test_other_plan_kinds_and_bad_indexes_refuse(cases):
    import zsc_amd
    texts = [idc.make_dict("text", 500 + k, 3000 + 700 * k) for k in range(3)]
    zs = [zlib.compress(t, 6) for t in texts]
    gz = []
    for t in texts:
        co = zlib.compressobj(6, zlib.DEFLATED, 31)
        gz.append(co.compress(t) + co.flush())
    lens, caps = [len(s) for s in zs], [len(t) for t in texts]
    kinds = {"sections": dict(sections=True), "chunks": dict(chunks=True), "resync": dict(resync=True),
             "indexed": dict(indexes=[None] * 3), "size": dict(size_only=True), "check": dict(check_only=True)}
    for kind, kw in kinds.items():
        plan = zsc_amd.InflatePlan(lens, caps, 15, **kw)
        try:
            assert plan.dict_enable([b"some dictionary"]) == Z_STREAM_ERROR, kind
            assert plan.dict_enable([b"some dictionary"], [0, NO_DICT, 0]) == Z_STREAM_ERROR, kind
            if kind in ("size", "check"):
                import torch
                src = np.zeros(plan.src_bytes, np.uint8)
                for s, off in zip(zs, plan.src_offsets):
                    src[off:off + len(s)] = np.frombuffer(s, np.uint8)
                d_src = torch.from_numpy(src).cuda()
                plan.run(d_src.data_ptr(), 0)
                out_lens, used, stat, _ = plan.results()
                assert (out_lens, used, stat) == (caps, lens, [0, 0, 0]), kind
            else:
                assert run_plan(plan, zs) == [(0, t, len(s)) for t, s in zip(texts, zs)], kind
        finally:
            plan.close()
    plan = zsc_amd.InflatePlan([len(s) for s in gz], caps, 31, members=True)
    try:
        assert plan.dict_enable([b"some dictionary"]) == Z_STREAM_ERROR
        assert run_plan(plan, gz) == [(0, t, len(s)) for t, s in zip(texts, gz)]
    finally:
        plan.close()
    # an index out of range: the plan is left as it was -- a plain plan, then one with its first set
    by = {c.name: c for c in cases}
    group = [by["adler-alone"], by["need-dict"], by["nofdict-ignored"]]
    streams = [c.stream for c in group]
    plan = zsc_amd.InflatePlan([len(s) for s in streams], [c.cap for c in group], 15)
    try:
        with pytest.raises(ValueError):
            plan.dict_ids()
        assert plan.dict_enable([group[0].dict], [0, 1, 0]) == Z_STREAM_ERROR
        assert plan.dict_enable([], None) == Z_STREAM_ERROR  # (dictionary 0 for every stream, and there is none)
        assert plan.scratch_bytes() == 0
        assert [r[0] for r in run_plan(plan, streams)] == [idc.Z_NEED_DICT, idc.Z_NEED_DICT, 0]
        assert plan.dict_enable([group[0].dict], [0, NO_DICT, 0]) == 0
        check(group, run_plan(plan, streams), "the first set")
        assert plan.dict_enable([b"x", b"y"], [0, 2, NO_DICT]) == Z_STREAM_ERROR
        check(group, run_plan(plan, streams), "the first set, after a refused second one")
        assert plan.dict_ids() == [zlib.adler32(group[0].dict)]
    finally:
        plan.close()


def test_host_pointer_batches(cases):
    import zsc_amd
    by = {c.name: c for c in cases}
    group = [by[n] for n in ("adler-alone", "need-dict", "wrong-dict", "id-of-the-whole", "nofdict-ignored", "rec036",
                             "rec041", "all-block-types-z")]
    group = [c for c in group if c.wbits == 15]
    assert len(group) >= 6
    dicts, of = dict_table(group)
    rc, outs, used, stat = zsc_amd.uncompress_dict_batch([c.stream for c in group], [c.cap for c in group], dicts, of, 15)
    assert rc == 0
    check(group, list(zip(stat, outs, used)), "zsc_amd.uncompress_dict_batch")
    # the C function itself, with arrays of this test's own
    n, nd = len(group), len(dicts)
    srcs = (C.c_char_p * n)(*[c.stream for c in group])
    slen = (C.c_uint32 * n)(*[len(c.stream) for c in group])
    bufs = [C.create_string_buffer(max(c.cap, 1)) for c in group]
    dsts = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    dlen = (C.c_uint32 * n)(*[c.cap for c in group])
    st = (C.c_int32 * n)()
    dptr = (C.c_char_p * nd)(*dicts)
    dl = (C.c_uint32 * nd)(*[len(d) for d in dicts])
    sd = (C.c_uint32 * n)(*of)
    rc = zsc_amd.lib.zsc_hip_uncompress_dict_batch(n, srcs, slen, dsts, dlen, st, 15, nd, dptr, dl, sd)
    assert rc == 0
    check(group, [(st[i], bufs[i].raw[:dlen[i]], slen[i]) for i in range(n)], "zsc_hip_uncompress_dict_batch")
    # one shared dictionary, stream_dict None: dictionary 0 for every stream
    c = by["adler-alone"]
    rc, outs, used, stat = zsc_amd.uncompress_dict_batch([c.stream] * 3, [c.cap] * 3, [c.dict])
    assert (rc, outs, used, stat) == (0, [c.out] * 3, [c.consumed] * 3, [0] * 3)
    rc, _, _, _ = zsc_amd.uncompress_dict_batch([c.stream], [c.cap], [c.dict], [1])
    assert rc == Z_STREAM_ERROR
