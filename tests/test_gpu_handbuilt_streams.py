"""Hand-built DEFLATE streams at the format's limits (tests/deflate_builder.py) through every inflate path of
the C ABI on the GPU.

Expected values are the records of tests/golden/handbuilt_golden.json (the compiled reference's answers) and
play(), the plain-Python statement of what the tokens inflate to; never a second GPU path alone.  The same
records pass through the lane emulations in tests/test_handbuilt_streams_emu.py.
"""
import pytest

import deflate_builder as B

pytestmark = pytest.mark.gpu

CHUNK = 8192


@pytest.fixture(scope="module")
def golden():
    """(records, streams by case name, the golden file, expected output by case name)"""
    recs, streams, g = B.records()
    wants = {name: want for name, _, _, _, want in B.cases()}
    return recs, streams, g, wants


def by_window_bits(recs):
    groups = {}
    for r in recs:
        groups.setdefault(r.window_bits, []).append(r)
    assert set(groups) == {15, 31, -15}
    return groups


def path_records(recs):
    """the composed streams and `deep`: what the plans that cut a stream into pieces are given"""
    names = set(B.composed_names()) | {"deep"}
    return [r for r in recs if r.name in names]


def sources(recs, streams):
    return [streams[r.name][:r.cut] for r in recs], [r.cap for r in recs]


def assert_records(what, recs, golden, stat, outs, used):
    """(status, bytes, consumed) of a path against the records, item by item"""
    _, _, g, wants = golden
    assert len(stat) == len(outs) == len(used) == len(recs)
    for r, st, out, u in zip(recs, stat, outs, used):
        assert (st, len(out), u) == (r.rc, r.out_len, r.consumed), (what, r.name, r.cut, r.cap, st, len(out), u)
        want = wants[r.name]
        if want is not None and out != want[:len(out)]:
            tokens = B.tokens_of(r.name) if r.name in ("deep", "ring-edge") else None
            n = next((i for i, (a, b) in enumerate(zip(out, want)) if a != b), min(len(out), len(want)))
            pytest.fail(f"{what}: {r.name} cut {r.cut} cap {r.cap}: " +
                        (B.first_difference(out, want, tokens) if tokens else f"first difference at offset {n}"))
    B.check_outputs(recs, g, outs, what)


def assert_sizes(what, recs, stat, sizes, used):
    for r, st, n, u in zip(recs, stat, sizes, used):
        assert (st, n, u) == (r.rc, r.out_len, r.consumed), (what, r.name, r.cut, r.cap, st, n, u)


def check_values_of(recs, wants):
    return [B.check_value(wants[r.name], r.window_bits) if r.rc == 0 else 0 for r in recs]


def test_uncompress_batch_in_every_group_slot(golden):
    """all records in one call per window_bits; then rotated by 1, 2 and 3 positions, so that a stream sits in
    other group slots of a wavefront, beside other neighbours"""
    import zsc_amd
    recs, streams, _, _ = golden
    for wbits, group in by_window_bits(recs).items():
        first = None
        for k in (0, 1, 2, 3):
            turned = group[k:] + group[:k]
            srcs, caps = sources(turned, streams)
            rc, outs, used, stat = zsc_amd.uncompress_batch(srcs, caps, window_bits=wbits)
            assert rc == 0
            assert_records(f"uncompress_batch w{wbits} rotated {k}", turned, golden, stat, outs, used)
            back = [x[len(group) - k:] + x[:len(group) - k] for x in (outs, used, stat)] if k else [outs, used, stat]
            if first is None:
                first = back
            assert back == first, (wbits, k)


def test_error_exits_beside_15_bit_codes(golden):
    """a wavefront's four streams share the instruction stream: `deep` and `ring-edge` (15-bit codes, every
    copy distance) with two erroneous streams between them, in every wavefront of a plain plan"""
    import torch
    import zsc_amd
    recs, streams, g, wants = golden
    full = {r.name: r for r in recs if r.cut == len(streams[r.name]) and r.cap == g["cases"][r.name]["cap"]}
    bad = [n for n, w in wants.items() if w is None and g["cases"][n]["window_bits"] == -15]
    assert len(bad) >= 28
    items = []
    for i in range(0, len(bad) - 1, 2):
        items += [full["deep"], full[bad[i]], full["ring-edge"], full[bad[i + 1]]]
    srcs, caps = sources(items, streams)
    plan = zsc_amd.InflatePlan([len(s) for s in srcs], caps, window_bits=-15, decode_order=list(range(len(items))))
    try:
        stat, outs, used, _ = run_plan(torch, plan, srcs)
    finally:
        plan.close()
    assert_records("plain plan in the given order", items, golden, stat, outs, used)


def test_sizes_and_check_batches(golden):
    import zsc_amd
    from test_inflate_size_emu import with_right_check
    recs, streams, _, wants = golden
    for wbits, group in by_window_bits(recs).items():
        srcs, caps = sources(group, streams)
        # the size path's one exception (a wrong check value in a whole trailer is not seen) applies to no
        # record: every check value here is right
        assert all(with_right_check(s, wbits) in (None, s) for s in srcs)
        rc, sizes, used, stat = zsc_amd.uncompress_sizes_batch(srcs, caps, window_bits=wbits)
        assert rc == 0
        assert_sizes(f"uncompress_sizes_batch w{wbits}", group, stat, sizes, used)
        rc, sizes, used, stat, values = zsc_amd.uncompress_check_batch(srcs, caps, window_bits=wbits)
        assert rc == 0
        assert_sizes(f"uncompress_check_batch w{wbits}", group, stat, sizes, used)
        assert values == check_values_of(group, wants), wbits


def run_plan(torch, plan, srcs, sized=False):
    """(statuses, outputs or sizes, consumed, sections())"""
    src = torch.zeros(plan.src_bytes, dtype=torch.uint8, device="cuda")
    for s, off in zip(srcs, plan.src_offsets):
        if s:
            src[off:off + len(s)] = torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda()
    if sized:
        plan.run(src.data_ptr(), 0)
        lens, used, stat, _ = plan.results()
        return stat, lens, used, plan.sections()
    dst = torch.zeros(plan.dst_bytes, dtype=torch.uint8, device="cuda")
    plan.run(src.data_ptr(), dst.data_ptr())
    lens, used, stat, _ = plan.results()
    host = dst.cpu().numpy()
    outs = [bytes(host[o:o + n]) for o, n in zip(plan.dst_offsets, lens)]
    return stat, outs, used, plan.sections()


def test_chunks_size_and_check_plans(golden):
    """chunk_bytes 8192: every composed stream decodes, is sized and is checked in more than one piece"""
    import torch
    import zsc_amd
    recs, streams, g, wants = golden
    for wbits, group in by_window_bits(path_records(recs)).items():
        srcs, caps = sources(group, streams)
        lens = [len(s) for s in srcs]
        whole = [i for i, r in enumerate(group) if r.name.startswith("composed-") and r.cut == len(streams[r.name])
                 and r.cap == len(wants[r.name])]
        assert len(whole) == 1
        plan = zsc_amd.InflatePlan(lens, caps, window_bits=wbits, chunks=True, chunk_bytes=CHUNK)
        try:
            stat, outs, used, pieces = run_plan(torch, plan, srcs)
        finally:
            plan.close()
        assert_records(f"chunks plan w{wbits}", group, golden, stat, outs, used)
        assert all(pieces[i] > 1 for i in whole), (wbits, pieces)
        plan = zsc_amd.InflatePlan(lens, caps, window_bits=wbits, size_only=True, chunk_bytes=CHUNK)
        try:
            stat, sizes, used, pieces = run_plan(torch, plan, srcs, sized=True)
        finally:
            plan.close()
        assert_sizes(f"size plan w{wbits}", group, stat, sizes, used)
        assert all(pieces[i] > 1 for i in whole), (wbits, pieces)
        plan = zsc_amd.InflatePlan(lens, caps, window_bits=wbits, check_only=True, chunk_bytes=CHUNK)
        try:
            stat, sizes, used, pieces = run_plan(torch, plan, srcs, sized=True)
            values = plan.check_values()
        finally:
            plan.close()
        assert_sizes(f"check plan w{wbits}", group, stat, sizes, used)
        assert values == check_values_of(group, wants), wbits
        assert all(pieces[i] > 1 for i in whole), (wbits, pieces)


def test_indexes_and_a_range(golden):
    import torch
    import zsc_amd
    recs, streams, g, wants = golden
    for wbits, group in by_window_bits(path_records(recs)).items():
        srcs, caps = sources(group, streams)
        blobs = zsc_amd.build_indexes(srcs, caps, window_bits=wbits, chunk_bytes=CHUNK)
        name = next(n for n in B.composed_names() if g["cases"][n]["window_bits"] == wbits)
        whole = next(i for i, r in enumerate(group) if r.name == name and r.cut == len(streams[name])
                     and r.cap == len(wants[name]))
        assert blobs[whole] is not None and zsc_amd.index_info(blobs[whole])["points"] > 1
        rc, outs, used, stat = zsc_amd.uncompress_indexed_batch(srcs, caps, blobs, window_bits=wbits)
        assert rc == 0
        assert_records(f"uncompress_indexed_batch w{wbits}", group, golden, stat, outs, used)
        # a read out of the middle: the whole pieces that cover it, as index_range reports them
        want, blob = wants[name], blobs[whole]
        begin, length = len(want) // 2 - 4321, 100000
        first, count, pbegin, plen = zsc_amd.index_range(blob, begin, length)
        assert pbegin <= begin and begin + length <= pbegin + plen and count >= 1
        plan = zsc_amd.InflatePlan([len(streams[name])], [plen], window_bits=wbits, indexes=[blob],
                                   ranges=[(begin, length)])
        try:
            stat, outs, used, pieces = run_plan(torch, plan, [streams[name]])
        finally:
            plan.close()
        assert (stat, pieces) == ([0], [count])
        assert outs[0] == want[pbegin:pbegin + plen], name


def test_sections_and_resync_batches(golden):
    """for these inputs (no flush markers to speak of) both paths are documented to equal uncompress_batch"""
    import zsc_amd
    recs, streams, _, _ = golden
    for wbits, group in by_window_bits(recs).items():
        srcs, caps = sources(group, streams)
        rc, outs, used, stat = zsc_amd.uncompress_sections_batch(srcs, caps, window_bits=wbits)
        assert rc == 0
        assert_records(f"uncompress_sections_batch w{wbits}", group, golden, stat, outs, used)
        rc, outs, used, stat = zsc_amd.uncompress_resync_batch(srcs, caps, window_bits=wbits)
        assert rc == 0
        assert_records(f"uncompress_resync_batch w{wbits}", group, golden, stat, outs, used)


def test_copy_quotient_and_ring(golden):
    """`deep` (every distance 1..770 with a 258-byte copy behind a fresh literal: the quotient of the
    lane-parallel copy from the hardware reciprocal) and `ring-edge` (sources around pos - 512), byte for
    byte against play(); a mismatch names the offset and the token, so a wrong quotient points at its distance"""
    import zsc_amd
    _, streams, _, wants = golden
    names = ["deep", "ring-edge"]
    srcs = [streams[n] for n in names]
    rc, outs, used, stat = zsc_amd.uncompress_batch(srcs, [len(wants[n]) for n in names], window_bits=-15)
    assert rc == 0 and stat == [0, 0] and used == [len(s) for s in srcs]
    for name, out in zip(names, outs):
        assert out == wants[name], f"{name}: " + B.first_difference(out, wants[name], B.tokens_of(name))
