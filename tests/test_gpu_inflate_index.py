"""Seek-point indexes on the GPU: export from a chunks plan, inflate from the index, ranges.  Every item is
compared with the oracle and with the plain plan."""
import random
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNK = 8192
Z_DATA_ERROR = -3


def _plan_run(torch, plan, streams, stream=0):
    src = torch.zeros(plan.src_bytes, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(plan.dst_bytes, dtype=torch.uint8, device="cuda")
    for s, off in zip(streams, plan.src_offsets):
        if s:
            src[off:off + len(s)] = torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda()
    plan.run(src.data_ptr(), dst.data_ptr(), stream)
    lens, used, stat, _ = plan.results()
    host = dst.cpu().numpy()
    outs = [bytes(host[o:o + n]) for o, n in zip(plan.dst_offsets, lens)]
    return lens, used, stat, outs, plan.sections()


def _indexed(torch, zsc_amd, streams, caps, wbits, blobs, ranges=None):
    plan = zsc_amd.InflatePlan([len(s) for s in streams], caps, window_bits=wbits, indexes=blobs, ranges=ranges)
    try:
        return _plan_run(torch, plan, streams)
    finally:
        plan.close()


def test_round_trip_batches(oracle):
    import torch
    import zsc_amd
    from test_inflate_chunks_emu import make_cases
    by_wbits = {}
    for c in make_cases(oracle):
        by_wbits.setdefault(c[3], []).append(c)
    took = 0
    for wbits, group in by_wbits.items():
        srcs = [c[1] for c in group]
        caps = [c[2] for c in group]
        blobs = zsc_amd.build_indexes(srcs, caps, window_bits=wbits, chunk_bytes=CHUNK)
        crc, couts, cused, cstat = zsc_amd.uncompress_chunks_batch(srcs, caps, window_bits=wbits)
        assert crc == 0
        rc, outs, used, stat = zsc_amd.uncompress_indexed_batch(srcs, caps, blobs, window_bits=wbits)
        prc, pouts, pused, pstat = zsc_amd.uncompress_batch(srcs, caps, window_bits=wbits)
        assert rc == prc == 0
        lens, iused, istat, iouts, ipieces = _indexed(torch, zsc_amd, srcs, caps, wbits, blobs)
        for i, (name, s, cap, _, _) in enumerate(group):
            want = oracle.uncompress(s, cap, window_bits=wbits)
            assert (cstat[i], couts[i], cused[i]) == want, name
            assert (stat[i], outs[i], used[i]) == want, name
            assert (pstat[i], pouts[i], pused[i]) == want, name
            assert (istat[i], iouts[i], iused[i]) == want, name
            if blobs[i] is None:
                assert ipieces[i] == 0, name
            else:
                h = zsc_amd.index_info(blobs[i])
                assert h["points"] > 1 and want[0] == 0, name
                assert (h["total_out"], h["consumed"], h["points"]) == (len(want[1]), want[2], ipieces[i]), name
                assert (h["chunk_bytes"], h["window_bits"]) == (CHUNK, wbits), name
                took += 1
    assert took > 25


def test_untrusted_blobs_in_one_batch(oracle):
    import torch
    import zsc_amd
    from test_inflate_index_emu import damaged_blobs, many_piece_streams
    for name, stream, sibling, cap, wbits in many_piece_streams(oracle):
        want = oracle.uncompress(stream, cap, window_bits=wbits)
        blob = zsc_amd.build_indexes([stream], [cap], window_bits=wbits, chunk_bytes=CHUNK)[0]
        assert blob is not None
        n = max(len(stream), len(sibling))
        a, b = stream + bytes(n - len(stream)), sibling + bytes(n - len(sibling))
        other = zsc_amd.build_indexes([b], [cap], window_bits=wbits, chunk_bytes=CHUNK)[0]
        assert other is not None
        junk = stream + b"\x01\x02junk after the trailer"
        # (what, stream, cap, blob, pieces expected: None = as many as the index has)
        items = [("true", stream, cap, blob, None), ("none", stream, cap, None, 0), ("junk", junk, cap, blob, None),
                 ("other-stream", a, cap, other, 0), ("short-cap", stream, cap - 1, blob, 0)]
        items += [(f"cut-{cut}", stream[:-cut], cap, blob, 0) for cut in (1, 5, len(stream) // 3)]
        items += [(what, stream, cap, bad, 0) for what, bad in damaged_blobs(blob)]
        srcs = [it[1] for it in items]
        caps = [it[2] for it in items]
        blobs = [it[3] for it in items]
        lens, used, stat, outs, pieces = _indexed(torch, zsc_amd, srcs, caps, wbits, blobs)
        rc, bouts, bused, bstat = zsc_amd.uncompress_indexed_batch(srcs, caps, blobs, window_bits=wbits)
        prc, pouts, pused, pstat = zsc_amd.uncompress_batch(srcs, caps, window_bits=wbits)
        assert rc == prc == 0
        npts = zsc_amd.index_info(blob)["points"]
        for i, (what, s, c, _, expect) in enumerate(items):
            orc = oracle.uncompress(s, c, window_bits=wbits)
            assert (stat[i], outs[i], used[i]) == orc, (name, what)
            assert (bstat[i], bouts[i], bused[i]) == orc, (name, what)
            assert (pstat[i], pouts[i], pused[i]) == orc, (name, what)
            assert pieces[i] == (npts if expect is None else expect), (name, what, pieces[i])
        assert (stat[2], outs[2], used[2]) == (0, want[1], len(stream))
        # another window_bits than the index's
        w2 = {15: 31, 31: 15, -15: 15}[wbits]
        lens, used, stat, outs, pieces = _indexed(torch, zsc_amd, [stream], [cap], w2, [blob])
        assert (stat[0], outs[0], used[0]) == oracle.uncompress(stream, cap, window_bits=w2) and pieces == [0]


def test_ranges_in_one_batch(oracle):
    import torch
    import zsc_amd
    from zsc_amd import corpus
    from test_inflate_chunks_emu import zlib_stream
    from test_inflate_index_emu import covering_run, flip, points, reseal
    text = corpus.make_buffer("text", 400000, 21)
    for wbits in (15, 31, -15):
        s = zlib_stream(text, 6, wbits)
        blob = zsc_amd.build_indexes([s], [len(text)], window_bits=wbits, chunk_bytes=CHUNK)[0]
        pts = points(blob)
        assert len(pts) >= 4
        rnd = random.Random(77)
        ranges = []
        for _ in range(50):
            b = rnd.randrange(len(text))
            ranges.append((b, rnd.randrange(1, min(len(text) - b, 120000) + 1)))
        edge = pts[len(pts) // 2]["off"]
        ranges += [(0, 1), (len(text) - 1, 1), (0, len(text)), (edge - 1, 1), (edge, 1), (edge - 1, 2)]
        want = [covering_run(pts, b, n) for b, n in ranges]
        assert [zsc_amd.index_range(blob, b, n) for b, n in ranges] == want
        k = len(pts) // 2
        bad = reseal(flip(blob, pts[k]["woff"] + pts[k]["wlen"] - 1, 0))
        # the ranges, a whole stream beside them, a damaged window, no index, a broken index
        n = len(ranges)
        srcs = [s] * (n + 4)
        caps = [w[3] for w in want] + [len(text), pts[k]["len"], 100, 100]
        blobs = [blob] * (n + 1) + [bad, None, blob[:-1]]
        rngs = ranges + [None, (pts[k]["off"], 1), (0, 1), (0, 1)]
        lens, used, stat, outs, pieces = _indexed(torch, zsc_amd, srcs, caps, wbits, blobs, rngs)
        trailer = struct.unpack_from("<I", blob, 36)[0]
        for i, (first, count, pbegin, plen) in enumerate(want):
            last = first + count
            end_bit = pts[last]["bit"] if last < len(pts) else 8 * trailer
            assert (stat[i], pieces[i], used[i]) == (0, count, (end_bit + 7) // 8), ranges[i]
            assert outs[i] == text[pbegin:pbegin + plen], ranges[i]
        assert (stat[n], outs[n], used[n], pieces[n]) == (0, text, len(s), len(pts))
        for i in (n + 1, n + 2, n + 3):
            assert (stat[i], lens[i], used[i], pieces[i]) == (Z_DATA_ERROR, 0, 0, 0), i
        for b, ln in ((len(text), 1), (len(text) - 1, 2), (0, len(text) + 1), (5, 0)):
            with pytest.raises(ValueError):
                zsc_amd.index_range(blob, b, ln)
            with pytest.raises(RuntimeError):
                zsc_amd.InflatePlan([len(s)], [len(text)], window_bits=wbits, indexes=[blob], ranges=[(b, ln)])


def test_index_enable_is_for_chunks_plans_only():
    import zsc_amd
    plan = zsc_amd.InflatePlan([100], [100])
    assert zsc_amd.lib.zsc_hip_inflate_plan_index_enable(plan._h, 1) == zsc_amd.Z_STREAM_ERROR
    plan.close()
    plan = zsc_amd.InflatePlan([100], [100], sections=True)
    assert zsc_amd.lib.zsc_hip_inflate_plan_index_enable(plan._h, 1) == zsc_amd.Z_STREAM_ERROR
    plan.close()


def test_indexed_device_plan_twice_on_two_streams(oracle):
    import torch
    import zsc_amd
    text = np.random.default_rng(6).choice(np.frombuffer(b"etaoin shrdlu", dtype=np.uint8), 1500000).tobytes()
    rnd = np.random.default_rng(7).integers(0, 40, 1500000, dtype=np.uint8).tobytes()
    streams = [zlib.compress(text, 1), zlib.compress(rnd, 6), zlib.compress(text[:3000], 6)]
    caps = [len(text), len(rnd), 3000]
    blobs = zsc_amd.build_indexes(streams, caps, chunk_bytes=16384)
    assert blobs[0] is not None and blobs[1] is not None and blobs[2] is None
    plan = zsc_amd.InflatePlan([len(s) for s in streams], caps, indexes=blobs)
    assert plan.scratch_bytes() > 0
    a = _plan_run(torch, plan, streams, 0)
    side = torch.cuda.Stream()
    b = _plan_run(torch, plan, streams, side.cuda_stream)
    assert a == b
    lens, used, stat, outs, pieces = a
    assert stat == [0, 0, 0] and outs == [text, rnd, text[:3000]] and used == [len(s) for s in streams]
    assert pieces == [zsc_amd.index_info(blobs[0])["points"], zsc_amd.index_info(blobs[1])["points"], 0]
    assert pieces[0] > 1 and pieces[1] > 1


def test_256mib_marker_free_stream_from_its_index():
    import torch
    import zsc_amd
    rng = np.random.default_rng(9)
    words = [bytes(rng.integers(97, 123, rng.integers(2, 9), dtype=np.uint8)) for _ in range(4000)]
    idx = rng.integers(0, len(words), 50_000_000)
    text = b" ".join(words[i] for i in idx)[: 256 << 20]
    text += b"x" * ((256 << 20) - len(text))
    s = zlib.compress(text, 1)
    assert s.count(b"\x00\x00\xff\xff") < 64
    plan = zsc_amd.InflatePlan([len(s)], [len(text)], chunks=True, keep_index=True)
    kept = _plan_run(torch, plan, [s])
    blob = plan.export_index(0)
    plan.close()
    plan = zsc_amd.InflatePlan([len(s)], [len(text)], chunks=True)
    plain = _plan_run(torch, plan, [s])
    plan.close()
    assert kept == plain  # the exporting plan returns what a chunks plan without keep_index returns
    lens, used, stat, outs, pieces = kept
    assert stat == [0] and used == [len(s)] and outs[0] == text and pieces[0] > 1
    assert blob is not None and zsc_amd.index_info(blob)["points"] == pieces[0]
    got = _indexed(torch, zsc_amd, [s], [len(text)], 15, [blob])
    assert got[1:3] == ([len(s)], [0]) and got[4] == pieces
    assert got[3][0] == text
    begin = (128 << 20) + 12345
    first, count, pbegin, plen = zsc_amd.index_range(blob, begin, 1 << 20)
    assert pbegin <= begin and pbegin + plen >= begin + (1 << 20)
    lens, used, stat, outs, rp = _indexed(torch, zsc_amd, [s], [plen], 15, [blob], [(begin, 1 << 20)])
    assert (stat, lens, rp) == ([0], [plen], [count])
    assert outs[0][begin - pbegin:begin - pbegin + (1 << 20)] == text[begin:begin + (1 << 20)]
    assert outs[0] == text[pbegin:pbegin + plen]
