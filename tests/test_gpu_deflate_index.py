"""Seek-point indexes written by a deflate plan on the GPU: every stream is the oracle's, every blob feeds an
indexed inflate plan that takes every piece, and a plan without the index is what it always was."""
import ctypes as C
import random
import struct

import pytest

pytestmark = pytest.mark.gpu

CHUNK = 8192
PLANS = [(6, 15), (1, 31), (9, -15), (6, 9)]
_CACHE = {}


def _mix(corpus, size, seed):
    third = size // 3
    return (corpus.make_buffer("text", third, seed) + corpus.make_buffer("random", third, seed + 1) +
            corpus.make_buffer("zero", size - 2 * third, seed + 2))


def _buffers(seed0=100, sizes=(1, 3072, 20000, 70001, 300000), kinds=("text", "random", "zero", "mix"), empty=True):
    """about 40 buffers: every kind at every size under two seeds, and the empty buffer"""
    key = (seed0, sizes, kinds, empty)
    if key not in _CACHE:
        from zsc_amd import corpus
        bufs = [b""] if empty else []
        for rep in range(2):
            for k, kind in enumerate(kinds):
                for size in sizes:
                    seed = seed0 + 10 * rep + k
                    bufs.append(_mix(corpus, size, seed) if kind == "mix" else corpus.make_buffer(kind, size, seed))
        _CACHE[key] = bufs
    return _CACHE[key]


def _oracle_streams(oracle, bufs, level, wbits):
    key = ("oracle", tuple(hash(b) for b in bufs), level, wbits)
    if key not in _CACHE:
        _CACHE[key] = [oracle.compress(b, level, window_bits=wbits)[1] for b in bufs]
    return _CACHE[key]


def _upload(torch, plan, bufs):
    src = torch.zeros(plan.in_bytes, dtype=torch.uint8, device="cuda")
    for s, off in zip(bufs, plan.in_offsets):
        if s:
            src[off:off + len(s)] = torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda()
    return src


def _run(torch, plan, src):
    dst = torch.zeros(plan.out_bytes, dtype=torch.uint8, device="cuda")
    plan.run(src.data_ptr(), dst.data_ptr())
    lens, stat = plan.results()
    host = dst.cpu().numpy().tobytes()
    return [host[o:o + n] for o, n in zip(plan.out_offsets, lens)], stat


def _inflate_indexed(torch, zsc_amd, streams, caps, wbits, blobs, ranges=None):
    """(statuses, outputs, consumed, pieces) of an indexed plan"""
    plan = zsc_amd.InflatePlan([len(s) for s in streams], caps, window_bits=wbits, indexes=blobs, ranges=ranges)
    try:
        src = torch.zeros(plan.src_bytes, dtype=torch.uint8, device="cuda")
        dst = torch.zeros(plan.dst_bytes, dtype=torch.uint8, device="cuda")
        for s, off in zip(streams, plan.src_offsets):
            if s:
                src[off:off + len(s)] = torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda()
        plan.run(src.data_ptr(), dst.data_ptr())
        lens, used, stat, _ = plan.results()
        host = dst.cpu().numpy().tobytes()
        return stat, [host[o:o + n] for o, n in zip(plan.dst_offsets, lens)], used, plan.sections()
    finally:
        plan.close()


def _check_batch(torch, zsc_amd, oracle, bufs, level, wbits, streams, stat, blobs, chunk=CHUNK):
    want = _oracle_streams(oracle, bufs, level, wbits)
    assert stat == [0] * len(bufs)
    for i, (got, w) in enumerate(zip(streams, want)):
        assert got == w, (i, len(bufs[i]))
    infos = []
    for i, blob in enumerate(blobs):
        assert blob is not None and zsc_amd.lib.zsc_hip_index_validate(blob, len(blob)) == 0, i
        h = zsc_amd.index_info(blob)
        assert (h["total_out"], h["consumed"], h["chunk_bytes"], h["window_bits"]) == (len(bufs[i]), len(streams[i]), chunk, wbits), i
        infos.append(h)
    caps = [len(b) for b in bufs]
    rc, outs, used, istat = zsc_amd.uncompress_indexed_batch(streams, caps, blobs, window_bits=wbits)
    assert rc == 0 and istat == [0] * len(bufs) and outs == bufs and used == [len(s) for s in streams]
    dstat, douts, dused, pieces = _inflate_indexed(torch, zsc_amd, streams, caps, wbits, blobs)
    assert dstat == [0] * len(bufs) and douts == bufs and dused == [len(s) for s in streams]
    assert pieces == [h["points"] for h in infos]
    assert any(p > 1 for p in pieces)
    rc, pouts, pused, pstat = zsc_amd.uncompress_batch(streams, caps, window_bits=wbits)
    assert rc == 0 and pstat == [0] * len(bufs) and pouts == bufs and pused == used


@pytest.mark.parametrize("level,wbits", PLANS)
def test_one_batch(oracle, level, wbits):
    import torch
    import zsc_amd
    bufs = _buffers()
    assert 35 <= len(bufs) <= 45
    plan = zsc_amd.DeflatePlan([len(b) for b in bufs], level, wbits)
    try:
        plan.index_enable(CHUNK)
        src = _upload(torch, plan, bufs)
        streams, stat = _run(torch, plan, src)
        blobs = plan.export_indexes(src.data_ptr())
    finally:
        plan.close()
    _check_batch(torch, zsc_amd, oracle, bufs, level, wbits, streams, stat, blobs)


def test_convenience_call(oracle):
    import torch
    import zsc_amd
    bufs = _buffers()[:12]
    streams, stat, blobs = zsc_amd.compress_batch_indexed(bufs, 6, 15, 8, 0, CHUNK)
    _check_batch(torch, zsc_amd, oracle, bufs, 6, 15, streams, stat, blobs)
    streams, stat, blobs = zsc_amd.compress_batch_indexed(bufs[:3], chunk_bytes=0)
    assert [zsc_amd.index_info(b)["chunk_bytes"] for b in blobs] == [128 * 1024] * 3


def test_two_sub_batches(oracle, monkeypatch):
    """the records of sub-batch 0 must survive sub-batch 1's reuse of the scratch"""
    import torch
    import zsc_amd
    bufs = _buffers()
    assert sum(len(b) for b in bufs) > 2 << 20
    monkeypatch.setenv("ZSC_HIP_SUBBATCH_MB", "1")
    plan = zsc_amd.DeflatePlan([len(b) for b in bufs], 6, 15)
    monkeypatch.delenv("ZSC_HIP_SUBBATCH_MB")
    try:
        assert plan.sub_batches >= 2
        plan.index_enable(CHUNK)
        plan.profile(True)
        src = _upload(torch, plan, bufs)
        streams, stat = _run(torch, plan, src)
        blobs = plan.export_indexes(src.data_ptr())
        assert plan.index_ms() > 0.0 and plan.kernel_times_ms()["total"] > 0.0
    finally:
        plan.close()
    _check_batch(torch, zsc_amd, oracle, bufs, 6, 15, streams, stat, blobs)


def test_second_run_on_another_input(oracle):
    import torch
    import zsc_amd
    shape = dict(sizes=(3072, 70001, 300000), kinds=("text", "random", "mix"), empty=False)
    first, second = _buffers(300, **shape), _buffers(400, **shape)
    assert [len(b) for b in first] == [len(b) for b in second] and all(a != b for a, b in zip(first, second))
    plan = zsc_amd.DeflatePlan([len(b) for b in first], 6, 15)
    try:
        plan.index_enable(CHUNK)
        src1 = _upload(torch, plan, first)
        streams1, stat1 = _run(torch, plan, src1)
        blobs1 = plan.export_indexes(src1.data_ptr())
        src2 = _upload(torch, plan, second)
        streams2, stat2 = _run(torch, plan, src2)
        blobs2 = plan.export_indexes(src2.data_ptr())
    finally:
        plan.close()
    _check_batch(torch, zsc_amd, oracle, first, 6, 15, streams1, stat1, blobs1)
    _check_batch(torch, zsc_amd, oracle, second, 6, 15, streams2, stat2, blobs2)
    # the first run's blobs are not the second run's streams': serial, the oracle's result
    caps = [len(b) for b in second]
    stat, outs, used, pieces = _inflate_indexed(torch, zsc_amd, streams2, caps, 15, blobs1)
    assert pieces == [0] * len(second)
    for i, s in enumerate(streams2):
        assert (stat[i], outs[i], used[i]) == oracle.uncompress(s, caps[i], window_bits=15), i


def test_off_by_default_and_the_errors(oracle):
    import torch
    import zsc_amd
    from zsc_amd import corpus
    bufs = [corpus.make_buffer("text", 300000, 51), corpus.make_buffer("text", 300000, 52), b"", b"x" * 3072]
    lens = [len(b) for b in bufs]
    plain = zsc_amd.DeflatePlan(lens, 6, 15)
    try:
        src = _upload(torch, plain, bufs)
        pstreams, pstat = _run(torch, plain, src)
        with pytest.raises(RuntimeError):
            plain.export_indexes(src.data_ptr())
        need = C.c_uint64(7)
        assert zsc_amd.lib.zsc_hip_deflate_plan_index_size(plain._h, 0, C.byref(need)) == zsc_amd.Z_STREAM_ERROR
        assert zsc_amd.lib.zsc_hip_deflate_plan_index_export(plain._h, 0, C.c_void_p(src.data_ptr()), None, 0,
                                                             C.byref(need)) == zsc_amd.Z_STREAM_ERROR
        ms = C.c_float()
        assert zsc_amd.lib.zsc_hip_deflate_plan_index_ms(plain._h, C.byref(ms)) == zsc_amd.Z_STREAM_ERROR
    finally:
        plain.close()
    plan = zsc_amd.DeflatePlan(lens, 6, 15)
    try:
        before = plan.scratch_bytes
        plan.index_enable(CHUNK)
        assert plan.scratch_bytes > before
        src = _upload(torch, plan, bufs)
        streams, stat = _run(torch, plan, src)
        assert (streams, stat) == (pstreams, pstat) and stat == [0] * 4
        blobs = plan.export_indexes(src.data_ptr())
        # a short cap: Z_BUF_ERROR and the bytes needed
        need, got = C.c_uint64(), C.c_uint64()
        assert zsc_amd.lib.zsc_hip_deflate_plan_index_size(plan._h, 0, C.byref(need)) == 0
        assert need.value == len(blobs[0])
        room = C.create_string_buffer(need.value)
        rc = zsc_amd.lib.zsc_hip_deflate_plan_index_export(plan._h, 0, C.c_void_p(src.data_ptr()), room,
                                                           need.value - 1, C.byref(got))
        assert (rc, got.value) == (zsc_amd.Z_BUF_ERROR, need.value)
        # another input (zeros): well-formed blobs with the wrong windows
        zeros = torch.zeros(plan.in_bytes, dtype=torch.uint8, device="cuda")
        wrong = plan.export_indexes(zeros.data_ptr())
    finally:
        plan.close()
    assert all(zsc_amd.lib.zsc_hip_index_validate(b, len(b)) == 0 for b in wrong)
    assert zsc_amd.index_info(wrong[0])["points"] > 1 and wrong[0] != blobs[0] and len(wrong[0]) == len(blobs[0])
    stat, outs, used, pieces = _inflate_indexed(torch, zsc_amd, streams[:2], lens[:2], 15, wrong[:2])
    assert pieces == [0, 0] and stat == [0, 0] and outs == bufs[:2] and used == [len(s) for s in streams[:2]]
    stat, outs, used, pieces = _inflate_indexed(torch, zsc_amd, streams, lens, 15, blobs)
    assert stat == [0] * 4 and outs == bufs and all(p >= 1 for p in pieces)


def test_short_out_cap_gives_no_blob(oracle):
    import torch
    import zsc_amd
    from zsc_amd import corpus
    bufs = [corpus.make_buffer("random", 20000, 61), corpus.make_buffer("text", 20000, 62)]
    n = 2
    lens = (C.c_uint32 * n)(*[len(b) for b in bufs])
    in_off, out_off, caps = (C.c_uint64 * n)(), (C.c_uint64 * n)(), (C.c_uint32 * n)()
    ib, ob = C.c_uint64(), C.c_uint64()
    assert zsc_amd.lib.zsc_hip_deflate_plan_layout(n, lens, 6, 15, 8, in_off, out_off, caps, C.byref(ib), C.byref(ob)) == 0
    want = [oracle.compress(b, 6)[1] for b in bufs]
    caps[0] = len(want[0]) - 1  # one byte short
    h = C.c_void_p()
    assert zsc_amd.lib.zsc_hip_deflate_plan_create(C.byref(h), n, lens, in_off, out_off, caps, 6, 15, 8, 0) == 0
    try:
        assert zsc_amd.lib.zsc_hip_deflate_plan_index_enable(h, 256) == 0
        src = torch.zeros(ib.value, dtype=torch.uint8, device="cuda")
        dst = torch.zeros(ob.value, dtype=torch.uint8, device="cuda")
        for b, off in zip(bufs, in_off):
            src[off:off + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
        assert zsc_amd.lib.zsc_hip_deflate_plan_run(h, C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), None) == 0
        dl, st = (C.c_uint32 * n)(), (C.c_int32 * n)()
        assert zsc_amd.lib.zsc_hip_deflate_plan_results(h, dl, st) == 0
        assert list(st) == [zsc_amd.Z_BUF_ERROR, 0]
        need = C.c_uint64(7)
        assert zsc_amd.lib.zsc_hip_deflate_plan_index_size(h, 0, C.byref(need)) == zsc_amd.Z_DATA_ERROR
        assert need.value == 0
        room = C.create_string_buffer(4096)
        got = C.c_uint64(7)
        assert zsc_amd.lib.zsc_hip_deflate_plan_index_export(h, 0, C.c_void_p(src.data_ptr()), room, 4096,
                                                             C.byref(got)) == zsc_amd.Z_DATA_ERROR
        assert got.value == 0
        assert zsc_amd.lib.zsc_hip_deflate_plan_index_size(h, 1, C.byref(need)) == 0 and need.value > 0
        assert zsc_amd.lib.zsc_hip_deflate_plan_index_size(h, 2, C.byref(need)) == zsc_amd.Z_STREAM_ERROR
    finally:
        zsc_amd.lib.zsc_hip_deflate_plan_destroy(h)


def test_ranges_in_one_batch(oracle):
    import torch
    import zsc_amd
    from zsc_amd import corpus
    from test_inflate_index_emu import covering_run, flip, points, reseal
    text = corpus.make_buffer("text", 400000, 21)
    for wbits in (15, 31, -15):
        streams, stat, blobs = zsc_amd.compress_batch_indexed([text], 6, wbits, 8, 0, CHUNK)
        s, blob = streams[0], blobs[0]
        assert stat == [0] and s == oracle.compress(text, 6, window_bits=wbits)[1]
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
        assert pts[k]["wlen"] > 0
        bad = reseal(flip(blob, pts[k]["woff"] + pts[k]["wlen"] - 1, 0))
        # the ranges, a whole stream beside them, a damaged window, no index, a broken index
        n = len(ranges)
        srcs = [s] * (n + 4)
        caps = [w[3] for w in want] + [len(text), pts[k]["len"], 100, 100]
        idxs = [blob] * (n + 1) + [bad, None, blob[:-1]]
        rngs = ranges + [None, (pts[k]["off"], 1), (0, 1), (0, 1)]
        stat, outs, used, pieces = _inflate_indexed(torch, zsc_amd, srcs, caps, wbits, idxs, rngs)
        trailer = struct.unpack_from("<I", blob, 36)[0]
        for i, (first, count, pbegin, plen) in enumerate(want):
            last = first + count
            end_bit = pts[last]["bit"] if last < len(pts) else 8 * trailer
            assert (stat[i], pieces[i], used[i]) == (0, count, (end_bit + 7) // 8), ranges[i]
            assert outs[i] == text[pbegin:pbegin + plen], ranges[i]
        assert (stat[n], outs[n], used[n], pieces[n]) == (0, text, len(s), len(pts))
        for i in (n + 1, n + 2, n + 3):
            assert (stat[i], len(outs[i]), used[i], pieces[i]) == (-3, 0, 0, 0), i
