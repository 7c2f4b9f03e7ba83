"""Check plans on the GPU (zsc_amd/csrc/inflate_check.h): status, size and consumed equal the oracle's and the
plain plan's at the same limits on the same streams, with no exception, and the check values handed out are
zlib's over the oracle's output."""
import os
import zlib

import numpy as np
import pytest

from zsc_amd import corpus

pytestmark = pytest.mark.gpu

CHUNK = 4096


def check_batch(oracle, names, streams, hints, wbits, limits):
    """one check call on the batch: equal to the oracle and to the plain plan on the same streams"""
    import zsc_amd
    from test_gpu_inflate_size import plain_caps
    from test_inflate_check_emu import answer
    rc, sizes, used, stat, vals = zsc_amd.uncompress_check_batch(streams, limits, window_bits=wbits)
    assert rc == 0
    prc, pouts, pused, pstat = zsc_amd.uncompress_batch(streams, plain_caps(oracle, streams, limits, wbits, hints),
                                                        window_bits=wbits)
    assert prc == 0
    for i, name in enumerate(names):
        want = answer(oracle, streams[i], limits[i], wbits, hints[i])
        got = (stat[i], sizes[i], used[i], vals[i])
        print(wbits, name, limits[i], got, want)
        assert got == want, (wbits, name, limits[i])
        assert got[:3] == (pstat[i], len(pouts[i]), pused[i]), (wbits, name, limits[i])


def test_check_equals_oracle_and_plain_plan(oracle):
    from test_gpu_inflate_size import shape_cases
    from test_inflate_check_emu import trailer_flips
    from test_inflate_size_emu import UNLIMITED, limits_of
    flips = trailer_flips()
    for wbits, group in shape_cases().items():
        group = group + [(f"flip-{name}", s, len(flips[wbits][1])) for name, s, _ in flips.get(wbits, (0, 0, []))[2]]
        names = [c[0] for c in group]
        streams = [c[1] for c in group]
        hints = [c[2] for c in group]
        per = [limits_of(oracle, s, wbits, h) for s, h in zip(streams, hints)]
        # limit class k: unlimited, the exact size, the size minus 1, 0 (a stream of size 0 has three)
        for k in range(4):
            check_batch(oracle, names, streams, hints, wbits, [p[min(k, len(p) - 1)] for p in per])
        # partly filled wavefronts: four streams share one
        if wbits == 15:
            pick = [i for i, n in enumerate(names) if n in ("dynamic", "far", "stored", "fixed", "flip-check2")]
            assert len(pick) == 5
            for count in (1, 3, 4, 5):
                sub = pick[:count]
                check_batch(oracle, [names[i] for i in sub], [streams[i] for i in sub], [hints[i] for i in sub],
                            wbits, [UNLIMITED] * count)


def _check_plan_run(torch, plan, streams, stream=0, d_dst=0):
    src = torch.zeros(plan.src_bytes, dtype=torch.uint8, device="cuda")
    for s, off in zip(streams, plan.src_offsets):
        if s:
            src[off:off + len(s)] = torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda()
    plan.run(src.data_ptr(), d_dst, stream)
    lens, used, stat, _ = plan.results()
    return lens, used, stat, plan.sections(), plan.data_errors(), plan.check_values()


def test_ring_wrap_and_fold_lengths(oracle):
    """outputs that end just before, at and just behind the fold boundaries and the ring's wrap, never cut;
    then 24 of them, long and short in turn, through four lane groups, so that every ring serves several"""
    import torch
    import zsc_amd
    from test_inflate_check_emu import WRAPPERS, answer, boundary_cases
    for wbits in WRAPPERS:
        cases = boundary_cases((wbits,))
        streams = [c[1] for c in cases]
        want = [answer(oracle, s, zsc_amd.NO_LIMIT, wbits, n) for _, s, _, n in cases]
        assert all(w[0] == 0 and w[1] == c[3] for w, c in zip(want, cases))
        plan = zsc_amd.InflatePlan([len(s) for s in streams], None, window_bits=wbits, check_only=True,
                                   chunk_bytes=zsc_amd.NO_LIMIT)
        lens, used, stat, pieces, errors, vals = _check_plan_run(torch, plan, streams)
        plan.close()
        for i, c in enumerate(cases):
            assert (stat[i], lens[i], used[i], vals[i]) == want[i] and pieces[i] == 0, (wbits, c[0])
        # ring reuse: the longest and the shortest outputs in turn, six streams to a ring
        by_len = sorted(range(len(cases)), key=lambda i: cases[i][3])
        pick = [i for pair in zip(by_len[-12:], by_len[:12]) for i in pair]
        assert len(pick) == 24
        os.environ["ZSC_HIP_CHECK_GROUPS"] = "4"
        try:
            plan = zsc_amd.InflatePlan([len(streams[i]) for i in pick], None, window_bits=wbits, check_only=True,
                                       chunk_bytes=zsc_amd.NO_LIMIT)
        finally:
            del os.environ["ZSC_HIP_CHECK_GROUPS"]
        assert plan.scratch_bytes() == 96 * 24 + 16 + 8 + 65536 * 4 + 4 * 24
        lens, used, stat, pieces, errors, vals = _check_plan_run(torch, plan, [streams[i] for i in pick])
        plan.close()
        for j, i in enumerate(pick):
            assert (stat[j], lens[j], used[j], vals[j]) == want[i], (wbits, cases[i][0])


def test_long_streams_in_pieces(oracle):
    """five long streams in one check plan next to a chunks plan on the same streams: text, zeros (flushed
    every 64 bytes, so that the stream is longer than a chunk), every match at distance 32 768, stored
    blocks, and the broken chain of the size tests in a zlib wrapper"""
    import struct
    import torch
    import zsc_amd
    from test_gpu_inflate_chunks import _plan_run
    from test_gpu_inflate_size import broken_chain_stream
    text = corpus.make_buffer("text", 300000, 91)
    rnd = np.random.default_rng(92).integers(0, 256, 32768, dtype=np.uint8).tobytes()
    noise = np.random.default_rng(93).integers(0, 256, 200000, dtype=np.uint8).tobytes()
    co = zlib.compressobj(6, zlib.DEFLATED, 15)
    zeros = b"".join(co.compress(bytes(64)) + co.flush(zlib.Z_SYNC_FLUSH) for _ in range(250000 // 64)) + co.flush()
    broken, broken_size = broken_chain_stream()
    broken_out = oracle.uncompress(broken, broken_size, window_bits=-15)[1]
    assert len(broken_out) == broken_size
    streams = [zlib.compress(text, 6), zeros, zlib.compress((rnd * 8)[:250000], 6), zlib.compress(noise, 0),
               b"\x78\x9c" + broken + struct.pack(">I", zlib.adler32(broken_out))]
    outs = [text, bytes(250000 // 64 * 64), (rnd * 8)[:250000], noise, broken_out]
    caps = [len(o) for o in outs]
    lens = [len(s) for s in streams]
    assert all(n > 2 * CHUNK for n in lens)
    chunks = zsc_amd.InflatePlan(lens, caps, chunks=True, chunk_bytes=CHUNK)
    clens, cused, cstat, couts, cpieces = _plan_run(torch, chunks, streams, caps, 0)
    chunks.close()
    assert couts == outs and cstat == [0] * 5
    plan = zsc_amd.InflatePlan(lens, caps, check_only=True, chunk_bytes=CHUNK)
    got = _check_plan_run(torch, plan, streams)
    print(got, cpieces)
    assert got[:4] == (clens, cused, cstat, cpieces)
    assert all(p > 1 for p in got[3][:4])
    assert got[5] == [zlib.adler32(o) for o in outs]
    # one byte of the text stream's check value flipped: that stream alone changes
    bad = streams[0][:-3] + bytes([streams[0][-3] ^ 0x08]) + streams[0][-2:]
    again = _check_plan_run(torch, plan, [bad] + streams[1:])
    plan.close()
    assert (again[2][0], again[0][0], again[1][0], again[3][0], again[5][0]) == (-3, caps[0], lens[0], 0, 0)
    assert [x[1:] for x in again] == [x[1:] for x in got]
    assert again[4][0] == 1 and got[4] == [0] * 5


def test_damaged_streams_and_limits(oracle):
    import torch
    import zsc_amd
    from test_gpu_inflate_chunks import _plan_run
    from test_inflate_check_emu import answer, damaged_flush_cases
    text = corpus.make_buffer("text", 150000, 94)
    for wbits in (15, 31):
        cases = [c for c in damaged_flush_cases() if c[2] == wbits]
        assert len(cases) == 3
        co = zlib.compressobj(6, zlib.DEFLATED, wbits)
        long_one = co.compress(text) + co.flush()
        streams = [c[1] for c in cases] + [long_one, long_one]
        limits = [c[3] for c in cases] + [len(text) - 50000, len(text)]
        lens = [len(s) for s in streams]
        plain = zsc_amd.InflatePlan(lens, limits, window_bits=wbits)
        plens, pused, pstat, _, _ = _plan_run(torch, plain, streams, limits, 0)
        perrors = plain.data_errors()
        plain.close()
        plan = zsc_amd.InflatePlan(lens, limits, window_bits=wbits, check_only=True, chunk_bytes=CHUNK)
        lens_, used, stat, pieces, errors, vals = _check_plan_run(torch, plan, streams)
        plan.close()
        assert (lens_, used, stat, errors) == (plens, pused, pstat, perrors)
        assert errors[:3] == [c[4] for c in cases] and stat[:3] == [-3, -3, -3] and vals[:4] == [0, 0, 0, 0]
        assert (stat[3], lens_[3], pieces[3]) == (-5, len(text) - 50000, 0)
        assert (stat[4], lens_[4]) == (0, len(text)) and pieces[4] > 1
        for i, s in enumerate(streams):
            assert (stat[i], lens_[i], used[i], vals[i]) == answer(oracle, s, limits[i], wbits, len(text)), (wbits, i)


def test_check_plan_contract():
    import torch
    import zsc_amd
    import ctypes as C
    text = corpus.make_buffer("text", 120000, 95)
    streams = [zlib.compress(text, 6), zlib.compress(text[:5000], 6), zlib.compress(text[:70000], 1)]
    lens = [len(s) for s in streams]
    want = ([len(text), 5000, 70000], lens, [0, 0, 0])
    values = [zlib.adler32(text), zlib.adler32(text[:5000]), zlib.adler32(text[:70000])]
    plans = [zsc_amd.InflatePlan(lens, [limit] * 3, check_only=True, chunk_bytes=16384)
             for limit in (1 << 20, zsc_amd.NO_LIMIT)]
    # scratch: the header's formula (include/zsc_hip.h), whatever the limits
    nchunks = sum(-(-n // 16384) for n in lens if n > 16384)
    nactive = sum(n > 16384 for n in lens)
    assert nactive >= 1
    formula = 65536 * 4 + 98372 * nchunks + 8 * max(nchunks - nactive, 1) + 4 * 3 + 96 * 3 + 16
    assert [p.scratch_bytes() for p in plans] == [formula, formula]
    plan = plans[0]
    out = (C.c_uint32 * 3)()
    # no values before a run, none from another kind of plan; nothing to pack, no index
    assert zsc_amd.lib.zsc_hip_inflate_plan_check_values(plan._h, out) == zsc_amd.Z_STREAM_ERROR
    with pytest.raises(ValueError):
        plan.pack_enable(16)
    assert zsc_amd.lib.zsc_hip_inflate_plan_pack_enable(plan._h, 16) == zsc_amd.Z_STREAM_ERROR
    assert zsc_amd.lib.zsc_hip_inflate_plan_index_enable(plan._h, 1) == zsc_amd.Z_STREAM_ERROR
    plain = zsc_amd.InflatePlan(lens, want[0])
    assert zsc_amd.lib.zsc_hip_inflate_plan_check_values(plain._h, out) == zsc_amd.Z_STREAM_ERROR
    # a NULL destination; a second run gives the same
    a = _check_plan_run(torch, plan, streams, 0, 0)
    assert a[:3] == want and a[4] == [0, 0, 0] and a[5] == values and a[3][1] == 0
    assert _check_plan_run(torch, plan, streams, 0, 0) == a
    assert _check_plan_run(torch, plans[1], streams, 0, 0) == a
    # a plain plan is what it was, also after check plans in the process
    from test_gpu_inflate_chunks import _plan_run
    got = _plan_run(torch, plain, streams, want[0], 0)
    assert got[:3] == want and got[3] == [text, text[:5000], text[:70000]]
    assert zsc_amd.lib.zsc_hip_inflate_plan_check_values(plain._h, out) == zsc_amd.Z_STREAM_ERROR
    for p in plans + [plain]:
        p.close()
