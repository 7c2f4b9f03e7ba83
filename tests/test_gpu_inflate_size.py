"""Size plans on the GPU (zsc_amd/csrc/inflate_size.h): status, size and consumed equal the oracle's and the
plain plan's at the same limits, with the one exception the contract names (include/zsc_hip.h; expect() of
tests/test_inflate_size_emu.py builds it into the expectation)."""
import struct
import zlib

import numpy as np
import pytest

from zsc_amd import corpus

pytestmark = pytest.mark.gpu

CHUNK = 4096


def _gz(data, level=6):
    co = zlib.compressobj(level, zlib.DEFLATED, 31)
    return co.compress(data) + co.flush()


def _raw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return co.compress(data) + co.flush()


def _zl(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, zdict=None):
    co = (zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy, zdict) if zdict is not None
          else zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy))
    return co.compress(data) + co.flush()


def shape_cases():
    """{window_bits: [(name, stream, size hint)]}: the shapes where the group decoder can go wrong"""
    text = corpus.make_buffer("text", 20000, 51)
    rnd = np.random.default_rng(52).integers(0, 256, 32768, dtype=np.uint8).tobytes()
    far = (rnd * 3)[:70000]  # 70 000 bytes, every match at distance 32 768
    half = rnd[:600]
    first_dist = b"\x03\x02"  # a final fixed block whose first symbol is a match: length 3, distance 1
    small_win = bytes([0x18, (31 - (0x18 * 256) % 31) % 31]) + _raw(half + half)  # a 512-byte window, distance 600
    dyn = _zl(text)
    assert (dyn[2] >> 1) & 3 == 2
    gz = _gz(text)
    z = [("len0", b"", 0), ("empty", zlib.compress(b""), 0), ("stored", _zl(text, 0), len(text)),
         ("fixed", _zl(text[:3000], 6, zlib.Z_FIXED), 3000), ("dynamic", dyn, len(text)),
         ("far", _zl(far), len(far)), ("first-dist", b"\x78\x9c" + first_dist, 0),
         ("wbits9-dist600", small_win, 1200), ("fdict", _zl(text, 6, zdict=b"the dictionary"), len(text))]
    z += [(f"cut{k}", dyn[:-k], len(text)) for k in range(1, 13)]
    r = [("stored", _raw(text, 0), len(text)), ("fixed", _raw(text[:3000], 6, zlib.Z_FIXED), 3000),
         ("dynamic", _raw(text), len(text)), ("far", _raw(far), len(far)), ("first-dist", first_dist, 0),
         ("len0", b"", 0)]
    r += [(f"cut{k}", r[2][1][:-k], len(text)) for k in range(1, 13)]
    g = [("dynamic", gz, len(text)), ("empty", _gz(b""), 0), ("far", _gz(far), len(far)),
         ("stored", _gz(text, 0), len(text))]
    g += [(f"cut{k}", gz[:-k], len(text)) for k in range(1, 13)]
    return {15: z, -15: r, 31: g}


def plain_caps(oracle, streams, limits, wbits, hints):
    """dest_caps that stand for the limits in a plain plan: an unlimited stream gets a capacity its output
    does not fill (a decode that never meets the end of its buffer is the decode without one)"""
    from test_inflate_size_emu import UNLIMITED, expect
    return [expect(oracle, s, UNLIMITED, wbits, h)[0][1] + 4096 if lim == UNLIMITED else lim
            for s, lim, h in zip(streams, limits, hints)]


def check_batch(oracle, names, streams, hints, wbits, limits):
    """one size call on the batch: equal to the oracle and to the plain plan, stream by stream"""
    import zsc_amd
    from test_inflate_size_emu import expect, with_right_check
    rc, sizes, used, stat = zsc_amd.uncompress_sizes_batch(streams, limits, window_bits=wbits)
    assert rc == 0
    # the plain plan sees the streams with their check values made right where that is the only fault
    fixed = [with_right_check(s, wbits) or s for s in streams]
    prc, pouts, pused, pstat = zsc_amd.uncompress_batch(fixed, plain_caps(oracle, streams, limits, wbits, hints),
                                                        window_bits=wbits)
    assert prc == 0
    for i, name in enumerate(names):
        want, _ = expect(oracle, streams[i], limits[i], wbits, hints[i])
        got = (stat[i], sizes[i], used[i])
        print(wbits, name, limits[i], got, want)
        assert got == want, (wbits, name, limits[i])
        assert got == (pstat[i], len(pouts[i]), pused[i]), (wbits, name, limits[i])


def test_sizes_equal_oracle_and_plain_plan(oracle):
    from test_inflate_size_emu import UNLIMITED, limits_of
    for wbits, group in shape_cases().items():
        names = [c[0] for c in group]
        streams = [c[1] for c in group]
        hints = [c[2] for c in group]
        per = [limits_of(oracle, s, wbits, h) for s, h in zip(streams, hints)]
        # limit class k: unlimited, the exact size, the size minus 1, 0 (a stream of size 0 has three)
        for k in range(4):
            check_batch(oracle, names, streams, hints, wbits, [p[min(k, len(p) - 1)] for p in per])
        # partly filled wavefronts: four streams share one
        if wbits == 15:
            pick = [i for i, n in enumerate(names) if n in ("dynamic", "far", "stored", "fixed", "cut3")]
            for count in (1, 3, 4, 5):
                sub = pick[:count]
                check_batch(oracle, [names[i] for i in sub], [streams[i] for i in sub], [hints[i] for i in sub],
                            wbits, [UNLIMITED] * count)


def _size_plan_run(torch, plan, streams, stream, d_dst=0):
    src = torch.zeros(plan.src_bytes, dtype=torch.uint8, device="cuda")
    for s, off in zip(streams, plan.src_offsets):
        if s:
            src[off:off + len(s)] = torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda()
    plan.run(src.data_ptr(), d_dst, stream)
    lens, used, stat, _ = plan.results()
    return lens, used, stat, plan.sections(), plan.data_errors()


def broken_chain_stream():
    """a raw stream whose chain breaks: a stored block that ends in chunk 2 behind four false dynamic-header
    candidates (complete little deflate streams in its payload), so the true boundary is not among the
    chunk's candidates, and a run of fixed-Huffman blocks, which the scan does not look for, to the end"""
    text = corpus.make_buffer("text", 60000, 41)
    mini = _raw(text[:700], 9)
    assert (mini[0] >> 1) & 3 == 2 and len(mini) < 600
    payload = bytearray(text[1000:12000])
    for j in range(4):
        at = 2 * CHUNK + 16 + j * 650 - 5
        payload[at:at + len(mini)] = mini
    s = b"\x00" + struct.pack("<HH", len(payload), len(payload) ^ 0xffff) + bytes(payload)
    s += _raw(text[20000:], 6, zlib.Z_FIXED)
    return s, len(payload) + len(text) - 20000


def test_chunked_sizing():
    import torch
    import zsc_amd
    many = np.random.default_rng(61).integers(0, 40, 65536, dtype=np.uint8).tobytes()
    text = corpus.make_buffer("text", 200000, 62)
    co = zlib.compressobj(6, zlib.DEFLATED, 15)
    sync = b"".join(co.compress(text[i:i + 8192]) + co.flush(zlib.Z_SYNC_FLUSH) for i in range(0, len(text), 8192))
    sync += co.flush()
    streams = [zlib.compress(many, 6), sync, zlib.compress(text[:3000], 6)]
    assert len(streams[0]) > 4 * CHUNK and len(streams[1]) > 4 * CHUNK and len(streams[2]) <= CHUNK
    want = [len(many), len(text), 3000]
    plan = zsc_amd.InflatePlan([len(s) for s in streams], None, size_only=True, chunk_bytes=CHUNK)
    a = _size_plan_run(torch, plan, streams, 0)  # (d_dst NULL)
    side = torch.cuda.Stream()
    b = _size_plan_run(torch, plan, streams, side.cuda_stream)
    assert a == b
    lens, used, stat, pieces, errors = a
    assert stat == [0, 0, 0] and lens == want and used == [len(s) for s in streams] and errors == [0, 0, 0]
    assert pieces[0] > 1 and pieces[1] > 1 and pieces[2] == 0
    nchunks = sum(-(-len(s) // CHUNK) for s in streams[:2])
    print("scratch bytes per chunk:", plan.scratch_bytes() / nchunks)
    assert 0 < plan.scratch_bytes() < 1024 * nchunks
    # a destination is not looked at either
    sentinel = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")
    assert _size_plan_run(torch, plan, streams, 0, sentinel.data_ptr()) == a
    assert bool((sentinel == 0xA5).all())
    plan.close()
    # a chain that breaks: sized by the whole-stream decode, still exact
    s, size = broken_chain_stream()
    plan = zsc_amd.InflatePlan([len(s), len(s)], [zsc_amd.NO_LIMIT, size - 1], window_bits=-15, size_only=True,
                               chunk_bytes=CHUNK)
    lens, used, stat, pieces, errors = _size_plan_run(torch, plan, [s, s], 0)
    assert (stat[0], lens[0], used[0], pieces[0]) == (0, size, len(s), 0)
    assert (stat[1], lens[1], pieces[1]) == (-5, size - 1, 0)
    with pytest.raises(ValueError):
        plan.pack_enable(16)
    assert zsc_amd.lib.zsc_hip_inflate_plan_index_enable(plan._h, 1) == zsc_amd.Z_STREAM_ERROR
    plan.close()


def test_chunks_cases_sized_in_pieces(oracle):
    """the streams of the chunks tests through one size plan per window_bits, cut at 4 KiB"""
    import torch
    import zsc_amd
    from test_inflate_chunks_emu import make_cases
    from test_inflate_size_emu import UNLIMITED, expect
    by_wbits = {}
    for c in make_cases(oracle):
        by_wbits.setdefault(c[3], []).append(c)
    parallel = 0
    for wbits, group in by_wbits.items():
        streams = [c[1] for c in group]
        for limits in ([UNLIMITED] * len(group), [c[2] for c in group]):
            plan = zsc_amd.InflatePlan([len(s) for s in streams], limits, window_bits=wbits, size_only=True,
                                       chunk_bytes=CHUNK)
            lens, used, stat, pieces, _ = _size_plan_run(torch, plan, streams, 0)
            plan.close()
            for i, (name, s, cap, _, _) in enumerate(group):
                want, _ = expect(oracle, s, limits[i], wbits, cap)
                assert (stat[i], lens[i], used[i]) == want, (wbits, name, limits[i])
                assert pieces[i] == 0 or stat[i] == 0, (wbits, name)
                parallel += pieces[i] > 1
    assert parallel > 50


def test_damaged_streams_equal_the_plain_plan(oracle):
    import torch
    import zsc_amd
    from test_inflate_size_emu import damaged_cases, expect, with_right_check
    by_wbits, seen = {}, set()
    for c in damaged_cases(oracle, 90):
        by_wbits.setdefault(c[2], []).append(c)
    for wbits, group in by_wbits.items():
        streams = [c[1] for c in group]
        fixed = [with_right_check(s, wbits) or s for s in streams]
        for limits in ([c[3] for c in group], [max(c[3] // 2, 1) for c in group]):
            plan = zsc_amd.InflatePlan([len(s) for s in streams], limits, window_bits=wbits, size_only=True,
                                       chunk_bytes=CHUNK)
            lens, used, stat, _, errors = _size_plan_run(torch, plan, streams, 0)
            plan.close()
            plain = zsc_amd.InflatePlan([len(s) for s in fixed], limits, window_bits=wbits)
            src = torch.zeros(plain.src_bytes, dtype=torch.uint8, device="cuda")
            dst = torch.zeros(plain.dst_bytes, dtype=torch.uint8, device="cuda")
            for s, off in zip(fixed, plain.src_offsets):
                src[off:off + len(s)] = torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda()
            plain.run(src.data_ptr(), dst.data_ptr(), 0)
            plens, pused, pstat, _ = plain.results()
            perrors = plain.data_errors()
            plain.close()
            for i, (name, s, _, hint) in enumerate(group):
                got = (stat[i], lens[i], used[i], errors[i])
                assert got == (pstat[i], plens[i], pused[i], perrors[i]), (wbits, name, limits[i])
                assert got[:3] == expect(oracle, s, limits[i], wbits, hint)[0], (wbits, name, limits[i])
                seen.add((stat[i], errors[i] > 1))
    assert {(-3, True), (-3, False), (0, False), (-5, False)} <= seen


def test_auto_round_trip():
    import zsc_amd
    bufs = [corpus.make_buffer(kind, size, 70 + i) for i, (kind, size) in enumerate(
        [("text", 300000), ("bitmap", 40000), ("table", 20000), ("random", 5000), ("zero", 3000), ("text", 0)])]
    streams = [zlib.compress(b, 1 + i) for i, b in enumerate(bufs)]
    streams.append(streams[0][:-4000])                              # truncated: Z_BUF_ERROR when sized
    streams.append(streams[1][:-1] + bytes([streams[1][-1] ^ 1]))  # a wrong Adler-32: sized Z_OK
    rc, sizes, used, sstat = zsc_amd.uncompress_sizes_batch(streams)
    assert rc == 0 and sstat == [0] * 6 + [-5, 0]
    rc, outs, used2, stat, sizes2 = zsc_amd.uncompress_batch_auto(streams)
    assert rc == 0 and sizes2 == sizes
    for i, b in enumerate(bufs):
        assert sizes[i] == len(b) and stat[i] == 0 and outs[i] == b and used2[i] == len(streams[i]), i
    assert outs[6] == bufs[0][:sizes[6]] and stat[6] == -5
    assert sizes[7] == len(bufs[1]) and outs[7] == bufs[1] and stat[7] == -3  # (the inflate finds the check value)
    # a limit: a guard against a bomb
    rc, outs, _, stat, sizes = zsc_amd.uncompress_batch_auto(streams[:2], limit=50000)
    assert rc == 0 and sizes == [50000, 40000] and stat == [-5, 0]
    assert outs == [bufs[0][:50000], bufs[1]]


def test_other_plan_kinds_unchanged():
    """a plain plan and a chunks plan give what they gave, before and after a size plan in the process"""
    import torch
    import zsc_amd
    from test_gpu_inflate_chunks import _plan_run
    text = corpus.make_buffer("text", 400000, 81)
    streams = [zlib.compress(text, 1), zlib.compress(text[:50000], 9), zlib.compress(text, 6)[:-7]]
    caps = [len(text), 50000, len(text)]
    lens = [len(s) for s in streams]

    def both():
        p = zsc_amd.InflatePlan(lens, caps)
        a = _plan_run(torch, p, streams, caps, 0)
        scratch = p.scratch_bytes()
        p.close()
        c = zsc_amd.InflatePlan(lens, caps, chunks=True, chunk_bytes=16384)
        b = _plan_run(torch, c, streams, caps, 0)
        scratch = (scratch, c.scratch_bytes())
        c.close()
        return a, b, scratch
    before = both()
    plan = zsc_amd.InflatePlan(lens, None, size_only=True, chunk_bytes=16384)
    got = _size_plan_run(torch, plan, streams, 0)
    plan.close()
    assert both() == before
    assert got[:3] == before[0][:3] and got[2] == [0, 0, -5] and got[0][:2] == [len(text), 50000]
    assert before[0][:4] == before[1][:4] and before[0][3][:2] == [text, text[:50000]]
    assert before[0][4] == [0, 0, 0] and before[1][4][0] > 1
