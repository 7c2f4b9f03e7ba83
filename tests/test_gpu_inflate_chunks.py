"""The chunks inflate path on the GPU: results equal the oracle's and the plain plan's, item by item."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_chunks_batch_equals_oracle_and_plain(oracle):
    import zsc_amd
    from test_inflate_chunks_emu import make_cases
    cases = make_cases(oracle)
    by_wbits = {}
    for c in cases:
        by_wbits.setdefault(c[3], []).append(c)
    for wbits, group in by_wbits.items():
        srcs = [c[1] for c in group]
        caps = [c[2] for c in group]
        rc, outs, used, stat = zsc_amd.uncompress_chunks_batch(srcs, caps, window_bits=wbits)
        prc, pouts, pused, pstat = zsc_amd.uncompress_batch(srcs, caps, window_bits=wbits)
        assert rc == prc == 0
        for i, (name, s, cap, _, _) in enumerate(group):
            orc, oout, oused = oracle.uncompress(s, cap, window_bits=wbits)
            assert (stat[i], outs[i], used[i]) == (orc, oout, oused), name
            assert (stat[i], outs[i], used[i]) == (pstat[i], pouts[i], pused[i]), name


def _plan_run(torch, plan, streams, caps, stream):
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


def test_device_plan_twice_on_two_streams(oracle):
    import torch
    import zsc_amd
    text = np.random.default_rng(6).choice(np.frombuffer(b"etaoin shrdlu", dtype=np.uint8), 1500000).tobytes()
    rnd = np.random.default_rng(7).integers(0, 40, 1500000, dtype=np.uint8).tobytes()
    streams = [zlib.compress(text, 1), zlib.compress(rnd, 6), zlib.compress(text[:3000], 6)]
    caps = [len(text), len(rnd), 3000]
    plan = zsc_amd.InflatePlan([len(s) for s in streams], caps, chunks=True, chunk_bytes=16384)
    assert plan.scratch_bytes() > 0
    a = _plan_run(torch, plan, streams, caps, 0)
    side = torch.cuda.Stream()
    b = _plan_run(torch, plan, streams, caps, side.cuda_stream)
    assert a == b
    lens, used, stat, outs, pieces = a
    assert stat == [0, 0, 0] and outs == [text, rnd, text[:3000]] and used == [len(s) for s in streams]
    assert pieces[0] > 1 and pieces[1] > 1 and pieces[2] == 0


def test_sync_flush_stream_in_pieces():
    import zsc_amd
    text = bytes(np.random.default_rng(8).integers(97, 123, 4 << 20, dtype=np.uint8))
    co = zlib.compressobj(6, zlib.DEFLATED, 15)
    s = b"".join(co.compress(text[i:i + 65536]) + co.flush(zlib.Z_SYNC_FLUSH) for i in range(0, len(text), 65536))
    s += co.flush()
    plan = zsc_amd.InflatePlan([len(s)], [len(text)], chunks=True)
    import torch
    lens, used, stat, outs, pieces = _plan_run(torch, plan, [s], [len(text)], 0)
    assert stat == [0] and outs == [text] and used == [len(s)]
    assert pieces[0] > 1


def test_256mib_marker_free_stream():
    import torch
    import zsc_amd
    rng = np.random.default_rng(9)
    words = [bytes(rng.integers(97, 123, rng.integers(2, 9), dtype=np.uint8)) for _ in range(4000)]
    idx = rng.integers(0, len(words), 50_000_000)
    text = b" ".join(words[i] for i in idx)[: 256 << 20]
    text += b"x" * ((256 << 20) - len(text))
    s = zlib.compress(text, 1)
    assert s.count(b"\x00\x00\xff\xff") < 64
    plan = zsc_amd.InflatePlan([len(s)], [len(text)], chunks=True)
    lens, used, stat, outs, pieces = _plan_run(torch, plan, [s], [len(text)], 0)
    assert stat == [0] and used == [len(s)] and lens == [len(text)]
    assert outs[0] == text
    assert pieces[0] > 1
