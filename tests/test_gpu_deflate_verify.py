"""Read-back verification of a deflate plan's streams on the GPU (zsc_amd/csrc/deflate_verify.h): every stream is
the oracle's and verifies OK; a damaged stream that the oracle's decoder does not turn back into the input never
does, and the verdict names the block the damage lies in; a plan without verification is what it always was."""
import random

import pytest

pytestmark = pytest.mark.gpu

PLANS = [(6, 15), (1, 31), (9, -15), (6, 9)]
OK, SKIPPED, HEADER, TRAILER = 0, -1, 1, 9
NONE = 0xFFFFFFFF
Z_STREAM_ERROR = -2
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


def _oracle_streams(oracle, bufs, level, wbits, mem_level=8):
    key = ("oracle", tuple(hash(b) for b in bufs), level, wbits, mem_level)
    if key not in _CACHE:
        _CACHE[key] = [oracle.compress(b, level, window_bits=wbits, mem_level=mem_level)[1] for b in bufs]
    return _CACHE[key]


def _upload(torch, plan, bufs):
    src = torch.zeros(plan.in_bytes, dtype=torch.uint8, device="cuda")
    for s, off in zip(bufs, plan.in_offsets):
        if s:
            src[off:off + len(s)] = torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda()
    return src


def _run(torch, plan, src):
    """(device output, streams, statuses)"""
    dst = torch.zeros(plan.out_bytes, dtype=torch.uint8, device="cuda")
    plan.run(src.data_ptr(), dst.data_ptr())
    lens, stat = plan.results()
    return dst, _streams(plan, dst, lens), stat


def _streams(plan, dst, lens):
    host = dst.cpu().numpy().tobytes()
    return [host[o:o + n] for o, n in zip(plan.out_offsets, lens)]


def _verify(plan, src, dst):
    assert plan.verify(src.data_ptr(), dst.data_ptr()) == 0
    return plan.verify_results()


def _check_clean(zsc_amd, oracle, plan, bufs, level, wbits, src, dst, streams, stat):
    assert stat == [0] * len(bufs)
    for i, (got, want) in enumerate(zip(streams, _oracle_streams(oracle, bufs, level, wbits))):
        assert got == want, (i, len(bufs[i]))
    res = _verify(plan, src, dst)
    assert res == [{"verdict": OK, "block": NONE, "bit_off": 0, "in_pos": 0}] * len(bufs)
    assert plan.verify_ms() > 0
    hdr = 0 if wbits < 0 else 10 if wbits > 15 else 2
    many = 0
    for i, b in enumerate(bufs):
        blocks = plan.verify_blocks(i)
        at = 0
        for k, (bit_off, in_begin, in_len, typ, last) in enumerate(blocks):
            assert in_begin == at and typ <= 2 and last == (k + 1 == len(blocks)), (i, k)
            assert bit_off < 8 * len(streams[i]) and (k > 0 or bit_off == 8 * hdr)
            at += in_len
        assert blocks and at == len(b), i
        assert [x[0] for x in blocks] == sorted(x[0] for x in blocks)
        many += len(blocks) > 1
    assert many


@pytest.mark.parametrize("level,wbits", PLANS)
def test_clean_batch(oracle, level, wbits):
    import torch
    import zsc_amd
    bufs = _buffers()
    assert 35 <= len(bufs) <= 45
    plan = zsc_amd.DeflatePlan([len(b) for b in bufs], level, wbits)
    try:
        plan.verify_enable()
        src = _upload(torch, plan, bufs)
        dst, streams, stat = _run(torch, plan, src)
        _check_clean(zsc_amd, oracle, plan, bufs, level, wbits, src, dst, streams, stat)
        # a second run of the same plan, and a second verification of it
        dst2, streams2, stat2 = _run(torch, plan, src)
        assert streams2 == streams
        assert [r["verdict"] for r in _verify(plan, src, dst2)] == [OK] * len(bufs)
        assert [r["verdict"] for r in _verify(plan, src, dst)] == [OK] * len(bufs)
    finally:
        plan.close()


def test_two_sub_batches(oracle, monkeypatch):
    """the block facts of sub-batch 0 must survive sub-batch 1's reuse of the records and plans"""
    import torch
    import zsc_amd
    bufs = _buffers()
    assert sum(len(b) for b in bufs) > 2 << 20
    monkeypatch.setenv("ZSC_HIP_SUBBATCH_MB", "1")
    plan = zsc_amd.DeflatePlan([len(b) for b in bufs], 6, 15)
    monkeypatch.delenv("ZSC_HIP_SUBBATCH_MB")
    try:
        assert plan.sub_batches >= 2
        plan.verify_enable()
        src = _upload(torch, plan, bufs)
        dst, streams, stat = _run(torch, plan, src)
        _check_clean(zsc_amd, oracle, plan, bufs, 6, 15, src, dst, streams, stat)
    finally:
        plan.close()


def test_with_the_index(oracle):
    """the index and verification on one plan: both work as they do alone"""
    import torch
    import zsc_amd
    bufs = _buffers()
    plan = zsc_amd.DeflatePlan([len(b) for b in bufs], 6, 15)
    try:
        plan.index_enable(8192)
        plan.verify_enable()
        src = _upload(torch, plan, bufs)
        dst, streams, stat = _run(torch, plan, src)
        _check_clean(zsc_amd, oracle, plan, bufs, 6, 15, src, dst, streams, stat)
        blobs = plan.export_indexes(src.data_ptr())
    finally:
        plan.close()
    caps = [len(b) for b in bufs]
    rc, outs, used, istat = zsc_amd.uncompress_indexed_batch(streams, caps, blobs, window_bits=15)
    assert rc == 0 and istat == [0] * len(bufs) and outs == bufs and used == [len(s) for s in streams]


@pytest.mark.parametrize("wbits", [-15, 31])
def test_damage_64_at_a_time(oracle, wbits):
    """one seeded bit flipped in 48 of 64 copies of a stream with many blocks, verified in one call"""
    import torch
    import zsc_amd
    from zsc_amd import corpus
    data = _mix(corpus, 70001, 300)
    copies = 64
    want = oracle.compress(data, 6, window_bits=wbits, mem_level=1)[1]
    trl = 0 if wbits < 0 else 8
    hdr = 0 if wbits < 0 else 10
    plan = zsc_amd.DeflatePlan([len(data)] * copies, 6, wbits, 1)
    try:
        plan.verify_enable()
        src = _upload(torch, plan, [data] * copies)
        dst, streams, stat = _run(torch, plan, src)
        assert stat == [0] * copies and streams == [want] * copies
        blocks = plan.verify_blocks(0)
        assert len(blocks) > 20 and all(plan.verify_blocks(i) == blocks for i in (1, copies - 1))
        rnd = random.Random(500 + wbits)
        flips = {}
        for i in range(copies):
            if i % 4:  # every fourth copy stays as it is
                bit = rnd.randrange(8 * len(want))
                flips[i] = bit
                dst[plan.out_offsets[i] + (bit >> 3)] ^= 1 << (bit & 7)
        res = _verify(plan, src, dst)
        damaged = _streams(plan, dst, [len(want)] * copies)
    finally:
        plan.close()
    starts = [b[0] for b in blocks]
    minded = 0
    for i in range(copies):
        verdict, block = res[i]["verdict"], res[i]["block"]
        if i not in flips:
            assert damaged[i] == want and (verdict, block) == (OK, NONE), i
            continue
        bit = flips[i]
        assert damaged[i] != want and sum(bin(a ^ b).count("1") for a, b in zip(damaged[i], want)) == 1
        rc, out, used = oracle.uncompress(damaged[i], len(data) + 64, window_bits=wbits)
        if rc == 0 and out == data and used == len(want):
            continue  # the decoder does not mind: either verdict is right
        minded += 1
        assert verdict not in (OK, SKIPPED), (i, bit)
        if bit < 8 * hdr:
            assert (verdict, block) == (HEADER, NONE), (i, bit, verdict, block)
        elif bit >= 8 * (len(want) - trl):
            assert (verdict, block) == (TRAILER, NONE), (i, bit, verdict, block)
        else:
            holder = max(k for k, s in enumerate(starts) if s <= bit)
            assert block == holder and verdict not in (HEADER, TRAILER), (i, bit, verdict, block, holder)
            assert res[i]["bit_off"] == starts[holder]
    assert minded > 40


def test_a_copy_elsewhere(oracle):
    import torch
    import zsc_amd
    bufs = _buffers()
    plan = zsc_amd.DeflatePlan([len(b) for b in bufs], 6, 31)
    try:
        plan.verify_enable()
        src = _upload(torch, plan, bufs)
        dst, streams, stat = _run(torch, plan, src)
        assert stat == [0] * len(bufs)
        clone = dst.clone()
        dst.zero_()
        assert [r["verdict"] for r in _verify(plan, src, clone)] == [OK] * len(bufs)
        # (zeros are not even the empty buffer's stream: its header is gone too)
        assert all(r["verdict"] not in (OK, SKIPPED) for r in _verify(plan, src, dst))
        assert [r["verdict"] for r in _verify(plan, src, clone)] == [OK] * len(bufs)
    finally:
        plan.close()


def test_not_enabled():
    import torch
    import zsc_amd
    bufs = _buffers()[:12]
    lens = [len(b) for b in bufs]
    # (a plan reports the blocks it holds, and a block from the library's cache may be larger than asked for:
    # with the cache empty two identical plans hold the same)
    zsc_amd.lib.zsc_hip_release_cached_memory()
    plain, other = zsc_amd.DeflatePlan(lens, 6, 15), zsc_amd.DeflatePlan(lens, 6, 15)
    try:
        before = plain.scratch_bytes
        assert other.scratch_bytes == before
        other.verify_enable()
        slots = sum(n // 16383 + 2 for n in lens)
        assert other.scratch_bytes >= before + 36 * slots + 52 * len(lens)
        assert plain.scratch_bytes == before
        src = _upload(torch, plain, bufs)
        dst, streams, stat = _run(torch, plain, src)
        assert stat == [0] * len(bufs)
        assert plain.verify(src.data_ptr(), dst.data_ptr()) == Z_STREAM_ERROR
        with pytest.raises(RuntimeError):
            plain.verify_results()
        with pytest.raises(RuntimeError):
            plain.verify_blocks(0)
        # an enabled plan before its first results(): nothing to verify yet
        assert other.verify(src.data_ptr(), dst.data_ptr()) == Z_STREAM_ERROR
    finally:
        plain.close()
        other.close()


def test_short_out_cap_is_skipped(oracle):
    """a buffer whose stream did not fit is SKIPPED and has no block map; its neighbours verify"""
    import ctypes as C
    import torch
    import zsc_amd
    from zsc_amd.api import VerifyBlock, VerifyResult, lib
    bufs = _buffers()[1:7]
    n = len(bufs)
    want = _oracle_streams(oracle, bufs, 6, 15)
    lens = (C.c_uint32 * n)(*[len(b) for b in bufs])
    in_off, out_off, caps = (C.c_uint64 * n)(), (C.c_uint64 * n)(), (C.c_uint32 * n)()
    ib, ob = C.c_uint64(), C.c_uint64()
    assert lib.zsc_hip_deflate_plan_layout(n, lens, 6, 15, 8, in_off, out_off, caps, C.byref(ib), C.byref(ob)) == 0
    short = 3
    caps[short] = len(want[short]) - 1
    h = C.c_void_p()
    assert lib.zsc_hip_deflate_plan_create(C.byref(h), n, lens, in_off, out_off, caps, 6, 15, 8, 0) == 0
    try:
        assert lib.zsc_hip_deflate_plan_verify_enable(h) == 0
        src = torch.zeros(ib.value, dtype=torch.uint8, device="cuda")
        for s, off in zip(bufs, in_off):
            src[off:off + len(s)] = torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda()
        dst = torch.zeros(ob.value, dtype=torch.uint8, device="cuda")
        assert lib.zsc_hip_deflate_plan_run(h, src.data_ptr(), dst.data_ptr(), None) == 0
        stat, out_lens = (C.c_int32 * n)(), (C.c_uint32 * n)()
        assert lib.zsc_hip_deflate_plan_results(h, out_lens, stat) == 0
        assert list(stat) == [-5 if i == short else 0 for i in range(n)]
        assert lib.zsc_hip_deflate_plan_verify(h, src.data_ptr(), dst.data_ptr(), None) == 0
        res = (VerifyResult * n)()
        assert lib.zsc_hip_deflate_plan_verify_results(h, res, None) == 0
        assert [r.verdict for r in res] == [SKIPPED if i == short else OK for i in range(n)]
        cnt = C.c_uint32(7)
        assert lib.zsc_hip_deflate_plan_verify_blocks(h, short, None, 0, C.byref(cnt)) == -3 and cnt.value == 0
        assert lib.zsc_hip_deflate_plan_verify_blocks(h, short + 1, None, 0, C.byref(cnt)) == -5 and cnt.value >= 1
        blocks = (VerifyBlock * cnt.value)()
        assert lib.zsc_hip_deflate_plan_verify_blocks(h, short + 1, blocks, cnt.value, C.byref(cnt)) == 0
        assert sum(b.in_len for b in blocks) == len(bufs[short + 1])
    finally:
        lib.zsc_hip_deflate_plan_destroy(h)


def test_compress_batch_verified(oracle):
    import zsc_amd
    bufs = [b for b in _buffers() if len(b) <= 20000][:10]
    assert len(bufs) == 10
    rc, streams, stat, verdicts = zsc_amd.compress_batch_verified(bufs, 6, 15, 8, 0)
    assert rc == 0 and stat == [0] * 10 and streams == _oracle_streams(oracle, bufs, 6, 15)
    assert [v["verdict"] for v in verdicts] == [zsc_amd.VERIFY_OK] * 10
