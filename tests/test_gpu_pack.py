"""Packing a plan's results into one image on the GPU (zsc_amd/csrc/pack.h, include/zsc_hip.h "packed images"):
the image of a deflate plan is the oracle's streams one after the other, a failed item takes no room, a short
image is not touched, an image packed with align 16 is an inflate plan's input as it lies, a damaged stream's
salvaged bytes are kept, the host calls give what the pointer batches give, and a plan that never enables
packing is what it always was."""
import gzip
import os
import re
import zlib

import pytest

from test_gpu_deflate_verify import _buffers, _oracle_streams, _upload

pytestmark = pytest.mark.gpu

PLANS = [(6, 15), (1, 31), (9, -15)]
CANARY = 0xC7
Z_STREAM_ERROR, Z_BUF_ERROR = -2, -5
HERE = os.path.dirname(os.path.abspath(__file__))


def _up(n, align):
    return (n + align - 1) // align * align


def _run(torch, plan, src):
    dst = torch.zeros(plan.out_bytes, dtype=torch.uint8, device="cuda")
    plan.run(src.data_ptr(), dst.data_ptr())
    return dst


def _pack(torch, plan, d_out, cap, spare=64):
    """(the image's tensor with `spare` canary bytes behind cap, offsets, total)"""
    img = torch.full((cap + spare,), CANARY, dtype=torch.uint8, device="cuda")
    assert plan.pack(d_out.data_ptr(), img.data_ptr(), cap) == 0
    off, total = plan.pack_results()
    assert off[0] == 0 and off[-1] == total and plan.pack_ms() > 0
    return img, off, total


def _check_image(host, off, total, items, align):
    """item i at off[i], zeros up to the next multiple of align, canary from total on"""
    at = 0
    for i, want in enumerate(items):
        assert off[i] == at and off[i] % align == 0, i
        assert host[at:at + len(want)] == want, (i, len(want))
        at = _up(at + len(want), align) if align > 1 else at + len(want)
        assert host[off[i] + len(want):at] == bytes(at - off[i] - len(want)), i
    assert at == total == off[len(items)]
    assert host[total:] == bytes([CANARY]) * (len(host) - total), "written at or behind total"


def _walk(image, wbits):
    """the members of a concatenation of zlib or raw streams, decoded one after the other"""
    outs, rest = [], image
    while rest:
        d = zlib.decompressobj(wbits)
        outs.append(d.decompress(rest))
        assert d.eof
        rest = d.unused_data
    return outs


@pytest.mark.parametrize("align", [1, 16])
@pytest.mark.parametrize("level,wbits", PLANS)
def test_deflate_plan_packs_the_oracles_streams(oracle, level, wbits, align):
    import torch
    import zsc_amd
    bufs = _buffers()
    assert 35 <= len(bufs) <= 45
    want = _oracle_streams(oracle, bufs, level, wbits)
    plan = zsc_amd.DeflatePlan([len(b) for b in bufs], level, wbits)
    try:
        plan.pack_enable(align)
        src = _upload(torch, plan, bufs)
        dst = _run(torch, plan, src)
        # after the run on the same stream, with no results() in between ...
        img, off, total = _pack(torch, plan, dst, plan.out_bytes)
        host = img.cpu().numpy().tobytes()
        _check_image(host, off, total, want, align)
        assert plan.results()[1] == [0] * len(bufs)
        # ... and again after results(), from a copy of the output
        img2, off2, total2 = _pack(torch, plan, dst.clone(), total)
        assert (off2, total2) == (off, total) and img2.cpu().numpy().tobytes()[:total] == host[:total]
        if align == 1:
            image = host[:total]
            if wbits > 15:
                assert gzip.decompress(image) == b"".join(bufs)
            else:
                assert _walk(image, wbits) == bufs
    finally:
        plan.close()


def test_a_failed_item_takes_no_room_and_a_short_image_is_not_touched(oracle):
    import torch
    import zsc_amd
    bufs = _buffers()
    want = list(_oracle_streams(oracle, bufs, 6, 15))
    k = max(range(len(bufs)), key=lambda i: len(want[i]))
    full = zsc_amd.DeflatePlan([len(b) for b in bufs], 6, 15)
    caps = list(full.out_caps)
    full.close()
    caps[k] = len(want[k]) // 2
    plan = zsc_amd.DeflatePlan([len(b) for b in bufs], 6, 15, out_caps=caps)
    try:
        plan.pack_enable(1)
        src = _upload(torch, plan, bufs)
        dst = _run(torch, plan, src)
        stat = plan.results()[1]
        assert stat == [Z_BUF_ERROR if i == k else 0 for i in range(len(bufs))]
        want[k] = b""
        img, off, total = _pack(torch, plan, dst, plan.out_bytes)
        assert off[k + 1] == off[k]
        _check_image(img.cpu().numpy().tobytes(), off, total, want, 1)
        # one byte short: the total all the same, and nothing written
        short = torch.full((total + 64,), CANARY, dtype=torch.uint8, device="cuda")
        assert plan.pack(dst.data_ptr(), short.data_ptr(), total - 1) == 0
        with pytest.raises(BufferError) as e:
            plan.pack_results()
        assert e.value.total == total and e.value.offsets == off
        assert bool((short == CANARY).all())
    finally:
        plan.close()


def test_scan_across_workgroups(oracle):
    """2 B + 1 empty and one-byte buffers, raw: the offsets come from three waves of the scan's lowest level"""
    import torch
    import zsc_amd
    text = open(os.path.join(HERE, "..", "zsc_amd", "csrc", "pack.h")).read()
    B = int(re.search(r"#define PK_SCAN_B (\d+)u", text).group(1))
    count = 2 * B + 1
    bufs = [b"" if i % 3 == 0 else bytes([i % 251]) for i in range(count)]
    memo = {}
    for b in set(bufs):
        memo[b] = oracle.compress(b, 6, window_bits=-15)[1]
    want = [memo[b] for b in bufs]
    assert len(memo[b""]) == 2
    plan = zsc_amd.DeflatePlan([len(b) for b in bufs], 6, -15)
    try:
        plan.pack_enable(1)
        dst = _run(torch, plan, _upload(torch, plan, bufs))
        img, off, total = _pack(torch, plan, dst, plan.out_bytes)
        _check_image(img.cpu().numpy().tobytes(), off, total, want, 1)
    finally:
        plan.close()


@pytest.mark.parametrize("level,wbits", PLANS)
def test_an_aligned_image_feeds_an_inflate_plan(oracle, level, wbits):
    import torch
    import zsc_amd
    bufs = _buffers()
    want = _oracle_streams(oracle, bufs, level, wbits)
    plan = zsc_amd.DeflatePlan([len(b) for b in bufs], level, wbits)
    try:
        plan.pack_enable(16)
        dst = _run(torch, plan, _upload(torch, plan, bufs))
        need = sum(_up(len(s), 16) for s in want)
        img, off, total = _pack(torch, plan, dst, need)  # (64 readable bytes behind it)
        assert total == need
    finally:
        plan.close()
    ip = zsc_amd.InflatePlan([len(s) for s in want], [len(b) for b in bufs], window_bits=wbits, src_offsets=off[:-1])
    try:
        ip.pack_enable(1)
        out = torch.full((ip.dst_bytes,), 0xEE, dtype=torch.uint8, device="cuda")
        ip.run(img.data_ptr(), out.data_ptr())  # the image as it lies: no copy in between
        lens, used, stat, _ = ip.results()
        assert stat == [0] * len(bufs) and used == [len(s) for s in want] and lens == [len(b) for b in bufs]
        host = out.cpu().numpy().tobytes()
        assert [host[o:o + n] for o, n in zip(ip.dst_offsets, lens)] == bufs
        joined, joff, jtotal = _pack(torch, ip, out, sum(lens))
        assert joined.cpu().numpy().tobytes()[:jtotal] == b"".join(bufs)
        assert [b - a for a, b in zip(joff, joff[1:])] == lens
    finally:
        ip.close()


def test_the_salvaged_bytes_of_a_damaged_stream_are_kept():
    """a resync plan over clean and damaged full-flush streams: every packed item is the dest_len bytes the
    plan reports, whatever the status"""
    import torch
    import zsc_amd
    from test_inflate_resync_emu import constructed_cases
    group = [c for c in constructed_cases() if c[3] == 15][:6]
    assert any(c[4][0] == -3 for c in group)
    streams, caps = [c[1] for c in group], [c[2] for c in group]
    ip = zsc_amd.InflatePlan([len(s) for s in streams], caps, window_bits=15, resync=True)
    try:
        ip.pack_enable(1)
        src = torch.zeros(ip.src_bytes, dtype=torch.uint8, device="cuda")
        for s, o in zip(streams, ip.src_offsets):
            src[o:o + len(s)] = torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda()
        out = torch.full((ip.dst_bytes,), 0xEE, dtype=torch.uint8, device="cuda")
        ip.run(src.data_ptr(), out.data_ptr())
        lens, used, stat, _ = ip.results()
        host = out.cpu().numpy().tobytes()
        outs = [host[o:o + n] for o, n in zip(ip.dst_offsets, lens)]
        for (name, _, _, _, (st, want, consumed, _, _)), o, s, u in zip(group, outs, stat, used):
            assert (s, o, u) == (st, want, consumed), name
        img, off, total = _pack(torch, ip, out, sum(caps))
        _check_image(img.cpu().numpy().tobytes(), off, total, outs, 1)
    finally:
        ip.close()


@pytest.mark.parametrize("level,wbits", PLANS)
def test_host_calls_give_what_the_pointer_batches_give(level, wbits):
    import zsc_amd
    bufs = _buffers()
    rc, streams, stat = zsc_amd.compress_batch(bufs, level, wbits)
    assert rc == 0
    for align in (1, 16):
        image, off, pstat = zsc_amd.compress_batch_packed(bufs, level, wbits, align=align)
        assert pstat == stat
        assert [image[off[i]:off[i] + len(s)] for i, s in enumerate(streams)] == streams
        assert all(o % align == 0 for o in off) and off[-1] == len(image)
        if align == 1:
            assert image == b"".join(streams)
    # and back: the streams plus one truncated and one with a damaged trailer (a raw stream has none: its
    # last byte goes instead)
    big = max(range(len(bufs)), key=lambda i: len(streams[i]))
    bad = bytearray(streams[big])
    bad[-1] ^= 0x55
    items = list(streams) + [streams[big][:len(streams[big]) // 2], bytes(bad)]
    caps = [len(b) for b in bufs] + [len(bufs[big])] * 2
    rc, outs, used, istat = zsc_amd.uncompress_batch(items, caps, wbits)
    assert rc == 0 and istat[:len(bufs)] == [0] * len(bufs) and istat[-2] != 0
    starts, at = [], 0
    for s in items:
        starts.append(at)
        at += len(s)
    for align in (1, 16):
        oimg, ooff, dlen, pused, pistat = zsc_amd.uncompress_batch_packed(b"".join(items), starts, [len(s) for s in items],
                                                                         caps, wbits, align=align)
        assert (pistat, pused, dlen) == (istat, used, [len(o) for o in outs])
        assert [oimg[ooff[i]:ooff[i] + n] for i, n in enumerate(dlen)] == outs
    # a round trip through both calls with align 1: the archive is the second call's input as it is
    image, off, _ = zsc_amd.compress_batch_packed(bufs, level, wbits, align=1)
    back, boff, dlen, _, bstat = zsc_amd.uncompress_batch_packed(image, off, [b - a for a, b in zip(off, off[1:])],
                                                                 [len(b) for b in bufs], wbits, align=1)
    assert bstat == [0] * len(bufs) and back == b"".join(bufs) and dlen == [len(b) for b in bufs]


def test_host_calls_refuse_level_0_and_a_bad_align():
    import zsc_amd
    with pytest.raises(zsc_amd.PackedCallError) as e:
        zsc_amd.compress_batch_packed([b"abc"], level=0)
    assert e.value.rc == Z_STREAM_ERROR
    for align in (0, 3, 8192):
        with pytest.raises(zsc_amd.PackedCallError) as e:
            zsc_amd.compress_batch_packed([b"abc"], align=align)
        assert e.value.rc == Z_STREAM_ERROR
    # a destination that is too small: Z_BUF_ERROR, and the offsets say what it takes
    with pytest.raises(zsc_amd.PackedCallError) as e:
        zsc_amd.compress_batch_packed([b"abc" * 100, b"x"], dest_cap=4)
    assert e.value.rc == Z_BUF_ERROR and e.value.offsets[-1] > 4


def test_unpack_writes_the_items_and_nothing_else():
    import torch
    import zsc_amd
    lens = [0, 1, 2, 15, 16, 17, 33, 5000, 3 * zsc_amd.PACK_TILE + 5, 2, 2, 0, 7]
    data = [bytes((7 * i + j) % 255 + 1 for j in range(n)) for i, n in enumerate(lens)]
    offs, at = [], 3  # (three bytes of something else in front)
    for d in data:
        offs.append(at)
        at += len(d) + (1 if len(d) % 2 else 0)
    image = bytearray(at)
    for o, d in zip(offs, data):
        image[o:o + len(d)] = d
    slots, at = [], 0
    for d in data:
        slots.append(at)
        at += _up(len(d), 16) + 32
    d_img = torch.frombuffer(image, dtype=torch.uint8).cuda()
    d_dst = torch.full((at,), CANARY, dtype=torch.uint8, device="cuda")
    assert zsc_amd.unpack(d_img.data_ptr(), offs, lens, d_dst.data_ptr(), slots) == 0
    torch.cuda.synchronize()
    want = bytearray([CANARY]) * at
    for s, d in zip(slots, data):
        want[s:s + len(d)] = d
    assert d_dst.cpu().numpy().tobytes() == bytes(want)
    assert zsc_amd.unpack(d_img.data_ptr(), offs, lens, d_dst.data_ptr(), [s + 8 for s in slots]) == Z_STREAM_ERROR
    assert zsc_amd.unpack(d_img.data_ptr(), offs[::-1], lens, d_dst.data_ptr(), slots) == Z_STREAM_ERROR


def test_a_plan_without_packing_is_unchanged(oracle):
    import torch
    import zsc_amd
    bufs = _buffers()
    want = _oracle_streams(oracle, bufs, 6, 15)
    # (a plan reports the blocks it holds, and a block from the library's cache may be larger than asked for:
    # with the cache empty two identical plans hold the same)
    zsc_amd.lib.zsc_hip_release_cached_memory()
    plain = zsc_amd.DeflatePlan([len(b) for b in bufs], 6, 15)
    packed = zsc_amd.DeflatePlan([len(b) for b in bufs], 6, 15)
    try:
        base = plain.scratch_bytes
        assert packed.scratch_bytes == base
        packed.verify_enable()
        packed.index_enable()
        with_checks = packed.scratch_bytes
        packed.pack_enable(16)
        assert packed.scratch_bytes >= with_checks + 16 * len(bufs) + 8 and plain.scratch_bytes == base
        with pytest.raises(ValueError):
            packed.pack_enable(24)
        outs = []
        for plan in (plain, packed):
            src = _upload(torch, plan, bufs)
            dst = _run(torch, plan, src)
            lens, stat = plan.results()
            host = dst.cpu().numpy().tobytes()
            outs.append(([host[o:o + n] for o, n in zip(plan.out_offsets, lens)], stat))
        assert outs[0] == outs[1] == (want, [0] * len(bufs))
        # never enabled: Z_STREAM_ERROR, from the pack and from its results
        img = torch.full((plain.out_bytes,), CANARY, dtype=torch.uint8, device="cuda")
        assert plain.pack(dst.data_ptr(), img.data_ptr(), plain.out_bytes) == Z_STREAM_ERROR
        with pytest.raises(RuntimeError):
            plain.pack_results()
        assert bool((img == CANARY).all()) and plain.scratch_bytes == base
        # the index and the verification of a plan that packs: still about the plan's own offsets
        pimg, off, total = _pack(torch, packed, dst, packed.out_bytes)
        _check_image(pimg.cpu().numpy().tobytes(), off, total, want, 16)
        assert packed.verify(src.data_ptr(), dst.data_ptr()) == 0
        assert [r["verdict"] for r in packed.verify_results()] == [0] * len(bufs)
        blobs = packed.export_indexes(src.data_ptr())
        for blob, s, b in zip(blobs, want, bufs):
            info = zsc_amd.index_info(blob)
            assert (info["consumed"], info["total_out"]) == (len(s), len(b))
    finally:
        plain.close()
        packed.close()
