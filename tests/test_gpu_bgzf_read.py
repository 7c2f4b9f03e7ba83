"""The BGZF index and the ranges plan on the MI355X (zsc_amd/csrc/bgzf_read.h; include/zsc_hip.h, "BGZF ranges"),
through the C ABI as zsc_amd.BgzfIndex and zsc_amd.InflatePlan.bgzf_ranges call it, over the cases of
tests/bgzf_read_cases.py: tables equal to the walk over BSIZE fields, bytes equal to CPython's gzip.decompress of
the file, sliced.  Every destination lies in an output filled with a canary, and every byte outside a Z_OK
request's [offset, + dest_len) must keep it.
"""
import gzip
import struct

import numpy as np
import pytest

import bgzf_read_cases as bc
from bgzf_read_cases import Z_BUF_ERROR, Z_DATA_ERROR, Z_OK, Z_STREAM_ERROR, Request
from test_bgzf_read_emu import all_requests, voffset_requests

pytestmark = pytest.mark.gpu

CANARY = 0xEE
GZ = 31


def device_files(datas, filler="zeros", gap=0):
    """the files one behind the other on the device -> (tensor, lens, offsets); `filler` in every other byte, `gap`
    more bytes between the files"""
    import torch
    import zsc_amd
    lens = [len(d) for d in datas]
    offs, at = [], 0
    for n in lens:
        offs.append(at)
        at += ((n + 64 + 15) & ~15) + gap
    nbytes = at + 64
    if filler == "zeros":
        img = np.zeros(nbytes, dtype=np.uint8)
    elif filler == "ones":
        img = np.full(nbytes, 0xFF, dtype=np.uint8)
    else:
        img = np.random.default_rng(3).integers(0, 256, nbytes, dtype=np.uint8)
    for d, o in zip(datas, offs):
        img[o:o + len(d)] = np.frombuffer(d, dtype=np.uint8)
    assert zsc_amd.BgzfIndex.layout(lens)[0] == offs or gap
    return torch.from_numpy(img).cuda(), lens, offs


def read_ranges(index, d_src, reqs, voffsets=False, runs=1, streams=(0,), pack=False):
    """one ranges plan over the requests, run `runs` times, run k on streams[k % len(streams)]: [(status, dest_len,
    consumed, bytes or None)] and the plan's (jobs, decoded bytes); asserts that every run gave the same and that
    nothing outside the Z_OK requests' own bytes was written"""
    import torch
    import zsc_amd
    plan = zsc_amd.InflatePlan.bgzf_ranges(index, [r.file for r in reqs], [r.begin for r in reqs],
                                           [r.length for r in reqs], [r.cap for r in reqs], voffsets=voffsets)
    try:
        assert plan.index_enable() == Z_STREAM_ERROR and plan.dict_enable([b"abc"]) == Z_STREAM_ERROR
        if pack:
            plan.pack_enable(16)
        d_dst = torch.full((plan.dst_bytes,), CANARY, dtype=torch.uint8, device="cuda")
        seen = []
        for k in range(runs):
            stream = streams[k % len(streams)]
            d_dst.fill_(CANARY)
            torch.cuda.synchronize()
            if len(streams) > 1:
                # (a run on the other stream right in front of it, not waited for: the plan orders its runs itself)
                plan.run(d_src.data_ptr(), d_dst.data_ptr(), streams[(k + 1) % len(streams)])
            plan.run(d_src.data_ptr(), d_dst.data_ptr(), stream)
            lens, used, stat, _ = plan.results()
            assert plan.results()[:3] == (lens, used, stat)
            host = d_dst.cpu().numpy()
            mask = np.ones(len(host), dtype=bool)
            res = []
            for i, r in enumerate(reqs):
                off = plan.dst_offsets[i]
                out = None
                if stat[i] == Z_OK:
                    assert lens[i] <= r.cap
                    mask[off:off + lens[i]] = False
                    out = host[off:off + lens[i]].tobytes()
                elif stat[i] == Z_DATA_ERROR:
                    mask[off:off + r.cap] = False  # (unspecified inside its own destination)
                res.append((stat[i], lens[i], used[i], out))
            assert bool((host[mask] == CANARY).all()), "a byte outside the requests' own bytes was written"
            if pack:
                d_packed = torch.full((plan.dst_bytes,), CANARY, dtype=torch.uint8, device="cuda")
                plan.pack(d_dst.data_ptr(), d_packed.data_ptr(), plan.dst_bytes, stream)
                offs, total = plan.pack_results()
                image = d_packed.cpu().numpy()
                for i in range(len(reqs)):
                    n = lens[i] if stat[i] == Z_OK else 0
                    assert offs[i + 1] - offs[i] == (n + 15) // 16 * 16
                    assert image[offs[i]:offs[i] + n].tobytes() == (res[i][3] or b"")
            seen.append(res)
        assert all(s == seen[0] for s in seen)  # (the plan run again gives the same)
        return seen[0], plan.jobs()
    finally:
        plan.close()


def check(files, reqs, got, where=""):
    assert len(got) == len(reqs)
    for r, g in zip(reqs, got):
        st, n, used, data = bc.expected(files[r.file], r)
        assert g[:3] == (st, n, used), (where, files[r.file].name, r, g[:3], (st, n, used))
        if st == Z_OK:
            assert g[3] == data, (where, files[r.file].name, r)


@pytest.fixture(scope="module")
def ranged():
    """the range files on the device with their index, built once"""
    import zsc_amd
    files = bc.range_files()
    d_src, lens, offs = device_files([f.data for f in files])
    index = zsc_amd.BgzfIndex(d_src.data_ptr(), lens)
    yield files, d_src, index
    index.close()


def test_index_tables_gzi_and_offsets():
    import zsc_amd
    files = bc.index_files()
    d_src, lens, offs = device_files([f.data for f in files])
    index = zsc_amd.BgzfIndex(d_src.data_ptr(), lens)
    try:
        assert index.scratch_bytes() == 16 * sum(len(f.coff) for f in files)
        for i, f in enumerate(files):
            assert index.table(i) == (f.coff, f.uoff), f.name
            assert index.info(i) == (len(f.coff) - 1, f.coff[-1], f.uoff[-1]), f.name
            image = index.to_gzi(i)
            assert image == bc.gzi(f), f.name
            back = zsc_amd.BgzfIndex.from_gzi(image, d_src.data_ptr(), lens[i], offs[i])
            assert back.table() == (f.coff, f.uoff) and back.info() == index.info(i), f.name
            back.close()
            us = list(f.uoff) + [u1 - 1 for u0, u1 in zip(f.uoff, f.uoff[1:]) if u1 > u0]
            for u in us:
                v = index.voffset(u, i)
                assert v == bc.to_voffset(f, u) and index.uoffset(v, i) == u, (f.name, u)
            for k in range(len(f.coff) - 1):
                assert index.uoffset(f.coff[k] << 16, i) == f.uoff[k]
            with pytest.raises(ValueError):
                index.voffset(f.uoff[-1] + 1, i)
            with pytest.raises(ValueError):
                index.uoffset((f.coff[-1] << 16) + 1, i)
        by = {f.name: i for i, f in enumerate(files)}
        assert index.info(by["plain-gzip"])[0] == 0 and index.info(by["empty"]) == (0, 0, 0)
        assert index.info(by["bsize-altered"])[0] == 1 and index.info(by["nested"])[0] == 4
        assert index.info(by["garbage"])[1] == index.info(by["padded"])[1] == len(files[by["padded"]].data) - 100
        # imports that do not fit the file
        s, image = by["sizes"], bc.gzi(files[by["sizes"]])
        n = struct.unpack_from("<Q", image)[0]
        moved = bytearray(image)
        moved[8 + 16 * 3] ^= 1
        left_out = struct.pack("<Q", n - 1) + image[8:8 + 16 * 4] + image[8 + 16 * 5:]
        for bad, where in ((bytes(moved), s), (left_out, s), (image, by["padded"]), (image[:-1], s)):
            with pytest.raises(ValueError):
                zsc_amd.BgzfIndex.from_gzi(bad, d_src.data_ptr(), lens[where], offs[where])
    finally:
        index.close()


def test_ranges_in_one_plan(ranged):
    files, d_src, index = ranged
    reqs = all_requests(files)
    assert len(reqs) >= 4 * 64
    got, (jobs, decoded) = read_ranges(index, d_src, reqs, runs=2, pack=True)
    check(files, reqs, got)
    assert jobs > len(reqs) and {g[0] for g in got} == {Z_OK, Z_BUF_ERROR}


def test_the_index_may_be_destroyed_before_the_run():
    import zsc_amd
    files = bc.range_files()[:2]
    d_src, lens, _ = device_files([f.data for f in files])
    index = zsc_amd.BgzfIndex(d_src.data_ptr(), lens)
    reqs = all_requests(files)[::5]
    plan = zsc_amd.BgzfRangesPlan(index, [r.file for r in reqs], [r.begin for r in reqs], [r.length for r in reqs],
                                  [r.cap for r in reqs])
    index.close()
    import torch
    d_dst = torch.zeros(plan.dst_bytes, dtype=torch.uint8, device="cuda")
    plan.run(d_src.data_ptr(), d_dst.data_ptr())
    lens_, used, stat, _ = plan.results()
    host = d_dst.cpu().numpy()
    got = [(stat[i], lens_[i], used[i], host[plan.dst_offsets[i]:plan.dst_offsets[i] + lens_[i]].tobytes()
            if stat[i] == Z_OK else None) for i in range(len(reqs))]
    plan.close()
    check(files, reqs, got)


def test_ranges_by_virtual_offsets(ranged):
    import zsc_amd
    files, d_src, index = ranged
    plain = [r for r in all_requests(files) if r.begin + r.length <= files[r.file].uoff[-1]]
    got, _ = read_ranges(index, d_src, voffset_requests(files, plain), voffsets=True)
    check(files, plain, got)
    f = files[0]
    k = next(k for k in range(len(f.coff) - 1) if f.uoff[k + 1] - f.uoff[k] == 15)
    for begin, end in (((f.coff[k] + 1) << 16, f.coff[k + 1] << 16),     # no member start
                       (f.coff[k] << 16, f.coff[k] << 16 | 16),          # beyond the member's length
                       (f.coff[-1] << 16 | 1, f.coff[-1] << 16 | 1),     # within the end entry
                       (f.coff[k] << 16 | 5, f.coff[k] << 16 | 4),       # end < begin
                       (f.coff[k + 1] << 16, f.coff[k] << 16)):
        with pytest.raises(ValueError):
            zsc_amd.InflatePlan.bgzf_ranges(index, [0], [begin], [end], [99], voffsets=True)
    with pytest.raises(ValueError):
        zsc_amd.InflatePlan.bgzf_ranges(index, [len(files)], [0], [1], [1])  # no such file


def test_staging_slots_are_reused(ranged, monkeypatch):
    """more edge jobs than lane groups: four groups, so one wavefront, take every job of the plan"""
    files, d_src, index = ranged
    reqs = all_requests(files)
    monkeypatch.setenv("ZSC_HIP_BGZF_GROUPS", "4")  # (read when the plan is created)
    got, _ = read_ranges(index, d_src, reqs)
    check(files, reqs, got)


def test_damage_fails_only_the_requests_that_touch_it():
    import torch
    import zsc_amd
    cases = bc.damage_cases()
    # one index over the files as they are indexed, then the late flips, then one plan over all of them
    d_src, lens, offs = device_files([data for _, data, _, _ in cases])
    index = zsc_amd.BgzfIndex(d_src.data_ptr(), lens)
    try:
        for i, (name, data, flips, f) in enumerate(cases):
            assert index.table(i) == (f.coff, f.uoff), name
            for pos, x in flips:
                d_src[offs[i] + pos] ^= x
        torch.cuda.synchronize()
        files = [f for _, _, _, f in cases]
        reqs = all_requests(files)
        got, _ = read_ranges(index, d_src, reqs, runs=2)
        check(files, reqs, got)
        kinds = [g[0] for g in got]
        assert kinds.count(Z_DATA_ERROR) > 40 and kinds.count(Z_OK) > 40
    finally:
        index.close()


def test_tiles_equal_the_members_plan():
    """knows no right answers: adjacent ranges that tile [0, total_out) concatenate to what the members plan
    writes, for tiles of 1, 4 096 and 100 000 bytes"""
    import torch
    import zsc_amd
    data, content = bc.tiles_file()
    d_src, lens, _ = device_files([data])
    total = len(content)
    mplan = zsc_amd.InflatePlan(lens, [total], window_bits=GZ, members=True)
    d_out = torch.zeros(mplan.dst_bytes, dtype=torch.uint8, device="cuda")
    mplan.run(d_src.data_ptr(), d_out.data_ptr())
    mlens, mused, mstat, _ = mplan.results()
    assert (mstat[0], mlens[0], mused[0]) == (Z_OK, total, len(data)) and mplan.sections()[0] == mplan.members()[0][0]
    whole = d_out.cpu().numpy()[:total]
    mplan.close()
    index = zsc_amd.BgzfIndex(d_src.data_ptr(), lens)
    try:
        assert index.info()[2] == total
        for tile in (1, 4096, 100000):
            begins = list(range(0, total, tile))
            sizes = [min(tile, total - b) for b in begins]
            # (destinations one behind the other without gaps: the tiles land where the members plan puts them)
            if tile % 16 == 0:
                dsts = begins
                step = 1
            else:
                dsts = [16 * k for k in range(len(begins))]
                step = 16
            plan = zsc_amd.InflatePlan.bgzf_ranges(index, [0] * len(begins), begins, sizes, sizes, dst_offsets=dsts)
            d_dst = torch.full((plan.dst_bytes,), CANARY, dtype=torch.uint8, device="cuda")
            plan.run(d_src.data_ptr(), d_dst.data_ptr())
            rl, ru, rs, _ = plan.results()
            plan.close()
            assert set(rs) == {Z_OK} and rl == sizes, tile
            host = d_dst.cpu().numpy()
            if step == 1:
                assert np.array_equal(host[:total], whole), tile
                assert bool((host[total:] == CANARY).all()), tile
            else:
                assert np.array_equal(host[:16 * len(begins)].reshape(-1, 16)[:, 0], whole), tile
                assert bool((host[:16 * len(begins)].reshape(-1, 16)[:, 1:] == CANARY).all()), tile
    finally:
        index.close()


def test_results_depend_on_the_request_alone(ranged):
    """in the manner of tests/surroundings.py: not on the other requests of the plan, not on the bytes around the
    file, not on the stream of a second run"""
    import torch
    import zsc_amd
    files, d_src, index = ranged
    reqs = all_requests(files)
    together, _ = read_ranges(index, d_src, reqs)
    some = reqs[7::11]
    alone, _ = read_ranges(index, d_src, some)
    assert alone == together[7::11]
    side = torch.cuda.Stream()
    # one plan on stream 0, then on the side stream, then on stream 0 again: the queue, the requests' marks and
    # the staging slots are the plan's, shared by its runs
    other, _ = read_ranges(index, d_src, some, streams=(0, side.cuda_stream), runs=3)
    assert other == alone
    whole, _ = read_ranges(index, d_src, reqs, streams=(side.cuda_stream, 0), runs=2, pack=True)
    assert whole == together
    for filler in ("ones", "noise"):
        d_hostile, lens, offs = device_files([f.data for f in files], filler=filler, gap=48)
        hostile = zsc_amd.BgzfIndex(d_hostile.data_ptr(), lens, offs)
        try:
            for i, f in enumerate(files):
                assert hostile.table(i) == (f.coff, f.uoff), (filler, f.name)
            got, _ = read_ranges(hostile, d_hostile, some)
            assert got == alone, filler
        finally:
            hostile.close()


def test_other_plan_kinds_in_the_same_process(ranged):
    """a plain, a members and a check plan made and run between two ranges plans give what they give"""
    import torch
    import zsc_amd
    files, d_src, index = ranged
    reqs = all_requests(files)[::7]
    first, _ = read_ranges(index, d_src, reqs)
    f = files[0]
    content = gzip.decompress(f.data)
    streams = [bc.gz(bc._bytes(5000, 1)), bc.gz(bc._bytes(70000, 2))]
    rc, outs, used, stat = zsc_amd.uncompress_batch(streams, [5000, 70000], window_bits=GZ)
    assert rc == 0 and stat == [0, 0] and outs == [bc._bytes(5000, 1), bc._bytes(70000, 2)]
    rc, outs, used, stat, members = zsc_amd.uncompress_members_batch([f.data], [len(content)])
    assert rc == 0 and stat == [0] and outs == [content] and members == [len(f.coff) - 1]
    rc, sizes, used, stat, values = zsc_amd.uncompress_check_batch(streams, window_bits=GZ)
    assert rc == 0 and stat == [0, 0] and sizes == [5000, 70000]
    assert values == [struct.unpack("<I", s[-8:-4])[0] for s in streams]
    again, _ = read_ranges(index, d_src, reqs)
    assert again == first
    check(files, reqs, again)


def test_host_batch_and_the_writer_round_trip():
    """zsc_amd.bgzf_read_ranges over files the BGZF writer made from a gzip deflate plan"""
    import zsc_amd
    contents = [bc._bytes(200000, 81), bc._bytes(1, 82), b"", bc._bytes(65280 * 2, 83)]
    images, stat = zsc_amd.bgzf_compress_batch(contents, level=6)
    assert list(stat) == [0] * len(contents)
    assert [gzip.decompress(i) for i in images] == contents
    reqs = []
    for i, c in enumerate(contents):
        n = len(c)
        reqs += [(i, 0, n), (i, n // 2, 70000), (i, max(n - 1, 0), 1), (i, 65279, 3), (i, n, 4), (i, 65280, 65280)]
    caps = [min(r[2], 70000) for r in reqs]
    rc, outs, lens, stat = zsc_amd.bgzf_read_ranges(images, reqs, caps)
    assert rc == 0
    for (i, b, n), cap, out, ln, st in zip(reqs, caps, outs, lens, stat):
        want = contents[i][b:b + n]
        if len(want) > cap:
            assert (st, ln, out) == (Z_BUF_ERROR, len(want), b""), (i, b, n)
        else:
            assert (st, ln, out) == (Z_OK, len(want), want), (i, b, n)
    # and by virtual offsets of the writer's own member table: member k of file 0 starts at 65 280 k
    walk = bc.claim_walk(images[0])
    v = [(0, walk[0][1] << 16 | 5, walk[0][2] << 16 | 7)]
    rc, outs, lens, stat = zsc_amd.bgzf_read_ranges(images, v, [65536], voffsets=True)
    assert (rc, stat, outs) == (0, [Z_OK], [contents[0][65280 + 5:65280 * 2 + 7]])
