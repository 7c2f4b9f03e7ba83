"""ZIP archives from a gzip deflate plan on the GPU (zsc_amd/csrc/zip.h, include/zsc_hip.h "ZIP archives").

One plan of about 140 buffers in about 75 archives at level 6, mem_level 8, run once and written once (module
fixture `main`); the tests look at that one image.  What an archive must be comes from the oracle alone: its
gzip streams, of which tests/zip_cases.py takes S[10:-8] and the trailer, and the format restated there.

A plan has one level, so the main plan holds the buffers tests/golden/bgzf_golden.json records at (6, 8); its
other (level, mem_level) pairs are a parametrised test of small plans.

Real streams reach the tile borders through stored blocks: a random buffer of n < 16 383 bytes gives a body of
n + 5 bytes, and the name lengths do the rest -- a local header k bytes before a border for every k it has bytes
(one archive of 30 entries, a border each), and a directory record and an end record likewise (an archive per k).

Not reachable from here: the refusal of a plan of sections (no public call hands one out), and an archive
longer than 4 294 967 295 bytes (tests/test_zip_emu.py fabricates one).
"""
import io
import json
import os
import random
import zipfile
import zlib

import pytest

from zip_cases import (DIR, END, END64, LOCAL, TILE, Z_BUF_ERROR, Z_MEM_ERROR, Z_OK, Z_STREAM_ERROR, expected, walk)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GZ = 31
CANARY = 0xC7
ALIGN = 16
STORED = 5  # a stored block's header: what a random buffer's body is longer than the buffer
_RANDOM = random.Random(5).randbytes(70000)
_memo = {}


def golden():
    if "golden" not in _memo:
        _memo["golden"] = json.load(open(os.path.join(HERE, "golden", "bgzf_golden.json")))["members"]
    return _memo["golden"]


def golden_buffer(rec):
    from zsc_amd import corpus
    return corpus.make_buffer(rec["kind"], rec["size"], rec["seed"])


def stream(oracle, buf, level=6, mem_level=8):
    key = (bytes(buf), level, mem_level)
    if key not in _memo:
        rc, s, _ = oracle.compress(buf, level, window_bits=GZ, mem_level=mem_level)
        assert rc == 0
        _memo[key] = s
    return _memo[key]


def rnd(at, n):
    return _RANDOM[at:at + n]


def main_archives():
    """[(title, [(name, buffer)])]; built once"""
    if "archives" in _memo:
        return _memo["archives"]
    from zsc_amd import corpus
    six = [r for r in golden() if (r["level"], r["mem_level"]) == (6, 8)]
    assert len(six) == 18
    arch = [("empty-first", []),
            ("golden-mix", [(b"golden/%s-%d.bin" % (r["kind"].encode(), r["size"]), golden_buffer(r)) for r in six])]
    # local headers: entry j + 1 starts k bytes before border j + 1, k = 1 .. 29; the names take what is left
    entries, at = [], 0
    for k in range(1, LOCAL):
        nl = k % 7
        n = k * TILE - k - at - LOCAL - nl - STORED
        assert n < 16383
        entries.append((bytes(97 + (k + j) % 26 for j in range(nl)), rnd(k, n)))
        at += LOCAL + nl + n + STORED
    entries.append((b"behind-the-last-border", corpus.make_buffer("text", 100, 3)))
    arch.append(("local-headers-at-borders", entries))
    for k in range(1, DIR):
        nl = k % 5
        arch.append((f"dir-at-border-minus-{k}", [(b"d" * nl, rnd(100 + k, TILE - k - LOCAL - nl - STORED))]))
    arch.append(("empty-between", []))
    for k in range(1, END):
        nl = 3 + k % 4
        arch.append((f"end-at-border-minus-{k}", [(b"e" * nl, rnd(200 + k, TILE - k - LOCAL - DIR - 2 * nl - STORED))]))
    arch += [("name-cut-by-border", [(b"ab", rnd(7, TILE - 35 - LOCAL - 2 - STORED)), (b"0123456789abcdefghij", b"x" * 77)]),
             ("long-names", [(bytes(65 + j % 26 for j in range(n)), corpus.make_buffer("text", 300 + n % 50, n))
                             for n in (0, 1, 15, 16, 17, 65535)]),
             ("names-around-the-lane-limit", [(bytes(97 + j % 26 for j in range(n)), corpus.make_buffer("text", 2000 + n, n))
                                              for n in (127, 128, 129, 300)]),
             ("twenty-small",[(b"s/%02d" % j, corpus.make_buffer("text", (37 * j) % 700, 200 + j)) for j in range(20)]),
             ("empty-last", [])]
    assert 120 <= sum(len(e) for _, e in arch) <= 160
    _memo["archives"] = arch
    return arch


def flatten(archives):
    names, bufs, first = [], [], [0]
    for _, entries in archives:
        for nm, b in entries:
            names.append(nm)
            bufs.append(b)
        first.append(len(bufs))
    return names, bufs, first


def upload(torch, plan, bufs):
    image = bytearray(plan.in_bytes)
    for b, off in zip(bufs, plan.in_offsets):
        image[off:off + len(b)] = b
    return torch.frombuffer(image, dtype=torch.uint8).cuda()


def write_archives(torch, plan, d_out, cap, stream=0):
    img = torch.full((cap + 64,), CANARY, dtype=torch.uint8, device="cuda")
    assert plan.zip(d_out.data_ptr(), img.data_ptr(), cap, stream) == 0
    return img


def image_cap(plan, names, first, align):
    na = len(first) - 1
    return sum(c + LOCAL + DIR + 2 * len(nm) for c, nm in zip(plan.out_caps, names)) + (END64 + align) * na


def run_plan(archives, level=6, mem_level=8, align=ALIGN, out_caps=None, datetimes=None, utf8=False, keep=False):
    """one plan, one run, one zip(): (host image with its canary, tables, statuses of the buffers, cap)"""
    import torch
    import zsc_amd
    names, bufs, first = flatten(archives)
    plan = zsc_amd.DeflatePlan([len(b) for b in bufs], level, GZ, mem_level, out_caps=out_caps)
    try:
        before = plan.scratch_bytes
        plan.zip_enable(first, names, datetimes, utf8, align)
        # 44 bytes per buffer, 36 per archive, the names, 8 for the sums (rounded up by the allocator: at least that)
        assert plan.scratch_bytes - before >= 44 * len(bufs) + 36 * (len(first) - 1) + sum(map(len, names)) + 8
        src = upload(torch, plan, bufs)
        dst = torch.zeros(plan.out_bytes, dtype=torch.uint8, device="cuda")
        plan.run(src.data_ptr(), dst.data_ptr())
        cap = image_cap(plan, names, first, align)
        img = write_archives(torch, plan, dst, cap)  # behind the run on the same stream, no results() between
        tables = plan.zip_results()
        assert plan.zip_ms() > 0
        stat = plan.results()[1]
        host = img.cpu().numpy().tobytes()
        if keep:
            return host, tables, stat, cap, img
        return host, tables, stat, cap
    finally:
        plan.close()


@pytest.fixture(scope="module")
def main(oracle):
    archives = main_archives()
    names, bufs, first = flatten(archives)
    streams = [stream(oracle, b) for b in bufs]
    want = expected(streams, [Z_OK] * len(bufs), names, first, ALIGN)
    host, tables, stat, cap, img = run_plan(archives, keep=True)
    return {"archives": archives, "names": names, "bufs": bufs, "first": first, "streams": streams, "want": want,
            "host": host, "tables": tables, "stat": stat, "cap": cap, "img": img}


def archive_bytes(host, t):
    return [host[o:o + n] for o, n in zip(t["arch_offsets"], t["arch_lens"])]


def check_zipfile(data, names, bufs, entry_offsets, datetime=0x00210000, utf8=False, every=1):
    with zipfile.ZipFile(io.BytesIO(data)) as z:
        assert z.testzip() is None
        infos = z.infolist()
        assert len(infos) == len(names)
        for k, (info, nm, b, off) in enumerate(zip(infos, names, bufs, entry_offsets)):
            assert info.filename == nm.decode("utf-8" if utf8 else "cp437")
            assert (info.file_size, info.CRC, info.header_offset) == (len(b), zlib.crc32(b), off)
            assert (info.create_system, info.extract_version, info.compress_type) == (0, 20, zipfile.ZIP_DEFLATED)
            dt = datetime if isinstance(datetime, int) else datetime[k]
            assert info.date_time == ((dt >> 25) + 1980, dt >> 21 & 15, dt >> 16 & 31, dt >> 11 & 31, dt >> 5 & 63,
                                      2 * (dt & 31))
            if k % every == 0:
                assert z.read(info) == b


def test_the_case_set_is_what_its_names_say(oracle):
    """the oracle alone: the headers, records and ends at the tile borders"""
    archives = main_archives()
    names, bufs, first = flatten(archives)
    w = expected([stream(oracle, b) for b in bufs], [Z_OK] * len(bufs), names, first, 1)
    titles = [t for t, _ in archives]

    def rel(title):
        a = titles.index(title)
        return a, w["arch_offsets"][a]

    a, base = rel("local-headers-at-borders")
    for k in range(1, LOCAL):
        assert w["entry_offsets"][first[a] + k] - base == k * TILE - k
    for k in range(1, DIR):
        a, base = rel(f"dir-at-border-minus-{k}")
        assert w["dir_offsets"][a] - base == TILE - k
    for k in range(1, END):
        a, base = rel(f"end-at-border-minus-{k}")
        assert w["arch_lens"][a] - END == TILE - k
    a, base = rel("name-cut-by-border")
    assert w["entry_offsets"][first[a] + 1] - base + LOCAL < TILE < w["data_offsets"][first[a] + 1] - base


def test_image_tables_padding_and_canary(main):
    """the image is the format built from the oracle's streams, byte for byte; the tables are the format's and the
    walker's; zeros between the archives; nothing at or behind total"""
    w, t, host = main["want"], main["tables"], main["host"]
    assert main["stat"] == [Z_OK] * len(main["bufs"])
    assert t["total"] == len(w["image"]) <= main["cap"]
    for key in ("arch_offsets", "arch_lens", "arch_statuses", "entry_offsets", "data_offsets", "dir_offsets"):
        assert t[key] == w[key], key
    assert all(o % ALIGN == 0 for o in t["arch_offsets"]) and t["arch_statuses"] == [Z_OK] * len(main["archives"])
    if host[:len(w["image"])] != w["image"]:
        bad = next(x for x in range(len(w["image"])) if host[x] != w["image"][x])
        raise AssertionError(("first wrong byte", bad, host[bad], w["image"][bad]))
    assert host[len(w["image"]):] == bytes([CANARY]) * (len(host) - len(w["image"])), "written at or behind total"
    for a, data in enumerate(archive_bytes(host, t)):
        entries, doff = walk(data)
        base, ids = t["arch_offsets"][a], range(main["first"][a], main["first"][a + 1])
        assert doff == t["dir_offsets"][a] - base
        assert [e["header_offset"] for e in entries] == [t["entry_offsets"][i] - base for i in ids]
        assert [e["data_offset"] for e in entries] == [t["data_offsets"][i] - base for i in ids]
        assert [e["name"] for e in entries] == [main["names"][i] for i in ids]
        assert [e["usize"] for e in entries] == [len(main["bufs"][i]) for i in ids]


def test_zipfile_reads_every_archive_back_to_the_inputs(main):
    t = main["tables"]
    for a, data in enumerate(archive_bytes(main["host"], t)):
        ids = range(main["first"][a], main["first"][a + 1])
        check_zipfile(data, [main["names"][i] for i in ids], [main["bufs"][i] for i in ids],
                      [t["entry_offsets"][i] - t["arch_offsets"][a] for i in ids])


def test_a_raw_inflate_plan_reads_the_entries_at_data_offsets(main):
    """the library reads its own ZIP entries: window_bits -15 over data_offsets and the compressed sizes, moved to
    the plan's aligned slots by zsc_hip_unpack"""
    import torch
    import zsc_amd
    t, bufs = main["tables"], main["bufs"]
    csize = [len(s) - 18 for s in main["streams"]]
    plan = zsc_amd.InflatePlan(csize, [len(b) for b in bufs], -15)
    try:
        src = torch.zeros(plan.src_bytes, dtype=torch.uint8, device="cuda")
        dst = torch.zeros(plan.dst_bytes, dtype=torch.uint8, device="cuda")
        assert zsc_amd.unpack(main["img"].data_ptr(), t["data_offsets"], csize, src.data_ptr(), plan.src_offsets) == 0
        plan.run(src.data_ptr(), dst.data_ptr())
        lens, used, stat, _ = plan.results()
        host = dst.cpu().numpy().tobytes()
        assert stat == [Z_OK] * len(bufs) and used == csize and lens == [len(b) for b in bufs]
        for i, (b, off) in enumerate(zip(bufs, plan.dst_offsets)):
            assert host[off:off + len(b)] == b, i
    finally:
        plan.close()


def test_a_failed_buffer_fails_its_archive_alone(oracle, main):
    """a buffer forced to Z_BUF_ERROR by a small capacity: its archive has no length, the others are byte for byte
    those of a plan without it"""
    import zsc_amd
    titles = ("golden-mix", "dir-at-border-minus-7", "twenty-small", "empty-between", "end-at-border-minus-3")
    archives = [a for a in main["archives"] if a[0] in titles]
    assert [a[0] for a in archives] == ["golden-mix", "dir-at-border-minus-7", "empty-between",
                                        "end-at-border-minus-3", "twenty-small"]
    names, bufs, first = flatten(archives)
    probe = zsc_amd.DeflatePlan([len(b) for b in bufs], 6, GZ)
    caps = list(probe.out_caps)
    probe.close()
    victim = first[1]  # the one buffer of the second archive: random bytes, which do not fit half their length
    caps[victim] = len(bufs[victim]) // 2
    host, t, stat, _ = run_plan(archives, out_caps=caps)
    assert [s != Z_OK for s in stat] == [i == victim for i in range(len(bufs))] and stat[victim] == Z_BUF_ERROR
    assert t["arch_statuses"] == [Z_OK, Z_BUF_ERROR, Z_OK, Z_OK, Z_OK] and t["arch_lens"][1] == 0
    assert t["arch_offsets"][2] == t["arch_offsets"][1] == t["entry_offsets"][victim] == t["dir_offsets"][1]
    host2, t2, stat2, _ = run_plan(archives[:1] + archives[2:])
    assert stat2 == [Z_OK] * (len(bufs) - 1)
    assert t2["total"] == t["total"] and host2[:t2["total"]] == host[:t["total"]]
    assert t2["arch_offsets"] == t["arch_offsets"][:1] + t["arch_offsets"][2:]
    w = expected([stream(oracle, b) for b in bufs], stat, names, first, ALIGN)
    assert host[:t["total"]] == w["image"] and t["arch_statuses"] == w["arch_statuses"]


def test_the_zip64_records_are_there_from_65535_entries_on(oracle):
    """65 536 buffers of 0 to 2 bytes in one archive and 65 534 in the next: the ZIP64 end record and its locator
    in the first alone; zipfile reads both"""
    def entries(n):
        return [(b"%05x" % j, bytes([65 + j % 7] * (j % 3))) for j in range(n)]

    archives = [("with", entries(65536)), ("without", entries(65534))]
    names, bufs, first = flatten(archives)
    host, t, stat, _ = run_plan(archives, align=1)
    assert stat == [Z_OK] * len(bufs) and t["arch_statuses"] == [Z_OK, Z_OK]
    w = expected([stream(oracle, b) for b in bufs], stat, names, first, 1)
    assert t["total"] == len(w["image"]) and host[:t["total"]] == w["image"]
    for key in ("arch_offsets", "arch_lens", "entry_offsets", "data_offsets", "dir_offsets"):
        assert t[key] == w[key], key
    big, small = archive_bytes(host, t)
    assert big[-END64:-END64 + 4] == b"PK\x06\x06" and big[-END - 20:-END - 16] == b"PK\x06\x07"
    assert b"PK\x06\x06" not in small[-END64:] and small[-END:-END + 4] == b"PK\x05\x06"
    for a, data in enumerate((big, small)):
        ids = range(first[a], first[a + 1])
        assert len(walk(data)[0]) == len(ids)
        check_zipfile(data, [names[i] for i in ids], [bufs[i] for i in ids],
                      [t["entry_offsets"][i] - t["arch_offsets"][a] for i in ids], every=509)


@pytest.mark.parametrize("level,mem_level", [(1, 8), (9, 1), (9, 8), (6, 1)])
def test_the_golden_buffers_at_their_other_levels(oracle, level, mem_level):
    """with a time and date per buffer and the UTF-8 flag"""
    recs = [r for r in golden() if (r["level"], r["mem_level"]) == (level, mem_level)]
    assert recs
    entries = [("%s-%d-é.bin" % (r["kind"], r["size"])).encode() for r in recs]
    archives = [("all", [(nm, golden_buffer(r)) for nm, r in zip(entries, recs)]), ("none", [])]
    names, bufs, first = flatten(archives)
    dts = [(j + 20 << 9 | 1 + j << 5 | 2 + j) << 16 | (j << 11 | 3 * j << 5 | j) for j in range(len(bufs))]
    host, t, stat, _ = run_plan(archives, level, mem_level, align=1, datetimes=dts, utf8=True)
    assert stat == [Z_OK] * len(bufs)
    w = expected([stream(oracle, b, level, mem_level) for b in bufs], stat, names, first, 1, dts, 0x0800)
    assert t["total"] == len(w["image"]) and host[:t["total"]] == w["image"]
    assert host[t["total"]:] == bytes([CANARY]) * (len(host) - t["total"])
    data = archive_bytes(host, t)
    check_zipfile(data[0], names, bufs, t["entry_offsets"], dts, utf8=True)
    assert data[1] == b"PK\x05\x06" + b"\0" * 18


def test_behind_the_run_on_a_stream_of_its_own_twice_and_on_a_copy(oracle, main):
    """_zip on the caller's stream behind _run with no results() between, twice, and on a copy of the output"""
    import torch
    import zsc_amd
    titles = ("dir-at-border-minus-3", "empty-between", "twenty-small", "end-at-border-minus-5")
    archives = [a for a in main["archives"] if a[0] in titles]
    names, bufs, first = flatten(archives)
    others = [bytes(reversed(b)) for b in bufs]  # other input of the same shape
    plan = zsc_amd.DeflatePlan([len(b) for b in bufs], 6, GZ)
    side = torch.cuda.Stream()
    try:
        plan.zip_enable(first, names)
        cap = image_cap(plan, names, first, 1)
        for data in (bufs, others):
            want = expected([stream(oracle, b) for b in data], [Z_OK] * len(data), names, first, 1)["image"]
            with torch.cuda.stream(side):
                src = upload(torch, plan, data)
                dst = torch.zeros(plan.out_bytes, dtype=torch.uint8, device="cuda")
                plan.run(src.data_ptr(), dst.data_ptr(), side.cuda_stream)
                imgs = [write_archives(torch, plan, dst, cap, side.cuda_stream) for _ in range(2)]
                copy = dst.clone()
                imgs.append(write_archives(torch, plan, copy, cap, side.cuda_stream))
            t = plan.zip_results()
            side.synchronize()
            for img in imgs:
                host = img.cpu().numpy().tobytes()
                assert t["total"] == len(want) and host[:len(want)] == want
                assert host[len(want):] == bytes([CANARY]) * (len(host) - len(want))
    finally:
        plan.close()


def test_a_short_image_is_not_touched_and_the_tables_are_filled(main):
    import torch
    import zsc_amd
    archives = [a for a in main["archives"] if a[0] in ("dir-at-border-minus-9", "empty-between", "twenty-small")]
    names, bufs, first = flatten(archives)
    plan = zsc_amd.DeflatePlan([len(b) for b in bufs], 6, GZ)
    try:
        plan.zip_enable(first, names, align=16)
        src = upload(torch, plan, bufs)
        dst = torch.zeros(plan.out_bytes, dtype=torch.uint8, device="cuda")
        plan.run(src.data_ptr(), dst.data_ptr())
        write_archives(torch, plan, dst, image_cap(plan, names, first, 16))
        full = plan.zip_results()
        short = write_archives(torch, plan, dst, full["total"] - 1)
        with pytest.raises(BufferError) as e:
            plan.zip_results()
        assert e.value.tables == full
        assert bool((short == CANARY).all())
    finally:
        plan.close()


def test_refusals_leave_the_plan_as_it_was(oracle):
    import torch
    import zsc_amd
    from zsc_amd import corpus
    bufs = [corpus.make_buffer("text", n, 300 + n) for n in (500, 0, 3000)]
    names = [b"a", b"", b"ccc"]
    want = [stream(oracle, b) for b in bufs]

    def runs_normally(plan):
        src = upload(torch, plan, bufs)
        dst = torch.zeros(plan.out_bytes, dtype=torch.uint8, device="cuda")
        plan.run(src.data_ptr(), dst.data_ptr())
        lens, stat = plan.results()
        host = dst.cpu().numpy().tobytes()
        return stat == [0, 0, 0] and [host[o:o + n] for o, n in zip(plan.out_offsets, lens)] == want, dst

    plan = zsc_amd.DeflatePlan([len(b) for b in bufs], 6, GZ)
    try:
        scratch = plan.scratch_bytes
        ok, dst = runs_normally(plan)
        assert ok
        img = torch.full((8192,), CANARY, dtype=torch.uint8, device="cuda")
        assert plan.zip(dst.data_ptr(), img.data_ptr(), 8192) == Z_STREAM_ERROR  # never enabled
        with pytest.raises(RuntimeError):
            plan.zip_results()
        long_name = [b"a", b"b" * 65536, b"c"]
        for first, nms, align in (([1, 3], names, 1), ([0, 2], names, 1), ([0, 4], names, 1), ([0, 2, 1, 3], names, 1),
                                  ([0, 3], names, 0), ([0, 3], names, 3), ([0, 3], names, 8192), ([0, 3], long_name, 1)):
            with pytest.raises(ValueError):
                plan.zip_enable(first, nms, align=align)
            assert plan.scratch_bytes == scratch
            assert plan.zip(dst.data_ptr(), img.data_ptr(), 8192) == Z_STREAM_ERROR
        import ctypes as C
        offs = (C.c_uint64 * 4)(0, 5, 3, 6)  # descending name offsets, and unknown flags: the C call itself
        one = (C.c_uint32 * 2)(0, 3)
        assert zsc_amd.lib.zsc_hip_deflate_plan_zip_enable(plan._h, 1, one, b"abcdef", offs, None, 0, 1) == Z_STREAM_ERROR
        offs = (C.c_uint64 * 4)(0, 1, 1, 4)
        assert zsc_amd.lib.zsc_hip_deflate_plan_zip_enable(plan._h, 1, one, b"abcd", offs, None, 2, 1) == Z_STREAM_ERROR
        assert plan.scratch_bytes == scratch
        assert runs_normally(plan)[0] and bool((img == CANARY).all())
        # a partition, then a refused one: the first stays; then another replaces everything
        plan.zip_enable([0, 1, 3], names)
        with pytest.raises(ValueError):
            plan.zip_enable([0, 5], names)
        ok, dst = runs_normally(plan)
        assert ok
        assert plan.zip(dst.data_ptr(), img.data_ptr(), 8192) == 0
        assert plan.zip_results()["arch_offsets"] == expected(want, [0] * 3, names, [0, 1, 3])["arch_offsets"]
        plan.zip_enable([0, 0, 3, 3], [b"x", b"yy", b"z" * 40], align=16)
        assert plan.zip(dst.data_ptr(), img.data_ptr(), 8192) == 0
        t = plan.zip_results()
        w = expected(want, [0] * 3, [b"x", b"yy", b"z" * 40], [0, 0, 3, 3], 16)
        assert t["arch_offsets"] == w["arch_offsets"] and img.cpu().numpy().tobytes()[:t["total"]] == w["image"]
    finally:
        plan.close()
    for kw in ({"window_bits": 15}, {"window_bits": -15}):  # not gzip
        plan = zsc_amd.DeflatePlan([len(b) for b in bufs], 6, **kw)
        try:
            with pytest.raises(ValueError):
                plan.zip_enable([0, 3], names)
        finally:
            plan.close()


def test_the_host_batch_equals_the_plan_path(oracle):
    """three archives, one of them empty, through zsc_amd.zip_compress_batch (zsc_hip_zip_compress_batch)"""
    import zsc_amd
    from zsc_amd import corpus
    sets = [[(b"a.txt", corpus.make_buffer("text", 200000, 11)), (b"dir/b.bin", corpus.make_buffer("table", 70000, 12)),
             (b"empty", b"")], [], [(b"one", corpus.make_buffer("bitmap", 5000, 13))]]
    archives = [(f"archive-{j}", s) for j, s in enumerate(sets)]
    host, t, stat, _ = run_plan(archives, align=16)
    plan_path = archive_bytes(host, t)
    got, statuses = zsc_amd.zip_compress_batch(sets)
    assert statuses == [Z_OK] * 3 and got == plan_path
    names, bufs, first = flatten(archives)
    w = expected([stream(oracle, b) for b in bufs], [Z_OK] * len(bufs), names, first, 1)
    assert b"".join(got) == w["image"] and got[1] == b"PK\x05\x06" + b"\0" * 18
    for data, s in zip(got, sets):
        check_zipfile(data, [n for n, _ in s], [b for _, b in s], [e["header_offset"] for e in walk(data)[0]])
    # only empty archives; a time and date and the flag; level 0 and what _zip_enable refuses
    assert zsc_amd.zip_compress_batch([[], []]) == ([b"PK\x05\x06" + b"\0" * 18] * 2, [Z_OK, Z_OK])
    dts = [0x5A8E6B2F, 0x00210000, 0x00210000, 0x5A8E0000]
    got2, _ = zsc_amd.zip_compress_batch(sets, dos_datetime=dts, utf8=True)
    check_zipfile(got2[0], [n for n, _ in sets[0]], [b for _, b in sets[0]],
                  [e["header_offset"] for e in walk(got2[0])[0]], dts[:3], utf8=True)
    with pytest.raises(zsc_amd.PackedCallError):
        zsc_amd.zip_compress_batch(sets, level=0)
    with pytest.raises(zsc_amd.PackedCallError):
        zsc_amd.zip_compress_batch([[(b"n" * 65536, b"data")]])
    # too little room for one archive: that archive alone
    tight, st = zsc_amd.zip_compress_batch(sets, dest_caps=[len(got[0]) - 1, END, len(got[2])])
    assert st == [Z_BUF_ERROR, Z_OK, Z_OK] and tight[1:] == got[1:]
    assert Z_MEM_ERROR == -4  # (an archive past 4 294 967 295 bytes is not built here: tests/test_zip_emu.py)
