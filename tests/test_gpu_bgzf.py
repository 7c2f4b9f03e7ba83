"""BGZF files from a gzip deflate plan on the GPU (zsc_amd/csrc/bgzf.h, include/zsc_hip.h "BGZF files").

One plan of about 150 buffers at level 6, mem_level 8, run once and written once (module fixture `main`); the
tests look at that one image.  What a member must be comes from the oracle alone: the 18-byte header and
oracle.compress(buf, 6, 16 + 15)[10:] (tests/bgzf_cases.py), and from tests/golden/bgzf_golden.json, which
records what the compiled reference writes when it is given the `BC` field in a gz_header.

Real streams reach the tile borders through stored blocks: a random buffer of n < 16 383 bytes gives a member of
n + 31 bytes, so a header or a tail is placed k bytes before offset 16 384 of its file for every k it has bytes.
The lengths whose members are 65 536 and 65 537 bytes long are looked for by asking the oracle.

Not reachable from here: the refusal of a plan of sections.  Such plans exist only inside
zsc_hip_compress_sections_*; no public call hands one out.
"""
import gzip
import hashlib
import json
import os
import random

import pytest

from bgzf_cases import BGZF_EOF, MAX_MEMBER, TILE, Z_BUF_ERROR, Z_OK, Z_STREAM_ERROR, expected, member, walk_bsize

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GZ = 31
CANARY = 0xC7
ALIGN = 16
_RANDOM = random.Random(5).randbytes(MAX_MEMBER + 64)
_memo = {}


def golden():
    if "golden" not in _memo:
        _memo["golden"] = json.load(open(os.path.join(HERE, "golden", "bgzf_golden.json")))["members"]
    return _memo["golden"]


def golden_buffer(rec):
    from zsc_amd import corpus
    return corpus.make_buffer(rec["kind"], rec["size"], rec["seed"])


def stream(oracle, buf, level=6, mem_level=8):
    key = (hash(buf), len(buf), level, mem_level)
    if key not in _memo:
        rc, s, _ = oracle.compress(buf, level, window_bits=GZ, mem_level=mem_level)
        assert rc == 0
        _memo[key] = s
    return _memo[key]


def limit_lengths(oracle):
    """(n, m): prefixes of one random buffer whose members are the longest that fits and the shortest that does
    not -- 65 536 and 65 537 bytes where the lengths do not skip"""
    if "limits" not in _memo:
        n = MAX_MEMBER - 60
        while len(stream(oracle, _RANDOM[:n + 1])) + 8 <= MAX_MEMBER:
            n += 1
        _memo["limits"] = (n, n + 1)
    return _memo["limits"]


def main_files(oracle):
    """[(name, [buffers])]; built once"""
    if "files" in _memo:
        return _memo["files"]
    from zsc_amd import corpus
    six = [r for r in golden() if (r["level"], r["mem_level"]) == (6, 8)]
    assert len(six) == 18 and {r["size"] for r in six} == {0, 1, 100, 4096, 65280, 65536}
    files = [("golden-mix", [golden_buffer(r) for r in six if "overflow" not in r]),
             ("empty-first", []),
             ("overflow-random-65536", [golden_buffer(r) for r in six if "overflow" in r])]
    text100 = corpus.make_buffer("text", 100, 3)
    for k in range(1, 18):
        files.append((f"header-at-border-minus-{k}", [_RANDOM[k:k + TILE - 31 - k], text100]))
    for k in range(1, 28):
        files.append((f"tail-at-border-minus-{k}", [_RANDOM[100 + k:100 + k + TILE - 31 - k]]))
    n, m = limit_lengths(oracle)
    files += [("longest-member", [_RANDOM[:n]]),
              ("neighbour-before", [corpus.make_buffer("text", 4096, 4)]),
              ("too-long", [text100, _RANDOM[:m], corpus.make_buffer("zero", 100, 5)]),
              ("neighbour-after", [corpus.make_buffer("zero", 4096, 6), corpus.make_buffer("text", 1, 7)]),
              ("empty-between", []),
              ("forty-small", [corpus.make_buffer("text", (37 * j) % 700, 200 + j) for j in range(40)]),
              ("empty-last", [])]
    assert 120 <= sum(len(b) for _, b in files) <= 180
    _memo["files"] = files
    return files


def flatten(files):
    bufs, first = [], [0]
    for _, f in files:
        bufs += f
        first.append(len(bufs))
    return bufs, first


def upload(torch, plan, bufs):
    image = bytearray(plan.in_bytes)
    for b, off in zip(bufs, plan.in_offsets):
        image[off:off + len(b)] = b
    return torch.frombuffer(image, dtype=torch.uint8).cuda()


def write_files(torch, plan, d_out, cap, stream=0):
    img = torch.full((cap + 64,), CANARY, dtype=torch.uint8, device="cuda")
    assert plan.bgzf(d_out.data_ptr(), img.data_ptr(), cap, stream) == 0
    return img


def run_plan(files, level=6, mem_level=8, align=ALIGN):
    """one plan, one run, one bgzf(): (host image with its canary, tables, statuses of the buffers)"""
    import torch
    import zsc_amd
    bufs, first = flatten(files)
    plan = zsc_amd.DeflatePlan([len(b) for b in bufs], level, GZ, mem_level)
    try:
        before = plan.scratch_bytes
        plan.bgzf_enable(first, align)
        # 20 bytes per buffer, 24 per file, 8 for the sums (rounded to the allocator's granules: at least that)
        assert plan.scratch_bytes - before >= 20 * len(bufs) + 24 * (len(first) - 1) + 8
        src = upload(torch, plan, bufs)
        dst = torch.zeros(plan.out_bytes, dtype=torch.uint8, device="cuda")
        plan.run(src.data_ptr(), dst.data_ptr())
        cap = sum(min(c + 8, MAX_MEMBER) for c in plan.out_caps) + (28 + align) * (len(first) - 1)
        img = write_files(torch, plan, dst, cap)  # behind the run on the same stream, no results() between
        tables = plan.bgzf_results()
        assert plan.bgzf_ms() > 0
        stat = plan.results()[1]
        return img.cpu().numpy().tobytes(), tables, stat, cap
    finally:
        plan.close()


@pytest.fixture(scope="module")
def main(oracle):
    files = main_files(oracle)
    bufs, first = flatten(files)
    streams = [stream(oracle, b) for b in bufs]
    want = expected(streams, [Z_OK] * len(bufs), first, ALIGN)
    host, tables, stat, cap = run_plan(files)
    return {"files": files, "bufs": bufs, "first": first, "streams": streams, "want": want, "host": host,
            "tables": tables, "stat": stat, "cap": cap}


def good_files(main):
    """[(name, buffers, the file's bytes)] of the files that are Z_OK"""
    t, out = main["tables"], []
    for f, (name, bufs) in enumerate(main["files"]):
        if t["file_statuses"][f] == Z_OK:
            out.append((name, bufs, main["host"][t["file_offsets"][f]:t["file_offsets"][f] + t["file_lens"][f]]))
    return out


def test_the_case_set_is_what_its_names_say(oracle):
    """the oracle alone: the members at the tile borders and on either side of the limit"""
    by = dict(main_files(oracle))
    for k in range(1, 18):
        assert len(stream(oracle, by[f"header-at-border-minus-{k}"][0])) + 8 == TILE - k
    for k in range(1, 28):
        assert len(stream(oracle, by[f"tail-at-border-minus-{k}"][0])) + 8 == TILE - k
    n, m = limit_lengths(oracle)
    fits, over = len(stream(oracle, _RANDOM[:n])) + 8, len(stream(oracle, _RANDOM[:m])) + 8
    assert fits <= MAX_MEMBER < over
    assert (fits, over) == (MAX_MEMBER, MAX_MEMBER + 1)  # (the lengths do not skip here)
    assert len(stream(oracle, by["overflow-random-65536"][0])) + 8 > MAX_MEMBER


def test_members_tables_padding_and_canary(main):
    """1, 2: every member is the header and the oracle's stream from byte 10; offsets, lengths, statuses and
    total are the format's; zeros between the files; nothing at or behind total"""
    image, file_off, file_lens, file_stat, member_off, _ = main["want"]
    t, host = main["tables"], main["host"]
    assert main["stat"] == [Z_OK] * len(main["bufs"])
    assert t["total"] == len(image) <= main["cap"]
    assert t["file_offsets"] == file_off and all(o % ALIGN == 0 for o in file_off)
    assert t["file_lens"] == file_lens and t["file_statuses"] == file_stat
    assert t["member_offsets"] == member_off
    for i, s in enumerate(main["streams"]):
        f = next(f for f in range(len(file_stat)) if main["first"][f] <= i < main["first"][f + 1])
        if file_stat[f] == Z_OK:
            m = member(s)
            assert host[member_off[i]:member_off[i] + len(m)] == m, i
    assert host[:len(image)] == image
    assert host[len(image):] == bytes([CANARY]) * (len(host) - len(image)), "written at or behind total"
    names = [n for n, _ in main["files"]]
    assert [n for n, st in zip(names, file_stat) if st != Z_OK] == ["overflow-random-65536", "too-long"]


def test_golden_members_equal_the_references_record(main):
    recs = [r for r in golden() if (r["level"], r["mem_level"]) == (6, 8) and "overflow" not in r]
    at = main["tables"]["member_offsets"]
    assert main["files"][0][0] == "golden-mix" and len(recs) == len(main["files"][0][1]) == 17
    for i, r in enumerate(recs):
        got = main["host"][at[i]:at[i] + r["len"]]
        assert hashlib.sha256(got).hexdigest() == r["sha256"], r
        if "hex" in r:
            assert got == bytes.fromhex(r["hex"])
        assert at[i + 1] - at[i] == r["len"] or i == len(recs) - 1


def test_too_long_file_fails_and_its_neighbours_do_not_notice(oracle, main):
    """3: the file with the member of 65 537 bytes is Z_BUF_ERROR with no length; the files around it are byte
    for byte those of a plan that does not have it"""
    t = main["tables"]
    names = [n for n, _ in main["files"]]
    k = names.index("too-long")
    assert t["file_statuses"][k] == Z_BUF_ERROR and t["file_lens"][k] == 0
    assert t["file_offsets"][k + 1] == t["file_offsets"][k]
    assert all(t["member_offsets"][i] == t["file_offsets"][k] for i in range(main["first"][k], main["first"][k + 1]))
    host2, t2, stat2, _ = run_plan(main["files"][:k] + main["files"][k + 1:])
    assert t2["total"] == t["total"] and host2[:t2["total"]] == main["host"][:t["total"]]
    assert t2["file_offsets"] == t["file_offsets"][:k] + t["file_offsets"][k + 1:]


def test_python_gzip_reads_every_good_file_and_bsize_walks_it(main):
    """4, 5"""
    files = good_files(main)
    assert len(files) == len(main["files"]) - 2
    for name, bufs, data in files:
        assert gzip.decompress(data) == b"".join(bufs), name
        walked = walk_bsize(data)
        assert len(walked) == len(bufs) + 1 and walked[-1][1] == len(BGZF_EOF), name


def test_a_members_plan_reads_every_good_file_by_its_claims(main):
    """6, 7: Z_OK, the input's bytes, consumed == len(file), claimed == members == buffers + 1"""
    from test_gpu_inflate_members import run_members
    files = good_files(main)
    res, clean = run_members([d for _, _, d in files], [sum(len(b) for b in bufs) for _, bufs, _ in files])
    assert clean
    for (name, bufs, data), (st, ol, out, used, members, prefix, claimed) in zip(files, res):
        assert (st, used) == (Z_OK, len(data)), name
        assert out == b"".join(bufs), name
        assert claimed == members == len(bufs) + 1, (name, claimed, members)


@pytest.mark.parametrize("level,mem_level,xfl", [(1, 8, 4), (9, 1, 2)])
def test_other_levels_write_their_xfl(oracle, level, mem_level, xfl):
    """8: XFL is the plan's own; at level 9 with mem_level 1 a random buffer of 65 280 bytes does not fit"""
    recs = [r for r in golden() if (r["level"], r["mem_level"]) == (level, mem_level)]
    files = [(f"{r['kind']}-{r['size']}", [golden_buffer(r)]) for r in recs]
    host, t, stat, _ = run_plan(files, level, mem_level, align=1)
    assert stat == [Z_OK] * len(files)
    streams = [stream(oracle, b[0], level, mem_level) for _, b in files]
    want = expected(streams, stat, list(range(len(files) + 1)), 1)
    assert host[:t["total"]] == want[0] and t["file_statuses"] == want[3]
    for r, s, off, st in zip(recs, streams, t["file_offsets"], t["file_statuses"]):
        if "overflow" in r:
            assert st == Z_BUF_ERROR and len(s) == r["overflow"]
        else:
            assert st == Z_OK and host[off + 8] == xfl
            assert hashlib.sha256(host[off:off + r["len"]]).hexdigest() == r["sha256"]
    assert sum("overflow" in r for r in recs) == (1 if level == 9 else 0)


def test_behind_the_run_on_a_stream_of_its_own_twice_and_after_another_run(oracle, main):
    """9"""
    import torch
    import zsc_amd
    names = ("header-at-border-minus-3", "empty-between", "neighbour-after", "tail-at-border-minus-5")
    files = [(n, b) for n, b in main["files"] if n in names]
    bufs, first = flatten(files)
    others = [bytes(reversed(b)) for b in bufs]  # other input of the same shape
    plan = zsc_amd.DeflatePlan([len(b) for b in bufs], 6, GZ)
    side = torch.cuda.Stream()
    try:
        plan.bgzf_enable(first, 1)
        cap = sum(c + 8 for c in plan.out_caps) + 28 * len(files)
        for data in (bufs, others):
            want = expected([stream(oracle, b) for b in data], [Z_OK] * len(data), first, 1)[0]
            with torch.cuda.stream(side):
                src = upload(torch, plan, data)
                dst = torch.zeros(plan.out_bytes, dtype=torch.uint8, device="cuda")
                plan.run(src.data_ptr(), dst.data_ptr(), side.cuda_stream)
                imgs = [write_files(torch, plan, dst, cap, side.cuda_stream) for _ in range(2)]
            t = plan.bgzf_results()
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
    files = [f for f in main["files"] if f[0] in ("neighbour-before", "empty-between", "neighbour-after")]
    bufs, first = flatten(files)
    plan = zsc_amd.DeflatePlan([len(b) for b in bufs], 6, GZ)
    try:
        plan.bgzf_enable(first, 16)
        src = upload(torch, plan, bufs)
        dst = torch.zeros(plan.out_bytes, dtype=torch.uint8, device="cuda")
        plan.run(src.data_ptr(), dst.data_ptr())
        write_files(torch, plan, dst, plan.out_bytes)
        full = plan.bgzf_results()
        short = write_files(torch, plan, dst, full["total"] - 1)
        with pytest.raises(BufferError) as e:
            plan.bgzf_results()
        assert e.value.tables == full
        assert bool((short == CANARY).all())
    finally:
        plan.close()


def test_refusals_leave_the_plan_as_it_was(oracle):
    """10"""
    import torch
    import zsc_amd
    from zsc_amd import corpus
    bufs = [corpus.make_buffer("text", n, 300 + n) for n in (500, 0, 3000)]
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
        img = torch.full((4096,), CANARY, dtype=torch.uint8, device="cuda")
        assert plan.bgzf(dst.data_ptr(), img.data_ptr(), 4096) == Z_STREAM_ERROR  # never enabled
        with pytest.raises(RuntimeError):
            plan.bgzf_results()
        for first, align in (([1, 3], 1), ([0, 2], 1), ([0, 4], 1), ([0, 2, 1, 3], 1), ([0, 3], 0), ([0, 3], 3),
                             ([0, 3], 8192)):
            with pytest.raises(ValueError):
                plan.bgzf_enable(first, align)
            assert plan.scratch_bytes == scratch
            assert plan.bgzf(dst.data_ptr(), img.data_ptr(), 4096) == Z_STREAM_ERROR
        assert runs_normally(plan)[0] and bool((img == CANARY).all())
        # a partition, then a refused one: the first stays; then another replaces it
        plan.bgzf_enable([0, 1, 3], 1)
        with pytest.raises(ValueError):
            plan.bgzf_enable([0, 5], 1)
        ok, dst = runs_normally(plan)
        assert ok
        assert plan.bgzf(dst.data_ptr(), img.data_ptr(), 4096) == 0
        assert plan.bgzf_results()["file_offsets"] == expected(want, [0] * 3, [0, 1, 3], 1)[1]
        plan.bgzf_enable([0, 0, 3, 3], 16)
        assert plan.bgzf(dst.data_ptr(), img.data_ptr(), 4096) == 0
        t = plan.bgzf_results()
        w = expected(want, [0] * 3, [0, 0, 3, 3], 16)
        assert t["file_offsets"] == w[1] and img.cpu().numpy().tobytes()[:t["total"]] == w[0]
    finally:
        plan.close()
    for kw in ({"window_bits": 15}, {"window_bits": -15}):  # not gzip
        plan = zsc_amd.DeflatePlan([len(b) for b in bufs], 6, **kw)
        try:
            with pytest.raises(ValueError):
                plan.bgzf_enable([0, 3], 1)
        finally:
            plan.close()
    plan = zsc_amd.DeflatePlan([100, MAX_MEMBER + 1], 6, GZ)  # a buffer too long for a member
    try:
        with pytest.raises(ValueError):
            plan.bgzf_enable([0, 2], 1)
    finally:
        plan.close()


def test_the_host_batch_equals_the_plan_path(oracle):
    """11: three files, one empty and one of 200 000 bytes"""
    import zsc_amd
    from zsc_amd import corpus
    files = [corpus.make_buffer("text", 200000, 11), b"", corpus.make_buffer("table", 70000, 12)]
    block = 65280
    cut = [(f"file-{j}", [f[at:at + block] for at in range(0, len(f), block)]) for j, f in enumerate(files)]
    host, t, stat, _ = run_plan(cut, align=1)
    plan_path = [host[o:o + n] for o, n in zip(t["file_offsets"], t["file_lens"])]
    got, statuses = zsc_amd.bgzf_compress_batch(files)
    assert statuses == [Z_OK] * 3 and got == plan_path
    assert got[1] == BGZF_EOF and [gzip.decompress(g) for g in got] == files
    assert [len(walk_bsize(g)) for g in got] == [5, 1, 3]
    bufs, first = flatten(cut)
    assert b"".join(got) == expected([stream(oracle, b) for b in bufs], [Z_OK] * len(bufs), first, 1)[0]
    # other block sizes, and the ones that are none
    got16, st16 = zsc_amd.bgzf_compress_batch([files[2][:1000], b""], block_bytes=16)
    assert st16 == [Z_OK, Z_OK] and gzip.decompress(got16[0]) == files[2][:1000] and len(walk_bsize(got16[0])) == 64
    assert zsc_amd.bgzf_compress_batch(files, block_bytes=0)[0] == got
    for bad in ({"block_bytes": 24}, {"block_bytes": 65552}, {"level": 0}):
        with pytest.raises(zsc_amd.PackedCallError):
            zsc_amd.bgzf_compress_batch(files, **bad)
    # too little room for one file: that file alone
    tight, st = zsc_amd.bgzf_compress_batch(files, dest_caps=[len(got[0]) - 1, 28, len(got[2])])
    assert st == [Z_BUF_ERROR, Z_OK, Z_OK] and tight[1:] == got[1:]
