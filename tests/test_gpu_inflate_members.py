"""Members plans on the MI355X (zsc_amd/csrc/inflate_members.h), through the C ABI as zsc_amd.InflatePlan
calls it: every file of tests/test_inflate_members_emu.py's case set equal to the oracle walk on (status,
bytes, consumed, members), with the verified prefix each case states, nothing written outside a file's own
slot, in one plan that holds every case (so the lane groups of one wavefront work on different files).

FDICT / Z_NEED_DICT does not arise with gzip (the header has no such flag), so no case fakes it.  The runtime
offers no hook for the candidate pool's size or the work bound, so those two are reached on the lane
emulation only (its setters); what can be reached here without a hook is the per-file candidate cap
(magic-dense-overflows), which takes the same way out as a used-up pool.
"""
import gzip

import numpy as np
import pytest

from test_inflate_members_emu import GZ, Z_OK, make_member_cases, walk

pytestmark = pytest.mark.gpu

CANARY = 0xEE


def run_members(files, caps, size_only=False, runs=1, src_offsets=None):
    """one members plan over the files: [(status, out_len, bytes or None, consumed, members, prefix, claimed)]
    per file, and whether every byte outside the files' own slots kept its canary"""
    import torch
    import zsc_amd
    plan = zsc_amd.InflatePlan([len(f) for f in files], caps, window_bits=GZ, members=True, size_only=size_only,
                               src_offsets=src_offsets)
    try:
        image = bytearray(plan.src_bytes)
        for f, off in zip(files, plan.src_offsets):
            image[off:off + len(f)] = f
        d_src = torch.frombuffer(image, dtype=torch.uint8).cuda()
        d_dst = None if size_only else torch.full((plan.dst_bytes,), CANARY, dtype=torch.uint8, device="cuda")
        seen = []
        for _ in range(runs):
            if d_dst is not None:
                d_dst.fill_(CANARY)
                torch.cuda.synchronize()
            plan.run(d_src.data_ptr(), 0 if size_only else d_dst.data_ptr())
            first = plan.results()[:3]
            assert plan.results()[:3] == first  # (results() twice)
            lens, used, stat = first
            members, claimed = plan.members()
            prefix = plan.sections()
            host = None if size_only else d_dst.cpu().numpy()
            res, clean = [], True
            if host is not None:
                mask = np.ones(len(host), dtype=bool)
                for off, cap in zip(plan.dst_offsets, caps):
                    mask[off:off + cap] = False
                clean = bool((host[mask] == CANARY).all())
            for i in range(len(files)):
                out = None
                if host is not None:
                    assert lens[i] <= caps[i]
                    out = host[plan.dst_offsets[i]:plan.dst_offsets[i] + lens[i]].tobytes()
                res.append((stat[i], lens[i], out, used[i], members[i], prefix[i], claimed[i]))
            seen.append((res, clean))
        assert all(s == seen[0] for s in seen)  # (the plan run again gives the same)
        return seen[0]
    finally:
        plan.close()


def check(c, want, got, claims=True):
    st, ol, out, used, members, prefix, claimed = got
    rc, wout, wused, wmembers = want
    assert (st, ol, used, members) == (rc, len(wout), wused, wmembers), (c.name, got[:2], got[3:])
    assert out == wout, c.name
    assert prefix == c.prefix, (c.name, prefix, c.prefix)
    if not claims:
        assert claimed == 0, c.name
    elif c.claimed is not None:
        assert claimed == c.claimed, (c.name, claimed)
    else:
        assert claimed <= prefix, c.name


@pytest.fixture(scope="module")
def walks(oracle):
    return {c.name: walk(oracle, c.data, c.cap) for c in make_member_cases(oracle)}


def test_every_case_in_one_plan_equals_the_walk(oracle, walks):
    cases = make_member_cases(oracle)
    assert sum(c.kind in ("clean", "bgzf") for c in cases) >= 40
    res, clean = run_members([c.data for c in cases], [c.cap for c in cases], runs=2)
    assert clean, "a byte outside the files' own slots was written"
    for c, got in zip(cases, res):
        check(c, walks[c.name], got)
        if c.kind in ("clean", "bgzf"):
            assert got[4] == got[5] == c.built, c.name  # sections() == members() == the built count
        if c.kind == "bgzf":
            assert got[6] == got[5], c.name             # every member of a clean BGZF file was claimed


def test_claims_switched_off_give_the_same_results(oracle, walks, monkeypatch):
    cases = [c for c in make_member_cases(oracle) if c.kind == "bgzf" or c.name.startswith(("lie-", "bgzf-"))]
    assert len(cases) >= 12
    monkeypatch.setenv("ZSC_HIP_MEMBERS_CLAIMS", "0")  # (read when the plan is created)
    res, clean = run_members([c.data for c in cases], [c.cap for c in cases])
    assert clean
    for c, got in zip(cases, res):
        want = walks[c.name]
        # (unclaimed, a liar is counted by decoding it: the prefix runs to the first member that is not Z_OK)
        check(c._replace(prefix=want[3]), want, got, claims=False)


def test_size_only_equals_the_size_walk(oracle):
    cases = make_member_cases(oracle)
    res, _ = run_members([c.data for c in cases], [c.cap for c in cases], size_only=True, runs=2)  # (d_dst is 0)
    for c, got in zip(cases, res):
        st, ol, _, used, members, prefix, claimed = got
        want = walk(oracle, c.data, c.cap, size_only=True)
        assert (st, ol, used, members) == want, (c.name, got, want)
        assert claimed == 0
        if c.kind in ("clean", "bgzf"):
            assert prefix == members == c.built, c.name
    # no limit at all
    few = [c for c in cases if c.name in ("clean-5-l6", "bgzf-40", "flip-isize", "cap-0")]
    res, _ = run_members([c.data for c in few], None, size_only=True)
    for c, got in zip(few, res):
        want = walk(oracle, c.data, 1 << 20, size_only=True)
        assert want[1] < 1 << 20 and (got[0], got[1], got[3], got[4]) == want, c.name


def test_seven_files_of_different_shapes_and_an_empty_plan(oracle, walks):
    import zsc_amd
    by = {c.name: c for c in make_member_cases(oracle)}
    seven = [by[n] for n in ("clean-300-empty", "clean-single-70000", "bgzf-40", "flip-crc", "empty-input",
                             "cap-inside-member-2", "gzip-in-stored-gzip")]
    res, clean = run_members([c.data for c in seven], [c.cap for c in seven])
    assert clean
    for c, got in zip(seven, res):
        check(c, walks[c.name], got)
    assert run_members([], []) == ([], True)
    rc, outs, used, stat, members = zsc_amd.uncompress_members_batch([], [])
    assert (rc, outs, used, stat, members) == (0, [], [], [], [])


def test_host_batch_and_what_a_members_plan_refuses(oracle, walks):
    import zsc_amd
    by = {c.name: c for c in make_member_cases(oracle)}
    some = [by[n] for n in ("clean-5-l6", "bgzf-3", "trailer-cut-4", "zero-pad-7")]
    rc, outs, used, stat, members = zsc_amd.uncompress_members_batch([c.data for c in some], [c.cap for c in some])
    assert rc == 0
    for i, c in enumerate(some):
        assert (stat[i], outs[i], used[i], members[i]) == walks[c.name], c.name
    rc, sizes, used, stat, members = zsc_amd.uncompress_members_batch([c.data for c in some], None, size_only=True)
    for i, c in enumerate(some):
        assert (stat[i], sizes[i], used[i], members[i]) == walk(oracle, c.data, 1 << 20, size_only=True), c.name
    # a plain plan stops behind member 0: what this plan kind is for
    prc, pouts, pused, pstat = zsc_amd.uncompress_batch([some[0].data], [some[0].cap], window_bits=GZ)
    assert pstat[0] == Z_OK and len(pouts[0]) < len(outs[0]) and pused[0] < used[0]
    for wbits in (15, -15, 47, 16 + 7):
        with pytest.raises(RuntimeError):
            zsc_amd.InflatePlan([10], [10], window_bits=wbits, members=True)
    for kw in ({"sections": True}, {"chunks": True}, {"check_only": True}, {"resync": True}, {"decode_order": [0]}):
        with pytest.raises(ValueError):
            zsc_amd.InflatePlan([10], [10], window_bits=GZ, members=True, **kw)
    plan = zsc_amd.InflatePlan([10], [10], window_bits=GZ, members=True)
    sized = zsc_amd.InflatePlan([10], None, window_bits=GZ, members=True, size_only=True)
    plain = zsc_amd.InflatePlan([10], [10], window_bits=GZ)
    try:
        assert zsc_amd.lib.zsc_hip_inflate_plan_index_enable(plan._h, 1) == zsc_amd.Z_STREAM_ERROR
        assert zsc_amd.lib.zsc_hip_inflate_plan_pack_enable(sized._h, 16) == zsc_amd.Z_STREAM_ERROR
        assert zsc_amd.lib.zsc_hip_inflate_plan_members(plain._h, None, None) == zsc_amd.Z_STREAM_ERROR
        assert plan.members() == ([0], [0]) and plan.sections() == [0]  # (before any run)
        # scratch, term by term (include/zsc_hip.h): pool slots, tiles, per file
        slots = 10 // 256 + 65536
        assert plan.scratch_bytes() == 28 * slots + 16 * 1 + 116 + 16
        assert sized.scratch_bytes() == 24 * slots + 16 * 1 + 116 + 16
    finally:
        plan.close()
        sized.close()
        plain.close()


def test_data_errors_are_the_plain_plans_on_the_member_that_failed(oracle, walks):
    """the damaged member with full-flush markers: its resynchronisations are counted as a plain plan counts
    them on file[at:], at being where that member starts"""
    import torch
    import zsc_amd
    c = {c.name: c for c in make_member_cases(oracle)}["damaged-flushed-then-more"]
    at = out = 0
    while True:  # the walk up to the member that is not Z_OK
        rc, o, used = oracle.uncompress(c.data[at:], c.cap - out, window_bits=GZ)
        if rc != Z_OK:
            break
        at, out = at + used, out + len(o)
    errors = []
    for data, cap, members in ((c.data, c.cap, True), (c.data[at:], c.cap - out, False)):
        ip = zsc_amd.InflatePlan([len(data)], [cap], window_bits=GZ, members=members)
        try:
            d_src = torch.frombuffer(bytearray(data) + bytearray(ip.src_bytes - len(data)), dtype=torch.uint8).cuda()
            d_dst = torch.zeros(ip.dst_bytes, dtype=torch.uint8, device="cuda")
            ip.run(d_src.data_ptr(), d_dst.data_ptr())
            lens, used, stat, _ = ip.results()
            assert stat == [walks[c.name][0]]
            errors.append(ip.data_errors())
        finally:
            ip.close()
    assert errors[0] == errors[1] and errors[0][0] >= 1


def test_round_trip_pack_align_1_then_a_members_plan(oracle):
    """a gzip DeflatePlan's results packed with align 1 are one multi-member gzip file: the single file of a
    members plan, as it lies in the image's tensor at a 16-byte aligned offset"""
    import torch
    import zsc_amd
    from test_gpu_deflate_verify import _buffers, _upload
    bufs = _buffers()
    dp = zsc_amd.DeflatePlan([len(b) for b in bufs], 6, GZ)
    try:
        dp.pack_enable(1)
        src = _upload(torch, dp, bufs)
        out = torch.zeros(dp.out_bytes, dtype=torch.uint8, device="cuda")
        dp.run(src.data_ptr(), out.data_ptr())
        at = 48  # (a multiple of 16 that is not 0; 64 readable bytes follow the image)
        img = torch.zeros(at + dp.out_bytes + 64, dtype=torch.uint8, device="cuda")
        assert dp.pack(out.data_ptr(), img.data_ptr() + at, dp.out_bytes) == 0
        off, total = dp.pack_results()
        assert dp.results()[1] == [0] * len(bufs)
    finally:
        dp.close()
    want = b"".join(bufs)
    image = img.cpu().numpy().tobytes()[at:at + total]
    assert gzip.decompress(image) == want
    ip = zsc_amd.InflatePlan([total], [len(want)], window_bits=GZ, members=True, src_offsets=[at])
    try:
        dst = torch.full((ip.dst_bytes,), CANARY, dtype=torch.uint8, device="cuda")
        ip.run(img.data_ptr(), dst.data_ptr())
        lens, used, stat, ms = ip.results()
        assert (stat, lens, used) == ([0], [len(want)], [total])
        assert dst.cpu().numpy().tobytes()[:len(want)] == want
        assert ip.members()[0] == [len(bufs)] and ip.sections() == [len(bufs)]
        assert ip.data_errors() == [0] and ms > 0
        # the plan's output packed again: one item, the bytes as they are
        ip.pack_enable(16)
        packed = torch.zeros(len(want) + 64, dtype=torch.uint8, device="cuda")
        assert ip.pack(dst.data_ptr(), packed.data_ptr(), len(want) + 16) == 0
        poff, ptotal = ip.pack_results()
        assert (poff, ptotal) == ([0, ptotal], (len(want) + 15) // 16 * 16)
        assert packed.cpu().numpy().tobytes()[:len(want)] == want
    finally:
        ip.close()


def test_other_kinds_are_untouched(oracle):
    """a plain plan and a sections plan on one small batch: the scratch their contract states (0; 28 bytes per
    pool slot, 16 per tile, 100 per stream and 16) and the oracle's results, with a members plan made and run
    in between"""
    import torch
    import zsc_amd
    from zsc_amd import corpus
    datas = [corpus.make_buffer("text", n, 5 + n) for n in (1, 9000, 20000)]
    streams = [oracle.compress(d, 6, window_bits=GZ, max_block_len=4096)[1] for d in datas]
    caps = [len(d) for d in datas]
    want = [oracle.uncompress(s, c, window_bits=GZ) for s, c in zip(streams, caps)]
    tiles = sum((len(s) + 4095) // 4096 for s in streams)
    expect_scratch = {False: 0, True: 28 * (sum(len(s) for s in streams) // 256 + 65536) + 16 * tiles + 100 * 3 + 16}

    def run(sections):
        ip = zsc_amd.InflatePlan([len(s) for s in streams], caps, window_bits=GZ, sections=sections)
        try:
            image = bytearray(ip.src_bytes)
            for s, off in zip(streams, ip.src_offsets):
                image[off:off + len(s)] = s
            d_src = torch.frombuffer(image, dtype=torch.uint8).cuda()
            d_dst = torch.zeros(ip.dst_bytes, dtype=torch.uint8, device="cuda")
            ip.run(d_src.data_ptr(), d_dst.data_ptr())
            lens, used, stat, _ = ip.results()
            host = d_dst.cpu().numpy()
            outs = [host[o:o + n].tobytes() for o, n in zip(ip.dst_offsets, lens)]
            with pytest.raises(RuntimeError):
                ip.members()
            return ip.scratch_bytes(), list(zip(stat, outs, used)), ip.sections()
        finally:
            ip.close()

    before = {k: run(k) for k in (False, True)}
    res, clean = run_members(streams, caps)
    assert clean and [(r[0], r[2], r[3]) for r in res] == want and [r[4] for r in res] == [1, 1, 1]
    after = {k: run(k) for k in (False, True)}
    assert before == after
    for k in (False, True):
        scratch, results, nsec = after[k]
        assert scratch == expect_scratch[k]
        assert results == want
        assert all(n > 1 for n in nsec[1:]) if k else nsec == [0, 0, 0]
