"""The device plans held to stream order (include/zsc_hip.h, "Streams").

Every other GPU test stages its input synchronously and runs on an idle device, most of them on stream 0, so a
launch, memset or copy that run() issued on the wrong stream, a host-side read of device state that is not ready
yet, or state shared between two plans would pass there.  Here every run() is enqueued on a side stream BEHIND
device work that is still running when the enqueue calls return, with its input produced by a copy on that
stream and its output consumed and then clobbered by work enqueued behind it:

  T1  behind a producer, in front of a consumer.  src holds batch A (damaged streams, noise, or a zero-filled
      decoy), a staging tensor batch B.  On a side stream: the delay, an event, src.copy_(staging), run(), for a
      DeflatePlan pack(), then snap.copy_(dst) and dst.fill_(0x5A).  Everything the plan reports must be what a
      fresh plan reports on B by the synchronous path -- the oracle's --, snap must hold B's outputs in the slots
      and the canary outside them.  A launch on another stream would have read A, or written after the snapshot.
  T2  three plans in flight on three streams, read in reverse order, closed in the order of enqueue.
  T3  one plan, two streams: run(X = A, O1) on s1 behind the delay, run(Y = B, O2) on s2 at once.  results()
      must have waited for all of it and be Y's, twice; O1 holds X's outputs and O2 Y's.
  T4  close() right behind a verify(), a pack() or a run() on a side stream returns only when that work is done,
      and the blocks it hands back to the cache serve a fresh plan well.

The delay is torch.cuda._sleep, calibrated once per module against HIP events, and every test records an event
directly behind its delay and asserts `not ev.query()` right after its last enqueue call: a test whose delay
was already over proves nothing, so it fails.  Afterwards the delay's device time is asserted to have been at
least 50 ms.

Measured on the MI355X (time.perf_counter around the enqueue calls that must fit inside the delay, printed by
every test as "enqueue ... ms"): 0.014 ms (a pack before close()), 0.06 to 0.22 ms (T1: copy, run, pack, snapshot
and clobber), 0.32 ms (T2: from the first job's copy to the last job's clobber, the other two delays included).
The delay chosen from it: 100 ms, 300 times the longest of them and twice the 50 ms floor.

What fails on the commit before the streams rule, reasoned from its code (zsc_amd/csrc/zsc_hip_runtime.hip):
  * T3: run() only stored `last_stream = st`, and _results waited for last_stream alone.  The second run
    (on s2, nothing in front of it) was over while the first still sat behind the delay on s1, so results()
    returned with e1 pending ("the accessors waited for all of the plan's work" fails), it reported Y's records
    before run X overwrote the same d_res, and the second results() -- after X -- reported X's: it differs from
    the first.  Both runs also shared every scratch array.
  * T4, verify: _destroy waited for last_stream and pack.stream, not for vf_stream, so close() returned with
    k_verify_blocks and k_verify_finish still queued and their buffers back in the cache: the event behind
    the delay is not complete when close() returns.  The pack and run cases passed before; they are pinned.

A superseded run of an inflate plan: the resynchronisation of damaged streams finishes in _results, for the
plan's last run only, so in T3 the slots of O1 are compared for the streams of X in which a decoder meets no
data error (a short capacity, clean streams: complete at the end of run(); CPython's zlib says which they
are); what the slot of a stream holds between its data error and its relaunch is left open by the contract.
"""
import time

import numpy as np
import pytest

import inflate_dict_cases as idc
import surroundings as sr
import test_gpu_inflate_dict as tid
import test_gpu_plan_rerun as rr

pytestmark = pytest.mark.gpu

DELAY_MS = 100.0  # (see the docstring)
LEAST_DELAY_MS = 50.0
CLOBBER = 0x5A
IDX_CHUNK = 4096
DEFLATE_PLANS = {  # name: (source lengths, level, window_bits, cut into two sub-batches)
    "l6-zlib": (rr.DEFLATE_LENS, 6, 15, False),
    "l1-gzip": (rr.DEFLATE_LENS, 1, 31, False),
    "l9-raw": (rr.DEFLATE_LENS, 9, -15, False),
    "two-sub-batches": (rr.DEFLATE_LENS * 6, 6, 15, True),
}
DICT_WBITS = (-15, 15)


class Gpu:
    """torch, three side streams (with stream 0 they take the four hardware queues a process has by default; more
    would share a queue and serialise falsely) and the delay"""

    def __init__(self):
        import torch
        self.torch = torch
        self.streams = [torch.cuda.Stream() for _ in range(3)]
        torch.cuda._sleep(1000)  # (loads the kernel)
        torch.cuda.synchronize()
        cycles = 1 << 20
        while True:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(cycles)
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
            if ms >= 5.0 or cycles >= 1 << 36:
                break
            cycles *= 8
        assert ms >= 5.0, "torch.cuda._sleep does not wait"
        self.cycles_per_ms = cycles / ms

    def delay(self, stream):
        """the delay at the head of `stream` and the event directly behind it (with one in front, to time it)"""
        torch = self.torch
        before, ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            before.record(stream)
            torch.cuda._sleep(int(DELAY_MS * self.cycles_per_ms))
            ev.record(stream)
        return Delay(before, ev)

    def delay_was_long_enough(self, delay):
        delay.ev.synchronize()
        ms = delay.before.elapsed_time(delay.ev)
        assert ms >= LEAST_DELAY_MS, f"the delay took {ms:.1f} ms of device time"


class Delay:
    def __init__(self, before, ev):
        self.before, self.ev = before, ev

    def query(self):
        """is the event directly behind the delay complete?"""
        return self.ev.query()


@pytest.fixture(scope="module")
def gpu():
    g = Gpu()
    yield g
    g.torch.cuda.synchronize()


def still_delayed(ev, what, t0):
    """right after the last enqueue call: the delay in front of it all must not be over"""
    ms = (time.perf_counter() - t0) * 1e3
    print(f"enqueue {what}: {ms:.3f} ms on the host, delay {DELAY_MS:.0f} ms")
    assert not ev.query(), f"{what}: the delay was over after the enqueue calls ({ms:.1f} ms): the test proves nothing"


_memo = {}


# ---- deflate ---------------------------------------------------------------------------------------------------

def make_deflate_plan(name, monkeypatch, features=True):
    import zsc_amd
    lens, level, wbits, two = DEFLATE_PLANS[name]
    if two:
        monkeypatch.setenv("ZSC_HIP_SUBBATCH_MB", "1")  # (read when the plan is created)
    try:
        plan = zsc_amd.DeflatePlan(list(lens), level, wbits)
    finally:
        if two:
            monkeypatch.delenv("ZSC_HIP_SUBBATCH_MB")
    assert not two or plan.sub_batches >= 2
    if features:
        plan.index_enable(IDX_CHUNK)
        plan.verify_enable()
        plan.pack_enable(16)
    return plan


def deflate_images(name, plan):
    """the host images of batch A (noise) and batch B (text and zeros), noise around the items; and the items"""
    if name not in _memo:
        a, b = rr.deflate_batches(DEFLATE_PLANS[name][0], 60)
        _memo[name] = (a, b, sr.place(a, plan.in_offsets, plan.in_bytes, "noise", 9),
                       sr.place(b, plan.in_offsets, plan.in_bytes, "noise", 9))
    return _memo[name]


def deflate_said(plan, src, out, img):
    """after results(), everything at rest: what the plan reports, read on stream 0 -- the verdicts of verify()
    on `out` (the run's output or a copy of it), the packed image's table, the blobs"""
    import zsc_amd
    lens, stat = plan.results()
    assert plan.verify(src.data_ptr(), out.data_ptr()) == 0
    verdicts = [v["verdict"] for v in plan.verify_results()]
    assert verdicts == [zsc_amd.VERIFY_OK] * plan.count, verdicts
    return {"lens": lens, "stat": stat, "verdicts": verdicts, "pack": plan.pack_results(),
            "blobs": plan.export_indexes(src.data_ptr())}


def check_deflate(oracle, name, items, plan_offsets, said, out_host, img_host, canary, caps):
    """against the oracle: statuses, streams in the slots, the canary outside them, the packed image, the indexes"""
    import zsc_amd
    _, level, wbits, _ = DEFLATE_PLANS[name]
    wants = sr.want_deflate(oracle, items, level, wbits, 0)
    assert said["stat"] == [0] * len(items)
    assert said["lens"] == [len(w) for w in wants]
    for it, off, w in zip(items, plan_offsets, wants):
        assert out_host[off:off + len(w)].tobytes() == w, it.name
    sr.assert_outside_untouched(out_host, plan_offsets, caps, canary)
    offsets, total = said["pack"]
    assert total == offsets[-1] and all(o % 16 == 0 for o in offsets[:-1])
    image = img_host.tobytes()
    for it, off, w in zip(items, offsets, wants):
        assert image[off:off + len(w)] == w, ("packed", it.name)
    assert all(b is not None for b in said["blobs"])
    rc, outs, used, stat = zsc_amd.uncompress_indexed_batch(wants, [len(it.data) for it in items], said["blobs"],
                                                             window_bits=wbits)
    assert rc == 0 and stat == [0] * len(items) and used == [len(w) for w in wants]
    assert outs == [it.data for it in items]


def fresh_deflate(gpu, oracle, name, monkeypatch):
    """a fresh plan on B by the synchronous path, checked against the oracle; kept for every test that needs it"""
    key = ("fresh-deflate", name)
    if key in _memo:
        return _memo[key]
    torch = gpu.torch
    plan = make_deflate_plan(name, monkeypatch)
    try:
        _, b, _, image_b = deflate_images(name, plan)
        src = torch.from_numpy(image_b).cuda()
        dst = sr.canary_image(torch, plan.out_bytes, 0xFF)
        img = torch.zeros(plan.out_bytes, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        plan.run(src.data_ptr(), dst.data_ptr())
        plan.results()
        assert plan.pack(dst.data_ptr(), img.data_ptr(), plan.out_bytes) == 0
        said = deflate_said(plan, src, dst, img)
        check_deflate(oracle, name, b, plan.out_offsets, said, dst.cpu().numpy(), img.cpu().numpy(), 0xFF, plan.out_caps)
    finally:
        plan.close()
    _memo[key] = said
    return said


class DeflateJob:
    """T1's steps for a DeflatePlan with index, verify and pack enabled"""

    def __init__(self, gpu, name, monkeypatch):
        torch = gpu.torch
        self.gpu, self.name = gpu, name
        self.plan = plan = make_deflate_plan(name, monkeypatch)
        _, self.items, image_a, image_b = deflate_images(name, plan)
        self.src = torch.from_numpy(image_a).cuda()
        self.staging = torch.from_numpy(image_b).cuda()
        self.dst = sr.canary_image(torch, plan.out_bytes, 0xFF)
        self.snap = torch.zeros(plan.out_bytes, dtype=torch.uint8, device="cuda")
        self.img = torch.zeros(plan.out_bytes, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def enqueue(self, side):
        torch, plan = self.gpu.torch, self.plan
        self.side = side
        self.ev = self.gpu.delay(side)
        self.t0 = time.perf_counter()
        with torch.cuda.stream(side):
            self.src.copy_(self.staging, non_blocking=True)
            plan.run(self.src.data_ptr(), self.dst.data_ptr(), side.cuda_stream)
            assert plan.pack(self.dst.data_ptr(), self.img.data_ptr(), plan.out_bytes, side.cuda_stream) == 0
            self.snap.copy_(self.dst, non_blocking=True)
            self.dst.fill_(CLOBBER)

    def check_delay(self):
        still_delayed(self.ev, f"deflate {self.name}", self.t0)

    def collect(self, oracle, fresh):
        plan = self.plan
        first = plan.results()
        self.side.synchronize()
        self.gpu.delay_was_long_enough(self.ev)
        said = deflate_said(plan, self.src, self.snap, self.img)
        assert first == (said["lens"], said["stat"])
        check_deflate(oracle, self.name, self.items, plan.out_offsets, said, self.snap.cpu().numpy(),
                      self.img.cpu().numpy(), 0xFF, plan.out_caps)
        assert said == fresh, "not what a fresh plan reports on B by the synchronous path"
        assert (self.dst.cpu().numpy() == CLOBBER).all()

    def close(self):
        self.plan.close()


@pytest.mark.parametrize("name", list(DEFLATE_PLANS))
def test_a_deflate_plan_behind_a_producer_and_in_front_of_a_consumer(gpu, oracle, monkeypatch, name):
    fresh = fresh_deflate(gpu, oracle, name, monkeypatch)
    job = DeflateJob(gpu, name, monkeypatch)
    try:
        job.enqueue(gpu.streams[0])
        job.check_delay()
        job.collect(oracle, fresh)
    finally:
        gpu.torch.cuda.synchronize()
        job.close()


# ---- inflate ---------------------------------------------------------------------------------------------------

def inflate_batches(gpu, oracle, kind):
    """(A items, B items, window_bits, blobs) of test_gpu_plan_rerun.py"""
    key = ("batches", kind)
    if key not in _memo:
        a, b, wbits = rr.batches(oracle, kind)
        assert [len(x.data) for x in a] == [len(y.data) for y in b]
        blobs = sr.build_blobs(gpu.torch, b, wbits) if kind == "indexed" else None
        _memo[key] = (a, b, wbits, blobs)
    return _memo[key]


def fresh_inflate(gpu, oracle, kind):
    """(results, everything else the plan reports) of a fresh plan on B by the synchronous path; the results are
    the oracle's"""
    key = ("fresh-inflate", kind)
    if key in _memo:
        return _memo[key]
    _, b, wbits, blobs = inflate_batches(gpu, oracle, kind)
    r = rr.Runner(gpu.torch, kind, b, wbits, blobs)
    try:
        got = r.run(b, 7)
    finally:
        r.close()
    for it, g in zip(b, got[0]):
        w = rr.want(oracle, kind, it, wbits)
        assert g == w, ("a fresh plan", it.name, sr.brief(g), sr.brief(w))
    _memo[key] = got
    return got


class InflateJob:
    """T1's steps for an inflate plan of any kind: image_a is what src holds, image_b what the staging tensor
    holds (host images laid out by the plan's offsets)"""

    def __init__(self, gpu, what, plan, caps, image_a, image_b, writes=True):
        torch = gpu.torch
        self.gpu, self.what, self.plan, self.caps = gpu, what, plan, caps
        plan._surroundings_caps = caps
        self.src = torch.from_numpy(image_a).cuda()
        self.staging = torch.from_numpy(image_b).cuda()
        self.dst = sr.canary_image(torch, plan.dst_bytes) if writes else None
        self.snap = torch.zeros(plan.dst_bytes, dtype=torch.uint8, device="cuda") if writes else None
        torch.cuda.synchronize()

    def enqueue(self, side):
        torch, plan = self.gpu.torch, self.plan
        self.side = side
        self.ev = self.gpu.delay(side)
        self.t0 = time.perf_counter()
        with torch.cuda.stream(side):
            self.src.copy_(self.staging, non_blocking=True)
            plan.run(self.src.data_ptr(), self.dst.data_ptr() if self.dst is not None else 0, side.cuda_stream)
            if self.dst is not None:
                self.snap.copy_(self.dst, non_blocking=True)
                self.dst.fill_(CLOBBER)

    def check_delay(self):
        still_delayed(self.ev, f"inflate {self.what}", self.t0)

    def collect(self):
        """-> (lens, consumed, statuses), the host copy of snap (None for a plan that writes nothing)"""
        lens, used, stat, _ = self.plan.results()
        self.side.synchronize()
        self.gpu.delay_was_long_enough(self.ev)
        host = None
        if self.dst is not None:
            host = self.snap.cpu().numpy()
            sr.assert_outside_untouched(host, self.plan.dst_offsets, self.caps)
            assert (self.dst.cpu().numpy() == CLOBBER).all()
        return (lens, used, stat), host

    def close(self):
        self.plan.close()


def inflate_job(gpu, oracle, kind):
    a, b, wbits, blobs = inflate_batches(gpu, oracle, kind)
    caps = [it.cap for it in b]
    plan = sr.make_inflate_plan(kind, [len(it.data) for it in b], caps, wbits, None, blobs)
    return InflateJob(gpu, kind, plan, caps, sr.place(a, plan.src_offsets, plan.src_bytes, "noise", 7),
                      sr.place(b, plan.src_offsets, plan.src_bytes, "noise", 7), sr.writes(kind))


def collect_like_the_rerun_test(job, kind):
    """what test_gpu_plan_rerun.Runner.run() returns, from the job's snapshot"""
    plan = job.plan
    first, host = job.collect()
    res = sr.read_inflate(plan, kind, host)
    assert first == tuple(plan.results()[:3])
    said = {"data_errors": plan.data_errors(), "sections": plan.sections()}
    if kind == "members":
        memb, claimed = plan.members()
        res = [r + (m,) for r, m in zip(res, memb)]
        said["claimed"] = claimed
    if kind == "check":
        res = [r + (v,) for r, v in zip(res, plan.check_values())]
    return res, said


def check_inflate(gpu, oracle, kind, got, fresh):
    _, b, wbits, _ = inflate_batches(gpu, oracle, kind)
    for it, g in zip(b, got[0]):
        w = rr.want(oracle, kind, it, wbits)
        assert g == w, (it.name, sr.brief(g), sr.brief(w))
    assert got[0] == fresh[0]
    assert got[1] == fresh[1], (got[1], fresh[1])
    assert got[1]["data_errors"] == [0] * len(b)


@pytest.mark.parametrize("kind", rr.KINDS)
def test_an_inflate_plan_behind_a_producer_and_in_front_of_a_consumer(gpu, oracle, kind):
    fresh = fresh_inflate(gpu, oracle, kind)
    job = inflate_job(gpu, oracle, kind)
    try:
        job.enqueue(gpu.streams[1])
        job.check_delay()
        check_inflate(gpu, oracle, kind, collect_like_the_rerun_test(job, kind), fresh)
    finally:
        gpu.torch.cuda.synchronize()
        job.close()


@pytest.mark.parametrize("wbits", DICT_WBITS)
def test_a_plan_with_dictionaries_behind_a_producer_and_in_front_of_a_consumer(gpu, wbits):
    import zsc_amd
    group = [c for c in idc.all_cases() if c.wbits == wbits]
    assert len(group) >= 8 and {c.status for c in group} >= {0, -3}
    dicts, of = tid.dict_table(group)
    streams = [c.stream for c in group]

    def make_plan():
        return zsc_amd.InflatePlan([len(s) for s in streams], [c.cap for c in group], wbits, dicts=dicts, stream_dict=of)

    plan = make_plan()
    try:
        fresh = tid.run_plan(plan, streams)
    finally:
        plan.close()
    tid.check(group, fresh, ("a fresh plan", wbits))
    plan = make_plan()
    image_b = np.zeros(plan.src_bytes, np.uint8)
    for s, off in zip(streams, plan.src_offsets):
        image_b[off:off + len(s)] = np.frombuffer(s, np.uint8)
    job = InflateJob(gpu, f"dictionaries {wbits}", plan, [c.cap for c in group], np.zeros(plan.src_bytes, np.uint8), image_b)
    try:
        job.enqueue(gpu.streams[2])
        job.check_delay()
        (lens, used, stat), host = job.collect()
        got = [(st, host[off:off + n].tobytes(), u) for off, n, u, st in zip(plan.dst_offsets, lens, used, stat)]
        tid.check(group, got, ("behind the delay", wbits))
        assert got == fresh
    finally:
        gpu.torch.cuda.synchronize()
        job.close()


# ---- T2 ----------------------------------------------------------------------------------------------------------

def test_three_plans_in_flight(gpu, oracle, monkeypatch):
    fresh_d = fresh_deflate(gpu, oracle, "l6-zlib", monkeypatch)
    fresh_c, fresh_m = fresh_inflate(gpu, oracle, "chunks"), fresh_inflate(gpu, oracle, "members")
    jobs = []
    try:
        jobs.append(DeflateJob(gpu, "l6-zlib", monkeypatch))
        jobs.append(inflate_job(gpu, oracle, "chunks"))
        jobs.append(inflate_job(gpu, oracle, "members"))
        for job, side in zip(jobs, gpu.streams):
            job.enqueue(side)
        for job in jobs:
            job.check_delay()
        # read in the reverse order of enqueue
        check_inflate(gpu, oracle, "members", collect_like_the_rerun_test(jobs[2], "members"), fresh_m)
        check_inflate(gpu, oracle, "chunks", collect_like_the_rerun_test(jobs[1], "chunks"), fresh_c)
        jobs[0].collect(oracle, fresh_d)
    finally:
        gpu.torch.cuda.synchronize()
        for job in jobs:  # closed in the order of enqueue
            job.close()


# ---- T3 ----------------------------------------------------------------------------------------------------------

def two_streams(gpu, plan, x, y, o1, o2, what):
    """run(x, o1) on s1 behind the delay, run(y, o2) on s2 at once; -> the first results(), which must have
    waited for both runs, and must be what results() says again when the device is idle"""
    torch = gpu.torch
    s1, s2 = gpu.streams[0], gpu.streams[1]
    e0 = gpu.delay(s1)
    t0 = time.perf_counter()
    plan.run(x.data_ptr(), o1.data_ptr(), s1.cuda_stream)
    e1 = torch.cuda.Event()
    e1.record(s1)
    plan.run(y.data_ptr(), o2.data_ptr(), s2.cuda_stream)
    still_delayed(e0, f"{what}, two streams", t0)
    first = plan.results()
    assert e1.query(), "results() returned while the plan's run on the other stream was pending"
    torch.cuda.synchronize()
    gpu.delay_was_long_enough(e0)
    again = plan.results()
    assert tuple(first)[:3] == tuple(again)[:3], "results() changed after it had returned"
    return first


def test_one_deflate_plan_on_two_streams(gpu, oracle, monkeypatch):
    torch = gpu.torch
    name = "l6-zlib"
    _, level, wbits, _ = DEFLATE_PLANS[name]
    plan = make_deflate_plan(name, monkeypatch, features=False)
    try:
        a, b, image_a, image_b = deflate_images(name, plan)
        x, y = torch.from_numpy(image_a).cuda(), torch.from_numpy(image_b).cuda()
        o1, o2 = sr.canary_image(torch, plan.out_bytes, 0xFF), sr.canary_image(torch, plan.out_bytes, 0xFF)
        torch.cuda.synchronize()
        lens, stat = two_streams(gpu, plan, x, y, o1, o2, "deflate")
        want_x, want_y = (sr.want_deflate(oracle, v, level, wbits, 0) for v in (a, b))
        assert stat == [0] * len(b) and lens == [len(w) for w in want_y], "the results are not the last run's"
        for out, wants, items in ((o1, want_x, a), (o2, want_y, b)):
            host = out.cpu().numpy()
            sr.assert_outside_untouched(host, plan.out_offsets, plan.out_caps, 0xFF)
            for it, off, w in zip(items, plan.out_offsets, wants):
                assert host[off:off + len(w)].tobytes() == w, it.name
    finally:
        torch.cuda.synchronize()
        plan.close()


def meets_a_data_error(item, wbits):
    """does a decoder meet a data error in the item before its output reaches the capacity?  (CPython's zlib says;
    it stops where the capacity is reached, as zsc_uncompress does)"""
    import zlib
    if item.cap == 0:
        return False
    try:
        zlib.decompressobj(wbits).decompress(item.data, item.cap)
    except zlib.error:
        return True
    return False


def test_one_chunks_plan_on_two_streams(gpu, oracle):
    torch = gpu.torch
    kind = "chunks"
    a, b, wbits, _ = inflate_batches(gpu, oracle, kind)
    fresh = fresh_inflate(gpu, oracle, kind)
    caps = [it.cap for it in b]
    plan = sr.make_inflate_plan(kind, [len(it.data) for it in b], caps, wbits, None)
    plan._surroundings_caps = caps
    try:
        x = torch.from_numpy(sr.place(a, plan.src_offsets, plan.src_bytes, "noise", 7)).cuda()
        y = torch.from_numpy(sr.place(b, plan.src_offsets, plan.src_bytes, "noise", 7)).cuda()
        o1, o2 = sr.canary_image(torch, plan.dst_bytes), sr.canary_image(torch, plan.dst_bytes)
        torch.cuda.synchronize()
        two_streams(gpu, plan, x, y, o1, o2, "inflate chunks")
        host1, host2 = o1.cpu().numpy(), o2.cpu().numpy()
        got = sr.read_inflate(plan, kind, host2), {"data_errors": plan.data_errors(), "sections": plan.sections()}
        check_inflate(gpu, oracle, kind, got, fresh)
        for host in (host1, host2):
            sr.assert_outside_untouched(host, plan.dst_offsets, caps)
        compared = 0
        for it, off in zip(a, plan.dst_offsets):
            if not meets_a_data_error(it, wbits):  # (see the module docstring: a superseded run is never resynchronised)
                out = rr.want(oracle, kind, it, wbits)[1]
                assert host1[off:off + len(out)].tobytes() == out, it.name
                compared += 1
        assert compared >= 3
    finally:
        torch.cuda.synchronize()
        plan.close()


# ---- T4 ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("work", ["verify", "pack", "run"])
def test_closing_a_deflate_plan_waits_for_its_work(gpu, oracle, monkeypatch, work):
    torch = gpu.torch
    name = "l6-zlib"
    fresh = fresh_deflate(gpu, oracle, name, monkeypatch)
    side = gpu.streams[2]
    plan = make_deflate_plan(name, monkeypatch)
    closed = False
    try:
        _, b, _, image_b = deflate_images(name, plan)
        src = torch.from_numpy(image_b).cuda()
        dst = sr.canary_image(torch, plan.out_bytes, 0xFF)
        img = torch.zeros(plan.out_bytes, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        plan.run(src.data_ptr(), dst.data_ptr())
        plan.results()
        ev = gpu.delay(side)
        t0 = time.perf_counter()
        if work == "verify":
            assert plan.verify(src.data_ptr(), dst.data_ptr(), side.cuda_stream) == 0
        elif work == "pack":
            assert plan.pack(dst.data_ptr(), img.data_ptr(), plan.out_bytes, side.cuda_stream) == 0
        else:
            plan.run(src.data_ptr(), dst.data_ptr(), side.cuda_stream)
        still_delayed(ev, f"deflate {work} before close()", t0)
        plan.close()
        closed = True
        assert ev.query(), f"close() returned while the {work} on the side stream was pending"
        torch.cuda.synchronize()
        gpu.delay_was_long_enough(ev)
        # the cache handed out sound blocks: a fresh plan of the same shape, run once
        del _memo[("fresh-deflate", name)]
        assert fresh_deflate(gpu, oracle, name, monkeypatch) == fresh
    finally:
        torch.cuda.synchronize()
        _memo[("fresh-deflate", name)] = fresh
        if not closed:
            plan.close()


@pytest.mark.parametrize("work", ["pack", "run"])
def test_closing_an_inflate_plan_waits_for_its_work(gpu, oracle, work):
    torch = gpu.torch
    kind = "chunks"
    _, b, wbits, _ = inflate_batches(gpu, oracle, kind)
    fresh = fresh_inflate(gpu, oracle, kind)
    side = gpu.streams[0]
    caps = [it.cap for it in b]
    plan = sr.make_inflate_plan(kind, [len(it.data) for it in b], caps, wbits, None)
    closed = False
    try:
        plan.pack_enable(16)
        src = torch.from_numpy(sr.place(b, plan.src_offsets, plan.src_bytes, "noise", 7)).cuda()
        dst = sr.canary_image(torch, plan.dst_bytes)
        img = torch.zeros(plan.dst_bytes, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        plan.run(src.data_ptr(), dst.data_ptr())
        plan.results()
        ev = gpu.delay(side)
        t0 = time.perf_counter()
        if work == "pack":
            assert plan.pack(dst.data_ptr(), img.data_ptr(), plan.dst_bytes, side.cuda_stream) == 0
        else:
            plan.run(src.data_ptr(), dst.data_ptr(), side.cuda_stream)
        still_delayed(ev, f"inflate {work} before close()", t0)
        plan.close()
        closed = True
        assert ev.query(), f"close() returned while the {work} on the side stream was pending"
        torch.cuda.synchronize()
        gpu.delay_was_long_enough(ev)
        del _memo[("fresh-inflate", kind)]
        assert fresh_inflate(gpu, oracle, kind) == fresh
    finally:
        torch.cuda.synchronize()
        _memo[("fresh-inflate", kind)] = fresh
        if not closed:
            plan.close()
