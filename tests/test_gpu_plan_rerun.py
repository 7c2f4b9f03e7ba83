"""One plan object run on two different batches: what the first run left in the plan's scratch and in the
output must not reach the second run's results.

For each kind of inflate plan and for a DeflatePlan, one object is run on batch A and then on batch B, a
second one on B and then on A.  The input is uploaded again between the runs (into the same tensor, noise
around the items) and the output is NOT cleared.  The second run's results must be the oracle's, and
everything the plan reports must be what a freshly created plan reports on that batch; no byte outside the
slots may differ from what the first run left there.

Inflate: source_lens[i] = max(len(A_i), len(B_i)), the shorter stream padded with seeded noise (the expected
value is the oracle's on exactly those padded bytes).  A uses the scratch hard -- damaged and truncated
streams, capacities too short, full-flush streams with false markers in stored data, a damaged stream of more
than three chunks, a multi-member file with a bad member --, B is clean: after B, data_errors() is all zero.
The blobs of an indexed plan fix the streams, so there A is a damaged copy of B.  Deflate: equal lengths, A
noise (many stored blocks), B text and zeros (few blocks), once cut into two sub-batches.
"""
import numpy as np
import pytest

import surroundings as sr
from zsc_amd import corpus

pytestmark = pytest.mark.gpu

KINDS = sr.INFLATE_KINDS + ("members",)
WBITS = 15


def _c(oracle, data, level=6, wbits=WBITS, **kw):
    rc, s, _ = oracle.compress(data, level, window_bits=wbits, **kw)
    assert rc == 0
    return s


def _flip(s, at, mask=0x5a, n=1):
    b = bytearray(s)
    for j in range(at, at + n):
        b[j] ^= mask
    return bytes(b)


def _pad(s, n, seed):
    return s + np.random.default_rng(seed).integers(0, 256, n - len(s), dtype=np.uint8).tobytes()


_memo = {}


def stream_pairs(oracle):
    """[(name, A_i, B_i, cap_i)] at window_bits 15, both padded to one length; cap_i is B_i's output"""
    if "streams" in _memo:
        return _memo["streams"]

    def text(n, seed):
        return corpus.make_buffer("text", n, seed)

    flushed = _c(oracle, text(9000, 41), max_block_len=1024)
    markers = bytearray(text(6000, 42))
    for p in range(40, len(markers) - 8, 211):
        markers[p:p + 4] = b"\x00\x00\xff\xff"
    false_markers = _c(oracle, bytes(markers), 0, max_block_len=1500)
    assert false_markers.count(b"\x00\x00\xff\xff") > 20
    long_a = _c(oracle, text(24000, 43), mem_level=3)
    long_b = _c(oracle, text(24000, 44), mem_level=3)
    assert min(len(long_a), len(long_b)) > 3 * sr.CHUNK
    pairs = [
        ("damaged", _flip(_c(oracle, text(5000, 45)), 900), _c(oracle, text(5000, 46)), 5000),
        ("truncated", _c(oracle, text(5000, 47))[:1100], _c(oracle, text(4000, 48)), 4000),
        ("short-cap", _c(oracle, text(6000, 49)), _c(oracle, text(3000, 50)), 3000),
        ("false-markers", false_markers, _c(oracle, text(9000, 51), max_block_len=1024), 9000),
        ("damaged-flushed", _flip(flushed, len(flushed) // 2, n=6), _c(oracle, text(9000, 52), max_block_len=2048), 9000),
        ("damaged-three-chunks", _flip(long_a, 9000, n=4), long_b, 24000),
        ("cap-0", _c(oracle, text(300, 53)), _c(oracle, b""), 0),
        ("one-byte", _flip(_c(oracle, b"z"), 3), _c(oracle, b"y"), 1),
        ("small", _c(oracle, bytes(range(100)) * 3)[:-2], _c(oracle, bytes(range(100, 200)) * 3), 300),
    ]
    out = []
    for j, (name, a, b, cap) in enumerate(pairs):
        n = max(len(a), len(b))
        out.append((name, _pad(a, n, 100 + j), _pad(b, n, 200 + j), cap))
    _memo["streams"] = out
    return out


def member_pairs(oracle):
    if "members" in _memo:
        return _memo["members"]
    from test_inflate_members_emu import make_member_cases
    by = {c.name: c for c in make_member_cases(oracle)}
    pairs = [("bad-crc", "flip-crc", "clean-5-l6"), ("damaged-flushed", "damaged-flushed-then-more", "clean-flushed-middle"),
             ("truncated", "trailer-cut-4", "bgzf-3"), ("liar", "lie-bsize-small", "clean-2-l1"),
             ("short-cap", "clean-5-l9", "clean-2-l6")]
    out = []
    for j, (name, a, b) in enumerate(pairs):
        n = max(len(by[a].data), len(by[b].data))
        out.append((name, _pad(by[a].data, n, 300 + j), _pad(by[b].data, n, 400 + j), by[b].cap))
    _memo["members"] = out
    return out


def batches(oracle, kind):
    """-> (A items, B items, window_bits)"""
    members = kind == "members"
    pairs = member_pairs(oracle) if members else stream_pairs(oracle)
    a = [sr.Item(f"A-{name}", x, cap) for name, x, _, cap in pairs]
    b = [sr.Item(f"B-{name}", y, cap) for name, _, y, cap in pairs]
    if kind == "indexed":  # the blobs are B's: A is a damaged copy of B
        a = [sr.Item(f"A-damaged-{it.name}", _flip(it.data, len(it.data) // 3, n=2), it.cap) for it in b]
    return a, b, sr.GZ if members else WBITS


def want(oracle, kind, item, wbits):
    return sr.want_inflate(oracle, kind, item, wbits)


class Runner:
    """one plan object, its input tensor and its output tensor, which is filled with the canary once"""

    def __init__(self, torch, kind, items, wbits, blobs):
        self.torch, self.kind = torch, kind
        self.caps = [it.cap for it in items]
        self.plan = sr.make_inflate_plan(kind, [len(it.data) for it in items], self.caps, wbits, None, blobs)
        self.plan._surroundings_caps = self.caps
        self.src = torch.zeros(self.plan.src_bytes, dtype=torch.uint8, device="cuda")
        self.dst = sr.canary_image(torch, self.plan.dst_bytes) if sr.writes(kind) else None
        self.before = None if self.dst is None else self.dst.cpu().numpy()

    def run(self, items, seed):
        """-> (results, everything else the plan reports)"""
        plan, torch = self.plan, self.torch
        self.src.copy_(torch.from_numpy(sr.place(items, plan.src_offsets, plan.src_bytes, "noise", seed)))
        torch.cuda.synchronize()
        plan.run(self.src.data_ptr(), self.dst.data_ptr() if self.dst is not None else 0)
        host = self.dst.cpu().numpy() if self.dst is not None else None
        res = sr.read_inflate(plan, self.kind, host)
        if host is not None:
            sr.assert_outside_untouched(host, plan.dst_offsets, self.caps, self.before)
            self.before = host
        said = {"data_errors": plan.data_errors(), "sections": plan.sections()}
        if self.kind == "members":
            memb, claimed = plan.members()
            res = [r + (m,) for r, m in zip(res, memb)]
            said["claimed"] = claimed
        if self.kind == "check":
            res = [r + (v,) for r, v in zip(res, plan.check_values())]
        return res, said

    def close(self):
        self.plan.close()


@pytest.mark.parametrize("kind", KINDS)
def test_an_inflate_plan_run_on_another_batch(oracle, kind):
    import torch
    a, b, wbits = batches(oracle, kind)
    assert [len(x.data) for x in a] == [len(y.data) for y in b]
    blobs = sr.build_blobs(torch, b, wbits) if kind == "indexed" else None
    if blobs is not None:
        assert sum(x is not None for x in blobs) >= 3
    wants = {"A": [want(oracle, kind, it, wbits) for it in a], "B": [want(oracle, kind, it, wbits) for it in b]}
    assert all(w[0] == 0 for w in wants["B"]), "B is clean"
    assert {w[0] for w in wants["A"]} >= ({sr.Z_DATA_ERROR} if kind == "indexed" else {sr.Z_DATA_ERROR, sr.Z_BUF_ERROR})
    items = {"A": a, "B": b}
    fresh = {}
    for which in "AB":
        r = Runner(torch, kind, items[which], wbits, blobs)
        try:
            fresh[which] = r.run(items[which], 7)
        finally:
            r.close()
        for it, g, w in zip(items[which], fresh[which][0], wants[which]):
            assert g == w, ("a fresh plan", it.name, sr.brief(g), sr.brief(w))
    assert fresh["B"][1]["data_errors"] == [0] * len(b)
    for first, second in ("AB", "BA"):
        r = Runner(torch, kind, items[first], wbits, blobs)
        try:
            assert r.run(items[first], 7) == fresh[first], f"the first run, on {first}"
            res, said = r.run(items[second], 7)
        finally:
            r.close()
        for it, g, w in zip(items[second], res, wants[second]):
            assert g == w, (f"{second} after {first}", it.name, sr.brief(g), sr.brief(w))
        assert said == fresh[second][1], (f"{second} after {first}", said, fresh[second][1])
        if second == "B":
            assert said["data_errors"] == [0] * len(b)


DEFLATE_LENS = (16, 300, 3072, 3088, 20000, 70000, 120000)


def deflate_batches(lens, seed):
    a = [sr.Item(f"A-noise-{n}", corpus.make_buffer("random", n, seed + j), 0) for j, n in enumerate(lens)]
    b = []
    for j, n in enumerate(lens):
        half = n // 2
        b.append(sr.Item(f"B-text-zeros-{n}", corpus.make_buffer("text", half, seed + 50 + j) + bytes(n - half), 0))
    return a, b


def deflate_rerun(torch, oracle, lens, level, wbits, make_plan):
    a, b = deflate_batches(lens, 60)
    items = {"A": a, "B": b}
    wants = {k: [(0, s) for s in sr.want_deflate(oracle, v, level, wbits, 0)] for k, v in items.items()}
    assert sum(len(s) for _, s in wants["A"]) > 3 * sum(len(s) for _, s in wants["B"])  # (stored against a few short blocks)
    for first, second in ("AB", "BA"):
        plan = make_plan()
        try:
            src = torch.zeros(plan.in_bytes, dtype=torch.uint8, device="cuda")
            dst = sr.canary_image(torch, plan.out_bytes, 0xFF)
            before = dst.cpu().numpy()
            for which in (first, second):
                src.copy_(torch.from_numpy(sr.place(items[which], plan.in_offsets, plan.in_bytes, "noise", 9)))
                torch.cuda.synchronize()
                plan.run(src.data_ptr(), dst.data_ptr())
                got_lens, stat = plan.results()
                host = dst.cpu().numpy()
                sr.assert_outside_untouched(host, plan.out_offsets, plan.out_caps, before)
                before = host
                for it, off, n, st, w in zip(items[which], plan.out_offsets, got_lens, stat, wants[which]):
                    g = (st, host[off:off + n].tobytes())
                    assert g == w, (f"{which} in the order {first}{second}", it.name, sr.brief(g), sr.brief(w))
        finally:
            plan.close()


@pytest.mark.parametrize("level,wbits", [(6, 15), (1, 31), (9, -15)])
def test_a_deflate_plan_run_on_another_batch(oracle, level, wbits):
    import torch
    import zsc_amd
    deflate_rerun(torch, oracle, DEFLATE_LENS, level, wbits, lambda: zsc_amd.DeflatePlan(list(DEFLATE_LENS), level, wbits))


def test_a_deflate_plan_of_two_sub_batches_run_on_another_batch(oracle, monkeypatch):
    """the scratch of a sub-batch is used again by the next one within a run, and by both in the next run"""
    import torch
    import zsc_amd
    lens = DEFLATE_LENS * 6
    assert 1 << 20 < sum(lens) < 2 << 20

    def make_plan():
        monkeypatch.setenv("ZSC_HIP_SUBBATCH_MB", "1")  # (read when the plan is created)
        try:
            plan = zsc_amd.DeflatePlan(list(lens), 6, 15)
        finally:
            monkeypatch.delenv("ZSC_HIP_SUBBATCH_MB")
        assert plan.sub_batches >= 2
        return plan

    deflate_rerun(torch, oracle, lens, 6, 15, make_plan)
