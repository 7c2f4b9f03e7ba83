"""The match search and the parsers on inputs built for their edges (tests/parser_cases.py), on a real MI355X,
through the C ABI of libzsc_hip.so.

One batch per parameter set holds all of that set's cases between ordinary corpus buffers.  Every stream must
be the oracle's and the compiled reference's (tests/golden/parser_edges_golden.json), the same wherever the case
sits in the batch (the batch runs again in reverse order), under every schedule the runtime can be put into when
a plan is created.  Families A, G and J also run as sections with a joint a few bytes before and behind the
planted edge.  tests/test_parser_edges_emu.py proves on the CPU that each case reaches the path it was built for.
"""
import os

import pytest

import parser_cases as P

pytestmark = pytest.mark.gpu

VERIFY_OK = 0
ENV = ("ZSC_HIP_SEG_PIPE", "ZSC_HIP_NO_SEG", "ZSC_HIP_FULL_RING", "ZSC_HIP_TABLE", "ZSC_HIP_TABLE_CAP",
       "ZSC_HIP_STAIR_MIN", "ZSC_HIP_LINK_KERNEL", "ZSC_HIP_FAST_RING")
# name: (environment read at plan creation, what DeflatePlan.seg_schedule must say for levels 4-9, levels)
SCHEDULES = {
    "default": ({}, "pipeline", range(1, 10)),
    "super-steps": ({"ZSC_HIP_SEG_PIPE": "0"}, "super-steps", range(4, 10)),
    "ring-classes": ({"ZSC_HIP_NO_SEG": "1"}, "none", range(4, 10)),
    "full-ring": ({"ZSC_HIP_FULL_RING": "1"}, "pipeline", range(4, 10)),
    "ring-classes-full-ring": ({"ZSC_HIP_NO_SEG": "1", "ZSC_HIP_FULL_RING": "1"}, "none", range(4, 10)),
    "table-cap8": ({"ZSC_HIP_TABLE": "1", "ZSC_HIP_TABLE_CAP": "8"}, "pipeline", range(4, 10)),
    "table-cap64": ({"ZSC_HIP_TABLE": "1", "ZSC_HIP_TABLE_CAP": "64"}, "pipeline", range(4, 10)),
    "stair-min-0": ({"ZSC_HIP_STAIR_MIN": "0"}, "pipeline", range(4, 10)),
    "stair-min-100000": ({"ZSC_HIP_STAIR_MIN": "100000"}, "pipeline", range(4, 10)),
    "link-kernel": ({"ZSC_HIP_LINK_KERNEL": "1"}, "pipeline", range(4, 10)),
    "fast-ring": ({"ZSC_HIP_FAST_RING": "1"}, None, range(1, 4)),
}


@pytest.fixture(scope="module")
def z():
    import zsc_amd
    assert zsc_amd.lib.zsc_hip_init(-1) == 0, "no usable gfx950 device: " + zsc_amd.device_info()
    return zsc_amd


@pytest.fixture(scope="module")
def groups():
    """{(level, window_bits, mem_level, strategy): cases}"""
    out = {}
    for c in P.cases():
        out.setdefault(c.params, []).append(c)
    assert len(out) <= 40
    # the ring classes of the wave-per-buffer parser (6, 10, 18 and 36 KiB) all get buffers of levels 4-9
    slow = [len(c.data) for c in P.cases() if P.levels()[c.level]["slow"] and c.strategy not in (P.RLE, P.HUFFMAN_ONLY)]
    assert any(n <= 6144 for n in slow) and any(6144 < n <= 10240 for n in slow)
    assert any(10240 < n <= 18432 for n in slow) and any(n > 18432 for n in slow)
    return out


_PAD = []


def padding():
    """ordinary buffers that go around and between the cases"""
    if not _PAD:
        from zsc_amd import corpus
        _PAD.extend([("pad-text", corpus.make_buffer("text", 3000, 41)), ("pad-table", corpus.make_buffer("table", 40000, 42)),
                     ("pad-zero", corpus.make_buffer("zero", 700, 43)), ("pad-object", corpus.make_buffer("object", 9000, 44))])
    return _PAD


def batch_of(cases):
    """[(name, data)]: a corpus buffer in front, one after every fourth case, and one at the end"""
    pad = padding()
    out = [pad[0]]
    for k, c in enumerate(cases):
        out.append((c.name, c.data))
        if k % 4 == 3:
            out.append(pad[(k // 4) % len(pad)])
    out.append(pad[1])
    return out


@pytest.fixture(scope="module")
def wanted(oracle, groups):
    """{(params, name): (rc, the oracle's stream)}, the padding included; the cases' streams are the golden ones"""
    golden = P.load_golden()["cases"]
    want = {}
    for params, cases in groups.items():
        level, wbits, ml, strat = params
        for name, data in [(c.name, c.data) for c in cases] + padding():
            rc, s, _ = oracle.compress(data, level, window_bits=wbits, mem_level=ml, strategy=strat, work_len=1 << 20)
            want[(params, name)] = (rc, s)
            if name in golden:
                assert [rc, len(s), P.sha(s)] == golden[name][:3], name
    assert set(golden) == {c.name for c in P.cases()}
    return want


class environment:
    """the schedule's variables set, and what was there before put back"""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.keep = {k: os.environ.get(k) for k in ENV}
        for k in ENV:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_streams_equal_oracle_and_golden_under_every_schedule(z, groups, wanted, schedule):
    env, says, levels = SCHEDULES[schedule]
    with environment(env):
        for params, cases in groups.items():
            level, wbits, ml, strat = params
            if level not in levels:
                continue
            batch = batch_of(cases)
            if says is not None and level >= 4:
                plan = z.DeflatePlan([len(d) for _, d in batch], level, wbits, ml, strat)
                try:
                    assert plan.seg_schedule == says, (schedule, params, plan.seg_schedule)
                finally:
                    plan.close()
            rc, outs, stats = z.compress_batch([d for _, d in batch], level=level, window_bits=wbits, mem_level=ml,
                                               strategy=strat)
            assert rc == 0 and len(outs) == len(batch), (schedule, params)
            for (name, data), out, st in zip(batch, outs, stats):
                assert (st, out) == wanted[(params, name)], (schedule, params, name, st, len(out))
            back = batch[::-1]
            rc, outs2, stats2 = z.compress_batch([d for _, d in back], level=level, window_bits=wbits, mem_level=ml,
                                                 strategy=strat)
            assert rc == 0 and outs2[::-1] == outs and stats2[::-1] == stats, (schedule, params)


SECTIONS_ALL_JOINTS = 13000


def section_items(cases):
    """(case, max_block_len) with a joint 1, 2, 3, 258 and 262 bytes before and behind the case's edge.  The
    cases of the 15-bit windows and the long ones of family G (33 to 196 KB each) get the joints 1 and 258
    bytes before and behind the edge only: the oracle states every expected stream, and ten joints for each of
    these would cost it more than all other cases together."""
    out = []
    for c in cases:
        if c.family in "AGJ" and c.edge is not None:
            for k in (1, 2, 3, 258, 262) if len(c.data) <= SECTIONS_ALL_JOINTS else (1, 258):
                for mbl in (c.edge - k, c.edge + k):
                    if 0 < mbl < len(c.data):
                        out.append((c, mbl))
    return out


@pytest.fixture(scope="module")
def section_streams(oracle, groups):
    """{params: [(case, max_block_len, the oracle's stream)]}, stated once for every schedule"""
    out = {}
    for params, cases in groups.items():
        level, wbits, ml, strat = params
        for c, mbl in section_items(cases):
            rc, s, uns = oracle.compress(c.data, level, window_bits=wbits, mem_level=ml, strategy=strat,
                                         max_block_len=mbl, work_len=1 << 20)
            assert rc == 0 and not uns, (c.name, mbl)
            out.setdefault(params, []).append((c, mbl, s))
    big = {c.name for items in out.values() for c, _, _ in items if len(c.data) > SECTIONS_ALL_JOINTS}
    assert {c.name for cs in groups.values() for c in cs if c.family in "AGJ" and len(c.data) > SECTIONS_ALL_JOINTS} == big
    return out


@pytest.mark.parametrize("schedule", ["default", "super-steps", "ring-classes"])
def test_sections_with_a_joint_next_to_the_edge(z, section_streams, schedule):
    """runs with joints go through the super-steps (or, told so, the wave-per-buffer parser with its hole map)
    and restart the window; the streams are the oracle's"""
    env, _, _ = SCHEDULES[schedule]
    seen = 0
    with environment(env):
        for params, items in section_streams.items():
            level, wbits, ml, strat = params
            rc, outs, stats = z.compress_sections_batch([c.data for c, _, _ in items], [m for _, m, _ in items],
                                                        level=level, window_bits=wbits, mem_level=ml, strategy=strat)
            assert rc == 0, (schedule, params, rc)
            for (c, mbl, w), out, st in zip(items, outs, stats):
                assert st == 0 and out == w, (schedule, params, c.name, mbl, st, len(out), len(w))
            seen += len(items)
    assert seen > 500


def test_streams_verify_and_inflate_back_on_the_device(z, groups, wanted):
    for params, cases in groups.items():
        level, wbits, ml, strat = params
        batch = batch_of(cases)
        datas = [d for _, d in batch]
        rc, streams, stats, verdicts = z.compress_batch_verified(datas, level=level, window_bits=wbits, mem_level=ml,
                                                                 strategy=strat)
        assert rc == 0 and stats == [0] * len(batch), params
        for (name, _), s, v in zip(batch, streams, verdicts):
            assert s == wanted[(params, name)][1], (params, name)
            assert v["verdict"] == VERIFY_OK, (params, name, v)
        rc, outs, used, stat = z.uncompress_batch(streams, [len(d) for d in datas], window_bits=wbits)
        assert rc == 0 and stat == [0] * len(batch), params
        assert used == [len(s) for s in streams], params
        for (name, data), out in zip(batch, outs):
            assert out == data, (params, name)
