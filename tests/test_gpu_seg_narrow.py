"""The pipeline schedule of the segmented parser in its own LDS geometry (k_parse_seg_narrow, SgLdsNarrow) on a
real MI355X, against the wide geometry and the super-steps.

ZSC_HIP_SEG_RING=narrow|wide is read when a plan is created, like ZSC_HIP_SEG_PIPE; DeflatePlan.seg_ring says
what the plan chose.  The inputs are those of tests/test_seg_narrow_emu.py (sizes around the window, the narrow
ring and its chunk; kinds that force redo rounds and a hand-over at every segment; the parser cases at MAX_DIST,
at slides and at segment hand-overs), as one batch.  Every stream is the oracle's and the same under the three
configurations.  With nothing said a sub-batch takes the narrow ring when it offers a CU more workgroups than
the wide one lets it hold; plans the narrow entry is not built for -- runs with joints, window_bits below 15 -- stay
wide whatever the environment says.
"""
import os

import pytest

import parser_cases as P

pytestmark = pytest.mark.gpu

from zsc_amd import corpus  # noqa: E402

KINDS = ("text", "bitmap", "zero", "runs", "table", "random")
WINDOW, R, CHUNK = 32768, 37888, 512     # (SgLdsNarrow; tests/test_seg_narrow_emu.py asserts the geometry itself)
SIZES = (3073, WINDOW - 1, WINDOW + 1, R - 1, R, R + 1, R + CHUNK - 1, R + CHUNK + 1, WINDOW + R - 1, WINDOW + R + 1,
         2 * R - 1, 2 * R + 1, 3 * R + 257, 200001)
ENV = ("ZSC_HIP_SEG_RING", "ZSC_HIP_SEG_PIPE")
# name: (environment at plan creation, seg_schedule, seg_ring)
CONFIGS = {
    "narrow": ({"ZSC_HIP_SEG_RING": "narrow"}, "pipeline", "narrow"),
    "wide": ({"ZSC_HIP_SEG_RING": "wide"}, "pipeline", "wide"),
    "super-steps": ({"ZSC_HIP_SEG_RING": "narrow", "ZSC_HIP_SEG_PIPE": "0"}, "super-steps", "wide"),
}


class environment:
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


@pytest.fixture(scope="module")
def z():
    import zsc_amd
    assert zsc_amd.lib.zsc_hip_init(-1) == 0, "no usable gfx950 device: " + zsc_amd.device_info()
    return zsc_amd


@pytest.fixture(scope="module")
def bufs():
    out = [corpus.make_buffer(kind, n, n + 17) for n in SIZES for kind in KINDS]
    edges = [c for c in P.cases() if c.segmented and abs(c.window_bits) == 15 and c.mem_level == 8
             and c.strategy == P.DEFAULT and c.family in "AGF" and 4 <= c.level <= 9]
    assert len(edges) >= 30
    return out + [c.data for c in edges]


def run_plan(z, bufs, level, schedule, ring, window_bits=15):
    """one batch through a DeflatePlan, which must say `schedule` and `ring`; the streams"""
    import torch
    plan = z.DeflatePlan([len(b) for b in bufs], level=level, window_bits=window_bits)
    try:
        assert (plan.seg_schedule, plan.seg_ring) == (schedule, ring)
        host = torch.zeros(plan.in_bytes, dtype=torch.uint8)
        for off, b in zip(plan.in_offsets, bufs):
            host[off:off + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8)
        d_in = host.to("cuda")
        d_out = torch.zeros(plan.out_bytes, dtype=torch.uint8, device="cuda")
        plan.run(d_in.data_ptr(), d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        lens, stats = plan.results()
        assert all(s == 0 for s in stats), [(i, s, len(bufs[i])) for i, s in enumerate(stats) if s]
        out = d_out.cpu()
        return [bytes(out[o:o + n].numpy()) for o, n in zip(plan.out_offsets, lens)]
    finally:
        plan.close()


@pytest.mark.parametrize("level", (6, 4, 9))
def test_narrow_wide_and_super_steps_give_the_oracle_streams(z, oracle, bufs, level):
    want = [oracle.compress(b, level)[1] for b in bufs]
    got = {}
    for name, (env, schedule, ring) in CONFIGS.items():
        with environment(env):
            got[name] = run_plan(z, bufs, level, schedule, ring)
    for i, b in enumerate(bufs):
        for name in CONFIGS:
            assert got[name][i] == want[i], (name, level, i, len(b))
        assert got["narrow"][i] == got["wide"][i] == got["super-steps"][i], (level, i, len(b))


def test_the_default_goes_by_the_workgroups_a_cu_is_offered(z):
    """nothing said: the narrow ring where a sub-batch has more long buffers than three per CU (the fourth
    workgroup is what it pays through), the wide ring below that"""
    import re
    cus = int(re.search(r"(\d+) CUs", z.device_info()).group(1))
    with environment({}):
        for count, ring in ((2, "wide"), (3 * cus, "wide"), (3 * cus + 1, "narrow")):
            plan = z.DeflatePlan([3073] * count, level=6)
            try:
                assert (plan.seg_schedule, plan.seg_ring) == ("pipeline", ring), count
            finally:
                plan.close()
        plan = z.DeflatePlan([70000, 5000], level=2)     # (levels 1-3: no segmented parser)
        try:
            assert plan.seg_ring == "none"
        finally:
            plan.close()
    with environment({"ZSC_HIP_SEG_RING": "neither"}):   # (an unknown word changes nothing)
        plan = z.DeflatePlan([70000], level=9)
        try:
            assert plan.seg_ring == "wide"
        finally:
            plan.close()
    with environment({"ZSC_HIP_SEG_RING": "wide"}):
        plan = z.DeflatePlan([3073] * (3 * cus + 1), level=6)
        try:
            assert plan.seg_ring == "wide"
        finally:
            plan.close()


def test_window_bits_below_15_stay_wide(z, oracle, bufs):
    some = [b for b in bufs if 3072 < len(b) <= R + 1][:24]
    with environment({"ZSC_HIP_SEG_RING": "narrow"}):
        got = run_plan(z, some, 6, "pipeline", "wide", window_bits=12)
    for i, b in enumerate(some):
        assert got[i] == oracle.compress(b, 6, window_bits=12)[1], (i, len(b))


def test_runs_with_joints_stay_wide(z, oracle, bufs):
    """a batch of sections: its plans carry joints and take the super-steps' kernel in the wide geometry
    (compress_sections_last_rings counts the sub-batches of the call's rounds by geometry)"""
    some = [b for b in bufs if len(b) >= WINDOW - 1][:18]
    mbl = [9000 + 501 * i for i in range(len(some))]
    with environment({"ZSC_HIP_SEG_RING": "narrow"}):
        rc, outs, stats = z.compress_sections_batch(some, mbl, level=6)
        wide, narrow = z.compress_sections_last_rings()
    assert rc == 0 and stats == [0] * len(some)
    assert wide >= 1 and narrow == 0
    for i, (b, m) in enumerate(zip(some, mbl)):
        orc, s, uns = oracle.compress(b, 6, max_block_len=m, work_len=1 << 20)
        assert orc == 0 and outs[i] == s, (i, len(b), m)
