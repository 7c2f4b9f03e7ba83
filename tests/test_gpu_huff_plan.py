"""The block planner (zsc_amd/csrc/huff_plan.h) on the inputs of tests/huff_plan_cases.py, on a real MI355X,
through the C ABI of libzsc_hip.so.

One batch per parameter set holds that set's cases between two corpus buffers.  Every stream must be the
oracle's, and the same when the batch runs in reverse order (other blocks around it, other waves' leftovers in
LDS).  tests/test_huff_plan_emu.py proves on the CPU that each case reaches the path it was built for.
"""
import pytest

import huff_plan_cases as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def z():
    import zsc_amd
    assert zsc_amd.lib.zsc_hip_init(-1) == 0, "no usable gfx950 device: " + zsc_amd.device_info()
    return zsc_amd


def test_streams_equal_the_oracle_wherever_they_sit(z, oracle):
    from zsc_amd import corpus
    pad = [("pad-text", corpus.make_buffer("text", 3000, 41)), ("pad-table", corpus.make_buffer("table", 40000, 42))]
    groups = H.groups()
    assert 4 <= len(groups) <= 8
    for params, cases in groups.items():
        level, wbits, ml, strat = params
        batch = [pad[0]] + [(c.name, c.data) for c in cases] + [pad[1]]
        want = [oracle.compress(d, level, window_bits=wbits, mem_level=ml, strategy=strat, work_len=1 << 20)[:2]
                for _, d in batch]
        rc, outs, stats = z.compress_batch([d for _, d in batch], level=level, window_bits=wbits, mem_level=ml,
                                           strategy=strat)
        assert rc == 0 and len(outs) == len(batch), params
        for (name, _), out, st, w in zip(batch, outs, stats, want):
            assert (st, out) == w, (params, name, st, len(out))
        rc, outs2, stats2 = z.compress_batch([d for _, d in batch[::-1]], level=level, window_bits=wbits,
                                             mem_level=ml, strategy=strat)
        assert rc == 0 and outs2[::-1] == outs and stats2[::-1] == stats, params
