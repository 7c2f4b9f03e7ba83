"""Lazy searches that cannot win (zsc_amd/csrc/lz_parse_seg.h: SG_LAZY_FILTER, SG_EMPTY_SKIP) on a real MI355X:
the buffers of tests/test_lazy_search_emu.py through the whole deflate path, one batch per configuration --
levels 4-9 with their own good_length / max_lazy / nice_match, the default strategy and Z_FILTERED (the generic
instantiation and its cur_len <= 5 rule), and window_bits 12 / mem_level 5 (the instantiation without the
lane-parallel search, where only the empty-chain test acts) -- and once more through a DeflatePlan run twice.
Every stream equals the oracle's byte for byte."""
import pytest

pytestmark = pytest.mark.gpu

from zsc_amd import corpus  # noqa: E402
from test_lazy_search_emu import KINDS, SIZES, LEVELS, Z_FILTERED, tail_buffer, cache_end_buffer  # noqa: E402

CONFIGS = [dict(level=lv, strategy=st) for lv in LEVELS for st in (0, Z_FILTERED)] + \
          [dict(level=6, window_bits=12, mem_level=5)]


@pytest.fixture(scope="module")
def bufs():
    return [corpus.make_buffer(kind, n, n + 5) for kind in KINDS for n in SIZES] + [tail_buffer(), cache_end_buffer()]


@pytest.fixture(scope="module")
def want(oracle, bufs):
    """the oracle's streams, per configuration (worked out once)"""
    out = {}
    for i, cfg in enumerate(CONFIGS):
        out[i] = []
        for b in bufs:
            rc, stream, _ = oracle.compress(b, **cfg)
            assert rc == 0
            out[i].append(stream)
    return out


@pytest.mark.parametrize("ci", range(len(CONFIGS)), ids=["-".join(f"{k}{v}" for k, v in c.items()) for c in CONFIGS])
def test_compress_batch_equals_the_oracle(bufs, want, ci):
    import zsc_amd
    assert zsc_amd.lib.zsc_hip_init(-1) == 0, "no usable gfx950 device: " + zsc_amd.device_info()
    assert min(len(b) for b in bufs) > 3072  # all of them go to the segmented parser
    rc, outs, stats = zsc_amd.compress_batch(bufs, **CONFIGS[ci])
    assert rc == 0 and all(s == 0 for s in stats), (rc, stats)
    for i, (b, got, w) in enumerate(zip(bufs, outs, want[ci])):
        assert got == w, (CONFIGS[ci], i, len(b), len(got), len(w))


def test_deflate_plan_equals_the_oracle(bufs, want):
    import torch
    import zsc_amd
    assert zsc_amd.lib.zsc_hip_init(-1) == 0, "no usable gfx950 device: " + zsc_amd.device_info()
    ci = CONFIGS.index(dict(level=6, strategy=0))
    plan = zsc_amd.DeflatePlan([len(b) for b in bufs], level=6)
    try:
        host = torch.zeros(plan.in_bytes, dtype=torch.uint8)
        for off, b in zip(plan.in_offsets, bufs):
            host[off:off + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8)
        d_in = host.to("cuda")
        d_out = torch.zeros(plan.out_bytes, dtype=torch.uint8, device="cuda")
        for _ in range(2):  # a plan is run again and again: the second run over the first one's scratch
            plan.run(d_in.data_ptr(), d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            lens, stats = plan.results()
            assert all(s == 0 for s in stats), [(i, s) for i, s in enumerate(stats) if s]
            out = d_out.cpu()
            for i, (o, n, w) in enumerate(zip(plan.out_offsets, lens, want[ci])):
                assert bytes(out[o:o + n].numpy()) == w, (i, len(bufs[i]), n, len(w))
    finally:
        plan.close()
