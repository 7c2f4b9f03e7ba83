"""The batched scatter of the tile sort (zsc_amd/csrc/hash_sort.h) on a real MI355X, through the whole
deflate path: level-6 streams equal the oracle's byte for byte at the sizes where a wave's batch of scatter
steps can go wrong (tests/test_hash_sort_emu.py has the same list): slices shorter than a batch, ragged last
batches, the tile's edges, a second tile; one bucket (zero), spread buckets (random) and text.  The buffers
below the segmented parser's 3 072-byte threshold take k_link_prev and the wave-per-buffer parser, the others
the segmented one, all in one batch."""
import pytest

pytestmark = pytest.mark.gpu

from zsc_amd import corpus  # noqa: E402

KINDS = ("zero", "random", "text")
SIZES = (3, 66, 1027, 2049, 16 * 64 * 3 + 5, 32767, 32768, 32769, 32770, 2 * 32768 + 7)


@pytest.fixture(scope="module")
def batch(oracle):
    bufs = [corpus.make_buffer(kind, n, 100 + n) for n in SIZES for kind in KINDS]
    want = []
    for b in bufs:
        rc, stream, _ = oracle.compress(b, 6)
        assert rc == 0
        want.append(stream)
    return bufs, want


def test_compress_batch_equals_the_oracle(batch):
    import zsc_amd
    assert zsc_amd.lib.zsc_hip_init(-1) == 0, "no usable gfx950 device: " + zsc_amd.device_info()
    bufs, want = batch
    assert min(len(b) for b in bufs) < 3072 < max(len(b) for b in bufs)
    rc, outs, stats = zsc_amd.compress_batch(bufs, level=6)
    assert rc == 0 and all(s == 0 for s in stats), (rc, stats)
    for i, (b, got, w) in enumerate(zip(bufs, outs, want)):
        assert got == w, (i, len(b), len(got), len(w))


def test_deflate_plan_equals_the_oracle(batch):
    import torch
    import zsc_amd
    assert zsc_amd.lib.zsc_hip_init(-1) == 0, "no usable gfx950 device: " + zsc_amd.device_info()
    bufs, want = batch
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
            for i, (o, n, w) in enumerate(zip(plan.out_offsets, lens, want)):
                assert bytes(out[o:o + n].numpy()) == w, (i, len(bufs[i]), n, len(w))
    finally:
        plan.close()
