"""Every kind of inflate plan with something other than zeros around its streams (tests/surroundings.py).

One batch per wrapper (zlib, gzip, raw) of a few dozen streams: clean ones of every length residue mod 4,
streams cut inside their header, inside a literal's code, between a length code and its distance, inside
stored data and inside the trailer -- source_len says where, and the bytes they were cut from lie directly
behind --, a full-flush stream cut right before a marker, a gzip file cut between two members and 1, 2 and 3
bytes into the next one's magic, a stream of more than three chunks cut in its last chunk right before a
dynamic block header, and capacities one byte and one half short.  The batch goes through all seven kinds of
plan, and a batch of gzip files through a members plan, under zeros (the control), 0xFF, noise and the true
continuation; the output is full of 0xEE.

Every (status, bytes[:out_len], consumed) must be what the oracle gives for exactly the stream's bytes, and
every byte outside the slots must keep its canary.  Size and check plans write nothing (d_dst is 0): status,
length and consumed, and the check plan's values.  tests/test_surroundings_cases.py checks the cases without
a GPU.
"""
import pytest

import surroundings as sr

pytestmark = pytest.mark.gpu

_blobs = {}


def blobs_of(torch, items, wbits):
    if wbits not in _blobs:
        _blobs[wbits] = sr.build_blobs(torch, items, wbits)
    return _blobs[wbits]


@pytest.mark.parametrize("wbits", sr.WRAPPERS)
@pytest.mark.parametrize("kind", sr.INFLATE_KINDS)
def test_results_depend_on_the_streams_own_bytes_only(oracle, kind, wbits):
    import torch
    items = sr.inflate_cases(oracle, wbits)
    wants = [sr.want_inflate(oracle, kind, it, wbits) for it in items]
    blobs = blobs_of(torch, items, wbits) if kind == "indexed" else None
    if blobs is not None:
        assert sum(b is not None for b in blobs) >= 2  # (the two clean streams of more than three chunks)
    sr.under_fillers([it.name for it in items], wants, lambda filler: sr.run_inflate(torch, kind, items, wbits, filler, blobs))


def test_members_depend_on_the_files_own_bytes_only(oracle):
    import torch
    items = sr.member_cases(oracle)
    wants = [sr.want_inflate(oracle, "members", it, sr.GZ) for it in items]
    sr.under_fillers([it.name for it in items], wants, lambda filler: sr.run_inflate(torch, "members", items, sr.GZ, filler))


def test_the_batch_in_the_plans_own_layout(oracle):
    """the same batch one stream behind the other as InflatePlan lays them out (64 to 79 spare bytes each),
    a plain and a chunks plan: the continuation then runs into the next stream's slot and is cut there"""
    import torch
    import zsc_amd
    for wbits in sr.WRAPPERS:
        items = sr.inflate_cases(oracle, wbits)
        lens, caps = [len(it.data) for it in items], [it.cap for it in items]
        wants = [sr.want_inflate(oracle, "plain", it, wbits) for it in items]
        for kw in ({}, {"chunks": True, "chunk_bytes": sr.CHUNK}):

            def run(filler):
                plan = zsc_amd.InflatePlan(lens, caps, window_bits=wbits, **kw)
                plan._surroundings_caps = caps
                try:
                    src = torch.from_numpy(sr.place(items, plan.src_offsets, plan.src_bytes, filler, seed=2)).cuda()
                    dst = sr.canary_image(torch, plan.dst_bytes)
                    plan.run(src.data_ptr(), dst.data_ptr())
                    host = dst.cpu().numpy()
                    res = sr.read_inflate(plan, "plain", host)
                    sr.assert_outside_untouched(host, plan.dst_offsets, caps)
                    return res
                finally:
                    plan.close()

            sr.under_fillers([it.name for it in items], wants, run)
