"""The sections inflate path on the MI355X: every item equal to the oracle and to the plain batch."""
import zlib

import pytest

from test_inflate_sections_emu import ANY, MARK, make_cases

gpu = pytest.mark.gpu


def _plan_run(zsc_amd, torch, streams, caps, wbits, sections, stream=0):
    ip = zsc_amd.InflatePlan([len(s) for s in streams], caps, window_bits=wbits, sections=sections)
    dev = torch.device("cuda", 0)
    host = torch.zeros(ip.src_bytes, dtype=torch.uint8)
    for off, s in zip(ip.src_offsets, streams):
        if s:
            host[off:off + len(s)] = torch.frombuffer(bytearray(s), dtype=torch.uint8)
    d_src = host.to(dev)
    d_dst = torch.full((ip.dst_bytes,), 0xEE, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    return ip, d_src, d_dst


@gpu
def test_gpu_sections_batch_equals_oracle_and_plain_batch(oracle):
    import zsc_amd
    cases = make_cases(oracle)
    for wbits in sorted({c[3] for c in cases}):
        group = [c for c in cases if c[3] == wbits]
        streams, caps = [c[1] for c in group], [c[2] for c in group]
        rc, outs, used, stat = zsc_amd.uncompress_sections_batch(streams, caps, window_bits=wbits)
        assert rc == 0
        prc, pouts, pused, pstat = zsc_amd.uncompress_batch(streams, caps, window_bits=wbits)
        assert prc == 0
        for i, (name, s, cap, _, _) in enumerate(group):
            want = oracle.uncompress(s, cap, window_bits=wbits)
            assert (stat[i], outs[i], used[i]) == want, name
            assert (stat[i], outs[i], used[i]) == (pstat[i], pouts[i], pused[i]), name


@gpu
def test_gpu_sections_plan_counts_and_repeat_runs(oracle):
    """every window_bits group of the mixed cases through a device plan, run twice (default and a
    non-default stream): identical results, the oracle's, and the expected section counts"""
    import torch
    import zsc_amd
    all_cases = make_cases(oracle)
    side = torch.cuda.Stream()
    parallel = 0
    for wbits in sorted({c[3] for c in all_cases}):
        cases = [c for c in all_cases if c[3] == wbits]
        streams, caps = [c[1] for c in cases], [c[2] for c in cases]
        ip, d_src, d_dst = _plan_run(zsc_amd, torch, streams, caps, wbits, True)
        runs = []
        for st in (0, side.cuda_stream):
            d_dst.fill_(0xEE)
            torch.cuda.synchronize()
            ip.run(d_src.data_ptr(), d_dst.data_ptr(), st)
            lens, used, stat, ms = ip.results()
            nsec = ip.sections()
            host = d_dst.cpu()
            outs = [bytes(host[o:o + n].numpy()) for o, n in zip(ip.dst_offsets, lens)]
            runs.append((lens, used, stat, nsec, outs))
            assert ms > 0
        assert runs[0] == runs[1], wbits
        lens, used, stat, nsec, outs = runs[0]
        for i, (name, s, cap, _, want_sec) in enumerate(cases):
            assert (stat[i], outs[i], used[i]) == oracle.uncompress(s, cap, window_bits=wbits), name
            if want_sec is not ANY:
                assert nsec[i] == want_sec, (name, nsec[i], want_sec)
            parallel += nsec[i] > 0
        assert ip.scratch_bytes() > 0
        ip.close()
    assert parallel >= sum(1 for c in all_cases if c[4])


@gpu
def test_gpu_sections_256mib_stream():
    """a ~256 MiB text-mix stream in 64 KiB sections; never decoded serially here (that would take
    minutes).  The library's own sections compressor makes one raw 16 MiB stream (a single call: one
    stream's re-parsed runs cost the latency of one workgroup each); its sections up
    to the last marker are independent, so they are repeated 16 times, then the last section, under a
    zlib header and trailer."""
    import torch
    import zsc_amd
    from zsc_amd import corpus
    kinds = ("text", "table", "token", "object")
    unit = b"".join(corpus.make_buffer(kinds[i % 4], 1 << 20, 900 + i) for i in range(16))
    rc, outs, stats = zsc_amd.compress_sections_batch([unit], [65536], level=6, window_bits=-15)
    assert rc == 0 and stats == [0]
    raw = outs[0]
    cut = raw.rfind(MARK) + 4
    assert cut > 4
    body, tail = raw[:cut], raw[cut:]
    head = zlib.decompressobj(-15).decompress(body)
    assert unit.startswith(head)
    # first the unit alone (its own sections plan): a stream that would go serial fails here, fast
    one = b"\x78\x01" + raw + zlib.adler32(unit).to_bytes(4, "big")
    ip1, d1, o1 = _plan_run(zsc_amd, torch, [one], [len(unit)], 15, True)
    ip1.run(d1.data_ptr(), o1.data_ptr(), 0)
    assert ip1.results()[2] == [0]
    assert ip1.sections() == [raw.count(MARK) + 1], "the unit did not decode in parallel"
    ip1.close()
    data = head * 16 + unit[len(head):]
    assert len(data) > 255 << 20
    comp = b"\x78\x01" + body * 16 + tail + zlib.adler32(data).to_bytes(4, "big")
    markers = comp.count(MARK)
    assert markers == 16 * body.count(MARK) and markers >= 2000
    ip, d_src, d_dst = _plan_run(zsc_amd, torch, [comp], [len(data)], 15, True)
    ip.run(d_src.data_ptr(), d_dst.data_ptr(), 0)
    lens, used, stat, ms = ip.results()
    assert (lens, used, stat) == ([len(data)], [len(comp)], [0])
    assert ip.sections() == [markers + 1]
    got = d_dst[:len(data)].cpu().numpy().tobytes()
    assert got == data
    ip.close()
