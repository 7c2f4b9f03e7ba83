"""The resync inflate path on the MI355X: the recorded reference cases, a mixed batch equal to a plain
plan's (data error counts included), repeat runs, and a 256 MiB damaged stream."""
import hashlib
import zlib

import pytest

from test_inflate_resync_emu import MARK, constructed_cases, damage_sections, damaged_sweep, golden_cases, serial_cases

gpu = pytest.mark.gpu


def _upload(zsc_amd, torch, streams, caps, wbits, **kind):
    ip = zsc_amd.InflatePlan([len(s) for s in streams], caps, window_bits=wbits, **kind)
    dev = torch.device("cuda", 0)
    host = torch.zeros(ip.src_bytes, dtype=torch.uint8)
    for off, s in zip(ip.src_offsets, streams):
        if s:
            host[off:off + len(s)] = torch.frombuffer(bytearray(s), dtype=torch.uint8)
    d_src = host.to(dev)
    d_dst = torch.full((ip.dst_bytes,), 0xEE, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    return ip, d_src, d_dst


def _run(torch, ip, d_src, d_dst, stream=0):
    d_dst.fill_(0xEE)
    torch.cuda.synchronize()
    ip.run(d_src.data_ptr(), d_dst.data_ptr(), stream)
    lens, used, stat, ms = ip.results()
    host = d_dst.cpu()
    outs = [bytes(host[o:o + n].numpy()) for o, n in zip(ip.dst_offsets, lens)]
    return stat, outs, used, ip.data_errors(), ip.sections()


@gpu
def test_gpu_resync_batch_recorded_reference_cases():
    import zsc_amd
    cases = golden_cases()
    for wbits in sorted({c[3] for c in cases}):
        group = [c for c in cases if c[3] == wbits]
        rc, outs, used, stat = zsc_amd.uncompress_resync_batch([c[1] for c in group], [c[2] for c in group],
                                                               window_bits=wbits)
        assert rc == 0
        for (name, _, _, _, want), o, u, st in zip(group, outs, used, stat):
            assert (st, len(o), u, hashlib.sha256(o).hexdigest()) == want, name


@gpu
def test_gpu_resync_plan_mixed_batch_equals_plain_plan(oracle):
    """clean, damaged, marker-free, Z_SYNC_FLUSH, truncated and short-cap streams: everything a plain
    plan reports, data error counts included; the constructed cases with their exact expectations;
    two runs of one plan (default and a non-default stream) agree"""
    import torch
    import zsc_amd
    from zsc_amd import corpus
    cons = constructed_cases()
    mixed = [(n, s, c, w) for n, s, c, w, _ in cons] + serial_cases() + damaged_sweep(oracle, 12, 240)
    text = corpus.make_buffer("text", 50000, 31)
    for wbits in (15, 31, -15):
        rc, plain, _ = oracle.compress(text, 6, window_bits=wbits)  # one section, no marker
        mixed.append((f"marker-free-w{wbits}", plain, len(text), wbits))
    expect = {n: w for n, _, _, _, w in cons}
    side = torch.cuda.Stream()
    parallel_damaged = 0
    for wbits in (15, 31, -15):
        group = [c for c in mixed if c[3] == wbits]
        streams, caps = [c[1] for c in group], [c[2] for c in group]
        ip, d_src, d_dst = _upload(zsc_amd, torch, streams, caps, wbits, resync=True)
        runs = [_run(torch, ip, d_src, d_dst, st) for st in (0, side.cuda_stream)]
        assert runs[0] == runs[1], wbits
        assert ip.scratch_bytes() > 0
        ip.close()
        pp, p_src, p_dst = _upload(zsc_amd, torch, streams, caps, wbits)
        pstat, pouts, pused, perr, psec = _run(torch, pp, p_src, p_dst)
        pp.close()
        assert psec == [0] * len(group)
        stat, outs, used, errs, nsec = runs[0]
        for i, (name, s, cap, _) in enumerate(group):
            assert (stat[i], outs[i], used[i], errs[i]) == (pstat[i], pouts[i], pused[i], perr[i]), name
            if name in expect:
                st, out, consumed, e, sec = expect[name]
                assert (stat[i], outs[i], used[i], errs[i], nsec[i]) == (st, out, consumed, e, sec), name
            parallel_damaged += stat[i] == -3 and nsec[i] > 0
    assert parallel_damaged >= sum(1 for c in cons if c[4][0] == -3)


def _marker_ends(b):
    """offsets just behind every 00 00 FF FF of b"""
    out, at = [], b.find(MARK)
    while at >= 0:
        out.append(at + 4)
        at = b.find(MARK, at + 1)
    return out


@gpu
def test_gpu_resync_256mib_stream_one_percent_damaged():
    """~256 MiB of output in 64 KiB full-flush sections, about 1 % of them damaged; the expected results
    come from the construction (damage_sections), so the stream is never decoded serially here.  A raw
    4 MiB unit of 64 sections, each ending in a marker, is repeated 64 times (each section stands
    alone), then an empty final block, under a zlib header and trailer."""
    import torch
    import zsc_amd
    from zsc_amd import corpus
    kinds = ("text", "table", "token", "object")
    unit = b"".join(corpus.make_buffer(kinds[i % 4], 1 << 20, 900 + i) for i in range(4))
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    pieces = [unit[i:i + 65536] for i in range(0, len(unit), 65536)]
    body = b"".join(co.compress(p) + co.flush(zlib.Z_FULL_FLUSH) for p in pieces)
    tail = co.flush()
    unit_starts = [0] + _marker_ends(body)[:-1]
    assert len(unit_starts) == len(pieces)

    def build(reps, damaged):
        data = unit * reps
        stream = b"\x78\x01" + body * reps + tail + zlib.adler32(data).to_bytes(4, "big")
        starts = [2 + r * len(body) + st for r in range(reps) for st in unit_starts] + [2 + reps * len(body)]
        return len(data), damage_sections(stream, pieces * reps + [b""], starts, damaged, 15)

    # the unit alone first, one section damaged: a stream that would go serial fails here, fast
    cap, (s, want) = build(1, [5])
    ip, d_src, d_dst = _upload(zsc_amd, torch, [s], [cap], 15, resync=True)
    got = _run(torch, ip, d_src, d_dst)
    ip.close()
    assert got[4] == [want[4]], "the unit did not decode in parallel"
    assert (got[0][0], got[1][0], got[2][0], got[3][0]) == want[:4]
    reps = 64
    nsec = reps * len(pieces) + 1
    damaged = list(range(7, nsec - 1, 97))  # ~1 %
    cap, (s, want) = build(reps, damaged)
    assert cap >= 256 << 20 and want[3] == len(damaged) + 1 and want[4] == nsec
    ip, d_src, d_dst = _upload(zsc_amd, torch, [s], [cap], 15, resync=True)
    stat, outs, used, errs, secs = _run(torch, ip, d_src, d_dst)
    ip.close()
    assert (stat[0], used[0], errs[0], secs[0]) == (want[0], want[2], want[3], want[4])
    assert len(outs[0]) == len(want[1]) and outs[0] == want[1]
