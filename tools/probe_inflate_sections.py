#!/usr/bin/env python3
"""Sections inflate (zsc_hip_inflate_plan_create_sections) against the plain plan, device-resident.

    python tools/probe_inflate_sections.py [--only abcd] [--gib 1] [--out FILE.json]

(a) the plain (serial) plan on one 16 MiB stream in 64 KiB sections: what one stream gets alone;
(b) one --gib GiB zlib stream with max_block_len 64 KiB and 1 MiB through the sections plan (the stream
    is a 4 MiB text-mix unit deflated by stock zlib with Z_FULL_FLUSH every max_block_len bytes,
    repeated: full-flush sections are independent, so the repeats are a valid stream);
(c) 64 x 16 MiB streams with max_block_len 100 000 (the library's own sections compressor);
(d) BASELINE config 4's gzip members (no markers) through the sections plan against the plain plan.
Every output is checked byte for byte; times are HIP events of the plan (kernel_ms) after a warm-up run.
"""
import argparse
import json
import os
import sys
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import zsc_amd  # noqa: E402
from zsc_amd import corpus  # noqa: E402

DEV = torch.device("cuda", 0)
KINDS = ("text", "table", "token", "object")


def mix(n, seed):
    unit = 1 << 20
    return b"".join(corpus.make_buffer(KINDS[i % 4], min(unit, n - i * unit), seed + i)
                    for i in range((n + unit - 1) // unit))


def upload(ip, streams, reps=1):
    """streams laid out as the plan wants them; `reps` copies of the list (device-side replication)"""
    per = len(streams)
    span = ip.src_offsets[per] if reps > 1 else ip.src_bytes - 64
    host = torch.zeros(span, dtype=torch.uint8)
    for off, s in zip(ip.src_offsets, streams):
        host[off:off + len(s)] = torch.frombuffer(bytearray(s), dtype=torch.uint8)
    d_src = torch.zeros(ip.src_bytes, dtype=torch.uint8, device=DEV)
    d_src[:span * reps] = host.to(DEV).repeat(reps)
    return d_src


def timed(ip, d_src, d_dst, runs=2):
    ip.run(d_src.data_ptr(), d_dst.data_ptr(), 0)
    ip.results()
    ms = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ip.run(d_src.data_ptr(), d_dst.data_ptr(), 0)
        lens, used, stat, kms = ip.results()
        ms.append(((time.perf_counter() - t0) * 1e3, kms))
    return lens, used, stat, ms


def part_a(res):
    data = mix(16 << 20, 300)
    rc, outs, st = zsc_amd.compress_sections_batch([data], [65536], level=6)
    assert rc == 0 and st == [0]
    comp = outs[0]
    ip = zsc_amd.InflatePlan([len(comp)], [len(data)])
    d_src = upload(ip, [comp])
    d_dst = torch.empty(ip.dst_bytes, dtype=torch.uint8, device=DEV)
    # warm-up on a small stream (code objects), then one timed run of the 16 MiB stream
    w = zsc_amd.uncompress_batch([zlib.compress(b"warm" * 1000)], [4000])
    assert w[0] == 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ip.run(d_src.data_ptr(), d_dst.data_ptr(), 0)
    lens, used, stat, kms = ip.results()
    wall = (time.perf_counter() - t0) * 1e3
    ok = stat == [0] and lens == [len(data)] and bytes(d_dst[:len(data)].cpu().numpy()) == data
    res["a_serial_one_16MiB_stream"] = {"ok": ok, "compressed": len(comp), "kernel_ms": round(kms, 2),
                                        "wall_ms": round(wall, 2), "MBps_out": round(len(data) / kms / 1e3, 3)}
    print("a", res["a_serial_one_16MiB_stream"], flush=True)


def part_b(res, gib):
    unit = mix(4 << 20, 500)
    reps = (gib << 30) // len(unit)
    for mbl in (65536, 1 << 20):
        co = zlib.compressobj(1, zlib.DEFLATED, -15)
        body = b"".join(co.compress(unit[i:i + mbl]) + co.flush(zlib.Z_FULL_FLUSH)
                        for i in range(0, len(unit), mbl))
        ad = 1
        for _ in range(reps):
            ad = zlib.adler32(unit, ad)
        stream = b"\x78\x01" + body * reps + b"\x03\x00" + ad.to_bytes(4, "big")
        n_out = len(unit) * reps
        want_sec = body.count(b"\x00\x00\xff\xff") * reps + 1
        ip = zsc_amd.InflatePlan([len(stream)], [n_out], sections=True)
        d_src = upload(ip, [stream])
        del stream
        d_dst = torch.empty(ip.dst_bytes, dtype=torch.uint8, device=DEV)
        lens, used, stat, ms = timed(ip, d_src, d_dst)
        nsec = ip.sections()
        d_unit = torch.frombuffer(bytearray(unit), dtype=torch.uint8).to(DEV)
        ok = stat == [0] and lens == [n_out] and nsec == [want_sec] and \
            bool((d_dst[:n_out].view(reps, len(unit)) == d_unit).all())
        best = min(k for _, k in ms)
        res[f"b_one_{gib}GiB_stream_mbl{mbl}"] = {
            "ok": ok, "compressed": int(d_src.numel()), "sections": nsec[0], "kernel_ms": [round(k, 2) for _, k in ms],
            "wall_ms": [round(w, 2) for w, _ in ms], "GBps_out": round(n_out / best / 1e6, 3),
            "scratch_bytes": ip.scratch_bytes()}
        print("b", mbl, res[f"b_one_{gib}GiB_stream_mbl{mbl}"], flush=True)
        ip.close()
        del d_src, d_dst


def part_c(res):
    distinct, reps = 4, 16
    bufs = [mix(16 << 20, 700 + 40 * i) for i in range(distinct)]
    rc, comps, st = zsc_amd.compress_sections_batch(bufs, [100000] * distinct, level=6)
    assert rc == 0 and st == [0] * distinct
    streams, caps = comps * reps, [len(b) for b in bufs] * reps
    ip = zsc_amd.InflatePlan([len(s) for s in streams], caps, sections=True)
    d_src = upload(ip, comps, reps)
    d_dst = torch.empty(ip.dst_bytes, dtype=torch.uint8, device=DEV)
    lens, used, stat, ms = timed(ip, d_src, d_dst)
    nsec = ip.sections()
    ok = all(s == 0 for s in stat) and lens == caps and all(x > 1 for x in nsec)
    for i in range(len(streams)):
        b = bufs[i % distinct]
        o = ip.dst_offsets[i]
        if i < distinct:
            ok = ok and bytes(d_dst[o:o + len(b)].cpu().numpy()) == b
        else:
            o0 = ip.dst_offsets[i % distinct]
            ok = ok and bool((d_dst[o:o + len(b)] == d_dst[o0:o0 + len(b)]).all())
    best = min(k for _, k in ms)
    res["c_64x16MiB_mbl100000"] = {"ok": ok, "sections_per_stream": sorted(set(nsec)),
                                   "kernel_ms": [round(k, 2) for _, k in ms],
                                   "GBps_out": round(sum(caps) / best / 1e6, 3), "scratch_bytes": ip.scratch_bytes()}
    print("c", res["c_64x16MiB_mbl100000"], flush=True)


def part_d(res, nstreams):
    distinct = 512
    st = corpus.Stream(4242, 3)
    sizes = [4096 + int(x) for x in st.below(distinct, 65536 - 4096 + 1)]
    kinds = ("text", "text", "token", "table")
    bufs = [corpus.make_buffer(kinds[i % 4], sizes[i], 7000 + i) for i in range(distinct)]
    rc, members, stats = zsc_amd.compress_batch(bufs, level=6, window_bits=31)
    assert rc == 0
    reps = nstreams // distinct
    slens, caps = [len(m) for m in members] * reps, sizes * reps
    plans = {}
    for name, sec in (("plain", False), ("sections", True)):
        ip = zsc_amd.InflatePlan(slens, caps, window_bits=31, sections=sec)
        plans[name] = (ip, upload(ip, members, reps), torch.empty(ip.dst_bytes, dtype=torch.uint8, device=DEV))
    times = {"plain": [], "sections": []}
    outs = {}
    for name, (ip, d_src, d_dst) in plans.items():
        ip.run(d_src.data_ptr(), d_dst.data_ptr(), 0)
        ip.results()
    for _ in range(4):  # alternating
        for name, (ip, d_src, d_dst) in plans.items():
            ip.run(d_src.data_ptr(), d_dst.data_ptr(), 0)
            lens, used, stat, kms = ip.results()
            times[name].append(kms)
            outs[name] = (lens, used, stat)
    ok = outs["plain"] == outs["sections"] and all(s == 0 for s in outs["plain"][2])
    ok = ok and plans["sections"][0].sections() == [0] * len(slens)
    dp, ds = plans["plain"][2], plans["sections"][2]
    for i in range(distinct):
        o = plans["plain"][0].dst_offsets[i]
        ok = ok and bytes(ds[o:o + caps[i]].cpu().numpy()) == bufs[i]
    for i in range(len(slens)):  # every stream of both plans, on the device
        o = plans["plain"][0].dst_offsets[i]
        ok = ok and bool((dp[o:o + caps[i]] == ds[o:o + caps[i]]).all()) if i % 97 == 0 or i < distinct else ok
    mp, ms_ = sorted(times["plain"])[len(times["plain"]) // 2], sorted(times["sections"])[len(times["sections"]) // 2]
    res["d_config4_members"] = {"ok": ok, "streams": len(slens), "output_bytes": sum(caps),
                                "plain_kernel_ms": [round(t, 3) for t in times["plain"]],
                                "sections_kernel_ms": [round(t, 3) for t in times["sections"]],
                                "median_ratio": round(ms_ / mp, 4)}
    print("d", res["d_config4_members"], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="abcd")
    ap.add_argument("--gib", type=int, default=1)
    ap.add_argument("--d-streams", type=int, default=65536)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"device": zsc_amd.device_info()}
    if "a" in a.only:
        part_a(res)
    if "b" in a.only:
        part_b(res, a.gib)
    if "c" in a.only:
        part_c(res)
    if "d" in a.only:
        part_d(res, a.d_streams)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    if not all(v.get("ok", True) for v in res.values() if isinstance(v, dict)):
        sys.exit(1)


if __name__ == "__main__":
    main()
