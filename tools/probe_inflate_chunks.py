#!/usr/bin/env python3
"""Chunks inflate (zsc_hip_inflate_plan_create_chunks) against the plain plan, device-resident.

    python tools/probe_inflate_chunks.py [--only abc] [--gib 1] [--out FILE.json]

(a) one --gib GiB-output marker-free zlib stream (stock zlib level 1 of a text-mix): the plain plan's
    rate on a 16 MiB stream of the same data (a whole GiB serially takes minutes), then the chunks plan
    at its default chunk_bytes and a chunk_bytes sweep;
(b) the same data with Z_SYNC_FLUSH every 64 KiB through the chunks plan, at the default chunk_bytes
    and at 64 KiB;
(c) BASELINE config 4's gzip members through the chunks plan against the plain plan (no member is
    longer than a chunk: this is what the path costs a batch it cannot help).
Every output is checked; times are HIP events of the plan (kernel_ms) after a warm-up run.
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

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
from probe_inflate_sections import DEV, mix, upload, timed, part_d  # noqa: E402


def one_stream(res, key, data, stream, chunk_bytes, d_want):
    ip = zsc_amd.InflatePlan([len(stream)], [len(data)], chunks=True, chunk_bytes=chunk_bytes)
    d_src = upload(ip, [stream])
    d_dst = torch.empty(ip.dst_bytes, dtype=torch.uint8, device=DEV)
    lens, used, stat, ms = timed(ip, d_src, d_dst)
    pieces = ip.sections()
    ok = stat == [0] and lens == [len(data)] and used == [len(stream)] and bool((d_dst[:len(data)] == d_want).all())
    best = min(k for _, k in ms)
    res[key] = {"ok": ok, "chunk_bytes": chunk_bytes, "compressed": len(stream), "pieces": pieces[0],
                "kernel_ms": [round(k, 2) for _, k in ms], "wall_ms": [round(w, 2) for w, _ in ms],
                "GBps_out": round(len(data) / best / 1e6, 3), "scratch_bytes": ip.scratch_bytes()}
    print(key, res[key], flush=True)
    ip.close()
    return best


def part_a(res, gib, sweep):
    data = mix(gib << 30, 900)
    d_want = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(DEV)
    small = data[:16 << 20]
    cs = zlib.compress(small, 1)
    ip = zsc_amd.InflatePlan([len(cs)], [len(small)])
    d_src = upload(ip, [cs])
    d_dst = torch.empty(ip.dst_bytes, dtype=torch.uint8, device=DEV)
    w = zsc_amd.uncompress_batch([zlib.compress(b"warm" * 1000)], [4000])
    assert w[0] == 0
    ip.run(d_src.data_ptr(), d_dst.data_ptr(), 0)
    lens, used, stat, kms = ip.results()
    ok = stat == [0] and bytes(d_dst[:len(small)].cpu().numpy()) == small
    plain_rate = len(small) / kms / 1e3
    res["a_plain_one_16MiB_stream"] = {"ok": ok, "compressed": len(cs), "kernel_ms": round(kms, 2),
                                       "MBps_out": round(plain_rate, 3)}
    print("a plain", res["a_plain_one_16MiB_stream"], flush=True)
    ip.close()
    stream = zlib.compress(data, 1)
    assert stream.count(b"\x00\x00\xff\xff") < 1024
    best = one_stream(res, f"a_chunks_one_{gib}GiB_stream_default", data, stream, 0, d_want)
    res["a_speedup_vs_plain"] = round(len(data) / best / 1e3 / plain_rate, 1)
    for cb in sweep:
        one_stream(res, f"a_chunks_one_{gib}GiB_stream_cb{cb}", data, stream, cb, d_want)
    return data, d_want


def part_b(res, gib, data, d_want):
    co = zlib.compressobj(1, zlib.DEFLATED, 15)
    stream = b"".join(co.compress(data[i:i + 65536]) + co.flush(zlib.Z_SYNC_FLUSH)
                      for i in range(0, len(data), 65536)) + co.flush()
    one_stream(res, f"b_chunks_one_{gib}GiB_stream_sync64k", data, stream, 0, d_want)
    one_stream(res, f"b_chunks_one_{gib}GiB_stream_sync64k_cb65536", data, stream, 65536, d_want)


def part_c(res, nstreams):
    # part_d of the sections probe, with the chunks plan in place of the sections plan
    real = zsc_amd.InflatePlan

    def chunks_plan(*a, sections=False, **k):
        return real(*a, chunks=sections, **k)
    zsc_amd.InflatePlan = chunks_plan
    try:
        part_d(res, nstreams)
    finally:
        zsc_amd.InflatePlan = real
    res["c_config4_members_chunks"] = res.pop("d_config4_members")
    r = res["c_config4_members_chunks"]
    r["chunks_kernel_ms"] = r.pop("sections_kernel_ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="abc")
    ap.add_argument("--gib", type=int, default=1)
    ap.add_argument("--sweep", default="32768,65536,131072,262144,1048576")
    ap.add_argument("--c-streams", type=int, default=65536)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"device": zsc_amd.device_info()}
    t0 = time.time()
    data = d_want = None
    if "a" in a.only or "b" in a.only:
        data, d_want = part_a(res, a.gib, [int(x) for x in a.sweep.split(",") if x] if "a" in a.only else [])
    if "b" in a.only:
        part_b(res, a.gib, data, d_want)
    if "c" in a.only:
        part_c(res, a.c_streams)
    res["probe_seconds"] = round(time.time() - t0, 1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    if not all(v.get("ok", True) for v in res.values() if isinstance(v, dict)):
        sys.exit(1)


if __name__ == "__main__":
    main()
