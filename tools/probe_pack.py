#!/usr/bin/env python3
"""What packing a plan's results into one image costs, and what the host-image calls gain.  Needs an MI355X:
there is no CPU path to fall back to.

    python tools/probe_pack.py [--copies 4096] [--host-copies 64] [--runs 5] [--out FILE.json]

Device: the bench's headline shape (Canterbury-like x --copies, level 6) is compressed once by a plan with
packing enabled; then, alternating in one process, the pack (align 16 and align 1; its own HIP events) and the
yardstick, one device-to-device copy of `total` bytes by the runtime (torch's copy_ of a contiguous uint8
tensor: one hipMemcpyAsync, timed with events), each warmed up and run --runs times; medians.  The image is
compared with the plan's own streams on the device.

Host: Canterbury-like x --host-copies (64: 704 buffers, about 180 MB) through zsc_hip_compress_batch and
through zsc_hip_compress_batch_packed, and the streams back through zsc_hip_uncompress_batch and
zsc_hip_uncompress_batch_packed: wall time of the library call alone (arguments built beforehand), the two sides
alternating, medians of --runs; the results are compared.  For scale, the device time of the same plans' kernels.

Prints one JSON line (and writes it to --out).
"""
import argparse
import ctypes as C
import itertools
import json
import os
import statistics
import sys
import time


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 3), "spread_ms": round(max(ms) - min(ms), 3),
            "runs_ms": [round(m, 3) for m in ms]}


def device_part(zsc_amd, torch, copies, seeds, runs):
    from zsc_amd import corpus
    sets = [corpus.canterbury_like(s) for s in range(seeds)]
    bufs = [b for st in sets for _, b in st]
    reps = copies // seeds
    lens = [len(b) for b in bufs] * reps
    plan = zsc_amd.DeflatePlan(lens, level=6)
    plan.pack_enable(16)
    per = plan.in_offsets[len(bufs)] if len(bufs) < len(lens) else plan.in_bytes - 64
    host = torch.zeros(per, dtype=torch.uint8)
    for off, b in zip(plan.in_offsets, bufs):
        host[off:off + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8)
    d_in = torch.zeros(plan.in_bytes, dtype=torch.uint8, device="cuda")
    d_in[:plan.in_bytes - 64] = host.to("cuda").repeat(reps)[:plan.in_bytes - 64]
    d_out = torch.zeros(plan.out_bytes, dtype=torch.uint8, device="cuda")
    plan.profile(True)
    plan.run(d_in.data_ptr(), d_out.data_ptr())
    slens, stat = plan.results()
    o = {"ok": all(s == 0 for s in stat), "buffers": len(lens), "input_bytes": sum(lens), "stream_bytes": sum(slens),
         "sparse_image_bytes": plan.out_bytes, "deflate_whole_pass_ms": round(plan.kernel_times_ms()["total"], 3),
         "scratch_bytes": plan.scratch_bytes}
    del d_in
    cap = sum((n + 15) // 16 * 16 for n in slens)
    img = torch.empty(cap + 64, dtype=torch.uint8, device="cuda")
    other = torch.empty(cap + 64, dtype=torch.uint8, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def pack(align):
        plan.pack_enable(align)
        assert plan.pack(d_out.data_ptr(), img.data_ptr(), cap) == 0
        off, total = plan.pack_results()
        return plan.pack_ms(), off, total

    def copy(total):
        e0.record()
        other[:total].copy_(img[:total])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for align in (16, 1):
        _, off, total = pack(align)  # (warm)
        copy(total)
        # the image against the plan's own streams, on the device: the first period and the last buffer
        for i in list(range(len(bufs))) + [len(lens) - 1]:
            a, b = off[i], plan.out_offsets[i]
            o["ok"] = o["ok"] and bool((img[a:a + slens[i]] == d_out[b:b + slens[i]]).all())
        o["ok"] = o["ok"] and total == (cap if align == 16 else sum(slens))
        pms, cms = [], []
        for _ in range(runs):
            pms.append(pack(align)[0])
            cms.append(copy(total))
        key = f"align_{align}"
        o[key] = {"total_bytes": total, "pack": summary(pms), "device_to_device_copy": summary(cms)}
        o[key]["pack_over_copy"] = round(o[key]["pack"]["median_ms"] / o[key]["device_to_device_copy"]["median_ms"], 3)
        o[key]["pack_gb_per_s"] = round(total / o[key]["pack"]["median_ms"] / 1e6, 1)
    plan.close()
    return o


def host_part(zsc_amd, torch, copies, seeds, runs):
    from zsc_amd import corpus
    lib = zsc_amd.lib
    sets = [corpus.canterbury_like(s) for s in range(min(seeds, copies))]
    bufs = [b for st in sets for _, b in st] * (copies // min(seeds, copies))
    n = len(bufs)
    lens = [len(b) for b in bufs]
    caps = [zsc_amd.compress_get_max_output_size2(m, max(m, 1), 6)[1] for m in lens]
    u32, u64, i32 = C.c_uint32 * n, C.c_uint64 * n, C.c_int32 * n

    # the pointer batch: one host buffer per item each way
    srcs = (C.c_char_p * n)(*bufs)
    dbufs = [C.create_string_buffer(c) for c in caps]
    dsts = (C.c_void_p * n)(*[C.addressof(b) for b in dbufs])
    stat = i32()
    out = {}

    def old_deflate():
        dl = u32(*caps)
        t = time.perf_counter()
        rc = lib.zsc_hip_compress_batch(n, srcs, u32(*lens), dsts, dl, stat, 6, 15, 8, 0)
        dt = time.perf_counter() - t
        assert rc == 0
        if "old" not in out:
            out["old"] = [dbufs[i].raw[:dl[i]] for i in range(n)]
        return dt * 1e3

    # the image: one host buffer each way
    image = b"".join(bufs)
    soff = (C.c_uint64 * (n + 1))(*([0] + list(itertools.accumulate(lens))))
    dcap = sum(caps)
    dimg = C.create_string_buffer(dcap)
    doff = (C.c_uint64 * (n + 1))()
    pstat = i32()

    def new_deflate():
        t = time.perf_counter()
        rc = lib.zsc_hip_compress_batch_packed(n, image, soff, dimg, dcap, doff, pstat, 6, 15, 8, 0, 1)
        dt = time.perf_counter() - t
        assert rc == 0
        return dt * 1e3

    old_deflate(), new_deflate()  # (warm: the first call of each shape allocates)
    to, tn = [], []
    for _ in range(runs):
        to.append(old_deflate())
        tn.append(new_deflate())
    streams = out["old"]
    ok = list(pstat) == list(stat) == [0] * n and dimg.raw[:doff[n]] == b"".join(streams)
    nbytes, zbytes = sum(lens), doff[n]
    res = {"buffers": n, "input_bytes": nbytes, "stream_bytes": zbytes,
           "compress_batch": summary(to), "compress_batch_packed": summary(tn)}
    for k in ("compress_batch", "compress_batch_packed"):
        res[k]["mb_per_s_in"] = round(nbytes / res[k]["median_ms"] / 1e3, 1)
    res["compress_packed_speedup"] = round(res["compress_batch"]["median_ms"] / res["compress_batch_packed"]["median_ms"], 3)

    # and back
    zsrcs = (C.c_char_p * n)(*streams)
    zlens = [len(s) for s in streams]
    obufs = [C.create_string_buffer(max(m, 1)) for m in lens]
    odsts = (C.c_void_p * n)(*[C.addressof(b) for b in obufs])
    istat = i32()

    def old_inflate():
        sl, dl = u32(*zlens), u32(*lens)
        t = time.perf_counter()
        rc = lib.zsc_hip_uncompress_batch(n, zsrcs, sl, odsts, dl, istat, 15)
        dt = time.perf_counter() - t
        assert rc == 0 and list(dl) == lens
        return dt * 1e3

    zimage = dimg.raw[:zbytes]
    zoff = u64(*list(doff)[:n])
    oimg = C.create_string_buffer(nbytes)
    ooff = (C.c_uint64 * (n + 1))()
    odl, oused, pistat = u32(), u32(), i32()

    def new_inflate():
        t = time.perf_counter()
        rc = lib.zsc_hip_uncompress_batch_packed(n, zimage, zoff, u32(*zlens), u32(*lens), oimg, nbytes, ooff, odl, oused,
                                                 pistat, 15, 1)
        dt = time.perf_counter() - t
        assert rc == 0
        return dt * 1e3

    old_inflate(), new_inflate()
    to, tn = [], []
    for _ in range(runs):
        to.append(old_inflate())
        tn.append(new_inflate())
    ok = ok and list(pistat) == list(istat) == [0] * n and oimg.raw == image and list(oused) == zlens
    ok = ok and all(obufs[i].raw[:lens[i]] == bufs[i] for i in range(0, n, 37))
    res["uncompress_batch"], res["uncompress_batch_packed"] = summary(to), summary(tn)
    for k in ("uncompress_batch", "uncompress_batch_packed"):
        res[k]["mb_per_s_out"] = round(nbytes / res[k]["median_ms"] / 1e3, 1)
    res["uncompress_packed_speedup"] = round(res["uncompress_batch"]["median_ms"] / res["uncompress_batch_packed"]["median_ms"], 3)

    # for scale: the device time of the kernels alone, and one pageable copy each way of the whole image
    plan = zsc_amd.DeflatePlan(lens, level=6)
    d_in = torch.zeros(plan.in_bytes, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(plan.out_bytes, dtype=torch.uint8, device="cuda")
    plan.run(d_in.data_ptr(), d_out.data_ptr())
    plan.results()
    plan.profile(True)
    plan.run(d_in.data_ptr(), d_out.data_ptr())
    plan.results()
    res["deflate_kernels_ms_zero_input"] = round(plan.kernel_times_ms()["total"], 3)
    plan.close()
    himg = torch.frombuffer(bytearray(image), dtype=torch.uint8)
    t = time.perf_counter()
    dimg_t = himg.to("cuda")
    torch.cuda.synchronize()
    res["one_pageable_upload_ms"] = round((time.perf_counter() - t) * 1e3, 3)
    t = time.perf_counter()
    dimg_t.cpu()
    res["one_pageable_download_ms"] = round((time.perf_counter() - t) * 1e3, 3)
    res["ok"] = bool(ok)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=4096)
    ap.add_argument("--host-copies", type=int, default=64)
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import zsc_amd
    if not torch.cuda.is_available():
        sys.exit("probe_pack needs an MI355X: no GPU here")
    t0 = time.time()
    assert zsc_amd.compress_batch([b"warm" * 1000])[0] == 0
    res = {"device": zsc_amd.device_info(), "pack_tile": zsc_amd.PACK_TILE}
    if a.copies:
        res["device_pack"] = dict(device_part(zsc_amd, torch, a.copies, max(1, min(a.seeds, a.copies)), a.runs),
                                  shape=f"canterbury_like x{a.copies}, level 6")
        torch.cuda.empty_cache()
        zsc_amd.lib.zsc_hip_release_cached_memory()
    if a.host_copies:
        res["host_calls"] = dict(host_part(zsc_amd, torch, a.host_copies, a.seeds, a.runs),
                                 shape=f"canterbury_like x{a.host_copies}, level 6, zlib wrapper")
    res["probe_seconds"] = round(time.time() - t0, 1)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
    if not all(v.get("ok", True) for v in res.values() if isinstance(v, dict)):
        sys.exit(1)


if __name__ == "__main__":
    main()
