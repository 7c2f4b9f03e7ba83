#!/usr/bin/env python3
"""What the seek-point index of a deflate plan costs, and what reading with it saves.  Needs an MI355X:
there is no CPU path to fall back to.

    python tools/probe_deflate_index.py [--only ab] [--copies 4096] [--mib 128] [--runs 5] [--out FILE.json]

(a) the bench's headline shape (Canterbury-like x --copies, level 6): a plan without the index and a plan
    with it (default chunk_bytes), one after the other, each warmed up and then run --runs times with
    profiling on.  Reported: the whole pass (index 8 of zsc_hip_deflate_plan_times) of both, and
    zsc_hip_deflate_plan_index_ms of the second; the streams of both plans are compared on the device.
(b) one text-mix buffer of --mib MiB at level 6, index on: the same two figures.  (One buffer is parsed by
    one workgroup, at about 6 MB/s, and a plan's buffer is limited to 535 822 335 bytes: the default size
    keeps the probe to a few minutes.)  Then its stream is inflated by three routes, warmed up and run alternately
    --runs times each (the plan's kernel_ms, HIP events around the whole run), every output compared with
    the input on the device: a chunks plan; an indexed plan fed by that chunks plan's blob; an indexed
    plan fed by the deflate plan's blob.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import zsc_amd  # noqa: E402
from zsc_amd import corpus  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
from probe_inflate_sections import DEV, mix, upload  # noqa: E402


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 3), "spread_ms": round(max(ms) - min(ms), 3),
            "runs_ms": [round(m, 3) for m in ms]}


def deflate_runs(plan, d_in, d_out, runs, indexed):
    """warm-up, then `runs` profiled runs one at a time: (whole-pass ms per run, index ms per run, lens, stat)"""
    plan.run(d_in.data_ptr(), d_out.data_ptr())
    plan.results()
    total, index = [], []
    for _ in range(runs):
        plan.profile(True)  # (a new measurement window: the times of this run alone)
        plan.run(d_in.data_ptr(), d_out.data_ptr())
        lens, stat = plan.results()
        total.append(plan.kernel_times_ms()["total"])
        print(f"deflate run: {total[-1]:.1f} ms", flush=True)
        if indexed:
            index.append(plan.index_ms())
    return total, index, lens, stat


def part_a(res, copies, seeds, runs):
    sets = [corpus.canterbury_like(s) for s in range(seeds)]
    bufs = [b for st in sets for _, b in st]
    lens = [len(b) for b in bufs] * (copies // seeds)
    outs = {}
    for name, indexed in (("index_off", False), ("index_on", True)):
        plan = zsc_amd.DeflatePlan(lens, level=6)
        if indexed:
            plan.index_enable(0)
        per = plan.in_offsets[len(bufs)] if len(bufs) < len(lens) else plan.in_bytes - 64
        host = torch.zeros(per, dtype=torch.uint8)
        for off, b in zip(plan.in_offsets, bufs):
            host[off:off + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8)
        d_in = torch.zeros(plan.in_bytes, dtype=torch.uint8, device=DEV)
        d_in[:plan.in_bytes - 64] = host.to(DEV).repeat(copies // seeds)[:plan.in_bytes - 64]
        d_out = torch.zeros(plan.out_bytes, dtype=torch.uint8, device=DEV)
        total, index, slens, stat = deflate_runs(plan, d_in, d_out, runs, indexed)
        o = {"ok": all(s == 0 for s in stat), "whole_pass": summary(total), "sub_batches": plan.sub_batches,
             "scratch_bytes": plan.scratch_bytes}
        if indexed:
            o["index"] = summary(index)
            o["index_share_of_whole_pass"] = round(o["index"]["median_ms"] / o["whole_pass"]["median_ms"], 5)
            t0 = time.perf_counter()
            blobs = plan.export_indexes(d_in.data_ptr())
            o["export_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            o["blob_bytes"] = sum(len(b) for b in blobs)
            o["points"] = sum(zsc_amd.index_info(b)["points"] for b in blobs[:len(bufs)])
            o["ok"] = o["ok"] and all(b is not None for b in blobs) and slens == outs["index_off"][1]
            # the streams of the first set: those of the plan without the index
            n = plan.out_offsets[len(bufs)]
            o["ok"] = o["ok"] and bool((d_out[:n] == outs["index_off"][0]).all())
        else:
            outs[name] = (d_out[:plan.out_offsets[len(bufs)]].clone(), slens)
        o["input_bytes"] = sum(lens)
        res[f"a_canterbury_x{copies}_{name}"] = o
        print(name, o, flush=True)
        plan.close()
        del d_in, d_out


def inflate_routes(res, data, stream, deflate_blob, runs):
    n, m = len(data), len(stream)
    d_want = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(DEV)
    kp = zsc_amd.InflatePlan([m], [n], chunks=True, keep_index=True)
    d_src = upload(kp, [stream])
    d_dst = torch.zeros(kp.dst_bytes, dtype=torch.uint8, device=DEV)
    kp.run(d_src.data_ptr(), d_dst.data_ptr(), 0)
    lens, used, stat, _ = kp.results()
    ok = stat == [0] and lens == [n] and bool((d_dst[:n] == d_want).all())
    chunks_blob = kp.export_index(0)
    kp.close()
    ok = ok and chunks_blob is not None
    plans = {"chunks": zsc_amd.InflatePlan([m], [n], chunks=True),
             "indexed_chunks_blob": zsc_amd.InflatePlan([m], [n], indexes=[chunks_blob]),
             "indexed_deflate_blob": zsc_amd.InflatePlan([m], [n], indexes=[deflate_blob])}
    times = {k: [] for k in plans}
    pieces = {}
    for r in range(runs + 1):  # (the first round warms up)
        for k, plan in plans.items():
            check = r in (0, runs)
            if check:
                d_dst.zero_()
            plan.run(d_src.data_ptr(), d_dst.data_ptr(), 0)
            lens, used, stat, kms = plan.results()
            if r:
                times[k].append(kms)
            if check:
                ok = ok and stat == [0] and lens == [n] and used == [m] and bool((d_dst[:n] == d_want).all())
                pieces[k] = plan.sections()[0]
    for plan in plans.values():
        plan.close()
    out = {"ok": ok and all(p > 1 for p in pieces.values()), "output_bytes": n, "compressed_bytes": m, "pieces": pieces,
           "chunks_blob_bytes": len(chunks_blob), "deflate_blob_bytes": len(deflate_blob)}
    for k in plans:
        out[k] = summary(times[k])
        out[k]["GBps_out"] = round(n / out[k]["median_ms"] / 1e6, 3)
    res["b_inflate_three_routes"] = out
    print("inflate", out, flush=True)


def part_b(res, mib, runs, deflate_runs_n):
    data = mix(mib << 20, 900)
    print(f"one buffer of {len(data)} bytes made", flush=True)
    plan = zsc_amd.DeflatePlan([len(data)], level=6)
    plan.index_enable(0)
    d_in = torch.zeros(plan.in_bytes, dtype=torch.uint8, device=DEV)
    d_in[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(DEV)
    d_out = torch.zeros(plan.out_bytes, dtype=torch.uint8, device=DEV)
    total, index, lens, stat = deflate_runs(plan, d_in, d_out, deflate_runs_n, True)
    t0 = time.perf_counter()
    blob = plan.export_indexes(d_in.data_ptr())[0]
    export_ms = (time.perf_counter() - t0) * 1e3
    stream = bytes(d_out[:lens[0]].cpu().numpy())
    plan.close()
    del d_in, d_out
    o = {"ok": stat == [0] and blob is not None, "input_bytes": len(data), "compressed_bytes": lens[0],
         "whole_pass": summary(total), "index": summary(index), "export_wall_ms": round(export_ms, 1),
         "blob_bytes": len(blob), "points": zsc_amd.index_info(blob)["points"]}
    o["index_share_of_whole_pass"] = round(o["index"]["median_ms"] / o["whole_pass"]["median_ms"], 5)
    res[f"b_one_{mib}MiB_buffer_level6"] = o
    print("deflate", o, flush=True)
    inflate_routes(res, data, stream, blob, runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="ab")
    ap.add_argument("--copies", type=int, default=4096)
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--mib", type=int, default=128)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--deflate-runs", type=int, default=2, help="timed runs of the one long buffer's deflate plan")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("probe_deflate_index needs an MI355X: no GPU here")
    res = {"device": zsc_amd.device_info()}
    t0 = time.time()
    assert zsc_amd.compress_batch([b"warm" * 1000])[0] == 0
    if "a" in a.only:
        part_a(res, a.copies, max(1, min(a.seeds, a.copies)), a.runs)
    if "b" in a.only:
        part_b(res, a.mib, a.runs, a.deflate_runs)
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
