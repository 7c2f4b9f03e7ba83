#!/usr/bin/env python3
"""Inflate from a seek-point index (zsc_hip_inflate_plan_create_indexed) against the chunks plan that
exported it, device-resident.  Needs an MI355X: there is no CPU path to fall back to.

    python tools/probe_inflate_index.py [--only ab] [--gib 1] [--runs 5] [--parent-lib LIB.so] [--out FILE.json]

(a) one --gib GiB-output marker-free zlib stream (stock zlib level 1 of a text-mix),
    indexed at 128 KiB and at 32 KiB chunks;
(b) a batch of 64 streams of 16 MiB output each (the same data, cut up), at the default chunk_bytes.
Per workload, in one process: the chunks plan and the indexed plan are warmed up, then run alternately
--runs times each (HIP events around the whole run: the plan's kernel_ms); every output is compared byte
for byte on the device after the warm-up and after the last run.  Reported: medians and spreads (max -
min) of both, the blob's size as a share of the compressed stream, the time of the export (wall clock,
size + export of every stream), the time of a 1 MiB range out of the middle.
--parent-lib: a libzsc_hip.so built from the parent commit; its chunks plan is run alternately with this
build's (keep_index off) on workload (a) at 128 KiB, through the same C calls.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import zsc_amd  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
from probe_inflate_sections import DEV, mix, upload  # noqa: E402


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 3), "spread_ms": round(max(ms) - min(ms), 3),
            "runs_ms": [round(m, 3) for m in ms]}


def run_once(plan, d_src, d_dst):
    plan.run(d_src.data_ptr(), d_dst.data_ptr(), 0)
    lens, used, stat, kms = plan.results()
    return lens, used, stat, kms


def same(plan, d_dst, d_wants, lens):
    return all(bool((d_dst[o:o + n] == w).all()) for o, n, w in zip(plan.dst_offsets, lens, d_wants))


def workload(res, key, datas, streams, chunk_bytes, runs):
    caps = [len(d) for d in datas]
    slens = [len(s) for s in streams]
    d_wants = [torch.frombuffer(bytearray(d), dtype=torch.uint8).to(DEV) for d in datas]
    # the export: a chunks plan with keep_index
    kp = zsc_amd.InflatePlan(slens, caps, chunks=True, chunk_bytes=chunk_bytes, keep_index=True)
    d_src = upload(kp, streams)
    d_dst = torch.zeros(kp.dst_bytes, dtype=torch.uint8, device=DEV)
    lens, used, stat, _ = run_once(kp, d_src, d_dst)
    ok = stat == [0] * len(streams) and lens == caps and used == slens and same(kp, d_dst, d_wants, lens)
    pieces = kp.sections()
    t0 = time.perf_counter()
    blobs = [kp.export_index(i) for i in range(len(streams))]
    export_ms = (time.perf_counter() - t0) * 1e3
    kp.close()
    ok = ok and all(b is not None for b in blobs)
    cp = zsc_amd.InflatePlan(slens, caps, chunks=True, chunk_bytes=chunk_bytes)
    t0 = time.perf_counter()
    ip = zsc_amd.InflatePlan(slens, caps, indexes=blobs)
    create_ms = (time.perf_counter() - t0) * 1e3
    assert cp.src_offsets == ip.src_offsets and cp.dst_offsets == ip.dst_offsets
    times = {"chunks": [], "indexed": []}
    for name, plan in (("chunks", cp), ("indexed", ip)):  # warm-up, checked
        d_dst.zero_()
        lens, used, stat, _ = run_once(plan, d_src, d_dst)
        ok = ok and stat == [0] * len(streams) and lens == caps and used == slens and same(plan, d_dst, d_wants, lens)
    for r in range(runs):
        for name, plan in (("chunks", cp), ("indexed", ip)):
            last = r == runs - 1
            if last:
                d_dst.zero_()
            lens, used, stat, kms = run_once(plan, d_src, d_dst)
            times[name].append(kms)
            if last:
                ok = ok and stat == [0] * len(streams) and lens == caps and same(plan, d_dst, d_wants, lens)
    ipieces = ip.sections()
    ok = ok and ipieces == pieces
    out = {"ok": ok, "streams": len(streams), "chunk_bytes": chunk_bytes, "output_bytes": sum(caps),
           "compressed_bytes": sum(slens), "pieces": sum(pieces), "chunks": summary(times["chunks"]),
           "indexed": summary(times["indexed"]), "blob_bytes": sum(len(b) for b in blobs),
           "blob_share_of_compressed": round(sum(len(b) for b in blobs) / sum(slens), 4),
           "export_wall_ms": round(export_ms, 2), "indexed_create_wall_ms": round(create_ms, 2),
           "chunks_scratch_bytes": cp.scratch_bytes(), "indexed_scratch_bytes": ip.scratch_bytes()}
    c, i = out["chunks"], out["indexed"]
    out["indexed_GBps_out"] = round(sum(caps) / i["median_ms"] / 1e6, 3)
    out["chunks_GBps_out"] = round(sum(caps) / c["median_ms"] / 1e6, 3)
    out["ratio_chunks_over_indexed"] = round(c["median_ms"] / i["median_ms"], 2)
    out["condition_met"] = c["median_ms"] - i["median_ms"] > max(c["spread_ms"], i["spread_ms"])
    cp.close()
    ip.close()
    # a 1 MiB range out of the middle of the first stream
    begin = caps[0] // 2 + 12345
    n = min(1 << 20, caps[0] - begin)
    first, count, pbegin, plen = zsc_amd.index_range(blobs[0], begin, n)
    rp = zsc_amd.InflatePlan(slens[:1], [plen], indexes=blobs[:1], ranges=[(begin, n)])
    r_src = upload(rp, streams[:1])
    r_dst = torch.zeros(rp.dst_bytes, dtype=torch.uint8, device=DEV)
    run_once(rp, r_src, r_dst)
    rms = []
    for _ in range(runs):
        lens, used, stat, kms = run_once(rp, r_src, r_dst)
        rms.append(kms)
    rok = stat == [0] and lens == [plen] and bool((r_dst[:plen] == d_wants[0][pbegin:pbegin + plen]).all())
    out["range_1MiB"] = dict(summary(rms), ok=rok, pieces=count, piece_len=plen)
    out["ok"] = out["ok"] and rok
    rp.close()
    res[key] = out
    print(key, out, flush=True)
    return d_src, d_wants


class RawChunksPlan:
    """a chunks plan of any build of the library, through the C calls both builds have"""

    def __init__(self, L, slens, caps, like, chunk_bytes):
        n = len(slens)
        L.zsc_hip_inflate_plan_create_chunks.argtypes = zsc_amd.lib.zsc_hip_inflate_plan_create_chunks.argtypes
        L.zsc_hip_inflate_plan_run.argtypes = zsc_amd.lib.zsc_hip_inflate_plan_run.argtypes
        L.zsc_hip_inflate_plan_results.argtypes = zsc_amd.lib.zsc_hip_inflate_plan_results.argtypes
        L.zsc_hip_inflate_plan_destroy.argtypes = [C.c_void_p]
        L.zsc_hip_inflate_plan_destroy.restype = None
        self.L, self.n, self._h = L, n, C.c_void_p()
        rc = L.zsc_hip_inflate_plan_create_chunks(C.byref(self._h), n, (C.c_uint32 * n)(*slens),
                                                  (C.c_uint64 * n)(*like.src_offsets), (C.c_uint32 * n)(*caps),
                                                  (C.c_uint64 * n)(*like.dst_offsets), 15, chunk_bytes)
        assert rc == 0, rc

    def run(self, d_src, d_dst, stream):
        assert self.L.zsc_hip_inflate_plan_run(self._h, C.c_void_p(d_src), C.c_void_p(d_dst), C.c_void_p(stream)) == 0

    def results(self):
        n = self.n
        lens, used, stat, ms = (C.c_uint32 * n)(), (C.c_uint32 * n)(), (C.c_int32 * n)(), C.c_float()
        assert self.L.zsc_hip_inflate_plan_results(self._h, lens, used, stat, C.byref(ms)) == 0
        return list(lens), list(used), list(stat), ms.value

    def close(self):
        self.L.zsc_hip_inflate_plan_destroy(self._h)


def against_parent(res, parent_lib, data, stream, d_src, d_want, runs):
    P = C.CDLL(parent_lib)
    like = zsc_amd.InflatePlan([len(stream)], [len(data)], chunks=True, chunk_bytes=0)
    plans = {"parent": RawChunksPlan(P, [len(stream)], [len(data)], like, 0),
             "this": RawChunksPlan(zsc_amd.lib, [len(stream)], [len(data)], like, 0)}
    d_dst = torch.zeros(like.dst_bytes, dtype=torch.uint8, device=DEV)
    times = {k: [] for k in plans}
    ok = True
    for r in range(runs + 1):  # (the first round warms up)
        for k, plan in plans.items():
            if r == runs:
                d_dst.zero_()
            plan.run(d_src.data_ptr(), d_dst.data_ptr(), 0)
            lens, used, stat, kms = plan.results()
            if r:
                times[k].append(kms)
            if r == runs:
                ok = ok and stat == [0] and lens == [len(data)] and bool((d_dst[:len(data)] == d_want).all())
    for plan in plans.values():
        plan.close()
    like.close()
    out = {"ok": ok, "parent": summary(times["parent"]), "this_keep_index_off": summary(times["this"])}
    out["difference_ms"] = round(out["this_keep_index_off"]["median_ms"] - out["parent"]["median_ms"], 3)
    res["chunks_plan_against_parent_build"] = out
    print("parent", out, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="ab")
    ap.add_argument("--gib", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("probe_inflate_index needs an MI355X: no GPU here")
    assert a.runs >= 5, "at least five timed runs of each plan"
    res = {"device": zsc_amd.device_info()}
    t0 = time.time()
    w = zsc_amd.uncompress_batch([zlib.compress(b"warm" * 1000)], [4000])
    assert w[0] == 0
    data = mix(a.gib << 30, 900)
    if "a" in a.only:
        stream = zlib.compress(data, 1)
        assert stream.count(b"\x00\x00\xff\xff") < 1024
        d_src, d_wants = workload(res, f"a_one_{a.gib}GiB_stream_cb131072", [data], [stream], 131072, a.runs)
        if a.parent_lib:
            against_parent(res, a.parent_lib, data, stream, d_src, d_wants[0], a.runs)
        del d_src, d_wants
        workload(res, f"a_one_{a.gib}GiB_stream_cb32768", [data], [stream], 32768, a.runs)
    if "b" in a.only:
        unit = 16 << 20
        datas = [data[i * unit:(i + 1) * unit] for i in range(min(64, len(data) // unit))]
        streams = [zlib.compress(d, 1) for d in datas]
        workload(res, f"b_batch_{len(datas)}x16MiB", datas, streams, 0, a.runs)
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
