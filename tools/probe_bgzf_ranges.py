#!/usr/bin/env python3
"""The BGZF index and the ranges plan (zsc_hip_bgzf_index_build, zsc_hip_inflate_plan_create_bgzf_ranges) against
the members plan and the plain plan, device-resident.

    python tools/probe_bgzf_ranges.py [--tree DIR] [--members 4096] [--ranges 65536] [--out FILE.json]
    python tools/probe_bgzf_ranges.py --merge --parent P1.json P2.json ... --new N1.json N2.json ... --out FILE.json
                                         [--bench PARENT.log NEW.log]

The file is the members probe's: --members BGZF members of 64 KiB of corpus data at level 6 (512 distinct ones,
repeated).  One process measures one build; --tree DIR imports zsc_amd from another checkout -- a build of the
parent commit, which has neither index nor ranges plan: only the yardsticks are timed there -- so that processes of
the two builds can alternate.  Every figure is the median of three runs after a warm-up, by the calls' own HIP
events (kernel_ms of a plan's _results, build_ms of the index).
  yardsticks (both builds):
    size_only   a members plan in size-only mode over the file
    members     a members plan inflating the whole file once
    plain       a plain plan given --ranges whole members as separate streams (every member --ranges / --members
                times, each from where it lies by itself, 16-byte aligned)
  this build:
    index       the index of the file
    random      --ranges ranges of 100 B .. 256 KiB at random places (seeded): kernel_ms, bytes delivered, bytes
                decoded (the plan's jobs), a sample of 512 outputs compared on the device with the content
    whole       --ranges ranges of one whole member each -- no edge job, no staging --, every output compared
--merge needs no device: it puts the files that processes of the two builds wrote (run in turns) into one: per
build and measure the per-process medians, their median and max / min, and the ratios of this build's figures to
the parent's yardsticks; with --bench, under "bench_full", the headline and the inflate figure of the last JSON line
of two bench.py outputs.  profiles/bgzf_range_probe.json is such a file.
"""
import argparse
import json
import os
import random
import statistics
import struct
import sys
import zlib

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--members", type=int, default=4096)
ap.add_argument("--ranges", type=int, default=65536)
ap.add_argument("--out", default=None)
ap.add_argument("--merge", action="store_true")
ap.add_argument("--parent", nargs="*", default=[])
ap.add_argument("--new", nargs="*", default=[])
ap.add_argument("--bench", nargs=2, default=None, metavar=("PARENT.log", "NEW.log"))
ARGS = ap.parse_args()

YARDSTICKS = ("size_only", "members", "plain")
OWN = ("index", "random", "whole")


def merge():
    runs = {who: [json.load(open(f)) for f in files] for who, files in (("parent", ARGS.parent), ("new", ARGS.new))}
    first = runs["new"][0]
    out = {"what": "tools/probe_bgzf_ranges.py --merge: the parent commit's build (--tree) and this build in turns, a "
                   "process each; per process the median of three runs after a warm-up (HIP events); here per measure "
                   "the per-process medians in ms, their median, and max / min",
           "turns": {who: len(r) for who, r in runs.items()}}
    for k in ("device", "member_count", "file_bytes", "content_bytes", "ranges"):
        out[k] = first[k]

    def agg(rs, key):
        ms = [r[key]["median_ms"] for r in rs]
        d = {"ms": ms, "median_ms": round(statistics.median(ms), 4), "max_over_min": round(max(ms) / min(ms), 4),
             "ok": all(r[key]["ok"] for r in rs)}
        for extra in ("streams", "jobs", "delivered_bytes", "decoded_bytes", "decoded_per_delivered", "scratch_bytes"):
            if extra in rs[0][key]:
                d[extra] = rs[0][key][extra]
        return d

    for who in ("parent", "new"):
        out[who] = {key: agg(runs[who], key) for key in YARDSTICKS}
    for key in OWN:
        out["new"][key] = agg(runs["new"], key)
    p, n = out["parent"], out["new"]
    out["ratios"] = {f"{a}_over_parent_{b}": round(n[a]["median_ms"] / p[b]["median_ms"], 4)
                     for a in OWN + YARDSTICKS for b in YARDSTICKS if a in OWN or a == b}
    for key in ("random", "whole"):
        out["ratios"][f"{key}_delivered_GBps"] = round(n[key]["delivered_bytes"] / n[key]["median_ms"] / 1e6, 2)
    if ARGS.bench:
        out["bench_full"] = {}
        for who, log in zip(("parent", "new"), ARGS.bench):
            d = json.loads([line for line in open(log) if line.startswith("{")][-1])
            out["bench_full"][who] = {"headline_MBps": d["value"], "ms_per_step": d["ms_per_step"],
                                      "steps": d["steps"], "warmup": d["warmup"], "inflate_MBps": d["inflate"]["value"],
                                      "distinct_buffers_vs_oracle": d["checked"]["distinct_buffers_vs_oracle"],
                                      "of": d["checked"]["of"]}
    with open(ARGS.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out["ratios"], indent=1))


if ARGS.merge:
    merge()
    sys.exit(0)
sys.path.insert(0, os.path.abspath(ARGS.tree))
import torch  # noqa: E402

import zsc_amd  # noqa: E402
from zsc_amd import corpus  # noqa: E402

DEV = torch.device("cuda", 0)
MEMBER = 65536
DISTINCT = 512


def build(distinct):
    kinds = ("text", "text", "token", "table")
    bufs = [corpus.make_buffer(kinds[i % 4], MEMBER, 7000 + i) for i in range(distinct)]
    rc, raws, stats = zsc_amd.compress_batch(bufs, level=6, window_bits=-15)
    assert rc == 0 and all(s == 0 for s in stats)
    out = []
    for d, r in zip(bufs, raws):
        total = 18 + len(r) + 8
        assert total <= 65536
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\x00BC\x02\x00" + struct.pack("<H", total - 1) + r +
                   struct.pack("<II", zlib.crc32(d), len(d)))
    return bufs, out


def timed(ip, d_src, d_dst, runs=3):
    ip.run(d_src.data_ptr(), d_dst.data_ptr() if d_dst is not None else 0, 0)
    ip.results()
    ms = []
    for _ in range(runs):
        ip.run(d_src.data_ptr(), d_dst.data_ptr() if d_dst is not None else 0, 0)
        lens, used, stat, kms = ip.results()
        ms.append(kms)
    return lens, used, stat, ms


def entry(ok, ms, **more):
    return dict({"ok": bool(ok), "ms": [round(k, 4) for k in ms], "median_ms": round(statistics.median(ms), 4)}, **more)


def main():
    distinct = min(DISTINCT, ARGS.members)
    reps = ARGS.members // distinct
    count = distinct * reps
    bufs, members = build(distinct)
    one = b"".join(members)
    n_file, n_out = len(one) * reps, count * MEMBER
    d_unit = torch.frombuffer(bytearray(b"".join(bufs)), dtype=torch.uint8).to(DEV)
    d_content = d_unit.repeat(reps)
    has_ranges = hasattr(zsc_amd, "BgzfIndex")
    res = {"device": zsc_amd.device_info(), "tree": os.path.abspath(ARGS.tree), "member_count": count,
           "file_bytes": n_file, "content_bytes": n_out, "ranges": ARGS.ranges}
    d_file = torch.zeros(((n_file + 64 + 15) & ~15) + 64, dtype=torch.uint8, device=DEV)
    d_file[:n_file] = torch.frombuffer(bytearray(one), dtype=torch.uint8).to(DEV).repeat(reps)

    ip = zsc_amd.InflatePlan([n_file], None, window_bits=31, members=True, size_only=True)
    lens, used, stat, ms = timed(ip, d_file, None)
    res["size_only"] = entry(stat == [0] and lens == [n_out] and used == [n_file], ms)
    ip.close()
    print("size_only", res["size_only"], flush=True)

    ip = zsc_amd.InflatePlan([n_file], [n_out], window_bits=31, members=True)
    d_dst = torch.empty(ip.dst_bytes, dtype=torch.uint8, device=DEV)
    lens, used, stat, ms = timed(ip, d_file, d_dst)
    res["members"] = entry(stat == [0] and lens == [n_out] and ip.sections() == [count] and
                           torch.equal(d_dst[:n_out], d_content), ms)
    ip.close()
    del d_dst
    print("members", res["members"], flush=True)

    # the plain plan: each distinct member once in the input, every member ranges / members times in the plan
    per = max(1, ARGS.ranges // count)
    slots, at = [], 0
    for m in members:
        slots.append(at)
        at += (len(m) + 64 + 15) & ~15
    host = torch.zeros(at + 64, dtype=torch.uint8)
    for off, m in zip(slots, members):
        host[off:off + len(m)] = torch.frombuffer(bytearray(m), dtype=torch.uint8)
    d_src = host.to(DEV)
    n_streams = count * per
    ip = zsc_amd.InflatePlan([len(members[i % distinct]) for i in range(n_streams)], [MEMBER] * n_streams,
                             window_bits=31, src_offsets=[slots[i % distinct] for i in range(n_streams)])
    d_dst = torch.empty(ip.dst_bytes, dtype=torch.uint8, device=DEV)
    lens, used, stat, ms = timed(ip, d_src, d_dst)
    got = d_dst[:n_streams * (MEMBER + 64)].view(-1, distinct, MEMBER + 64)[:, :, :MEMBER]
    res["plain"] = entry(all(s == 0 for s in stat) and bool((got == d_unit.view(distinct, MEMBER)).all()), ms,
                         streams=n_streams, delivered_bytes=n_streams * MEMBER)
    ip.close()
    del d_dst, d_src, got
    print("plain", res["plain"], flush=True)

    if has_ranges:
        ms = []
        for k in range(4):
            ix = zsc_amd.BgzfIndex(d_file.data_ptr(), [n_file])
            if k:
                ms.append(ix.build_ms())
            if k < 3:
                ix.close()
        info = ix.info()
        res["index"] = entry(info == (count, n_file, n_out), ms, scratch_bytes=ix.scratch_bytes())
        print("index", res["index"], flush=True)

        rng = random.Random(11)
        kinds = {"random": [(rng.randrange(0, n_out - 100), rng.randrange(100, 256 * 1024 + 1))
                            for _ in range(ARGS.ranges)],
                 "whole": [((i % count) * MEMBER, MEMBER) for i in range(ARGS.ranges)]}
        for name, reqs in kinds.items():
            begins = [b for b, _ in reqs]
            sizes = [min(n, n_out - b) for b, n in reqs]
            plan = zsc_amd.InflatePlan.bgzf_ranges(ix, [0] * len(reqs), begins, sizes, sizes)
            d_dst = torch.empty(plan.dst_bytes, dtype=torch.uint8, device=DEV)
            lens, used, stat, ms = timed(plan, d_file, d_dst)
            ok = all(s == 0 for s in stat) and lens == sizes
            if name == "whole":
                got = d_dst[:len(reqs) * (MEMBER + 64)].view(-1, count, MEMBER + 64)[:, :, :MEMBER]
                ok = ok and bool((got == d_content.view(count, MEMBER)).all())
                del got
            else:
                for i in range(0, len(reqs), max(1, len(reqs) // 512)):
                    o = plan.dst_offsets[i]
                    ok = ok and torch.equal(d_dst[o:o + sizes[i]], d_content[begins[i]:begins[i] + sizes[i]])
            jobs, decoded = plan.jobs()
            delivered = sum(sizes)
            best = statistics.median(ms)
            res[name] = entry(ok, ms, jobs=jobs, delivered_bytes=delivered, decoded_bytes=decoded,
                              decoded_per_delivered=round(decoded / delivered, 4),
                              delivered_GBps=round(delivered / best / 1e6, 2), scratch_bytes=plan.scratch_bytes())
            plan.close()
            del d_dst
            print(name, res[name], flush=True)
        ix.close()

    if ARGS.out:
        os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
        with open(ARGS.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    if not all(v.get("ok", True) for v in res.values() if isinstance(v, dict)):
        sys.exit(1)


if __name__ == "__main__":
    main()
