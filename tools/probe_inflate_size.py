#!/usr/bin/env python3
"""Size plans (zsc_hip_inflate_plan_create_size) against the full inflate of the same streams, device-resident.

    python tools/probe_inflate_size.py [--only ab] [--a-streams 65536] [--b-mib 256] [--b-serial-mib 16]
                                       [--repeats 5] [--out FILE.json]

(a) --a-streams zlib members of 4-64 KiB (the bench's inflate mix, 512 distinct members replicated): the
    size plan against the plain plan;
(b) one --b-mib MiB marker-free level-1 zlib stream (the text of test_256mib_marker_free_stream): the size
    plan (default chunk_bytes: sized in pieces) against the chunks plan, and against one run of the plain
    plan (which decodes the stream serially, in about a minute); then, on the first --b-serial-mib MiB of
    the same text, the size plan that never cuts a stream (the whole-stream size decode) against the plain
    plan.
Every result is checked.  Times are the plans' own HIP events (kernel_ms): after a warm-up run of every
plan, --repeats rounds that alternate between the plans; best and median of each, and the ratios of the
size plan's to the full inflate's.
"""
import argparse
import json
import os
import sys
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import zsc_amd  # noqa: E402
from zsc_amd import corpus  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
from probe_inflate_sections import DEV, upload  # noqa: E402


def median(xs):
    return sorted(xs)[len(xs) // 2]


def alternate(plans, repeats):
    """plans: {name: (plan, d_src, d_dst or None)} -> ({name: [kernel_ms]}, {name: (lens, used, stat)})"""
    def run(name):
        ip, d_src, d_dst = plans[name]
        ip.run(d_src.data_ptr(), d_dst.data_ptr() if d_dst is not None else 0, 0)
        lens, used, stat, kms = ip.results()
        return (lens, used, stat), kms
    times, outs = {name: [] for name in plans}, {}
    for name in plans:  # warm-up
        run(name)
    for k in range(repeats):
        for name in plans:
            outs[name], kms = run(name)
            times[name].append(kms)
        print("round", k, {name: round(t[-1], 3) for name, t in times.items()}, flush=True)
    return times, outs


def report(times):
    r = {}
    for name, t in times.items():
        r[name + "_kernel_ms"] = [round(x, 3) for x in t]
        r[name + "_best_ms"] = round(min(t), 3)
        r[name + "_median_ms"] = round(median(t), 3)
        r[name + "_spread"] = round(max(t) / min(t), 4)
    return r


def ratios(r, times, size_name, full_name, key):
    r[key + "_best"] = round(min(times[size_name]) / min(times[full_name]), 4)
    r[key + "_median"] = round(median(times[size_name]) / median(times[full_name]), 4)


def part_a(res, nstreams, repeats):
    distinct = 512
    st = corpus.Stream(4242, 3)
    sizes = [4096 + int(x) for x in st.below(distinct, 65536 - 4096 + 1)]
    kinds = ("text", "text", "token", "table")
    bufs = [corpus.make_buffer(kinds[i % 4], sizes[i], 7000 + i) for i in range(distinct)]
    rc, members, stats = zsc_amd.compress_batch(bufs, level=6, window_bits=15)
    assert rc == 0
    reps = max(1, nstreams // distinct)
    slens, caps = [len(m) for m in members] * reps, sizes * reps
    plain = zsc_amd.InflatePlan(slens, caps)
    size = zsc_amd.InflatePlan(slens, None, size_only=True)
    d_src = upload(plain, members, reps)
    assert size.src_offsets == plain.src_offsets
    plans = {"plain": (plain, d_src, torch.empty(plain.dst_bytes, dtype=torch.uint8, device=DEV)),
             "size": (size, d_src, None)}
    times, outs = alternate(plans, repeats)
    ok = outs["plain"] == outs["size"] and all(s == 0 for s in outs["size"][2]) and outs["size"][0] == caps
    r = {"ok": ok, "streams": len(slens), "input_bytes": sum(slens), "output_bytes": sum(caps),
         "size_scratch_bytes": size.scratch_bytes()}
    r.update(report(times))
    ratios(r, times, "size", "plain", "size_over_plain")
    res["a_members"] = r
    print("a", r, flush=True)
    plain.close()
    size.close()


def part_b(res, mib, serial_mib, repeats):
    rng = np.random.default_rng(9)
    words = [bytes(rng.integers(97, 123, rng.integers(2, 9), dtype=np.uint8)) for _ in range(4000)]
    idx = rng.integers(0, len(words), 50_000_000 * mib // 256 + 1000)
    text = b" ".join(words[i] for i in idx)[: mib << 20]
    text += b"x" * ((mib << 20) - len(text))
    s = zlib.compress(text, 1)
    assert s.count(b"\x00\x00\xff\xff") < 64
    n = len(text)
    print("b: stream made", len(s), flush=True)
    # the whole stream: the size plan and the chunks plan alternate; the plain plan decodes it serially
    # (a minute or so), so it runs once
    plain = zsc_amd.InflatePlan([len(s)], [n])
    chunks = zsc_amd.InflatePlan([len(s)], [n], chunks=True)
    size = zsc_amd.InflatePlan([len(s)], None, size_only=True)
    d_src = upload(plain, [s])
    d_dst = torch.empty(plain.dst_bytes, dtype=torch.uint8, device=DEV)
    times, outs = alternate({"chunks": (chunks, d_src, d_dst), "size": (size, d_src, None)}, repeats)
    ok = all(o == ([n], [len(s)], [0]) for o in outs.values())
    ok = ok and bytes(d_dst[:n].cpu().numpy()) == text
    pieces = {"chunks": chunks.sections()[0], "size": size.sections()[0]}
    ok = ok and pieces["size"] > 1
    print("b: chunked plans done", flush=True)
    d_dst.zero_()
    plain.run(d_src.data_ptr(), d_dst.data_ptr(), 0)
    lens, used, stat, plain_ms = plain.results()
    ok = ok and (lens, used, stat) == ([n], [len(s)], [0]) and bytes(d_dst[:n].cpu().numpy()) == text
    r = {"ok": ok, "input_bytes": len(s), "output_bytes": n, "pieces": pieces,
         "chunks_scratch_bytes": chunks.scratch_bytes(), "size_scratch_bytes": size.scratch_bytes(),
         "plain_single_run_ms": round(plain_ms, 1)}
    r.update(report(times))
    ratios(r, times, "size", "chunks", "size_over_chunks")
    r["size_over_plain_single_run"] = round(median(times["size"]) / plain_ms, 6)
    res["b_one_stream"] = r
    print("b", r, flush=True)
    for ip in (plain, chunks, size):
        ip.close()
    del d_src, d_dst
    # the whole-stream size decode against the plain plan, one group each: the first serial_mib MiB of the
    # same text (five repeats of the whole stream would take ten minutes)
    small = text[: serial_mib << 20]
    cs = zlib.compress(small, 1)
    plain = zsc_amd.InflatePlan([len(cs)], [len(small)])
    whole = zsc_amd.InflatePlan([len(cs)], None, size_only=True, chunk_bytes=zsc_amd.NO_LIMIT)
    d_src = upload(plain, [cs])
    d_dst = torch.empty(plain.dst_bytes, dtype=torch.uint8, device=DEV)
    times, outs = alternate({"plain": (plain, d_src, d_dst), "size_never_cut": (whole, d_src, None)}, repeats)
    ok = all(o == ([len(small)], [len(cs)], [0]) for o in outs.values()) and whole.sections() == [0]
    ok = ok and bytes(d_dst[:len(small)].cpu().numpy()) == small
    r = {"ok": ok, "input_bytes": len(cs), "output_bytes": len(small)}
    r.update(report(times))
    ratios(r, times, "size_never_cut", "plain", "size_never_cut_over_plain")
    res["b_one_stream_serial"] = r
    print("b serial", r, flush=True)
    plain.close()
    whole.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="ab")
    ap.add_argument("--a-streams", type=int, default=65536)
    ap.add_argument("--b-mib", type=int, default=256)
    ap.add_argument("--b-serial-mib", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"device": zsc_amd.device_info(), "repeats": a.repeats}
    t0 = time.time()
    w = zsc_amd.uncompress_batch([zlib.compress(b"warm" * 1000)], [4000])
    assert w[0] == 0
    if "a" in a.only:
        part_a(res, a.a_streams, a.repeats)
    if "b" in a.only:
        part_b(res, a.b_mib, a.b_serial_mib, a.repeats)
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
