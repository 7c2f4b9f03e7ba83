#!/usr/bin/env python3
"""Check plans (zsc_hip_inflate_plan_create_check) against the full inflate of the same streams, device-resident.

    python tools/probe_inflate_check.py [--only ab] [--a-streams 65536] [--b-mib 256] [--repeats 3]
                                        [--out FILE.json]

(a) --a-streams gzip members of 4-64 KiB (the size probe's batch: 512 distinct members replicated): the
    check plan against the plain plan and the size plan;
(b) one --b-mib MiB marker-free level-1 zlib stream (the size probe's text): the check plan against the
    chunks plan, both at the default chunk_bytes.
Every result is checked, the check values against zlib's.  Times are the plans' own HIP events (kernel_ms):
after a warm-up run of every plan, --repeats rounds that alternate between the plans; best, median and
spread of each, the ratios of the check plan's to its yardsticks', and the device memory each side held
(scratch_bytes() plus the output buffer the yardstick needs).
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
from probe_inflate_size import alternate, ratios, report  # noqa: E402


def part_a(res, nstreams, repeats):
    distinct = 512
    st = corpus.Stream(4242, 3)
    sizes = [4096 + int(x) for x in st.below(distinct, 65536 - 4096 + 1)]
    kinds = ("text", "text", "token", "table")
    bufs = [corpus.make_buffer(kinds[i % 4], sizes[i], 7000 + i) for i in range(distinct)]
    rc, members, stats = zsc_amd.compress_batch(bufs, level=6, window_bits=31)
    assert rc == 0
    reps = max(1, nstreams // distinct)
    slens, caps = [len(m) for m in members] * reps, sizes * reps
    plain = zsc_amd.InflatePlan(slens, caps, window_bits=31)
    size = zsc_amd.InflatePlan(slens, None, window_bits=31, size_only=True)
    check = zsc_amd.InflatePlan(slens, None, window_bits=31, check_only=True)
    d_src = upload(plain, members, reps)
    assert size.src_offsets == plain.src_offsets and check.src_offsets == plain.src_offsets
    plans = {"plain": (plain, d_src, torch.empty(plain.dst_bytes, dtype=torch.uint8, device=DEV)),
             "size": (size, d_src, None), "check": (check, d_src, None)}
    times, outs = alternate(plans, repeats)
    ok = outs["plain"] == outs["check"] == outs["size"] and all(s == 0 for s in outs["check"][2])
    ok = ok and outs["check"][0] == caps and check.check_values() == [zlib.crc32(b) for b in bufs] * reps
    r = {"ok": ok, "streams": len(slens), "input_bytes": sum(slens), "output_bytes": sum(caps),
         "plain_device_bytes": plain.scratch_bytes() + plain.dst_bytes,
         "size_device_bytes": size.scratch_bytes(), "check_device_bytes": check.scratch_bytes()}
    r.update(report(times))
    ratios(r, times, "check", "plain", "check_over_plain")
    ratios(r, times, "check", "size", "check_over_size")
    res["a_members"] = r
    print("a", r, flush=True)
    for ip in (plain, size, check):
        ip.close()


def part_b(res, mib, repeats):
    rng = np.random.default_rng(9)
    words = [bytes(rng.integers(97, 123, rng.integers(2, 9), dtype=np.uint8)) for _ in range(4000)]
    idx = rng.integers(0, len(words), 50_000_000 * mib // 256 + 1000)
    text = b" ".join(words[i] for i in idx)[: mib << 20]
    text += b"x" * ((mib << 20) - len(text))
    s = zlib.compress(text, 1)
    assert s.count(b"\x00\x00\xff\xff") < 64
    n = len(text)
    print("b: stream made", len(s), flush=True)
    chunks = zsc_amd.InflatePlan([len(s)], [n], chunks=True)
    check = zsc_amd.InflatePlan([len(s)], None, check_only=True)
    d_src = upload(chunks, [s])
    d_dst = torch.empty(chunks.dst_bytes, dtype=torch.uint8, device=DEV)
    times, outs = alternate({"chunks": (chunks, d_src, d_dst), "check": (check, d_src, None)}, repeats)
    ok = all(o == ([n], [len(s)], [0]) for o in outs.values())
    ok = ok and bytes(d_dst[:n].cpu().numpy()) == text and check.check_values() == [zlib.adler32(text)]
    pieces = {"chunks": chunks.sections()[0], "check": check.sections()[0]}
    ok = ok and pieces["check"] > 1 and pieces["check"] == pieces["chunks"]
    r = {"ok": ok, "input_bytes": len(s), "output_bytes": n, "pieces": pieces,
         "chunks_device_bytes": chunks.scratch_bytes() + chunks.dst_bytes, "check_device_bytes": check.scratch_bytes()}
    r.update(report(times))
    ratios(r, times, "check", "chunks", "check_over_chunks")
    res["b_one_stream"] = r
    print("b", r, flush=True)
    chunks.close()
    check.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="ab")
    ap.add_argument("--a-streams", type=int, default=65536)
    ap.add_argument("--b-mib", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"device": zsc_amd.device_info(), "repeats": a.repeats}
    t0 = time.time()
    w = zsc_amd.uncompress_batch([zlib.compress(b"warm" * 1000)], [4000])
    assert w[0] == 0
    if "a" in a.only:
        part_a(res, a.a_streams, a.repeats)
    if "b" in a.only:
        part_b(res, a.b_mib, a.repeats)
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
