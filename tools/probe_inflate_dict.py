#!/usr/bin/env python3
"""Plans with preset dictionaries (zsc_hip_inflate_plan_dict_enable) on small records, against the plain plan
on the same records written without a dictionary, device-resident.

    python tools/probe_inflate_dict.py [--streams 131072] [--distinct 512] [--repeats 5]
                                       [--parent-tree DIR] [--out FILE.json]

The batch: --distinct records of 256 B - 4 KiB, Canterbury-like text of zsc_amd/corpus.py, replicated to
--streams, and one shared 32 KiB dictionary cut from the same generator (the same seed, which is what gives
records and dictionary one vocabulary).  CPython's zlib writes every record
twice, outside the timed region: with the dictionary (zlib wrapper, FDICT) and without it.  Measured:
  - both compressed totals;
  - the dictionary plan over the streams written with the dictionary, against the plain plan over the streams
    written without it.  With --parent-tree the plain plan is the one of the checkout at DIR (built there:
    its zsc_amd/libzsc_hip.so), timed by this same file in a process of its own (--plain-only --tree DIR)
    before and after this build's runs, so that the spread of its own repeated runs in the session is known;
    this build's plain plan is timed besides.
The decode order keeps the replicas of a record out of each other's wavefronts (bench.py does the same for its
inflate batch).  Every result is checked against the records.  Times are the plans' own HIP events
(kernel_ms): after a warm-up run of every plan, --repeats rounds that alternate between the plans.
"""
import argparse
import json
import os
import subprocess
import sys
import time
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))


def tree_arg():
    for k, a in enumerate(sys.argv):
        if a == "--tree" and k + 1 < len(sys.argv):
            return os.path.abspath(sys.argv[k + 1])
    return os.path.dirname(HERE)


sys.path.insert(0, tree_arg())
import torch  # noqa: E402

import zsc_amd  # noqa: E402
from zsc_amd import corpus  # noqa: E402

DEV = torch.device("cuda", 0)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def make_batch(distinct):
    st = corpus.Stream(5151, 3)
    sizes = [256 + int(x) for x in st.below(distinct, 4096 - 256 + 1)]
    # (a seed of the text generator is a vocabulary: records and dictionary are cut from one buffer, as the
    # records of one source and a dictionary trained on earlier ones would be)
    text = corpus.make_buffer("text", 32768 + sum(sizes), 8999)
    d, records, at = text[:32768], [], 32768
    for n in sizes:
        records.append(text[at:at + n])
        at += n
    plain, withd = [], []
    for r in records:
        plain.append(zlib.compress(r, 6))
        co = zlib.compressobj(6, zlib.DEFLATED, 15, zdict=d)
        withd.append(co.compress(r) + co.flush())
    return records, d, plain, withd


def neighbours_differ(caps):
    """longest output first in steps of 64 bytes, and within a step replica by replica"""
    return sorted(range(len(caps)), key=lambda i: (-(caps[i] // 64), i))


def upload(ip, streams, reps):
    per = len(streams)
    span = ip.src_offsets[per] if reps > 1 else ip.src_bytes - 64
    host = torch.zeros(span, dtype=torch.uint8)
    for off, s in zip(ip.src_offsets, streams):
        host[off:off + len(s)] = torch.frombuffer(bytearray(s), dtype=torch.uint8)
    d_src = torch.zeros(ip.src_bytes, dtype=torch.uint8, device=DEV)
    d_src[:span * reps] = host.to(DEV).repeat(reps)
    return d_src


def check_outputs(ip, d_dst, records, reps, lens, used, stat, streams):
    n = len(records)
    ok = all(s == 0 for s in stat) and lens == [len(r) for r in records] * reps and used == [len(s) for s in streams] * reps
    host = d_dst.cpu().numpy()
    for k in list(range(n)) + list(range(n * (reps - 1), n * reps)):
        off = ip.dst_offsets[k]
        ok = ok and host[off:off + lens[k]].tobytes() == records[k % n]
    return ok


def alternate(plans, repeats):
    """plans: {name: (plan, d_src, d_dst)} -> ({name: [kernel_ms]}, {name: (lens, used, stat)})"""
    def run(name):
        ip, d_src, d_dst = plans[name]
        ip.run(d_src.data_ptr(), d_dst.data_ptr(), 0)
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


def report(r, name, t, out_bytes):
    r[name + "_kernel_ms"] = [round(x, 3) for x in t]
    r[name + "_best_ms"] = round(min(t), 3)
    r[name + "_median_ms"] = round(median(t), 3)
    r[name + "_spread"] = round(max(t) / min(t), 4)
    r[name + "_median_out_mb_s"] = round(out_bytes / median(t) / 1e3, 1)


def measure(a, with_dict):
    records, d, plain_s, dict_s = make_batch(a.distinct)
    reps = max(1, a.streams // a.distinct)
    caps = [len(r) for r in records] * reps
    order = neighbours_differ(caps)
    out_bytes = sum(caps)
    r = {"streams": len(caps), "distinct": a.distinct, "output_bytes": out_bytes,
         "plain_compressed_bytes": sum(len(s) for s in plain_s) * reps,
         "dict_compressed_bytes": sum(len(s) for s in dict_s) * reps, "dict_bytes": len(d)}
    r["dict_over_plain_compressed"] = round(r["dict_compressed_bytes"] / r["plain_compressed_bytes"], 4)
    plans = {}
    pp = zsc_amd.InflatePlan([len(s) for s in plain_s] * reps, caps, 15, decode_order=order)
    plans["plain"] = (pp, upload(pp, plain_s, reps), torch.empty(pp.dst_bytes, dtype=torch.uint8, device=DEV))
    if with_dict:
        dp = zsc_amd.InflatePlan([len(s) for s in dict_s] * reps, caps, 15, decode_order=order, dicts=[d])
        plans["dict"] = (dp, upload(dp, dict_s, reps), torch.empty(dp.dst_bytes, dtype=torch.uint8, device=DEV))
        r["dict_scratch_bytes"] = dp.scratch_bytes()
    times, outs = alternate(plans, a.repeats)
    r["ok"] = all(check_outputs(plans[n][0], plans[n][2], records, reps, *outs[n], plain_s if n == "plain" else dict_s)
                  for n in plans)
    for name, t in times.items():
        report(r, name, t, out_bytes)
    for ip, _, _ in plans.values():
        ip.close()
    return r


def parent_run(a, tag):
    """this file in a process of its own, on the checkout at --parent-tree: its plain plan alone"""
    out = os.path.join(a.scratch, f"parent_{tag}.json")
    subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-only", "--tree", a.parent_tree, "--streams",
                    str(a.streams), "--distinct", str(a.distinct), "--repeats", str(a.repeats), "--out", out], check=True)
    return json.load(open(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=131072)
    ap.add_argument("--distinct", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--plain-only", action="store_true", help="(the parent's side: no dictionary plan is made)")
    ap.add_argument("--tree", default=None, help="(the checkout whose zsc_amd is imported; this file's by default)")
    ap.add_argument("--scratch", default="/tmp")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    t0 = time.time()
    res = {"device": zsc_amd.device_info(), "repeats": a.repeats, "library": os.path.relpath(zsc_amd.lib_path, os.path.dirname(HERE))}
    w = zsc_amd.uncompress_batch([zlib.compress(b"warm" * 1000)], [4000])
    assert w[0] == 0
    if a.plain_only:
        res["batch"] = measure(a, False)
    else:
        if a.parent_tree:
            res["parent_before"] = parent_run(a, "before")
        res["batch"] = measure(a, True)
        b = res["batch"]
        if a.parent_tree:
            res["parent_after"] = parent_run(a, "after")
            pt = res["parent_before"]["batch"]["plain_kernel_ms"] + res["parent_after"]["batch"]["plain_kernel_ms"]
            b["parent_plain_kernel_ms"] = pt
            b["parent_plain_median_ms"] = round(median(pt), 3)
            b["parent_plain_spread"] = round(max(pt) / min(pt), 4)
            b["dict_over_parent_plain_median"] = round(b["dict_median_ms"] / median(pt), 4)
            b["plain_over_parent_plain_median"] = round(b["plain_median_ms"] / median(pt), 4)
        b["dict_over_plain_median"] = round(b["dict_median_ms"] / b["plain_median_ms"], 4)
    res["probe_seconds"] = round(time.time() - t0, 1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    ok = res["batch"]["ok"] and all(res[k]["batch"]["ok"] for k in ("parent_before", "parent_after") if k in res)
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
