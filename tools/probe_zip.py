#!/usr/bin/env python3
"""ZIP archives from a gzip deflate plan (zsc_hip_deflate_plan_zip) against the align-1 pack, device-resident.

    python tools/probe_zip.py [--tree DIR] [--buffers 4096] [--per-archive 16] [--out FILE.json]

The workload: --buffers buffers of 65 280 bytes of corpus data at level 6, gzip wrapper (512 distinct ones,
repeated), one plan; written once as ONE archive and once as archives of --per-archive buffers.  After a
warm-up, ms of _pack with align 1 and of _zip on the same run's output, three each in turns (HIP events of the
calls themselves), the median reported.  --tree DIR imports zsc_amd from another checkout -- a build of the
parent commit, which has no _zip: only the pack is timed there --, so that processes of the two builds can
alternate.  Every archive is walked on the host once (tests/zip_cases.py) and one entry of each shape is
inflated with CPython's zlib and compared with its input.
"""
import argparse
import json
import os
import statistics
import sys
import zlib

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--buffers", type=int, default=4096)
ap.add_argument("--per-archive", type=int, default=16)
ap.add_argument("--out", default=None)
ARGS = ap.parse_args()
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tests"))
sys.path.insert(0, os.path.abspath(ARGS.tree))
import torch  # noqa: E402

import zsc_amd  # noqa: E402
from zsc_amd import corpus  # noqa: E402

DEV = torch.device("cuda", 0)
BLOCK = 65280
DISTINCT = 512


def main():
    distinct = min(DISTINCT, ARGS.buffers)
    reps = ARGS.buffers // distinct
    count = distinct * reps
    kinds = ("text", "text", "token", "table")
    bufs = [corpus.make_buffer(kinds[i % 4], BLOCK, 7000 + i) for i in range(distinct)]
    n_in = count * BLOCK
    has_zip = hasattr(zsc_amd.DeflatePlan, "zip_enable")
    res = {"device": zsc_amd.device_info(), "tree": os.path.abspath(ARGS.tree), "buffers": count, "input_bytes": n_in}

    plan = zsc_amd.DeflatePlan([BLOCK] * count, 6, 31)
    plan.pack_enable(1)
    assert plan.in_offsets[1] == BLOCK  # (a multiple of 16: the buffers lie one behind the other)
    d_unit = torch.frombuffer(bytearray(b"".join(bufs)), dtype=torch.uint8).to(DEV)
    d_in = torch.zeros(plan.in_bytes, dtype=torch.uint8, device=DEV)
    d_in[:n_in] = d_unit.repeat(reps)
    d_out = torch.zeros(plan.out_bytes, dtype=torch.uint8, device=DEV)
    plan.run(d_in.data_ptr(), d_out.data_ptr())
    lens, stat = plan.results()
    assert all(s == 0 for s in stat)
    names = [b"shard/%06d.bin" % i for i in range(count)]
    cap = sum(lens) + (76 + 2 * 16) * count + 98 * count
    d_pack = torch.zeros(cap + 64, dtype=torch.uint8, device=DEV)
    d_zip = torch.zeros(cap + 64, dtype=torch.uint8, device=DEV)

    def pack_once():
        assert plan.pack(d_out.data_ptr(), d_pack.data_ptr(), cap) == 0
        total = plan.pack_results()[1]
        return total, plan.pack_ms()

    def zip_once():
        assert plan.zip(d_out.data_ptr(), d_zip.data_ptr(), cap) == 0
        t = plan.zip_results()
        assert not any(t["arch_statuses"])
        return t, plan.zip_ms()

    pack_total = pack_once()[0]
    shapes = (("one_archive", [0, count]), ("archives_of_%d" % ARGS.per_archive,
                                            list(range(0, count, ARGS.per_archive)) + [count]))
    for title, first in shapes:
        if has_zip:
            plan.zip_enable(first, names)
            t = zip_once()[0]
            from zip_cases import walk
            host = d_zip[:t["total"]].cpu().numpy().tobytes()
            for a in range(len(first) - 1):
                entries, _ = walk(host[t["arch_offsets"][a]:t["arch_offsets"][a] + t["arch_lens"][a]])
                assert len(entries) == first[a + 1] - first[a]
                e = entries[0]
                at = t["arch_offsets"][a] + e["data_offset"]
                assert zlib.decompress(host[at:at + e["csize"]], -15) == bufs[first[a] % distinct]
        pk, zp = [], []
        for _ in range(3):
            pk.append(round(pack_once()[1], 4))
            if has_zip:
                zp.append(round(zip_once()[1], 4))
        res[title] = {"archives": len(first) - 1,
                      "pack_align1": {"bytes": pack_total, "ms": pk, "median_ms": statistics.median(pk)}}
        if has_zip:
            res[title]["zip"] = {"bytes": t["total"], "ms": zp, "median_ms": statistics.median(zp),
                                 "bytes_over_pack": round(t["total"] / pack_total, 5)}
        print(title, res[title], flush=True)
    plan.close()
    if ARGS.out:
        os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
        with open(ARGS.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
