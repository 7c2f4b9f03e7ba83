#!/usr/bin/env python3
"""BGZF files from a gzip deflate plan (zsc_hip_deflate_plan_bgzf) against the align-1 pack, device-resident.

    python tools/probe_bgzf.py [--tree DIR] [--only ab] [--buffers 4096] [--out FILE.json]

The workload: --buffers buffers of 65 280 bytes of corpus data at level 6, gzip wrapper (512 distinct ones,
repeated), one plan, one file.  After a warm-up:
  a. the move: ms of _pack with align 1 and of _bgzf on the same run's output, three each in turns (HIP events of
     the calls themselves).  --tree DIR imports zsc_amd from another checkout -- a build of the parent commit,
     which has no _bgzf: only the pack is timed there --, so that runs of the two builds can alternate;
  b. the way back: a members plan on the BGZF image and on the packed image, beside a plain plan on the same
     members as separate streams where the run left them; kernel_ms of the plans, three runs each.  Every output
     is compared on the device with the input.
"""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--only", default="ab")
ap.add_argument("--buffers", type=int, default=4096)
ap.add_argument("--out", default=None)
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.tree))
import torch  # noqa: E402

import zsc_amd  # noqa: E402
from zsc_amd import corpus  # noqa: E402

DEV = torch.device("cuda", 0)
BLOCK = 65280
DISTINCT = 512


def inflate_timed(ip, d_src, d_dst, runs=3):
    ip.run(d_src.data_ptr(), d_dst.data_ptr(), 0)
    ip.results()
    ms = []
    for _ in range(runs):
        ip.run(d_src.data_ptr(), d_dst.data_ptr(), 0)
        lens, used, stat, kms = ip.results()
        ms.append(round(kms, 3))
    return lens, used, stat, ms


def main():
    distinct = min(DISTINCT, ARGS.buffers)
    reps = ARGS.buffers // distinct
    count = distinct * reps
    kinds = ("text", "text", "token", "table")
    bufs = [corpus.make_buffer(kinds[i % 4], BLOCK, 7000 + i) for i in range(distinct)]
    n_in = count * BLOCK
    has_bgzf = hasattr(zsc_amd.DeflatePlan, "bgzf_enable")
    res = {"device": zsc_amd.device_info(), "tree": os.path.abspath(ARGS.tree), "buffers": count, "input_bytes": n_in}

    plan = zsc_amd.DeflatePlan([BLOCK] * count, 6, 31)
    plan.pack_enable(1)
    if has_bgzf:
        plan.bgzf_enable([0, count], 1)
    assert plan.in_offsets[1] == BLOCK  # (a multiple of 16: the buffers lie one behind the other)
    d_unit = torch.frombuffer(bytearray(b"".join(bufs)), dtype=torch.uint8).to(DEV)
    d_in = torch.zeros(plan.in_bytes, dtype=torch.uint8, device=DEV)
    d_in[:n_in] = d_unit.repeat(reps)
    d_out = torch.zeros(plan.out_bytes, dtype=torch.uint8, device=DEV)
    plan.run(d_in.data_ptr(), d_out.data_ptr())
    lens, stat = plan.results()
    assert all(s == 0 for s in stat)
    cap = sum(lens) + 8 * count + 28
    d_pack = torch.zeros(cap + 64, dtype=torch.uint8, device=DEV)
    d_bgzf = torch.zeros(cap + 64, dtype=torch.uint8, device=DEV)

    def pack_once():
        assert plan.pack(d_out.data_ptr(), d_pack.data_ptr(), cap) == 0
        total = plan.pack_results()[1]
        return total, plan.pack_ms()

    def bgzf_once():
        assert plan.bgzf(d_out.data_ptr(), d_bgzf.data_ptr(), cap) == 0
        t = plan.bgzf_results()
        assert t["file_statuses"] == [0]
        return t["total"], plan.bgzf_ms()

    pack_total = pack_once()[0]
    bgzf_total = bgzf_once()[0] if has_bgzf else None
    if "a" in ARGS.only:
        pk, bz = [], []
        for _ in range(3):
            pk.append(round(pack_once()[1], 4))
            if has_bgzf:
                bz.append(round(bgzf_once()[1], 4))
        res["a_pack_align1"] = {"bytes": pack_total, "ms": pk, "median_ms": statistics.median(pk)}
        if has_bgzf:
            assert bgzf_total == pack_total + 8 * count + 28
            res["a_bgzf"] = {"bytes": bgzf_total, "ms": bz, "median_ms": statistics.median(bz)}
        print("a", res.get("a_pack_align1"), res.get("a_bgzf"), flush=True)

    if "b" in ARGS.only and has_bgzf:
        n_out = n_in

        def same(d_dst):
            return bool((d_dst[:n_out].view(reps, distinct * BLOCK) == d_unit).all())

        ip = zsc_amd.InflatePlan(lens, [BLOCK] * count, window_bits=31, src_offsets=plan.out_offsets)
        d_dst = torch.empty(ip.dst_bytes, dtype=torch.uint8, device=DEV)
        olens, used, istat, ms = inflate_timed(ip, d_out, d_dst)
        assert ip.dst_offsets[1] == BLOCK + 64  # (a multiple of 16: the slots lie that far apart)
        slots = d_dst[:count * (BLOCK + 64)].view(reps, distinct, BLOCK + 64)[:, :, :BLOCK]
        ok = all(s == 0 for s in istat) and olens == [BLOCK] * count and \
            bool((slots == d_unit.view(distinct, BLOCK)).all())
        res["b1_plain_plan_separate_streams"] = {"ok": ok, "kernel_ms": ms}
        print("b1", res["b1_plain_plan_separate_streams"], flush=True)
        ip.close()
        del d_dst
        for name, image, total, claims in (("b2_members_plan_on_bgzf", d_bgzf, bgzf_total, count + 1),
                                           ("b3_members_plan_on_pack_align1", d_pack, pack_total, 0)):
            ip = zsc_amd.InflatePlan([total], [n_out], window_bits=31, members=True, src_offsets=[0])
            d_dst = torch.empty(ip.dst_bytes, dtype=torch.uint8, device=DEV)
            olens, used, istat, ms = inflate_timed(ip, image, d_dst)
            memb, claimed = ip.members()
            ok = istat == [0] and olens == [n_out] and used == [total] and claimed == [claims] and \
                memb == [count + (1 if claims else 0)] and same(d_dst)
            res[name] = {"ok": ok, "kernel_ms": ms, "claimed": claimed[0], "members": memb[0],
                         "over_plain": round(min(ms) / min(res["b1_plain_plan_separate_streams"]["kernel_ms"]), 3)}
            print(name, res[name], flush=True)
            ip.close()
            del d_dst
    plan.close()
    if ARGS.out:
        os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
        with open(ARGS.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    if not all(v.get("ok", True) for v in res.values() if isinstance(v, dict)):
        sys.exit(1)


if __name__ == "__main__":
    main()
