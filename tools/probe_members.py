#!/usr/bin/env python3
"""Members plans (zsc_hip_inflate_plan_create_members) against the plain plan, device-resident.

    python tools/probe_members.py [--only 1234] [--members 4096] [--out FILE.json]

File A: --members BGZF members of 64 KiB of corpus data at level 6 (512 distinct ones, repeated); file B: the
same members without the `BC` subfield.  Four timings, kernel_ms of the plan (HIP events) after a warm-up run:
  1. the yardstick: the members of A as separate streams through a plain plan (the boundaries given);
  2. a members plan on A;
  3. a members plan on A with ZSC_HIP_MEMBERS_CLAIMS=0;
  4. a members plan on B.
Expected: (3) and (4) decode everything twice, near twice (1); (2) decodes once, near (1) plus the scan.
Every output is compared on the device with the input buffers.
"""
import argparse
import json
import os
import struct
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import zsc_amd  # noqa: E402
from zsc_amd import corpus  # noqa: E402

DEV = torch.device("cuda", 0)
MEMBER = 65536
DISTINCT = 512
BC = b"BC\x02\x00"


def build(distinct):
    kinds = ("text", "text", "token", "table")
    bufs = [corpus.make_buffer(kinds[i % 4], MEMBER, 7000 + i) for i in range(distinct)]
    rc, raws, stats = zsc_amd.compress_batch(bufs, level=6, window_bits=-15)
    assert rc == 0 and all(s == 0 for s in stats)
    a, b = [], []
    for d, r in zip(bufs, raws):
        tail = struct.pack("<II", zlib.crc32(d), len(d))
        total = 12 + 6 + len(r) + 8
        assert total <= 65536
        a.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\x00" + BC + struct.pack("<H", total - 1) + r + tail)
        b.append(b"\x1f\x8b\x08\x00\0\0\0\0\0\xff" + r + tail)
    return bufs, a, b


def timed(ip, d_src, d_dst, runs=3):
    ip.run(d_src.data_ptr(), d_dst.data_ptr(), 0)
    ip.results()
    ms = []
    for _ in range(runs):
        ip.run(d_src.data_ptr(), d_dst.data_ptr(), 0)
        lens, used, stat, kms = ip.results()
        ms.append(kms)
    return lens, used, stat, ms


def same(d_dst, d_unit, reps):
    return bool((d_dst[:reps * d_unit.numel()].view(reps, d_unit.numel()) == d_unit).all())


def entry(ok, ms, n_out, **more):
    best = min(ms)
    return dict({"ok": ok, "kernel_ms": [round(k, 3) for k in ms], "GBps_out": round(n_out / best / 1e6, 3)}, **more)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="1234")
    ap.add_argument("--members", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    distinct = min(DISTINCT, a.members)
    reps = a.members // distinct
    count = distinct * reps
    bufs, mem_a, mem_b = build(distinct)
    n_out = count * MEMBER
    d_unit = torch.frombuffer(bytearray(b"".join(bufs)), dtype=torch.uint8).to(DEV)
    res = {"device": zsc_amd.device_info(), "members": count, "output_bytes": n_out,
           "file_a_bytes": sum(map(len, mem_a)) * reps, "file_b_bytes": sum(map(len, mem_b)) * reps}

    if "1" in a.only:
        ip = zsc_amd.InflatePlan([len(m) for m in mem_a] * reps, [MEMBER] * count, window_bits=31)
        # (MEMBER + 64 is a multiple of 16, so the outputs lie MEMBER + 64 apart: compare them slot by slot)
        host = torch.zeros(ip.src_offsets[distinct] if reps > 1 else ip.src_bytes, dtype=torch.uint8)
        for off, s in zip(ip.src_offsets, mem_a):
            host[off:off + len(s)] = torch.frombuffer(bytearray(s), dtype=torch.uint8)
        d_src = torch.zeros(ip.src_bytes, dtype=torch.uint8, device=DEV)
        d_src[:host.numel() * reps] = host.to(DEV).repeat(reps)
        d_dst = torch.empty(ip.dst_bytes, dtype=torch.uint8, device=DEV)
        lens, used, stat, ms = timed(ip, d_src, d_dst)
        slots = d_dst[:count * (MEMBER + 64)].view(reps, distinct, MEMBER + 64)[:, :, :MEMBER]
        ok = all(s == 0 for s in stat) and lens == [MEMBER] * count and \
            bool((slots == d_unit.view(distinct, MEMBER)).all())
        res["1_plain_plan_separate_streams"] = entry(ok, ms, n_out)
        print("1", res["1_plain_plan_separate_streams"], flush=True)
        ip.close()
        del d_src, d_dst

    for key, name, members, claims in (("2", "2_members_plan_A", mem_a, "1"), ("3", "3_members_plan_A_claims_off", mem_a, "0"),
                                       ("4", "4_members_plan_B", mem_b, "1")):
        if key not in a.only:
            continue
        one = b"".join(members)
        os.environ["ZSC_HIP_MEMBERS_CLAIMS"] = claims  # (read when the plan is created)
        ip = zsc_amd.InflatePlan([len(one) * reps], [n_out], window_bits=31, members=True)
        del os.environ["ZSC_HIP_MEMBERS_CLAIMS"]
        d_src = torch.zeros(ip.src_bytes, dtype=torch.uint8, device=DEV)
        d_src[:len(one) * reps] = torch.frombuffer(bytearray(one), dtype=torch.uint8).to(DEV).repeat(reps)
        d_dst = torch.empty(ip.dst_bytes, dtype=torch.uint8, device=DEV)
        lens, used, stat, ms = timed(ip, d_src, d_dst)
        memb, claimed = ip.members()
        ok = stat == [0] and lens == [n_out] and used == [len(one) * reps] and memb == [count] and \
            ip.sections() == [count] and claimed == [count if members is mem_a and claims == "1" else 0] and \
            same(d_dst, d_unit, reps)
        res[name] = entry(ok, ms, n_out, claimed=claimed[0], prefix=ip.sections()[0], scratch_bytes=ip.scratch_bytes())
        print(key, res[name], flush=True)
        ip.close()
        del d_src, d_dst

    y = res.get("1_plain_plan_separate_streams")
    if y:
        for name in ("2_members_plan_A", "3_members_plan_A_claims_off", "4_members_plan_B"):
            if name in res:
                res[name]["over_yardstick"] = round(min(res[name]["kernel_ms"]) / min(y["kernel_ms"]), 3)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    if not all(v.get("ok", True) for v in res.values() if isinstance(v, dict)):
        sys.exit(1)


if __name__ == "__main__":
    main()
