#!/usr/bin/env python3
"""What read-back verification of a deflate plan costs.  Needs an MI355X: there is no CPU path to fall back to.

    python tools/probe_deflate_verify.py [--copies 512] [--runs 5] [--parent-root DIR] [--out FILE.json]

The bench's headline shape (Canterbury-like x --copies, level 6): a plan that never enables verification and
a plan that does, each warmed up and then run --runs times with profiling on.  Reported: the whole pass
(index 8 of zsc_hip_deflate_plan_times) of both, and the device time of zsc_hip_deflate_plan_verify on the
second (every verdict must be OK); the streams of both plans are compared on the device.

--parent-root DIR: a directory holding another build's `zsc_amd` package (the parent commit's, built with the
same flags).  The never-enabled plan is then measured on that build too, by this script in a child process
(--baseline-only --root DIR), before and after this build's own measurement, so that the figures share one
session: an un-enabled plan must cost what it cost before the feature existed.

Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 3), "spread_ms": round(max(ms) - min(ms), 3),
            "runs_ms": [round(m, 3) for m in ms]}


def measure(zsc_amd, torch, copies, seeds, runs, verify):
    from zsc_amd import corpus
    sets = [corpus.canterbury_like(s) for s in range(seeds)]
    bufs = [b for st in sets for _, b in st]
    lens = [len(b) for b in bufs] * (copies // seeds)
    plan = zsc_amd.DeflatePlan(lens, level=6)
    if verify:
        plan.verify_enable()
    per = plan.in_offsets[len(bufs)] if len(bufs) < len(lens) else plan.in_bytes - 64
    host = torch.zeros(per, dtype=torch.uint8)
    for off, b in zip(plan.in_offsets, bufs):
        host[off:off + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8)
    d_in = torch.zeros(plan.in_bytes, dtype=torch.uint8, device="cuda")
    d_in[:plan.in_bytes - 64] = host.to("cuda").repeat(copies // seeds)[:plan.in_bytes - 64]
    d_out = torch.zeros(plan.out_bytes, dtype=torch.uint8, device="cuda")
    plan.run(d_in.data_ptr(), d_out.data_ptr())
    plan.results()
    total, vms = [], []
    ok = True
    for _ in range(runs):
        plan.profile(True)  # (a new measurement window: the times of this run alone)
        plan.run(d_in.data_ptr(), d_out.data_ptr())
        slens, stat = plan.results()
        total.append(plan.kernel_times_ms()["total"])
        ok = ok and all(s == 0 for s in stat)
        if verify:
            ok = ok and plan.verify(d_in.data_ptr(), d_out.data_ptr()) == 0
            res = plan.verify_results()
            ok = ok and all(r["verdict"] == 0 for r in res)
            vms.append(plan.verify_ms())
    o = {"ok": ok, "input_bytes": sum(lens), "buffers": len(lens), "whole_pass": summary(total),
         "sub_batches": plan.sub_batches, "scratch_bytes": plan.scratch_bytes}
    if verify:
        o["verify"] = summary(vms)
        o["verify_share_of_whole_pass"] = round(o["verify"]["median_ms"] / o["whole_pass"]["median_ms"], 5)
        o["blocks"] = sum(len(plan.verify_blocks(i)) for i in range(len(bufs))) * (copies // seeds)
        # one flipped bit must be found, so that the time above is that of a check that checks
        d_out[plan.out_offsets[1] + slens[1] // 2] ^= 4
        ok2 = plan.verify(d_in.data_ptr(), d_out.data_ptr()) == 0
        res = plan.verify_results()
        o["ok"] = ok and ok2 and res[1]["verdict"] > 0 and all(r["verdict"] == 0 for k, r in enumerate(res) if k != 1)
        d_out[plan.out_offsets[1] + slens[1] // 2] ^= 4
    head = d_out[:plan.out_offsets[len(bufs)]].clone()
    plan.close()
    return o, head


def parent_baseline(root, a):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--baseline-only", "--root", root, "--copies", str(a.copies),
                        "--seeds", str(a.seeds), "--runs", str(a.runs)], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.exit(f"the parent build's measurement failed: {r.stdout[-2000:]} {r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=512)
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    parent = [parent_baseline(a.parent_root, a)] if a.parent_root else []  # (before this process opens the GPU)
    sys.path.insert(0, a.root)
    import torch
    import zsc_amd
    if not torch.cuda.is_available():
        sys.exit("probe_deflate_verify needs an MI355X: no GPU here")
    seeds = max(1, min(a.seeds, a.copies))
    t0 = time.time()
    assert zsc_amd.compress_batch([b"warm" * 1000])[0] == 0
    if a.baseline_only:
        o, _ = measure(zsc_amd, torch, a.copies, seeds, a.runs, False)
        print(json.dumps(o))
        sys.exit(0 if o["ok"] else 1)
    res = {"device": zsc_amd.device_info(), "shape": f"canterbury_like x{a.copies}, level 6"}
    off, head_off = measure(zsc_amd, torch, a.copies, seeds, a.runs, False)
    on, head_on = measure(zsc_amd, torch, a.copies, seeds, a.runs, True)
    on["ok"] = on["ok"] and bool((head_on == head_off).all())
    res["verify_never_enabled"], res["verify_enabled"] = off, on
    del head_on, head_off
    torch.cuda.empty_cache()
    zsc_amd.lib.zsc_hip_release_cached_memory()
    if a.parent_root:
        parent.append(parent_baseline(a.parent_root, a))
        res["parent_build_before"], res["parent_build_after"] = parent
        pm = statistics.median(parent[0]["whole_pass"]["runs_ms"] + parent[1]["whole_pass"]["runs_ms"])
        res["never_enabled_over_parent"] = round(off["whole_pass"]["median_ms"] / pm, 4)
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
