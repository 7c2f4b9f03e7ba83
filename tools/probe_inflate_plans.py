#!/usr/bin/env python3
"""The launches of every kind of inflate plan, and the host cost of making a chunks plan.

    python tools/probe_inflate_plans.py                      one run of each kind (for rocprofv3 --kernel-trace)
    python tools/probe_inflate_plans.py --launches TRACE.csv the trace as lines of "kernel grid workgroup", in order
    python tools/probe_inflate_plans.py --create 21          create + destroy of a chunks plan over 4096 streams

The batch is the largest of tests/test_gpu_inflate_plan_kinds.py: outputs of 0, 1 and 300 bytes and one
incompressible stream of a little over three chunks with a full flush in its middle.  Before the seven runs the
indexes are taken from a chunks plan that keeps them, so the trace starts with that plan's launches.
"""
import argparse
import csv
import itertools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run_kinds():
    import torch
    import test_gpu_inflate_plan_kinds as t
    streams = t.batches()[2]
    caps = [len(t._inflate(s)[0]) for s in streams]
    blobs = t.build_blobs(torch, streams, caps)
    for kind in t.KINDS:
        plan = t.make_plan(kind, [len(s) for s in streams], caps, blobs)
        src = t.upload(torch, plan, streams)
        dst = torch.zeros(plan.dst_bytes, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        plan.run(src.data_ptr(), 0 if kind in ("size", "check") else dst.data_ptr(), 0)
        lens, used, stat, _ = plan.results()
        assert stat == [0] * len(streams) and lens == caps, (kind, stat, lens)
        print(kind, "pieces", plan.sections(), "scratch", plan.scratch_bytes(), flush=True)
        plan.close()


def launches(path):
    """the library's kernels (k_*) and the fills of its hipMemsetAsync calls in a rocprofv3 kernel trace, in the
    order they were dispatched (torch fills with kernels of its own)"""
    with open(path, newline="") as f:
        rows = [r for r in csv.DictReader(f) if r["Kernel_Name"].startswith(("k_", "__amd_rocclr_fillBuffer"))]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))  # (start times of launches back to back may cross by a few hundred ns)
    lines = [" ".join((r["Kernel_Name"].split("(")[0], r["Grid_Size_X"], r["Workgroup_Size_X"])) for r in rows]
    for line, run in itertools.groupby(lines):  # (a run of equal launches, the fills mostly, on one line)
        n = len(list(run))
        print(line if n == 1 else f"{line} x{n}")


def create_destroy(repeats):
    """4096 streams of the inflate benchmark's sizes (outputs of 4-64 KiB, a third of that compressed), cut at the
    default chunk size (no stream is cut) and at the least one (nearly every stream is)"""
    import zsc_amd
    from zsc_amd import corpus
    st = corpus.Stream(4242, 3)
    caps = [4096 + int(x) for x in st.below(4096, 65536 - 4096 + 1)]
    lens = [c // 3 for c in caps]
    zsc_amd.InflatePlan(lens, caps, chunks=True).close()
    res = {"streams": len(lens)}
    for name, cb in (("default_chunk", 0), ("least_chunk", 4096)):
        ms = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            zsc_amd.InflatePlan(lens, caps, chunks=True, chunk_bytes=cb).close()
            ms.append(round((time.perf_counter() - t0) * 1e3, 3))
        res[name] = {"ms": ms, "min": min(ms), "median": sorted(ms)[len(ms) // 2], "max": max(ms)}
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", metavar="TRACE.csv")
    ap.add_argument("--create", type=int, default=0, metavar="REPEATS")
    a = ap.parse_args()
    if a.launches:
        launches(a.launches)
    elif a.create:
        create_destroy(a.create)
    else:
        run_kinds()
