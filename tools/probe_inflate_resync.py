#!/usr/bin/env python3
"""Resync inflate (zsc_hip_inflate_plan_create_resync) on damaged full-flush streams, device-resident.

    python tools/probe_inflate_resync.py [--gib 1] [--reps 3] [--no-serial] [--out FILE.json]

One --gib GiB-output zlib stream in 64 KiB full-flush sections (a 16 MiB text-mix unit compressed by
stock zlib level 6 with Z_FULL_FLUSH every 64 KiB, its sections repeated), and these cases, alternated
round by round after one warm-up run each:
  clean_sections     the clean stream through a sections plan;
  clean_resync       the clean stream through a resync plan;
  damaged1_resync    1 % of its sections damaged (their first 5 bytes made a stored block with
                     LEN != ~NLEN), through a resync plan;
  damaged10_resync   10 % damaged, through a resync plan;
  serial16_plain     a 16 MiB stream of the same kind, 1 % damaged, through the plain plan (the serial
                     decoder; skipped with --no-serial).
Every output, status, consumed count, data error count and section count is checked against the
construction.  Times: kernel_ms (HIP events of the plan's run: for the plain plan only its first
k_inflate launch, so its rate comes from wall_ms) and wall_ms (run + results, with the host's
relaunches for resynchronisation).
"""
import argparse
import json
import os
import sys
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import zsc_amd  # noqa: E402
from zsc_amd import corpus  # noqa: E402

DEV = torch.device("cuda", 0)
MARK = b"\x00\x00\xff\xff"
BAD_BLOCK = b"\x00\x34\x12\x55\x55"
SECTION = 65536
UNIT = 16 << 20


def unit_stream(seed=900):
    """a raw stream of 64 KiB sections of a text-mix, each ending in a marker; the offsets where the
    sections start"""
    kinds = ("text", "table", "token", "object")
    data = b"".join(corpus.make_buffer(kinds[i % 4], 1 << 20, seed + i) for i in range(UNIT >> 20))
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = b"".join(co.compress(data[i:i + SECTION]) + co.flush(zlib.Z_FULL_FLUSH) for i in range(0, UNIT, SECTION))
    starts, at = [0], body.find(MARK)
    while at >= 0:
        starts.append(at + 4)
        at = body.find(MARK, at + 1)
    assert len(starts) == UNIT // SECTION + 1 and starts[-1] == len(body)
    return data, body, co.flush(), starts[:-1]


def build(unit, reps, every):
    """reps copies of the unit's sections and an empty final block under a zlib header and trailer, one
    section in `every` damaged (0: none).  Returns (stream, kept-section mask, sections, errors)."""
    data, body, tail, starts = unit
    nsec = reps * len(starts) + 1
    stream = bytearray(b"\x78\x01" + body * reps + tail)
    keep = [True] * nsec
    if every:
        for k in range(every // 2, nsec - 1, every):
            r, j = divmod(k, len(starts))
            at = 2 + r * len(body) + starts[j]
            stream[at:at + len(BAD_BLOCK)] = BAD_BLOCK
            keep[k] = False
    adler = zlib.adler32(data)
    for _ in range(reps - 1):
        adler = zlib.adler32(data, adler)
    stream += adler.to_bytes(4, "big")
    damaged = keep.count(False)
    return bytes(stream), keep, nsec, damaged + (1 if damaged else 0)


def upload(ip, stream):
    d_src = torch.zeros(ip.src_bytes, dtype=torch.uint8, device=DEV)
    d_src[:len(stream)] = torch.frombuffer(bytearray(stream), dtype=torch.uint8).to(DEV)
    return d_src


class Case:
    def __init__(self, name, stream, cap, want, nsec, errors, **kind):
        """cap: dest_len, the undamaged stream's output size (as a caller knows it); want: the output"""
        self.name, self.want, self.nsec, self.errors, self.kind = name, want, nsec, errors, kind
        self.n = len(stream)
        self.ip = zsc_amd.InflatePlan([len(stream)], [cap], **kind)
        self.d_src = upload(self.ip, stream)
        self.d_dst = torch.empty(self.ip.dst_bytes, dtype=torch.uint8, device=DEV)
        self.ms, self.ok = [], True

    def run(self, record=True):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.ip.run(self.d_src.data_ptr(), self.d_dst.data_ptr(), 0)
        lens, used, stat, kms = self.ip.results()
        wall = (time.perf_counter() - t0) * 1e3
        errs = self.ip.data_errors()
        secs = self.ip.sections()
        out = self.want.numel()
        ok = lens == [out] and used == [self.n] and stat == [-3 if self.errors else 0] and errs == [self.errors]
        ok = ok and secs == [self.nsec] and bool((self.d_dst[:out] == self.want).all())
        self.ok = self.ok and ok
        if record:
            self.ms.append((wall, kms))
        return ok

    def report(self):
        best_k = min(k for _, k in self.ms)
        best_w = min(w for w, _ in self.ms)
        out = self.want.numel()
        return {"ok": self.ok, "output_bytes": out, "compressed": self.n, "sections": self.nsec,
                "data_errors": self.errors, "kernel_ms": [round(k, 2) for _, k in self.ms],
                "wall_ms": [round(w, 2) for w, _ in self.ms], "GBps_out_kernel": round(out / best_k / 1e6, 3),
                "GBps_out_wall": round(out / best_w / 1e6, 4), "scratch_bytes": self.ip.scratch_bytes()}


T0 = time.perf_counter()


def log(msg):
    print(f"[{time.perf_counter() - T0:8.2f} s] {msg}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-serial", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"device": zsc_amd.device_info()}
    unit = unit_stream()
    log("unit ready")
    reps = (a.gib << 30) // UNIT
    d_unit = torch.frombuffer(bytearray(unit[0]), dtype=torch.uint8).to(DEV)
    clean = d_unit.repeat(reps)

    def want(keep):
        views = d_unit.view(-1, SECTION)
        per = views.shape[0]
        return torch.cat([views[k % per] for k in range(len(keep) - 1) if keep[k]])

    # one damaged 16 MiB unit through a resync plan first: a stream that would go serial (minutes at
    # 1 GiB) stops the probe here, in seconds
    s, keep, nsec, errs = build(unit, 1, 100)
    first = Case("unit_check", s, UNIT, want(keep), nsec, errs, resync=True)
    if not first.run(record=False):
        log(f"the damaged unit did not decode in parallel as constructed: sections {first.ip.sections()}")
        sys.exit(1)
    first.ip.close()
    log("damaged unit decoded in parallel")
    cases = []
    s, keep, nsec, errs = build(unit, reps, 0)
    cap = clean.numel()
    cases.append(Case("clean_sections", s, cap, clean, nsec, errs, sections=True))
    cases.append(Case("clean_resync", s, cap, clean, nsec, errs, resync=True))
    log("clean cases ready")
    for pct, every in ((1, 100), (10, 10)):
        s, keep, nsec, errs = build(unit, reps, every)
        cases.append(Case(f"damaged{pct}_resync", s, cap, want(keep), nsec, errs, resync=True))
        log(f"damaged{pct} ready")
    if not a.no_serial:
        s, keep, nsec, errs = build(unit, 1, 100)
        cases.append(Case("serial16_plain", s, UNIT, want(keep), 0, errs))
    del s
    for c in cases:
        log(f"warm-up {c.name}: {'ok' if c.run(record=False) else 'WRONG'}")
    for r in range(a.reps):
        for c in cases:
            c.run()
        log(f"round {r} done")
    for c in cases:
        res[c.name] = c.report()
        print(c.name, res[c.name], flush=True)
    base = res["clean_sections"]["GBps_out_kernel"]
    res["resync_clean_vs_sections"] = round(res["clean_resync"]["GBps_out_kernel"] / base, 3)
    res["damaged1_vs_clean_resync"] = round(res["damaged1_resync"]["GBps_out_kernel"] / res["clean_resync"]["GBps_out_kernel"], 3)
    if not a.no_serial:
        res["damaged1_resync_vs_serial_wall"] = round(res["damaged1_resync"]["GBps_out_wall"] /
                                                      res["serial16_plain"]["GBps_out_wall"], 1)
    print(json.dumps({k: v for k, v in res.items() if not isinstance(v, dict)}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if not all(c.ok for c in cases):
        sys.exit(1)


if __name__ == "__main__":
    main()
