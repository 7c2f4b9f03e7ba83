"""The BGZF index and the ranges plan (zsc_amd/csrc/bgzf_read.h, bgzf_read_host.h) on the lane emulation, at 64,
16 and 8 lanes: tests/emu_bgzf_read runs the kernels' own source step by step as the runtime enqueues it, over the
cases of tests/bgzf_read_cases.py, whose right answers are the walk over BSIZE fields and CPython's
gzip.decompress, sliced.  The sanitizer build runs as the stand-alone program it is.
"""
import os
import struct
import subprocess

import pytest

import bgzf_read_cases as bc
from bgzf_read_cases import Z_BUF_ERROR, Z_DATA_ERROR, Z_OK, Request

HERE = os.path.dirname(os.path.abspath(__file__))
LANES = [64, 16, 8]


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_bgzf_read")], check=True)


@pytest.fixture(scope="module")
def built_san():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_bgzf_read"), "SAN=-fsanitize=address,undefined"],
                   check=True)


def run_emu(tmp_path, prog, files, requests=(), gzis=(), flips=(), flags=0, pool=0):
    """one run of the program: {"index": [(members, indexed, total, coff, uoff)], "vo": [[(u, ok, v, ok2, back)]],
    "gzihex": [bytes], "gzi": [(rc, coff, uoff)], "plan": (rc, jobs, edges, decoded), "req": [(status, dest_len,
    consumed, canaries, tail, bytes)]}"""
    case = struct.pack("<II", pool, len(files))
    for d in files:
        case += struct.pack("<I", len(d)) + d
    case += struct.pack("<I", len(gzis))
    for f, image in gzis:
        case += struct.pack("<II", f, len(image)) + image
    case += struct.pack("<I", len(flips))
    for f, pos, x in flips:
        case += struct.pack("<III", f, pos, x)
    case += struct.pack("<II", flags, len(requests))
    for r in requests:
        case += struct.pack("<IQQI", r.file, r.begin, r.length, r.cap)
    cpath, opath = tmp_path / "case.bin", tmp_path / "out.bin"
    cpath.write_bytes(case)
    p = subprocess.run([os.path.join(HERE, "emu_bgzf_read", prog), str(cpath), str(opath)], capture_output=True,
                       text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.split("\n")
    blob = opath.read_bytes()
    res = {"index": [], "vo": [], "gzihex": [], "gzi": [], "plan": None, "req": []}
    k = at = 0

    def table(n):
        nonlocal k
        rows = [tuple(int(x) for x in lines[k + j].split()) for j in range(n)]
        k += n
        return [r[0] for r in rows], [r[1] for r in rows]

    while k < len(lines):
        w = lines[k].split()
        k += 1
        if not w:
            continue
        if w[0] == "index":
            coff, uoff = table(int(w[2]) + 1)
            res["index"].append((int(w[2]), int(w[3]), int(w[4]), coff, uoff))
            res["vo"].append([])
        elif w[0] == "vo":
            res["vo"][-1].append(tuple(int(x) for x in w[1:]))
        elif w[0] == "gzihex":
            res["gzihex"].append(bytes.fromhex(w[1]))
        elif w[0] == "gzi":
            coff, uoff = table(int(w[2]) + 1) if int(w[1]) == 0 else ([], [])
            res["gzi"].append((int(w[1]), coff, uoff))
        elif w[0] == "plan":
            res["plan"] = tuple(int(x) for x in w[1:])
        elif w[0] == "req":
            st, n = int(w[1]), int(w[2])
            out = None
            if st == 0:
                out = blob[at:at + n]
                at += n
            res["req"].append((st, n, int(w[3]), int(w[4]), int(w[5]), out))
    assert at == len(blob)
    return res


def check_requests(files, requests, got, where=""):
    assert len(got) == len(requests)
    for r, g in zip(requests, got):
        st, n, used, data = bc.expected(files[r.file], r)
        assert g[3] == 1, (where, r, "a canary around the destination was written")
        assert g[4] == 1, (where, r, "bytes behind dest_len were written")
        assert g[:3] == (st, n, used), (where, files[r.file].name, r, g[:3], (st, n, used))
        if st == Z_OK:
            assert g[5] == data, (where, files[r.file].name, r)


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("pool", [0, 1])
def test_index_equals_the_walk(built, tmp_path, lanes, pool):
    """pool 1: no file gets candidate records, so every file is walked header by header instead of chained"""
    files = bc.index_files()
    res = run_emu(tmp_path, f"emu_bgzf_read{lanes}", [f.data for f in files], pool=pool)
    by = {}
    for f, (members, indexed, total, coff, uoff), vo, image in zip(files, res["index"], res["vo"], res["gzihex"]):
        assert (coff, uoff) == (f.coff, f.uoff), f.name
        assert (members, indexed, total) == (len(f.coff) - 1, f.coff[-1], f.uoff[-1]), f.name
        assert image == bc.gzi(f), f.name
        for u, ok, v, ok2, back in vo:
            if u > f.uoff[-1]:
                assert ok == 0, (f.name, u)
            else:
                assert (ok, v, ok2, back) == (1, bc.to_voffset(f, u), 1, u), (f.name, u)
        by[f.name] = f
    assert len(by["plain-gzip"].coff) == 1 and len(by["empty"].coff) == 1  # no members, and no error
    base_len = len(by["padded"].data) - 100
    assert by["garbage"].coff[-1] == by["padded"].coff[-1] == base_len     # the index ends where the walk ends
    assert len(by["bsize-altered"].coff) - 1 == 1                          # ... in front of the altered member
    assert len(by["nested"].coff) - 1 == 4                                 # the inner headers are not members
    assert by["nested"].data.count(b"\x1f\x8b\x08\x04") == 4 + 3
    lens = [u1 - u0 for u0, u1 in zip(by["sizes"].uoff, by["sizes"].uoff[1:])]
    assert set(bc.SIZES) <= set(lens) and lens.count(0) == 3  # (the empty member, the tail in the middle and at the end)
    assert len(by["foreign"].coff) - 1 == 4


@pytest.mark.parametrize("lanes", LANES)
def test_gzi_import_is_the_built_index_or_refused(built, tmp_path, lanes):
    files = bc.index_files()
    sizes = next(i for i, f in enumerate(files) if f.name == "sizes")
    padded = next(i for i, f in enumerate(files) if f.name == "padded")
    good = [(i, bc.gzi(f)) for i, f in enumerate(files)]
    image = bc.gzi(files[sizes])
    n = struct.unpack_from("<Q", image)[0]
    moved = bytearray(image)
    moved[8 + 16 * 3] ^= 1                                   # one entry's compressed offset moved by a byte
    moved_u = bytearray(image)
    moved_u[16 + 16 * 3] ^= 1                                # ... its uncompressed offset
    left_out = struct.pack("<Q", n - 1) + image[8:8 + 16 * 4] + image[8 + 16 * 5:]
    tail_short = struct.pack("<Q", n - 2) + image[8:8 + 16 * (n - 2)]  # the last entries left to the walk
    bad = [(sizes, bytes(moved)), (sizes, bytes(moved_u)), (sizes, left_out), (padded, image), (sizes, image[:-1]),
           (sizes, b""), (sizes, struct.pack("<Q", 1 << 60))]
    res = run_emu(tmp_path, f"emu_bgzf_read{lanes}", [f.data for f in files], gzis=good + [(sizes, tail_short)] + bad)
    for (i, _), (rc, coff, uoff) in zip(good + [(sizes, tail_short)], res["gzi"]):
        assert (rc, coff, uoff) == (0, files[i].coff, files[i].uoff), files[i].name
    for k, (rc, _, _) in enumerate(res["gzi"][len(good) + 1:]):
        assert rc == Z_DATA_ERROR, k


def all_requests(files):
    reqs = []
    for i, f in enumerate(files):
        reqs += bc.requests_for(i, f)
    # mixed over the files, not file by file
    return reqs[::3] + reqs[1::3] + reqs[2::3]


@pytest.mark.parametrize("lanes", LANES)
def test_ranges_in_one_plan(built, tmp_path, lanes):
    files = bc.range_files()
    reqs = all_requests(files)
    res = run_emu(tmp_path, f"emu_bgzf_read{lanes}", [f.data for f in files], reqs)
    rc, jobs, edges, decoded = res["plan"]
    assert rc == 0 and edges > 100 and jobs > edges  # one staging slot, reused by every edge job
    check_requests(files, reqs, res["req"])
    kinds = {bc.expected(files[r.file], r)[0] for r in reqs}
    assert kinds == {Z_OK, Z_BUF_ERROR}


def voffset_requests(files, reqs):
    out = []
    for r in reqs:
        f = files[r.file]
        total = f.uoff[-1]
        if r.begin + r.length <= total:
            out.append(Request(r.file, bc.to_voffset(f, r.begin), bc.to_voffset(f, r.begin + r.length), r.cap))
    return out


@pytest.mark.parametrize("lanes", LANES)
def test_ranges_by_virtual_offsets(built, tmp_path, lanes):
    files = bc.range_files()
    plain = [r for r in all_requests(files) if r.begin + r.length <= files[r.file].uoff[-1]]
    assert len(plain) > 200
    res = run_emu(tmp_path, f"emu_bgzf_read{lanes}", [f.data for f in files], voffset_requests(files, plain), flags=1)
    assert res["plan"][0] == 0
    check_requests(files, plain, res["req"])
    f = files[0]
    k = next(k for k in range(len(f.coff) - 1) if f.uoff[k + 1] - f.uoff[k] == 15)
    ok = Request(0, f.coff[k] << 16, f.coff[k] << 16 | 15, 15)
    for bad in (Request(0, (f.coff[k] + 1) << 16, f.coff[k + 1] << 16, 99),  # no member start
                Request(0, f.coff[k] << 16, f.coff[k] << 16 | 16, 99),       # beyond the member's length
                Request(0, f.coff[-1] << 16 | 1, f.coff[-1] << 16 | 1, 99),  # within the end entry
                Request(0, f.coff[k] << 16 | 5, f.coff[k] << 16 | 4, 99),    # end < begin
                Request(0, f.coff[k + 1] << 16, f.coff[k] << 16, 99)):
        res = run_emu(tmp_path, f"emu_bgzf_read{lanes}", [f.data for f in files], [ok, bad], flags=1)
        assert res["plan"][0] == bc.Z_STREAM_ERROR, bad
    res = run_emu(tmp_path, f"emu_bgzf_read{lanes}", [f.data for f in files], [ok], flags=1)
    assert res["plan"][0] == 0 and res["req"][0][:3] == (0, 15, f.coff[k + 1])


@pytest.mark.parametrize("lanes", LANES)
def test_damage_fails_only_the_requests_that_touch_it(built, tmp_path, lanes):
    for name, data, flips, f in bc.damage_cases():
        reqs = bc.requests_for(0, f)
        res = run_emu(tmp_path, f"emu_bgzf_read{lanes}", [data], reqs, flips=[(0, p, x) for p, x in flips])
        index = res["index"][0]
        assert (index[3], index[4]) == (f.coff, f.uoff), name
        check_requests([f], reqs, res["req"], name)
        kinds = [bc.expected(f, r)[0] for r in reqs]
        assert kinds.count(Z_DATA_ERROR) > 10 and kinds.count(Z_OK) > 10, name


@pytest.mark.parametrize("lanes", LANES)
def test_exact_allocations_under_the_sanitizers(built_san, tmp_path, lanes):
    """the programs of their own with AddressSanitizer and UBSan, over tables, staging slot and destinations of
    exactly the sizes the runtime gives them: the index of every file by chain and by walk, an import, and the
    damaged files' requests"""
    files = bc.index_files()
    for pool in (0, 1):
        res = run_emu(tmp_path, f"emu_bgzf_read{lanes}_san", [f.data for f in files], pool=pool,
                      gzis=[(i, bc.gzi(f)) for i, f in enumerate(files)])
        assert [(x[3], x[4]) for x in res["index"]] == [(f.coff, f.uoff) for f in files]
        assert [g[0] for g in res["gzi"]] == [0] * len(files)
    files = bc.range_files()[1:]
    reqs = all_requests(files)
    res = run_emu(tmp_path, f"emu_bgzf_read{lanes}_san", [f.data for f in files], reqs)
    check_requests(files, reqs, res["req"])
    name, data, flips, f = bc.damage_cases()[0]
    reqs = bc.requests_for(0, f)[::4]
    res = run_emu(tmp_path, f"emu_bgzf_read{lanes}_san", [data], reqs)
    check_requests([f], reqs, res["req"], name)
