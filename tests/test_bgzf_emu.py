"""The BGZF writer's kernels (zsc_amd/csrc/bgzf.h) on the lane emulation, against the format built in Python.

tests/emu_bgzf builds the kernel sources with -DZSC_WAVE_EMU into a stand-alone program at 64, 16 and 8 lanes;
it runs file lengths -> scan -> member offsets -> move, as the runtime enqueues them.  No deflate is involved:
the result records and the slots' bytes are fabricated here, so every length is reachable (a member of L = 28
is a stream of 20 bytes, whatever they are).  The expected images come from tests/bgzf_cases.py.

Every image is written twice, over 0xA5 and over 0x5A: both give the same [0, total) and leave what is behind
total as it was.  The same cases then go once through the programs built with AddressSanitizer and UBSan --
stand-alone, not loaded into python --, the image allocated at exactly its capacity and every slot at exactly
its length rounded up to 16.
"""
import os
import random
import struct
import subprocess

import pytest

from bgzf_cases import TILE, Z_BUF_ERROR, Z_OK, expected

HERE = os.path.dirname(os.path.abspath(__file__))
LANES = (64, 16, 8)
PAD = 4096  # what emu_bgzf allocates behind the capacity


def fab(length, seed, status=Z_OK):
    """(status, a stream whose member is `length` bytes long): any bytes, XFL one of the reference's three"""
    rnd = random.Random(seed)
    s = bytearray(rnd.randbytes(length - 8))
    s[8] = (0, 2, 4)[seed % 3]
    return status, bytes(s)


class Case:
    def __init__(self, name, files, align=1, short_by=0):
        self.name, self.align, self.short_by = name, align, short_by
        self.first = [0]
        self.items = []
        for f in files:
            self.items += f
            self.first.append(len(self.items))
        self.want = expected([s for _, s in self.items], [st for st, _ in self.items], self.first, align)

    def record(self):
        r = struct.pack("<4I", len(self.items), len(self.first) - 1, self.align, self.short_by)
        r += struct.pack(f"<{len(self.first)}I", *self.first)
        for st, s in self.items:
            r += struct.pack("<iII", st, len(s), len(s)) + s
        return r


_memo = []


def make_cases():
    """built once, changed by no one"""
    if _memo:
        return _memo
    cases = _memo
    # a member header that starts k bytes before a tile border, for every byte a header has
    for k in range(1, 18):
        cases.append(Case(f"header-at-border-minus-{k}", [[fab(TILE - k, k), fab(100 + k, 50 + k)]], (1, 16)[k % 2]))
    # the same for a file's tail; a second file behind it, so the tail's zeros are cut too
    for k in range(1, 28):
        cases.append(Case(f"tail-at-border-minus-{k}", [[fab(TILE - k, 100 + k)], [fab(40, k)]], (1, 16, 4096)[k % 3]))
    # the shortest members and the longest, and one too long: its file fails, the others stay
    edge = [[fab(28, 1)], [fab(29, 2), fab(28, 3)], [fab(65535, 4)], [fab(65536, 5)], [fab(33, 6), fab(65537, 7)],
            [fab(65536, 8), fab(28, 9)]]
    for align in (1, 16, 4096):
        cases.append(Case(f"length-limits-align-{align}", edge, align))
    assert cases[-1].want[3] == [Z_OK] * 4 + [Z_BUF_ERROR, Z_OK]
    assert cases[-1].want[0][cases[-1].want[4][4] + 16:][:2] == b"\xff\xff"  # BSIZE of L = 65 536
    # a failed status in the first, a middle and the last buffer of a file
    def five(bad, seed):
        return [fab(200 + 37 * j, seed + j, Z_BUF_ERROR if j == bad else Z_OK) for j in range(5)]

    for align in (1, 16):
        cases.append(Case(f"failed-status-align-{align}",
                          [five(None, 10), five(0, 20), five(None, 30), five(2, 40), five(4, 50), five(None, 60)], align))
    assert cases[-1].want[3] == [Z_OK, Z_BUF_ERROR, Z_OK, Z_BUF_ERROR, Z_BUF_ERROR, Z_OK]
    # a failed buffer whose record holds no length to speak of
    cases.append(Case("failed-status-wild-length", [[fab(100, 1)], [(Z_BUF_ERROR, b"")], [fab(100, 2)]], 16))
    # empty files: first, last, between others, two in a row, and nothing but
    e = []
    cases.append(Case("empty-files", [e, [fab(300, 1)], e, e, [fab(5000, 2), fab(28, 3)], e], 1))
    cases.append(Case("empty-files-align-16", [e, [fab(300, 1)], e, e, [fab(5000, 2), fab(28, 3)], e], 16))
    cases.append(Case("only-empty-files", [e, e, e], 4096))
    cases.append(Case("no-files", [], 16))
    # a file of 130 members: the scan inside the file takes more than two steps at 64 lanes
    cases.append(Case("130-members", [[fab(40, 1)], [fab(28 + (53 * j) % 900, j) for j in range(130)], [fab(40, 2)]], 16))
    # 1 100 one-member files: the scan of the files goes past PK_SCAN_B
    cases.append(Case("1100-files", [[fab(28 + j % 40, j)] if j % 97 else [] for j in range(1100)], 1))
    cases.append(Case("1100-files-align-16", [[fab(28 + j % 40, j)] for j in range(1100)], 16))
    # an image one byte longer than its capacity: nothing is written, the tables are filled
    cases.append(Case("cap-one-short", [[fab(20000, 1), fab(300, 2)], e, [fab(40000, 3)]], 16, short_by=1))
    assert len({c.name for c in cases}) == len(cases)
    return cases


def run_emu(tmp_path, program, cases, exact=False):
    """[(total, launches, file_off, parts, image allocation)] per case and pass"""
    cpath = os.path.join(str(tmp_path), "cases.bin")
    opath = os.path.join(str(tmp_path), "out.bin")
    if not os.path.exists(cpath):
        with open(cpath, "wb") as f:
            for c in cases:
                f.write(c.record())
    r = subprocess.run([os.path.join(HERE, "emu_bgzf", program), cpath, opath] + (["exact"] if exact else []),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-4000:]
    assert len(r.stdout.decode().split("\n")) == len(cases) + 1
    blob = memoryview(open(opath, "rb").read())
    at, res = 0, []
    for c in cases:
        passes = []
        for _ in range(1 if exact else 2):
            nf, np_ = len(c.first), len(c.items) + len(c.first)
            total, launches = struct.unpack_from("<2Q", blob, at)
            file_off = list(struct.unpack_from(f"<{nf}Q", blob, at + 16))
            parts = list(struct.unpack_from(f"<{np_}Q", blob, at + 16 + 8 * nf))
            at += 16 + 8 * (nf + np_)
            n, = struct.unpack_from("<Q", blob, at)
            passes.append((total, launches, file_off, parts, bytes(blob[at + 8:at + 8 + n])))
            at += 8 + n
        res.append(passes)
    assert at == len(blob)
    return res


def check(c, passes, exact):
    image, file_off, _, _, _, parts = c.want
    for (total, launches, got_off, got_parts, alloc), fill in zip(passes, (0xA5, 0x5A)):
        assert total == len(image), c.name
        assert got_off == file_off, c.name
        assert got_parts == parts, c.name
        nfiles = len(c.first) - 1
        assert launches == (1 if nfiles <= 1024 else 3), c.name
        cap = max(total - c.short_by, 0)
        assert len(alloc) == (cap if exact else cap + PAD), c.name
        if c.short_by:
            assert alloc == bytes([fill]) * len(alloc), c.name  # nothing at all
            continue
        if alloc[:total] != image:
            bad = next(x for x in range(total) if alloc[x] != image[x])
            raise AssertionError((c.name, "first wrong byte", bad, alloc[bad], image[bad]))
        assert alloc[total:] == bytes([fill]) * (len(alloc) - total), c.name


def test_the_case_set_is_what_its_names_say():
    """the reference side alone, before any kernel is asked"""
    by = {c.name: c for c in make_cases()}
    for k in range(1, 18):
        assert by[f"header-at-border-minus-{k}"].want[4][1] == TILE - k
    for k in range(1, 28):
        c = by[f"tail-at-border-minus-{k}"]
        assert c.want[5][1] == TILE - k and c.want[2][0] == TILE - k + 28
    assert by["1100-files"].want[1][-1] == len(by["1100-files"].want[0])
    assert by["only-empty-files"].want[1] == [0, 4096, 8192, 12288]
    assert by["no-files"].want[0] == b""
    import gzip
    sound = by["empty-files"]
    assert sound.want[0].count(b"\x1f\x8b\x08\x04") >= 9 and gzip.decompress(sound.want[0][-28:]) == b""


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_bgzf")], check=True)


@pytest.mark.parametrize("lanes", LANES)
def test_images_and_tables_are_the_formats(built, tmp_path, lanes):
    cases = make_cases()
    for c, passes in zip(cases, run_emu(tmp_path, f"emu_bgzf{lanes}", cases)):
        check(c, passes, exact=False)
        if not c.short_by:
            assert passes[0][4][:passes[0][0]] == passes[1][4][:passes[1][0]], c.name


@pytest.fixture(scope="module")
def built_san():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_bgzf"), "SAN=-fsanitize=address,undefined"], check=True)


@pytest.mark.parametrize("lanes", LANES)
def test_exact_allocations_under_the_sanitizers(built_san, tmp_path, lanes):
    """the programs of their own with AddressSanitizer and UBSan: no byte read outside a slot's granules, none
    written outside the image"""
    cases = make_cases()
    for c, passes in zip(cases, run_emu(tmp_path, f"emu_bgzf{lanes}_san", cases, exact=True)):
        check(c, passes, exact=True)
