"""The ZIP writer's kernels (zsc_amd/csrc/zip.h) on the lane emulation, against the format built in Python.

tests/emu_zip builds the kernel sources with -DZSC_WAVE_EMU into a stand-alone program at 64, 16 and 8 lanes; it
runs archive lengths -> scan -> part offsets -> move, as the runtime enqueues them.  No deflate is involved: the
result records and the slots' bytes are fabricated here, so every length is reachable (a body of 1 byte is a
stream of 19 bytes, whatever they are).  The expected images come from tests/zip_cases.py.

Every image is written twice, over 0xA5 and over 0x5A: both give the same [0, total) and leave what is behind
total as it was.  The cases whose bodies are real DEFLATE data (CPython's raw zlib, test data only) are then
opened by CPython's zipfile.  The same cases go once through the programs built with AddressSanitizer and UBSan
-- stand-alone, not loaded into python --, the image allocated at exactly its capacity, every slot at exactly
its length rounded up to 16 and the names at exactly their size.
"""
import io
import os
import random
import struct
import subprocess
import zipfile
import zlib

import pytest

from zip_cases import (DIR, END, END64, LOCAL, TILE, UTF8, Z_BUF_ERROR, Z_MEM_ERROR, Z_OK, expected, walk)

HERE = os.path.dirname(os.path.abspath(__file__))
LANES = (64, 16, 8)
PAD = 4096  # what emu_zip allocates behind the capacity
ST = {0: Z_OK, 1: Z_BUF_ERROR, 2: Z_MEM_ERROR}  # ZP_ST_*


def fab(body, seed, status=Z_OK):
    """(status, a stream whose body is `body` bytes long, None): any bytes"""
    return status, random.Random(seed).randbytes(body + 18), None


_real = {}


def real(data, level=6):
    """(Z_OK, the gzip stream of data with the plain 10-byte header, data)"""
    key = (bytes(data), level)
    if key not in _real:
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        body = c.compress(data) + c.flush()
        _real[key] = (b"\x1f\x8b\x08\0\0\0\0\0\0\x03" + body +
                      struct.pack("<II", zlib.crc32(data), len(data)))
    return Z_OK, _real[key], bytes(data)


def entry(item, name=b""):
    return name, item


class Case:
    """archives: lists of (name, (status, stream, input or None)); out_lens: {buffer: a fabricated out_len}"""

    def __init__(self, name, archives, align=1, short_by=0, flags=0, datetimes=None, out_lens=None):
        self.name, self.align, self.short_by, self.flags, self.datetimes = name, align, short_by, flags, datetimes
        self.first, self.items, self.names = [0], [], []
        for arch in archives:
            for nm, it in arch:
                self.names.append(nm)
                self.items.append(it)
            self.first.append(len(self.items))
        self.out_lens = [len(s) for _, s, _ in self.items]
        for i, n in (out_lens or {}).items():
            self.out_lens[i] = n
        self.real = all(d is not None for _, _, d in self.items)
        self.want = expected([s for _, s, _ in self.items], [st for st, _, _ in self.items], self.names, self.first,
                             align, datetimes, flags, self.out_lens)

    def record(self):
        count = len(self.items)
        r = [struct.pack("<6I", count, len(self.first) - 1, self.align, self.short_by, self.flags,
                         1 if self.datetimes is not None else 0),
             struct.pack(f"<{len(self.first)}I", *self.first)]
        offs = [0]
        for nm in self.names:
            offs.append(offs[-1] + len(nm))
        r.append(struct.pack(f"<{count + 1}Q", *offs))
        r += self.names
        if self.datetimes is not None:
            r.append(struct.pack(f"<{count}I", *self.datetimes))
        for (st, s, _), n in zip(self.items, self.out_lens):
            r.append(struct.pack("<iII", st, n, len(s)))
            r.append(s)
        return b"".join(r)


def hexname(j, n=5):
    return (b"%0" + str(n).encode() + b"x") % j


def big(entries, end_before_border, seed):
    """one archive of `entries` entries of 0 to 2 input bytes, real bodies, whose end records start
    end_before_border bytes before a tile border (the last entry's input is sized for that), and a small one"""
    arch = [entry(real(bytes([65 + j % 7] * (j % 3))), hexname(j)) for j in range(entries - 1)]
    size = sum(LOCAL + DIR + 2 * len(nm) + len(it[1]) - 18 for nm, it in arch) + LOCAL + DIR + 2 * 4
    want = (-(size + end_before_border)) % TILE  # the body length that puts the end there
    if want < 40:
        want += TILE
    # the last entry: one stored block (zlib's level 0, as test data), 5 bytes longer than its input
    last = entry(real(random.Random(seed).randbytes(want - 5), 0), b"last")
    assert len(last[1][1]) - 18 == want
    return [arch + [last], [entry(real(b"neighbour"), b"n")]]


_memo = []


def make_cases():
    """built once, changed by no one"""
    if _memo:
        return _memo
    cases = _memo
    # a local header that starts k bytes before a tile border, for every byte a header has
    for k in range(1, LOCAL):
        n0 = k % 7
        cases.append(Case(f"local-at-border-minus-{k}",
                          [[entry(fab(TILE - k - LOCAL - n0, k), b"a" * n0), entry(fab(100 + k, 50 + k), b"second")]],
                          (1, 16)[k % 2]))
    # the same for a directory record: one entry, the directory right behind it
    for k in range(1, DIR):
        n0 = k % 5
        cases.append(Case(f"dir-at-border-minus-{k}", [[entry(fab(TILE - k - LOCAL - n0, 100 + k), b"d" * n0)],
                                                       [entry(fab(40, k), b"x")]], (1, 16, 4096)[k % 3]))
    # ... and for the end record; an archive behind it, so the end's zeros are cut too
    for k in range(1, END):
        n0 = 3 + k % 4
        cases.append(Case(f"end-at-border-minus-{k}",
                          [[entry(fab(TILE - k - LOCAL - DIR - 2 * n0, 200 + k), b"e" * n0)], [entry(fab(40, k), b"y")]],
                          (1, 16, 4096)[k % 3]))
    # a name cut by a border; the name lengths around a granule and the longest (it spans four tiles)
    cases.append(Case("name-cut-by-border", [[entry(fab(TILE - 35 - LOCAL - 2, 1), b"ab"),
                                              entry(fab(77, 2), b"0123456789abcdefghij")]]))
    rnd = random.Random(7)
    lens = (0, 1, 15, 16, 17, 65535)
    cases.append(Case("name-lengths", [[entry(fab(50 + j, j), rnd.randbytes(n)) for j, n in enumerate(lens)],
                                       [entry(fab(33, 9), rnd.randbytes(65535))]], 16))
    # names on either side of the length up to which the header's lane writes them (128), some cut by a border
    around = (127, 128, 129, 300, 128, 129, 127)
    cases.append(Case("name-lengths-around-the-lane-limit",
                      [[entry(fab(40 + j, j), rnd.randbytes(n)) for j, n in enumerate(around)],
                       [entry(fab(TILE - 3 * (LOCAL + DIR) - 700 - 64 * j, 70 + j), rnd.randbytes(n))
                        for j, n in enumerate((129, 128, 200))]], 16))
    # names at every alignment in the blob (17 bytes each: every residue of 16), bodies at every phase of the image
    for blen in (1, 2, 15, 16, 17):
        cases.append(Case(f"body-{blen}-every-phase",
                          [[entry(fab(blen, 16 * blen + j), rnd.randbytes(17)) for j in range(16)] +
                           [entry(fab(blen, 400 + j), rnd.randbytes(j)) for j in range(16)]]))
    # empty archives: first, last, between others, two in a row, and nothing but
    e = []
    some = [e, [entry(fab(300, 1), b"one")], e, e, [entry(fab(5000, 2), b"two"), entry(fab(2, 3), b"")], e]
    cases.append(Case("empty-archives", some, 1))
    cases.append(Case("empty-archives-align-16", some, 16))
    cases.append(Case("only-empty-archives", [e, e, e], 4096))
    cases.append(Case("no-archives", [], 16))
    # an archive of 1 300 entries: both per-archive passes take more than two steps at 64 lanes
    cases.append(Case("1300-entries", [[entry(fab(40, 1), b"p")],
                                       [entry(fab(2 + (53 * j) % 900, j), hexname(j, j % 9)) for j in range(1300)],
                                       [entry(fab(40, 2), b"q")]], 16))
    # 1 100 archives: the scan of the archives goes past PK_SCAN_B
    cases.append(Case("1100-archives", [[entry(fab(2 + j % 40, j), hexname(j, 3))] if j % 97 else [] for j in range(1100)]))
    cases.append(Case("1100-archives-align-16", [[entry(fab(2 + j % 40, j), b"")] for j in range(1100)], 16))
    # a failed status in the first, a middle and the last buffer of an archive; the same without those archives
    def five(bad, seed):
        return [entry(fab(200 + 37 * j, seed + j, Z_BUF_ERROR if j == bad else Z_OK), hexname(seed + j)) for j in range(5)]

    sound = [five(None, 10), five(None, 30), five(None, 60)]
    for align in (1, 16):
        cases.append(Case(f"failed-status-align-{align}",
                          [sound[0], five(0, 20), sound[1], five(2, 40), five(4, 50), sound[2]], align))
        cases.append(Case(f"failed-status-without-align-{align}", sound, align))
    assert cases[-2].want["arch_statuses"] == [Z_OK, Z_BUF_ERROR, Z_OK, Z_BUF_ERROR, Z_BUF_ERROR, Z_OK]
    # a failed buffer whose record holds no length to speak of
    cases.append(Case("failed-status-wild-length", [[entry(fab(100, 1), b"a")], [entry((Z_BUF_ERROR, b"", None), b"b")],
                                                    [entry(fab(100, 2), b"c")]], 16))
    # an archive whose records sum past 4 294 967 295 bytes (no slot bytes: nothing of it may be read)
    huge = [entry((Z_OK, b"", None), hexname(j)) for j in range(5)]
    cases.append(Case("archive-past-4g", [[entry(fab(100, 1), b"a")], huge, [entry(fab(100, 2), b"c")]], 16,
                      out_lens={1 + j: 0x38000000 for j in range(5)}))
    assert cases[-1].want["arch_statuses"] == [Z_OK, Z_MEM_ERROR, Z_OK]
    # an image one byte longer than its capacity: nothing is written, the tables are filled
    cases.append(Case("cap-one-short", [[entry(fab(20000, 1), b"first"), entry(fab(300, 2), b"second")], e,
                                        [entry(fab(40000, 3), b"third")]], 16, short_by=1))
    # real bodies: zipfile reads these.  A per-buffer time and date and the UTF-8 flag; the name lengths again
    texts = [bytes(rnd.randrange(97, 105) for _ in range(n)) for n in (0, 1, 2, 100, 5000, 70000)]
    dts = [((1980 + j) - 1980 << 9 | (1 + j) << 5 | (2 + j)) << 16 | (j << 11 | (3 * j) << 5 | j) for j in range(8)]
    cases.append(Case("real-datetime-utf8",
                      [[entry(real(t), "näme%d".encode() % j) for j, t in enumerate(texts)],
                       [entry(real(b"x" * 17), "日本".encode()), entry(real(b""), b"empty")]], 16, flags=UTF8,
                      datetimes=dts))
    cases.append(Case("real-name-lengths",
                      [[entry(real(texts[j % 6], 1 + j), b"k" * n) for j, n in enumerate(lens)], e,
                       [entry(real(texts[4], 9), b"a/b/c.txt")]], 4096))
    # the ZIP64 threshold, the end records cut by a border in the ZIP64 record, the locator and the end record
    cases.append(Case("65534-entries", big(65534, 11, 1)))
    cases.append(Case("65535-entries", big(65535, 30, 2), 16))
    cases.append(Case("65536-entries", big(65536, 66, 3)))
    cases.append(Case("65535-entries-end-cut", big(65535, 85, 4), 4096))
    assert len({c.name for c in cases}) == len(cases)
    return cases


def run_emu(tmp_path, program, cases, exact=False):
    """[{total, launches, arch_off, arch_st, parts, alloc}] per case and pass"""
    cpath = os.path.join(str(tmp_path), "cases.bin")
    opath = os.path.join(str(tmp_path), "out.bin")
    if not os.path.exists(cpath):
        with open(cpath, "wb") as f:
            for c in cases:
                f.write(c.record())
    r = subprocess.run([os.path.join(HERE, "emu_zip", program), cpath, opath] + (["exact"] if exact else []),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-4000:]
    assert len(r.stdout.decode().split("\n")) == len(cases) + 1
    blob = memoryview(open(opath, "rb").read())
    at, res = 0, []
    for c in cases:
        passes = []
        for _ in range(1 if exact else 2):
            na = len(c.first) - 1
            np_ = 2 * len(c.items) + na + 1
            total, launches = struct.unpack_from("<2Q", blob, at)
            arch_off = list(struct.unpack_from(f"<{na + 1}Q", blob, at + 16))
            arch_st = list(struct.unpack_from(f"<{na}Q", blob, at + 16 + 8 * (na + 1)))
            parts = list(struct.unpack_from(f"<{np_}Q", blob, at + 16 + 8 * (2 * na + 1)))
            at += 16 + 8 * (2 * na + 1 + np_)
            n, = struct.unpack_from("<Q", blob, at)
            passes.append(dict(total=total, launches=launches, arch_off=arch_off, arch_st=arch_st, parts=parts,
                               alloc=bytes(blob[at + 8:at + 8 + n])))
            at += 8 + n
        res.append(passes)
    assert at == len(blob)
    return res


def check(c, passes, exact):
    w = c.want
    image = w["image"]
    for got, fill in zip(passes, (0xA5, 0x5A)):
        total, alloc = got["total"], got["alloc"]
        assert total == len(image), c.name
        assert got["arch_off"] == w["arch_offsets"], c.name
        assert [ST[s] for s in got["arch_st"]] == w["arch_statuses"], c.name
        assert got["parts"] == w["parts"], c.name
        assert got["launches"] == (1 if len(c.first) - 1 <= 1024 else 3), c.name
        cap = max(total - c.short_by, 0)
        assert len(alloc) == (cap if exact else cap + PAD), c.name
        if c.short_by:
            assert alloc == bytes([fill]) * len(alloc), c.name  # nothing at all
            continue
        if alloc[:total] != image:
            bad = next(x for x in range(total) if alloc[x] != image[x])
            raise AssertionError((c.name, "first wrong byte", bad, alloc[bad], image[bad]))
        assert alloc[total:] == bytes([fill]) * (len(alloc) - total), c.name


def archives_of(c, image):
    """the bytes of each sound archive"""
    w = c.want
    return [image[o:o + n] for o, n, s in zip(w["arch_offsets"], w["arch_lens"], w["arch_statuses"]) if s == Z_OK]


def test_the_case_set_is_what_its_names_say():
    """the reference side alone, before any kernel is asked"""
    by = {c.name: c for c in make_cases()}
    for k in range(1, LOCAL):
        assert by[f"local-at-border-minus-{k}"].want["entry_offsets"][1] == TILE - k
    for k in range(1, DIR):
        assert by[f"dir-at-border-minus-{k}"].want["dir_offsets"][0] == TILE - k
    for k in range(1, END):
        c = by[f"end-at-border-minus-{k}"]
        assert c.want["parts"][2] == TILE - k and c.want["arch_lens"][0] == TILE - k + END
    c = by["name-cut-by-border"]
    assert c.want["entry_offsets"][1] + LOCAL < TILE < c.want["data_offsets"][1]
    assert by["only-empty-archives"].want["arch_offsets"] == [0, 4096, 8192, 12288]
    assert by["only-empty-archives"].want["image"][:END] == b"PK\x05\x06" + b"\0" * 18
    assert by["no-archives"].want["image"] == b""
    for name, k, length in (("65534-entries", 11, END), ("65535-entries", 30, END64), ("65536-entries", 66, END64),
                            ("65535-entries-end-cut", 85, END64)):
        w = by[name].want
        end_at = w["arch_lens"][0] - length
        assert end_at % TILE == TILE - k, name
        assert (w["image"][end_at:end_at + 4] == b"PK\x06\x06") == (length == END64), name
    # the walker takes every sound archive of the reference side, and refuses one with a byte changed
    for c in make_cases():
        for data in archives_of(c, c.want["image"]):
            walk(data)
    data = bytearray(archives_of(by["empty-archives"], by["empty-archives"].want["image"])[1])
    data[26] ^= 1  # the local header's name length
    with pytest.raises(AssertionError):
        walk(bytes(data))


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_zip")], check=True)


@pytest.fixture(scope="module")
def images64(built, tmp_path_factory):
    cases = make_cases()
    return run_emu(tmp_path_factory.mktemp("zip64lanes"), "emu_zip64", cases)


@pytest.mark.parametrize("lanes", LANES)
def test_images_and_tables_are_the_formats(built, images64, tmp_path, lanes):
    cases = make_cases()
    res = images64 if lanes == 64 else run_emu(tmp_path, f"emu_zip{lanes}", cases)
    for c, passes in zip(cases, res):
        check(c, passes, exact=False)
        if not c.short_by:
            assert passes[0]["alloc"][:passes[0]["total"]] == passes[1]["alloc"][:passes[1]["total"]], c.name


def test_a_failed_archive_leaves_its_neighbours_what_they_are_without_it(images64):
    cases = make_cases()
    by = {c.name: (c, p) for c, p in zip(cases, images64)}
    for align in (1, 16):
        c, p = by[f"failed-status-align-{align}"]
        d, q = by[f"failed-status-without-align-{align}"]
        assert p[0]["total"] == q[0]["total"]
        assert archives_of(c, p[0]["alloc"]) == archives_of(d, q[0]["alloc"])
        assert p[0]["alloc"][:p[0]["total"]] == q[0]["alloc"][:q[0]["total"]]
    c, p = by["archive-past-4g"]
    assert [ST[s] for s in p[0]["arch_st"]] == [Z_OK, Z_MEM_ERROR, Z_OK]
    assert p[0]["arch_off"][1] == p[0]["arch_off"][2]  # no room taken


def test_zipfile_reads_every_image_of_real_bodies(images64):
    cases = make_cases()
    seen = 0
    for c, passes in zip(cases, images64):
        if not c.real or c.short_by:
            continue
        w = c.want
        for a, data in enumerate(archives_of(c, passes[0]["alloc"])):  # (every archive of a real case is sound)
            ids = range(c.first[a], c.first[a + 1])
            entries, doff = walk(data)
            assert doff == w["dir_offsets"][a] - w["arch_offsets"][a]
            with zipfile.ZipFile(io.BytesIO(data)) as z:
                assert z.testzip() is None, c.name
                infos = z.infolist()
                assert len(infos) == len(ids) == len(entries)
                step = 1 if len(ids) < 1000 else 251
                for k, (i, info, ent) in enumerate(zip(ids, infos, entries)):
                    _, s, src = c.items[i]
                    dt = c.datetimes[i] if c.datetimes is not None else 0x00210000
                    assert info.filename == c.names[i].decode("utf-8" if c.flags & UTF8 else "cp437"), c.name
                    assert (info.file_size, info.compress_size, info.CRC) == (len(src), len(s) - 18, zlib.crc32(src))
                    assert info.header_offset == w["entry_offsets"][i] - w["arch_offsets"][a] == ent["header_offset"]
                    assert info.date_time == ((dt >> 25) + 1980, dt >> 21 & 15, dt >> 16 & 31, dt >> 11 & 31,
                                              dt >> 5 & 63, 2 * (dt & 31))
                    assert (info.create_system, info.extract_version) == (0, 20)
                    assert bool(info.flag_bits & UTF8) == bool(c.flags & UTF8)
                    if k % step == 0:
                        assert z.read(info) == src, (c.name, i)
            seen += 1
    assert seen >= 12


@pytest.fixture(scope="module")
def built_san():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_zip"), "SAN=-fsanitize=address,undefined"], check=True)


@pytest.mark.parametrize("lanes", LANES)
def test_exact_allocations_under_the_sanitizers(built_san, tmp_path, lanes):
    """the programs of their own with AddressSanitizer and UBSan: no byte read outside a slot's granules or the
    names, none written outside the image"""
    cases = make_cases()
    for c, passes in zip(cases, run_emu(tmp_path, f"emu_zip{lanes}_san", cases, exact=True)):
        check(c, passes, exact=True)
