"""BGZF files, their indexes and range requests for the BGZF index and the ranges plan (include/zsc_hip.h,
"BGZF ranges"; zsc_amd/csrc/bgzf_read.h), with the right answers.

Shared by tests/test_bgzf_read_emu.py (the lane emulation) and tests/test_gpu_bgzf_read.py (the MI355X).  Nothing
here asks the code under test anything: a table is the walk over BSIZE fields (bgzf_cases.walk_bsize on a clean
file; claim_walk, the contract's own rule restated, on every file), and bytes are CPython's gzip.decompress of the
file, sliced.  The members are CPython-written deflate streams in bgzf_cases.member's header.
"""
import gzip
import struct
import zlib
from collections import namedtuple

from bgzf_cases import BGZF_EOF, member, walk_bsize

Z_OK, Z_STREAM_ERROR, Z_DATA_ERROR, Z_BUF_ERROR = 0, -2, -3, -5
MAX_ISIZE = 65536


def _bytes(n, seed):
    """n bytes that deflate into literals and matches (level 6: dynamic blocks), cheap to make"""
    out = bytearray()
    x = seed * 2654435761 & 0xffffffff
    while len(out) < n:
        x = (x * 1103515245 + 12345) & 0xffffffff
        out += b"the quick brown fox %08x jumps over %d lazy dogs; " % (x, x % 97)
    return bytes(out[:n])


def gz(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    """a gzip stream with the plain 10-byte header, as CPython writes it"""
    c = zlib.compressobj(level, zlib.DEFLATED, 31, 8, strategy)
    s = c.compress(data) + c.flush()
    assert s[3] == 0 and len(s) >= 18
    return s


def stored(data):
    return member(gz(data, 0))


def fixed(data):
    return member(gz(data, 6, zlib.Z_FIXED))


def dynamic(data):
    return member(gz(data, 6))


def foreign_first(data):
    """a member whose FEXTRA holds another subfield in front of `BC`"""
    s = gz(data, 6)
    extra_front = b"XY\x03\0abc"
    length = 12 + len(extra_front) + 6 + len(s) - 10
    return (b"\x1f\x8b\x08\x04\0\0\0\0" + s[8:9] + b"\xff" + struct.pack("<H", len(extra_front) + 6) + extra_front +
            b"BC\x02\0" + struct.pack("<H", length - 1) + s[10:])


def claim(data, at):
    """the contract's rule at offset `at`: (stop, length) of the member the header claims, or None"""
    n = len(data)
    if at > n or n - at < 20:
        return None
    b = data[at:]
    if b[0] != 0x1f or b[1] != 0x8b or b[2] != 8 or (b[3] & 0xe4) != 4:
        return None
    end = 12 + (b[10] | b[11] << 8)
    if end > n - at:
        return None
    p = 12
    while p + 4 <= end:
        slen = b[p + 2] | b[p + 3] << 8
        if slen > end - p - 4:
            return None
        if b[p:p + 2] == b"BC" and slen == 2:
            total = (b[p + 4] | b[p + 5] << 8) + 1
            if total < end + 8 or total > n - at:
                return None
            isize = struct.unpack_from("<I", b, total - 4)[0]
            if isize > MAX_ISIZE:
                return None
            return at + total, isize
        p += 4 + slen
    return None


def claim_walk(data):
    """(coffsets, uoffsets), members + 1 entries each"""
    at = out = 0
    coff, uoff = [], []
    while True:
        c = claim(data, at)
        if c is None:
            break
        coff.append(at)
        uoff.append(out)
        at, out = c[0], out + c[1]
    return coff + [at], uoff + [out]


def member_bytes(data, coff, uoff):
    """per member of a table: its output, or None where CPython does not decode it to the claimed length"""
    outs = []
    for k in range(len(coff) - 1):
        try:
            d = zlib.decompressobj(31)
            got = d.decompress(data[coff[k]:coff[k + 1]])
            ok = d.eof and d.unused_data == b"" and len(got) == uoff[k + 1] - uoff[k]
        except zlib.error:
            ok = False
        outs.append(got if ok else None)
    return outs


File = namedtuple("File", "name data coff uoff outs clean")


def _file(name, data, clean=True, plain_headers=True):
    coff, uoff = claim_walk(data)
    outs = member_bytes(data, coff, uoff)
    if clean:
        # the two references agree: the members by BSIZE alone, and CPython's decode of the indexed bytes
        assert all(o is not None for o in outs), name
        body = data[:coff[-1]]
        if body.endswith(BGZF_EOF) and plain_headers:
            assert [a for a, _ in walk_bsize(body)] == coff[:-1], name
        assert b"".join(outs) == (gzip.decompress(body) if body else b""), name
    return File(name, data, coff, uoff, outs, clean)


SIZES = [0, 1, 15, 16, 17, 511, 512, 513, 65280, 65536]


def sizes_file():
    """members of every output length that matters, in stored, fixed and dynamic blocks, the 28-byte EOF member
    in the middle (as `cat` leaves it) and at the end"""
    parts = []
    for i, n in enumerate(SIZES):
        d = _bytes(n, 100 + i)
        parts.append((stored, fixed, dynamic)[i % 3](d) if n <= 65280 else dynamic(d))
        if n == 17:
            parts.append(BGZF_EOF)
    parts += [fixed(_bytes(513, 3)), stored(_bytes(511, 4)), BGZF_EOF]
    return b"".join(parts)


def nested_file():
    """a BGZF file stored at level 0 inside a BGZF member: its headers are candidates off the chain"""
    inner = dynamic(_bytes(700, 21)) + fixed(_bytes(40, 22)) + BGZF_EOF
    return dynamic(_bytes(100, 23)) + stored(inner) + dynamic(_bytes(200, 24)) + BGZF_EOF


def index_files():
    """every file the index tests look at, the damaged ones included (their tables are the walk's all the same)"""
    base = dynamic(_bytes(3000, 31)) + fixed(_bytes(100, 32)) + stored(_bytes(1000, 33)) + BGZF_EOF
    k = len(dynamic(_bytes(3000, 31)))
    altered = bytearray(base)
    altered[k + 16] ^= 0x01  # the second member's BSIZE
    return [
        _file("sizes", sizes_file()),
        _file("one", dynamic(_bytes(5000, 41))),
        # (walk_bsize knows the 18-byte header only)
        _file("foreign", stored(_bytes(50, 42)) + foreign_first(_bytes(300, 7)) + fixed(_bytes(20, 43)) + BGZF_EOF,
              plain_headers=False),
        _file("eof-only", BGZF_EOF),
        _file("empty", b""),
        _file("plain-gzip", gz(_bytes(2000, 51)) + gz(_bytes(300, 52)), clean=True),
        _file("garbage", base + b"\x1f\x8b\x08\x04 not a member at all " * 3),
        _file("padded", base + b"\0" * 100),
        _file("bsize-altered", bytes(altered), clean=False),
        _file("nested", nested_file()),
        # more candidate headers than a members plan gives a file room for (source_len / 16 + 8): the file has no
        # candidate records and is walked header by header
        _file("magic-dense", fixed(_bytes(30, 91)) + stored(b"\x1f\x8b\x08\x00" * 600) + dynamic(_bytes(900, 92)) +
              BGZF_EOF),
    ]


def range_files():
    """the files the range requests go to"""
    fs = index_files()
    return [f for f in fs if f.name in ("sizes", "one", "foreign", "nested", "padded", "magic-dense")]


def tiles_file():
    """(file, content): a few hundred KiB in members of many sizes, one of bgzip's 65 280 bytes, for the tiling
    equivalence (tiles of one byte decode a member once per byte of it: most members are kept short)"""
    cuts = [8000, 1000, 7, 12000, 4096] * 8 + [65280, 513]
    data = _bytes(sum(cuts), 61)
    parts, at = [], 0
    for i, n in enumerate(cuts):
        parts.append((dynamic, fixed, dynamic, stored)[i % 4](data[at:at + n]))
        at += n
    return b"".join(parts) + BGZF_EOF, data


Request = namedtuple("Request", "file begin length cap")


def requests_for(fi, f):
    """the requests of one file (index fi): (Request, ...)"""
    total = f.uoff[-1]
    bounds = sorted(set(f.uoff))
    spans = set()
    for i, b in enumerate(bounds):
        nb = bounds[i + 1] if i + 1 < len(bounds) else total
        for begin in (b - 1, b, b + 1):
            for end in (b - 1, b, b + 1, nb - 1, nb, nb + 1):
                if 0 <= begin < end:
                    spans.add((begin, end - begin))
    for k in range(len(f.coff) - 1):
        u0, u1 = f.uoff[k], f.uoff[k + 1]
        spans.add((u0, u1 - u0))                        # exactly one member (an empty one: length 0)
        if u1 - u0 >= 3:
            spans.add((u0 + 1, u1 - u0 - 2))            # strictly inside one member
            spans.add((u0 + (u1 - u0) // 3, 1))
        if u1 == u0 and u0 > 0 and u1 < total:
            spans.add((u0 - 1, 2))                      # across an empty member
            spans.add((0, total))
    spans |= {(0, total), (max(total - 1, 0), 1), (total // 2, 0), (total, 5), (total + 7, 5), (total + 7, 0),
              (max(total - 3, 0), 1000), (0, 1 << 40), (1 << 40, 1 << 40)}
    reqs = []
    for begin, length in sorted(spans):
        clipped = max(0, min(begin + length, total) - min(begin, total))
        reqs.append(Request(fi, begin, length, clipped))
    # capacities: one below the clipped length, 0, and more than it (the tail must stay untouched)
    reqs += [Request(fi, 0, total, max(total - 1, 0)), Request(fi, 0, total, 0), Request(fi, total, 9, 0),
             Request(fi, 1, 700, 699), Request(fi, 1, 700, 1000), Request(fi, 0, 10, 4096)]
    # two requests over the same members
    reqs += [Request(fi, 2, 600, 600), Request(fi, 2, 600, 600)]
    return reqs


def expected(f, r):
    """(status, dest_len, consumed, bytes or None) of request r against file f by the index's coordinates"""
    total = f.uoff[-1]
    b = min(r.begin, total)
    e = min(r.begin + r.length, total)
    if e <= b:
        return Z_OK, 0, 0, b""
    if e - b > r.cap:
        return Z_BUF_ERROR, e - b, 0, None
    out, last = bytearray(), 0
    for k in range(len(f.coff) - 1):
        u0, u1 = f.uoff[k], f.uoff[k + 1]
        if u1 == u0 or u1 <= b or u0 >= e:
            continue
        if f.outs[k] is None:
            return Z_DATA_ERROR, 0, 0, None
        out += f.outs[k][max(b, u0) - u0:min(e, u1) - u0]
        last = f.coff[k + 1]
    return Z_OK, e - b, last, bytes(out)


def to_voffset(f, u):
    """uncompressed offset -> virtual offset by the table: the member that holds the byte; total_out: the end"""
    if u >= f.uoff[-1]:
        assert u == f.uoff[-1]
        return f.coff[-1] << 16
    k = max(i for i in range(len(f.coff) - 1) if f.uoff[i] <= u)
    return f.coff[k] << 16 | (u - f.uoff[k])


def gzi(f):
    """the .gzi image of a file's table"""
    n = max(len(f.coff) - 2, 0)
    return struct.pack("<Q", n) + b"".join(struct.pack("<QQ", f.coff[k + 1], f.uoff[k + 1]) for k in range(n))


def damage_cases():
    """[(name, file as indexed, flips applied after indexing [(pos, xor)], file as read, index tables)]: a flipped
    byte in one member's deflate data, CRC-32 or ISIZE with the index built after the flip, and a BSIZE flipped
    after the index was built"""
    parts = [dynamic(_bytes(3000, 71)), fixed(_bytes(600, 72)), dynamic(_bytes(65280, 73)), stored(_bytes(900, 74)),
             BGZF_EOF]
    base = b"".join(parts)
    at = [0]
    for p in parts:
        at.append(at[-1] + len(p))
    cases = []
    for name, pos in (("data", at[2] + 18 + 200), ("crc", at[3] - 8), ("isize", at[3] - 4)):
        d = bytearray(base)
        d[pos] ^= 0x10
        cases.append((name, bytes(d), [], _file("damage-" + name, bytes(d), clean=False)))
    late = bytearray(base)
    late[at[1] + 16] ^= 0x02  # the second member's BSIZE, after the index was built
    fi = _file("damage-bsize-late", base)
    outs = list(fi.outs)
    outs[1] = None  # its own claim disagrees with the index
    cases.append(("bsize-late", base, [(at[1] + 16, 0x02)], fi._replace(outs=outs)))
    return cases
