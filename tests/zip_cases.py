"""The ZIP archive format of include/zsc_hip.h ("ZIP archives") restated in Python: what the writer must give.

Shared by tests/test_zip_emu.py and tests/test_gpu_zip.py.  Nothing here asks the code under test anything.
"""
import struct

Z_OK, Z_STREAM_ERROR, Z_MEM_ERROR, Z_BUF_ERROR = 0, -2, -4, -5
TILE = 16384
LOCAL, DIR, END, END64 = 30, 46, 22, 98
ZIP64_AT = 65535
MAX_ARCHIVE = 0xFFFFFFFF
NO_DATETIME = 0x00210000
UTF8 = 0x0800


def round_up(v, align):
    return (v + align - 1) // align * align


def end_len(entries):
    return END64 if entries >= ZIP64_AT else END


def local_header(flags, dt, crc, csize, usize, n):
    return struct.pack("<4sHHHHHIIIHH", b"PK\x03\x04", 20, flags, 8, dt & 0xFFFF, dt >> 16, crc, csize, usize, n, 0)


def dir_record(flags, dt, crc, csize, usize, n, offset):
    return struct.pack("<4sHHHHHHIIIHHHHHII", b"PK\x01\x02", 20, 20, flags, 8, dt & 0xFFFF, dt >> 16, crc, csize,
                       usize, n, 0, 0, 0, 0, 0, offset)


def end_records(entries, dsize, doff):
    out = b""
    if entries >= ZIP64_AT:
        out += struct.pack("<4sQHHIIQQQQ", b"PK\x06\x06", 44, 45, 45, 0, 0, entries, entries, dsize, doff)
        out += struct.pack("<4sIQI", b"PK\x06\x07", 0, doff + dsize, 1)
    return out + struct.pack("<4sHHHHIIH", b"PK\x05\x06", 0, 0, min(entries, 0xFFFF), min(entries, 0xFFFF), dsize,
                             doff, 0)


def expected(streams, statuses, names, arch_first, align=1, datetimes=None, flags=0, out_lens=None):
    """The image and its tables from the plan's gzip streams (a body is stream[10:-8], CRC-32 and the size are
    its last 8 bytes).  out_lens: what the result records say where that is not len(stream) (fabricated).
    Returns a dict: image, arch_offsets [narchives + 1], arch_lens, arch_statuses, entry_offsets, data_offsets,
    dir_offsets, parts [2 * count + narchives + 1]."""
    count = len(streams)
    image = bytearray()
    arch_offsets, arch_lens, arch_statuses, dir_offsets = [], [], [], []
    entry_offsets, data_offsets, parts = [0] * count, [0] * count, []
    out_lens = out_lens or [len(s) for s in streams]
    for a in range(len(arch_first) - 1):
        ids = range(arch_first[a], arch_first[a + 1])
        at = len(image)
        arch_offsets.append(at)
        status = Z_OK
        if any(statuses[i] != Z_OK or out_lens[i] < 18 for i in ids):
            status = Z_BUF_ERROR
        else:
            length = sum(LOCAL + DIR + 2 * len(names[i]) + out_lens[i] - 18 for i in ids) + end_len(len(ids))
            if length > MAX_ARCHIVE:
                status = Z_MEM_ERROR
        arch_statuses.append(status)
        if status != Z_OK:
            arch_lens.append(0)
            dir_offsets.append(at)
            for i in ids:
                entry_offsets[i] = data_offsets[i] = at
            parts += [at] * (2 * len(ids) + 1)
            continue
        directory = bytearray()
        dparts = []
        for i in ids:
            s = streams[i]
            crc, usize = struct.unpack("<II", s[-8:])
            dt = datetimes[i] if datetimes is not None else NO_DATETIME
            entry_offsets[i] = len(image)
            parts.append(len(image))
            image += local_header(flags, dt, crc, len(s) - 18, usize, len(names[i])) + names[i]
            data_offsets[i] = len(image)
            image += s[10:-8]
            dparts.append(len(directory))
            directory += dir_record(flags, dt, crc, len(s) - 18, usize, len(names[i]), entry_offsets[i] - at) + names[i]
        doff = len(image)
        dir_offsets.append(doff)
        parts += [doff + d for d in dparts]
        image += directory
        parts.append(len(image))
        image += end_records(len(ids), len(directory), doff - at)
        arch_lens.append(len(image) - at)
        image += b"\0" * (round_up(len(image), align) - len(image))
    arch_offsets.append(len(image))
    parts.append(len(image))
    return dict(image=bytes(image), arch_offsets=arch_offsets, arch_lens=arch_lens, arch_statuses=arch_statuses,
                entry_offsets=entry_offsets, data_offsets=data_offsets, dir_offsets=dir_offsets, parts=parts)


def walk(data):
    """One archive, strictly: the end record (and the ZIP64 records where the count says so), the directory, then
    every local header from offset 0; local and directory facts agree, the entries tile [0, directory) without a
    gap, the directory ends where the end records begin.  Returns (entries, dir_offset), an entry being a dict of
    name, header_offset, data_offset, csize, usize, crc, datetime, flags."""
    assert len(data) >= END and data[-END:-END + 4] == b"PK\x05\x06", "no end record where it must be"
    d0, d1, n0, n1, dsize, doff, clen = struct.unpack("<HHHHIIH", data[-END + 4:])
    assert (d0, d1, clen) == (0, 0, 0) and n0 == n1
    count, end_at = n0, len(data) - END
    if n0 == 0xFFFF:
        loc = data[-END - 20:-END]
        sig, disk, z64, disks = struct.unpack("<4sIQI", loc)
        assert (sig, disk, disks) == (b"PK\x06\x07", 0, 1) and z64 == len(data) - END64
        sig, size, made, need, da, db, c0, c1, dsize64, doff64 = struct.unpack("<4sQHHIIQQQQ", data[z64:z64 + 56])
        assert (sig, size, made, need, da, db) == (b"PK\x06\x06", 44, 45, 45, 0, 0) and c0 == c1 >= ZIP64_AT
        assert (dsize64, doff64) == (dsize, doff)
        count, end_at = c0, z64
    assert doff + dsize == end_at, "the directory does not end where the end records begin"
    entries, at, local_at = [], doff, 0
    for _ in range(count):
        (sig, made, need, flags, method, tm, dt, crc, csize, usize, n, extra, comment, disk, internal, external,
         offset) = struct.unpack("<4sHHHHHHIIIHHHHHII", data[at:at + DIR])
        assert (sig, made, need, method, extra, comment, disk, internal, external) == (b"PK\x01\x02", 20, 20, 8, 0, 0,
                                                                                      0, 0, 0), at
        name = data[at + DIR:at + DIR + n]
        assert len(name) == n
        at += DIR + n
        assert offset == local_at, "the entries leave a gap or overlap"
        lh = struct.unpack("<4sHHHHHIIIHH", data[offset:offset + LOCAL])
        assert lh == (b"PK\x03\x04", 20, flags, 8, tm, dt, crc, csize, usize, n, 0), offset
        assert data[offset + LOCAL:offset + LOCAL + n] == name
        entries.append(dict(name=bytes(name), header_offset=offset, data_offset=offset + LOCAL + n, csize=csize,
                            usize=usize, crc=crc, datetime=dt << 16 | tm, flags=flags))
        local_at = offset + LOCAL + n + csize
    assert at == doff + dsize and local_at == doff
    return entries, doff
