"""The BGZF file format of include/zsc_hip.h ("BGZF files") restated in Python: what the writer must give.

Shared by tests/test_bgzf_emu.py and tests/test_gpu_bgzf.py.  Nothing here asks the code under test anything.
"""
import struct

Z_OK, Z_STREAM_ERROR, Z_BUF_ERROR = 0, -2, -5
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
MAX_MEMBER = 65536
TILE = 16384


def member(stream):
    """the BGZF member of a gzip stream with the plain 10-byte header"""
    length = len(stream) + 8
    assert 28 <= length <= MAX_MEMBER
    return (b"\x1f\x8b\x08\x04\0\0\0\0" + stream[8:9] + b"\xff\x06\0BC\x02\0" + struct.pack("<H", length - 1) +
            stream[10:])


def round_up(v, align):
    return (v + align - 1) // align * align


def expected(streams, statuses, file_first, align):
    """(image, file_offsets [nfiles + 1], file_lens, file_statuses, member_offsets, parts [count + nfiles + 1])"""
    image = bytearray()
    file_offsets, file_lens, file_statuses, member_offsets, parts = [], [], [], [0] * len(streams), []
    for f in range(len(file_first) - 1):
        ids = range(file_first[f], file_first[f + 1])
        at = len(image)
        file_offsets.append(at)
        if any(statuses[i] != Z_OK or len(streams[i]) + 8 > MAX_MEMBER for i in ids):
            file_lens.append(0)
            file_statuses.append(Z_BUF_ERROR)
            for i in ids:
                member_offsets[i] = at
            parts += [at] * (len(ids) + 1)
            continue
        for i in ids:
            member_offsets[i] = len(image)
            parts.append(len(image))
            image += member(streams[i])
        parts.append(len(image))
        image += BGZF_EOF
        file_lens.append(len(image) - at)
        file_statuses.append(Z_OK)
        image += b"\0" * (round_up(len(image), align) - len(image))
    file_offsets.append(len(image))
    parts.append(len(image))
    return bytes(image), file_offsets, file_lens, file_statuses, member_offsets, parts


def walk_bsize(data):
    """the members of a BGZF file by BSIZE alone: [(offset, length)]; the last is the 28-byte tail and ends the
    file, or the walk raises"""
    at, out = 0, []
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 10:at + 16] == b"\x06\0BC\x02\0", at
        length = struct.unpack_from("<H", data, at + 16)[0] + 1
        out.append((at, length))
        at += length
    assert at == len(data) and out and data[out[-1][0]:] == BGZF_EOF
    return out
