"""Record the BGZF members the compiled reference writes for buffers of zsc_amd/corpus.py.

    python tests/golden/make_bgzf_golden.py        (needs oracle/_ref/libzsc_ref.so)

The reference is called as a BGZF writer calls it: zsc_compress_gzip2 with a gz_header of text 0, time 0, os
255, no name, comment or header CRC, and the extra field "BC" 02 00 BSIZE, BSIZE being the member's length - 1
(known from a first call without a gz_header: the member is 8 bytes longer than that stream).  Writes
tests/golden/bgzf_golden.json: per buffer (kind, size, seed), level and mem_level, the member's length and
SHA-256, and its bytes in hex where it is shorter than 2 KiB.  A buffer whose member would pass 65 536 bytes has
no member: the length of its plain stream is kept as "overflow".

Asserted on the way: the member is the 18-byte header of include/zsc_hip.h ("BGZF files") followed by the
plain stream from byte 10 on, and CPython's gzip module gives the input back.
"""
import gzip
import hashlib
import json
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle.oracle_py import Reference  # noqa: E402
from zsc_amd import corpus  # noqa: E402
from zsc_amd.api import gz_header_for_writing  # noqa: E402

GOLDEN = os.path.join(HERE, "bgzf_golden.json")
SIZES = (0, 1, 100, 4096, 65280, 65536)


def entries():
    """(kind, size, seed, level, mem_level)"""
    out = []
    for k, kind in enumerate(("text", "zero", "random")):
        for j, size in enumerate(SIZES):
            out.append((kind, size, 40 + 6 * k + j, 6, 8))
    for kind in ("text", "random"):
        for size in (100, 4096, 65280):
            out.append((kind, size, 70 + size % 7, 1, 8))
    out.append(("zero", 65536, 77, 1, 8))
    for kind in ("text", "random", "zero"):
        for size in (100, 4096, 65280):
            out.append((kind, size, 80 + size % 7, 9, 1))
    out += [("text", 4096, 90, 9, 8), ("text", 65536, 91, 9, 8), ("text", 65280, 92, 6, 1), ("random", 4096, 93, 6, 1)]
    return out


def main():
    if not Reference.available():
        sys.exit("the compiled reference is not built: make -C oracle ref")
    ref = Reference()
    recs = []
    for kind, size, seed, level, mem_level in entries():
        buf = corpus.make_buffer(kind, size, seed)
        rc, plain = ref.compress(buf, level, window_bits=31, mem_level=mem_level)
        assert rc == 0, (kind, size, rc)
        rec = {"kind": kind, "size": size, "seed": seed, "level": level, "mem_level": mem_level}
        if len(plain) + 8 > 65536:
            rec["overflow"] = len(plain)
            recs.append(rec)
            continue
        bsize = len(plain) + 8 - 1
        h, keep = gz_header_for_writing(text=0, time=0, os=255, extra=b"BC\x02\x00" + struct.pack("<H", bsize))
        rc, member = ref.compress(buf, level, window_bits=31, mem_level=mem_level, gz_header=h)
        assert rc == 0, (kind, size, rc)
        want = (b"\x1f\x8b\x08\x04\0\0\0\0" + plain[8:9] + b"\xff\x06\0BC\x02\0" + struct.pack("<H", bsize) + plain[10:])
        assert member == want, (kind, size, level, mem_level)
        assert gzip.decompress(member) == buf
        rec["len"] = len(member)
        rec["sha256"] = hashlib.sha256(member).hexdigest()
        if len(member) < 2048:
            rec["hex"] = member.hex()
        recs.append(rec)
    golden = {"note": "recorded by tests/golden/make_bgzf_golden.py from the compiled reference", "members": recs}
    with open(GOLDEN, "w") as f:
        json.dump(golden, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(recs)} members, {sum('overflow' in r for r in recs)} overflow, {os.path.getsize(GOLDEN)} bytes -> {GOLDEN}")


if __name__ == "__main__":
    main()
