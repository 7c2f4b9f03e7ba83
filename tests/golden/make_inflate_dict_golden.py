"""Writes tests/golden/inflate_dict_golden.json: streams CPython's zlib wrote with preset dictionaries.

    python tests/golden/make_inflate_dict_golden.py

The streams are recorded, not made when the tests run, so that another zlib build cannot change them.  Each
entry holds the stream as hex, its dictionary as (generator, seed, length) of zsc_amd/corpus.py, and length
and SHA-256 of the expected output.  Asserted here: every output equals what zlib.decompressobj(wbits,
zdict=D) gives, and every raw stream needs its dictionary -- zlib.decompressobj(-15) without it raises.
"""
import hashlib
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import inflate_dict_cases as idc  # noqa: E402


def main():
    streams = []
    for spec in idc.recorded_specs():
        d = idc.make_dict(**spec["dict"])
        rec = idc.record_of(spec, d)
        assert 64 <= len(rec) <= 8192
        co = zlib.compressobj(spec["level"], zlib.DEFLATED, spec["wbits"], zdict=d)
        s = co.compress(rec) + co.flush()
        o = zlib.decompressobj(spec["wbits"], zdict=d)
        assert o.decompress(s) == rec and o.eof and not o.unused_data, spec["name"]
        if spec["wbits"] < 0:
            try:
                zlib.decompressobj(-15).decompress(s)
            except zlib.error:
                pass
            else:
                raise AssertionError(spec["name"] + " does not need its dictionary")
        else:
            assert s[1] & 0x20, spec["name"]
        streams.append({"name": spec["name"], "wbits": spec["wbits"], "level": spec["level"], "dict": spec["dict"],
                        "hex": s.hex(), "out_len": len(rec), "sha256": hashlib.sha256(rec).hexdigest()})
    path = os.path.join(HERE, "inflate_dict_golden.json")
    with open(path, "w") as f:
        json.dump({"zlib_version": zlib.ZLIB_RUNTIME_VERSION, "streams": streams}, f, indent=0)
        f.write("\n")
    print(len(streams), "streams,", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 256 * 1024


if __name__ == "__main__":
    main()
