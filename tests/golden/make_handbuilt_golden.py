"""Record what the compiled reference makes of the hand-built streams of tests/deflate_builder.py.

    python tests/golden/make_handbuilt_golden.py        (needs oracle/_ref/libzsc_ref.so)

Writes tests/golden/handbuilt_golden.json: per case the SHA-256 of the stream, the dest cap, window_bits
and the reference's (rc, out_len, consumed, sha256(out)) -- for the whole stream, and for the truncations
and caps of deflate_builder.sweep_of().  A short case is recorded at every truncation and four caps; to keep
that small its sweep is stored as run-length lists of rc, out_len and consumed - cut per cap, with one
SHA-256 over the outputs' digests (deflate_builder.group_digest).  Results and hashes only: no stream bytes.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import deflate_builder as B  # noqa: E402
from oracle.oracle_py import Reference  # noqa: E402


def main():
    if not Reference.available():
        sys.exit("the compiled reference is not built: make -C oracle ref")
    ref = Reference()
    # the reference reports every failed decode through printf: thousands of lines here
    sys.stdout.flush()
    keep = os.dup(1)
    null = os.open(os.devnull, os.O_WRONLY)
    os.dup2(null, 1)
    golden = {"note": "recorded by tests/golden/make_handbuilt_golden.py from the compiled reference", "cases": {}}
    total = 0
    for name, stream, cap, wbits, want in B.cases():
        rc, out, used = ref.uncompress(stream, cap, window_bits=wbits)
        if want is not None:
            assert (rc, out) == (0, want) and used <= len(stream), (name, rc, len(out), used)
        g = {"stream_sha256": B.sha(stream), "stream_len": len(stream), "cap": cap, "window_bits": wbits,
             "full": [rc, len(out), used, B.sha(out)]}
        sweep = B.sweep_of(name, stream, cap, None if want is None else len(want))
        total += 1 + len(sweep)
        if len(stream) >= B.SHORT:
            g["points"] = []
            for cut, c in sweep:
                rc, out, used = ref.uncompress(stream[:cut], c, window_bits=wbits)
                g["points"].append([cut, c, rc, len(out), used, B.sha(out)])
        else:
            g["sweep"], g["sweep_sha256"] = {}, {}
            for c in dict.fromkeys(c for _, c in sweep):
                rows = [ref.uncompress(stream[:cut], c, window_bits=wbits) + (cut,) for cut, cc in sweep if cc == c]
                g["sweep"][str(c)] = {"rc": B.rle([r[0] for r in rows]), "out_len": B.rle([len(r[1]) for r in rows]),
                                      "consumed_minus_cut": B.rle([r[2] - r[3] for r in rows])}
                g["sweep_sha256"][str(c)] = B.group_digest([r[1] for r in rows])
        golden["cases"][name] = g
    ctypes.CDLL(None).fflush(None)
    os.dup2(keep, 1)
    path = B.GOLDEN
    with open(path, "w") as f:
        json.dump(golden, f, separators=(",", ":"))
        f.write("\n")
    recs, _, _ = B.records(golden)
    assert len(recs) == total
    print(f"{len(golden['cases'])} cases, {total} records, {os.path.getsize(path)} bytes -> {path}")


if __name__ == "__main__":
    main()
