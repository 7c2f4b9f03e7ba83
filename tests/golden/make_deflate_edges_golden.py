"""Record what the compiled reference makes of the inputs of tests/deflate_cases.py.

    python tests/golden/make_deflate_edges_golden.py        (needs oracle/_ref/libzsc_ref.so)

Writes tests/golden/deflate_edges_golden.json: per case the reference's rc, the length of its stream and the
stream's SHA-256.  Family F (every length 0..300 of four kinds of data, four parameter sets) is kept as one
record per kind and parameter set: the lists of rc and length, and one SHA-256 over the streams' SHA-256s.
Results and hashes only; the inputs are generated again from their seeds wherever they are needed.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import deflate_cases as D  # noqa: E402
from oracle.oracle_py import Reference  # noqa: E402


def main():
    if not Reference.available():
        sys.exit("the compiled reference is not built: make -C oracle ref")
    ref = Reference()
    cases = D.cases()
    results = {}
    for c in cases:
        rc, out = ref.compress(c.data, c.level, window_bits=c.window_bits, mem_level=c.mem_level,
                               strategy=c.strategy, work_len=1 << 20)
        assert rc == 0, (c.name, rc)
        results[c.name] = (rc, out)
    golden = {"note": "recorded by tests/golden/make_deflate_edges_golden.py from the compiled reference",
              "cases": {c.name: [results[c.name][0], len(results[c.name][1]), D.sha(results[c.name][1])]
                        for c in cases if c.family != "F"},
              "groups": {}}
    for name, g in D.f_groups(cases).items():
        got = [results[c.name] for c in g]
        golden["groups"][name] = {"rc": [r[0] for r in got], "out_len": [len(r[1]) for r in got],
                                  "sha256": D.group_digest([r[1] for r in got])}
    with open(D.GOLDEN, "w") as f:
        json.dump(golden, f, separators=(",", ":"))
        f.write("\n")
    D.check_against_golden(golden, cases, results, "reference")
    print(f"{len(golden['cases'])} cases, {len(golden['groups'])} groups, {os.path.getsize(D.GOLDEN)} bytes -> {D.GOLDEN}")


if __name__ == "__main__":
    main()
