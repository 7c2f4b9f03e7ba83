"""Record what the compiled reference makes of the inputs of tests/parser_cases.py.

    python tests/golden/make_parser_edges_golden.py        (needs oracle/_ref/libzsc_ref.so)

Writes tests/golden/parser_edges_golden.json: per case the reference's rc, the length of its stream, the stream's
SHA-256, and the tokens the walker reads from it at the places the case's features name.  Every feature must
hold on the reference's stream: a case whose edge token cannot be seen there is refused here.
Results and hashes only; the inputs are generated again from their seeds wherever they are needed.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import parser_cases as P  # noqa: E402
from oracle.oracle_py import Reference  # noqa: E402


def main():
    if not Reference.available():
        sys.exit("the compiled reference is not built: make -C oracle ref")
    ref = Reference()
    golden = {"note": "recorded by tests/golden/make_parser_edges_golden.py from the compiled reference", "cases": {}}
    for c in P.cases():
        rc, out = ref.compress(c.data, c.level, window_bits=c.window_bits, mem_level=c.mem_level,
                               strategy=c.strategy, work_len=1 << 20)
        assert rc == 0, (c.name, rc)
        ps = P.Parse(out, c.window_bits)
        assert ps.data == c.data, c.name
        assert not ps.missing(c.features), (c.name, ps.missing(c.features))
        golden["cases"][c.name] = [rc, len(out), P.sha(out), ps.summary(c.features)]
    with open(P.GOLDEN, "w") as f:
        json.dump(golden, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(golden['cases'])} cases, {os.path.getsize(P.GOLDEN)} bytes -> {P.GOLDEN}")


if __name__ == "__main__":
    main()
