#!/usr/bin/env python3
"""Record the compiled reference's answers to every test that takes the `reference` fixture
into tests/golden/reference_calls.json (see tests/reference_calls.py).

Run where the reference can be built (oracle/_ref/libzsc_ref.so, `make -C oracle ref`):
    python tests/golden/record_reference_calls.py
Each such test is run once against the live reference, so the recording is only written
when every one of them passes.
"""
import importlib
import inspect
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path[:0] = [ROOT, TESTS]
from oracle.oracle_py import Oracle, Reference, build  # noqa: E402
from reference_calls import GOLDEN, Recorder  # noqa: E402

MODULES = ("test_api_host", "test_oracle")


def main() -> None:
    build(ref=True)
    if not Reference.available():
        raise SystemExit("oracle/_ref/libzsc_ref.so could not be built: the reference sources are needed")
    oracle, ref = Oracle(), Reference()
    out = {}
    for mod_name in MODULES:
        mod = importlib.import_module(mod_name)
        for name, fn in sorted(vars(mod).items()):
            if not (name.startswith("test_") and callable(fn)):
                continue
            params = inspect.signature(fn).parameters
            if "reference" not in params:
                continue
            rec = Recorder(ref)
            fixtures = {"reference": rec, "oracle": oracle}
            fn(**{p: fixtures[p] for p in params})
            out[name] = rec.calls
            print(f"{mod_name}::{name}: {len(rec.calls)} calls")
    with open(GOLDEN, "w") as f:
        f.write("{\n")
        f.write(",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in sorted(out.items())))
        f.write("\n}\n")
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
