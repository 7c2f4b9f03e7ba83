"""The compiled reference's answers, recorded, for machines where it cannot be built.

The tests that compare the oracle with the compiled reference (the `reference` fixture)
call it in a fixed, seeded order.  tests/golden/record_reference_calls.py runs them once
against the live reference (oracle/_ref/libzsc_ref.so) and stores every answer in
tests/golden/reference_calls.json, bytes as length + SHA-256 prefix.  Where the reference
is absent, RecordedReference answers the same calls from that file: each call is
restated by the oracle and must match what the reference answered, call by call, or the
test fails there; answers the oracle cannot restate (the work-size helpers) are returned
as recorded.
"""
from __future__ import annotations

import hashlib
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_calls.json")
_cache = {}


def norm(x):
    """An answer in storable form: bytes -> ["b", length, sha256 prefix], tuples -> lists."""
    if isinstance(x, (bytes, bytearray)):
        return ["b", len(x), hashlib.sha256(bytes(x)).hexdigest()[:16]]
    if isinstance(x, (tuple, list)):
        return [norm(v) for v in x]
    return x


def recorded_calls(test_name: str):
    if not _cache:
        _cache.update(json.load(open(GOLDEN)))
    return _cache.get(test_name)


class Recorder:
    """Wraps the live reference and notes every answer (used by record_reference_calls.py)."""

    def __init__(self, reference):
        self._ref = reference
        self.calls = []

    def __getattr__(self, method):
        fn = getattr(self._ref, method)

        def call(*args, **kw):
            res = fn(*args, **kw)
            self.calls.append([method, norm(res)])
            return res
        return call


class RecordedReference:
    """Stands in for oracle_py.Reference in one test: answers its calls in order from the recording."""

    def __init__(self, calls, oracle):
        self._calls = calls
        self._next = 0
        self._oracle = oracle

    def exhausted(self) -> bool:
        return self._next == len(self._calls)

    def _answer(self, method, own, args):
        assert self._next < len(self._calls), f"call {self._next} ({method}) was not recorded: re-record"
        name, want = self._calls[self._next]
        self._next += 1
        assert name == method, f"call {self._next - 1}: recorded {name}, called {method}: re-record"
        if own is None:  # nothing to restate: the reference's own answer
            return tuple(want) if isinstance(want, list) else want
        if norm(own) != want:
            raise AssertionError(f"call {self._next - 1} {method}{args}: the oracle answers {norm(own)}, "
                                 f"the reference answered {want}")
        return own

    @staticmethod
    def _brief(args):
        return tuple(f"<{len(a)} bytes>" if isinstance(a, (bytes, bytearray)) else a for a in args)

    def compress(self, data, *args, **kw):
        return self._answer("compress", self._oracle.compress(data, *args, **kw)[:2], self._brief((data,) + args))

    def uncompress(self, data, *args, **kw):
        return self._answer("uncompress", self._oracle.uncompress(data, *args, **kw), self._brief((data,) + args))

    def max_output(self, *args):
        return self._answer("max_output", self._oracle.max_output(*args), args)

    def adler32(self, data, *args):
        return self._answer("adler32", self._oracle.adler32(data, *args), self._brief((data,) + args))

    def crc32(self, data, *args):
        return self._answer("crc32", self._oracle.crc32(data, *args), self._brief((data,) + args))

    def compress_min_work(self, *args):
        return self._answer("compress_min_work", None, args)

    def uncompress_min_work(self, *args):
        return self._answer("uncompress_min_work", None, args)
