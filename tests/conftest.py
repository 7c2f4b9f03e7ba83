"""pytest configuration: markers, paths, and one-time builds of the checkers."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    # build what the tests load; hipcc cross-compiles here, nothing needs a GPU
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "oracle", "ref"], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu")], check=True)
    if not os.path.exists(os.path.join(ROOT, "zsc_amd", "libzsc_hip.so")) or os.path.isdir("/opt/rocm/bin"):
        try:
            subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "zsc_amd", "csrc")], check=True)
        except Exception as exc:  # pragma: no cover
            print("warning: could not (re)build libzsc_hip.so:", exc)


@pytest.fixture(scope="session")
def oracle():
    from oracle.oracle_py import Oracle
    return Oracle()


@pytest.fixture(scope="session")
def live_reference():
    from oracle.oracle_py import Reference
    return Reference() if Reference.available() else None


@pytest.fixture
def reference(request, live_reference, oracle):
    """The compiled reference where the build could make oracle/_ref/libzsc_ref.so; elsewhere its
    recorded answers to this test's calls (tests/reference_calls.py), each restated by the oracle."""
    if live_reference is not None:
        yield live_reference
        return
    from reference_calls import RecordedReference, recorded_calls
    calls = recorded_calls(request.node.name)
    if calls is None:
        pytest.fail(f"no recorded reference answers for {request.node.name}: run tests/golden/record_reference_calls.py")
    rec = RecordedReference(calls, oracle)
    yield rec
    # (only where the test body passed: a failure of its own already says what went wrong)
    rep = getattr(request.node, "rep_call", None)
    if rep is not None and rep.passed:
        assert rec.exhausted(), f"{request.node.name} made fewer reference calls than were recorded: re-record"


@pytest.hookimpl(hookwrapper=True)
def pytest_runtest_makereport(item, call):
    """Keep each phase's report on the test item (rep_setup / rep_call), for fixture teardowns."""
    outcome = yield
    rep = outcome.get_result()
    setattr(item, "rep_" + rep.when, rep)


def gpu_available() -> bool:
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.fixture(autouse=True)
def _flush_c_stdio():
    """The compiled reference reports through printf (its own example configuration header,
    /root/reference/test/zsc_test_private.h:73-81): flush C stdio while pytest still captures the test's
    output, so that those lines stay with their test instead of pouring out when the process exits."""
    yield
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
