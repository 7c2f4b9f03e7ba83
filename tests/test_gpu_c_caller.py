"""A C program compiled against the REFERENCE'S OWN headers and linked to libzsc_hip.so
(tests/c_caller/caller.c, built into oracle/_ref/): the drop-in boundary as a C user sees it --
prototypes, enum widths and gz_header's layout are checked by a compiler, not by reading.  The same program compiled
against this project's own include/ runs wherever the library was built."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
BIN = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "caller_ref")  # oracle/Makefile caller_ref
BIN_OWN = os.path.join(HERE, "c_caller", "caller_own")


def _run(binary):
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(HERE, "..", "zsc_amd") + ":" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.startswith("OK "), (r.returncode, r.stdout, r.stderr[-2000:])


@pytest.mark.gpu
def test_c_caller_built_against_reference_headers():
    if not os.path.exists(BIN):
        pytest.skip("oracle/_ref/caller_ref was not built (needs the reference's headers at build time)")
    _run(BIN)


@pytest.mark.gpu
def test_c_caller_built_against_own_headers():
    assert os.path.exists(BIN_OWN), "tests/c_caller/caller_own was not built (make -C tests/c_caller)"
    _run(BIN_OWN)
