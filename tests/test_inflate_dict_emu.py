"""The decoder's dictionary variant (zsc_amd/csrc/inflate.h, INF_SEC_DICT) on the lane emulation.

tests/emu_dict builds the kernel sources with -DZSC_WAVE_EMU into a stand-alone program at 64, 16 (the
decoder's group width on the GPU) and 8 lanes; it makes each dictionary's id and window image as the runtime's
kernel makes them and decodes with the relaunches after data errors.

Every recorded and every hand-built case of tests/inflate_dict_cases.py: (status, out_len, consumed, bytes)
must be the expectation, and every byte of the destination beyond out_len untouched (the program checks dest_cap
+ 64 bytes).  The programs built with AddressSanitizer and UndefinedBehaviorSanitizer run the hand-built set
once; there the window image is allocated at the dictionary's own size, so that a read before its first byte
is a read outside the allocation.
"""
import os
import struct
import subprocess

import pytest

import inflate_dict_cases as idc

HERE = os.path.dirname(os.path.abspath(__file__))
LANES = (64, 16, 8)
NO_DICT = 0xFFFFFFFF


def run_emu(tmp_path, lanes, cases, san=False):
    """[(status, out_len, consumed, clean, bytes)] of the cases"""
    path = os.path.join(str(tmp_path), f"cases{lanes}.bin")
    outp = os.path.join(str(tmp_path), f"out{lanes}.bin")
    with open(path, "wb") as f:
        for c in cases:
            d = b"" if c.dict is None else c.dict
            f.write(struct.pack("<iIII", c.wbits, c.cap, NO_DICT if c.dict is None else len(d), len(c.stream)))
            f.write(d + c.stream)
    prog = os.path.join(HERE, "emu_dict", f"emu_dict{lanes}" + ("_san" if san else ""))
    r = subprocess.run([prog, path, outp], check=True, stdout=subprocess.PIPE)
    rows = [tuple(int(x) for x in line.split()) for line in r.stdout.decode().splitlines()]
    assert len(rows) == len(cases)
    blob, at, res = open(outp, "rb").read(), 0, []
    for row in rows:
        res.append(row + (blob[at:at + row[1]],))
        at += row[1]
    assert at == len(blob)
    return res


def check(cases, rows, lanes):
    for c, (status, out_len, consumed, clean, out) in zip(cases, rows):
        assert (status, out_len, consumed) == (c.status, len(c.out), c.consumed), (lanes, c.name)
        assert out == c.out, (lanes, c.name)
        assert clean == 1, (lanes, c.name)


@pytest.fixture(scope="module")
def emu_built():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_dict")], check=True)


@pytest.fixture(scope="module")
def emu_san_built():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_dict"), "SAN=-fsanitize=address,undefined"], check=True)


@pytest.fixture(scope="module")
def recorded():
    return idc.recorded()


@pytest.fixture(scope="module")
def handbuilt():
    return idc.handbuilt()


def test_the_cases_cover_the_contract(recorded, handbuilt):
    assert {c.wbits for c in recorded} == set(range(9, 16)) | set(range(-15, -8))
    assert {len(c.dict) for c in recorded} == {1, 511, 512, 513, 32767, 32768, 32769, 51200}
    assert {c.status for c in handbuilt} == {0, 2, -3}
    assert any(c.dict is None for c in handbuilt) and any(c.dict == b"" for c in handbuilt)


@pytest.mark.parametrize("lanes", LANES)
def test_recorded_streams(emu_built, tmp_path, recorded, lanes):
    check(recorded, run_emu(tmp_path, lanes, recorded), lanes)


@pytest.mark.parametrize("lanes", LANES)
def test_handbuilt_streams(emu_built, tmp_path, handbuilt, lanes):
    check(handbuilt, run_emu(tmp_path, lanes, handbuilt), lanes)


@pytest.mark.parametrize("lanes", LANES)
def test_handbuilt_streams_under_the_sanitizers(emu_san_built, tmp_path, handbuilt, lanes):
    check(handbuilt, run_emu(tmp_path, lanes, handbuilt, san=True), lanes)
