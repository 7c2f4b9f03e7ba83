"""Read-back verification of a deflate plan's streams (zsc_amd/csrc/deflate_verify.h) on the lane emulation,
against the oracle.

tests/emu_verify builds the deflate pipeline's kernel sources and deflate_verify.h with -DZSC_WAVE_EMU and
runs what zsc_hip_deflate_plan_run enqueues for one buffer with verification on, then what
zsc_hip_deflate_plan_verify enqueues, on a stream and an input this file supplies.  The streams are the
oracle's; whether a damaged stream is still good is decided by the oracle's uncompress: verification must
never call a stream good that the oracle's decoder does not turn back into the input (soundness), and must
name the block the damage lies in (localisation).  It may be stricter than a decoder where a decoder does
not care (padding bits, the gzip header's MTIME / XFL / OS), but only in a small share of the flips.
"""
import ctypes as C
import os
import random
import subprocess
import sys

import pytest

from test_deflate_index_emu import CASES, buffer, case_id

HERE = os.path.dirname(os.path.abspath(__file__))
Z_BUF_ERROR = -5
OK, SKIPPED, HEADER, BLOCK_HDR, CODES, LITERAL, DISTANCE, MATCH, LENGTH, BIT_END, TRAILER = 0, -1, 1, 2, 3, 4, 5, 6, 7, 8, 9
NONE = 0xFFFFFFFF
BT_STORED, BT_STATIC, BT_DYNAMIC = 0, 1, 2


def load(name):
    L = C.CDLL(os.path.join(HERE, "emu_verify", name))
    L.emu_verify_compress.argtypes = [C.c_char_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32,
                                      C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32,
                                      C.POINTER(C.c_uint32)]
    L.emu_verify_check.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int,
                                   C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_int32)]
    L.emu_verify_check.restype = None
    # the deflate pipeline is whole-wave code for 64 lanes: a 16-lane build verifies what the 64-lane one wrote
    L.pipeline = L if "16" not in name else load(name.replace("16", "64"))
    return L


@pytest.fixture(scope="module", params=["libvfy_emu64.so", "libvfy_emu16.so"])
def vfy(request):
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_verify")], check=True)
    return load(request.param)


@pytest.fixture(scope="module")
def vfy64():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_verify")], check=True)
    return load("libvfy_emu64.so")


class Plan:
    """one buffer of a plan with verification enabled, after its run"""

    def __init__(self, L, data, level, wbits, mem_level, strategy, out_cap):
        self.L, self.data, self.params, self.out_cap = L, data, (level, wbits, mem_level, strategy), out_cap
        out = C.create_string_buffer(max(out_cap, 1) + 64)
        max_blocks = len(data) // ((1 << (mem_level + 6)) - 1) + 2
        facts = (C.c_uint32 * (4 * max_blocks))()
        ol, nb = C.c_uint32(), C.c_uint32()
        self.status = L.pipeline.emu_verify_compress(data, len(data), level, wbits, mem_level, strategy, out_cap, out,
                                            C.byref(ol), facts, max_blocks, C.byref(nb))
        assert nb.value <= max_blocks
        self.out_len, self.facts, self.nblocks = ol.value, facts, nb.value
        self.stream = out.raw[:ol.value] if self.status == 0 else b""
        # (bit_off, in_begin, in_len, type, last)
        self.blocks = [(facts[4 * i], facts[4 * i + 1], facts[4 * i + 2], facts[4 * i + 3] & 0xff, facts[4 * i + 3] >> 8)
                       for i in range(nb.value)]

    def verify(self, stream=None, data=None, cap=None):
        """(verdict, block, bit_off, in_pos) of verifying `stream` (lying in `cap` bytes) against `data`"""
        stream = self.stream if stream is None else stream
        data = self.data if data is None else data
        cap = self.out_cap if cap is None else cap
        room = stream + bytes(cap - len(stream))
        res = (C.c_int32 * 4)()
        level, wbits, mem_level, strategy = self.params
        self.L.emu_verify_check(data, len(data), room, cap, self.out_len, self.status, level, wbits, mem_level,
                                strategy, self.facts, self.nblocks, res)
        return res[0], res[1] & 0xFFFFFFFF, res[2] & 0xFFFFFFFF, res[3] & 0xFFFFFFFF


def plan_for(L, oracle, data, level, wbits, mem_level, strategy=0):
    cap = oracle.max_output(len(data), max(len(data), 1), level, wbits, mem_level)[1]
    return Plan(L, data, level, wbits, mem_level, strategy, cap)


def wrapper(wbits):
    """(kind, header bytes, trailer bytes)"""
    return (0, 0, 0) if wbits < 0 else (2, 10, 8) if wbits > 15 else (1, 2, 4)


# ---- an independent walk over a stream's blocks: where each starts and which type it has ----------------

class Bits:
    def __init__(self, data, pos):
        self.d, self.p = data, pos

    def peek(self, n):
        at = self.p >> 3
        return (int.from_bytes(self.d[at:at + 4], "little") >> (self.p & 7)) & ((1 << n) - 1)

    def take(self, n):
        v = self.peek(n)
        self.p += n
        return v


def canonical(lens):
    """{(length, code): symbol}"""
    code, out = 0, {}
    for l in range(1, 16):
        for s, sl in enumerate(lens):
            if sl == l:
                out[(l, code)] = s
                code += 1
        code <<= 1
    return out


def decode(br, table):
    w, code = br.peek(15), 0
    for l in range(1, 16):
        code = code << 1 | ((w >> (l - 1)) & 1)
        if (l, code) in table:
            br.p += l
            return table[(l, code)]
    raise AssertionError("no code")


LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_L = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_D = canonical([5] * 30)


_WALKS = {}


def walk(stream, first_bit):
    """[(bit_off, type, out_bytes)] of the blocks of a deflate stream, and the bit after the last one"""
    if (stream, first_bit) not in _WALKS:
        _WALKS[(stream, first_bit)] = walk_blocks(stream, first_bit)
    return _WALKS[(stream, first_bit)]


def walk_blocks(stream, first_bit):
    br, blocks = Bits(stream, first_bit), []
    while True:
        at = br.p
        final, typ = br.take(1), br.take(2)
        n = 0
        if typ == 0:
            br.p = (br.p + 7) & ~7
            n = br.take(16)
            assert br.take(16) == n ^ 0xffff
            br.p += 8 * n
        else:
            if typ == 1:
                lt, dt = FIXED_L, FIXED_D
            else:
                hlit, hdist, hclen = br.take(5) + 257, br.take(5) + 1, br.take(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[CL_ORDER[i]] = br.take(3)
                ct, lens = canonical(cl), []
                while len(lens) < hlit + hdist:
                    s = decode(br, ct)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + br.take(2))
                    elif s == 17:
                        lens += [0] * (3 + br.take(3))
                    else:
                        lens += [0] * (11 + br.take(7))
                lt, dt = canonical(lens[:hlit]), canonical(lens[hlit:hlit + hdist])
            while True:
                s = decode(br, lt)
                if s < 256:
                    n += 1
                elif s == 256:
                    break
                else:
                    n += LBASE[s - 257] + br.take(LEXT[s - 257])
                    br.take(DEXT[decode(br, dt)])
        blocks.append((at, typ, n))
        if final:
            return blocks, br.p


def check_clean(L, oracle, case):
    kind, size, seed, level, wbits, mem_level, strategy, _ = case
    data = buffer(kind, size, seed)
    orc, want, _ = oracle.compress(data, level, window_bits=wbits, mem_level=mem_level, strategy=strategy)
    assert orc == 0
    pl = plan_for(L, oracle, data, level, wbits, mem_level, strategy)
    assert pl.status == 0 and pl.stream == want
    assert pl.verify() == (OK, NONE, 0, 0)
    # the map tiles the input, and only its last block is the last
    at = 0
    for i, (_, in_begin, in_len, _, last) in enumerate(pl.blocks):
        assert in_begin == at and last == (i + 1 == len(pl.blocks))
        at += in_len
    assert at == len(data) and pl.blocks
    # every block starts where a walk over the stream's bits finds it
    _, hdr, trl = wrapper(wbits)
    walked, end = walk(want, 8 * hdr)
    assert [(b[0], b[3], b[2]) for b in pl.blocks] == walked
    assert (end + 7) // 8 == len(want) - trl
    return pl


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_clean(vfy, oracle, case):
    """1. clean streams: the oracle's stream, OK, a block map that tiles the input and agrees with a walk"""
    check_clean(vfy, oracle, case)


# ---- 2. single-bit damage --------------------------------------------------------------------------

def damage_plans():
    """(name, data, level, window_bits, mem_level, seed of the flips)"""
    half = 70001 // 2
    return [("mix-raw", buffer("mix", 70001, 31), 6, -15, 8, 101),
            ("text-zlib-m1", buffer("text", 70001, 32), 6, 15, 1, 102),
            ("random+text-gzip", buffer("random", half, 33) + buffer("text", 70001 - half, 34), 1, 31, 8, 103)]


def flip_positions(pl, wbits, seed):
    """150 seeded bit positions uniform over the stream, the first and last bit of every block and of the trailer"""
    _, hdr, trl = wrapper(wbits)
    nbits = 8 * len(pl.stream)
    rnd = random.Random(seed)
    pos = [rnd.randrange(nbits) for _ in range(150)]
    starts = [b[0] for b in pl.blocks] + [nbits - 8 * trl]
    for i in range(len(pl.blocks)):
        pos += [starts[i], starts[i + 1] - 1]
    if trl:
        pos += [nbits - 8 * trl, nbits - 1]
    return sorted(set(pos))


def region(pl, wbits, bit):
    """'header', 'trailer' or the block a bit of the stream lies in (the last block's padding is its own)"""
    _, hdr, trl = wrapper(wbits)
    if bit < 8 * hdr:
        return "header"
    if bit >= 8 * (len(pl.stream) - trl):
        return "trailer"
    return max(i for i, b in enumerate(pl.blocks) if b[0] <= bit)


def flipped(stream, bit):
    s = bytearray(stream)
    s[bit >> 3] ^= 1 << (bit & 7)
    return bytes(s)


def ref_ok(oracle, stream, data, wbits):
    rc, out, used = oracle.uncompress(stream, len(data) + 64, window_bits=wbits)
    return rc == 0 and out == data and used == len(stream)


def check_flip(pl, oracle, wbits, bit):
    """soundness and localisation of one flip; returns ref_ok"""
    bad = flipped(pl.stream, bit)
    good = ref_ok(oracle, bad, pl.data, wbits)
    verdict, block, _, _ = pl.verify(stream=bad)
    where = region(pl, wbits, bit)
    if not good:
        assert verdict != OK, (bit, where)
        if where == "header":
            assert (verdict, block) == (HEADER, NONE), (bit, verdict, block)
        elif where == "trailer":
            assert (verdict, block) == (TRAILER, NONE), (bit, verdict, block)
        else:
            assert block == where and verdict not in (HEADER, TRAILER, SKIPPED), (bit, where, verdict, block)
    elif verdict != OK and isinstance(where, int):
        assert block == where  # stricter than the decoder, but about the right block
    return good


@pytest.mark.parametrize("which", [0, 1, 2])
def test_single_bit_damage(vfy64, oracle, which):
    name, data, level, wbits, mem_level, seed = damage_plans()[which]
    pl = plan_for(vfy64, oracle, data, level, wbits, mem_level)
    assert pl.status == 0 and pl.stream == oracle.compress(data, level, window_bits=wbits, mem_level=mem_level)[1]
    assert pl.verify()[0] == OK
    flips = flip_positions(pl, wbits, seed)
    tolerated = sum(check_flip(pl, oracle, wbits, bit) for bit in flips)
    print(f"{name}: {len(flips)} flips over {len(pl.blocks)} blocks, {tolerated} the oracle's decoder does not mind")
    # the cap: a sample in which the decoder minds almost every flip
    assert tolerated < 0.05 * len(flips)


# ---- 3. wrong input -------------------------------------------------------------------------------------

def symbols_of(oracle, data, level, wbits, mem_level):
    """[(input offset, length, distance)] of the oracle's parse"""
    assert wbits in (-15, 15, 31)
    syms, ns, _, _ = oracle.parse(data, level, wbits=15, mem_level=mem_level)
    syms = [(syms[i].dist, syms[i].lc) for i in range(ns)]
    out, p = [], 0
    for dist, lc in syms:
        n = lc + 3 if dist else 1
        out.append((p, n, dist))
        p += n
    assert p == len(data)
    return out


@pytest.mark.parametrize("wbits", [-15, 15, 31])
def test_wrong_input(vfy64, oracle, wbits):
    data = buffer("text", 70001, 41)
    pl = plan_for(vfy64, oracle, data, 6, wbits, 8)
    assert pl.status == 0 and pl.verify()[0] == OK
    syms = symbols_of(oracle, data, 6, wbits, 8)
    lits = [p for p, n, d in syms if d == 0 and p > 40000]
    # a byte that a later match copies from: the source of a match far enough back to be outside the match
    src = next(p - d for p, n, d in syms if d > n and p > 40000)
    for at in (lits[0], src, len(data) - 1):
        wrong = bytearray(data)
        wrong[at] ^= 0x20
        verdict, block, _, _ = pl.verify(data=bytes(wrong))
        assert verdict != OK, at
        if wbits < 0:
            # raw: no trailer to catch it -- the block holding the byte, or a later one that copies from it
            holder = max(i for i, b in enumerate(pl.blocks) if b[1] <= at)
            assert verdict in (LITERAL, MATCH) and holder <= block < len(pl.blocks), (at, verdict, block)


# ---- 4. bounds ------------------------------------------------------------------------------------------

def bounds_case(L, oracle):
    """A stream of zeros whose dynamic header's HLIT has a bit flipped, lying at the very end of its allocation:
    the failing block would decode far past it.  Ends with a verdict."""
    data = bytes(300000)
    pl = plan_for(L, oracle, data, 6, -15, 8)
    assert pl.status == 0 and pl.blocks[0][3] == BT_DYNAMIC
    bad = flipped(pl.stream, pl.blocks[0][0] + 3 + 2)  # HLIT follows the 3-bit block header
    assert not ref_ok(oracle, bad, data, -15)
    for cap in (len(bad), pl.out_cap):
        verdict, block, bit_off, _ = pl.verify(stream=bad, cap=cap)
        assert verdict not in (OK, SKIPPED) and (block, bit_off) == (0, pl.blocks[0][0]), (verdict, block)
    # and every other bit of the header, the same way
    for k in range(3, 17):
        bad = flipped(pl.stream, pl.blocks[0][0] + k)
        verdict, block, _, _ = pl.verify(stream=bad, cap=len(bad))
        assert ref_ok(oracle, bad, data, -15) or (verdict not in (OK, SKIPPED) and block == 0)
    # block facts that point outside the input or the stream fail, they do not read there
    keep = list(pl.facts)
    for word, value in ((0, 8 * pl.out_cap + 5), (1, len(data) + 1), (2, len(data) + 1), (0, 0xFFFFFFF0)):
        pl.facts[word] = value
        assert pl.verify(cap=len(pl.stream))[0] not in (OK, SKIPPED)
        pl.facts[word] = keep[word]
    assert pl.verify(cap=len(pl.stream))[0] == OK


def test_bounds(vfy64, oracle):
    bounds_case(vfy64, oracle)


ASAN_CASES = [c for c in CASES if c[1] <= 3072] + [CASES[0], CASES[3], CASES[5], CASES[12]]

ASAN_CHILD = """
import sys
sys.path[:0] = {paths!r}
import test_deflate_verify_emu as t
from oracle.oracle_py import Oracle
L, oracle = t.load("libvfy_emu64_asan.so"), Oracle()
t.bounds_case(L, oracle)
for case in t.ASAN_CASES:
    t.check_clean(L, oracle, case)
name, data, level, wbits, mem_level, seed = t.damage_plans()[1]
pl = t.plan_for(L, oracle, data, level, wbits, mem_level)
for bit in t.flip_positions(pl, wbits, seed)[::4]:
    pl.verify(stream=t.flipped(pl.stream, bit), cap=len(pl.stream))
t.test_short_out_cap(L, oracle)
print("deflate verification under AddressSanitizer: ok")
"""


def test_bounds_under_address_sanitizer():
    """The bounds case, clean cases and damaged streams once more on a build of the emulation with
    AddressSanitizer (host code only), in a child process with the sanitizer's runtime preloaded.  The driver
    copies the stream and the input to allocations of exactly their size: a read outside them ends the child
    with a report, not a verdict."""
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_verify"), "asan"], check=True)
    rt = subprocess.run(["g++", "-print-file-name=libasan.so"], check=True, capture_output=True, text=True).stdout.strip()
    assert os.path.isabs(rt), "no AddressSanitizer runtime beside the compiler"
    env = dict(os.environ)
    env["LD_PRELOAD"] = " ".join(filter(None, [rt, env.get("LD_PRELOAD", "")]))
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=0:exitcode=66:verify_asan_link_order=0"
    code = ASAN_CHILD.format(paths=[os.path.dirname(HERE), HERE])
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0 and "ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-6000:])


# ---- 5. short out_cap -----------------------------------------------------------------------------------

def test_short_out_cap(vfy64, oracle):
    """one byte short: Z_BUF_ERROR from the pipeline, SKIPPED from verification, no block map"""
    for kind, size in (("text", 70001), ("random", 3072), ("text", 0)):
        data = buffer(kind, size, 11)
        want = oracle.compress(data, 6)[1]
        pl = Plan(vfy64, data, 6, 15, 8, 0, len(want) - 1)
        assert (pl.status, pl.stream, pl.blocks) == (Z_BUF_ERROR, b"", [])
        assert pl.verify(stream=bytes(len(want) - 1)) == (SKIPPED, NONE, 0, 0)
        pl = Plan(vfy64, data, 6, 15, 8, 0, len(want))
        assert (pl.status, pl.stream) == (0, want) and pl.verify() == (OK, NONE, 0, 0)
