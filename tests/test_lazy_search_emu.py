"""Lazy searches that cannot win (zsc_amd/csrc/lz_parse_seg.h: SG_LAZY_FILTER, SG_EMPTY_SKIP) on the lane emulation.

tests/emu_lazy builds the kernel sources with -DZSC_WAVE_EMU twice, with both parts switched on and with
both off, at 64 and at 16 lanes per wave.  Every buffer goes through the segmented parser of both builds and
must come out as the oracle's stream byte for byte (64 lanes: the whole stream; 16 lanes: the symbols and block
records, since the kernels behind the parser are whole-wave code).  The counters are printed; what is asserted
of them is only what the construction gives: the build with the parts on never searches, passes, steps or
long-compares more than the one without, and on 64 KiB of text and of table data strictly fewer passes reach
their first compare step.
"""
import ctypes as C
import os
import subprocess

import pytest

from zsc_amd import corpus

HERE = os.path.dirname(os.path.abspath(__file__))

Z_FILTERED = 1
KINDS = ("text", "table", "bitmap", "random", "zero")
# just above the segmented parser's threshold, the tile's edge (chains continue in the previous tile), the first
# slide of the window
SIZES = (3073, 4099, 32767, 32768, 32769, 40000, 65537, 70001)
LEVELS = (4, 5, 6, 7, 8, 9)
# what the counters are called in the output: (array, index)
COUNTERS = {"searches": ("g_sg_cnt", 5), "passes": ("g_sg_cnt", 12), "long compares": ("g_sg_cnt", 1),
            "skipped by the empty-chain test": ("g_sg_cnt", 9), "passes entered with best >= 4": ("g_lazy_cnt", 0),
            "passes ended early": ("g_lazy_cnt", 1), "compare steps": ("g_lazy_cnt", 2),
            "passes reaching a compare step": ("g_lazy_cnt", 3)}
NEVER_MORE = ("searches", "passes", "compare steps", "long compares", "passes reaching a compare step")


class Rec(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("sym_begin", "sym_count", "in_begin", "in_len", "stored_ok", "last", "cut", "wend", "at")]


def load(name):
    L = C.CDLL(os.path.join(HERE, "emu_lazy", name))
    L.emu_compress.argtypes = [C.c_char_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.emu_parse.argtypes = [C.c_char_p, C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                            C.POINTER(Rec), C.POINTER(C.c_uint32)]
    L.emu_set_params.argtypes = [C.c_int, C.c_int]
    L.emu_set_stair_min.argtypes = [C.c_uint32]
    L.emu_set_table(0)        # the product's defaults: no match table,
    L.emu_set_stair_min(256)  # chains of 256 entries or more searched as a staircase,
    L.emu_set_seg_mode(2)     # and every buffer here to the segmented parser, as the runtime sends them
    return L


@pytest.fixture(scope="module", params=["64", "16"], ids=["wave64", "group16"])
def builds(request):
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_lazy")], check=True)
    on, off = load(f"liblazy_on{request.param}.so"), load(f"liblazy_off{request.param}.so")
    on.wide = off.wide = request.param == "64"
    return on, off


def counters(L):
    out = {}
    for name, (arr, i) in COUNTERS.items():
        out[name] = (C.c_ulonglong * 16).in_dll(L, arr)[i] if arr == "g_sg_cnt" else (C.c_ulonglong * 4).in_dll(L, arr)[i]
    return out


def run(L, oracle, want, data, level, strategy, wbits, mem_level, what):
    """one buffer through one build: the oracle's stream (or stage P), and the counters of the run"""
    n = len(data)
    L.emu_set_params(wbits, mem_level)
    L.emu_lazy_reset()
    try:
        if L.wide:
            cap = n + (n >> 3) + 256
            out, ol = C.create_string_buffer(cap), C.c_uint32()
            assert L.emu_compress(data, n, level, 1, strategy, out, cap, C.byref(ol)) == 0, what
            assert out.raw[:ol.value] == want["stream"], what
        else:
            syms = (C.c_uint32 * (n + 64))()
            blocks = (Rec * (n // ((1 << (mem_level + 6)) - 1) + 4))()
            ns, nb = C.c_uint32(), C.c_uint32()
            assert L.emu_parse(data, n, level, strategy, syms, C.byref(ns), blocks, C.byref(nb)) == 0, what
            assert list(syms[:ns.value]) == want["syms"], what
            got = [(b.sym_begin, b.sym_count, b.in_begin, b.in_len, b.stored_ok, b.last) for b in blocks[:nb.value]]
            assert got == want["recs"], what
    finally:
        L.emu_set_params(15, 8)
    return counters(L)


def expected(oracle, wide, data, level, strategy, wbits, mem_level):
    if wide:
        rc, stream, _ = oracle.compress(data, level, window_bits=wbits, mem_level=mem_level, strategy=strategy)
        assert rc == 0
        return {"stream": stream}
    osy, ons, obl, onb = oracle.parse(data, level, wbits, mem_level, strategy)
    return {"syms": [(osy[i].dist << 16) | osy[i].lc for i in range(ons)],
            "recs": [(b.sym_begin, b.sym_count, b.in_begin, b.in_len, b.stored_ok, b.last) for b in (obl[i] for i in range(onb))]}


def both(builds, oracle, data, level, strategy=0, wbits=15, mem_level=8, what=None):
    """both builds give the oracle's result, and the one with the parts on never does more of anything"""
    on, off = builds
    want = expected(oracle, on.wide, data, level, strategy, wbits, mem_level)
    c_on = run(on, oracle, want, data, level, strategy, wbits, mem_level, (what, "on"))
    c_off = run(off, oracle, want, data, level, strategy, wbits, mem_level, (what, "off"))
    for k in NEVER_MORE:
        assert c_on[k] <= c_off[k], (what, k, c_on, c_off)
    assert c_off["skipped by the empty-chain test"] == c_off["passes ended early"] == c_off["passes entered with best >= 4"] == 0
    return c_on, c_off


def add(total, c):
    for k, v in c.items():
        total[k] = total.get(k, 0) + v


def tail_buffer():
    """text whose last 300 bytes repeat an earlier stretch: a pending match reaches the end of the data
    (cap <= best, nice cut to the lookahead)"""
    t = corpus.make_buffer("text", 9000, 3)
    return t[:8700] + t[2000:2300]


def cache_end_buffer():
    """text whose last 40 bytes repeat an earlier stretch: matches are pending while the register cache of 64
    positions holds the last positions that own a trigram, and those behind them that own none"""
    t = corpus.make_buffer("text", 5000, 4)
    return t[:4960] + t[1000:1040]


def test_every_kind_size_level_and_strategy(builds, oracle, capsys):
    sums = {}
    for kind in KINDS:
        for n in SIZES:
            data = corpus.make_buffer(kind, n, n + 5)
            for level in LEVELS:
                for strategy in (0, Z_FILTERED):
                    c_on, c_off = both(builds, oracle, data, level, strategy, what=(kind, n, level, strategy))
                    if level == 4:  # max_lazy is 4: no search with four bytes or more pending, the filter has nothing to do
                        assert c_on["passes entered with best >= 4"] == 0, (kind, n, strategy)
                    add(sums.setdefault((kind, "on"), {}), c_on)
                    add(sums.setdefault((kind, "off"), {}), c_off)
    with capsys.disabled():
        print()
        for (kind, which), c in sums.items():
            print(f"lazy searches [{'wave64' if builds[0].wide else 'group16'}] {kind} {which}: " + ", ".join(f"{k} {v}" for k, v in c.items()))
    # the levels above 4 do have such passes, each with its own good_length / max_lazy / nice_match
    assert sums[("text", "on")]["passes entered with best >= 4"] > 0 and sums[("text", "on")]["passes ended early"] > 0


def test_small_window_and_hash(builds, oracle):
    """window_bits 12 / mem_level 5: the generic instantiation, where the lane-parallel search is off and only
    the empty-chain test acts"""
    for kind in KINDS:
        for n in (3073, 4099, 40000):
            data = corpus.make_buffer(kind, n, n + 5)
            for level in (6, 9):
                c_on, _ = both(builds, oracle, data, level, 0, 12, 5, what=(kind, n, level, "wbits 12 mem_level 5"))
                assert c_on["passes"] == 0, (kind, n, level)


def test_pending_match_at_the_end_of_the_data(builds, oracle):
    for data, name in ((tail_buffer(), "tail of 300"), (cache_end_buffer(), "tail of 40")):
        assert len(data) > 3072
        for level in LEVELS:
            for strategy in (0, Z_FILTERED):
                both(builds, oracle, data, level, strategy, what=(name, level, strategy))


def test_fewer_passes_reach_a_compare_step_on_text_and_table(builds, oracle, capsys):
    lines = []
    for kind in ("text", "table"):
        data = corpus.make_buffer(kind, 65536, 1)
        c_on, c_off = both(builds, oracle, data, 6, what=(kind, 65536))
        lines.append(f"lazy searches 64 KiB {kind} L6: on  " + ", ".join(f"{k} {v}" for k, v in c_on.items()))
        lines.append(f"lazy searches 64 KiB {kind} L6: off " + ", ".join(f"{k} {v}" for k, v in c_off.items()))
        assert c_on["passes reaching a compare step"] < c_off["passes reaching a compare step"], (kind, c_on, c_off)
    with capsys.disabled():
        print()
        for ln in lines:
            print(ln)
