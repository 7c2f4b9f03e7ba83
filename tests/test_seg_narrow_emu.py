"""The pipeline schedule of the segmented parser in its own LDS geometry (SgLdsNarrow: a ring of 37 888 bytes
loaded in chunks of 512, 18 slots) on the lane emulation.

tests/emu_pipe_narrow builds the kernel sources with -DZSC_WAVE_EMU at 64 and at 16 lanes and instantiates
sg_pipe_step with the narrow type.  Every ring read and every chunk load asserts the window invariant
(tests/emu_pipe/emu_pipe.cpp, built here with -DPIPE_NARROW), and every run must give the oracle's stage P
(symbols and block records).  The sizes lie around the places where the narrow ring can go wrong: the window, the ring R, the ring and a chunk C, a window
and a ring, two and three rings; the kinds force parsers that give up and redo rounds (zero, runs, bitmap) and a
hand-over at every segment (random).  The cases of tests/parser_cases.py that put a candidate at MAX_DIST and
around slides and segment hand-overs read the oldest byte the floor allows.

In the ring of this geometry the segments rel .. rel + 14 can be in flight (rel the oldest segment that has not
given its slot back) once the window has begun to move; before that, and when the whole input is in the ring, the
18 slots are the bound.  The test prints the largest number seen and the number of polls that found no job, and
asserts that no run ends because no wave finds a job (on the GPU: the idle bound, Z_STREAM_ERROR).
"""
import ctypes as C
import os
import subprocess

import pytest

import parser_cases as P
from zsc_amd import corpus

HERE = os.path.dirname(os.path.abspath(__file__))

KINDS = ("text", "bitmap", "zero", "runs", "table", "random")
LEVELS = (6, 4, 9)
MODES = {0: "round robin", 1: "reverse", 2: "wave 0 only", 3: "every wave but 0", 4: "random"}
# the schedules of a run: ascending hand-out with the most urgent job first (what the GPU's waves do: every size,
# kind and level), the least urgent first (speculative parses as far ahead as the ring allows), one wave alone,
# and seeded random orders
ORDERS = ((0, 0), (1, 0), (2, 0), (4, 1), (4, 2))
ORDERS_LONG = ((0, 0), (1, 0), (4, 1))     # (levels 4 and 9, and the sizes of two rings and more: for the time they take)
WINDOW = 32768
# what sg_pipe_may_load (hi <= R + rel SG_G - window) and sg_pipe_want (hi >= (g + 1) SG_G + SG_OV + 2 MIN_LOOKAHEAD)
# leave: g + 1 - rel segments
IN_FLIGHT = lambda R: (R - WINDOW - (P.SG_OV + 2 * P.MIN_LOOKAHEAD)) // P.SG_G


class Rec(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("sym_begin", "sym_count", "in_begin", "in_len", "stored_ok", "last", "cut", "wend", "at")]


@pytest.fixture(scope="module", params=["libpipe_narrow64.so", "libpipe_narrow16.so"], ids=["wave64", "group16"])
def pipe(request):
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_pipe_narrow")], check=True)
    L = C.CDLL(os.path.join(HERE, "emu_pipe_narrow", request.param))
    L.emu_pipe_open.restype = C.c_void_p
    L.emu_pipe_open.argtypes = [C.c_char_p, C.c_uint32, C.c_int, C.c_int]
    L.emu_pipe_run.argtypes = [C.c_void_p, C.c_int, C.c_uint32]
    L.emu_pipe_figures.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
    L.emu_pipe_parse_result.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(Rec),
                                        C.POINTER(C.c_uint32)]
    L.emu_pipe_close.argtypes = [C.c_void_p]
    L.emu_set_table.argtypes = [C.c_int]
    L.emu_set_stair_min.argtypes = [C.c_uint32]
    L.emu_set_table(0)        # the product's defaults: no match table,
    L.emu_set_stair_min(256)  # chains of 256 entries or more searched as a staircase
    geo = (C.c_uint32 * 4)()
    L.emu_pipe_geometry(geo)
    L.ring, L.chunk, L.slots, L.lds_bytes = geo[0], geo[1], geo[2], geo[3]
    return L


def counter(L, name):
    return C.c_ulonglong.in_dll(L, name).value


def sizes(R, Cc):
    return (3073, WINDOW - 1, WINDOW + 1, R - 1, R, R + 1, R + Cc - 1, R + Cc + 1, WINDOW + R - 1, WINDOW + R + 1,
            2 * R - 1, 2 * R + 1, 3 * R + 257, 200001)


def stage_p(oracle, data, level):
    osy, ons, obl, onb = oracle.parse(data, level)
    syms = [(osy[i].dist << 16) | osy[i].lc for i in range(ons)]
    recs = [(b.sym_begin, b.sym_count, b.in_begin, b.in_len, b.stored_ok, b.last) for b in (obl[i] for i in range(onb))]
    return syms, recs


def run_all(L, data, level, want, orders, what, figures):
    n = len(data)
    for mode, seed in orders:
        ctx = L.emu_pipe_open(data, n, level, 0)
        try:
            here = what + (MODES[mode], seed)
            # 0: finished.  -1: no wave found a job although the buffer is not finished -- what the idle bound
            # ends on the GPU; -4: p_stuck
            assert L.emu_pipe_run(ctx, mode, seed) == 0, here
            syms = (C.c_uint32 * (n + 64))()
            blocks = (Rec * (n // 16383 + 4))()
            ns, nb = C.c_uint32(), C.c_uint32()
            L.emu_pipe_parse_result(ctx, syms, C.byref(ns), blocks, C.byref(nb))
            assert list(syms[:ns.value]) == want[0], here
            got = [(b.sym_begin, b.sym_count, b.in_begin, b.in_len, b.stored_ok, b.last) for b in blocks[:nb.value]]
            assert got == want[1], here
            f = (C.c_ulonglong * 7)()
            L.emu_pipe_figures(ctx, f)
            figures["idle"] += f[4]
            figures["redo"] += f[0]
            figures["in_flight"] = max(figures["in_flight"], f[5])
            figures["in_flight_ring"] = max(figures["in_flight_ring"], f[6])
            figures["runs"] += 1
        finally:
            L.emu_pipe_close(ctx)


def check_invariant(L, figures, bad0, capsys, title):
    bound = IN_FLIGHT(L.ring)
    with capsys.disabled():
        print(f"\n{title}: ring {L.ring} chunk {L.chunk} slots {L.slots} LDS {L.lds_bytes} B; {figures['runs']} runs, "
              f"most segments in flight {figures['in_flight']}, with the window moving {figures['in_flight_ring']} (the ring admits {bound}), redo rounds {figures['redo']}, "
              f"polls that found no job {figures['idle']}, ring reads {counter(L, 'g_pipe_reads')}, "
              f"chunk loads {counter(L, 'g_pipe_loads')}")
    # once the window moves the ring, not the slots, bounds what is in flight -- and a parser two segments past
    # its own still finds slots
    assert 0 < figures["in_flight"] <= L.slots
    assert figures["in_flight_ring"] <= bound <= L.slots - 2
    assert counter(L, "g_pipe_reads") > 0 and counter(L, "g_pipe_loads") > 0
    # the window invariant: no ring read below what the loader promises to keep, no load over a byte in use
    assert (counter(L, "g_pipe_bad_reads"), counter(L, "g_pipe_bad_loads")) == bad0 == (0, 0)


def test_geometry_fits_four_workgroups(pipe):
    assert (pipe.ring, pipe.chunk, pipe.slots) == (37888, 512, 18)
    assert pipe.ring % pipe.chunk == 0 and pipe.lds_bytes <= 40960     # four in a CU's 160 KiB
    assert IN_FLIGHT(pipe.ring) == 15


def test_sizes_around_the_ring_give_the_serial_parse(pipe, oracle, capsys):
    bad0 = counter(pipe, "g_pipe_bad_reads"), counter(pipe, "g_pipe_bad_loads")
    figures = {"idle": 0, "redo": 0, "in_flight": 0, "in_flight_ring": 0, "runs": 0}
    R, Cc = pipe.ring, pipe.chunk
    for n in sizes(R, Cc):
        for kind in KINDS:
            data = corpus.make_buffer(kind, n, n + 17)
            for level in LEVELS:
                want = stage_p(oracle, data, level)
                orders = ORDERS if n < 2 * R - 1 and level == 6 else ORDERS_LONG
                run_all(pipe, data, level, want, orders, (kind, n, level), figures)
    assert figures["redo"] > 0          # (zero, runs and bitmap: parsers that give up)
    check_invariant(pipe, figures, bad0, capsys, "sizes around the ring")


def edge_cases():
    """the cases that read the oldest byte the floor allows (a candidate at MAX_DIST and next to it, at and around
    window slides) and those around segment hand-overs, as far as the narrow entry takes them: the segmented
    parser at window_bits 15, mem_level 8"""
    out = [c for c in P.cases() if c.segmented and abs(c.window_bits) == 15 and c.mem_level == 8 and c.strategy == P.DEFAULT
           and c.family in "AGF" and 4 <= c.level <= 9]
    assert sum(c.family == "A" for c in out) >= 10 and sum(c.family == "G" for c in out) >= 10
    return out


def test_edges_of_the_window_and_the_hand_overs(pipe, oracle, capsys):
    bad0 = counter(pipe, "g_pipe_bad_reads"), counter(pipe, "g_pipe_bad_loads")
    figures = {"idle": 0, "redo": 0, "in_flight": 0, "in_flight_ring": 0, "runs": 0}
    for c in edge_cases():
        want = stage_p(oracle, c.data, c.level)
        run_all(pipe, c.data, c.level, want, ORDERS, (c.name, len(c.data), c.level), figures)
    check_invariant(pipe, figures, bad0, capsys, "parser edge cases")
