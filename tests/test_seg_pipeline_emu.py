"""The pipeline schedule of the segmented parser (zsc_amd/csrc/lz_parse_pipe.h) on the lane emulation.

tests/emu_pipe builds the kernel sources with -DZSC_WAVE_EMU at 64 and at 16 lanes.  A job of the pipeline
(redo, resolve, load, parse) never waits inside, so any order in which the waves ask for jobs is a legal
schedule: the driver offers jobs in the order the test chooses and every order must give the oracle's
stage P (symbols, block records) and, at 64 lanes, the whole stream.  Two hooks that are empty in the
product check the window invariant on every ring read and every chunk load (emu_pipe.cpp).
"""
import ctypes as C
import os
import subprocess

import pytest

from zsc_amd import corpus

HERE = os.path.dirname(os.path.abspath(__file__))

DONE, WORKED, IDLE = 0, 1, 2
KINDS = ("text", "bitmap", "zero", "runs", "table", "random")
# the sizes of test_segmented_parser_hand_over_orders and the edges of segments, groups of them and chunks;
# 140 000 is more than three rings (135 168): every ring byte is overwritten more than once
SIZES = (0, 3, 255, 256, 257, 1025, 4095, 4096, 4097, 8191, 8193, 40000, 70000, 140000)
RANDOM_ORDERS = 20
RANDOM_ORDERS_LONG = 4
MODES = {0: "round robin", 1: "reverse", 2: "wave 0 only", 3: "every wave but 0"}


class Rec(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("sym_begin", "sym_count", "in_begin", "in_len", "stored_ok", "last", "cut", "wend", "at")]


@pytest.fixture(scope="module", params=["libpipe_emu64.so", "libpipe_emu16.so"], ids=["wave64", "group16"])
def pipe(request):
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_pipe")], check=True)
    L = C.CDLL(os.path.join(HERE, "emu_pipe", request.param))
    L.wide = request.param.endswith("64.so")
    L.emu_pipe_open.restype = C.c_void_p
    L.emu_pipe_open.argtypes = [C.c_char_p, C.c_uint32, C.c_int, C.c_int]
    L.emu_pipe_step.argtypes = [C.c_void_p, C.c_int, C.c_uint32]
    L.emu_pipe_run.argtypes = [C.c_void_p, C.c_int, C.c_uint32]
    L.emu_pipe_jobs.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
    L.emu_pipe_parse_result.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(Rec),
                                        C.POINTER(C.c_uint32)]
    L.emu_pipe_stream.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.emu_pipe_close.argtypes = [C.c_void_p]
    L.emu_set_table.argtypes = [C.c_int]
    L.emu_set_stair_min.argtypes = [C.c_uint32]
    L.emu_set_table(0)        # the product's defaults: no match table,
    L.emu_set_stair_min(256)  # chains of 256 entries or more searched as a staircase
    return L


def counter(L, name):
    return C.c_ulonglong.in_dll(L, name).value


def stage_p(oracle, data, level):
    osy, ons, obl, onb = oracle.parse(data, level)
    syms = [(osy[i].dist << 16) | osy[i].lc for i in range(ons)]
    recs = [(b.sym_begin, b.sym_count, b.in_begin, b.in_len, b.stored_ok, b.last) for b in (obl[i] for i in range(onb))]
    return syms, recs


def check_run(L, ctx, data, want_p, want_stream, what):
    n = len(data)
    syms = (C.c_uint32 * (n + 64))()
    blocks = (Rec * (n // 16383 + 4))()
    ns, nb = C.c_uint32(), C.c_uint32()
    L.emu_pipe_parse_result(ctx, syms, C.byref(ns), blocks, C.byref(nb))
    assert list(syms[:ns.value]) == want_p[0], what
    got = [(b.sym_begin, b.sym_count, b.in_begin, b.in_len, b.stored_ok, b.last) for b in blocks[:nb.value]]
    assert got == want_p[1], what
    if L.wide:  # (the Huffman and bit-packing kernels behind the parser are whole-wave code)
        cap = n + (n >> 3) + 256
        out = C.create_string_buffer(cap)
        ol = C.c_uint32()
        assert L.emu_pipe_stream(ctx, 1, out, cap, C.byref(ol)) == 0, what
        assert out.raw[:ol.value] == want_stream, what


def test_every_schedule_gives_the_serial_parse(pipe, oracle):
    """Round robin, reverse (parses run as far ahead as slots and window allow), wave 0 alone (no job
    needs a second wave: the design cannot deadlock on a wave that is busy or late), every wave but 0,
    and seeded random orders; all kinds and sizes, levels 4, 6 and 9."""
    bad0 = counter(pipe, "g_pipe_bad_reads"), counter(pipe, "g_pipe_bad_loads")
    for n in SIZES:
        for kind in KINDS:
            data = corpus.make_buffer(kind, n, n + 17)
            for level in (6, 9, 4):
                want_p = stage_p(oracle, data, level)
                want_stream = oracle.compress(data, level)[1]
                # (levels 4 and 9 on the buffers of more than a ring: fewer random orders, for the time they take)
                nrand = RANDOM_ORDERS if level == 6 or n <= 40000 else RANDOM_ORDERS_LONG
                orders = [(m, 0) for m in MODES] + [(4, s + 1) for s in range(nrand)]
                for mode, seed in orders:
                    ctx = pipe.emu_pipe_open(data, n, level, 0)
                    try:
                        what = (kind, n, level, MODES.get(mode, "random"), seed)
                        assert pipe.emu_pipe_run(ctx, mode, seed) == 0, what
                        check_run(pipe, ctx, data, want_p, want_stream, what)
                    finally:
                        pipe.emu_pipe_close(ctx)
    assert counter(pipe, "g_pipe_reads") > 0
    # (reads behind the ring's data happen, at the end of the input only: the hook counts any other as bad)
    print("ring reads", counter(pipe, "g_pipe_reads"), "of them behind the loaded input", counter(pipe, "g_pipe_reads_ahead"))
    # the window invariant: no ring read below what the loader promises to keep, no load over a byte in use
    assert (counter(pipe, "g_pipe_bad_reads"), counter(pipe, "g_pipe_bad_loads")) == bad0 == (0, 0)


def test_steps_one_at_a_time(pipe, oracle):
    """The exported step itself, wave by wave from Python: a wave that is only ever offered one kind of job
    (wave w: kind w % 4) plus one wave that takes anything; and the match table switched on."""
    for table in (0, 1):
        pipe.emu_set_table(table)
        try:
            for kind, n in (("text", 70000), ("bitmap", 50000), ("runs", 20000)):
                data = corpus.make_buffer(kind, n, 5)
                ctx = pipe.emu_pipe_open(data, n, 6, 0)
                try:
                    idle_rounds = 0
                    for _ in range(100000):
                        results = [pipe.emu_pipe_step(ctx, w, 1 << (w % 4)) for w in range(7)]
                        results.append(pipe.emu_pipe_step(ctx, 7, 15))
                        if DONE in results:
                            break
                        idle_rounds = idle_rounds + 1 if all(r == IDLE for r in results) else 0
                        assert idle_rounds < 2, (kind, n, "no job is ready and the buffer is not finished")
                    else:
                        pytest.fail("the pipeline did not finish")
                    jobs = (C.c_ulonglong * 4)()
                    pipe.emu_pipe_jobs(ctx, jobs)
                    # (the last segments need no speculative parse when a parse from an exact state reaches the end)
                    assert 0 < jobs[3] <= (n + 255) // 256 and jobs[2] == (n + 2047) // 2048 and jobs[1] > 0
                    check_run(pipe, ctx, data, stage_p(oracle, data, 6), oracle.compress(data, 6)[1], (kind, n, table))
                finally:
                    pipe.emu_pipe_close(ctx)
        finally:
            pipe.emu_set_table(0)


# ---- the model figure (printed and recorded, never asserted) ---------------------------------------------
#
# Costs are in candidate batches as the emulation logs them per parsed segment (g_sg_log), plus 8 per
# segment for its loop (tools/seg_stats.py).  The serial work is priced in the same unit, by assumption:
# LOAD per 2 KiB chunk of the window, RESOLVE per segment resolved (about 1.2 trips of 64 tokens).
LOAD, RESOLVE, SEG = 4, 2, 8


def seg_log(L):
    log = (C.c_uint * (1 << 20)).in_dll(L, "g_sg_log")
    n = C.c_uint.in_dll(L, "g_sg_nlog")
    recs = [(log[i], log[i + 1]) for i in range(0, n.value, 2)]
    C.c_uint.in_dll(L, "g_sg_nlog").value = 0
    return recs


def split_steps(recs):
    """the records of a super-step run, step by step: {"q": [(segment, cost)], "redo": [(segment, cost)]}"""
    steps, cur, prev = [], None, -1
    for seg, b in recs:
        redo, sgn = seg >= 0x10000, seg & 0xffff
        if not redo and (cur is None or sgn > prev or cur["redo"]):
            cur = {"q": [], "redo": []}
            steps.append(cur)
        if redo:
            cur["redo"].append((sgn, b))
        else:
            cur["q"].append((sgn, b))
            prev = sgn
    return steps


def super_step_length(recs, waves=8):
    """phase by phase: window (one wave), parse (list scheduling in hand-out order, then the barrier),
    resolve (one wave); a redo round is one wave parsing and one wave resolving"""
    total = 0
    for s in split_steps(recs):
        t = [0] * waves
        for _, c in s["q"]:
            i = t.index(min(t))
            t[i] += c + SEG
        total += LOAD * ((len(s["q"]) + 7) // 8) + max(t) + RESOLVE * len(s["q"])
        total += sum(c + SEG + RESOLVE for _, c in s["redo"])
    return total


def as_one_buffer(recs):
    """the same records with the segments numbered through the buffer, in ascending order: what the
    pipeline hands out.  (The costs are those of parsers that found their successors' traces, as on the
    GPU, where the successor runs at the same time; the job-atomic emulation of the pipeline itself never
    has a successor's trace in time and would only model a serial parse.)"""
    out = []
    for i, s in enumerate(split_steps(recs)):
        out += sorted((i * 32 + g, c) for g, c in s["q"])
        out += [(0x10000 + i * 32 + g, c) for g, c in s["redo"]]
    return out


def pipeline_length(recs, waves=8, slots=32):
    """event by event: a free wave takes the redo, the resolver, a chunk load or the next segment, in that
    order, as sg_pipe_step does; the resolver stops at a segment that is to be parsed again"""
    spec = [b for seg, b in recs if seg < 0x10000]
    redo = {}
    for seg, b in recs:
        if seg >= 0x10000:
            redo.setdefault(seg & 0xffff, []).append(b)
    nseg = len(spec)
    free = [0] * waves
    parse_done = [None] * nseg
    nxt = resolved = loaded = 0     # next segment to hand out, segments resolved, segments the window covers
    res_busy_until = redo_busy_until = load_busy_until = 0
    pending_redo = None
    while resolved < nseg:
        w = free.index(min(free))
        t = free[w]
        done = lambda g: parse_done[g] is not None and parse_done[g] <= t
        if pending_redo is not None and redo_busy_until <= t and res_busy_until <= t and done(pending_redo[0]):
            g, c = pending_redo
            pending_redo = None
            free[w] = redo_busy_until = t + c + SEG
            redo[g].pop(0)
            continue
        if pending_redo is None and res_busy_until <= t and redo_busy_until <= t and resolved < nseg and done(resolved):
            k = resolved
            cost = 0
            while k < nseg and done(k):
                if redo.get(k):
                    pending_redo = (k, redo[k][0])
                    break
                cost += RESOLVE
                k += 1
            if k > resolved or pending_redo:
                resolved = k
                free[w] = res_busy_until = t + max(cost, 1)
                continue
        if load_busy_until <= t and loaded < nseg and loaded < resolved + slots + 8 and loaded < nxt + 16:
            loaded += 8
            free[w] = load_busy_until = t + LOAD
            continue
        if nxt < nseg and nxt < resolved + slots and nxt < loaded:
            parse_done[nxt] = free[w] = t + spec[nxt] + SEG
            nxt += 1
            continue
        later = [x for x in free + [res_busy_until, redo_busy_until, load_busy_until] if x > t]
        free[w] = min(later) if later else t + 1
    return max(max(free), res_busy_until)


def test_model_of_the_two_schedules(pipe, oracle, capsys):
    """The length of the pipelined schedule against the super-step schedule on 8 waves for 512 KiB of text,
    table and bitmap, both with their serial work, from the per-segment costs of the emulation.  A figure
    for the record, not a check."""
    if not pipe.wide:
        return  # (the model is worked out once, from the 64-lane costs)
    E = C.CDLL(os.path.join(HERE, "emu", "libzsc_emu.so"))
    lines = []
    for kind in ("text", "table", "bitmap"):
        n = 512 * 1024
        data = corpus.make_buffer(kind, n, 1)
        cap = n + (n >> 3) + 256
        out, ol = C.create_string_buffer(cap), C.c_uint32()
        E.emu_set_seg_mode(2)
        C.c_uint.in_dll(E, "g_sg_nlog").value = 0
        E.emu_set_table(0)        # the product's defaults, as tools/seg_stats.py
        E.emu_set_stair_min(256)
        try:
            assert E.emu_compress(data, n, 6, 1, 0, out, cap, C.byref(ol)) == 0
        finally:  # (the library is the one tests/test_emu_kernels.py uses: leave it as it was loaded)
            E.emu_set_seg_mode(0)
            E.emu_set_table(1)
            E.emu_set_stair_min(0)
        recs = seg_log(E)
        ss = super_step_length(recs)
        pl = pipeline_length(as_one_buffer(recs))
        serial = sum(b + SEG for _, b in recs)
        lines.append(f"model {kind} 512 KiB L6: super-steps {ss}  pipeline {pl}  ratio {ss / pl:.3f}  "
                     f"(all parses on one wave {serial}, re-parsed segments {sum(1 for s, _ in recs if s >= 0x10000)})")
    with capsys.disabled():
        print()
        for ln in lines:
            print(ln)
