"""A deflate plan with something other than zeros around its buffers (tests/surroundings.py).

One buffer of about 120 KB -- text, a period-7 run, zeros, text again -- is cut into consecutive pieces of 16,
48, 272, 3072 (the largest the wave-per-buffer parser takes), 3088 (the first for the segmented one), 32784,
40000 bytes and the rest.  In the plan's own layout the device input is then the long buffer itself: every
piece is followed by its true continuation and preceded by its true past, and matches exist across every
boundary in both directions.  A second cut has lengths that are no multiples of 16; the gaps of 1 to 15 bytes
hold the piece's continuation.  The control is the same pieces 64 bytes and more apart with zeros between
them; every stream must be oracle.compress(piece, ...) under every filler.

The output is full of 0xFF, with the layout's capacities, with capacities of exactly the oracle's stream
length (every residue mod 4: tests/test_surroundings_cases.py) and with one byte less (Z_BUF_ERROR, nothing
asserted inside the slot), and no byte outside [out_offsets[i], + out_caps[i]) may change.
"""
import pytest

import surroundings as sr

pytestmark = pytest.mark.gpu

CUTS = (sr.PIECES_16, sr.PIECES_ODD)


def abutting(items):
    """the plan's own layout: io += (n + 15) & ~15"""
    offs, at = [], 0
    for it in items:
        offs.append(at)
        at += sr.round16(len(it.data))
    return offs, at + sr.TAIL


@pytest.mark.parametrize("level,wbits,strategy", sr.DEFLATE_PLANS)
def test_streams_depend_on_the_pieces_own_bytes_only(oracle, level, wbits, strategy):
    import torch
    for lengths in CUTS:
        items = sr.pieces(lengths)
        lens = [len(it.data) for it in items]
        wants = [(0, s) for s in sr.want_deflate(oracle, items, level, wbits, strategy)]
        names = [it.name for it in items]
        spread, spread_bytes = sr.spread_offsets(items)
        own, own_bytes = abutting(items)

        def run(filler, offsets=spread, nbytes=spread_bytes, custom=True):
            plan = sr.make_deflate_plan(lens, level, wbits, strategy, in_offsets=offsets if custom else None)
            try:
                assert plan.in_offsets == offsets and plan.in_bytes <= nbytes
                return sr.run_deflate(torch, plan, sr.place(items, offsets, nbytes, filler), verify=True)
            finally:
                plan.close()

        sr.under_fillers(names, wants, run)
        # the plan's own layout: the pieces abut (or nearly), and what lies between and behind them is the truth
        sr.under_fillers(names, wants, lambda filler: run(filler if filler == "zeros" else "continuation", own, own_bytes, False),
                         fillers=("zeros", "continuation"))
        if lengths is sr.PIECES_16:
            assert sr.place(items, own, own_bytes, "continuation").tobytes() == sr.long_buffer()


@pytest.mark.parametrize("level,wbits,strategy", sr.DEFLATE_PLANS)
def test_exact_capacities_and_one_byte_less(oracle, level, wbits, strategy):
    """out_caps of exactly the stream's length: the stream is the oracle's and the bytes behind it, which the
    next word of the output holds, stay as they were.  One byte less: Z_BUF_ERROR, as the oracle reports it"""
    import torch
    for lengths in CUTS:
        items = sr.pieces(lengths)
        lens = [len(it.data) for it in items]
        streams = sr.want_deflate(oracle, items, level, wbits, strategy)
        own, own_bytes = abutting(items)
        image = sr.place(items, own, own_bytes, "continuation")
        for less in (0, 1):
            caps = [len(s) - less for s in streams]
            wants = [(sr.Z_BUF_ERROR, b"")] * len(items) if less else [(0, s) for s in streams]
            plan = sr.make_deflate_plan(lens, level, wbits, strategy, out_caps=caps)
            try:
                assert plan.out_caps == caps and plan.in_offsets == own
                got = sr.run_deflate(torch, plan, image, verify=not less)
            finally:
                plan.close()
            assert got[len(items):] == [None] * (1 if less else 2), (less, got[len(items):])
            for it, g, w in zip(items, got, wants):
                assert g == w, (it.name, less, sr.brief(g), sr.brief(w))


def test_sections_of_abutting_pieces(oracle):
    """zsc_hip_compress_sections_device with the caller's in_offsets: the pieces abut in the long buffer, and
    max_block_len is below the piece length, so every piece is a stream of sections with joints between them"""
    import torch
    import zsc_amd
    items = sr.pieces(sr.PIECES_16)[3:]
    lens = [len(it.data) for it in items]
    mbls = [1024, 2048, 8192, 16384, 4096]
    assert len(mbls) == len(items) and all(m < n for m, n in zip(mbls, lens))
    at = sum(len(it.data) for it in sr.pieces(sr.PIECES_16)[:3])
    in_offsets, o = [], at
    for n in lens:
        in_offsets.append(o)
        o += n
    assert all(x % 16 == 0 for x in in_offsets) and o == sr.LONG
    wants = []
    for it, m in zip(items, mbls):
        rc, s, unsupported = oracle.compress(it.data, 6, max_block_len=m)
        assert rc == 0 and not unsupported and s.count(b"\x00\x00\xff\xff") >= 1
        wants.append(s)
    caps = [oracle.max_output(n, m, 6)[1] for n, m in zip(lens, mbls)]
    out_offsets, o = [], 48
    for c in caps:
        out_offsets.append(o)
        o += sr.round16(c) + 32
    src = torch.frombuffer(bytearray(sr.long_buffer()), dtype=torch.uint8).cuda()
    dst = sr.canary_image(torch, o + sr.TAIL, 0xFF)
    torch.cuda.synchronize()
    rc, got_lens, stat = zsc_amd.compress_sections_device(src.data_ptr(), in_offsets, lens, mbls, dst.data_ptr(), out_offsets,
                                                          caps, 6)
    assert rc == 0 and stat == [0] * len(items)
    host = dst.cpu().numpy()
    for it, off, n, w in zip(items, out_offsets, got_lens, wants):
        assert host[off:off + n].tobytes() == w, it.name
    sr.assert_outside_untouched(host, out_offsets, caps, 0xFF)
