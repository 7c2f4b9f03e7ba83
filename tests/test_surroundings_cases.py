"""The case lists of tests/surroundings.py against the oracle alone, so that a failure of the GPU tests that
use them cannot be a bad case: every class of cut is there and lands where its name says, the statuses and
the residue classes are complete, and the images put every byte where the filler says."""
import numpy as np
import pytest

import deflate_cases as dc
import surroundings as sr
from test_inflate_members_emu import walk


def _inflated(oracle, s, wbits):
    rc, out, used = oracle.uncompress(s, 1 << 20, window_bits=wbits)
    return rc, out, used


@pytest.mark.parametrize("wbits", sr.WRAPPERS)
def test_inflate_cases_are_what_their_names_say(oracle, wbits):
    items = sr.inflate_cases(oracle, wbits)
    by = {it.name: it for it in items}
    assert len(by) == len(items) and 20 <= len(items) <= 48
    classes = {it.what for it in items}
    want = {"clean", "damaged", "inside-code", "length-distance", "stored", "marker", "block-header", "cap"}
    if wbits != -15:
        want |= {"header", "trailer-1", "trailer-2", "trailer-3"}
    if wbits == sr.GZ:
        want |= {"member-0", "member-1", "member-2", "member-3"}
    assert classes == want
    results = {it.name: oracle.uncompress(it.data, it.cap, window_bits=wbits) for it in items}
    # clean streams: status 0, all consumed, outputs of 0, 1, 300 and a few thousand bytes, every residue
    clean = [it for it in items if it.what == "clean"]
    for it in clean:
        rc, out, used = results[it.name]
        assert (rc, len(out), used) == (0, it.cap, len(it.data)), it.name
    assert {0, 1, 300} <= {it.cap for it in clean} and any(3000 <= it.cap < 4000 for it in clean)
    assert {len(it.data) % 4 for it in clean if it.name.startswith("clean-text")} == {0, 1, 2, 3}
    big = by["clean-noise-three-chunks"]
    assert 3 * sr.CHUNK < len(big.data) < 3 * sr.CHUNK + 256 and max(len(it.data) for it in items) < 3 * sr.CHUNK + 512
    # cut streams: the whole stream is sound, the cut one is not Z_OK, and the truth lies behind the cut
    cut = [it for it in items if it.name.startswith("cut-")]
    assert {len(it.data) % 4 for it in cut} == {0, 1, 2, 3}
    for it in cut:
        whole = it.data + it.behind
        rc, out, used = _inflated(oracle, whole, wbits)
        assert rc == 0 and len(it.behind) >= min(64, len(whole) - len(it.data)) and len(it.behind) > 0, it.name
        if not it.what.startswith("member-"):
            assert results[it.name][0] != 0 and used > len(it.data), (it.name, results[it.name][0])
    hdr = dc.body_offset(by["clean-1"].data, wbits)
    if wbits != -15:
        assert 0 < len(by["cut-in-header"].data) < hdr
        for short in (1, 2, 3):
            it = by[f"cut-trailer-{short}-short"]
            rc, out, used = _inflated(oracle, it.data + it.behind, wbits)
            assert used - len(it.data) == short and len(it.behind) == short and results[it.name][1] == out
    # inside a literal's code; between a length code and its distance: found again with the stream reader
    text_stream = by["cap-one-short"].data
    tokens = []
    (block,), _, _ = dc.walk(text_stream, wbits, tokens)
    spans = list(zip(tokens, block.sym_pos, block.sym_bits))
    for it in (i for i in items if i.what == "inside-code"):
        k = len(it.data)
        assert text_stream[:k] == it.data
        hit = [(t, p, nb) for t, p, nb in spans if p < 8 * k < p + nb]
        assert len(hit) == 1 and hit[0][0][2] == 0 and hit[0][0][1] == 1, it.name  # a literal, cut inside its code
    it = by["cut-between-length-and-distance"]
    k = len(it.data)
    (t, p, nb), = [(t, p, nb) for t, p, nb in spans if p < 8 * k < p + nb]
    assert t[2] > 0  # a copy: the boundary is behind its length code and extra bits, before its distance code
    sym = sr._length_symbol(t[1])
    assert p + block.lit_lens[sym] + dc.LEN_EXTRA[sym - 257] == 8 * k
    # stored data with LEN reaching past the cut
    it = by["cut-in-stored-data"]
    (sb,), _, _ = dc.walk(it.data + it.behind, wbits)
    data_at = (sb.end_bit >> 3) - sb.stored_len
    assert sb.type == 0 and data_at < len(it.data) < data_at + sb.stored_len
    # the marker, the members and the block header lie right behind their cuts
    assert by["cut-before-flush-marker"].behind[:4] == b"\x00\x00\xff\xff" and len(by["cut-before-flush-marker"].behind) > 1000
    if wbits == sr.GZ:
        first = _inflated(oracle, by["cut-0-into-next-member"].data + by["cut-0-into-next-member"].behind, wbits)[2]
        for into in range(4):
            it = by[f"cut-{into}-into-next-member"]
            assert len(it.data) == first + into and (it.data + it.behind)[first:first + 3] == b"\x1f\x8b\x08"
            assert results[it.name] == results["cut-0-into-next-member"] and results[it.name][0] == 0
    it = by["cut-before-dynamic-header-in-last-chunk"]
    whole = by["clean-many-blocks-three-chunks"].data
    assert whole[:len(it.data)] == it.data and len(whole) > 3 * sr.CHUNK < len(it.data)
    blocks, _, _ = dc.walk(whole, wbits)
    assert len(blocks) > 8 and any(b.type == 2 and b.first_bit >> 3 == len(it.data) for b in blocks)
    # short capacities
    for name in ("cap-one-short", "cap-half", "cap-half-noise"):
        rc, out, _ = results[name]
        assert rc == sr.Z_BUF_ERROR and len(out) == by[name].cap, name
    assert {r[0] for r in results.values()} == {0, sr.Z_DATA_ERROR, sr.Z_BUF_ERROR}


def test_statuses_0_data_error_and_buf_error_all_occur(oracle):
    seen = set()
    for wbits in sr.WRAPPERS:
        seen |= {oracle.uncompress(it.data, it.cap, window_bits=wbits)[0] for it in sr.inflate_cases(oracle, wbits)}
    seen |= {walk(oracle, it.data, it.cap)[0] for it in sr.member_cases(oracle)}
    assert seen >= {0, sr.Z_DATA_ERROR, sr.Z_BUF_ERROR}, seen


def test_member_cuts_land_where_they_say(oracle):
    items = sr.member_cases(oracle)
    by = {it.name: it for it in items}
    assert len(by) == len(items)
    whole = by["cut-0-into-member-1"].data + by["cut-0-into-member-1"].behind
    rc, out, used, members = walk(oracle, whole, len(out_of(oracle, whole)))
    assert (rc, members, used) == (0, 4, len(whole))
    first = oracle.uncompress(whole, 1 << 20, window_bits=sr.GZ)[2]
    for into in range(4):
        it = by[f"cut-{into}-into-member-1"]
        assert len(it.data) == first + into and it.behind[:3 - into] == b"\x1f\x8b\x08"[into:]
        rc, out, used, members = walk(oracle, it.data, it.cap)
        # (the walk goes on into the next member once its two magic bytes are there)
        assert (members, used) == (1, first + (into if into >= 2 else 0)) and rc == (0 if into < 2 else sr.Z_BUF_ERROR), (it.name, rc)
    assert {len(it.data) % 4 for it in items if it.name.startswith("cut-")} == {0, 1, 2, 3}
    for name, members in (("cut-in-member-2-header", 2), ("cut-in-member-2-body", 2), ("cut-last-trailer-1-short", 3),
                          ("cut-last-trailer-5-short", 3)):
        rc, _, _, m = walk(oracle, by[name].data, by[name].cap)
        assert rc != 0 and m == members, name
    assert walk(oracle, by["cap-half"].data, by["cap-half"].cap)[0] == sr.Z_BUF_ERROR


def out_of(oracle, gz_file):
    import gzip
    return gzip.decompress(gz_file)


def test_deflate_pieces_and_exact_caps(oracle):
    buf = sr.long_buffer()
    for lengths in (sr.PIECES_16, sr.PIECES_ODD):
        items = sr.pieces(lengths)
        assert b"".join(it.data for it in items) == buf[:sr.LONG]
        at = 0
        for it in items:
            assert it.behind == buf[at + len(it.data):at + len(it.data) + 64] and len(it.behind) == 64
            assert it.before == buf[max(0, at - 64):at]
            at += len(it.data)
    even = sr.pieces(sr.PIECES_16)
    assert all(len(it.data) % 16 == 0 for it in even) and {3072, 3088, 32784, 40000} <= {len(it.data) for it in even}
    assert all(len(it.data) % 16 for it in sr.pieces(sr.PIECES_ODD)[:-1])
    # laid out one behind the other at multiples of 16, the first cut's image is the long buffer itself
    offs, at = [], 0
    for it in even:
        offs.append(at)
        at += sr.round16(len(it.data))
    img = sr.place(even, offs, sr.LONG + 64, "continuation")
    assert img.tobytes() == buf
    # the exact-capacity runs meet every residue of the stream length mod 4, under every plan
    for level, wbits, strategy in sr.DEFLATE_PLANS:
        lens = [len(s) for lengths in (sr.PIECES_16, sr.PIECES_ODD)
                for s in sr.want_deflate(oracle, sr.pieces(lengths), level, wbits, strategy)]
        assert {n % 4 for n in lens} == {0, 1, 2, 3}, (level, wbits, strategy, lens)
        # one byte less is Z_BUF_ERROR, as the oracle reports it
        it = even[3]
        s = sr.want_deflate(oracle, even, level, wbits, strategy)[3]
        assert oracle.compress(it.data, level, window_bits=wbits, strategy=strategy, dest_cap=len(s) - 1)[0] == sr.Z_BUF_ERROR


def test_place_and_the_canary_check():
    items = [sr.Item("a", b"AAAA", 4, b"behind-a" * 20, b"before-a"), sr.Item("b", b"BBBBB", 5, b"behind-b", b"before-b" * 20)]
    offs, n = sr.spread_offsets(items)
    assert all(o % 16 == 0 for o in offs)
    for filler, fill in (("zeros", 0), ("ones", 0xFF)):
        img = sr.place(items, offs, n, filler)
        mask = np.ones(n, dtype=bool)
        for it, o in zip(items, offs):
            assert img[o:o + len(it.data)].tobytes() == it.data
            mask[o:o + len(it.data)] = False
        assert (img[mask] == fill).all()
    noise, cont = sr.place(items, offs, n, "noise"), sr.place(items, offs, n, "continuation")
    assert len(set(noise.tobytes())) > 100 and (sr.place(items, offs, n, "noise") == noise).all()
    for it, o in zip(items, offs):
        end = o + len(it.data)
        assert cont[o:end].tobytes() == it.data and noise[o:end].tobytes() == it.data
    assert cont[offs[0] + 4:offs[0] + 4 + 160].tobytes() == items[0].behind
    assert cont[offs[0] - 8:offs[0]].tobytes() == b"before-a" and cont[offs[1] - 8:offs[1]].tobytes() == b"before-b"
    assert cont[offs[1] + 5:offs[1] + 13].tobytes() == b"behind-b"
    # the canary check: silent about the inside of a slot, loud about a gap and about the bytes behind the last slot
    image = np.full(400, sr.CANARY, dtype=np.uint8)
    slots, caps = [16, 128], [10, 200]
    image[16:26] = 1
    image[128:328] = 2
    sr.assert_outside_untouched(image, slots, caps)
    for at in (0, 15, 26, 127, 328, 391):
        bad = image.copy()
        bad[at] = 0
        with pytest.raises(AssertionError):
            sr.assert_outside_untouched(bad, slots, caps)
        sr.assert_outside_untouched(bad, slots, caps, canary=bad.copy())  # (an earlier run's output as the canary)
    # under_fillers tells a wrong case from a leak
    with pytest.raises(AssertionError, match="wrong with zeros around it as well"):
        sr.under_fillers(["x"], [1], lambda filler: [2])
    with pytest.raises(AssertionError, match="the surroundings leaked in"):
        sr.under_fillers(["x"], [1], lambda filler: [1 if filler == "zeros" else 2])
    with pytest.raises(AssertionError, match="outside the slots"):
        sr.under_fillers(["x"], [1], lambda filler: [1, "3 bytes outside the slots were written"])
    sr.under_fillers(["x"], [1], lambda filler: [1, None])
