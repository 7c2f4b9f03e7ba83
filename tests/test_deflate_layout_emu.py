"""The layout of a deflate plan, on the CPU.

zsc_amd/csrc/deflate_plan_layout.h decides how zsc_hip_deflate_plan_create folds its parameters, cuts a batch into
sub-batches, numbers tiles / block slots / symbol slots inside each, orders the buffers and cuts the order into
ring classes.  tests/emu/libzsc_emu.so exports that very code as emu_plan_layout; the rules are restated here and
held against it.  Only lengths and offsets go in, so nothing of a buffer's size is allocated.

One rule is stated as the code has it and not as one might expect it: whether a buffer is "segment-able" depends on
the plan's use_seg (the segmented parser is allowed and the level has a lazy parse) and on the length alone, not on
the strategy.  A Z_RLE plan at level 6 therefore still counts its long buffers into cseg (the run ignores the cut:
Z_RLE and Z_HUFFMAN_ONLY take one parse kernel for every buffer), while a plan at levels 1-3 has cseg == 0.
"""
import ctypes as C
import os
import random

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
Z_OK, Z_STREAM_ERROR, Z_MEM_ERROR = 0, -2, -4
Z_FILTERED, Z_HUFFMAN_ONLY, Z_RLE, Z_FIXED = 1, 2, 3, 4
RINGS = (18432, 10240, 6144)  # a buffer no longer than one of these takes that ring
MAX_BUFFER = 0x1FF00000
KNOBS = dict(sub_limit=(1 << 64) - 1, use_seg=1, seg_min=3072, full_ring_only=0, ring_said=0, cus=256)
LENGTHS = [0, 1, 3072, 3073, 6144, 6145, 10240, 10241, 18432, 18433, 40000, 70000]
random.Random(7).shuffle(LENGTHS)


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(os.path.join(HERE, "emu", "libzsc_emu.so"))
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    L.emu_plan_layout.restype = C.c_int
    L.emu_plan_layout.argtypes = [C.c_uint32, u32p, u64p, u64p, C.c_int, C.c_int, C.c_int, C.c_int, u64p,
                                  C.POINTER(C.c_int), u32p, u32p, u32p, C.c_uint32, u64p, u32p, u32p, u32p, C.c_uint64]
    return L


def ntiles(n):
    return 1 if n == 0 else (n + 32768 - 1) // 32768


def max_blocks(n, mem_level):
    return n // ((1 << (mem_level + 6)) - 1) + 2


def layout(lib, lens, level=6, window_bits=15, mem_level=8, strategy=0, in_off=None, out_off=None, **knobs):
    """(rc, bad, folded, subs, per_buf): subs a list of dicts with their order and owner arrays, per_buf rows of
    (tile0, ntiles, blk0, max_blocks, sym_off)"""
    k = dict(KNOBS, **knobs)
    count = len(lens)
    a_lens = np.asarray(lens, dtype=np.uint32)
    a_in, a_out = (np.asarray(o if o is not None else [0] * count, dtype=np.uint64) for o in (in_off, out_off))
    a_knobs = np.asarray([k[x] for x in KNOBS], dtype=np.uint64)  # (in the order of the export's knobs)
    owners_cap = sum(max(ntiles(n), max_blocks(n, max(mem_level, 1))) for n in lens if n < MAX_BUFFER) + 1
    folded = np.zeros(4, dtype=np.int32)
    bad, nsubs = C.c_uint32(0), C.c_uint32(0)
    subs = np.zeros((count + 1, 9), dtype=np.uint32)
    per_buf = np.zeros((count + 1, 5), dtype=np.uint64)
    order = np.zeros(count + 1, dtype=np.uint32)
    tile_owner, blk_owner = (np.full(owners_cap, 0xEEEEEEEE, dtype=np.uint32) for _ in range(2))
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    rc = lib.emu_plan_layout(count, a_lens.ctypes.data_as(u32p), a_in.ctypes.data_as(u64p), a_out.ctypes.data_as(u64p),
                             level, window_bits, mem_level, strategy, a_knobs.ctypes.data_as(u64p),
                             folded.ctypes.data_as(C.POINTER(C.c_int)), C.byref(bad), C.byref(nsubs),
                             subs.ctypes.data_as(u32p), count + 1, per_buf.ctypes.data_as(u64p),
                             order.ctypes.data_as(u32p), tile_owner.ctypes.data_as(u32p),
                             blk_owner.ctypes.data_as(u32p), owners_cap)
    out, k0, t0, s0 = [], 0, 0, 0
    for row in subs[:nsubs.value].tolist():
        sb = dict(zip(("first", "count", "ntiles", "nslots", "cseg", "c36", "c16", "c8", "seg_narrow"), row))
        sb["order"] = order[k0:k0 + sb["count"]].tolist()
        sb["tile_owner"] = tile_owner[t0:t0 + sb["ntiles"]].tolist()
        sb["blk_owner"] = blk_owner[s0:s0 + sb["nslots"]].tolist()
        k0, t0, s0 = k0 + sb["count"], t0 + sb["ntiles"], s0 + sb["nslots"]
        out.append(sb)
    return rc, bad.value, folded.tolist(), out, per_buf[:count].tolist()


def check_rules(lens, subs, per_buf, level=6, mem_level=8, **knobs):
    """every rule of the layout, restated"""
    k = dict(KNOBS, **knobs)
    use_seg = bool(k["use_seg"]) and level >= 4
    # the cut into sub-batches: a sub-batch takes buffers while they fit, and always one
    cuts, i = [], 0
    while i < len(lens):
        first, total = i, 0
        while i < len(lens) and (i == first or total + lens[i] <= k["sub_limit"]):
            total += lens[i]
            i += 1
        cuts.append((first, i - first))
    assert [(sb["first"], sb["count"]) for sb in subs] == cuts
    for sb in subs:
        mine = lens[sb["first"]:sb["first"] + sb["count"]]
        tile0 = blk0 = sym_off = 0  # the numbering restarts in every sub-batch
        tile_owner, blk_owner = [], []
        for j, n in enumerate(mine):
            assert per_buf[sb["first"] + j] == [tile0, ntiles(n), blk0, max_blocks(n, mem_level), sym_off]
            tile_owner += [j] * ntiles(n)
            blk_owner += [j] * max_blocks(n, mem_level)
            tile0, blk0, sym_off = tile0 + ntiles(n), blk0 + max_blocks(n, mem_level), sym_off + ((n + 64) & ~63)
        assert (sb["ntiles"], sb["nslots"]) == (tile0, blk0)
        assert sb["tile_owner"] == tile_owner and sb["blk_owner"] == blk_owner
        seg_able = [use_seg and n > k["seg_min"] for n in mine]
        # segment-able first, then longest first, stable among equals
        assert sb["order"] == sorted(range(len(mine)), key=lambda j: (not seg_able[j], -mine[j]))
        rest = [mine[j] for j in sb["order"][sum(seg_able):]]
        assert sb["cseg"] == sum(seg_able)
        if k["full_ring_only"]:
            assert sb["c36"] == sb["c16"] == sb["c8"] == sb["count"]
        else:
            assert [sb["c36"], sb["c16"], sb["c8"]] == [sb["cseg"] + sum(n > r for n in rest) for r in RINGS]
        want_narrow = k["ring_said"] == 2 or (k["ring_said"] == 0 and sb["cseg"] > 3 * k["cus"])
        assert sb["seg_narrow"] == int(want_narrow)


def test_lengths_at_the_thresholds_level_6(lib):
    rc, _, folded, subs, per_buf = layout(lib, LENGTHS, level=6)
    assert rc == Z_OK and folded == [1, 6, 1, 15] and len(subs) == 1
    check_rules(LENGTHS, subs, per_buf, level=6)
    sb = subs[0]
    assert [LENGTHS[j] for j in sb["order"]] == sorted(LENGTHS, reverse=True)
    # everything above 3072 goes to the segmented parser, which leaves nothing for the three larger rings
    assert sb["cseg"] == sb["c36"] == sb["c16"] == sb["c8"] == 9
    assert LENGTHS[sb["order"][8]] == 3073 and LENGTHS[sb["order"][9]] == 3072


@pytest.mark.parametrize("how", [dict(level=1), dict(level=3), dict(level=6, use_seg=0)], ids=str)
def test_ring_classes_fall_at_the_thresholds(lib, how):
    rc, _, _, subs, per_buf = layout(lib, LENGTHS, **how)
    assert rc == Z_OK and len(subs) == 1
    check_rules(LENGTHS, subs, per_buf, **how)
    sb = subs[0]
    by_len = [LENGTHS[j] for j in sb["order"]]
    assert by_len == sorted(LENGTHS, reverse=True)
    assert sb["cseg"] == 0
    # > 18 432 | > 10 240 | > 6 144 | the rest: a length equal to a ring still takes that ring
    assert by_len[:sb["c36"]] == [70000, 40000, 18433]
    assert by_len[sb["c36"]:sb["c16"]] == [18432, 10241]
    assert by_len[sb["c16"]:sb["c8"]] == [10240, 6145]
    assert by_len[sb["c8"]:] == [6144, 3073, 3072, 1, 0]


def test_full_ring_only_equal_lengths_and_mem_level(lib):
    rc, _, _, subs, per_buf = layout(lib, LENGTHS, level=6, full_ring_only=1)
    assert rc == Z_OK
    check_rules(LENGTHS, subs, per_buf, level=6, full_ring_only=1)
    assert subs[0]["cseg"] == 9 and subs[0]["c36"] == subs[0]["c16"] == subs[0]["c8"] == len(LENGTHS)
    lens = [5000, 100, 5000, 100, 5000, 3072, 3072]  # equal lengths keep their order
    rc, _, _, subs, per_buf = layout(lib, lens, level=6)
    check_rules(lens, subs, per_buf, level=6)
    assert rc == Z_OK and subs[0]["order"] == [0, 2, 4, 5, 6, 1, 3]
    for mem_level in (1, 9):  # the block slots follow mem_level
        rc, _, _, subs, per_buf = layout(lib, LENGTHS, level=6, mem_level=mem_level)
        assert rc == Z_OK
        check_rules(LENGTHS, subs, per_buf, level=6, mem_level=mem_level)


@pytest.mark.parametrize("strategy", [Z_RLE, Z_HUFFMAN_ONLY, Z_FILTERED, Z_FIXED])
def test_strategy_does_not_enter_the_layout(lib, strategy):
    """as the code stands: the order is by length, and what counts as segment-able depends on use_seg and the length
    only (the module's docstring) -- so also for Z_RLE, whose run ignores cseg"""
    rc, _, _, subs, per_buf = layout(lib, LENGTHS, level=6, strategy=strategy)
    assert rc == Z_OK
    check_rules(LENGTHS, subs, per_buf, level=6)
    assert [LENGTHS[j] for j in subs[0]["order"]] == sorted(LENGTHS, reverse=True)
    assert subs == layout(lib, LENGTHS, level=6)[3]
    rc, _, _, subs, _ = layout(lib, LENGTHS, level=1, strategy=strategy)
    assert rc == Z_OK and subs[0]["cseg"] == 0


KIB, MIB = 1 << 10, 1 << 20


@pytest.mark.parametrize("lens, want", [
    ([600 * KIB] * 3, [(0, 1), (1, 1), (2, 1)]),
    ([400 * KIB] * 3, [(0, 2), (2, 1)]),
    ([1 * KIB, 2 * MIB, 1 * KIB], [(0, 1), (1, 1), (2, 1)]),  # the one that is over the limit stands alone
    ([512 * KIB, 512 * KIB, 1], [(0, 2), (2, 1)]),             # exactly the limit still fits
], ids=["3x600K", "3x400K", "2M-between", "exact"])
def test_sub_batches_of_one_mib(lib, lens, want):
    rc, _, _, subs, per_buf = layout(lib, lens, level=6, sub_limit=MIB)
    assert rc == Z_OK
    assert [(sb["first"], sb["count"]) for sb in subs] == want
    check_rules(lens, subs, per_buf, level=6, sub_limit=MIB)
    for sb in subs:  # the numbering restarts at 0 in each
        assert per_buf[sb["first"]][0] == per_buf[sb["first"]][2] == per_buf[sb["first"]][4] == 0
        assert sorted(sb["order"]) == list(range(sb["count"]))


@pytest.mark.parametrize("nlong, said, narrow", [(4, 0, 1), (3, 0, 0), (4, 1, 0), (3, 2, 1), (0, 2, 1)])
def test_narrow_ring_with_one_cu(lib, nlong, said, narrow):
    lens = [100] + [5000] * nlong + [200]
    rc, _, _, subs, per_buf = layout(lib, lens, level=6, cus=1, ring_said=said)
    assert rc == Z_OK and subs[0]["cseg"] == nlong
    check_rules(lens, subs, per_buf, level=6, cus=1, ring_said=said)
    assert subs[0]["seg_narrow"] == narrow


def test_refusals(lib):
    # (only the length is passed: nothing that large exists)
    rc, bad, _, _, _ = layout(lib, [100, 5, MAX_BUFFER, 7])
    assert (rc, bad) == (Z_MEM_ERROR, 2)
    lens = [100, MAX_BUFFER - 1]
    rc, _, _, subs, per_buf = layout(lib, lens)
    assert rc == Z_OK
    check_rules(lens, subs, per_buf)
    rc, bad, _, _, _ = layout(lib, [100, 100, 100], in_off=[0, 112, 232])
    assert (rc, bad) == (Z_STREAM_ERROR, 2)
    rc, bad, _, _, _ = layout(lib, [100, 100, 100], out_off=[0, 8, 256])
    assert (rc, bad) == (Z_STREAM_ERROR, 1)
    rc, _, _, _, _ = layout(lib, [100, 100, 100], in_off=[0, 112, 224], out_off=[16, 160, 320])
    assert rc == Z_OK


@pytest.mark.parametrize("args, want", [
    # (level, window_bits, mem_level, strategy) -> ok, level, wrap, wbits
    ((6, 15, 8, 0), [1, 6, 1, 15]),
    ((-1, 15, 8, 0), [1, 6, 1, 15]),   # Z_DEFAULT_COMPRESSION
    ((6, -15, 8, 0), [1, 6, 0, 15]),
    ((6, 31, 8, 0), [1, 6, 2, 15]),
    ((6, 8, 8, 0), [1, 6, 1, 9]),      # zlib alone turns a window of 256 into one of 512
    ((6, 24, 8, 0), [0, 6, 2, 8]),
    ((6, -8, 8, 0), [0, 6, 0, 8]),
    ((9, 25, 9, Z_RLE), [1, 9, 2, 9]),
    ((0, 15, 8, 0), [0, 0, 1, 15]),
    ((10, 15, 8, 0), [0, 10, 1, 15]),
    ((6, 15, 10, 0), [0, 6, 1, 15]),
    ((6, 15, 8, 5), [0, 6, 1, 15]),
])
def test_parameter_folding(lib, args, want):
    level, wb, ml, strategy = args
    rc, _, folded, subs, _ = layout(lib, [100], level=level, window_bits=wb, mem_level=ml, strategy=strategy)
    assert folded == want
    assert rc == (Z_OK if want[0] else Z_STREAM_ERROR) and len(subs) == want[0]
