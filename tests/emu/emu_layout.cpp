/*
 * emu_layout.cpp -- TEST INFRASTRUCTURE ONLY.
 *
 * The layout of a deflate plan (zsc_amd/csrc/deflate_plan_layout.h) as zsc_hip_deflate_plan_create makes it, handed
 * out as plain arrays so that tests/test_deflate_layout_emu.py can hold it against the rules.  Only lengths and
 * offsets come in: nothing of a buffer's size is allocated.
 */
#include "../../zsc_amd/csrc/deflate_plan_layout.h"

/* knobs: sub_limit, use_seg, seg_min, full_ring_only, ring_said, cus.  folded: ok, level, wrap, wbits as
 * dpl_fold_params leaves them.  Returns dpl_layout's code with *bad the buffer it refuses (-2 too where the
 * parameters do not fold), -100 where a cap is short.  subs: per sub-batch first, count, ntiles, nslots, cseg, c36,
 * c16, c8, seg_narrow; per_buf: tile0, ntiles, blk0, max_blocks, sym_off; order / tile_owner / blk_owner: the
 * sub-batches' arrays one after the other */
extern "C" int emu_plan_layout(uint32_t count, const uint32_t *lens, const uint64_t *in_offsets,
                               const uint64_t *out_offsets, int level, int window_bits, int mem_level, int strategy,
                               const uint64_t *knobs, int *folded, uint32_t *bad, uint32_t *nsubs, uint32_t *subs,
                               uint32_t subs_cap, uint64_t *per_buf, uint32_t *order, uint32_t *tile_owner,
                               uint32_t *blk_owner, uint64_t owners_cap)
{
    int wrap, wbits;
    folded[0] = dpl_fold_params(&level, window_bits, mem_level, strategy, &wrap, &wbits);
    folded[1] = level;
    folded[2] = wrap;
    folded[3] = wbits;
    *bad = *nsubs = 0;
    if (!folded[0])
        return DPL_STREAM_ERROR;
    const DplKnobs K = {knobs[0], knobs[1] != 0, (uint32_t)knobs[2], knobs[3] != 0, (int)knobs[4], (uint32_t)knobs[5]};
    const std::vector<uint32_t> caps(count, 0u);
    DplLayout L;
    const int rc = dpl_layout(count, lens, in_offsets, out_offsets, caps.data(), level, wrap, wbits, mem_level,
                              strategy, nullptr, K, L, bad);
    if (rc != DPL_OK)
        return rc;
    uint64_t nt = 0, ns = 0;
    for (const DplSub &sb : L.subs)
        nt += sb.ntiles, ns += sb.nslots;
    if (L.subs.size() > subs_cap || nt > owners_cap || ns > owners_cap)
        return -100;
    *nsubs = (uint32_t)L.subs.size();
    for (const DplSub &sb : L.subs) {
        const uint32_t v[9] = {sb.first, sb.count, sb.ntiles, sb.nslots, sb.cseg, sb.c36, sb.c16, sb.c8, sb.seg_narrow};
        memcpy(subs, v, sizeof v);
        subs += 9;
        order = std::copy(sb.order.begin(), sb.order.end(), order);
        tile_owner = std::copy(sb.tile_owner.begin(), sb.tile_owner.end(), tile_owner);
        blk_owner = std::copy(sb.blk_owner.begin(), sb.blk_owner.end(), blk_owner);
    }
    for (uint32_t i = 0; i < count; i++) {
        const ZdBuf &b = L.bufs[i];
        const uint64_t v[5] = {b.tile0, b.ntiles, b.blk0, b.max_blocks, b.sym_off};
        memcpy(per_buf + 5 * i, v, sizeof v);
    }
    return DPL_OK;
}
