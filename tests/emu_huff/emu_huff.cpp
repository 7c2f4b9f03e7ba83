/*
 * emu_huff.cpp -- TEST INFRASTRUCTURE ONLY.
 *
 * The block planner (zsc_amd/csrc/huff_plan.h) alone in the lane emulation: the symbols and block cuts of a
 * parse go in, the plans (block type, sizes, code tables, header bits) come out.  Built at 64, 16 and 8 lanes
 * per wave, so that every lane-parallel part of the planner runs with more than one step per tree.  The
 * planner's path hooks (HP_PATH) are counted here.
 */
#define ZSC_WAVE_EMU 1
#include <stdint.h>
static unsigned long long g_hp_path[16];
#define HP_PATH(id) (g_hp_path[(id)]++)
#include "../../zsc_amd/csrc/huff_plan.h"
#include <string.h>

extern "C" int emu_huff_lanes(void)
{
    return WAVE;
}

extern "C" void emu_huff_paths(unsigned long long *out, int clear)
{
    memcpy(out, g_hp_path, sizeof g_hp_path);
    if (clear)
        memset(g_hp_path, 0, sizeof g_hp_path);
}

/* recs: nblocks x 9 words (ZdBlockRec); plans: nblocks x sizeof(ZdBlockPlan) bytes, of which the bytes of hdr[]
 * behind the header's last bit are cleared so that two builds' plans compare as bytes.  Returns sizeof(ZdBlockPlan).
 * The planner's LDS image is filled with `fill` once and then reused from block to block, as one wave's is. */
extern "C" uint32_t emu_huff_plan(const uint32_t *syms, const uint32_t *recs, uint32_t nblocks, uint32_t strategy,
                                  uint8_t *plans, uint32_t fill)
{
    static_assert(sizeof(ZdBlockRec) == 9 * sizeof(uint32_t), "ZdBlockRec is nine words");
    HpLds hl;
    memset(&hl, (int)fill, sizeof hl);
    for (uint32_t b = 0; b < nblocks && plans; b++) {
        ZdBlockRec rec;
        memcpy(&rec, recs + 9 * b, sizeof rec);
        ZdBlockPlan plan;
        memset(&plan, 0, sizeof plan);
        huff_plan_block(syms + rec.sym_begin, &rec, strategy, &plan, &hl);
        const uint32_t used = (plan.hdr_bits + 7) / 8;
        if (plan.hdr_bits & 7)
            plan.hdr[used - 1] &= (uint8_t)((1u << (plan.hdr_bits & 7)) - 1u);
        memset(plan.hdr + used, 0, ZD_HDR_BYTES - used);
        memcpy(plans + (size_t)b * sizeof plan, &plan, sizeof plan);
    }
    return (uint32_t)sizeof(ZdBlockPlan);
}

extern "C" uint32_t emu_huff_lds_bytes(void)
{
    return (uint32_t)sizeof(HpLds);
}
