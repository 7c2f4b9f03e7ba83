/*
 * deflate_plan_layout.h -- the host side of a deflate plan: which parameters are offloaded and how they fold,
 * the level table, and how a batch is cut into sub-batches and numbered (tiles, block slots, symbol slots, the
 * length-sorted order and its ring classes).  Host only: no device code, no HIP call and no getenv, so the
 * runtime (zsc_hip_runtime.hip) and the lane-emulation harnesses (tests/emu*) run the same code -- the runtime
 * over a whole batch, a harness with count == 1.  What the runtime reads from the environment comes in as
 * DplKnobs.
 */
#ifndef ZSC_DEFLATE_PLAN_LAYOUT_H
#define ZSC_DEFLATE_PLAN_LAYOUT_H

#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "zsc_dev.h"

/* ZlibReturn values of dpl_layout and the last strategy (Z_FIXED), by number: the harnesses know no zsc header */
enum { DPL_OK = 0, DPL_STREAM_ERROR = -2, DPL_MEM_ERROR = -4, DPL_FIXED = 4 };

/* the longest buffer one plan entry may be: deflateBound of it stays below 2^29 bytes = 2^32 bits */
#define ZSC_HIP_MAX_BUFFER 0x1ff00000u

/* The LDS geometry the pipeline runs in when nothing is said (ZSC_HIP_SEG_RING).  The narrow ring pays through
 * the fourth workgroup on a CU and costs through the shorter pipeline (+4.2 % on the
 * headline; 2 to 21 % slower, by class, where a CU is offered three workgroups or fewer), so a sub-batch takes it
 * when it has more long buffers than three per CU, each sub-batch for itself. */
#define ZSC_SEG_WIDE_WG_PER_CU 3u

/* Is the combination offloaded?  window_bits as zsc_compress2 takes it: the wrapper (0 raw, 1 zlib, 2 gzip) and
 * the window size come out of it, Z_DEFAULT_COMPRESSION becomes level 6. */
inline bool dpl_fold_params(int *level, int window_bits, int mem_level, int strategy, int *wrap, int *wbits)
{
    int wb = window_bits;
    *wrap = 1;
    if (wb < 0) {
        *wrap = 0;
        wb = -wb;
    } else if (wb > 15) {
        *wrap = 2;
        wb -= 16;
    }
    if (wb == 8 && *wrap == 1)
        wb = 9; /* reference src/deflate.c:329-331 */
    *wbits = wb;
    if (*level == -1)
        *level = 6;
    return wb >= 9 && wb <= 15 && mem_level >= 1 && mem_level <= 9 && *level >= 1 && *level <= 9 && strategy >= 0 &&
           strategy <= DPL_FIXED;
}

/* lit_bufsize - 1 symbols per block, reference src/deflate.c:362 + include/zsc/deflate.h:338-354 */
inline uint32_t dpl_sym_cap(int mem_level) { return (1u << (mem_level + 6)) - 1u; }

/* level 1..9, wbits 9..15 */
inline ZdLevel dpl_level(int level, int wbits, int mem_level)
{
    static const ZdLevel kLevels[10] = {
        {0, 0, 0, 0, 0},         {4, 4, 8, 4, 0},       {4, 5, 16, 8, 0},     {4, 6, 32, 32, 0},
        {4, 4, 16, 16, 1},       {8, 16, 32, 32, 1},    {8, 16, 128, 128, 1}, {8, 32, 128, 256, 1},
        {32, 128, 258, 1024, 1}, {32, 258, 258, 4096, 1}};
    ZdLevel cfg = kLevels[level];
    cfg.wsize = 1u << wbits;                     /* reference src/deflate.c:343-346 */
    cfg.max_dist = cfg.wsize - ZD_MIN_LOOKAHEAD; /* MAX_DIST, include/zsc/deflate.h:304 */
    cfg.sym_cap = dpl_sym_cap(mem_level);
    cfg.hbits = (uint32_t)mem_level + 7u;
    return cfg;
}

/* block slots of a buffer of n bytes: every block but the last is full; a joint can cut a block */
inline uint32_t dpl_max_blocks(uint32_t n, int mem_level, uint32_t joints)
{
    return n / dpl_sym_cap(mem_level) + 2 + joints;
}

/* the ring class of the wave-per-buffer lazy parser (lz_parse.h) for a buffer of n bytes:
 * 0 the full ring, 1 LzLds16k, 2 LzLds8k, 3 LzLds4k */
inline int dpl_ring_class(uint32_t n)
{
    return n > ZD_RING_16K ? 0 : n > ZD_RING_8K ? 1 : n > ZD_RING_4K ? 2 : 3;
}

/* what a plan of runs of sections (sections.h) knows beyond the lengths */
struct PlanRuns {
    const uint32_t *more;      /* per buffer: ZdBuf.more */
    const uint32_t *n0;        /* per buffer: length of the first section */
    const uint32_t *sched_off; /* per buffer: first joint in sched[] */
    const uint32_t *sched_n;
    const uint32_t *seg_ok;    /* per buffer: sections.h sec_seg_ok */
    const ZdSched *sched;
    uint32_t nsched;
};

/* what the runtime reads from the environment */
struct DplKnobs {
    uint64_t sub_limit = ~0ull;  /* input bytes per sub-batch (a sub-batch always takes one buffer) */
    bool use_seg = true;         /* the segmented parser may take buffers (levels 4-9 only, whatever this says) */
    uint32_t seg_min = 3072u;    /* ... those longer than this */
    bool full_ring_only = false; /* no ring classes: every other buffer in the full ring */
    int ring_said = 0;           /* the segmented parser's geometry: 1 wide, 2 narrow, 0 by the count of long buffers */
    uint32_t cus = 256;          /* compute units of the device */
};

/* a group of buffers that shares one set of scratch arrays: its size and the cuts of its order */
struct DplSubShape {
    uint32_t first = 0, count = 0; /* buffers [first, first+count) of the plan */
    uint32_t ntiles = 0, nslots = 0;
    uint64_t nsym_slots = 0;
    /* the length-sorted order (longest first) splits into ring-size classes:
     * [0,c36) full ring, [c36,c16) <= 18 432 B, [c16,c8) <= 10 240 B, [c8,count) <= 6 144 B */
    uint32_t c36 = 0, c16 = 0, c8 = 0;
    uint32_t cseg = 0;       /* [0,cseg) of the length-sorted order go to the segmented parser */
    bool seg_narrow = false; /* ... in the pipeline's own LDS geometry (k_parse_seg_narrow); fixed when the plan is made */
};
struct DplSub : DplSubShape {
    std::vector<uint32_t> tile_owner, blk_owner, order; /* numbered inside the sub-batch */
};

struct DplLayout {
    std::vector<ZdBuf> bufs; /* tile0 / blk0 / sym_off / rank_off count from the start of the buffer's sub-batch */
    std::vector<DplSub> subs;
    bool use_seg = false; /* DplKnobs.use_seg at a level with a lazy parse */
    /* the largest of any sub-batch: what the shared scratch is sized for */
    uint64_t max_tiles = 0, max_slots = 0, max_syms = 0, max_rank_span = 0, max_count = 0, max_seg = 0;
};

/* level / wrap / wbits as dpl_fold_params left them.  Returns DPL_OK; DPL_MEM_ERROR for a buffer of
 * ZSC_HIP_MAX_BUFFER bytes or more, DPL_STREAM_ERROR for one that is not 16-byte aligned in the batch, with
 * *bad the buffer. */
inline int dpl_layout(uint32_t count, const uint32_t *source_lens, const uint64_t *in_offsets,
                      const uint64_t *out_offsets, const uint32_t *out_caps, int level, int wrap, int wbits,
                      int mem_level, int strategy, const PlanRuns *runs, const DplKnobs &K, DplLayout &L,
                      uint32_t *bad)
{
    L.bufs.resize(count);
    L.use_seg = K.use_seg && dpl_level(level, wbits, mem_level).slow;
    /* cut into sub-batches and number tiles / block slots / symbol slots inside each */
    uint32_t i = 0;
    while (i < count) {
        DplSub sb;
        sb.first = i;
        uint64_t bytes = 0;
        while (i < count && (sb.count == 0 || bytes + source_lens[i] <= K.sub_limit)) {
            const uint32_t n = source_lens[i];
            /* bit positions inside one stream are 32-bit (ZdBlockPlan.bit_off, the layout and emit kernels): a
             * stream must stay below 2^32 bits */
            const bool aligned = !(in_offsets[i] & 15u || out_offsets[i] & 15u);
            if (n >= ZSC_HIP_MAX_BUFFER || !aligned) {
                *bad = i;
                return n >= ZSC_HIP_MAX_BUFFER ? DPL_MEM_ERROR : DPL_STREAM_ERROR;
            }
            ZdBuf &b = L.bufs[i];
            memset(&b, 0, sizeof b);
            b.in_off = in_offsets[i];
            b.out_off = out_offsets[i];
            b.in_len = n;
            b.out_cap = out_caps[i];
            b.ntiles = n == 0 ? 1u : (uint32_t)(((uint64_t)n + ZD_TILE - 1) / ZD_TILE);
            b.tile0 = sb.ntiles;
            b.n0 = n;
            if (runs) {
                b.more = runs->more[i];
                b.n0 = runs->n0[i];
                b.sched_off = runs->sched_off[i];
                b.sched_n = runs->sched_n[i];
                b.seg_ok = runs->seg_ok[i];
            }
            b.max_blocks = dpl_max_blocks(n, mem_level, b.sched_n);
            b.blk0 = sb.nslots;
            b.sym_off = sb.nsym_slots;
            b.rank_off = sb.nsym_slots; /* one u16 per (padded) input position */
            b.level = (uint32_t)level;
            b.wrap = (uint32_t)wrap;
            b.strategy = (uint32_t)strategy;
            b.wbits = (uint32_t)wbits;
            sb.ntiles += b.ntiles;
            sb.nslots += b.max_blocks;
            sb.nsym_slots += ((uint64_t)n + 64u) & ~63ull;
            bytes += n;
            sb.count++;
            i++;
        }
        L.subs.push_back(std::move(sb));
    }

    for (DplSub &sb : L.subs) {
        const ZdBuf *bufs = &L.bufs[sb.first];
        sb.tile_owner.resize(sb.ntiles);
        sb.blk_owner.resize(sb.nslots);
        sb.order.resize(sb.count);
        for (uint32_t k = 0; k < sb.count; k++) {
            const ZdBuf &b = bufs[k];
            for (uint32_t t = 0; t < b.ntiles; t++)
                sb.tile_owner[b.tile0 + t] = k;
            for (uint32_t s = 0; s < b.max_blocks; s++)
                sb.blk_owner[b.blk0 + s] = k;
            sb.order[k] = k;
        }
        /* longest first; those the segmented parser may take come first */
        auto seg_able = [&](uint32_t k) {
            return L.use_seg && bufs[k].in_len > K.seg_min && (bufs[k].sched_n == 0 || bufs[k].seg_ok);
        };
        std::stable_sort(sb.order.begin(), sb.order.end(), [&](uint32_t a, uint32_t c) {
            const bool sa = seg_able(a), sc = seg_able(c);
            if (sa != sc)
                return sa;
            return bufs[a].in_len > bufs[c].in_len;
        });
        auto len_at = [&](uint32_t idx) { return bufs[sb.order[idx]].in_len; };
        uint32_t k = 0;
        while (k < sb.count && seg_able(sb.order[k]))
            k++;
        sb.cseg = k;
        sb.seg_narrow = K.ring_said == 2 || (K.ring_said == 0 && sb.cseg > ZSC_SEG_WIDE_WG_PER_CU * K.cus);
        while (k < sb.count && (K.full_ring_only || dpl_ring_class(len_at(k)) == 0))
            k++;
        sb.c36 = k;
        while (k < sb.count && dpl_ring_class(len_at(k)) == 1)
            k++;
        sb.c16 = k;
        while (k < sb.count && dpl_ring_class(len_at(k)) == 2)
            k++;
        sb.c8 = k;
        L.max_tiles = std::max<uint64_t>(L.max_tiles, sb.ntiles);
        L.max_slots = std::max<uint64_t>(L.max_slots, sb.nslots);
        L.max_syms = std::max<uint64_t>(L.max_syms, sb.nsym_slots);
        L.max_rank_span = std::max<uint64_t>(L.max_rank_span, sb.nsym_slots + 64);
        L.max_count = std::max<uint64_t>(L.max_count, sb.count);
        L.max_seg = std::max<uint64_t>(L.max_seg, sb.cseg);
    }
    return DPL_OK;
}

#endif
