/*
 * inflate_plan_layout.h -- the host side of the inflate plans that cut streams: how a batch is cut into
 * tiles (sections, resync, members) or chunks (chunks, size, check), and the device views (IsecPlan, IchkPlan, MemPlan) over
 * a set of buffers.  Host only: no device code and no HIP call, so the runtime (zsc_hip_runtime.hip) and
 * the lane-emulation harnesses (tests/emu_*) run the same code -- the runtime over its device buffers, a
 * harness with count == 1 over vectors of the exact sizes.
 */
#ifndef ZSC_INFLATE_PLAN_LAYOUT_H
#define ZSC_INFLATE_PLAN_LAYOUT_H

#include <stdint.h>
#include <algorithm>
#include <vector>

#include "inflate_chunks.h"
#include "inflate_members.h"

/* what the host builds before anything is allocated */
struct InfLayout {
    std::vector<IsecItem> items;  /* one per stream */
    std::vector<IsecTile> tiles;  /* sections: every tile of SEC_TILE input bytes; chunks: every chunk but a
                                   * stream's first (the scan visits these) */
    std::vector<uint32_t> active; /* chunks: the streams that are cut */
    uint64_t pool = 0;            /* sections: candidate records; chunks: chunks of all active streams */
};

/* per stream: its tiles of SEC_TILE input bytes; candidate records from one pool */
inline void sec_layout(uint32_t count, const uint32_t *source_lens, const uint64_t *src_offsets,
                       const uint64_t *dst_offsets, const uint32_t *dest_caps, InfLayout &L)
{
    L.items.resize(count);
    uint64_t total_in = 0;
    for (uint32_t i = 0; i < count; i++) {
        IsecItem &it = L.items[i];
        it.src_off = src_offsets[i];
        it.dst_off = dst_offsets[i];
        it.src_len = source_lens[i];
        it.dst_cap = dest_caps[i];
        it.cap = source_lens[i] / SEC_CAND_DIV + SEC_CAND_MIN;
        it.tile0 = (uint32_t)L.tiles.size();
        it.ntiles = (source_lens[i] + SEC_TILE - 1u) / SEC_TILE;
        it.pad = 0;
        for (uint32_t t = 0; t < it.ntiles; t++)
            L.tiles.push_back(IsecTile{i, t * SEC_TILE});
        total_in += source_lens[i];
    }
    L.pool = std::min<uint64_t>(SEC_POOL_SLOTS(total_in), 0x0ffffff0u);
}

/* a members plan: the sections layout over files, with a candidate cap no file of real members reaches (a
 * member has 20 bytes or more).  dst_offsets and dest_caps may be null (size-only: nothing written, no limit). */
inline void mem_layout(uint32_t count, const uint32_t *source_lens, const uint64_t *src_offsets,
                       const uint64_t *dst_offsets, const uint32_t *dest_caps, InfLayout &L)
{
    std::vector<uint64_t> zero;
    std::vector<uint32_t> unlimited;
    if (!dst_offsets) {
        zero.assign(count, 0);
        dst_offsets = zero.data();
    }
    if (!dest_caps) {
        unlimited.assign(count, 0xffffffffu);
        dest_caps = unlimited.data();
    }
    sec_layout(count, source_lens, src_offsets, dst_offsets, dest_caps, L);
    for (IsecItem &it : L.items)
        it.cap = it.src_len / MEM_CAND_DIV + SEC_CAND_MIN;
}

/* per stream longer than a chunk of cb bytes that may_cut(i) allows: its chunks; the scan visits every chunk
 * but the first.  dst_offsets may be null (a plan that writes nothing: every offset 0).  cb is the resolved
 * chunk size: the caller applies the default and the minimum (the harnesses go below it on purpose). */
template <class MayCut>
inline void chk_layout(uint32_t count, const uint32_t *source_lens, const uint64_t *src_offsets,
                       const uint64_t *dst_offsets, const uint32_t *dest_caps, uint32_t cb, MayCut may_cut,
                       InfLayout &L)
{
    L.items.resize(count);
    for (uint32_t i = 0; i < count; i++) {
        IsecItem &it = L.items[i];
        it.src_off = src_offsets[i];
        it.dst_off = dst_offsets ? dst_offsets[i] : 0;
        it.src_len = source_lens[i];
        it.dst_cap = dest_caps[i];
        it.cap = 0;
        it.tile0 = (uint32_t)L.pool;
        it.ntiles = 0;
        it.pad = 0;
        if (source_lens[i] > cb && may_cut(i)) {
            it.ntiles = (uint32_t)(((uint64_t)source_lens[i] + cb - 1u) / cb);
            for (uint32_t k = 1; k < it.ntiles; k++)
                L.tiles.push_back(IsecTile{i, k});
            L.active.push_back(i);
            L.pool += it.ntiles;
        }
    }
}

/* the buffers the views point into, by the names of the views' members; null: the plan has none */
struct InfPlanMem {
    void *items, *tiles, *tile_cnt, *tile_off, *scount, *nsec, *st, *active, *q;
    void *cstart, *cstop, *clink, *clen, *chain_k, *chain_off, *chain_ck;
    void *cand, *cused, *creach, *want, *ring, *win; /* chunk records */
};

inline void sec_plan_view(IsecPlan &P, const InfPlanMem &m, const InfLayout &L, int32_t window_bits,
                          uint32_t work_mul = SEC_WORK_MUL, uint32_t work_add = SEC_WORK_ADD)
{
    P.items = (const IsecItem *)m.items;
    P.tiles = (const IsecTile *)m.tiles;
    P.tile_cnt = (uint32_t *)m.tile_cnt;
    P.tile_off = (uint32_t *)m.tile_off;
    P.scount = (uint32_t *)m.scount;
    P.nsec = (uint32_t *)m.nsec;
    P.st = (IsecStream *)m.st;
    P.active = (uint32_t *)m.active;
    P.q = (uint32_t *)m.q;
    P.cstart = (uint32_t *)m.cstart;
    P.cstop = (uint32_t *)m.cstop;
    P.clink = (uint32_t *)m.clink;
    P.clen = (uint32_t *)m.clen;
    P.chain_k = (uint32_t *)m.chain_k;
    P.chain_off = (uint32_t *)m.chain_off;
    P.chain_ck = (uint32_t *)m.chain_ck;
    P.count = (uint32_t)L.items.size();
    P.ntiles = (uint32_t)L.tiles.size();
    P.pool = (uint32_t)L.pool;
    P.window_bits = window_bits;
    P.work_mul = work_mul;
    P.work_add = work_add;
}

inline void mem_plan_view(MemPlan &M, const InfPlanMem &m, const InfLayout &L, int32_t window_bits, void *mf,
                          bool size_only, bool claims, uint32_t work_mul = SEC_WORK_MUL,
                          uint32_t work_add = SEC_WORK_ADD)
{
    sec_plan_view(M.sp, m, L, window_bits, work_mul, work_add);
    M.mf = (MemFile *)mf;
    M.size_only = size_only;
    M.claims = claims;
}

/* (keep_index stays as it is: a run state of chunks plans) */
inline void chk_plan_view(IchkPlan &P, const InfPlanMem &m, const InfLayout &L, int32_t window_bits, uint32_t cb,
                          uint32_t work_mul = SEC_WORK_MUL, uint32_t work_add = SEC_WORK_ADD)
{
    sec_plan_view(P.sp, m, L, window_bits, work_mul, work_add);
    P.cand = (uint64_t *)m.cand;
    P.cused = (uint32_t *)m.cused;
    P.creach = (uint32_t *)m.creach;
    P.want = (uint32_t *)m.want;
    P.ring = (uint16_t *)m.ring;
    P.win = (uint8_t *)m.win;
    P.nactive = (uint32_t)L.active.size();
    P.chunk_bytes = cb;
}

#endif
