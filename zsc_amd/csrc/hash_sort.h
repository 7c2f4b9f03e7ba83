/*
 * hash_sort.h -- kernel 1: per-tile hash-chain construction by sorting.
 *
 * Replaces the reference's INSERT_STRING / head[] / prev[] machinery
 * (src/deflate.c:174-189, slide_hash :204-231).  For compression levels 4-9
 * every position is inserted into the chain of its 3-byte hash
 * (src/deflate.c:2018,2069-2075), so "the chain of p" is simply: all earlier
 * positions with the same hash, newest first.  Sorting a tile's positions by
 * (hash, position) makes that chain a CONTIGUOUS, descending run that a
 * wavefront can fetch 64 candidates at a time with one coalesced load, instead
 * of chasing prev[] links one dependent load at a time.
 *
 * One workgroup of HS_WAVES wavefronts per tile of 32 768 positions.  Stable
 * LSD radix sort in two passes over the 15-bit hash (8 low bits, 7 high bits):
 *   phase 0  clear counters
 *   phase 1  per-wave-slice histogram of the low digit
 *   phase 2  exclusive scan (digit-major, wave-minor)
 *   phase 3  stable scatter into tmp: rank inside a 64-element step comes from
 *            ballot "multi-split" (one ballot per digit bit), not from atomics
 *   phase 4  per-wave-slice histogram of the high digit over tmp
 *   phase 5  scan
 *   phase 6  stable scatter into sorted[] + rank[]
 *   phase 7  bucket directory dir[h] = first sorted index with hash >= h
 * Counters are tiny (24 KiB of LDS), two tiles are resident per CU.
 *
 * Round 2 also built the sort wholly inside LDS (tile bytes, a 16-bit order array permuted in
 * place through registers, sorted[] / rank[] / dir[] written once and coalesced; commit
 * "hash sort staged wholly in LDS"): 41 ms per 1024 Canterbury-like sets with the ballot
 * multi-split, 49 ms with an LDS match table in its place, against 40 ms for this version --
 * the scattered accesses move from the texture path to LDS bank conflicts and cost the same
 * ~10 CU cycles per position.  Neither HBM (about 3 TB/s read and written) nor instruction issue
 * (about 100 instructions per 64 positions) nor the LDS explains that rate; what the scatter loops
 * did was to keep one step of 64 positions in flight per wave, each step waiting for the scattered
 * stores of the one before it.  A wave now takes HS_SCATTER_BATCH steps through a scatter as one
 * unit (hs_scatter_batch; hs_directory likewise), DESIGN section 5g.
 *
 * Bytes per input byte (TILE positions): read 2 (input, twice) + tmp 4w+4r +
 * sorted 4w(+4r for dir) + rank 2w + dir 2w.
 */
#ifndef ZSC_HASH_SORT_H
#define ZSC_HASH_SORT_H

#include "wave.h"
#include "zsc_dev.h"

#define HS_WAVES 16

typedef struct {
    uint32_t cnt0[256 * HS_WAVES];
    uint32_t cnt1[128 * HS_WAVES];
} HsLds;

typedef struct {
    const uint8_t *in;  /* the tile's buffer */
    uint32_t n;         /* buffer length */
    uint32_t start;     /* absolute position of the tile's first byte */
    uint32_t m;         /* positions of this tile that own a 3-byte string (pos <= n-3) */
    uint32_t *sorted;   /* TILE entries */
    uint32_t *tmp;      /* TILE entries */
    uint16_t *rank;     /* per position of the buffer */
    uint16_t *dir;      /* DIR_STRIDE entries: first sorted index of every bucket */
    const uint16_t *dir_prev; /* directory of the previous tile of the same buffer, or null */
    uint16_t *hib;      /* per position of the buffer: last sorted index of its bucket in the previous tile */
    uint32_t *cnt;      /* per position of the buffer: earlier members of its bucket in its own tile (low
                           half) and members of the bucket in the previous tile (high half) */
} HsTile;

/* UPDATE_HASH over three bytes, reference src/deflate.c:174-175 */
DEV uint32_t hs_hash_word(uint32_t w) /* of the three low bytes of w, the first one lowest */
{
    const uint32_t b0 = w & 0xff, b1 = (w >> 8) & 0xff, b2 = (w >> 16) & 0xff;
    return ((b0 << 10) ^ (b1 << 5) ^ b2) & ZD_HASH_MASK;
}

/* the three bytes at pos in the three low bytes of a word (the top byte is whatever follows them, or 0):
 * on the usual path nothing but the load, so that a caller can have several of them in flight */
DEV uint32_t hs_word3(const uint8_t *in, uint32_t pos, uint32_t n)
{
    if (pos + 4 <= n)
        return ld_u32(in + pos);
    return (uint32_t)in[pos] | ((uint32_t)in[pos + 1] << 8) | ((uint32_t)in[pos + 2] << 16);
}

DEV uint32_t hs_hash3(const uint8_t *in, uint32_t pos, uint32_t n)
{
    return hs_hash_word(hs_word3(in, pos, n));
}

DEV uint32_t hs_slice(uint32_t m)
{
    uint32_t per = (m + HS_WAVES * WAVE - 1) / (HS_WAVES * WAVE);
    return per * WAVE;
}

/* Steps (of WAVE positions) a wave takes through a scatter as one unit: all their loads, then their
 * multi-splits in step order, then all their stores.  A gfx9 wave counts loads and stores with one
 * counter that retires in order, so the wait for a step's load is also a wait for every scattered
 * store issued before it; a wave that loops over single steps has one store round trip per step on its
 * critical path, a batch has one per HS_SCATTER_BATCH steps. */
#define HS_SCATTER_BATCH 4

/* One batch of a wave's scatter: the steps at s, s + WAVE, ... of its positions [lo, end).  FULL: every
 * lane of every step has a position (all but a wave's last batch) -- one piece of straight-line code, in
 * which the compiler keeps the loads, and then the stores, in flight together; where lanes have to be
 * switched off step by step it cuts the code into pieces that each wait for the memory operations before. */
template <bool FULL>
DEV void hs_scatter_batch(const HsTile &t, HsLds *lds, int w, int pass, uint32_t s, uint32_t lo, uint32_t end,
                          uint32_t slice)
{
    const int nbits = pass == 0 ? 8 : 7;
    uint32_t *off = pass == 0 ? lds->cnt0 : lds->cnt1;
    LANEARR(uint32_t, ent, HS_SCATTER_BATCH);
    LANEARR(uint32_t, dst, HS_SCATTER_BATCH);
    /* 1. the loads of every step: pass 0 the input word of every position, pass 1 its entry in tmp
     * (a lane without a position loads the wave's first one over again and drops it) */
    UNROLL_FULL
    for (uint32_t k = 0; k < HS_SCATTER_BATCH; k++) {
        FOR_LANES
        {
            const uint32_t i = s + k * WAVE + (uint32_t)LANE;
            const uint32_t ii = FULL || i < end ? i : lo;
            LVA(ent, k) = pass == 0 ? hs_word3(t.in, t.start + ii, t.n) : t.tmp[ii];
            LVA(dst, k) = 0;
        }
    }
    /* 2. where every entry goes, step by step in ascending order: a step reads the offsets of its
     * digits and moves them past its own entries before the next step reads them (stability) */
    UNROLL_FULL
    for (uint32_t k = 0; k < HS_SCATTER_BATCH; k++) {
        if (FULL || s + k * WAVE < end) {
            LANEVAR(uint32_t, dig);
            LANEVAR(int, ok);
            FOR_LANES
            {
                const uint32_t i = s + k * WAVE + (uint32_t)LANE;
                LV(ok) = FULL || i < end;
                if (pass == 0) /* the entry of the position from its input word */
                    LVA(ent, k) = i | (hs_hash_word(LVA(ent, k)) << 16);
                LV(dig) = pass == 0 ? ((LVA(ent, k) >> 16) & 0xff) : (LVA(ent, k) >> 24);
            }
            /* ballot multi-split: lanes with the same digit find each other */
            LANEVAR(uint64_t, peers);
            uint64_t live = BALLOT(ok);
            FOR_LANES { LV(peers) = live; }
            for (int b = 0; b < nbits; b++) {
                LANEVAR(int, bit);
                FOR_LANES { LV(bit) = (int)((LV(dig) >> b) & 1u); }
                uint64_t ones = BALLOT(bit);
                FOR_LANES { LV(peers) &= LV(bit) ? ones : ~ones; }
            }
            FOR_LANES
            {
                if (LV(ok)) {
                    uint32_t before = (uint32_t)POPC64(LV(peers) & ((1ull << LANE) - 1ull));
                    LVA(dst, k) = off[LV(dig) * HS_WAVES + (uint32_t)w] + before;
                }
            }
            FOR_LANES
            {
                if (LV(ok)) {
                    uint64_t mine = LV(peers);
                    if ((mine & ((1ull << LANE) - 1ull)) == 0) /* first lane of its digit group */
                        off[LV(dig) * HS_WAVES + (uint32_t)w] += (uint32_t)POPC64(mine);
                }
            }
        }
    }
    /* 3. the stores of every step */
    UNROLL_FULL
    for (uint32_t k = 0; k < HS_SCATTER_BATCH; k++) {
        FOR_LANES
        {
            if (FULL || s + k * WAVE + (uint32_t)LANE < end) {
                if (pass == 0) {
                    t.tmp[LVA(dst, k)] = LVA(ent, k);
                    /* the second pass counts its digits per wave slice of tmp: where this entry
                     * lands decides the slice, so that count is taken here and the counting
                     * pass over tmp is saved */
                    LDS_ADD_U32(&lds->cnt1[(LVA(ent, k) >> 24) * HS_WAVES + LVA(dst, k) / slice], 1u);
                } else {
                    t.sorted[LVA(dst, k)] = LVA(ent, k);
                    t.rank[t.start + (LVA(ent, k) & ZD_TILE_MASK)] = (uint16_t)LVA(dst, k);
                }
            }
        }
    }
}

/* stable scatter of one pass; pass 1 reads its entries from tmp */
DEV void hs_scatter(const HsTile &t, HsLds *lds, int w, int pass)
{
    const uint32_t slice = hs_slice(t.m);
    const uint32_t lo = (uint32_t)w * slice;
    const uint32_t end = lo + slice < t.m ? lo + slice : t.m; /* the wave's positions are [lo, end) */
    uint32_t s = lo;
    for (; s + HS_SCATTER_BATCH * WAVE <= end; s += HS_SCATTER_BATCH * WAVE)
        hs_scatter_batch<true>(t, lds, w, pass, s, lo, end, slice);
    if (s < end) /* fewer steps than a batch, or a last step that is not full */
        hs_scatter_batch<false>(t, lds, w, pass, s, lo, end, slice);
}

DEV void hs_count(const HsTile &t, HsLds *lds, int w, int pass)
{
    const uint32_t slice = hs_slice(t.m);
    const uint32_t lo = (uint32_t)w * slice;
    uint32_t *cnt = pass == 0 ? lds->cnt0 : lds->cnt1;
    for (uint32_t s = lo; s < lo + slice && s < t.m; s += WAVE) {
        FOR_LANES
        {
            uint32_t i = s + (uint32_t)LANE;
            if (i < t.m) {
                uint32_t d;
                if (pass == 0)
                    d = hs_hash3(t.in, t.start + i, t.n) & 0xff;
                else
                    d = t.tmp[i] >> 24;
                LDS_ADD_U32(&cnt[d * HS_WAVES + (uint32_t)w], 1u);
            }
        }
    }
}

/* exclusive scan of ndig*HS_WAVES counters, digit-major; done by wave 0 */
DEV void hs_scan(uint32_t *cnt, int ndig)
{
    uint32_t run = 0;
    const int total = ndig * HS_WAVES;
    for (int s = 0; s < total; s += WAVE) {
        LANEVAR(uint32_t, v);
        LANEVAR(uint32_t, ex);
        FOR_LANES { LV(v) = cnt[s + LANE]; }
        uint32_t tot;
        WAVE_EXSCAN(v, ex, tot);
        FOR_LANES { cnt[s + LANE] = run + LV(ex); }
        run += tot;
    }
}

DEV void hs_directory(const HsTile &t, int w)
{
    /* bucket starts: sorted index i opens every bucket in (h[i-1], h[i]] */
    /* (the loads of HS_SCATTER_BATCH steps before the first store, as in hs_scatter) */
    for (uint32_t s = (uint32_t)w * WAVE; s < t.m; s += HS_SCATTER_BATCH * HS_WAVES * WAVE) {
        LANEARR(uint32_t, cur, HS_SCATTER_BATCH);
        LANEARR(uint32_t, prv, HS_SCATTER_BATCH);
        UNROLL_FULL
        for (uint32_t k = 0; k < HS_SCATTER_BATCH; k++) {
            FOR_LANES
            {
                const uint32_t i = s + k * HS_WAVES * WAVE + (uint32_t)LANE;
                const uint32_t ii = i < t.m ? i : 0; /* (a lane past m loads entry 0 and drops it) */
                LVA(cur, k) = t.sorted[ii];
                LVA(prv, k) = t.sorted[ii ? ii - 1 : 0]; /* (not used where i is 0) */
            }
        }
        UNROLL_FULL
        for (uint32_t k = 0; k < HS_SCATTER_BATCH; k++) {
            FOR_LANES
            {
                const uint32_t i = s + k * HS_WAVES * WAVE + (uint32_t)LANE;
                if (i < t.m) {
                    const int32_t h = (int32_t)(LVA(cur, k) >> 16);
                    const int32_t hp = i == 0 ? -1 : (int32_t)(LVA(prv, k) >> 16);
                    for (int32_t hh = hp + 1; hh <= h; hh++)
                        t.dir[hh] = (uint16_t)i;
                }
            }
        }
    }
    /* buckets past the last occupied one (and the end sentinel) point at m */
    int32_t hl = t.m == 0 ? -1 : (int32_t)(t.sorted[t.m - 1] >> 16);
    for (int32_t s = hl + 1 + w * WAVE; s <= 32768; s += HS_WAVES * WAVE) {
        FOR_LANES
        {
            int32_t hh = s + LANE;
            if (hh <= 32768)
                t.dir[hh] = (uint16_t)t.m;
        }
    }
}

/* kernel 1b (after every tile of the batch has its directory): for each position of
 * this tile, how long its chain is inside the tile, and where its hash bucket lies in
 * the PREVIOUS tile's sorted array.  With rank[] this makes a position's whole chain
 * addressable up front -- the parser never does a dependent table lookup and never
 * has to look at an entry to find the end of a bucket. */
#define HS_LINK_BATCH 4 /* steps whose loads are all issued before the first store (a gfx9 load waits for earlier stores) */
DEV void hs_link_prev(const HsTile &t, int w)
{
    for (uint32_t s = (uint32_t)w * WAVE; s < t.m; s += HS_LINK_BATCH * HS_WAVES * WAVE) {
        LANEARR(uint32_t, h, HS_LINK_BATCH);
        LANEARR(uint32_t, rk, HS_LINK_BATCH);
        LANEARR(uint32_t, d0, HS_LINK_BATCH);
        LANEARR(uint32_t, plo, HS_LINK_BATCH);
        LANEARR(uint32_t, pend, HS_LINK_BATCH);
        UNROLL_FULL
        for (uint32_t k = 0; k < HS_LINK_BATCH; k++) {
            FOR_LANES
            {
                const uint32_t i = s + k * HS_WAVES * WAVE + (uint32_t)LANE;
                LVA(h, k) = 0;
                LVA(rk, k) = 0;
                if (i < t.m) {
                    LVA(h, k) = hs_hash3(t.in, t.start + i, t.n);
                    LVA(rk, k) = (uint32_t)t.rank[t.start + i];
                }
            }
        }
        UNROLL_FULL
        for (uint32_t k = 0; k < HS_LINK_BATCH; k++) {
            FOR_LANES
            {
                const uint32_t i = s + k * HS_WAVES * WAVE + (uint32_t)LANE;
                LVA(d0, k) = 0;
                LVA(plo, k) = 0;
                LVA(pend, k) = 0;
                if (i < t.m) {
                    LVA(d0, k) = t.dir[LVA(h, k)];
                    if (t.dir_prev) {
                        /* dir_prev[h] and dir_prev[h + 1] in one (2-byte aligned) load: the kernel is
                         * bound by the rate of its scattered reads */
                        const uint32_t two = ld_u32((const uint8_t *)(t.dir_prev + LVA(h, k)));
                        LVA(plo, k) = two & 0xffffu;
                        LVA(pend, k) = two >> 16;
                    }
                }
            }
        }
        UNROLL_FULL
        for (uint32_t k = 0; k < HS_LINK_BATCH; k++) {
            FOR_LANES
            {
                const uint32_t i = s + k * HS_WAVES * WAVE + (uint32_t)LANE;
                if (i < t.m) {
                    uint32_t c = LVA(rk, k) - LVA(d0, k), hb = 0xffffu;
                    if (t.dir_prev) {
                        hb = (LVA(pend, k) - 1u) & 0xffffu; /* 0xffff: bucket empty from the start */
                        t.hib[t.start + i] = (uint16_t)hb;
                        c |= (LVA(pend, k) - LVA(plo, k)) << 16;
                    }
                    t.cnt[t.start + i] = c;
                }
            }
        }
    }
}

/* one phase of the tile sort, executed by wave `w` of the tile's workgroup;
 * the caller puts a workgroup barrier between phases */
DEV void hash_sort_phase(const HsTile &t, HsLds *lds, int w, int phase)
{
    switch (phase) {
    case 0:
        for (int i = w * WAVE; i < 256 * HS_WAVES; i += HS_WAVES * WAVE) {
            FOR_LANES { lds->cnt0[i + LANE] = 0; }
        }
        for (int i = w * WAVE; i < 128 * HS_WAVES; i += HS_WAVES * WAVE) {
            FOR_LANES { lds->cnt1[i + LANE] = 0; }
        }
        break;
    case 1:
        hs_count(t, lds, w, 0);
        break;
    case 2:
        if (w == 0)
            hs_scan(lds->cnt0, 256);
        break;
    case 3:
        hs_scatter(t, lds, w, 0);
        break;
    case 4:
        break; /* counted while scattering (hs_scatter, pass 0) */
    case 5:
        if (w == 0)
            hs_scan(lds->cnt1, 128);
        break;
    case 6:
        hs_scatter(t, lds, w, 1);
        break;
    case 7:
        hs_directory(t, w);
        break;
    }
}
#define HS_PHASES 8

#endif
