/*
 * pack.h -- a plan's results moved into one contiguous image, and back.
 *
 * A plan leaves item i at sparse_off[i] (a multiple of 16) in a slot sized for the worst case; how long the
 * item is, is known on the device only (ZdResult / InfResult).  Two pieces of wavefront code, written once
 * for the GPU and for the lane emulation of the CPU tests:
 *
 *   pk_scan_block   the dense offsets: an exclusive prefix sum of the item lengths, each rounded up to
 *                   `align`, as 64-bit values, for any 32-bit count.  One wave takes PK_SCAN_B values;
 *                   more values than that are summed per wave first (reduce), the sums are scanned the
 *                   same way (recursively: pk_scan_levels), and a last pass adds each wave's base (apply).
 *                   Every pass is a launch of its own: no workgroup waits for another one.
 *   pk_move_tile    the bytes: one wave moves ZSC_HIP_PACK_TILE bytes of the DENSE side.  It finds the first
 *                   item of its tile by a wave-uniform binary search in the offsets and walks the items
 *                   that overlap the tile; of each it moves the part inside the tile, one 16-byte granule
 *                   of the DESTINATION per lane and step.  Whole destination granules are written with one
 *                   aligned 16-byte store, the partial ones at an item's head and tail byte by byte, so a
 *                   granule shared by several short items is written by each of them in its own bytes only.
 *                   The source of a granule is two aligned 16-byte loads and a funnel shift, since source
 *                   and destination are misaligned against each other by any amount.  Only source granules
 *                   that hold a byte of the item are loaded, and none whole beyond `src_end`.
 *                   pack:   sparse slots -> dense image, the padding up to `align` written as zeros
 *                   unpack: dense image -> sparse slots, the item's own bytes and nothing else
 */
#ifndef ZSC_PACK_H
#define ZSC_PACK_H

#include "wave.h"
#include "zsc_hip.h"

#define PK_TILE ((uint64_t)ZSC_HIP_PACK_TILE)
#define PK_SCAN_B 1024u /* values per scan wave: count <= B one launch, <= B * B three, <= B^3 five, any U32 seven */
#define PK_MAX_LEVELS 4

/* Where the items' lengths are: records of stride_w words, the length in word len_w; an item whose word
 * st_w is not 0 has length 0 (PK_NO_STATUS: every length counts). */
#define PK_NO_STATUS 0xffffffffu
typedef struct {
    const uint32_t *rec;
    uint32_t stride_w, len_w, st_w;
} PkLens;

DEV uint32_t pk_len(const PkLens &L, uint64_t i)
{
    const uint32_t *r = L.rec + i * L.stride_w;
    if (L.st_w != PK_NO_STATUS && r[L.st_w] != 0u)
        return 0u;
    return r[L.len_w];
}

DEV uint64_t pk_round_up(uint64_t v, uint32_t align)
{
    return (v + (align - 1u)) & ~(uint64_t)(align - 1u);
}

/* The scan's levels (host and device agree on them): n[0] = count values, n[k + 1] = the waves of level k,
 * up to the first level one wave takes alone.  Returns the number of levels. */
static inline uint32_t pk_scan_levels(uint64_t count, uint64_t n[PK_MAX_LEVELS])
{
    uint32_t k = 0;
    n[0] = count;
    while (n[k] > PK_SCAN_B) {
        n[k + 1u] = (n[k] + PK_SCAN_B - 1u) / PK_SCAN_B;
        k++;
    }
    return k + 1u;
}

/* Wave g of a level of n values: values [g * B, +B), WAVE at a time.  The values are vals[] or, without vals,
 * the item lengths rounded up to align.
 *   out == null  reduce: sums[g] = the sum of the wave's values
 *   out != null  apply:  out[i] = base[g] (0 without base) + the values before i; the wave that holds the
 *                last value (or wave 0 of no values) also writes out[n], the sum of everything.  out may be
 *                vals: every value is read before its place is written. */
DEV void pk_scan_block(const PkLens &lens, uint32_t align, const uint64_t *vals, uint64_t n, uint64_t g,
                       const uint64_t *base, uint64_t *out, uint64_t *sums)
{
    const uint64_t first = g * PK_SCAN_B;
    uint64_t run = (out && base) ? base[g] : 0u;
    for (uint32_t k = 0; k < PK_SCAN_B && first + k < n; k += WAVE) {
        /* a 64-bit scan from the 32-bit one: three slices of 26 bits, whose sums over 64 lanes fit */
        LANEVAR(uint32_t, p0);
        LANEVAR(uint32_t, p1);
        LANEVAR(uint32_t, p2);
        LANEVAR(uint32_t, e0);
        LANEVAR(uint32_t, e1);
        LANEVAR(uint32_t, e2);
        FOR_LANES
        {
            const uint64_t i = first + k + (uint32_t)LANE;
            uint64_t v = 0;
            if (i < n)
                v = vals ? vals[i] : pk_round_up(pk_len(lens, i), align);
            LV(p0) = (uint32_t)v & 0x3ffffffu;
            LV(p1) = (uint32_t)(v >> 26) & 0x3ffffffu;
            LV(p2) = (uint32_t)(v >> 52);
        }
        uint32_t t0, t1, t2;
        WAVE_EXSCAN(p0, e0, t0);
        WAVE_EXSCAN(p1, e1, t1);
        WAVE_EXSCAN(p2, e2, t2);
        if (out) {
            FOR_LANES
            {
                const uint64_t i = first + k + (uint32_t)LANE;
                if (i < n)
                    out[i] = run + LV(e0) + ((uint64_t)LV(e1) << 26) + ((uint64_t)LV(e2) << 52);
            }
        }
        run += t0 + ((uint64_t)t1 << 26) + ((uint64_t)t2 << 52);
    }
    if (out) {
        if (first + PK_SCAN_B >= n) {
            ON_LANE0 out[n] = run;
        }
    } else {
        ON_LANE0 sums[g] = run;
    }
}

/* ---- the move ------------------------------------------------------------------------------------------ */

typedef struct __attribute__((aligned(16))) {
    uint32_t w[4];
} PkQ;

DEV uint32_t pk_funnel(uint32_t hi, uint32_t lo, uint32_t bs) /* bytes bs .. bs + 3 of hi:lo */
{
    return bs ? (lo >> (8u * bs)) | (hi << (32u - 8u * bs)) : lo;
}

/* the aligned source granule at `at`, of which bytes [sa, sb) are wanted: one 16-byte load where the whole
 * granule lies below src_end, else the wanted bytes one by one (the rest 0) */
DEV PkQ pk_load_granule(const uint8_t *src, uint64_t at, uint64_t sa, uint64_t sb, uint64_t src_end)
{
    PkQ q;
    if (at + 16u <= src_end) {
        COPY16(&q, src + at);
    } else {
        q.w[0] = q.w[1] = q.w[2] = q.w[3] = 0u;
        UNROLL_FULL
        for (uint32_t k = 0; k < 16u; k++)
            if (at + k >= sa && at + k < sb)
                q.w[k >> 2] |= (uint32_t)src[at + k] << (8u * (k & 3u));
    }
    return q;
}

/* One destination granule (one lane).  The segment is destination bytes [e0, e1), of which the first ndata
 * come from src[s0 ...] and the rest are zeros; gp, a multiple of 16 like the destination's base, is a
 * granule that holds at least one of them. */
DEV void pk_granule(uint8_t *dst, uint64_t gp, uint64_t e0, uint64_t e1, const uint8_t *src, uint64_t s0,
                    uint64_t ndata, uint64_t src_end)
{
    const uint64_t lo = gp > e0 ? gp : e0, hi = gp + 16u < e1 ? gp + 16u : e1; /* this granule's bytes */
    const uint64_t dend = e0 + ndata;
    const uint64_t dhi = hi < dend ? hi : dend; /* [lo, dhi): those that are data */
    PkQ o;
    o.w[0] = o.w[1] = o.w[2] = o.w[3] = 0u;
    if (dhi > lo) {
        const uint64_t sa = s0 + (lo - e0), sb = s0 + (dhi - e0); /* their source bytes */
        /* the source byte that lands in byte 0 of the granule; before the source's start (by 15 at most)
         * where the segment begins inside the granule */
        const int64_t sp = (int64_t)sa - (int64_t)(lo - gp);
        const uint32_t shift = (uint32_t)sp & 15u;
        const int64_t ga = sp - (int64_t)shift, gb = ga + 16;
        PkQ a, b;
        a.w[0] = a.w[1] = a.w[2] = a.w[3] = 0u;
        b = a;
        if (gb > (int64_t)sa) /* (and ga < sb: ga <= sp < sb) */
            a = pk_load_granule(src, (uint64_t)ga, sa, sb, src_end);
        if (gb < (int64_t)sb)
            b = pk_load_granule(src, (uint64_t)gb, sa, sb, src_end);
        uint32_t w0 = a.w[0], w1 = a.w[1], w2 = a.w[2], w3 = a.w[3], w4 = b.w[0], w5 = b.w[1], w6 = b.w[2],
                 w7 = b.w[3];
        if (shift & 4u) {
            w0 = w1, w1 = w2, w2 = w3, w3 = w4, w4 = w5, w5 = w6, w6 = w7;
        }
        if (shift & 8u) {
            w0 = w2, w1 = w3, w2 = w4, w3 = w5, w4 = w6;
        }
        const uint32_t bs = shift & 3u;
        o.w[0] = pk_funnel(w1, w0, bs);
        o.w[1] = pk_funnel(w2, w1, bs);
        o.w[2] = pk_funnel(w3, w2, bs);
        o.w[3] = pk_funnel(w4, w3, bs);
        /* what lies behind the data is padding: zeros */
        const uint32_t nz = (uint32_t)(dhi - gp); /* 1 .. 16 */
        UNROLL_FULL
        for (uint32_t k = 0; k < 4u; k++) {
            if (nz <= 4u * k)
                o.w[k] = 0u;
            else if (nz < 4u * k + 4u)
                o.w[k] &= (1u << (8u * (nz - 4u * k))) - 1u;
        }
    }
    if (lo == gp && hi == gp + 16u) {
        COPY16(dst + gp, &o);
    } else {
        UNROLL_FULL
        for (uint32_t k = 0; k < 16u; k++)
            if (gp + k >= lo && gp + k < hi)
                dst[gp + k] = (uint8_t)(o.w[k >> 2] >> (8u * (k & 3u)));
    }
}

/* a segment by the whole wave: one destination granule per lane and step */
DEV void pk_segment(uint8_t *dst, uint64_t e0, uint64_t e1, const uint8_t *src, uint64_t s0, uint64_t ndata,
                    uint64_t src_end)
{
    for (uint64_t g = e0 & ~15ull; g < e1; g += 16ull * WAVE) {
        FOR_LANES
        {
            const uint64_t gp = g + 16ull * (uint32_t)LANE;
            if (gp < e1)
                pk_granule(dst, gp, e0, e1, src, s0, ndata, src_end);
        }
    }
}

typedef struct {
    const uint64_t *off;        /* count + 1 dense offsets, ascending; off[count]: the image's length */
    const uint64_t *sparse_off; /* count slot offsets, multiples of 16 */
    PkLens lens;                /* item i: lens bytes at off[i]; what follows up to off[i + 1] is padding */
    uint32_t count;
    uint32_t unpack;
    uint64_t cap;               /* pack: the bytes the dense image may take */
} PkMove;

/* Tile `tile` of the dense side.  dense and sparse: the two images' bases, both 16-byte aligned.  Nothing
 * moves where the image is longer than cap, and a tile behind the image's end returns at once. */
DEV void pk_move_tile(const PkMove &M, uint8_t *dense, uint8_t *sparse, uint64_t tile)
{
    const uint64_t total = M.off[M.count];
    if (!M.unpack && total > M.cap)
        return;
    const uint64_t t0 = tile * PK_TILE;
    if (t0 >= total)
        return;
    const uint64_t t1 = t0 + PK_TILE < total ? t0 + PK_TILE : total;
    /* the first item that ends behind t0 (there is one: the last item ends at total) */
    uint32_t lo = 0, hi = M.count - 1u;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (M.off[mid + 1u] > t0)
            hi = mid;
        else
            lo = mid + 1u;
    }
    for (uint32_t i = lo; i < M.count; i++) {
        const uint64_t a = M.off[i];
        if (a >= t1)
            break;
        const uint64_t b = M.off[i + 1u];
        const uint64_t d0 = a > t0 ? a : t0, d1 = b < t1 ? b : t1; /* the item's part of the tile */
        if (d1 <= d0)
            continue;
        uint64_t n = pk_len(M.lens, i);
        if (n > b - a) /* (the offsets were made from these lengths) */
            n = b - a;
        const uint64_t dend = a + n < d1 ? a + n : d1; /* the data in it ends here */
        const uint64_t so = M.sparse_off[i];
        if (!M.unpack)
            pk_segment(dense, d0, d1, sparse, so + (d0 - a), dend > d0 ? dend - d0 : 0u, ~0ull);
        else if (dend > d0)
            pk_segment(sparse, so + (d0 - a), so + (dend - a), dense, d0, dend - d0, total);
    }
}

#endif
