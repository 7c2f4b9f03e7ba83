/*
 * inflate_sections.h -- kernel 6: one stream's full-flush sections inflated in parallel
 * (DESIGN.md section 7).
 *
 * A stream written with Z_FULL_FLUSH every max_block_len bytes (src/zsc_compress.c:121-138) is a
 * chain of sections, each ending in a non-final empty stored block whose LEN/NLEN are the
 * byte-aligned 00 00 FF FF, and each decodable without the output before it.  The steps, each
 * a launch of its own (zsc_hip_runtime.hip):
 *   1. scan     every stream's bytes for 00 00 FF FF, one wavefront per 64 * WAVE bytes: the
 *               positions just behind the patterns are the candidate section starts (twice: count
 *               per tile, then, after setup, write them in order);
 *   2. setup    per stream with candidates: the tiles' offsets in its candidate list; position
 *               0 (the header) is always candidate 0;
 *   3. count    every candidate decoded by one group, nothing stored (inflate_stream with
 *               INF_SEC_STOP | INF_SEC_COUNT | INF_SEC_NOTRAIL): output length, where it stopped,
 *               the longest distance, an outcome; candidate 0 with the stream's wrapper, the
 *               others raw;
 *   4. resolve  per stream: follow the chain from candidate 0 -- a section that ended at a
 *               marker continues at the candidate where it stopped -- to the one that reached
 *               the final block; output offsets by a running sum;
 *   5. write    every section of every resolved chain decoded again into its place, and the
 *               Adler-32 / CRC-32 of its own slice;
 *   6. finish   per stream: the slice checksums combined, compared with the trailer (and ISIZE);
 *               a stream that passes is finished: status Z_OK, resume state 2.
 * Then k_inflate runs over the whole plan as usual and decodes every other stream serially.
 * The new path only ever reports a clean Z_OK; every other outcome -- data errors and their
 * resynchronisation, Z_BUF_ERROR, Z_NEED_DICT, truncation, a wrong trailer, a section that
 * needs the history of an earlier one, a candidate list that overflows, the work bound -- is
 * left to the serial decoder, so the results equal zsc_hip_uncompress_batch's by construction.
 *
 * Why local decoding is sound: a section decoded from its start rejects every distance beyond
 * its own output, where the reference rejects only distances beyond the whole output so far;
 * every other check of the decoder is local to a block.  So a chain of sections that all pass
 * locally passes in the reference too, with the same bytes.  The distance limit of a zlib header
 * (dmax) is only known to candidate 0, so the others are decoded with 32 KiB and the resolve step
 * compares each section's longest distance with the header's limit.
 */
#ifndef ZSC_INFLATE_SECTIONS_H
#define ZSC_INFLATE_SECTIONS_H

#include "inflate.h"

#define SEC_TILE (WAVE * 64u)    /* input bytes one wavefront scans: four steps of 16 per lane */
#define SEC_CAND_DIV 32u         /* candidates a stream may have: source_len / 32 + 8 */
#define SEC_CAND_MIN 8u
/* candidate records of all streams come from one pool, taken by the streams that have candidates:
 * (sum of source_lens) / 256 + 64 Ki slots -- sections of 256 compressed bytes on average; a stream
 * that finds the pool used up stays serial */
#define SEC_POOL_SLOTS(total_in) ((total_in) / 256u + 65536u)
#define SEC_WORK_MUL 4u          /* the count pass stops decoding a stream's candidates once they */
#define SEC_WORK_ADD 65536u      /* have consumed 4 * source_len + 64 KiB input bytes */
#define SEC_LINK_NIL 0x0fffffffu /* link of a candidate: did not end cleanly at a candidate */
#define SEC_LINK_FIN 0x0ffffffeu /* ... reached the final block */

#ifdef ZSC_WAVE_EMU
#define SEC_ADD(p, v) ((*(p) += (v)) - (v))
#define SEC_OR(p, v) (*(p) |= (v))
#define SEC_CAS(p, e, d) (*(p) == (e) ? (*(p) = (d), (e)) : *(p))
#define SEC_LOAD(p) (*(p))
#define SEC_FENCE() ((void)0)
#else
#define SEC_ADD(p, v) atomicAdd((p), (v))
#define SEC_OR(p, v) atomicOr((p), (v))
#define SEC_CAS(p, e, d) atomicCAS((p), (e), (d))
#define SEC_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define SEC_FENCE() __threadfence_block()
#endif

/* one stream of a sections plan (host-built, read-only) */
typedef struct {
    uint64_t src_off, dst_off;
    uint32_t src_len, dst_cap;
    uint32_t cap; /* candidates it may have */
    uint32_t tile0, ntiles;
    uint32_t pad;
} IsecItem;

typedef struct {
    uint32_t stream, start;
} IsecTile;

/* per stream, set up by sec_setup for the streams with candidates */
typedef struct {
    unsigned long long work; /* input bytes the count pass has decoded */
    uint32_t ncand;          /* candidates (0: the stream stays serial) */
    uint32_t take, take2;    /* count / write queue positions */
    uint32_t serial;         /* set: overflow, work bound, a write pass that disagreed */
    uint32_t nchain;         /* sections of the resolved chain (0: none) */
    uint32_t head;           /* candidate 0: gzip | log2(dmax) << 8 */
    uint32_t total;          /* output bytes of the chain */
    uint32_t trailer;        /* input offset of the trailer */
    uint32_t base;           /* its candidate records start here in the pool */
    uint32_t pad;
} IsecStream;

typedef struct {
    const IsecItem *items;
    const IsecTile *tiles;
    uint32_t *tile_cnt, *tile_off;
    uint32_t *scount; /* per stream: candidates found by the scan (zeroed before every run) */
    uint32_t *nsec;   /* per stream: sections decoded in parallel (zeroed before every run) */
    IsecStream *st;
    uint32_t *active; /* the streams with candidates, in the order the scan found them */
    uint32_t *q;      /* [0] active streams, [1] count queue, [2] write queue, [3] pool slots taken
                       * (zeroed before every run) */
    uint32_t *cstart, *cstop, *clink, *clen; /* per candidate (pool slot) */
    uint32_t *chain_k, *chain_off, *chain_ck; /* per section of the chain (pool slot) */
    uint32_t count, ntiles, pool;
    int32_t window_bits;
    uint32_t work_mul, work_add;
} IsecPlan;

/* ---- whole-wave code: scan and setup ---- */

/* what the scan looks for, as template arguments of the scan.  HIT(v, p, n): the four bytes v at position p of
 * a stream of n bytes are a pattern; the candidate is then p + ADV.  ENLIST_ALL: every stream with a tile joins
 * the active list (at its first tile), not only those with a pattern. */
DEV bool sec_hit_flush(uint32_t v, uint32_t p, uint32_t n)
{
    return v == 0xffff0000u && p + 4u < n;
}

/* step 1 for tile t: write = 0 counts the candidates (and enlists the stream), write = 1 stores
 * their positions in order.  Step k of the four reads 16 * WAVE contiguous bytes, 16 per lane (one
 * dwordx4 load), and the dword behind them: a pattern may straddle lanes, steps and tiles. */
template <bool (*HIT)(uint32_t, uint32_t, uint32_t), uint32_t ADV, bool ENLIST_ALL>
DEV void sec_scan_tile_for(const IsecPlan &P, const uint8_t *src_all, uint32_t t, int write)
{
    const uint32_t s = GUNI(P.tiles[t].stream);
    const uint32_t t0 = GUNI(P.tiles[t].start);
    const uint8_t *src = src_all + P.items[s].src_off;
    const uint32_t n = GUNI(P.items[s].src_len);
    if (write && (GUNI(P.tile_cnt[t]) == 0u || GUNI(P.st[s].ncand) == 0u))
        return;
    LANEVAR(uint64_t, hits); /* bit 16 k + b: a pattern at t0 + 16 WAVE k + 16 LANE + b */
    LANEVAR(uint32_t, cnt);
    FOR_LANES
    {
        uint64_t m = 0;
        for (uint32_t k = 0; k < 4u; k++) {
            const uint32_t a = t0 + 16u * WAVE * k + 16u * (uint32_t)LANE;
            if (a >= n)
                break;
            alignas(16) uint32_t w[8];
            if (a + 16u <= n) {
                COPY16(w, src + a); /* (streams are 16-byte aligned, so is a) */
            } else {
                for (int j = 0; j < 4; j++)
                    w[j] = inf_input_dword(src, a + 4u * (uint32_t)j, n);
            }
            w[4] = inf_input_dword(src, a + 16u, n);
            for (int j = 0; j < 4; j++) {
                for (int sh = 0; sh < 4; sh++) {
                    const uint32_t v = sh ? (w[j] >> (8 * sh)) | (w[j + 1] << (32 - 8 * sh)) : w[j];
                    const uint32_t p = a + 4u * (uint32_t)j + (uint32_t)sh;
                    if (HIT(v, p, n))
                        m |= 1ull << (16u * k + 4u * (uint32_t)j + (uint32_t)sh);
                }
            }
        }
        LV(hits) = m;
        LV(cnt) = (uint32_t)POPC64(m);
    }
    if (!write) {
        uint32_t total = (uint32_t)WAVE_SUM(cnt);
        ON_LANE0
        {
            P.tile_cnt[t] = total;
            if constexpr (ENLIST_ALL) {
                if (total)
                    SEC_ADD(&P.scount[s], total);
                if (t0 == 0u)
                    P.active[SEC_ADD(&P.q[0], 1u)] = s;
            } else
            if (total && SEC_ADD(&P.scount[s], total) == 0u)
                P.active[SEC_ADD(&P.q[0], 1u)] = s;
        }
        return;
    }
    /* positions ascend by step, then lane, then bit */
    uint32_t at = GUNI(P.st[s].base) + 1u + GUNI(P.tile_off[t]);
    for (uint32_t k = 0; k < 4u; k++) {
        LANEVAR(uint32_t, ck);
        LANEVAR(uint32_t, ex);
        FOR_LANES { LV(ck) = (uint32_t)POPC64((LV(hits) >> (16u * k)) & 0xffffu); }
        uint32_t tot;
        WAVE_EXSCAN(ck, ex, tot);
        FOR_LANES
        {
            uint32_t m = (uint32_t)((LV(hits) >> (16u * k)) & 0xffffu);
            uint32_t r = at + LV(ex);
            while (m) {
                const uint32_t b = (uint32_t)CTZ32(m);
                m &= m - 1u;
                P.cstart[r++] = t0 + 16u * WAVE * k + 16u * (uint32_t)LANE + b + ADV;
            }
        }
        at += tot;
    }
}

DEV void sec_scan_tile(const IsecPlan &P, const uint8_t *src_all, uint32_t t, int write)
{
    sec_scan_tile_for<sec_hit_flush, 4u, false>(P, src_all, t, write);
}

/* step 2 for the a-th stream with candidates */
DEV void sec_setup(const IsecPlan &P, uint32_t a)
{
    const uint32_t s = GUNI(P.active[a]);
    const IsecItem *it = &P.items[s];
    const uint32_t ncand = 1u + GUNI(P.scount[s]);
    uint32_t base = 0;
    if (ncand <= GUNI(it->cap)) {
        ON_LANE0 { base = SEC_ADD(&P.q[3], ncand); }
        base = UNI(base);
    }
    const uint32_t fits = ncand <= GUNI(it->cap) && base <= P.pool && P.pool - base >= ncand;
    ON_LANE0
    {
        IsecStream *S = &P.st[s];
        S->work = 0;
        S->ncand = fits ? ncand : 0u;
        S->take = S->take2 = 0;
        S->serial = !fits;
        S->nchain = S->head = S->total = S->trailer = 0;
        S->base = base;
        if (fits)
            P.cstart[base] = 0;
    }
    if (!fits)
        return;
    const uint32_t tile0 = GUNI(it->tile0), ntiles = GUNI(it->ntiles);
    uint32_t run = 0;
    for (uint32_t b = 0; b < ntiles; b += WAVE) {
        LANEVAR(uint32_t, c);
        LANEVAR(uint32_t, ex);
        FOR_LANES { LV(c) = b + (uint32_t)LANE < ntiles ? P.tile_cnt[tile0 + b + (uint32_t)LANE] : 0u; }
        uint32_t tot;
        WAVE_EXSCAN(c, ex, tot);
        FOR_LANES
        {
            if (b + (uint32_t)LANE < ntiles)
                P.tile_off[tile0 + b + (uint32_t)LANE] = run + LV(ex);
        }
        run += tot;
    }
}

/* ---- group code (INF_GROUP lanes per unit, as the decoder) ---- */
#undef ZSC_GROUP
#define ZSC_GROUP INF_GROUP
#include "wave_group.h"

#ifdef ZSC_WAVE_EMU
#define SEC_GBCAST(v) (v)
#else
#define SEC_GBCAST(v) ((uint32_t)__shfl((int)(v), (int)(threadIdx.x & (64u - GRP))))
#endif

/* x^(8 len) mod P, reflected */
DEV uint32_t sec_xpow8(uint32_t len)
{
    uint32_t p = 0x80000000u;
    for (uint32_t j = 0; j < 32u; j++)
        if ((len >> j) & 1u)
            p = ck_mulmod(p, ck_x2n(j + 3u));
    return p;
}

/* CRC-32 of A || B from crc(A), crc(B) and |B|: r(A || B) = r(A) x^(8|B|) + r(B) (the pre- and
 * post-inversions cancel) */
DEV uint32_t sec_crc32_combine(uint32_t c1, uint32_t c2, uint32_t len2)
{
    return ck_mulmod(c1, sec_xpow8(len2)) ^ c2;
}

/* Adler-32 of A || B: a = a1 + a2 - 1, b = b1 + b2 + |B| (a1 - 1), mod 65521 */
DEV uint32_t sec_adler32_combine(uint32_t ad1, uint32_t ad2, uint32_t len2)
{
    const uint64_t rem = len2 % CK_BASE;
    const uint64_t a1 = ad1 & 0xffffu, b1 = ad1 >> 16, a2 = ad2 & 0xffffu, b2 = ad2 >> 16;
    const uint64_t a = (a1 + a2 + CK_BASE - 1u) % CK_BASE;
    const uint64_t b = (b1 + b2 + rem * a1 + CK_BASE - rem) % CK_BASE;
    return (uint32_t)((b << 16) | a);
}

/* the next (stream, index) of a two-level queue over the active streams: q[which] is the active
 * stream being handed out, take[] its next index; a group that finds it used up moves q on.
 * Returns 0 when every stream is used up. */
template <int WHICH>
DEV int sec_next_unit(const IsecPlan &P, uint32_t *s_out, uint32_t *k_out)
{
    uint32_t s = 0, k = 0, found = 0;
    ON_GLANE0
    {
        for (;;) {
            const uint32_t a = SEC_LOAD(&P.q[WHICH]);
            if (a >= SEC_LOAD(&P.q[0]))
                break;
            s = P.active[a];
            IsecStream *S = &P.st[s];
            k = SEC_ADD(WHICH == 1 ? &S->take : &S->take2, 1u);
            if (k < (WHICH == 1 ? S->ncand : S->nchain)) {
                found = 1;
                break;
            }
            (void)SEC_CAS(&P.q[WHICH], a, a + 1u);
        }
    }
    *s_out = SEC_GBCAST(s);
    *k_out = SEC_GBCAST(k);
    return (int)SEC_GBCAST(found);
}

/* the index of candidate position `pos` of a stream (positions ascend), or SEC_LINK_NIL */
DEV uint32_t sec_find(const uint32_t *cstart, uint32_t ncand, uint32_t pos)
{
    uint32_t lo = 0, hi = ncand;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (cstart[mid] < pos)
            lo = mid + 1u;
        else
            hi = mid;
    }
    return lo < ncand && cstart[lo] == pos ? lo : SEC_LINK_NIL;
}

/* step 3: a group decodes candidates until the queue is empty */
DEV void sec_count_worker(const IsecPlan &P, const uint8_t *src_all, InfLds *lds, InfSecInfo *si)
{
    uint32_t s, k;
    while (sec_next_unit<1>(P, &s, &k)) {
        IsecStream *S = &P.st[s];
        const IsecItem *it = &P.items[s];
        const uint32_t n = GUNI(it->src_len);
        if (GUNI(S->serial))
            continue;
        if ((unsigned long long)SEC_LOAD(&S->work) > (unsigned long long)P.work_mul * n + P.work_add) {
            ON_GLANE0 { SEC_OR(&S->serial, 1u); }
            continue;
        }
        const uint32_t cb = GUNI(S->base);
        const uint32_t start = GUNI(P.cstart[cb + k]);
        InfJob job;
        job.src = src_all + it->src_off + start;
        job.n = n - start;
        job.dst = nullptr;
        job.cap = GUNI(it->dst_cap);
        job.window_bits = k == 0u ? P.window_bits : -15;
        inflate_stream<INF_SEC_STOP | INF_SEC_COUNT | INF_SEC_NOTRAIL>(job, lds, nullptr, nullptr, si);
        const uint32_t outcome = GUNI(si->outcome), stop = start + GUNI(si->stop);
        const uint32_t maxd = GUNI(si->maxd);
        ON_GLANE0
        {
            uint32_t link = SEC_LINK_NIL;
            if (outcome == INF_SEC_SYNC)
                link = sec_find(P.cstart + cb, S->ncand, stop);
            else if (outcome == INF_SEC_FINAL)
                link = SEC_LINK_FIN;
            const uint32_t dlog = maxd ? 32u - CLZ32(maxd - 1u) : 0u; /* ceil(log2) */
            P.clink[cb + k] = link | dlog << 28;
            P.clen[cb + k] = si->out_len;
            P.cstop[cb + k] = stop;
            if (k == 0u)
                S->head = si->gzip | (31u - CLZ32(si->dmax)) << 8;
            SEC_ADD(&S->work, (unsigned long long)(stop - start));
        }
        WAVE_SYNC();
    }
}

/* step 4 for the a-th active stream: the chain from candidate 0, GRP links read at a time */
DEV void sec_resolve(const IsecPlan &P, uint32_t a)
{
    const uint32_t s = GUNI(P.active[a]);
    IsecStream *S = &P.st[s];
    const IsecItem *it = &P.items[s];
    const uint32_t ncand = GUNI(S->ncand);
    if (ncand == 0u || GUNI(S->serial))
        return;
    const uint32_t cb = GUNI(S->base);
    const uint32_t dlog = (GUNI(S->head) >> 8) & 31u, cap = GUNI(it->dst_cap);
    LANEVAR(uint32_t, lk);
    LANEVAR(uint32_t, ln);
    uint32_t k = 0, wbase = 0, j = 0, ok = 0, trailer = 0;
    uint64_t sum = 0;
    int loaded = 0;
    for (;;) {
        if (!loaded || k - wbase >= GRP) {
            wbase = k;
            loaded = 1;
            FOR_GLANES
            {
                const uint32_t i = wbase + (uint32_t)GLANE;
                LV(lk) = i < ncand ? P.clink[cb + i] : SEC_LINK_NIL;
                LV(ln) = i < ncand ? P.clen[cb + i] : 0u;
            }
        }
        const uint32_t link = GREADLANE(lk, k - wbase), len = GREADLANE(ln, k - wbase);
        if ((link >> 28) > dlog || sum + len > cap)
            break;
        ON_GLANE0
        {
            P.chain_k[cb + j] = k;
            P.chain_off[cb + j] = (uint32_t)sum;
        }
        sum += len;
        j++;
        const uint32_t nx = link & 0x0fffffffu;
        if (nx == SEC_LINK_FIN) {
            ok = 1;
            trailer = GUNI(P.cstop[cb + k]);
            break;
        }
        if (nx == SEC_LINK_NIL || nx <= k || nx >= ncand)
            break;
        k = nx;
    }
    ON_GLANE0
    {
        S->nchain = ok ? j : 0u;
        S->total = (uint32_t)sum;
        S->trailer = trailer;
    }
    WAVE_SYNC();
}

/* step 5: a group decodes chained sections into place until the queue is empty */
DEV void sec_write_worker(const IsecPlan &P, const uint8_t *src_all, uint8_t *dst_all, InfLds *lds, InfSecInfo *si)
{
    uint32_t s, j;
    while (sec_next_unit<2>(P, &s, &j)) {
        IsecStream *S = &P.st[s];
        const IsecItem *it = &P.items[s];
        const uint32_t cb = GUNI(S->base);
        const uint32_t k = GUNI(P.chain_k[cb + j]), off = GUNI(P.chain_off[cb + j]);
        const uint32_t start = GUNI(P.cstart[cb + k]), len = GUNI(P.clen[cb + k]);
        uint8_t *dst = dst_all + it->dst_off + off;
        InfJob job;
        job.src = src_all + it->src_off + start;
        job.n = GUNI(it->src_len) - start;
        job.dst = dst;
        job.cap = len;
        job.window_bits = k == 0u ? P.window_bits : -15;
        inflate_stream<INF_SEC_STOP | INF_SEC_NOTRAIL>(job, lds, nullptr, nullptr, si);
        const uint32_t outcome = GUNI(si->outcome);
        const int same = (outcome == INF_SEC_SYNC || outcome == INF_SEC_FINAL) && GUNI(si->out_len) == len &&
                         start + GUNI(si->stop) == GUNI(P.cstop[cb + k]);
        uint32_t ck = 0;
        if (P.window_bits >= 0) {
            SEC_FENCE();
            ck = (GUNI(S->head) & 1u) ? INF_CK(crc32_tx)<1>(dst, len, lds->cktab, INF_CKX(lds))
                                      : INF_CK(adler32)(dst, len);
        }
        ON_GLANE0
        {
            P.chain_ck[cb + j] = ck;
            if (!same)
                SEC_OR(&S->serial, 1u);
        }
        WAVE_SYNC();
    }
}

/* the check value of a stream's output from its chain's slices (chain_ck, clen): lane l combines the
 * slices of its share of the chain, then the lanes' results are combined in order */
DEV uint32_t sec_chain_check(const IsecPlan &P, uint32_t cb, uint32_t nchain, uint32_t gzip)
{
    const uint32_t per = (nchain + GRP - 1u) / GRP;
    LANEVAR(uint32_t, pc);
    LANEVAR(uint32_t, pl);
    FOR_GLANES
    {
        const uint32_t j0 = (uint32_t)GLANE * per;
        const uint32_t j1 = j0 + per < nchain ? j0 + per : nchain;
        uint32_t c = gzip ? 0u : 1u, l = 0;
        for (uint32_t j = j0; j < j1; j++) {
            const uint32_t len = P.clen[cb + P.chain_k[cb + j]], cj = P.chain_ck[cb + j];
            c = gzip ? sec_crc32_combine(c, cj, len) : sec_adler32_combine(c, cj, len);
            l += len;
        }
        LV(pc) = c;
        LV(pl) = l;
    }
    uint32_t want = gzip ? 0u : 1u;
    for (uint32_t l = 0; l < GRP; l++) {
        const uint32_t c = GREADLANE(pc, l), len = GREADLANE(pl, l);
        want = gzip ? sec_crc32_combine(want, c, len) : sec_adler32_combine(want, c, len);
    }
    return want;
}

/* step 6 for the a-th active stream: combine, check the trailer, finish */
DEV void sec_finish(const IsecPlan &P, const uint8_t *src_all, InfResult *res, InfResume *resume, uint32_t a)
{
    const uint32_t s = GUNI(P.active[a]);
    IsecStream *S = &P.st[s];
    const IsecItem *it = &P.items[s];
    const uint32_t nchain = GUNI(S->nchain);
    if (nchain == 0u || GUNI(S->serial))
        return;
    const uint32_t cb = GUNI(S->base);
    const uint8_t *src = src_all + it->src_off;
    const uint32_t n = GUNI(it->src_len), total = GUNI(S->total), t = GUNI(S->trailer);
    const uint32_t gzip = GUNI(S->head) & 1u;
    /* inflateReset2 (as inflate_stream) */
    int wrap = 0, wb = P.window_bits;
    if (wb >= 0)
        wrap = (wb >> 4) + 5;
    uint32_t consumed = t;
    if (wrap) {
        const uint32_t tl = gzip ? 8u : 4u;
        if (t > n || n - t < tl)
            return; /* truncated trailer: Z_BUF_ERROR, the serial decoder says so */
        const uint32_t v = inf_input_dword(src, t, n);
        if (wrap & 4) {
            const uint32_t want = sec_chain_check(P, cb, nchain, gzip);
            const uint32_t got = gzip ? v : ((v >> 24) | ((v >> 8) & 0xff00u) | ((v & 0xff00u) << 8) | (v << 24));
            if (got != want)
                return;
        }
        if (gzip && inf_input_dword(src, t + 4u, n) != total)
            return;
        consumed = t + tl;
    }
    ON_GLANE0
    {
        res[s].status = 0;
        res[s].out_len = total;
        res[s].consumed = consumed;
        res[s].pad = 0;
        resume[s].state = 2;
        P.nsec[s] = nchain;
    }
    WAVE_SYNC();
}

#undef SEC_GBCAST
/* back to whole-wave groups for whatever is compiled after this */
#undef ZSC_GROUP
#define ZSC_GROUP 64
#include "wave_group.h"

#endif
