/*
 * inflate_chunks.h -- kernel 7: any single stream inflated in parallel, in pieces that start at
 * block boundaries found by trial.
 *
 * The sections path (inflate_sections.h) needs full-flush markers; this one needs nothing of the
 * writer.  A chunks plan cuts each stream longer than chunk_bytes into chunks of chunk_bytes
 * compressed bytes.  The steps, each a launch of its own (zsc_hip_runtime.hip, chk_enqueue):
 *   1. setup    per stream: its state; candidate 0 of chunk 0 is the stream's start (with wrapper);
 *   2. scan     one wavefront per later chunk: the first INF_PC_CANDS candidate block starts at or
 *               after the chunk's start, as bit offsets, of two kinds -- the byte behind a stored
 *               block (byte-aligned LEN, ~LEN at p: p + 4 + LEN, which covers the byte behind a
 *               00 00 FF FF flush marker) and a dynamic-Huffman block header at any bit offset, one
 *               lane per offset, tested by inf_dyn_header_ok with the decoder's own rules;
 *   3. count    one group per chunk tries its candidates in order, decoding raw from the bit offset
 *               (candidate 0 of chunk 0 parses the wrapper), until one ends cleanly: at the first
 *               block boundary in a later chunk that is a candidate of that chunk, or at the final
 *               block.  The output is kept as 16-bit symbols in a ring of INF_WIN entries per
 *               chunk: a byte, or a placeholder for a byte of the unknown window before the piece.
 *               Recorded: length, link, the farthest reach before the start, the longest distance;
 *               the ring is the piece's tail;
 *   3b. retry   a clean piece of one chunk may end at a candidate of a later chunk other than the one
 *               that chunk's count took (a false candidate before it that happened to decode
 *               cleanly): each such chunk decodes the wanted candidate again, once;
 *   4. resolve  per stream: the chain from the header, following links, as inflate_sections.h, and
 *               checking that no piece reaches further back than the output before it or than the
 *               header's window;
 *   5. window   one workgroup per stream: the window each chained piece starts with, in chain
 *               order, each a 32 K-entry gather from the previous window and the previous tail;
 *   6. write    every chained piece decoded again into its place, references before its start
 *               read from its window (never from dst, so pieces do not race), with the Adler-32 /
 *               CRC-32 of its slice;
 *   7. finish   sec_finish of inflate_sections.h, unchanged: the slice checksums combined and
 *               compared with the trailer (and ISIZE).
 * Then k_inflate runs over the plan and decodes every stream the path did not finish.
 *
 * The safety rule is inflate_sections.h's: the path only ever reports a clean Z_OK.  Data errors,
 * Z_BUF_ERROR, truncation, Z_NEED_DICT, a bad trailer, a broken chain, a reach too far back, a
 * write pass that disagrees with the count pass, the work bound -- everything else goes to the
 * serial decoder from the stream's start, so status, bytes and consumed equal the plain plan's.
 *
 * Why decoding from a block start with placeholders is sound: where a block ends, and how the next
 * one is read, depends only on the bits and the codes of the block, never on the bytes of the
 * output, so a decode that starts at a true block boundary sees the same blocks, symbols, lengths
 * and distances as the reference's decode from the stream's start.  The bytes differ only where a
 * copy reaches before the piece's start; those become placeholders (count) or are read from the
 * window the pieces before produced (write).  The reference's only non-local check is the distance
 * limit: a distance may not reach before the whole output (nor beyond the zlib header's window),
 * and resolve applies exactly that with the piece's farthest reach and longest distance.  A piece
 * that starts at a false candidate is never chained: the chain runs from the stream's true start
 * through block boundaries the decoder itself reached, and a candidate is only entered where the
 * piece before ended at it.  A missed boundary (a fixed-Huffman block, a chunk whose candidates
 * all lie elsewhere) only makes a piece longer.
 */
#ifndef ZSC_INFLATE_CHUNKS_H
#define ZSC_INFLATE_CHUNKS_H

#include "inflate_sections.h"

/* compressed bytes per chunk when the caller passes 0 (the sweep), and the
 * least a plan takes */
#define CHK_DEFAULT_BYTES (128u * 1024u)
#define CHK_MIN_BYTES 4096u
/* the stored-block kind looks this far before a chunk for LEN, ~LEN whose block ends inside it */
#define CHK_STORED_BACK 65539u
#define CHK_USED_NONE 0xffffffffu

typedef struct {
    IsecPlan sp;       /* items (tile0 / ntiles: first chunk / chunks), st, active, q, nsec, clen, clink,
                        * cstop, chain_k, chain_off, chain_ck: as the sections path, for sec_finish */
    uint64_t *cand;    /* per chunk: INF_PC_CANDS bit offsets, ascending, INF_PC_NONE after the last */
    uint32_t *cused;   /* per chunk: the candidate the count pass ended cleanly from */
    uint32_t *creach;  /* per chunk: that piece's farthest reach before its start */
    uint32_t *want;    /* per chunk: a candidate a clean piece ended at, where the count pass took another */
    uint16_t *ring;    /* per chunk: INF_WIN symbols, the piece's tail */
    uint8_t *win;      /* per chunk: INF_WIN bytes, the window of a chained piece */
    uint32_t nactive;  /* streams with more than one chunk (P.sp.active) */
    uint32_t chunk_bytes;
    uint32_t keep_index; /* the write pass takes the slice check values of raw streams too (inflate_index.h) */
} IchkPlan;

/* ---- whole-wave code: setup and scan ---- */

/* step 1 for the a-th stream with chunks */
DEV void chk_setup(const IchkPlan &P, uint32_t a)
{
    const uint32_t s = GUNI(P.sp.active[a]);
    const IsecItem *it = &P.sp.items[s];
    ON_LANE0
    {
        IsecStream *S = &P.sp.st[s];
        S->work = 0;
        S->ncand = it->ntiles;
        S->take = S->take2 = 0;
        S->serial = 0;
        S->nchain = S->head = S->total = S->trailer = 0;
        S->base = it->tile0;
        S->pad = 0; /* (set by the scan when a later chunk has a candidate) */
        uint64_t *c = P.cand + (uint64_t)it->tile0 * INF_PC_CANDS;
        c[0] = 0;
        for (uint32_t j = 1; j < INF_PC_CANDS; j++)
            c[j] = INF_PC_NONE;
        if (a == 0)
            P.sp.q[0] = P.nactive;
    }
    const uint32_t c0 = GUNI(it->tile0), nch = GUNI(it->ntiles);
    FOR_LANES
    {
        for (uint32_t k = (uint32_t)LANE; k < nch; k += WAVE)
            P.want[c0 + k] = CHK_USED_NONE;
    }
}

/* step 3b, first half, for the a-th stream: the candidates clean pieces ended at that their chunk's
 * count did not take; the count queue starts over for the retry */
DEV void chk_want(const IchkPlan &P, uint32_t a)
{
    const uint32_t s = GUNI(P.sp.active[a]);
    IsecStream *S = &P.sp.st[s];
    const uint32_t cb = GUNI(S->base), nch = GUNI(S->ncand);
    FOR_LANES
    {
        for (uint32_t k = (uint32_t)LANE; k < nch; k += WAVE) {
            if (P.cused[cb + k] == CHK_USED_NONE)
                continue;
            const uint32_t nx = P.sp.clink[cb + k] & 0x0fffffffu, m = nx / INF_PC_CANDS;
            if (nx != SEC_LINK_FIN && nx != SEC_LINK_NIL && m > k && m < nch && P.cused[cb + m] != nx % INF_PC_CANDS)
                P.want[cb + m] = nx % INF_PC_CANDS; /* (two pieces that want different ones: either) */
        }
    }
    ON_LANE0
    {
        S->take = 0;
        if (a == 0)
            P.sp.q[1] = 0;
    }
}

/* nb (<= 16) bits of the stream from bit offset `bit`, zeros past its end */
DEV uint32_t chk_peek(const uint8_t *src, uint32_t n, uint64_t bit, uint32_t nb)
{
    const uint64_t by = bit >> 3;
    uint32_t v = 0;
    for (uint32_t j = 0; j < 3u; j++)
        if (by + j < n)
            v |= (uint32_t)src[by + j] << (8u * j);
    return (v >> (uint32_t)(bit & 7u)) & ((1u << nb) - 1u);
}

/* Is there a dynamic-Huffman block header at bit offset `bit` that inflate_stream accepts?  One lane's
 * scalar walk of the header: the decoder reads it with a lane group (ballot decoding, lengths in LDS),
 * which one lane per bit offset cannot do, so the walk is written twice, but every rule it applies is
 * the decoder's own routine from inflate.h: HLIT / HDIST in range (INF_HDR_COUNTS_BAD), the validity of
 * the code-length, literal/length and distance codes (inf_count_verdict), a repeat with no length
 * before it (INF_HDR_REP16_BAD), a repeat past HLIT + HDIST (INF_HDR_REP_OVERRUN), a zero length for
 * code 256 (INF_HDR_EOB_BAD); every bit of it inside the stream.  tests/test_inflate_chunks_emu.py
 * compares it with the decoder's verdict at every bit offset of several streams; a disagreement
 * would cost speed (a missed or a false candidate), never a wrong result.  (An empty code-length code is
 * rejected at once: the decoder reads only zero lengths with it and then fails at code 256.) */
DEV int inf_dyn_header_ok(const uint8_t *src, uint32_t n, uint64_t bit)
{
    const uint64_t end = (uint64_t)n * 8u;
    if (bit + 17u > end || (chk_peek(src, n, bit, 3) >> 1) != 2u)
        return 0;
    const uint32_t v = chk_peek(src, n, bit + 3u, 14);
    const uint32_t nlen = (v & 31u) + 257u, ndist = ((v >> 5) & 31u) + 1u, ncode = (v >> 10) + 4u;
    if (INF_HDR_COUNTS_BAD(nlen, ndist))
        return 0;
    uint64_t at = bit + 17u;
    if (at + 3u * ncode > end)
        return 0;
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint8_t cl[19];
    for (int i = 0; i < 19; i++)
        cl[i] = 0;
    for (uint32_t i = 0; i < ncode; i++)
        cl[order[i]] = (uint8_t)chk_peek(src, n, at + 3u * i, 3);
    at += 3u * ncode;
    uint16_t cnt[16];
    for (int l = 0; l < 16; l++)
        cnt[l] = 0;
    for (int i = 0; i < 19; i++)
        cnt[cl[i]]++;
    int max = 7;
    while (max >= 1 && cnt[max] == 0)
        max--;
    if (max == 0 || inf_count_verdict(cnt, max, 0))
        return 0;
    /* the code-length code's symbols by code (canonical order) */
    uint8_t sym[19];
    uint32_t offs[8];
    offs[1] = 0;
    for (int l = 1; l < 7; l++)
        offs[l + 1] = offs[l] + cnt[l];
    for (int i = 0; i < 19; i++)
        if (cl[i])
            sym[offs[cl[i]]++] = (uint8_t)i;
    uint16_t lc[16], dc[16];
    for (int l = 0; l < 16; l++)
        lc[l] = dc[l] = 0;
    const uint32_t total = nlen + ndist;
    uint32_t have = 0, prev = 0, l256 = 0;
    while (have < total) {
        /* one code, bit by bit, MSB first (the set is complete, so one of max bits matches) */
        uint32_t code = 0, first = 0, index = 0, s = 0xffu;
        for (int l = 1; l <= max; l++) {
            if (at >= end)
                return 0;
            code |= chk_peek(src, n, at++, 1);
            const uint32_t c = cnt[l];
            if (code - first < c) {
                s = sym[index + code - first];
                break;
            }
            index += c;
            first = (first + c) << 1;
            code <<= 1;
        }
        uint32_t len = s, rep = 1;
        if (s == 16u) {
            if (INF_HDR_REP16_BAD(have) || at + 2u > end)
                return 0;
            len = prev;
            rep = 3u + chk_peek(src, n, at, 2);
            at += 2u;
        } else if (s == 17u) {
            if (at + 3u > end)
                return 0;
            len = 0;
            rep = 3u + chk_peek(src, n, at, 3);
            at += 3u;
        } else if (s == 18u) {
            if (at + 7u > end)
                return 0;
            len = 0;
            rep = 11u + chk_peek(src, n, at, 7);
            at += 7u;
        }
        if (INF_HDR_REP_OVERRUN(have, rep, total))
            return 0;
        const uint32_t lit_end = have + rep < nlen ? have + rep : nlen;
        const uint32_t nl = lit_end > have ? lit_end - have : 0u;
        lc[len] = (uint16_t)(lc[len] + nl);
        dc[len] = (uint16_t)(dc[len] + (rep - nl));
        if (have <= 256u && 256u < have + rep)
            l256 = len;
        prev = len;
        have += rep;
    }
    if (INF_HDR_EOB_BAD(l256))
        return 0;
    int ml = 15, md = 15;
    while (ml >= 1 && lc[ml] == 0)
        ml--;
    while (md >= 1 && dc[md] == 0)
        md--;
    return inf_count_verdict(lc, ml, 1) == 0 && inf_count_verdict(dc, md, 2) == 0;
}

/* put candidate c into the sorted list (cl[0..INF_PC_CANDS), INF_PC_NONE-padded), dropping the largest */
DEV void chk_insert(uint64_t *cl, uint64_t c)
{
    for (uint32_t j = 0; j < INF_PC_CANDS; j++) {
        if (cl[j] == c)
            return;
        if (c < cl[j]) {
            for (uint32_t m = INF_PC_CANDS - 1u; m > j; m--)
                cl[m] = cl[m - 1u];
            cl[j] = c;
            return;
        }
    }
}

/* step 2 for scan entry t (stream, chunk): the first INF_PC_CANDS candidates in the chunk.  The
 * dynamic kind tests the chunk's bit offsets in ascending order, 64 per step, until it has
 * INF_PC_CANDS hits: at most 8 * chunk_bytes tests (most fail on the 3-bit block type or the
 * 14-bit counts; one in a few dozen reads a code-length code, and far fewer read code lengths).
 * The stored kind then reads the 4 bytes at every p from CHK_STORED_BACK before the chunk to its
 * end (or to the last candidate so far) and merges what it finds. */
DEV void chk_scan(const IchkPlan &P, const uint8_t *src_all, uint32_t t)
{
    const uint32_t s = GUNI(P.sp.tiles[t].stream), k = GUNI(P.sp.tiles[t].start);
    const IsecItem *it = &P.sp.items[s];
    const uint8_t *src = src_all + it->src_off;
    const uint32_t n = GUNI(it->src_len), cb = P.chunk_bytes;
    const uint64_t cs = (uint64_t)k * cb, ce = cs + cb < n ? cs + cb : n;
    uint64_t cl[INF_PC_CANDS];
    for (uint32_t j = 0; j < INF_PC_CANDS; j++)
        cl[j] = INF_PC_NONE;
    uint32_t found = 0;
    for (uint64_t b0 = cs * 8u; b0 < ce * 8u && found < INF_PC_CANDS; b0 += WAVE) {
        LANEVAR(int, hit);
        FOR_LANES
        {
            const uint64_t bit = b0 + (uint64_t)LANE;
            LV(hit) = bit < ce * 8u && inf_dyn_header_ok(src, n, bit);
        }
        uint64_t m = BALLOT(hit);
        while (m && found < INF_PC_CANDS) {
            cl[found++] = b0 + (uint64_t)CTZ64(m);
            m &= m - 1u;
        }
    }
    const uint64_t p0 = cs > CHK_STORED_BACK ? cs - CHK_STORED_BACK : 0u;
    for (uint64_t q0 = p0; q0 + 4u <= ce; q0 += WAVE) {
        if (found == INF_PC_CANDS && q0 * 8u >= cl[INF_PC_CANDS - 1u])
            break; /* (a stored block's end lies behind its LEN) */
        LANEVAR(uint32_t, c);
        LANEVAR(int, hit);
        FOR_LANES
        {
            const uint64_t p = q0 + (uint64_t)LANE;
            uint32_t w = 0;
            if (p + 4u <= n)
                w = (uint32_t)src[p] | (uint32_t)src[p + 1u] << 8 | (uint32_t)src[p + 2u] << 16 |
                    (uint32_t)src[p + 3u] << 24;
            const uint32_t len = w & 0xffffu;
            const uint64_t at = p + 4u + len;
            LV(c) = (uint32_t)(at - cs);
            LV(hit) = p + 4u <= n && len == ((w >> 16) ^ 0xffffu) && at >= cs && at < ce;
        }
        uint64_t m = BALLOT(hit);
        while (m) {
            const uint32_t l = (uint32_t)CTZ64(m);
            m &= m - 1u;
            chk_insert(cl, (cs + READLANE(c, l)) * 8u);
        }
        found = 0;
        while (found < INF_PC_CANDS && cl[found] != INF_PC_NONE)
            found++;
    }
    ON_LANE0
    {
        uint64_t *out = P.cand + ((uint64_t)it->tile0 + k) * INF_PC_CANDS;
        for (uint32_t j = 0; j < INF_PC_CANDS; j++)
            out[j] = cl[j];
        if (cl[0] != INF_PC_NONE)
            SEC_OR(&P.sp.st[s].pad, 1u);
    }
}

/* ---- group code (INF_GROUP lanes per unit, as the decoder) ---- */
#undef ZSC_GROUP
#define ZSC_GROUP INF_GROUP
#include "wave_group.h"

/* the piece context for chunk k's candidate at bit offset `bit` (SIZE: a size plan, inflate_size.h, which
 * has no rings) */
template <bool SIZE = false>
DEV void chk_piece(const IchkPlan &P, uint32_t cb, uint32_t k, uint32_t nchunks, uint64_t bit, InfPiece *pc,
                   const uint8_t *win)
{
    ON_GLANE0
    {
        pc->base_bit = bit & ~7ull;
        pc->chunk_bits = (uint64_t)P.chunk_bytes * 8u;
        pc->cand = P.cand + (uint64_t)cb * INF_PC_CANDS;
        if constexpr (SIZE)
            pc->ring = nullptr;
        else
        pc->ring = P.ring + (uint64_t)(cb + k) * INF_WIN;
        pc->win = win;
        pc->skip = (uint32_t)(bit & 7u);
        pc->chunk = k;
        pc->nchunks = nchunks;
    }
    WAVE_SYNC();
}

/* decode chunk k of stream s from candidate j0 on (only j0 if `single`) until one ends cleanly, and
 * record the outcome in the chunk's records (its ring holds the tail; SIZE: the piece is only counted,
 * and there is no ring) */
template <bool SIZE = false>
DEV void chk_count_chunk(const IchkPlan &P, const uint8_t *src_all, InfLds *lds, InfSecInfo *si, InfPiece *pc,
                         uint32_t s, uint32_t k, uint32_t j0, int single)
{
    IsecStream *S = &P.sp.st[s];
    const IsecItem *it = &P.sp.items[s];
    const uint32_t n = GUNI(it->src_len), cb = GUNI(S->base), nch = GUNI(S->ncand);
    uint32_t used = CHK_USED_NONE, link = SEC_LINK_NIL, len = 0, stop = 0, reach = 0;
    for (uint32_t j = j0; j < INF_PC_CANDS; j++) {
        if (GUNI(S->serial))
            break;
        if ((unsigned long long)SEC_LOAD(&S->work) > (unsigned long long)P.sp.work_mul * n + P.sp.work_add) {
            ON_GLANE0 { SEC_OR(&S->serial, 1u); }
            break;
        }
        const uint64_t bit = P.cand[(uint64_t)(cb + k) * INF_PC_CANDS + j];
        if (bit == INF_PC_NONE)
            break;
        const uint32_t start = (uint32_t)(bit >> 3);
        chk_piece<SIZE>(P, cb, k, nch, bit, pc, nullptr);
        InfJob job;
        job.src = src_all + it->src_off + start;
        job.n = n - start;
        job.dst = nullptr;
        job.cap = GUNI(it->dst_cap);
        job.window_bits = k == 0u ? P.sp.window_bits : -15;
        if constexpr (SIZE)
            inflate_stream<INF_SEC_BITSTART | INF_SEC_COUNT | INF_SEC_NOTRAIL>(job, lds, nullptr, nullptr, si, pc);
        else
        inflate_stream<INF_SEC_BITSTART | INF_SEC_SYM16 | INF_SEC_NOTRAIL>(job, lds, nullptr, nullptr, si, pc);
        const uint32_t outcome = GUNI(si->outcome);
        ON_GLANE0 { SEC_ADD(&S->work, (unsigned long long)GUNI(si->stop)); }
        if (outcome == INF_SEC_SYNC || outcome == INF_SEC_FINAL) {
            const uint32_t maxd = GUNI(si->maxd);
            const uint32_t dlog = maxd ? 32u - CLZ32(maxd - 1u) : 0u; /* ceil(log2) */
            used = j;
            link = (outcome == INF_SEC_SYNC ? GUNI(pc->link) : SEC_LINK_FIN) | dlog << 28;
            len = GUNI(si->out_len);
            stop = start + GUNI(si->stop);
            reach = GUNI(pc->reach);
            if (k == 0u) {
                ON_GLANE0 { S->head = si->gzip | (31u - CLZ32(si->dmax)) << 8; }
            }
            break;
        }
        if (k == 0u || single)
            break; /* (the stream's start is its only candidate) */
    }
    ON_GLANE0
    {
        P.cused[cb + k] = used;
        P.sp.clink[cb + k] = link;
        P.sp.clen[cb + k] = len;
        P.sp.cstop[cb + k] = stop;
        P.creach[cb + k] = reach;
    }
    WAVE_SYNC();
}

/* step 3: a group takes chunks until the queue is empty, and tries each one's candidates in order
 * (RETRY: only the wanted candidate of the chunks that have one).  A stream in whose later chunks the
 * scan found no candidate at all cannot be split: it goes to the serial decoder at once. */
template <bool RETRY = false, bool SIZE = false>
DEV void chk_count_worker(const IchkPlan &P, const uint8_t *src_all, InfLds *lds, InfSecInfo *si, InfPiece *pc)
{
    uint32_t s, k;
    while (sec_next_unit<1>(P.sp, &s, &k)) {
        IsecStream *S = &P.sp.st[s];
        if (!RETRY && GUNI(S->pad) == 0u) { /* (pad: the scan found a candidate) */
            ON_GLANE0 { SEC_OR(&S->serial, 1u); }
            continue;
        }
        const uint32_t wanted = RETRY ? GUNI(P.want[GUNI(S->base) + k]) : 0u;
        if (RETRY && wanted == CHK_USED_NONE)
            continue;
        chk_count_chunk<SIZE>(P, src_all, lds, si, pc, s, k, wanted, RETRY);
    }
}

/* step 4 for the a-th stream: the chain from the stream's start.  Where the chain enters a chunk at a
 * candidate that chunk's count (and retry) did not take -- a false candidate before it decoded cleanly
 * too -- the group decodes the entered candidate here and goes on, so no run of such chunks breaks the
 * chain.  A chain of one piece is left to the serial decoder: nothing runs in parallel, and the
 * write pass would decode it once more at the serial rate. */
template <bool SIZE = false>
DEV void chk_resolve(const IchkPlan &P, const uint8_t *src_all, InfLds *lds, InfSecInfo *si, InfPiece *pc, uint32_t a)
{
    const uint32_t s = GUNI(P.sp.active[a]);
    IsecStream *S = &P.sp.st[s];
    const IsecItem *it = &P.sp.items[s];
    if (GUNI(S->serial))
        return;
    const uint32_t cb = GUNI(S->base), nch = GUNI(S->ncand);
    const uint32_t dlog = (GUNI(S->head) >> 8) & 31u, cap = GUNI(it->dst_cap);
    uint32_t k = 0, j = 0, i = 0, ok = 0, trailer = 0;
    uint64_t sum = 0;
    for (;;) {
        if (GUNI(P.cused[cb + k]) != j)
            chk_count_chunk<SIZE>(P, src_all, lds, si, pc, s, k, j, 1);
        if (GUNI(P.cused[cb + k]) != j)
            break; /* (the entered candidate did not end cleanly, or the work bound was reached) */
        const uint32_t link = GUNI(P.sp.clink[cb + k]), len = GUNI(P.sp.clen[cb + k]);
        if ((link >> 28) > dlog || GUNI(P.creach[cb + k]) > sum || sum + len > cap)
            break;
        ON_GLANE0
        {
            P.sp.chain_k[cb + i] = k;
            P.sp.chain_off[cb + i] = (uint32_t)sum;
        }
        sum += len;
        i++;
        const uint32_t nx = link & 0x0fffffffu;
        if (nx == SEC_LINK_FIN) {
            ok = 1;
            trailer = GUNI(P.sp.cstop[cb + k]);
            break;
        }
        if (nx == SEC_LINK_NIL || nx / INF_PC_CANDS <= k || nx / INF_PC_CANDS >= nch)
            break;
        k = nx / INF_PC_CANDS;
        j = nx % INF_PC_CANDS;
    }
    ON_GLANE0
    {
        S->nchain = ok && i > 1u ? i : 0u;
        S->total = (uint32_t)sum;
        S->trailer = trailer;
    }
    WAVE_SYNC();
}

/* step 6: a group decodes chained pieces into place until the queue is empty */
DEV void chk_write_worker(const IchkPlan &P, const uint8_t *src_all, uint8_t *dst_all, InfLds *lds, InfSecInfo *si,
                          InfPiece *pc)
{
    uint32_t s, i;
    while (sec_next_unit<2>(P.sp, &s, &i)) {
        IsecStream *S = &P.sp.st[s];
        const IsecItem *it = &P.sp.items[s];
        const uint32_t cb = GUNI(S->base), nch = GUNI(S->ncand);
        const uint32_t k = GUNI(P.sp.chain_k[cb + i]), off = GUNI(P.sp.chain_off[cb + i]);
        const uint32_t len = GUNI(P.sp.clen[cb + k]);
        const uint64_t bit = P.cand[(uint64_t)(cb + k) * INF_PC_CANDS + GUNI(P.cused[cb + k])];
        const uint32_t start = (uint32_t)(bit >> 3);
        chk_piece(P, cb, k, nch, bit, pc, P.win + (uint64_t)(cb + k) * INF_WIN);
        uint8_t *dst = dst_all + it->dst_off + off;
        InfJob job;
        job.src = src_all + it->src_off + start;
        job.n = GUNI(it->src_len) - start;
        job.dst = dst;
        job.cap = len;
        job.window_bits = k == 0u ? P.sp.window_bits : -15;
        inflate_stream<INF_SEC_BITSTART | INF_SEC_EXTWIN | INF_SEC_NOTRAIL>(job, lds, nullptr, nullptr, si, pc);
        const uint32_t outcome = GUNI(si->outcome), link = GUNI(P.sp.clink[cb + k]) & 0x0fffffffu;
        const int same = GUNI(si->out_len) == len &&
                         ((outcome == INF_SEC_SYNC && GUNI(pc->link) == link) ||
                          (outcome == INF_SEC_FINAL && link == SEC_LINK_FIN &&
                           start + GUNI(si->stop) == GUNI(P.sp.cstop[cb + k])));
        uint32_t ck = 0;
        if (P.sp.window_bits >= 0 || P.keep_index) {
            SEC_FENCE();
            ck = (GUNI(S->head) & 1u) ? INF_CK(crc32_tx)<1>(dst, len, lds->cktab, INF_CKX(lds))
                                      : INF_CK(adler32)(dst, len);
        }
        ON_GLANE0
        {
            P.sp.chain_ck[cb + i] = ck;
            if (!same)
                SEC_OR(&S->serial, 1u);
        }
        WAVE_SYNC();
    }
}

/* back to whole-wave groups for whatever is compiled after this */
#undef ZSC_GROUP
#define ZSC_GROUP 64
#include "wave_group.h"

/* step 5 for one stream, by `nthr` threads (thread `tid` of them): the windows of its chain in order.
 * Window x of piece i + 1 is the byte INF_WIN - x before its start: the symbol of piece i's tail
 * that distance back, its placeholders resolved through piece i's window, or, where piece i is
 * shorter than that, piece i's window further back.  The first piece's window is zeros (its reach
 * is 0, so nothing reads it).  `barrier` orders the steps (a workgroup barrier on the GPU). */
template <class Barrier>
DEV void chk_windows(const IchkPlan &P, uint32_t s, uint32_t tid, uint32_t nthr, Barrier barrier)
{
    const IsecStream *S = &P.sp.st[s];
    const uint32_t nchain = S->nchain;
    if (nchain < 2u || S->serial)
        return;
    const uint32_t cb = S->base;
    uint8_t *w0 = P.win + (uint64_t)(cb + P.sp.chain_k[cb]) * INF_WIN;
    for (uint32_t x = tid; x < INF_WIN; x += nthr)
        w0[x] = 0;
    barrier();
    for (uint32_t i = 0; i + 1u < nchain; i++) {
        const uint32_t k = P.sp.chain_k[cb + i], len = P.sp.clen[cb + k];
        const uint8_t *w = P.win + (uint64_t)(cb + k) * INF_WIN;
        const uint16_t *tail = P.ring + (uint64_t)(cb + k) * INF_WIN;
        uint8_t *wn = P.win + (uint64_t)(cb + P.sp.chain_k[cb + i + 1u]) * INF_WIN;
        for (uint32_t x = tid; x < INF_WIN; x += nthr) {
            const uint32_t back = INF_WIN - x; /* 1 .. INF_WIN bytes before piece i + 1 */
            uint8_t b;
            if (back <= len) {
                const uint32_t v = tail[(len - back) & (INF_WIN - 1u)];
                b = (v & INF_PH) ? w[v & (INF_WIN - 1u)] : (uint8_t)v;
            } else {
                b = w[x + len];
            }
            wn[x] = b;
        }
        barrier();
    }
}

#endif
