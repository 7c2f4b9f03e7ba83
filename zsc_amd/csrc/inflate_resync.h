/*
 * inflate_resync.h -- kernel 8: damaged full-flush streams inflated in parallel, with the
 * reference's resynchronisation.
 *
 * zsc_uncompress answers a data error with inflateSync (src/zsc_uncompr.c:104-125): the next
 * 00 00 FF FF -- first in what the bit buffer still holds, then in the input -- and decoding goes on
 * behind it as a raw stream with an empty window.  The sections path (inflate_sections.h) gives up at
 * the first data error; a resync plan follows the reference past it.  It is a sections plan whose
 * count, resolve, write and finish steps are these (scan and setup are the sections path's):
 *   3. count    every candidate decoded as sec_count_worker does (INF_SEC_ERRSTATE added): also, at a
 *               data error in the blocks, what the reference's bit buffer held (stream-absolute
 *               sy_start, sy_rb) and whether it was a distance beyond the section's own output;
 *   4. resolve  per stream, one group: the chain from candidate 0.  A section that ends at a marker
 *               links on; one that ends in a data error is a chain entry with its partial output,
 *               then inflateSync's search runs from its error state -- the bytes of the bit buffer
 *               as inf_sync_search sees them, then the first candidate whose pattern starts at or
 *               after nin (the loaded links, else a binary search over cstart) -- and the chain
 *               resumes at the candidate it lands on; no pattern: Z_DATA_ERROR, all input consumed;
 *   5. write    every chain entry decoded into place as sec_write_worker does; an entry that ends in a
 *               data error is decoded with cap = its length, so the write may stop at "output full"
 *               instead of at the error (the count pass's record of the error is authoritative);
 *   6. finish   per stream: the slices' check values combined and compared with the trailer, ISIZE
 *               against the output since the last resume; a failing trailer is one more data error,
 *               searched from the trailer's error state; status, out_len, consumed, and the error
 *               count in InfResume.errors (the reference's data_errors).
 * Then k_inflate decodes every stream the path did not finish, from its start.
 *
 * Why the chain equals the reference: a candidate is decoded from an empty bit buffer at the byte
 * behind a pattern, raw, with dmax 32768 and nothing to copy from before it -- exactly the state
 * inflateSync leaves (mode TYPE, inflateReset).  A section entered at a marker is decoded as in the
 * sections path, whose soundness argument holds between two resumes.  Everything the local decode
 * cannot see is left to the serial decoder: an error in the header, Z_NEED_DICT, truncation, a data
 * error where the output has reached dest_cap, a landing point the count pass did not decode, a chain that does not
 * advance, a distance beyond a section entered at a marker (it may lie in the output before it), the
 * header's dmax exceeded before the first resume, the work bound, the pool or candidate limit, a
 * write pass that disagrees, a pattern inside or behind a failing trailer, and an error count that
 * would reach the reference's loop limit, max(dest_len, 10) inflate() calls.
 */
#ifndef ZSC_INFLATE_RESYNC_H
#define ZSC_INFLATE_RESYNC_H

#include "inflate_sections.h"

/* a candidate's error record: sy_start << 8 | RSY_BAD | RSY_HIST | sy_rb (0 when it ended without a
 * data error in the blocks) */
#define RSY_RB_MASK 63ull
#define RSY_BAD 64ull  /* a data error in the blocks */
#define RSY_HIST 128ull /* ... a distance beyond the section's own output */
#define RSY_SY_SHIFT 8u
/* chain entry flags */
#define RSY_FL_ERROR 1u   /* the entry ends in a data error (its output is partial) */
#define RSY_FL_RESUMED 2u /* it starts where a resynchronisation landed */
/* how a resolved chain ends (0: it does not; the stream goes serial) */
#define RSY_END_FINAL 1u /* at the final block: finish checks the trailer */
#define RSY_END_LOST 2u  /* at a data error with no pattern behind it: Z_DATA_ERROR, all input consumed */
#define RSY_NONE 0xffffffffu
#define RSY_PATTERN 0xffff0000u /* 00 00 FF FF as a little-endian dword */

/* per stream, written by resolve */
typedef struct {
    uint32_t errors; /* data errors of the chain (the reference's data_errors) */
    uint32_t base;   /* output offset of the last resume: the gzip ISIZE counts from here */
    uint32_t end;    /* RSY_END_* */
    uint32_t pad;
} IrsyStream;

typedef struct {
    IsecPlan sp;        /* a sections plan's: scan, setup, the candidate records and the chain */
    uint64_t *cerr;     /* per candidate (pool slot): its error record */
    uint32_t *chain_fl; /* per chain entry (pool slot): RSY_FL_* */
    IrsyStream *rst;    /* per stream */
} IrsyPlan;

/* ---- group code (INF_GROUP lanes per unit, as the decoder) ---- */
#undef ZSC_GROUP
#define ZSC_GROUP INF_GROUP
#include "wave_group.h"

/* inflateSync's search in the bytes of the reference's bit buffer, as inf_sync_search: sy_rb bits of
 * the stream from bit sy_start, after "hold <<= bits & 7", with the input from nin behind them.  The
 * landing point (input offset behind a pattern that starts in the buffer), or RSY_NONE; a pattern
 * that starts in the input is the caller's to find. */
DEV uint32_t rsy_hold_search(const uint8_t *src, uint32_t n, uint64_t sy_start, uint32_t sy_rb, uint32_t nin)
{
    const uint32_t hold = inf_sync_hold(src, n, sy_start, sy_rb);
    const uint32_t nh = sy_rb >> 3;
    for (uint32_t m = 0; m < nh; m++) {
        int ok = 1;
        for (uint32_t j = 0; j < 4u && ok; j++) {
            const uint32_t i = m + j;
            uint32_t c = 0x100u;
            if (i < nh)
                c = (hold >> (8u * i)) & 0xffu;
            else if (nin + (i - nh) < n)
                c = GUNI(src[nin + (i - nh)]);
            ok = c == (j < 2u ? 0u : 0xffu);
        }
        if (ok)
            return nin + (m + 4u > nh ? m + 4u - nh : 0u);
    }
    return RSY_NONE;
}

/* the one pattern the scan does not list: the input's last four bytes, when they start at or after nin */
DEV int rsy_tail_pattern(const uint8_t *src, uint32_t n, uint32_t nin)
{
    return n >= 4u && n - 4u >= nin && inf_input_dword(src, n - 4u, n) == RSY_PATTERN;
}

/* step 3: a group decodes candidates until the queue is empty (sec_count_worker, plus the error record) */
DEV void rsy_count_worker(const IrsyPlan &R, const uint8_t *src_all, InfLds *lds, InfSecErr *si)
{
    const IsecPlan &P = R.sp;
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
        inflate_stream<INF_SEC_STOP | INF_SEC_COUNT | INF_SEC_NOTRAIL | INF_SEC_ERRSTATE>(job, lds, nullptr, nullptr, si);
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
            uint64_t e = 0;
            if (si->err == INF_SEC_ERR_BODY)
                e = (8ull * start + si->sy_start) << RSY_SY_SHIFT | RSY_BAD |
                    (outcome == INF_SEC_HISTORY ? RSY_HIST : 0ull) | si->sy_rb;
            R.cerr[cb + k] = e;
            if (k == 0u)
                S->head = si->gzip | (31u - CLZ32(si->dmax)) << 8;
            SEC_ADD(&S->work, (unsigned long long)(stop - start));
        }
        WAVE_SYNC();
    }
}

/* step 4 for the a-th active stream: the chain from candidate 0 through markers and resumes, GRP
 * candidates' records read at a time */
DEV void rsy_resolve(const IrsyPlan &R, const uint8_t *src_all, uint32_t a)
{
    const IsecPlan &P = R.sp;
    const uint32_t s = GUNI(P.active[a]);
    IsecStream *S = &P.st[s];
    const IsecItem *it = &P.items[s];
    const uint32_t ncand = GUNI(S->ncand);
    if (ncand == 0u || GUNI(S->serial))
        return;
    const uint32_t cb = GUNI(S->base);
    const uint8_t *src = src_all + it->src_off;
    const uint32_t n = GUNI(it->src_len);
    const uint32_t dlog = (GUNI(S->head) >> 8) & 31u, cap = GUNI(it->dst_cap);
    const uint32_t limit = cap > 10u ? cap : 10u; /* the reference's loop_limit */
    LANEVAR(uint32_t, lk);
    LANEVAR(uint32_t, ln);
    LANEVAR(uint32_t, lc);
    LANEVAR(uint32_t, lel);
    LANEVAR(uint32_t, leh);
    uint32_t k = 0, wbase = 0, j = 0, end = 0, trailer = 0, errors = 0, base = 0, fl = 0, resumed = 0;
    uint64_t sum = 0;
    int loaded = 0;
    for (;;) {
        if (!loaded || k - wbase >= GRP) {
            wbase = k;
            loaded = 1;
            FOR_GLANES
            {
                const uint32_t i = wbase + (uint32_t)GLANE;
                const uint64_t e = i < ncand ? R.cerr[cb + i] : 0ull;
                LV(lk) = i < ncand ? P.clink[cb + i] : SEC_LINK_NIL;
                LV(ln) = i < ncand ? P.clen[cb + i] : 0u;
                LV(lc) = i < ncand ? P.cstart[cb + i] : 0xffffffffu;
                LV(lel) = (uint32_t)e;
                LV(leh) = (uint32_t)(e >> 32);
            }
        }
        const uint32_t l = k - wbase;
        const uint32_t link = GREADLANE(lk, l), len = GREADLANE(ln, l);
        const uint64_t e = (uint64_t)GREADLANE(leh, l) << 32 | GREADLANE(lel, l);
        const uint32_t nx = link & 0x0fffffffu;
        if (!resumed && (link >> 28) > dlog)
            break; /* beyond the header's window before the first resume: the error lies elsewhere */
        if (!(e & RSY_BAD)) {
            /* ended at a marker or at the final block (output that fills dest_cap exactly is sound here:
             * the reference only tests for a full output where a literal or a copy is to be written,
             * and the section wrote all of its own); anything else is the serial decoder's */
            if (sum + len > cap || nx == SEC_LINK_NIL || (nx != SEC_LINK_FIN && (nx <= k || nx >= ncand)))
                break;
            ON_GLANE0
            {
                P.chain_k[cb + j] = k;
                P.chain_off[cb + j] = (uint32_t)sum;
                R.chain_fl[cb + j] = fl;
            }
            sum += len;
            j++;
            if (nx == SEC_LINK_FIN) {
                end = RSY_END_FINAL;
                trailer = GUNI(P.cstop[cb + k]);
                break;
            }
            k = nx;
            fl = 0;
            continue;
        }
        /* a data error: a distance beyond the output is one only where the window is the section's own */
        if ((e & RSY_HIST) && !(k == 0u || (fl & RSY_FL_RESUMED)))
            break;
        if (sum + len >= cap || errors + 2u >= limit)
            break;
        ON_GLANE0
        {
            P.chain_k[cb + j] = k;
            P.chain_off[cb + j] = (uint32_t)sum;
            R.chain_fl[cb + j] = fl | RSY_FL_ERROR;
        }
        sum += len;
        j++;
        errors++;
        /* inflateSync */
        const uint64_t sy = e >> RSY_SY_SHIFT;
        const uint32_t rb = (uint32_t)(e & RSY_RB_MASK);
        const uint32_t nin = (uint32_t)((sy + rb) >> 3);
        if (nin >= n && rb < 8u)
            break; /* Z_BUF_ERROR (:1562-1565) */
        uint32_t nk = SEC_LINK_NIL;
        const uint32_t land = rsy_hold_search(src, n, sy, rb, nin);
        if (land != RSY_NONE) {
            nk = sec_find(P.cstart + cb, ncand, land);
        } else {
            /* the first candidate behind a pattern at or after nin: among the loaded ones, else by
             * binary search over the rest (candidates up to k start at or before nin) */
            LANEVAR(int, hit);
            FOR_GLANES
            {
                const uint32_t i = wbase + (uint32_t)GLANE;
                LV(hit) = i > k && i < ncand && LV(lc) >= nin + 4u;
            }
            const uint64_t hm = GBALLOT(hit);
            if (hm != 0) {
                nk = wbase + (uint32_t)CTZ64(hm);
            } else {
                uint32_t lo = wbase + GRP > k + 1u ? wbase + GRP : k + 1u, hi = ncand;
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (GUNI(P.cstart[cb + mid]) < nin + 4u)
                        lo = mid + 1u;
                    else
                        hi = mid;
                }
                nk = lo;
            }
            if (nk >= ncand) {
                if (!rsy_tail_pattern(src, n, nin)) /* (a pattern that ends the input lands at its end: serial) */
                    end = RSY_END_LOST;
                break;
            }
        }
        if (nk == SEC_LINK_NIL || nk <= k)
            break;
        k = nk;
        fl = RSY_FL_RESUMED;
        resumed = 1;
        base = (uint32_t)sum;
    }
    ON_GLANE0
    {
        S->nchain = end ? j : 0u;
        S->total = (uint32_t)sum;
        S->trailer = trailer;
        R.rst[s].errors = errors;
        R.rst[s].base = base;
        R.rst[s].end = end;
        R.rst[s].pad = 0;
    }
    WAVE_SYNC();
}

/* step 5: a group decodes chain entries into place until the queue is empty */
DEV void rsy_write_worker(const IrsyPlan &R, const uint8_t *src_all, uint8_t *dst_all, InfLds *lds, InfSecInfo *si)
{
    const IsecPlan &P = R.sp;
    uint32_t s, j;
    while (sec_next_unit<2>(P, &s, &j)) {
        IsecStream *S = &P.st[s];
        const IsecItem *it = &P.items[s];
        const uint32_t cb = GUNI(S->base);
        const uint32_t k = GUNI(P.chain_k[cb + j]), off = GUNI(P.chain_off[cb + j]);
        const uint32_t fl = GUNI(R.chain_fl[cb + j]);
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
        const int same = GUNI(si->out_len) == len &&
                         ((fl & RSY_FL_ERROR) ? outcome == INF_SEC_ERROR || outcome == INF_SEC_HISTORY
                                              : (outcome == INF_SEC_SYNC || outcome == INF_SEC_FINAL) &&
                                                    start + GUNI(si->stop) == GUNI(P.cstop[cb + k]));
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

/* step 6 for the a-th active stream: the trailer, the results */
DEV void rsy_finish(const IrsyPlan &R, const uint8_t *src_all, InfResult *res, InfResume *resume, uint32_t a)
{
    const IsecPlan &P = R.sp;
    const uint32_t s = GUNI(P.active[a]);
    IsecStream *S = &P.st[s];
    const IsecItem *it = &P.items[s];
    const uint32_t nchain = GUNI(S->nchain);
    if (nchain == 0u || GUNI(S->serial))
        return;
    const uint32_t cb = GUNI(S->base), ncand = GUNI(S->ncand);
    const uint8_t *src = src_all + it->src_off;
    const uint32_t n = GUNI(it->src_len), total = GUNI(S->total), t = GUNI(S->trailer);
    const uint32_t gzip = GUNI(S->head) & 1u, cap = GUNI(it->dst_cap);
    uint32_t errors = GUNI(R.rst[s].errors), consumed = n;
    if (GUNI(R.rst[s].end) == RSY_END_FINAL) {
        /* inflateReset2 (as inflate_stream) */
        int wrap = 0, wb = P.window_bits;
        if (wb >= 0)
            wrap = (wb >> 4) + 5;
        consumed = t;
        if (wrap) {
            const uint32_t tl = gzip ? 8u : 4u;
            if (t > n || n - t < tl)
                return; /* truncated trailer: Z_BUF_ERROR, the serial decoder says so */
            uint64_t sy = ~0ull; /* the error state of a failing trailer: 32 bits in hold, :1333-1351 */
            if (wrap & 4) {
                const uint32_t v = inf_input_dword(src, t, n);
                const uint32_t got = gzip ? v : ((v >> 24) | ((v >> 8) & 0xff00u) | ((v & 0xff00u) << 8) | (v << 24));
                if (got != sec_chain_check(P, cb, nchain, gzip))
                    sy = 8ull * t;
            }
            if (sy == ~0ull && gzip && inf_input_dword(src, t + 4u, n) != total - GUNI(R.rst[s].base))
                sy = 8ull * (t + 4u);
            if (sy == ~0ull) {
                consumed = t + tl;
            } else {
                /* one more data error; a pattern in the trailer or behind it resumes decoding there, which
                 * is the serial decoder's work */
                errors++;
                const uint32_t nin = (uint32_t)((sy + 32u) >> 3);
                const uint32_t limit = cap > 10u ? cap : 10u;
                if (errors + 1u >= limit || rsy_hold_search(src, n, sy, 32u, nin) != RSY_NONE ||
                    GUNI(P.cstart[cb + ncand - 1u]) >= nin + 4u || rsy_tail_pattern(src, n, nin))
                    return;
                consumed = n; /* the search used up all the input (:1585-1593) */
            }
        }
    }
    ON_GLANE0
    {
        res[s].status = errors ? INF_DATA : 0;
        res[s].out_len = total;
        res[s].consumed = consumed;
        res[s].pad = 0;
        resume[s].state = 2;
        resume[s].errors = errors;
        P.nsec[s] = nchain;
    }
    WAVE_SYNC();
}

/* back to whole-wave groups for whatever is compiled after this */
#undef ZSC_GROUP
#define ZSC_GROUP 64
#include "wave_group.h"

#endif
