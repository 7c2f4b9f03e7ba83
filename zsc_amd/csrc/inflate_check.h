/*
 * inflate_check.h -- kernel 11: compressed streams checked on the device without their output
 * (DESIGN.md section 15).
 *
 * A size plan (inflate_size.h) cannot compare the check value of a zlib / gzip trailer: it makes no
 * bytes.  A check plan makes them and keeps only the last window: it decodes as the plain plan does,
 * stores into a byte ring of CHK_RING bytes owned by the lane group instead of into dst, and folds the
 * ring into the running Adler-32 / CRC-32 a quarter (CHK_FOLD bytes) at a time before the ring wraps
 * over it.  Status, length and consumed are the plain plan's for every input, with no exception, and
 * the check value computed is handed out (Adler-32 for zlib and raw streams, CRC-32 for gzip ones).
 *
 *   check_stream  the whole stream, inflate_stream<INF_SEC_RING>: SEC = 0 with every store to dst[x]
 *                 and every far read of dst[s] aimed at ring[x mod CHK_RING]; the 512-byte LDS stage
 *                 stays.  A data error leaves through InfResume as ever; the relaunch is the *size*
 *                 decode (size_stream), not this one: nothing behind an inflateSync can copy from
 *                 before it, and the check value of an output with a hole in it is taken as failed, as
 *                 the size path does and as the plain plan finds it.  So rings need not survive a launch.
 *
 *   the chunked   for streams longer than chunk_bytes: the chunks plan's setup, scan, count, want /
 *   path          retry, resolve and window unchanged (a check value needs the bytes, so the 16-bit
 *                 rings and the windows are needed), then chk_check_worker in place of the write pass:
 *                 inflate_stream<BITSTART | EXTWIN | NOTRAIL | RING> decodes each chained piece into a
 *                 byte ring -- the chunk's own symbol ring, dead once the windows are made, so there is
 *                 no scratch beyond a chunks plan's -- and leaves the piece's check value in chain_ck.
 *                 sec_finish, unchanged, combines and compares; check_finish copies the value out.
 *
 * The ring invariant.  The decoder folds quarter q (positions q CHK_FOLD .. (q + 1) CHK_FOLD - 1) as soon
 * as pos has passed its end and before it decodes on, so at every symbol pos - folded < CHK_FOLD.  A symbol
 * writes at most 258 positions, x < pos + 258, and position x lands on the slot of x - CHK_RING, which
 * is below folded + CHK_FOLD + 258 - CHK_RING <= folded: a quarter is overwritten no earlier than
 * CHK_RING - CHK_FOLD - 258 = 48 KiB - 258 bytes after it was completed, by when it is folded and, being
 * more than 32 768 back, out of every distance's reach.  CHK_RING is the smallest power of two that holds
 * a window and one copy.  The next stream a group takes reuses the ring; the decoder's own "distance
 * beyond the output so far" check keeps it from reading what the stream before left there.  The lane
 * emulation asserts all of it with a shadow of the ring (InfCheck::shadow).
 *
 * The safety rule is the chunks plan's: the chunked path only ever reports a clean Z_OK; everything
 * else -- a check-value mismatch, a broken chain, a limit passed, the work bound, any error -- goes to
 * check_stream from the stream's start.
 */
#ifndef ZSC_INFLATE_CHECK_H
#define ZSC_INFLATE_CHECK_H

#include "inflate_size.h"

#define CHK_RING 65536u /* bytes of a group's ring: a power of two >= INF_WIN + CHK_FOLD + 258 */
#define CHK_FOLD 16384u /* bytes folded into the check value at a time: divides CHK_RING, a multiple of 16 */
static_assert((CHK_RING & (CHK_RING - 1u)) == 0 && CHK_RING % CHK_FOLD == 0 && CHK_FOLD % 16u == 0 &&
                  CHK_RING >= INF_WIN + CHK_FOLD + 258u,
              "a quarter is folded before the ring wraps over it, and stays out of reach until then");
static_assert(CHK_RING <= 2u * INF_WIN, "a chunk's symbol ring serves as its byte ring");

#ifdef ZSC_WAVE_EMU
#include <stdio.h>
#include <stdlib.h>
#define CHK_SHADOW_FAIL(what, a, b)                                                                      \
    do {                                                                                                 \
        fprintf(stderr, "inflate_check: %s (%llu, %llu)\n", what, (unsigned long long)(a), (unsigned long long)(b)); \
        abort();                                                                                         \
    } while (0)
#endif

/* ---- group code (INF_GROUP lanes per unit, as the decoder) ---- */
#undef ZSC_GROUP
#define ZSC_GROUP INF_GROUP
#include "wave_group.h"

/* (DEV makes a free function; a member is inlined the same way) */
#ifdef ZSC_WAVE_EMU
#define CHK_MEM inline
#define CHK_MEM_OUT inline
#else
#define CHK_MEM __device__ __forceinline__
#define CHK_MEM_OUT __device__ __noinline__
#endif

/* the ring of one lane group and the running check value of the stream (or piece) it is decoding:
 * what inflate_stream<INF_SEC_RING> stores through.  Every member is group-uniform. */
struct InfCheck {
    uint8_t *ring;   /* in: CHK_RING bytes, 16-byte aligned */
    uint32_t gzip;   /* in: the stream is known to be a gzip one (a piece after the first does not see the header) */
    uint32_t value;  /* out: the check value of positions 0 .. folded - 1; of the whole output at the end */
    uint32_t folded; /* a multiple of CHK_FOLD until the tail is folded */
#ifdef ZSC_WAVE_EMU
    uint64_t *shadow; /* per slot: generation << 32 | the position last written (NULL: not kept) */
    uint64_t gen;     /* this decode's generation, never 0 */
#endif

    CHK_MEM void start(uint32_t gz)
    {
        gzip |= gz;
        value = gzip ? 0u : 1u;
        folded = 0;
#ifdef ZSC_WAVE_EMU
        static uint64_t generations = 0;
        gen = ++generations;
#endif
    }
    /* the stores and far reads of the decoder, which keeps the ring and the end of the last quarter folded
     * in registers (rg == ring, done == folded): nothing here reads a member on the GPU */
    CHK_MEM void put(uint8_t *rg, uint32_t done, uint32_t x, uint8_t b)
    {
#ifdef ZSC_WAVE_EMU
        if (rg != ring || done != folded)
            CHK_SHADOW_FAIL("the decoder's copy of the ring state is stale", done, folded);
        if (shadow) {
            const uint64_t old = shadow[x & (CHK_RING - 1u)];
            if ((old >> 32) == gen && (uint32_t)old >= folded)
                CHK_SHADOW_FAIL("a position not yet folded is overwritten", (uint32_t)old, x);
            shadow[x & (CHK_RING - 1u)] = gen << 32 | x;
        }
#endif
        rg[x & (CHK_RING - 1u)] = b;
    }
    CHK_MEM uint8_t get(const uint8_t *rg, uint32_t s) const
    {
#ifdef ZSC_WAVE_EMU
        if (shadow && shadow[s & (CHK_RING - 1u)] != (gen << 32 | s))
            CHK_SHADOW_FAIL("a slot read does not hold the position asked for", s, shadow[s & (CHK_RING - 1u)]);
#endif
        return rg[s & (CHK_RING - 1u)];
    }
    static CHK_MEM bool due(uint32_t pos, uint32_t done) { return pos - done >= CHK_FOLD; }

    /* positions folded .. folded + n - 1 (n <= CHK_FOLD, inside one quarter) into the value */
    CHK_MEM void fold_bytes(uint32_t n, InfLds *lds)
    {
        const uint8_t *q = ring + (folded & (CHK_RING - 1u));
#ifdef ZSC_WAVE_EMU
        for (uint32_t j = 0; shadow && j < n; j++)
            if (shadow[(folded + j) & (CHK_RING - 1u)] != (gen << 32 | (folded + j)))
                CHK_SHADOW_FAIL("a slot folded does not hold its position", folded + j, shadow[(folded + j) & (CHK_RING - 1u)]);
#else
        __threadfence_block();
#endif
        if (gzip)
            value = sec_crc32_combine(value, INF_CK(crc32_tx)<1>(q, n, lds->cktab, INF_CKX(lds)), n);
        else
            value = sec_adler32_combine(value, INF_CK(adler32)(q, n), n);
        folded += n;
    }
    /* the CRC routine's exchange area lies in the stage (inflate.h): put back the bytes it stood on */
    CHK_MEM void restage(uint32_t pos, InfLds *lds)
    {
        if (!gzip)
            return;
        const uint32_t from = pos > INF_STAGE ? pos - INF_STAGE : 0u;
        FOR_GLANES
        {
            for (uint32_t p = from + (uint32_t)GLANE; p < pos; p += GRP)
                lds->stage[p & (INF_STAGE - 1)] = get(ring, p);
        }
        WAVE_SYNC();
    }
    /* every quarter pos has passed (one, as the decoder calls it), and at the end of the output (tail) the
     * last, partial one.  Returns folded.  Kept out of line, and called from outside the symbol loop only
     * (the loop leaves through its one exit for it): it is reached once in CHK_FOLD bytes, and a call inside
     * the loop had the decoder's code tables spilled around it and reloaded at every match (DESIGN.md
     * section 15). */
    CHK_MEM_OUT uint32_t fold(uint32_t pos, InfLds *lds, bool tail = false)
    {
        while (pos - folded >= CHK_FOLD)
            fold_bytes(CHK_FOLD, lds);
        if (tail) {
            if (pos != folded)
                fold_bytes(pos - folded, lds);
        } else
            restage(pos, lds);
        return folded;
    }
    CHK_MEM void fold_tail(uint32_t pos, InfLds *lds) { (void)fold(pos, lds, true); }
};

/* one entry of the whole-stream ring decode (inflate_stream's contract: 1 = a data error, to be entered
 * once more -- by size_stream).  *value: the check value of the output when the stream is Z_OK. */
DEV int check_stream(const InfJob &job, InfLds *lds, InfResult *res, InfResume *rs, InfCheck *ck, uint32_t *value)
{
    ck->gzip = 0;
    ck->value = 0;
    const int again = inflate_stream<INF_SEC_RING>(job, lds, res, rs, nullptr, nullptr, ck);
    const uint32_t v = ck->value;
    ON_GLANE0 { *value = v; }
    return again;
}

/* the same for one stream on the host emulation: the ring decode, then the size decode after every
 * recovered data error, as the runtime relaunches */
DEV void check_with_resync(const InfJob &job, InfLds *lds, InfResult *res, InfResume *rs, InfCheck *ck, uint32_t *value)
{
    rs->state = 0;
    rs->out_pos = rs->errors = rs->gzip = rs->sy_lo = rs->sy_hi = rs->sy_rb = 0;
    if (!check_stream(job, lds, res, rs, ck, value))
        return;
    for (uint32_t round = 0; round < job.n / 4u + 2u; round++) {
        if (!size_stream(job, lds, res, rs))
            return;
    }
}

/* the chunked path's write pass: a group decodes chained pieces until the queue is empty, each into the
 * byte ring its chunk's symbol ring has become, and leaves the piece's check value in chain_ck (raw
 * streams included).  chk_write_worker with nothing written: the same comparison with the count pass. */
DEV void chk_check_worker(const IchkPlan &P, const uint8_t *src_all, InfLds *lds, InfSecInfo *si, InfPiece *pc
#ifdef ZSC_WAVE_EMU
                          ,
                          uint64_t *shadow = nullptr
#endif
)
{
    uint32_t s, i;
    while (sec_next_unit<2>(P.sp, &s, &i)) {
        IsecStream *S = &P.sp.st[s];
        const IsecItem *it = &P.sp.items[s];
        const uint32_t cb = GUNI(S->base), nch = GUNI(S->ncand);
        const uint32_t k = GUNI(P.sp.chain_k[cb + i]);
        const uint32_t len = GUNI(P.sp.clen[cb + k]);
        const uint64_t bit = P.cand[(uint64_t)(cb + k) * INF_PC_CANDS + GUNI(P.cused[cb + k])];
        const uint32_t start = (uint32_t)(bit >> 3);
        chk_piece(P, cb, k, nch, bit, pc, P.win + (uint64_t)(cb + k) * INF_WIN);
        InfCheck ck;
        ck.ring = (uint8_t *)(P.ring + (uint64_t)(cb + k) * INF_WIN);
        ck.gzip = GUNI(S->head) & 1u;
        ck.value = 0;
#ifdef ZSC_WAVE_EMU
        ck.shadow = shadow;
#endif
        InfJob job;
        job.src = src_all + it->src_off + start;
        job.n = GUNI(it->src_len) - start;
        job.dst = nullptr;
        job.cap = len;
        job.window_bits = k == 0u ? P.sp.window_bits : -15;
        inflate_stream<INF_SEC_BITSTART | INF_SEC_EXTWIN | INF_SEC_NOTRAIL | INF_SEC_RING>(job, lds, nullptr, nullptr, si,
                                                                                          pc, &ck);
        const uint32_t outcome = GUNI(si->outcome), link = GUNI(P.sp.clink[cb + k]) & 0x0fffffffu;
        const int same = GUNI(si->out_len) == len &&
                         ((outcome == INF_SEC_SYNC && GUNI(pc->link) == link) ||
                          (outcome == INF_SEC_FINAL && link == SEC_LINK_FIN &&
                           start + GUNI(si->stop) == GUNI(P.sp.cstop[cb + k])));
        const uint32_t v = ck.value;
        ON_GLANE0
        {
            P.sp.chain_ck[cb + i] = v;
            if (!same)
                SEC_OR(&S->serial, 1u);
        }
        WAVE_SYNC();
    }
}

/* the chunked path's last step for the a-th stream with chunks, after sec_finish: the combined check
 * value of a stream it finished, for zsc_hip_inflate_plan_check_values */
DEV void check_finish(const IchkPlan &P, const InfResume *resume, uint32_t *values, uint32_t a)
{
    const uint32_t s = GUNI(P.sp.active[a]);
    const IsecStream *S = &P.sp.st[s];
    const uint32_t nchain = GUNI(S->nchain);
    if (nchain == 0u || GUNI(S->serial) || GUNI(resume[s].state) != 2u)
        return;
    const uint32_t v = sec_chain_check(P.sp, GUNI(S->base), nchain, GUNI(S->head) & 1u);
    ON_GLANE0 { values[s] = v; }
    WAVE_SYNC();
}

/* back to whole-wave groups for whatever is compiled after this */
#undef ZSC_GROUP
#define ZSC_GROUP 64
#include "wave_group.h"

#endif
