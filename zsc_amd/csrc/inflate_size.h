/*
 * inflate_size.h -- kernel 10: the output length of compressed streams, without their output
 * (DESIGN.md section 14).
 *
 * Every inflate entry point needs dest_caps[i]; a size plan finds them.  It decodes each stream as
 * the plain plan does and stores nothing: no byte to dst, no match copy, no Adler-32 / CRC-32 of the
 * output.  Two parts:
 *
 *   size_stream   the whole stream, inflate_stream<INF_SEC_SIZE | INF_SEC_COUNT>: the wrapper, the
 *                 blocks, the trailer (ISIZE compared), results through InfResult / InfResume, a data
 *                 error re-entered through inflateSync by another launch, exactly as k_inflate.  What
 *                 the decoder checks without output bytes stays: header rules, code sets, invalid
 *                 symbols, a distance beyond the output so far or the header's window, truncation,
 *                 Z_NEED_DICT.  "Output full" is taken against job.cap, the caller's limit.
 *
 *   the chunked   for streams longer than chunk_bytes: the chunks plan's setup, scan, want / retry and
 *   path          resolve (inflate_chunks.h, unchanged) over a piece count variant,
 *                 inflate_stream<INF_SEC_BITSTART | INF_SEC_COUNT | INF_SEC_NOTRAIL>, which writes no
 *                 16-bit ring and reads no window: a length needs the blocks, lengths and distances of
 *                 a piece, never its bytes (inflate_chunks.h explains why those are the reference's).
 *                 Then size_finish per stream: the chain's sum (resolve has applied the limit and the
 *                 reach rules), the trailer's position, ISIZE.  No window and no write launch; scratch
 *                 per chunk is the candidates and records only.
 *
 * The safety rule is the chunks plan's: the chunked path only ever reports a clean Z_OK; a broken
 * chain, a reach before the output or beyond the header's window, the work bound, a total above the
 * limit, an ISIZE mismatch, a truncated trailer, any error -- the stream goes to size_stream from its
 * start, which runs over the plan last.
 *
 * The one difference from the plain plan (include/zsc_hip.h): the check value of a zlib / gzip trailer
 * is not compared, there being no bytes to take it over, so a stream whose only fault is its check
 * value is Z_OK with its full length.  Once a data error has been survived the salvaged output cannot
 * match the writer's check value (short of a stream built for it), and the check is taken as failed, as
 * the plain plan finds it: damaged streams give the plain plan's status, length, consumed and error
 * count.
 */
#ifndef ZSC_INFLATE_SIZE_H
#define ZSC_INFLATE_SIZE_H

#include "inflate_chunks.h"

/* ---- group code (INF_GROUP lanes per unit, as the decoder) ---- */
#undef ZSC_GROUP
#define ZSC_GROUP INF_GROUP
#include "wave_group.h"

/* one entry of the whole-stream size decode (inflate_stream's contract: 1 = enter once more) */
DEV int size_stream(const InfJob &job, InfLds *lds, InfResult *res, InfResume *rs)
{
    return inflate_stream<INF_SEC_SIZE | INF_SEC_COUNT>(job, lds, res, rs);
}

/* the same for one stream on the host emulation, entered again after every recovered data error */
DEV void size_with_resync(const InfJob &job, InfLds *lds, InfResult *res)
{
    InfResume rs;
    rs.state = 0;
    rs.out_pos = rs.errors = rs.gzip = rs.sy_lo = rs.sy_hi = rs.sy_rb = 0;
    for (uint32_t round = 0; round < job.n / 4u + 2u; round++) {
        if (!size_stream(job, lds, res, &rs))
            return;
    }
}

/* the chunked path's last step for the a-th stream with chunks: the chain resolve left (nchain pieces,
 * their lengths summed against the limit, the trailer's offset) becomes the stream's result if the
 * trailer is all there and, for gzip, ISIZE is the sum */
DEV void size_finish(const IchkPlan &P, const uint8_t *src_all, InfResult *res, InfResume *resume, uint32_t a)
{
    const uint32_t s = GUNI(P.sp.active[a]);
    IsecStream *S = &P.sp.st[s];
    const IsecItem *it = &P.sp.items[s];
    const uint32_t nchain = GUNI(S->nchain);
    if (nchain == 0u || GUNI(S->serial))
        return;
    const uint8_t *src = src_all + it->src_off;
    const uint32_t n = GUNI(it->src_len), total = GUNI(S->total), t = GUNI(S->trailer);
    const uint32_t gzip = GUNI(S->head) & 1u;
    uint32_t consumed = t;
    if (P.sp.window_bits >= 0) { /* (inflateReset2: every window_bits but the raw ones has a trailer) */
        const uint32_t tl = gzip ? 8u : 4u;
        if (t > n || n - t < tl)
            return; /* truncated trailer: Z_BUF_ERROR, the serial decode says so */
        if (gzip) {
            uint32_t isize = 0;
            for (uint32_t j = 0; j < 4u; j++)
                isize |= (uint32_t)GUNI(src[t + 4u + j]) << (8u * j);
            if (isize != total)
                return;
        }
        consumed = t + tl;
    }
    ON_GLANE0
    {
        res[s].status = 0;
        res[s].out_len = total;
        res[s].consumed = consumed;
        res[s].pad = 0;
        resume[s].state = 2;
        P.sp.nsec[s] = nchain;
    }
    WAVE_SYNC();
}

/* back to whole-wave groups for whatever is compiled after this */
#undef ZSC_GROUP
#define ZSC_GROUP 64
#include "wave_group.h"

#endif
