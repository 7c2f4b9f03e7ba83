/*
 * deflate_index.h -- kernels 4c-4e: the seek-point index of a stream, written while it is compressed
 * (DESIGN.md section 11).
 *
 * An indexed inflate plan (inflate_index.h) decodes a stream in pieces from a blob of seek points.  A
 * chunks inflate plan finds those points by trial; the compressor knows them: ZdBlockPlan.bit_off is
 * where every block starts, ZdBlockRec.in_begin / in_len are the input bytes it covers, the symbols
 * hold every distance the parser chose, and the window before a piece is the input before it.  With
 * the index enabled, a deflate plan runs three more launches per sub-batch, after layout and emit and
 * before the next sub-batch reuses the block records, plans and symbols:
 *   reach   (dix_block_reach, one wave per block) how far the block's matches read before the block's
 *           own first byte: R_b = max(dist - rel_pos) over its symbols with dist > rel_pos, rel_pos the
 *           symbol's position relative to in_begin (a wave prefix sum of the symbol lengths); 0 for a
 *           stored block, whatever the parser's symbols say -- the decoder copies bytes there;
 *   points  (dix_points, one thread per buffer) point 0 is the stream's start; a later block opens a
 *           point if it holds input and starts in a later chunk of 8 * chunk_bytes bits than the point
 *           before it, so every chunk holds at most one point.  A piece is the blocks from its point to
 *           the next; its window length is max over its blocks of R_b - (in_begin_b - off), floored at
 *           0: exactly what the decoder's pc->reach will say, which is what an indexed plan demands;
 *   check   (dix_piece_check, one wave per piece) CRC-32 (gzip) or Adler-32 (zlib, raw) of the piece's
 *           input bytes, with the routines of checksum.h.
 * The records (ZidxRec, inflate_index.h) go to storage the plan owns; the windows are not stored: the
 * export gathers them from the device input (dix_gather).
 *
 * Whole-wave code on wave.h, compiled a second time by tests/emu_dindex.
 */
#ifndef ZSC_DEFLATE_INDEX_H
#define ZSC_DEFLATE_INDEX_H

#include "checksum.h"
#include "inflate_index.h"
#include "wave.h"
#include "zsc_dev.h"

#ifdef ZSC_WAVE_EMU
#include <assert.h>
#define DIX_ASSERT(x) assert(x)
#else
#define DIX_ASSERT(x) ((void)0)
#endif

#define DIX_DEFAULT_CHUNK (128u * 1024u) /* the chunks inflate plans' default (inflate_chunks.h) */

/* chunk_bytes as zsc_hip_deflate_plan_index_enable takes it */
static inline uint32_t dix_chunk_bytes(uint32_t chunk_bytes)
{
    if (chunk_bytes == 0u)
        chunk_bytes = DIX_DEFAULT_CHUNK;
    return chunk_bytes < ZIDX_MIN_CHUNK ? ZIDX_MIN_CHUNK : chunk_bytes;
}

/* The header of the blob of a stream of out_len bytes made from in_len bytes by a plan with this wrapper
 * (0 raw, 1 zlib, 2 gzip) and window size.  window_bits is what an inflate plan must be given for the
 * wrapper; head is what its decoder reports for the stream's header (inflate.h: gzip | log2(distance
 * limit) << 8 -- only a zlib header names a limit below 32 KiB). */
static inline ZidxInfo dix_blob_info(uint32_t wrap, int wbits, uint32_t chunk_bytes, uint32_t out_len, uint32_t in_len,
                                     uint32_t npoints)
{
    ZidxInfo h;
    h.window_bits = wrap == 0u ? -wbits : wrap == 2u ? wbits + 16 : wbits;
    h.kind = wrap;
    h.head = wrap == 2u ? (1u | 15u << 8) : wrap == 1u ? (uint32_t)wbits << 8 : 15u << 8;
    h.chunk_bytes = chunk_bytes;
    h.consumed = out_len;
    h.total = in_len;
    h.trailer = out_len - (wrap == 1u ? 4u : wrap == 2u ? 8u : 0u);
    h.npoints = npoints;
    return h;
}

/* R_b of one block; `syms` = the block's first symbol.  The same in every lane. */
DEV uint32_t dix_block_reach(const uint32_t *syms, const ZdBlockRec *rec, const ZdBlockPlan *plan)
{
    const uint32_t type = plan->type;
    if (type != ZD_BT_STATIC && type != ZD_BT_DYNAMIC)
        return 0; /* stored, or nothing was emitted (Z_BUF_ERROR) */
    const uint32_t count = rec->sym_count;
    uint32_t pos = 0; /* of symbol s, relative to in_begin (wave-uniform) */
    LANEVAR(uint32_t, best);
    FOR_LANES { LV(best) = 0; }
    /* (a distance is at most ZIDX_WIN: from there on no symbol reaches before the block) */
    for (uint32_t s = 0; s < count && pos < ZIDX_WIN; s += WAVE) {
        LANEVAR(uint32_t, dist);
        LANEVAR(uint32_t, len);
        LANEVAR(uint32_t, ex);
        uint32_t tot;
        FOR_LANES
        {
            const uint32_t i = s + (uint32_t)LANE;
            const uint32_t sym = i < count ? syms[i] : 0u;
            LV(dist) = sym >> 16;
            LV(len) = i < count ? ((sym >> 16) ? (sym & 0xffu) + 3u : 1u) : 0u;
        }
        WAVE_EXSCAN(len, ex, tot);
        FOR_LANES
        {
            const uint32_t p = pos + LV(ex);
            if (LV(dist) > p && LV(dist) - p > LV(best))
                LV(best) = LV(dist) - p;
        }
        pos += tot;
    }
    FOR_LANES { LV(best) = ~LV(best); }
    return ~WAVE_MIN_U32(best);
}

/* The points of one buffer (one thread).  recs / plans / reach: the buffer's first block; out: room for
 * `cap` records, of which *npts are written -- 0 for a buffer whose stream was not written.  ck and woff
 * are left to dix_piece_check and the export. */
DEV void dix_points(const ZdBuf *buf, const ZdParseOut *po, const ZdBlockRec *recs, const ZdBlockPlan *plans,
                    const uint32_t *reach, const ZdResult *res, uint32_t chunk_bytes, ZidxRec *out, uint32_t cap,
                    uint32_t *npts)
{
    if (res->status != 0 || po->nblocks > buf->max_blocks || cap == 0u) {
        *npts = 0;
        return;
    }
    const uint64_t cbits = 8ull * chunk_bytes;
    uint32_t n = 1;
    uint64_t chunk = 0;
    ZidxRec cur;
    cur.bit = 0; /* the first piece parses the stream's real header */
    cur.woff = 0;
    cur.off = 0;
    cur.len = 0;
    cur.ck = 0;
    cur.wlen = 0;
    for (uint32_t i = 0; i < po->nblocks; i++) {
        const ZdBlockRec *r = &recs[i];
        const uint64_t at = (uint64_t)plans[i].bit_off / cbits;
        if (i != 0u && r->in_len > 0u && at > chunk && n < cap) {
            cur.len = r->in_begin - cur.off;
            out[n - 1u] = cur;
            cur.bit = plans[i].bit_off; /* the first bit of the 3-bit block header */
            cur.off = r->in_begin;
            cur.wlen = 0;
            chunk = at;
            n++;
        }
        const uint32_t back = r->in_begin - cur.off; /* the piece's bytes before this block */
        if (reach[i] > back && reach[i] - back > cur.wlen)
            cur.wlen = reach[i] - back;
        DIX_ASSERT(cur.wlen <= cur.off && cur.wlen <= ZIDX_WIN);
    }
    cur.len = buf->in_len - cur.off;
    out[n - 1u] = cur;
    *npts = n;
}

/* the check value of one piece's input, as the indexed plan's write pass takes it of the piece's output;
 * `in` = the buffer's input */
DEV uint32_t dix_piece_check(const uint8_t *in, const ZidxRec *r, uint32_t wrap, CkLds *lds)
{
    return wrap == 2u ? ck_crc32(in + r->off, r->len, lds) : ck_adler32(in + r->off, r->len);
}

/* export: the window of record r copied from the buffer's input to out + r->woff by nthr threads */
DEV void dix_gather(const uint8_t *in, const ZidxRec *r, uint8_t *out, uint32_t tid, uint32_t nthr)
{
    const uint32_t wlen = r->wlen;
    if (wlen > r->off)
        return; /* (cannot happen; nothing is read before the buffer) */
    const uint8_t *w = in + (r->off - wlen);
    for (uint32_t x = tid; x < wlen; x += nthr)
        out[r->woff + x] = w[x];
}

#endif
