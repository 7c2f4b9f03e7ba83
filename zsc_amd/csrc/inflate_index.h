/*
 * inflate_index.h -- kernel 9: a stream inflated from a seek-point index.
 *
 * A chunks plan (inflate_chunks.h) finds out, on every run, where the chained pieces of a stream
 * start, how long each one's output is and which bytes before its start it reads.  With the index
 * enabled it keeps these facts: the index of one stream is one blob (layout: include/zsc_hip.h) with a
 * point per chained piece -- start as a bit offset, output offset and length, the check value of the
 * piece's own output, and its window cut down to the bytes the piece reaches.  An indexed plan decodes
 * from the blob with none of the chunks plan's scan, count, retry, resolve or window launches:
 *   1. write    (idx_write_worker) every piece decoded into place from its point with its window, by
 *               inflate_stream<INF_SEC_BITSTART | INF_SEC_EXTWIN | INF_SEC_NOTRAIL> as the chunks
 *               plan's write pass; the candidate list holds each chunk's one point;
 *   2. finish   sec_finish of inflate_sections.h, unchanged;
 *   3. k_inflate over the plan for everything the path did not finish.
 *
 * The rule is the one of the sections and chunks paths: the path only ever reports a clean Z_OK.  A
 * piece counts only if it stopped exactly at the next point (the last one: at the final block, at the
 * indexed trailer offset), produced exactly the indexed length, reached back exactly as far as its
 * window is long, used no distance beyond the header's limit, and its output has the indexed check
 * value; the first piece parses the stream's real header and its verdict (gzip, distance limit) must
 * be the index's.  Then the chain runs from the stream's true start through block boundaries the
 * decoder itself reached to the true final block, and sec_finish compares the combined check value of
 * the bytes that were written with the stream's own trailer.  Everything else is decoded serially from
 * the stream's start.  (A raw stream has no trailer and a range is not checked against one: see
 * include/zsc_hip.h.)
 *
 * Memory safety: the device windows are packed one behind the other behind INF_WIN zero bytes.  A
 * piece's window pointer is set so that its window ends where INF_WIN entries would; a distance is at
 * most 32 768, so a reach beyond the window's length reads the bytes before it in the same allocation
 * (the guard, or other windows), never outside, and fails the piece (reach != window length).  Every
 * other offset of a blob is checked on the host before anything is uploaded (zidx_validate).
 *
 * The first part of this file is plain C++ without any device code: the blob's format and the host
 * functions, shared with tests/emu_index.
 */
#ifndef ZSC_INFLATE_INDEX_H
#define ZSC_INFLATE_INDEX_H

#include <stdint.h>
#include <string.h>

/* ---- the blob (little-endian; documented field by field in include/zsc_hip.h) ---- */
#define ZIDX_MAGIC 0x4943535au /* "ZSCI" */
#define ZIDX_VERSION 1u
#define ZIDX_HEADER 48u
#define ZIDX_POINT 32u
#define ZIDX_WIN 32768u      /* the longest window */
#define ZIDX_MIN_CHUNK 256u  /* the least chunk_bytes a blob may name (bounds the candidate table) */
/* header offsets */
#define ZIDX_H_MAGIC 0u
#define ZIDX_H_VERSION 4u
#define ZIDX_H_CRC 8u        /* CRC-32 of blob[12 .. len) */
#define ZIDX_H_WBITS 12u
#define ZIDX_H_KIND 16u      /* 0 raw, 1 zlib, 2 gzip */
#define ZIDX_H_HEAD 20u      /* gzip | log2(distance limit) << 8 */
#define ZIDX_H_CHUNK 24u
#define ZIDX_H_CONSUMED 28u
#define ZIDX_H_TOTAL 32u
#define ZIDX_H_TRAILER 36u
#define ZIDX_H_NPOINTS 40u
#define ZIDX_H_RESERVED 44u  /* 0 */
/* point offsets */
#define ZIDX_P_BIT 0u        /* u64 */
#define ZIDX_P_WOFF 8u       /* u64: from the blob's start */
#define ZIDX_P_OFF 16u
#define ZIDX_P_LEN 20u
#define ZIDX_P_CHECK 24u
#define ZIDX_P_WLEN 28u

typedef struct {
    int32_t window_bits;
    uint32_t kind, head, chunk_bytes, consumed, total, trailer, npoints;
} ZidxInfo;

/* a point as the export kernel writes it and the blob stores it (woff: from the first window on the
 * device, from the blob's start in a blob) */
typedef struct {
    uint64_t bit, woff;
    uint32_t off, len, ck, wlen;
} ZidxRec;

static inline uint32_t zidx_ld32(const uint8_t *p)
{
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
static inline uint64_t zidx_ld64(const uint8_t *p) { return (uint64_t)zidx_ld32(p) | (uint64_t)zidx_ld32(p + 4) << 32; }
static inline void zidx_st32(uint8_t *p, uint32_t v)
{
    p[0] = (uint8_t)v;
    p[1] = (uint8_t)(v >> 8);
    p[2] = (uint8_t)(v >> 16);
    p[3] = (uint8_t)(v >> 24);
}
static inline void zidx_st64(uint8_t *p, uint64_t v)
{
    zidx_st32(p, (uint32_t)v);
    zidx_st32(p + 4, (uint32_t)(v >> 32));
}

/* CRC-32 (the gzip polynomial), four bits at a time */
static inline uint32_t zidx_crc32(const uint8_t *p, uint64_t n)
{
    static const uint32_t t[16] = {0x00000000u, 0x1db71064u, 0x3b6e20c8u, 0x26d930acu, 0x76dc4190u, 0x6b6b51f4u,
                                   0x4db26158u, 0x5005713cu, 0xedb88320u, 0xf00f9344u, 0xd6d6a3e8u, 0xcb61b38cu,
                                   0x9b64c2b0u, 0x86d3d2d4u, 0xa00ae278u, 0xbdbdf21cu};
    uint32_t c = 0xffffffffu;
    for (uint64_t i = 0; i < n; i++) {
        c ^= p[i];
        c = (c >> 4) ^ t[c & 15u];
        c = (c >> 4) ^ t[c & 15u];
    }
    return ~c;
}

static inline void zidx_point(const uint8_t *blob, uint32_t i, ZidxRec *r)
{
    const uint8_t *p = blob + ZIDX_HEADER + (uint64_t)ZIDX_POINT * i;
    r->bit = zidx_ld64(p + ZIDX_P_BIT);
    r->woff = zidx_ld64(p + ZIDX_P_WOFF);
    r->off = zidx_ld32(p + ZIDX_P_OFF);
    r->len = zidx_ld32(p + ZIDX_P_LEN);
    r->ck = zidx_ld32(p + ZIDX_P_CHECK);
    r->wlen = zidx_ld32(p + ZIDX_P_WLEN);
}

/* Is the blob a well-formed index?  1, and *info (may be NULL) filled; 0 otherwise.  Beyond the list in
 * include/zsc_hip.h the layout is canonical: the windows lie in point order, without gaps, from the end
 * of the points to the end of the blob. */
static inline int zidx_validate(const uint8_t *blob, uint64_t len, ZidxInfo *info)
{
    if (blob == nullptr || len < ZIDX_HEADER + ZIDX_POINT)
        return 0;
    if (zidx_ld32(blob + ZIDX_H_MAGIC) != ZIDX_MAGIC || zidx_ld32(blob + ZIDX_H_VERSION) != ZIDX_VERSION)
        return 0;
    if (zidx_ld32(blob + ZIDX_H_CRC) != zidx_crc32(blob + ZIDX_H_WBITS, len - ZIDX_H_WBITS))
        return 0;
    ZidxInfo h;
    h.window_bits = (int32_t)zidx_ld32(blob + ZIDX_H_WBITS);
    h.kind = zidx_ld32(blob + ZIDX_H_KIND);
    h.head = zidx_ld32(blob + ZIDX_H_HEAD);
    h.chunk_bytes = zidx_ld32(blob + ZIDX_H_CHUNK);
    h.consumed = zidx_ld32(blob + ZIDX_H_CONSUMED);
    h.total = zidx_ld32(blob + ZIDX_H_TOTAL);
    h.trailer = zidx_ld32(blob + ZIDX_H_TRAILER);
    h.npoints = zidx_ld32(blob + ZIDX_H_NPOINTS);
    if (zidx_ld32(blob + ZIDX_H_RESERVED) != 0u)
        return 0;
    /* the wrapper: raw with a negative window_bits only; gzip as the header field says */
    if ((h.head & ~0x1f01u) != 0u || ((h.head >> 8) & 31u) > 15u)
        return 0;
    if (h.kind != (h.window_bits < 0 ? 0u : (h.head & 1u) ? 2u : 1u))
        return 0;
    if (h.chunk_bytes < ZIDX_MIN_CHUNK || h.total >= 0x80000000u)
        return 0;
    if ((uint64_t)h.trailer + (h.kind == 0u ? 0u : h.kind == 1u ? 4u : 8u) != h.consumed)
        return 0;
    if (h.npoints == 0u || (len - ZIDX_HEADER) / ZIDX_POINT < h.npoints)
        return 0;
    uint64_t wat = ZIDX_HEADER + (uint64_t)ZIDX_POINT * h.npoints, sum = 0, chunk = 0, bit = 0;
    const uint64_t cbits = (uint64_t)h.chunk_bytes * 8u;
    for (uint32_t i = 0; i < h.npoints; i++) {
        ZidxRec r;
        zidx_point(blob, i, &r);
        if (i == 0u ? (r.bit != 0u || r.wlen != 0u) : (r.bit <= bit || r.bit / cbits <= chunk))
            return 0; /* strictly ascending in bit offset and in chunk: at most one per chunk */
        if (r.bit > (uint64_t)h.trailer * 8u)
            return 0;
        if (r.off != sum || r.len > h.total - sum)
            return 0;
        if (r.wlen > ZIDX_WIN || r.wlen > sum || r.woff != wat || r.wlen > len - wat)
            return 0;
        bit = r.bit;
        chunk = r.bit / cbits;
        sum += r.len;
        wat += r.wlen;
    }
    if (sum != h.total || wat != len)
        return 0;
    if (info)
        *info = h;
    return 1;
}

/* The smallest run of whole pieces that covers output bytes [begin, begin + n) of a valid blob:
 * 1 and the run; 0 when the range is empty or not inside the output. */
static inline int zidx_range(const uint8_t *blob, const ZidxInfo *h, uint64_t begin, uint64_t n, uint32_t *first,
                             uint32_t *count, uint32_t *piece_begin, uint32_t *piece_len)
{
    if (n == 0u || begin >= h->total || n > h->total - begin)
        return 0;
    const uint8_t *pts = blob + ZIDX_HEADER;
    /* the last point at or before `begin`, the last point before the range's end */
    uint32_t lo = 0, hi = h->npoints;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (zidx_ld32(pts + (uint64_t)ZIDX_POINT * mid + ZIDX_P_OFF) <= begin)
            lo = mid;
        else
            hi = mid;
    }
    const uint32_t f = lo;
    hi = h->npoints;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (zidx_ld32(pts + (uint64_t)ZIDX_POINT * mid + ZIDX_P_OFF) < begin + n)
            lo = mid;
        else
            hi = mid;
    }
    ZidxRec a, b;
    zidx_point(blob, f, &a);
    zidx_point(blob, lo, &b);
    *first = f;
    *count = lo - f + 1u;
    *piece_begin = a.off;
    *piece_len = b.off + b.len - a.off;
    return 1;
}

/* bytes of the blob of `n` records whose windows take `wbytes` */
static inline uint64_t zidx_blob_bytes(uint32_t n, uint64_t wbytes) { return ZIDX_HEADER + (uint64_t)ZIDX_POINT * n + wbytes; }

/* Write the blob: header from *h, points from recs (woff counted from the first window), then the
 * windows, which the caller has put (or puts before zidx_seal) at blob + zidx_blob_bytes(n, 0). */
static inline void zidx_write_head(uint8_t *blob, const ZidxInfo *h, const ZidxRec *recs)
{
    zidx_st32(blob + ZIDX_H_MAGIC, ZIDX_MAGIC);
    zidx_st32(blob + ZIDX_H_VERSION, ZIDX_VERSION);
    zidx_st32(blob + ZIDX_H_CRC, 0u);
    zidx_st32(blob + ZIDX_H_WBITS, (uint32_t)h->window_bits);
    zidx_st32(blob + ZIDX_H_KIND, h->kind);
    zidx_st32(blob + ZIDX_H_HEAD, h->head);
    zidx_st32(blob + ZIDX_H_CHUNK, h->chunk_bytes);
    zidx_st32(blob + ZIDX_H_CONSUMED, h->consumed);
    zidx_st32(blob + ZIDX_H_TOTAL, h->total);
    zidx_st32(blob + ZIDX_H_TRAILER, h->trailer);
    zidx_st32(blob + ZIDX_H_NPOINTS, h->npoints);
    zidx_st32(blob + ZIDX_H_RESERVED, 0u);
    const uint64_t w0 = zidx_blob_bytes(h->npoints, 0);
    for (uint32_t i = 0; i < h->npoints; i++) {
        uint8_t *p = blob + ZIDX_HEADER + (uint64_t)ZIDX_POINT * i;
        zidx_st64(p + ZIDX_P_BIT, recs[i].bit);
        zidx_st64(p + ZIDX_P_WOFF, w0 + recs[i].woff);
        zidx_st32(p + ZIDX_P_OFF, recs[i].off);
        zidx_st32(p + ZIDX_P_LEN, recs[i].len);
        zidx_st32(p + ZIDX_P_CHECK, recs[i].ck);
        zidx_st32(p + ZIDX_P_WLEN, recs[i].wlen);
    }
}
static inline void zidx_seal(uint8_t *blob, uint64_t len)
{
    zidx_st32(blob + ZIDX_H_CRC, zidx_crc32(blob + ZIDX_H_WBITS, len - ZIDX_H_WBITS));
}

/* ---- device code (and its lane emulation) ---- */
#ifndef ZIDX_HOST_ONLY

#include "inflate_chunks.h"

static_assert(ZIDX_WIN == INF_WIN, "a window is the decoder's");
static_assert(sizeof(ZidxRec) == ZIDX_POINT, "a record is a point of the blob");

#define IDX_FIRST 1u
#define IDX_LAST 2u
/* one decode unit of an indexed plan: a piece of a stream (host-built, read-only) */
typedef struct {
    uint64_t bit;     /* where it starts */
    uint64_t end_bit; /* where it must stop: the next point, or 8 * the trailer's offset */
    uint64_t wend;    /* its window ends at P.win + wend + INF_WIN (INF_WIN guard bytes lie in front of the windows) */
    uint32_t off, len, ck, wlen;
    uint32_t stream, flags;
} IdxPiece;

/* per stream with an index (host-built; `done` is zeroed before every run) */
typedef struct {
    uint64_t cand_off;   /* its candidate table in P.cand */
    uint32_t nchunks;    /* the last point's chunk + 1 */
    uint32_t chunk_bytes;
    uint32_t range;      /* 1: a range item -- the last unit to end writes the result */
    uint32_t nunits;
    uint32_t shift;      /* a range's piece_begin: its output starts at the item's dst_offset */
    uint32_t out_len, consumed; /* a range's result */
    uint32_t pad;
} IdxStream;

typedef struct {
    IsecPlan sp;           /* items, st (base: the stream's first unit slot; nchain, head, total, trailer from the
                            * index), active (the whole-stream items), q, nsec, clen, chain_k, chain_ck: for sec_finish */
    const IdxPiece *pieces; /* per slot */
    const uint32_t *units;  /* slots, longest output first */
    const IdxStream *xs;    /* per stream */
    uint32_t *done;         /* per stream: units ended */
    const uint64_t *cand;
    const uint8_t *win;
    uint32_t nunits;
} IidxPlan;

#ifdef ZSC_WAVE_EMU
#define IDX_FENCE() ((void)0)
#else
#define IDX_FENCE() __threadfence()
#endif

/* ---- export: the records and windows of a chunks plan's chain (whole-wave / per-thread code) ---- */

/* record i of stream s's chain; woff is left to the prefix sum */
DEV void idx_record(const IchkPlan &P, uint32_t s, uint32_t i, ZidxRec *r)
{
    const uint32_t cb = P.sp.st[s].base, k = P.sp.chain_k[cb + i];
    const uint32_t reach = P.creach[cb + k];
    r->bit = P.cand[(uint64_t)(cb + k) * INF_PC_CANDS + P.cused[cb + k]];
    r->woff = 0;
    r->off = P.sp.chain_off[cb + i];
    r->len = P.sp.clen[cb + k];
    r->ck = P.sp.chain_ck[cb + i];
    r->wlen = reach < INF_WIN ? reach : INF_WIN;
}

/* the window of record r (chain entry i of stream s) copied to out + r->woff by nthr threads */
DEV void idx_gather(const IchkPlan &P, uint32_t s, uint32_t i, const ZidxRec *r, uint8_t *out, uint32_t tid,
                    uint32_t nthr)
{
    const uint32_t cb = P.sp.st[s].base, k = P.sp.chain_k[cb + i], wlen = r->wlen;
    const uint8_t *w = P.win + (uint64_t)(cb + k) * INF_WIN + (INF_WIN - wlen);
    for (uint32_t x = tid; x < wlen; x += nthr)
        out[r->woff + x] = w[x];
}

/* ---- group code (INF_GROUP lanes per unit, as the decoder) ---- */
#undef ZSC_GROUP
#define ZSC_GROUP INF_GROUP
#include "wave_group.h"

#ifdef ZSC_WAVE_EMU
#define IDX_GBCAST(v) (v)
#else
#define IDX_GBCAST(v) ((uint32_t)__shfl((int)(v), (int)(threadIdx.x & (64u - GRP))))
#endif

/* step 1: a group decodes units into place until the queue (q[2]) is empty */
DEV void idx_write_worker(const IidxPlan &P, const uint8_t *src_all, uint8_t *dst_all, InfLds *lds, InfSecInfo *si,
                          InfPiece *pc, InfResult *res, InfResume *resume)
{
    for (;;) {
        uint32_t u = 0;
        ON_GLANE0 { u = SEC_ADD(&P.sp.q[2], 1u); }
        u = IDX_GBCAST(u);
        if (u >= P.nunits)
            break;
        const uint32_t slot = GUNI(P.units[u]);
        const IdxPiece *p = &P.pieces[slot];
        const uint32_t s = GUNI(p->stream), flags = GUNI(p->flags), len = GUNI(p->len), wlen = GUNI(p->wlen);
        IsecStream *S = &P.sp.st[s];
        const IdxStream *X = &P.xs[s];
        const IsecItem *it = &P.sp.items[s];
        const uint64_t bit = p->bit;
        const uint32_t start = (uint32_t)(bit >> 3);
        ON_GLANE0
        {
            pc->base_bit = bit & ~7ull;
            pc->chunk_bits = (uint64_t)X->chunk_bytes * 8u;
            pc->cand = P.cand + X->cand_off;
            pc->ring = nullptr;
            pc->win = P.win + p->wend; /* (win[INF_WIN - d]: d bytes before the window's end) */
            pc->skip = (uint32_t)(bit & 7u);
            pc->chunk = (uint32_t)(bit / ((uint64_t)X->chunk_bytes * 8u));
            pc->nchunks = X->nchunks;
        }
        WAVE_SYNC();
        uint8_t *dst = dst_all + it->dst_off + (p->off - X->shift);
        InfJob job;
        job.src = src_all + it->src_off + start;
        job.n = GUNI(it->src_len) - start;
        job.dst = dst;
        job.cap = len;
        job.window_bits = (flags & IDX_FIRST) ? P.sp.window_bits : -15;
        inflate_stream<INF_SEC_BITSTART | INF_SEC_EXTWIN | INF_SEC_NOTRAIL>(job, lds, nullptr, nullptr, si, pc);
        SEC_FENCE();
        const uint32_t head = GUNI(S->head);
        const uint32_t ck = (head & 1u) ? INF_CK(crc32_tx)<1>(dst, len, lds->cktab, INF_CKX(lds))
                                        : INF_CK(adler32)(dst, len);
        ON_GLANE0
        {
            int good = si->out_len == len && pc->reach == wlen && ck == p->ck &&
                       si->maxd <= (1u << ((head >> 8) & 31u));
            if (flags & IDX_LAST)
                good = good && si->outcome == INF_SEC_FINAL && ((uint64_t)start + si->stop) * 8u == p->end_bit;
            else
                good = good && si->outcome == INF_SEC_SYNC && pc->end_bit == p->end_bit;
            if (flags & IDX_FIRST) /* the real header's verdict is the index's */
                good = good && (si->gzip | (31u - CLZ32(si->dmax)) << 8) == head;
            P.sp.chain_ck[slot] = ck;
            if (!good)
                SEC_OR(&S->serial, 1u);
            if (X->range) {
                IDX_FENCE();
                if (SEC_ADD(&P.done[s], 1u) + 1u == X->nunits) {
                    IDX_FENCE();
                    const uint32_t bad = SEC_LOAD(&S->serial);
                    res[s].status = bad ? INF_DATA : 0;
                    res[s].out_len = bad ? 0u : X->out_len;
                    res[s].consumed = bad ? 0u : X->consumed;
                    res[s].pad = 0;
                    resume[s].state = 2;
                    P.sp.nsec[s] = bad ? 0u : X->nunits;
                }
            }
        }
        WAVE_SYNC();
    }
}

#undef IDX_GBCAST
/* back to whole-wave groups for whatever is compiled after this */
#undef ZSC_GROUP
#define ZSC_GROUP 64
#include "wave_group.h"


/* ---- host side of an indexed plan: the device tables from the blobs (shared with tests/emu_index) ---- */
#include <algorithm>
#include <vector>

struct IdxBuild {
    std::vector<IsecItem> items;
    std::vector<IsecStream> st;   /* the state every run starts from */
    std::vector<IdxStream> xs;
    std::vector<IdxPiece> pieces;
    std::vector<uint32_t> units, active, clen, chain_k;
    std::vector<uint64_t> cand;
    std::vector<uint8_t> win;
    std::vector<InfResult> res0;  /* results fixed at create: a range item that cannot be decoded */
    std::vector<uint32_t> state0; /* ... and its resume state (2: finished) */
    bool any_fixed = false;

    IdxBuild() : win(INF_WIN, 0) {}

    /* Stream i of the plan.  0, or -2 (Z_STREAM_ERROR) for a range that is not inside the output.  A
     * stream whose blob cannot be used stays without units: the serial decoder takes it (a whole
     * stream), or its result is fixed here (a range: Z_DATA_ERROR, or Z_BUF_ERROR for a dest_cap
     * below piece_len; nothing written, nothing consumed). */
    int add(uint32_t src_len, uint64_t src_off, uint32_t dst_cap, uint64_t dst_off, int32_t window_bits,
            const uint8_t *blob, uint64_t blob_len, bool has_range, uint64_t rbegin, uint64_t rlen)
    {
        const uint32_t i = (uint32_t)items.size();
        IsecItem it = {};
        it.src_off = src_off;
        it.dst_off = dst_off;
        it.src_len = src_len;
        it.dst_cap = dst_cap;
        items.push_back(it);
        st.push_back(IsecStream{});
        xs.push_back(IdxStream{});
        res0.push_back(InfResult{0, 0, 0, 0});
        state0.push_back(0);
        ZidxInfo h;
        const bool valid = blob != nullptr && zidx_validate(blob, blob_len, &h) && h.window_bits == window_bits &&
                           src_len >= h.consumed;
        uint32_t first = 0, count = 0, pbegin = 0, plen = 0;
        if (has_range) {
            if (valid && !zidx_range(blob, &h, rbegin, rlen, &first, &count, &pbegin, &plen))
                return -2;
            if (!valid || dst_cap < plen) {
                res0[i].status = valid ? INF_BUF : INF_DATA;
                state0[i] = 2;
                any_fixed = true;
                return 0;
            }
        } else {
            if (!valid || dst_cap < h.total)
                return 0;
            count = h.npoints;
            plen = h.total;
        }
        IsecStream &S = st[i];
        IdxStream &X = xs[i];
        S.base = (uint32_t)pieces.size();
        S.nchain = has_range ? 0u : count;
        S.head = h.head;
        S.total = h.total;
        S.trailer = h.trailer;
        const uint64_t cbits = (uint64_t)h.chunk_bytes * 8u;
        ZidxRec r, nx;
        zidx_point(blob, first, &r);
        uint64_t end_bit = 0;
        X.cand_off = cand.size();
        for (uint32_t j = first; j < first + count; j++, r = nx) {
            const bool last = j + 1u == h.npoints;
            nx = r;
            if (!last) {
                zidx_point(blob, j + 1u, &nx);
                /* the candidate list: each chunk's one point (only the points a unit may stop at) */
                const uint64_t m = nx.bit / cbits;
                cand.resize(X.cand_off + (m + 1u) * INF_PC_CANDS, INF_PC_NONE);
                cand[X.cand_off + m * INF_PC_CANDS] = nx.bit;
                X.nchunks = (uint32_t)(m + 1u);
            }
            end_bit = last ? (uint64_t)h.trailer * 8u : nx.bit;
            win.insert(win.end(), blob + r.woff, blob + r.woff + r.wlen);
            IdxPiece p = {};
            p.bit = r.bit;
            p.end_bit = end_bit;
            p.wend = win.size() - INF_WIN;
            p.off = r.off;
            p.len = r.len;
            p.ck = r.ck;
            p.wlen = r.wlen;
            p.stream = i;
            p.flags = (j == 0u ? IDX_FIRST : 0u) | (last ? IDX_LAST : 0u);
            pieces.push_back(p);
            clen.push_back(r.len);
            chain_k.push_back(j - first);
        }
        if (X.nchunks == 0u)
            X.nchunks = (uint32_t)(r.bit / cbits) + 1u; /* (only the stream's last piece: it stops at no point) */
        X.chunk_bytes = h.chunk_bytes;
        X.range = has_range ? 1u : 0u;
        X.nunits = count;
        X.shift = has_range ? pbegin : 0u;
        X.out_len = plen;
        X.consumed = (uint32_t)((end_bit + 7u) >> 3);
        if (!has_range)
            active.push_back(i);
        return 0;
    }

    /* the decode order: longest output first (known before any launch; k_inflate's rule for streams) */
    void finish()
    {
        units.resize(pieces.size());
        for (uint32_t u = 0; u < units.size(); u++)
            units[u] = u;
        std::stable_sort(units.begin(), units.end(),
                         [&](uint32_t a, uint32_t b) { return pieces[a].len > pieces[b].len; });
    }
};

#endif /* ZIDX_HOST_ONLY */
#endif
