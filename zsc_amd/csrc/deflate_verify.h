/*
 * deflate_verify.h -- kernels 4f-4h: read-back verification of a deflate plan's streams against their
 * input.
 *
 * A deflate plan leaves its streams in HBM with a status of Z_OK.  What the compressor knows makes it
 * cheap to check that they decode to the input, with no second output image: ZdBlockPlan.bit_off is
 * where every block starts, ZdBlockRec.in_begin / in_len / last are the input bytes it stands for, and
 * the input itself is the decoder's window.  So every block of every stream is checked on its own:
 *   keep    (dvf_keep, one thread per block slot of a sub-batch, after layout and before the next
 *           sub-batch reuses the records and plans) 16 bytes of facts per block -- bit offset, in_begin,
 *           in_len, type | last << 8 -- to storage the plan owns for the blocks of all sub-batches, and
 *           the block count per buffer;
 *   blocks  (dvf_check_block, one wave per kept block, all buffers in one launch) decodes the block from
 *           the emitted bits: the 3-bit header against the kept type and last flag; a stored block's
 *           padding, LEN / NLEN and bytes; a dynamic block's code description under the decoder's rules
 *           (inf_build, INF_HDR_*: inflate.h); every literal against input[p], every match as
 *           1 <= dist <= min(p, 1 << window_bits) and input[p + i] == input[p + i - dist]; the
 *           end-of-block code on the block's last input byte and on the next block's first bit (the last
 *           block: zero padding up to the trailer).  Symbol decode is serial, with wave-uniform state; the
 *           stream and the input pass through the lanes' registers 4 * WAVE bytes at a time; the compare
 *           of a match, of a stored block's bytes and the block's check value (checksum.h) are
 *           lane-parallel.  Nothing is read beyond the stream's out_cap or the buffer's in_len, whatever
 *           the bits say: a block that would run past its end fails, it does not fault;
 *   finish  (dvf_finish, one thread per buffer) the blocks tile [0, in_len) in order, the verdict of the
 *           lowest-numbered failing block; with none, the header bytes are the plan's, the blocks' check
 *           values combined (inflate_sections.h) equal the trailer's as read from the stream, ISIZE.
 * Nothing is taken from the symbol buffers, the Huffman plans or ZdResult.adler.
 *
 * Whole-wave code on wave.h, compiled a second time by tests/emu_verify.
 */
#ifndef ZSC_DEFLATE_VERIFY_H
#define ZSC_DEFLATE_VERIFY_H

#include "checksum.h"
#include "inflate_sections.h" /* sec_*_combine; inflate.h: InfCodeT, inf_build, inf_input_dword, INF_HDR_* */
#include "wave.h"
#include "zsc_dev.h"

static_assert(WAVE >= 16, "lane l tests the codes of length l, 1..15");

/* the verdicts: ZSC_HIP_VERIFY_* of include/zsc_hip.h */
#define DVF_OK 0
#define DVF_SKIPPED (-1)
#define DVF_HEADER 1
#define DVF_BLOCK_HDR 2
#define DVF_CODES 3
#define DVF_LITERAL 4
#define DVF_DISTANCE 5
#define DVF_MATCH 6
#define DVF_LENGTH 7
#define DVF_BIT_END 8
#define DVF_TRAILER 9
#define DVF_NONE 0xffffffffu

typedef struct {
    uint32_t bit_off, in_begin, in_len, type_last; /* ZD_BT_* | last << 8: zsc_hip_verify_block */
} DvfBlock;

/* what the check of one block leaves for the finisher */
typedef struct {
    uint32_t reason; /* DVF_OK or why the block failed */
    uint32_t in_pos; /* the input offset the check had reached */
    uint32_t ck;     /* CRC-32 (gzip) / Adler-32 (zlib) of the block's input */
    uint32_t pad;
} DvfVerdict;

typedef struct {
    int32_t verdict;
    uint32_t block, bit_off, in_pos; /* zsc_hip_verify_result */
} DvfResult;

/* one buffer of the plan */
typedef struct {
    uint64_t in_off, out_off; /* as the plan was given them */
    uint32_t in_len, out_cap;
    uint32_t first;           /* its first kept block */
    uint32_t max_blocks;
} DvfBuf;

typedef struct {
    InfCodeT<288> lit;
    union {
        InfCodeT<32> dist;
        InfCodeT<20> cl; /* dead once the lengths are read */
    };
    uint8_t lens[320];
    CkLds ck;
} DvfLds;

/* keep: block j of one buffer; recs / plans / out: the buffer's first */
DEV void dvf_keep(const ZdBuf *buf, const ZdParseOut *po, const ZdBlockRec *recs, const ZdBlockPlan *plans,
                  const ZdResult *res, uint32_t j, DvfBlock *out, uint32_t *nblk)
{
    const uint32_t n = res->status == 0 && po->nblocks <= buf->max_blocks ? po->nblocks : 0u;
    if (j == 0u)
        *nblk = n;
    if (j < n) {
        DvfBlock b;
        b.bit_off = plans[j].bit_off;
        b.in_begin = recs[j].in_begin;
        b.in_len = recs[j].in_len;
        b.type_last = plans[j].type | (recs[j].last ? 1u : 0u) << 8;
        out[j] = b;
    }
}

/* bytes a .. a+3 of b as a dword, zero from byte n on; reads exactly the bytes below n */
DEV uint32_t dvf_dword(const uint8_t *b, uint32_t a, uint32_t n)
{
    if (a + 4u <= n)
        return ld_u32(b + a);
    uint32_t v = 0;
    for (uint32_t j = 0; j < 4u; j++)
        if (a + j < n)
            v |= (uint32_t)b[a + j] << (8u * j);
    return v;
}

/* The wave-uniform bit reader: `hold` has nbits bits of the stream, next_dw is the next dword to pull
 * into it, out of the WAVE dwords from chunk_dw on that the lanes hold in `cur`. */
#define VF_PULL()                                                                                      \
    do {                                                                                               \
        if (next_dw - chunk_dw >= (uint32_t)WAVE) {                                                    \
            chunk_dw = next_dw;                                                                        \
            FOR_LANES { LV(cur) = inf_input_dword(src, 4u * (chunk_dw + (uint32_t)LANE), src_n); }     \
        }                                                                                              \
        hold |= (uint64_t)(uint32_t)READLANE(cur, next_dw - chunk_dw) << nbits;                        \
        nbits += 32u;                                                                                  \
        next_dw++;                                                                                     \
    } while (0)
#define VF_NEED(nb)           \
    while (nbits < (nb))      \
    VF_PULL() /* nb <= 32 */
#define VF_TAKE(var, nb)                                        \
    do {                                                        \
        (var) = (uint32_t)(hold & ((1ull << (nb)) - 1ull));     \
        hold >>= (nb);                                          \
        nbits -= (nb);                                          \
    } while (0)
#define VF_USED ((uint64_t)next_dw * 32u - nbits)
#define VF_FAIL(r)      \
    do {                \
        *in_pos = p;    \
        return (r);     \
    } while (0)

/* lane l gets first | count << 16 of the codes of length l of a code inf_build accepted */
#define VF_LOAD_FC(C, FC)                                                                           \
    FOR_LANES                                                                                       \
    {                                                                                               \
        const uint32_t _l = (uint32_t)LANE;                                                         \
        LV(FC) = _l >= 1u && _l <= (C)->max_len ? (uint32_t)(C)->first[_l] | (uint32_t)(C)->count[_l] << 16 : 0u; \
    }

/* one symbol of code C (inflate.h's table-free decode: the 15 bits MSB first, lane l tests length l, the
 * lowest hit is the code's length); -1 where the bits are no code of the set */
#define VF_DECODE(C, FC, OUT)                                                                       \
    do {                                                                                            \
        VF_NEED(32u);                                                                               \
        const uint32_t _r = BREV32((uint32_t)hold & 0x7fffu) >> 17;                                 \
        LANEVAR(int, _hit);                                                                         \
        FOR_LANES                                                                                   \
        {                                                                                           \
            const uint32_t _l = (uint32_t)LANE & 15u, _fc = LV(FC);                                 \
            LV(_hit) = (uint32_t)LANE < 16u && ((_r >> (15u - _l)) - (_fc & 0xffffu)) < (_fc >> 16); \
        }                                                                                           \
        const uint64_t _m = BALLOT(_hit);                                                           \
        if (_m == 0) {                                                                              \
            (OUT) = -1;                                                                             \
            break;                                                                                  \
        }                                                                                           \
        const uint32_t _len = (uint32_t)CTZ64(_m);                                                  \
        const uint32_t _f = (uint32_t)READLANE(FC, _len) & 0xffffu;                                 \
        (OUT) = (int)UNI((C)->sym[(C)->offs[_len] + ((_r >> (15u - _len)) - _f)]);                  \
        hold >>= _len;                                                                              \
        nbits -= _len;                                                                              \
    } while (0)

/* Checks one block of a stream (one wave).  in / in_n: the buffer's input; src / src_n: its stream and
 * how much of it may be read (out_cap); end_bit: where the block must end -- the next block's first bit,
 * the trailer's for the last block (after its padding); wsize: 1 << window_bits.  Returns DVF_OK or the
 * reason; *in_pos = how far into the input the check got. */
DEV uint32_t dvf_check_block(const uint8_t *in, uint32_t in_n, const uint8_t *src, uint32_t src_n, DvfBlock blk,
                             uint64_t end_bit, uint32_t wsize, DvfLds *lds, uint32_t *in_pos)
{
    const uint32_t type = blk.type_last & 0xffu, last = blk.type_last >> 8;
    uint32_t p = blk.in_begin;
    if (blk.in_begin > in_n || blk.in_len > in_n - blk.in_begin)
        VF_FAIL(DVF_LENGTH);
    const uint32_t pend = blk.in_begin + blk.in_len;
    if (type > ZD_BT_DYNAMIC || last > 1u)
        VF_FAIL(DVF_BLOCK_HDR);
    /* no bit past this is the block's: reading on means it has failed */
    const uint64_t limit = end_bit < 8ull * src_n ? end_bit : 8ull * src_n;
    if ((uint64_t)blk.bit_off + 3u > limit)
        VF_FAIL(DVF_BIT_END);

    uint64_t hold = 0;
    uint32_t nbits = 0, next_dw = blk.bit_off >> 5, chunk_dw = next_dw + 1u; /* (no chunk yet) */
    LANEVAR(uint32_t, cur);
    FOR_LANES { LV(cur) = 0; }
    uint32_t v;
    VF_NEED(32u);
    VF_TAKE(v, blk.bit_off & 31u);
    VF_NEED(3u);
    VF_TAKE(v, 3u);
    if ((v & 1u) != last || (v >> 1) != type)
        VF_FAIL(DVF_BLOCK_HDR);

    if (type == ZD_BT_STORED) {
        const uint32_t padn = (8u - (uint32_t)(VF_USED & 7u)) & 7u;
        VF_NEED(8u);
        VF_TAKE(v, padn);
        if (v != 0u)
            VF_FAIL(DVF_BLOCK_HDR);
        uint32_t len, nlen;
        VF_NEED(32u);
        VF_TAKE(len, 16u);
        VF_TAKE(nlen, 16u);
        if (len != blk.in_len || nlen != (~len & 0xffffu))
            VF_FAIL(DVF_BLOCK_HDR);
        const uint64_t at64 = VF_USED >> 3;
        if ((at64 + len) * 8u > limit)
            VF_FAIL(DVF_BIT_END);
        const uint32_t at = (uint32_t)at64;
        for (uint32_t i = 0; i < len; i += 4u * WAVE) {
            LANEVAR(int, bad);
            FOR_LANES
            {
                const uint32_t k = i + 4u * (uint32_t)LANE;
                LV(bad) = k < len && dvf_dword(src, at + k, at + len) != dvf_dword(in, p + k, pend);
            }
            const uint64_t m = BALLOT(bad);
            if (m != 0) {
                p += i + 4u * (uint32_t)CTZ64(m);
                VF_FAIL(DVF_LITERAL);
            }
        }
        p = pend;
        if ((at64 + len) * 8u != end_bit)
            VF_FAIL(DVF_BIT_END);
        *in_pos = p;
        return DVF_OK;
    }

    LANEVAR(uint32_t, fc_l); /* the literal/length code, by lane = code length */
    LANEVAR(uint32_t, fc_d); /* the distance code (and, before it, the code-length code) */
    if (type == ZD_BT_STATIC) {
        for (uint32_t i = 0; i < 288u; i += WAVE) {
            FOR_LANES
            {
                const uint32_t s = i + (uint32_t)LANE;
                if (s < 288u)
                    lds->lens[s] = (uint8_t)(s < 144u ? 8u : s < 256u ? 9u : s < 280u ? 7u : 8u);
            }
        }
        WAVE_SYNC();
        (void)inf_build(&lds->lit, lds->lens, 288, 1);
        for (uint32_t i = 0; i < 32u; i += WAVE) {
            FOR_LANES
            {
                if (i + (uint32_t)LANE < 32u)
                    lds->lens[i + (uint32_t)LANE] = 5;
            }
        }
        WAVE_SYNC();
        (void)inf_build(&lds->dist, lds->lens, 32, 2);
    } else {
        uint32_t nlen, ndist, ncode;
        VF_NEED(14u);
        VF_TAKE(nlen, 5u);
        VF_TAKE(ndist, 5u);
        VF_TAKE(ncode, 4u);
        nlen += 257u;
        ndist += 1u;
        ncode += 4u;
        if (INF_HDR_COUNTS_BAD(nlen, ndist))
            VF_FAIL(DVF_CODES);
        for (uint32_t i = 0; i < 19u; i++) {
            /* the order of the code-length code's lengths: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15 */
            const uint32_t at = i < 3u ? 16u + i : i == 3u ? 0u : (i & 1u) ? 8u - ((i - 3u) >> 1) : 7u + ((i - 2u) >> 1);
            uint32_t l = 0;
            if (i < ncode) {
                VF_NEED(3u);
                VF_TAKE(l, 3u);
            }
            ON_LANE0 { lds->lens[at] = (uint8_t)l; }
        }
        WAVE_SYNC();
        if (inf_build(&lds->cl, lds->lens, 19, 0))
            VF_FAIL(DVF_CODES);
        VF_LOAD_FC(&lds->cl, fc_d);
        WAVE_SYNC();
        const uint32_t total = nlen + ndist;
        uint32_t have = 0, prev = 0;
        while (have < total) {
            int s;
            VF_DECODE(&lds->cl, fc_d, s);
            if (s < 0)
                VF_FAIL(DVF_CODES);
            uint32_t rep = 1, val = (uint32_t)s;
            if (s == 16) {
                if (INF_HDR_REP16_BAD(have))
                    VF_FAIL(DVF_CODES);
                VF_NEED(2u);
                VF_TAKE(rep, 2u);
                rep += 3u;
                val = prev;
            } else if (s == 17) {
                VF_NEED(3u);
                VF_TAKE(rep, 3u);
                rep += 3u;
                val = 0;
            } else if (s == 18) {
                VF_NEED(7u);
                VF_TAKE(rep, 7u);
                rep += 11u;
                val = 0;
            }
            if (INF_HDR_REP_OVERRUN(have, rep, total))
                VF_FAIL(DVF_CODES);
            ON_LANE0
            {
                for (uint32_t k = 0; k < rep; k++)
                    lds->lens[have + k] = (uint8_t)val;
            }
            have += rep;
            prev = val;
            if (VF_USED > limit)
                VF_FAIL(DVF_BIT_END);
        }
        WAVE_SYNC();
        if (INF_HDR_EOB_BAD(UNI(lds->lens[256])))
            VF_FAIL(DVF_CODES);
        if (inf_build(&lds->lit, lds->lens, (int)nlen, 1))
            VF_FAIL(DVF_CODES);
        if (inf_build(&lds->dist, lds->lens + nlen, (int)ndist, 2))
            VF_FAIL(DVF_CODES);
    }
    VF_LOAD_FC(&lds->lit, fc_l);
    VF_LOAD_FC(&lds->dist, fc_d);

    /* the input passes through the lanes too: 4 * WAVE bytes from in_chunk on */
    LANEVAR(uint32_t, inw);
    FOR_LANES { LV(inw) = 0; }
    uint32_t in_chunk = 0xffffffffu; /* (none yet) */
    for (;;) {
        int s;
        VF_DECODE(&lds->lit, fc_l, s);
        if (s < 0)
            VF_FAIL(DVF_LENGTH);
        if (s < 256) {
            if (p >= pend)
                VF_FAIL(DVF_LENGTH);
            if (p < in_chunk || p - in_chunk >= 4u * WAVE) {
                in_chunk = p & ~3u;
                FOR_LANES { LV(inw) = dvf_dword(in, in_chunk + 4u * (uint32_t)LANE, in_n); }
            }
            const uint32_t have = ((uint32_t)READLANE(inw, (p - in_chunk) >> 2) >> (8u * (p & 3u))) & 0xffu;
            if (have != (uint32_t)s)
                VF_FAIL(DVF_LITERAL);
            p++;
        } else if (s == 256) {
            break;
        } else {
            const uint32_t lc = (uint32_t)s - 257u;
            if (lc > 28u)
                VF_FAIL(DVF_LENGTH);
            /* RFC 1951 section 3.2.5, as formulas */
            const uint32_t lx = lc < 8u || lc == 28u ? 0u : (lc >> 2) - 1u;
            uint32_t len = lc == 28u ? 258u : lc < 8u ? 3u + lc : 3u + ((4u + (lc & 3u)) << lx);
            VF_TAKE(v, lx); /* (VF_DECODE left 17 bits at least) */
            len += v;
            int d;
            VF_DECODE(&lds->dist, fc_d, d);
            if (d < 0 || d > 29)
                VF_FAIL(DVF_LENGTH);
            const uint32_t dx = d < 4 ? 0u : ((uint32_t)d >> 1) - 1u;
            uint32_t dist = d < 4 ? 1u + (uint32_t)d : 1u + ((2u + ((uint32_t)d & 1u)) << dx);
            VF_TAKE(v, dx);
            dist += v;
            if (dist > p || dist > wsize)
                VF_FAIL(DVF_DISTANCE);
            if (len > pend - p)
                VF_FAIL(DVF_LENGTH);
            for (uint32_t i = 0; i < len; i += 4u * WAVE) {
                LANEVAR(int, bad);
                FOR_LANES
                {
                    const uint32_t k = i + 4u * (uint32_t)LANE;
                    LV(bad) = k < len && dvf_dword(in, p + k, p + len) != dvf_dword(in, p + k - dist, p + len - dist);
                }
                if (BALLOT(bad) != 0)
                    VF_FAIL(DVF_MATCH);
            }
            p += len;
        }
        if (VF_USED > limit)
            VF_FAIL(DVF_BIT_END);
    }
    if (p != pend)
        VF_FAIL(DVF_LENGTH);
    uint64_t end = VF_USED;
    if (last) { /* bi_windup: zeros up to the byte boundary */
        const uint32_t padn = (8u - (uint32_t)(end & 7u)) & 7u;
        VF_NEED(8u);
        VF_TAKE(v, padn);
        if (v != 0u)
            VF_FAIL(DVF_BIT_END);
        end += padn;
    }
    if (end != end_bit)
        VF_FAIL(DVF_BIT_END);
    *in_pos = p;
    return DVF_OK;
}

#undef VF_PULL
#undef VF_NEED
#undef VF_TAKE
#undef VF_USED
#undef VF_FAIL
#undef VF_LOAD_FC
#undef VF_DECODE

DEV uint32_t dvf_header_bytes(uint32_t wrap)
{
    return wrap == 1u ? 2u : wrap == 2u ? 10u : 0u;
}
DEV uint32_t dvf_trailer_bytes(uint32_t wrap)
{
    return wrap == 1u ? 4u : wrap == 2u ? 8u : 0u;
}

/* blocks: kept block j of one buffer (one wave); in / src: the buffer's input and stream, facts / verd: its
 * first kept block, n: how many it has, out_len: the stream's length by the plan's result */
DEV void dvf_block_item(const uint8_t *in, const uint8_t *src, const DvfBuf *buf, const DvfBlock *facts, uint32_t n,
                        uint32_t j, uint32_t out_len, uint32_t wrap, uint32_t wbits, DvfLds *lds, DvfVerdict *verd)
{
    const uint32_t trl = dvf_trailer_bytes(wrap);
    const DvfBlock blk = facts[j];
    /* (an out_len the stream's room cannot hold is the finisher's to report: no block ends there) */
    const uint64_t end_bit = j + 1u < n ? facts[j + 1u].bit_off : out_len >= trl ? 8ull * (out_len - trl) : 0ull;
    uint32_t in_pos = blk.in_begin;
    const uint32_t reason = dvf_check_block(in, buf->in_len, src, buf->out_cap, blk, end_bit, 1u << wbits, lds, &in_pos);
    uint32_t ck = 0;
    if (wrap != 0u && blk.in_begin <= buf->in_len && blk.in_len <= buf->in_len - blk.in_begin) {
        WAVE_SYNC();
        ck = wrap == 2u ? ck_crc32(in + blk.in_begin, blk.in_len, &lds->ck) : ck_adler32(in + blk.in_begin, blk.in_len);
    }
    ON_LANE0
    {
        DvfVerdict r;
        r.reason = reason;
        r.in_pos = in_pos;
        r.ck = ck;
        r.pad = 0;
        verd[j] = r;
    }
}

/* finish: one buffer (one thread); src: its stream; facts / verd: its first kept block */
DEV void dvf_finish(const uint8_t *src, const DvfBuf *buf, const DvfBlock *facts, const DvfVerdict *verd, uint32_t n,
                    const ZdResult *res, uint32_t wrap, uint32_t wbits, uint32_t level, uint32_t strategy,
                    DvfResult *out)
{
    DvfResult r;
    r.verdict = DVF_OK;
    r.block = DVF_NONE;
    r.bit_off = 0;
    r.in_pos = 0;
    if (res->status != 0) {
        r.verdict = DVF_SKIPPED;
        *out = r;
        return;
    }
    const uint32_t hdr = dvf_header_bytes(wrap), trl = dvf_trailer_bytes(wrap);
    /* the lowest-numbered block that failed its check or does not follow the one before it */
    uint32_t expect = 0, ck = wrap == 1u ? 1u : 0u;
    for (uint32_t i = 0; i < n; i++) {
        const DvfBlock b = facts[i];
        uint32_t reason = verd[i].reason, in_pos = verd[i].in_pos;
        if (reason == DVF_OK && b.in_begin != expect) {
            reason = DVF_LENGTH;
            in_pos = expect;
        }
        if (reason == DVF_OK && (b.type_last >> 8) != (i + 1u == n ? 1u : 0u))
            reason = DVF_BLOCK_HDR;
        if (reason != DVF_OK) {
            r.verdict = (int32_t)reason;
            r.block = i;
            r.bit_off = b.bit_off;
            r.in_pos = in_pos;
            *out = r;
            return;
        }
        expect += b.in_len;
        if (wrap == 2u)
            ck = sec_crc32_combine(ck, verd[i].ck, b.in_len);
        else if (wrap == 1u)
            ck = sec_adler32_combine(ck, verd[i].ck, b.in_len);
    }
    if (n == 0u || expect != buf->in_len) { /* the blocks end before the input does */
        r.verdict = DVF_LENGTH;
        r.block = n ? n - 1u : DVF_NONE;
        r.bit_off = n ? facts[n - 1u].bit_off : 0u;
        r.in_pos = expect;
        *out = r;
        return;
    }
    const uint32_t out_len = res->out_len;
    if (out_len > buf->out_cap || out_len < hdr + trl) {
        r.verdict = DVF_TRAILER;
        *out = r;
        return;
    }
    /* the header the plan writes (bit_emit.h layout_buffer; reference src/deflate.c:1031-1049, 1068-1082) */
    uint8_t want[10];
    if (wrap == 1u) {
        uint32_t h = (8u + ((wbits - 8u) << 4)) << 8;
        h |= ((strategy >= 2u || level < 2u) ? 0u : level < 6u ? 1u : level == 6u ? 2u : 3u) << 6;
        h += 31u - h % 31u;
        want[0] = (uint8_t)(h >> 8);
        want[1] = (uint8_t)h;
    } else if (wrap == 2u) {
        want[0] = 31;
        want[1] = 139;
        want[2] = 8;
        want[3] = want[4] = want[5] = want[6] = want[7] = 0;
        want[8] = level == 9u ? 2 : (strategy >= 2u || level < 2u) ? 4 : 0;
        want[9] = 3;
    }
    int bad = facts[0].bit_off != 8u * hdr;
    for (uint32_t k = 0; k < hdr; k++)
        bad |= src[k] != want[k];
    if (bad) {
        r.verdict = DVF_HEADER;
        *out = r;
        return;
    }
    const uint8_t *t = src + (out_len - trl);
    if (wrap == 1u) {
        const uint32_t got = (uint32_t)t[0] << 24 | (uint32_t)t[1] << 16 | (uint32_t)t[2] << 8 | t[3];
        bad = got != ck;
    } else if (wrap == 2u) {
        uint32_t got = 0, isize = 0;
        for (uint32_t k = 0; k < 4u; k++) {
            got |= (uint32_t)t[k] << (8u * k);
            isize |= (uint32_t)t[4u + k] << (8u * k);
        }
        bad = got != ck || isize != buf->in_len;
    }
    if (bad)
        r.verdict = DVF_TRAILER;
    *out = r;
}

#endif
