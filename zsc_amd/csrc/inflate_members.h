/*
 * inflate_members.h -- kernel 12: multi-member gzip files inflated member by member, in parallel
 * (DESIGN.md section 16).
 *
 * A file is a run of gzip members, each with its own header, CRC-32 and ISIZE, each decodable without
 * the others.  What the plan reports for a file is the result of this walk (include/zsc_hip.h): decode
 * the member at `at` as the plain plan decodes a stream, with the capacity that is left; stop at the
 * first member that is not Z_OK, or when fewer than two bytes remain or they are not 1f 8b.  The steps,
 * each a launch of its own, built on the sections plan's parts (inflate_sections.h: IsecPlan, IsecStream,
 * sec_setup, sec_next_unit, sec_find, the pool and the work bound):
 *   1. scan     every file's bytes for 1f 8b 08 with the reserved FLG bits clear, one wavefront per
 *               64 * WAVE bytes (the sections scan over another pattern; twice: count, then write);
 *               offset 0 is always candidate 0, and every file with a byte in it takes part;
 *   2. setup    sec_setup as it is;
 *   3. claims   one candidate per lane: a header whose FEXTRA holds a `B` `C` subfield of length 2 says
 *               how long the member is (BSIZE + 1, the BGZF convention), and the ISIZE at that end how
 *               long its output.  Such a candidate is claimed: the count pass does not decode it;
 *   4. count    every other candidate decoded by one group as one whole gzip member with nothing stored
 *               (the size decode): status, output length, where it stopped.  A clean Z_OK links to the
 *               candidate at its stop, or to "end" where the walk's stop rule holds;
 *   5. resolve  per file: the chain from candidate 0 while the members are Z_OK or claimed, linked and
 *               inside dest_caps; output offsets by a running sum;
 *   6. write    every member of every chain decoded by the plain decode (inflate_stream<0>) into its
 *               place with capacity = its counted or claimed length: it must come back Z_OK with exactly
 *               that length and that consumed count;
 *   7. finish   per file: the verified prefix -- the chain entries before the first write that disagreed.
 *               Where it reaches the chain's clean end the file is finished; otherwise where it ends
 *               (input offset, output offset, members) is kept;
 *   8. serial   one group per unfinished file goes on with the walk from the end of its verified prefix.
 *
 * Why a verified prefix is sound: a member of the walk depends on two things only, where it starts and
 * how much capacity is left.  By induction over the prefix, entry j starts where the walk's member j
 * starts (entry 0 at byte 0, entry j + 1 at the consumed count the plain decode of entry j gave), and it
 * was decoded by the walk's own decoder with a capacity (its length) that the walk's capacity (what is
 * left of dest_caps, at least that length by the resolve step's sum) changes nothing about for a member
 * that ends Z_OK.  So the prefix is the walk's first members with the walk's bytes, and the walk from its
 * end is the rest of the walk.
 *
 * A claim is never trusted: it only saves the count pass's decode.  The write pass decodes a claimed member
 * like any other, into a slice of exactly the claimed length, so a false claim cannot write outside its
 * slice, and it must reproduce the claimed length and end exactly (the CRC-32 and ISIZE are the decode's
 * own checks); one that does not ends the verified prefix in front of it.
 *
 * Size-only mode (no write pass, nothing stored): every member follows the size plan's contract
 * (inflate_size.h), so the check value is not compared.  Claims are not used there -- there is no write
 * pass to verify them, and a length nobody decoded is not a size: every member is decoded once, by the count
 * pass, and the chain is its own verification.
 */
#ifndef ZSC_INFLATE_MEMBERS_H
#define ZSC_INFLATE_MEMBERS_H

#include "inflate_sections.h"

#define MEM_CAND_DIV 16u         /* candidates a file may have: source_len / 16 + 8 (a member has 20 bytes or more) */
#define MEM_LINK_END SEC_LINK_FIN /* link of a candidate: the walk ends behind it */
#define MEM_CLAIMED (1u << 28)   /* flags of a candidate, above its link: stop and length come from its header */
#define MEM_OK (1u << 29)        /* ... it decoded as a clean Z_OK member */
#define MEM_LINK(v) ((v) & 0x0fffffffu)
#define MEM_CLAIM_MAX_ISIZE 65536u

/* where the serial step takes a file up, and what is reported of it (zeroed before every run) */
typedef struct {
    uint32_t at, out; /* the end of the verified prefix: input and output offset */
    uint32_t members; /* members of the walk that were Z_OK */
    uint32_t claimed; /* members of the verified prefix that were claimed */
} MemFile;

typedef struct {
    IsecPlan sp;
    MemFile *mf;
    uint32_t size_only; /* nothing stored, no write pass */
    uint32_t claims;    /* step 3 looks at the headers */
} MemPlan;

/* the scan's pattern: 1f 8b 08 and a FLG byte with bits 5-7 clear (a byte past the end reads as 0), anywhere
 * but at offset 0, which is candidate 0 without being looked at */
DEV bool mem_hit_magic(uint32_t v, uint32_t p, uint32_t n)
{
    return (v & 0xe0ffffffu) == 0x00088b1fu && p != 0u && p + 3u <= n;
}

DEV void mem_scan_tile(const MemPlan &M, const uint8_t *src_all, uint32_t t, int write)
{
    sec_scan_tile_for<mem_hit_magic, 0u, true>(M.sp, src_all, t, write);
}

/* the walk's stop rule at input offset `at` (<= n) of a file */
DEV uint32_t mem_at_end(const uint8_t *src, uint32_t n, uint32_t at)
{
    return n - at < 2u || src[at] != 0x1fu || src[at + 1u] != 0x8bu;
}

/* the link of a member that stopped at `stop` */
DEV uint32_t mem_link(const uint32_t *cstart, uint32_t ncand, const uint8_t *src, uint32_t n, uint32_t stop)
{
    return mem_at_end(src, n, stop) ? MEM_LINK_END : sec_find(cstart, ncand, stop);
}

/* what the header at `start` claims: 1 with the member's end and output length if FEXTRA holds a `B` `C`
 * subfield of length 2 (BSIZE = the member's length - 1), the member lies inside the file with room for the
 * extra field and a trailer, and the ISIZE at its end is at most 64 KiB */
DEV uint32_t mem_claim(const uint8_t *src, uint32_t n, uint32_t start, uint32_t *stop, uint32_t *len)
{
    if (n - start < 12u + 8u)
        return 0;
    const uint8_t *b = src + start;
    if (b[0] != 0x1fu || b[1] != 0x8bu || b[2] != 8u || (b[3] & 0xe4u) != 4u)
        return 0;
    const uint32_t end = 12u + ((uint32_t)b[10] | (uint32_t)b[11] << 8);
    if (end > n - start)
        return 0;
    for (uint32_t p = 12u; p + 4u <= end;) {
        const uint32_t slen = (uint32_t)b[p + 2u] | (uint32_t)b[p + 3u] << 8;
        if (slen > end - p - 4u)
            return 0;
        if (b[p] == 'B' && b[p + 1u] == 'C' && slen == 2u) {
            const uint32_t total = ((uint32_t)b[p + 4u] | (uint32_t)b[p + 5u] << 8) + 1u;
            if (total < end + 8u || total > n - start)
                return 0;
            const uint8_t *z = b + total - 4u;
            const uint32_t isize = (uint32_t)z[0] | (uint32_t)z[1] << 8 | (uint32_t)z[2] << 16 | (uint32_t)z[3] << 24;
            if (isize > MEM_CLAIM_MAX_ISIZE)
                return 0;
            *stop = start + total;
            *len = isize;
            return 1;
        }
        p += 4u + slen;
    }
    return 0;
}

/* step 3 for the a-th active file (whole-wave code): every candidate's flags start here, claimed or 0 */
DEV void mem_claims(const MemPlan &M, const uint8_t *src_all, uint32_t a)
{
    const IsecPlan &P = M.sp;
    const uint32_t s = UNI(P.active[a]);
    const uint32_t ncand = UNI(P.st[s].ncand), cb = UNI(P.st[s].base);
    const uint8_t *src = src_all + P.items[s].src_off;
    const uint32_t n = UNI(P.items[s].src_len);
    const uint32_t on = M.claims && !M.size_only;
    for (uint32_t k0 = 0; k0 < ncand; k0 += WAVE) {
        FOR_LANES
        {
            const uint32_t k = k0 + (uint32_t)LANE;
            if (k < ncand) {
                uint32_t stop = 0, len = 0, link = 0;
                if (on && mem_claim(src, n, P.cstart[cb + k], &stop, &len)) {
                    link = MEM_CLAIMED | mem_link(P.cstart + cb, ncand, src, n, stop);
                    P.cstop[cb + k] = stop;
                    P.clen[cb + k] = len;
                }
                P.clink[cb + k] = link;
            }
        }
    }
}

/* ---- group code (INF_GROUP lanes per unit, as the decoder) ---- */
#undef ZSC_GROUP
#define ZSC_GROUP INF_GROUP
#include "wave_group.h"

DEV void mem_resume_clear(InfResume *rs)
{
    ON_GLANE0 { rs->state = rs->out_pos = rs->errors = rs->gzip = rs->sy_lo = rs->sy_hi = rs->sy_rb = 0; }
    WAVE_SYNC();
}

/* step 4: a group decodes unclaimed candidates until the queue is empty; r and rs are the group's own */
DEV void mem_count_worker(const MemPlan &M, const uint8_t *src_all, InfLds *lds, InfResult *r, InfResume *rs)
{
    const IsecPlan &P = M.sp;
    uint32_t s, k;
    while (sec_next_unit<1>(P, &s, &k)) {
        IsecStream *S = &P.st[s];
        const IsecItem *it = &P.items[s];
        const uint32_t n = GUNI(it->src_len);
        if (GUNI(S->serial))
            continue;
        const uint32_t cb = GUNI(S->base);
        if (GUNI(P.clink[cb + k]) & MEM_CLAIMED)
            continue;
        if ((unsigned long long)SEC_LOAD(&S->work) > (unsigned long long)P.work_mul * n + P.work_add) {
            ON_GLANE0 { SEC_OR(&S->serial, 1u); }
            continue;
        }
        const uint32_t start = GUNI(P.cstart[cb + k]);
        const uint8_t *src = src_all + it->src_off;
        mem_resume_clear(rs);
        InfJob job;
        job.src = src + start;
        job.n = n - start;
        job.dst = nullptr;
        job.cap = GUNI(it->dst_cap);
        job.window_bits = P.window_bits;
        const int again = inflate_stream<INF_SEC_SIZE | INF_SEC_COUNT>(job, lds, r, rs);
        WAVE_SYNC();
        const uint32_t ok = !again && GUNI(r->status) == 0;
        ON_GLANE0
        {
            /* (a data error leaves no consumed count: the bits the reference had read by then) */
            const uint32_t used = again ? (uint32_t)((((uint64_t)rs->sy_hi << 32) | rs->sy_lo) >> 3) : r->consumed;
            const uint32_t stop = start + (used < n - start ? used : n - start);
            P.clink[cb + k] = ok ? MEM_OK | mem_link(P.cstart + cb, S->ncand, src, n, stop) : SEC_LINK_NIL;
            P.clen[cb + k] = ok ? r->out_len : 0u;
            P.cstop[cb + k] = stop;
            SEC_ADD(&S->work, (unsigned long long)(stop - start));
        }
        WAVE_SYNC();
    }
}

/* step 5 for the a-th active file: the chain from candidate 0, GRP links read at a time.  S->head: the chain
 * reached a clean end; S->total, S->trailer: the output and input offset behind its last member */
DEV void mem_resolve(const MemPlan &M, uint32_t a)
{
    const IsecPlan &P = M.sp;
    const uint32_t s = GUNI(P.active[a]);
    IsecStream *S = &P.st[s];
    const uint32_t ncand = GUNI(S->ncand);
    if (ncand == 0u || GUNI(S->serial))
        return;
    const uint32_t cb = GUNI(S->base), cap = GUNI(P.items[s].dst_cap);
    LANEVAR(uint32_t, lk);
    LANEVAR(uint32_t, ln);
    LANEVAR(uint32_t, sp);
    uint32_t k = 0, wbase = 0, j = 0, clean = 0, at = 0;
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
                LV(sp) = i < ncand ? P.cstop[cb + i] : 0u;
            }
        }
        const uint32_t link = GREADLANE(lk, k - wbase), len = GREADLANE(ln, k - wbase);
        if (!(link & (MEM_OK | MEM_CLAIMED)) || sum + len > cap)
            break;
        ON_GLANE0
        {
            P.chain_k[cb + j] = k;
            P.chain_off[cb + j] = (uint32_t)sum;
        }
        sum += len;
        at = GREADLANE(sp, k - wbase);
        j++;
        const uint32_t nx = MEM_LINK(link);
        if (nx == MEM_LINK_END) {
            clean = 1;
            break;
        }
        if (nx == SEC_LINK_NIL || nx <= k || nx >= ncand)
            break;
        k = nx;
    }
    ON_GLANE0
    {
        S->nchain = j;
        S->head = clean;
        S->total = (uint32_t)sum;
        S->trailer = at;
    }
    WAVE_SYNC();
}

/* step 6: a group decodes chained members into place until the queue is empty; chain_ck[j]: the plain decode
 * gave what the chain says */
DEV void mem_write_worker(const MemPlan &M, const uint8_t *src_all, uint8_t *dst_all, InfLds *lds, InfResult *r,
                          InfResume *rs)
{
    const IsecPlan &P = M.sp;
    uint32_t s, j;
    while (sec_next_unit<2>(P, &s, &j)) {
        IsecStream *S = &P.st[s];
        const IsecItem *it = &P.items[s];
        const uint32_t cb = GUNI(S->base);
        const uint32_t k = GUNI(P.chain_k[cb + j]), off = GUNI(P.chain_off[cb + j]);
        const uint32_t start = GUNI(P.cstart[cb + k]), len = GUNI(P.clen[cb + k]);
        mem_resume_clear(rs);
        InfJob job;
        job.src = src_all + it->src_off + start;
        job.n = GUNI(it->src_len) - start;
        job.dst = dst_all + it->dst_off + off;
        job.cap = len;
        job.window_bits = P.window_bits;
        const int again = inflate_stream<0>(job, lds, r, rs);
        WAVE_SYNC();
        const uint32_t same = !again && GUNI(r->status) == 0 && GUNI(r->out_len) == len &&
                              start + GUNI(r->consumed) == GUNI(P.cstop[cb + k]);
        ON_GLANE0 { P.chain_ck[cb + j] = same; }
        WAVE_SYNC();
    }
}

/* step 7 for the a-th active file */
DEV void mem_finish(const MemPlan &M, InfResult *res, InfResume *resume, uint32_t a)
{
    const IsecPlan &P = M.sp;
    const uint32_t s = GUNI(P.active[a]);
    IsecStream *S = &P.st[s];
    if (GUNI(S->ncand) == 0u || GUNI(S->serial))
        return;
    const uint32_t cb = GUNI(S->base), nchain = GUNI(S->nchain);
    /* the first entry whose write disagreed: every lane looks at its share, the smallest wins */
    LANEVAR(uint32_t, first);
    FOR_GLANES
    {
        uint32_t f = nchain;
        if (!M.size_only)
            for (uint32_t j = (uint32_t)GLANE; j < nchain; j += GRP)
                if (!P.chain_ck[cb + j]) {
                    f = j;
                    break;
                }
        LV(first) = f;
    }
    const uint32_t prefix = GMIN_U32(first);
    LANEVAR(uint64_t, cl);
    FOR_GLANES
    {
        uint32_t c = 0;
        for (uint32_t j = (uint32_t)GLANE; j < prefix; j += GRP)
            c += (P.clink[cb + P.chain_k[cb + j]] & MEM_CLAIMED) != 0u;
        LV(cl) = c;
    }
    const uint32_t claimed = (uint32_t)GSUM64(cl);
    const uint32_t whole = prefix == nchain;
    const uint32_t at = whole ? GUNI(S->trailer) : GUNI(P.cstart[cb + GUNI(P.chain_k[cb + prefix])]);
    const uint32_t out = whole ? GUNI(S->total) : GUNI(P.chain_off[cb + prefix]);
    ON_GLANE0
    {
        MemFile *F = &M.mf[s];
        F->at = at;
        F->out = out;
        F->members = prefix;
        F->claimed = claimed;
        P.nsec[s] = prefix;
        if (whole && S->head) {
            res[s].status = 0;
            res[s].out_len = out;
            res[s].consumed = at;
            res[s].pad = 0;
            resume[s].state = 2;
        }
    }
    WAVE_SYNC();
}

/* step 8 for file s, if it is not finished: the walk from the end of its verified prefix, member by member
 * with the plain decode (SIZE: the size decode), each entered again after every recovered data error as the
 * plain plan's relaunches do (the member that needs it is the file's last); r and rs are the group's own */
template <bool SIZE>
DEV void mem_serial(const MemPlan &M, const uint8_t *src_all, uint8_t *dst_all, InfLds *lds, InfResult *r,
                    InfResume *rs, InfResult *res, InfResume *resume, uint32_t s)
{
    const IsecPlan &P = M.sp;
    if (GUNI(resume[s].state) == 2u)
        return;
    const IsecItem *it = &P.items[s];
    const uint8_t *src = src_all + it->src_off;
    const uint32_t n = GUNI(it->src_len), cap = GUNI(it->dst_cap);
    uint32_t at = GUNI(M.mf[s].at), out = GUNI(M.mf[s].out), members = GUNI(M.mf[s].members);
    int32_t status;
    for (;;) {
        mem_resume_clear(rs);
        InfJob job;
        job.src = src + at;
        job.n = n - at;
        job.dst = SIZE ? nullptr : dst_all + it->dst_off + out;
        job.cap = cap - out;
        job.window_bits = P.window_bits;
        for (uint32_t round = 0; round < job.n / 4u + 2u; round++) {
            int again;
            if constexpr (SIZE)
                again = inflate_stream<INF_SEC_SIZE | INF_SEC_COUNT>(job, lds, r, rs);
            else
                again = inflate_stream<0>(job, lds, r, rs);
            WAVE_SYNC();
            if (!again)
                break;
        }
        status = (int32_t)GUNI(r->status);
        out += GUNI(r->out_len);
        at += GUNI(r->consumed);
        if (status != 0)
            break;
        members++;
        if (mem_at_end(src, n, at))
            break;
    }
    ON_GLANE0
    {
        res[s].status = status;
        res[s].out_len = out;
        res[s].consumed = at;
        res[s].pad = r->pad;
        resume[s] = *rs;
        M.mf[s].members = members;
    }
    WAVE_SYNC();
}

/* back to whole-wave groups for whatever is compiled after this */
#undef ZSC_GROUP
#define ZSC_GROUP 64
#include "wave_group.h"

#endif
