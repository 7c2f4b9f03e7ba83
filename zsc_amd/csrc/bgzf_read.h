/*
 * bgzf_read.h -- kernel 14: ranges read out of BGZF files from a member index.
 *
 * The INDEX of a file is the table of this walk, which decodes nothing:
 *     at = 0; out = 0; k = 0
 *     while mem_claim(file, n, at) holds:  coffset[k] = at; uoffset[k] = out; k += 1
 *                                          at = claim.stop; out += claim.len
 *     coffset[k] = at; uoffset[k] = out                       (the end entry)
 * It is built from the members plan's steps 1-3 as they are (inflate_members.h: the scan for 1f 8b 08, sec_setup,
 * one claim per lane, each with the link to the candidate at its end) and bgi_chain below: the claimed links
 * followed from candidate 0, GRP of them a load, with the running sum of the claimed lengths.  A candidate off
 * that chain -- a BGZF file stored inside a member -- is never looked at.  A file with more candidates than the
 * members plan gives it room for is walked header by header instead (bgi_walk), which is the definition itself.
 *
 * The index is a set of CLAIMS (a BSIZE field and the ISIZE in front of the end it names).  A RANGES plan
 * verifies what it uses: the host cuts every request into one job per member that contributes a byte, and a
 * lane group that takes a job from the queue first evaluates mem_claim at the member's start again -- it must
 * give the index's end and length -- then decodes the member with the plain decode (inflate_stream<0>) with
 * capacity = the member's length, which must come back Z_OK with exactly that length and that consumed count
 * (CRC-32 and ISIZE are the decode's own checks).  A member the range covers whole (an INTERIOR job) is decoded
 * straight into its place.  Of any other (an EDGE job; a range has two at the most) the whole member goes into
 * the lane group's staging slot -- matches reach back into earlier output, so a clipped head cannot be left
 * undecoded -- and the group copies the slice out.  The member is decoded at the offset inside the slot that
 * gives the slice the destination's alignment, so the copy moves whole 16-byte granules between a byte-wise head
 * and tail.  Staging is a slot per lane group of the launch, whatever the number of requests.  A job that is
 * not good marks its request; bgr_finish reports per request what create worked out, or Z_DATA_ERROR.
 *
 * Coordinates are the index's: a member whose ISIZE field was altered shifts everything behind it, here as in
 * every BGZF reader (and that member fails its own decode).
 */
#ifndef ZSC_BGZF_READ_H
#define ZSC_BGZF_READ_H

#include "inflate_members.h"

#define BGR_MAX_MEMBER 65536u            /* a claimed length at the most (MEM_CLAIM_MAX_ISIZE) */
#define BGR_SLOT (BGR_MAX_MEMBER + 16u)  /* bytes of a lane group's staging slot: a member at an offset of 0..15 */
#define BGI_MIN_MEMBER 26u               /* bytes of the shortest member mem_claim accepts */
/* entries a file's table may need: a member per BGI_MIN_MEMBER bytes, and the end entry */
#define BGI_TABLE_CAP(n) ((uint64_t)(n) / BGI_MIN_MEMBER + 2u)

/* one member of one request (host-built, read-only) */
typedef struct {
    uint64_t dst;             /* where the slice goes, from the destination's base */
    uint32_t file, req;
    uint32_t start, stop, len; /* the index's member: where it starts and ends in the file, its output length */
    uint32_t clip0, clip1;    /* bytes [clip0, clip1) of its output are the slice */
    uint32_t pad;
} BgrJob;

typedef struct {
    uint64_t src_off;
    uint32_t src_len, pad;
} BgrFile;

typedef struct {
    const BgrFile *files;
    const BgrJob *jobs; /* longest member first */
    uint32_t *bad;      /* per request: a job of it was not good (zeroed before every run) */
    uint32_t *q;        /* [0] the job queue (zeroed before every run) */
    uint32_t njobs, count;
} BgrPlan;

/* ---- group code (INF_GROUP lanes per unit, as the decoder) ---- */
#undef ZSC_GROUP
#define ZSC_GROUP INF_GROUP
#include "wave_group.h"

/* the walk itself from input offset `at` with `sum` bytes out in front of it, header by header: coff / uoff take
 * the entries (tcap of them at the most, the end entry included), *members their count without the end entry */
DEV void bgi_walk(const uint8_t *src, uint32_t n, uint32_t at, uint64_t sum, uint64_t *coff, uint64_t *uoff,
                  uint64_t tcap, uint32_t *members)
{
    uint32_t j = 0;
    while ((uint64_t)j + 2u <= tcap && at < n) {
        uint32_t stop = 0, len = 0;
        if (!mem_claim(src, n, at, &stop, &len))
            break;
        ON_GLANE0
        {
            coff[j] = at;
            uoff[j] = sum;
        }
        j++;
        at = stop;
        sum += len;
    }
    ON_GLANE0
    {
        coff[j] = at;
        uoff[j] = sum;
        *members = j;
    }
}

/* the index of file s of the members plan's view M, after its claims step.  A file of no bytes has no stream
 * record, and one with more candidates than it has room for has no candidates: both are walked. */
DEV void bgi_chain(const MemPlan &M, const uint8_t *src_all, uint32_t s, uint64_t *coff, uint64_t *uoff, uint64_t tcap,
                   uint32_t *members)
{
    const IsecPlan &P = M.sp;
    const uint32_t n = GUNI(P.items[s].src_len);
    const IsecStream *S = &P.st[s];
    if (n == 0u || GUNI(S->serial) || GUNI(S->ncand) == 0u) {
        bgi_walk(src_all + P.items[s].src_off, n, 0u, 0u, coff, uoff, tcap, members);
        return;
    }
    const uint32_t ncand = GUNI(S->ncand), cb = GUNI(S->base);
    LANEVAR(uint32_t, lk);
    LANEVAR(uint32_t, ln);
    LANEVAR(uint32_t, sp);
    uint32_t k = 0, wbase = 0, j = 0, at = 0;
    uint64_t sum = 0;
    int loaded = 0;
    while ((uint64_t)j + 2u <= tcap) {
        if (!loaded || k - wbase >= GRP) {
            wbase = k;
            loaded = 1;
            FOR_GLANES
            {
                const uint32_t i = wbase + (uint32_t)GLANE;
                LV(lk) = i < ncand ? P.clink[cb + i] : 0u;
                LV(ln) = i < ncand ? P.clen[cb + i] : 0u;
                LV(sp) = i < ncand ? P.cstop[cb + i] : 0u;
            }
        }
        const uint32_t link = GREADLANE(lk, k - wbase);
        if (!(link & MEM_CLAIMED))
            break;
        /* (candidate k starts at `at`: candidate 0 at byte 0, and a link names the candidate at the stop) */
        ON_GLANE0
        {
            coff[j] = at;
            uoff[j] = sum;
        }
        sum += GREADLANE(ln, k - wbase);
        at = GREADLANE(sp, k - wbase);
        j++;
        const uint32_t nx = MEM_LINK(link);
        if (nx == MEM_LINK_END || nx == SEC_LINK_NIL || nx <= k || nx >= ncand)
            break;
        k = nx;
    }
    ON_GLANE0
    {
        coff[j] = at;
        uoff[j] = sum;
        *members = j;
    }
}

/* n bytes from s to d, which have the same alignment to 16: the group's lanes a granule each */
DEV void bgr_copy(uint8_t *d, const uint8_t *s, uint32_t n)
{
    const uint32_t mis = (uint32_t)((16u - ((uintptr_t)d & 15u)) & 15u);
    const uint32_t head = mis < n ? mis : n;
    const uint32_t body = (n - head) & ~15u;
    FOR_GLANES
    {
        for (uint32_t k = (uint32_t)GLANE; k < head; k += GRP)
            d[k] = s[k];
        for (uint32_t k = head + 16u * (uint32_t)GLANE; k < head + body; k += 16u * GRP)
            COPY16(d + k, s + k);
        for (uint32_t k = head + body + (uint32_t)GLANE; k < n; k += GRP)
            d[k] = s[k];
    }
}

/* a group takes jobs until the queue is empty; slot: its BGR_SLOT staging bytes (16-byte aligned); r and rs
 * are the group's own */
DEV void bgr_worker(const BgrPlan &B, const uint8_t *src_all, uint8_t *dst_all, uint8_t *slot, InfLds *lds,
                    InfResult *r, InfResume *rs)
{
    for (;;) {
        LANEVAR(uint32_t, take);
        FOR_GLANES { LV(take) = GLANE == 0 ? SEC_ADD(&B.q[0], 1u) : 0u; }
        const uint32_t j = GREADLANE(take, 0);
        if (j >= B.njobs)
            break;
        const BgrJob *J = &B.jobs[j];
        const BgrFile *F = &B.files[GUNI(J->file)];
        const uint8_t *src = src_all + F->src_off;
        const uint32_t n = GUNI(F->src_len), start = GUNI(J->start), len = GUNI(J->len);
        const uint32_t clip0 = GUNI(J->clip0), clip1 = GUNI(J->clip1);
        uint32_t stop = 0, claimed = 0;
        uint32_t good = start < n && mem_claim(src, n, start, &stop, &claimed) && stop == GUNI(J->stop) &&
                        claimed == len && len <= BGR_MAX_MEMBER && clip0 <= clip1 && clip1 <= len;
        if (good) {
            const uint32_t interior = clip0 == 0u && clip1 == len;
            uint8_t *out = dst_all + J->dst;
            uint8_t *to = interior ? out : slot + (((uintptr_t)out - clip0) & 15u);
            mem_resume_clear(rs);
            InfJob job;
            job.src = src + start;
            job.n = n - start;
            job.dst = to;
            job.cap = len;
            job.window_bits = 31;
            const int again = inflate_stream<0>(job, lds, r, rs);
            WAVE_SYNC();
            good = !again && GUNI(r->status) == 0 && GUNI(r->out_len) == len && start + GUNI(r->consumed) == stop;
            if (good && !interior)
                bgr_copy(out, to + clip0, clip1 - clip0);
        }
        if (!good) {
            ON_GLANE0 { SEC_OR(&B.bad[GUNI(J->req)], 1u); }
        }
        WAVE_SYNC();
    }
}

/* back to whole-wave groups for whatever is compiled after this */
#undef ZSC_GROUP
#define ZSC_GROUP 64
#include "wave_group.h"

/* ---- whole-wave code ---- */

/* Entries e0 .. e0 + WAVE - 1 of cnt member starts somebody else names (a .gzi file; entry 0 is byte 0), an entry
 * per lane: the header there must claim a member that ends at the next entry with the length the uncompressed
 * offsets differ by.  Behind the last entry the walk goes on by itself (bgi_walk), so the last named start need
 * only be one -- and entry 0, where it is the only one, need not: a file of no members has that table. */
DEV void bgi_verify(const uint8_t *src, uint32_t n, const uint64_t *coff, const uint64_t *uoff, uint32_t cnt,
                    uint32_t e0, uint32_t *bad)
{
    FOR_LANES
    {
        const uint32_t e = e0 + (uint32_t)LANE;
        if (e < cnt && cnt > 1u) {
            const uint64_t c = coff[e];
            uint32_t stop = 0, len = 0;
            uint32_t ok = c < n && mem_claim(src, n, (uint32_t)c, &stop, &len);
            if (ok && e + 1u < cnt)
                ok = coff[e + 1u] == stop && uoff[e + 1u] - uoff[e] == len;
            if (!ok)
                GLOBAL_OR_U32(bad, 1u);
        }
    }
}

/* request i: what create worked out (res0), or Z_DATA_ERROR with nothing where one of its jobs was not good */
DEV void bgr_finish(const BgrPlan &B, const InfResult *res0, InfResult *res, uint32_t i)
{
    InfResult v = res0[i];
    if (B.bad[i]) {
        v.status = -3;
        v.out_len = v.consumed = 0u;
    }
    res[i] = v;
}

#endif
