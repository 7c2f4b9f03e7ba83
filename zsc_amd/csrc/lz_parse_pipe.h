/*
 * lz_parse_pipe.h -- the segmented parser (lz_parse_seg.h) run as a pipeline of segments.
 *
 * The super-step schedule drives every SG_SPAN positions through three phases with a workgroup
 * barrier between them: one wave slides the window, all waves parse until the slowest segment is
 * done, one wave resolves (and every parser that gave up costs a round in which one wave parses).
 * None of that waiting is needed by the result: a speculative segment depends on window bytes only,
 * and only the resolver is ordered.  Here the segments of the whole buffer are numbered 0, 1, 2 ...,
 * segment g uses slot g % NSLOT of trace / tkind / wv and of the scratch, and the waves of the
 * workgroup never meet between the first and the last segment.  A wave takes the most urgent JOB whose
 * preconditions hold, runs it to the end without waiting for anybody inside it, and comes back:
 *
 *   redo     parse on from the exact state of a parser that gave up (or ran out of slots)
 *   resolve  follow the chain of hand-overs as far as complete segments allow, append their tokens,
 *            give the slots of the segments behind the chain back (trace cleared first)
 *   load     bring the next chunk of the input into the window ring
 *   parse    the next speculative segment, fresh at its first position, in ascending order
 *
 * Every job is claimed through one word in LDS (compare-and-swap), so any wave can do any job and a
 * single wave can do all of them: no job needs a second wave to make progress.  What a job leaves for
 * others is published with a workgroup-scope release (LDS_STORE_REL: the wave's stores to LDS and to
 * memory are complete before the word changes) and picked up with an acquire.
 *
 * The window.  The ring holds position x at x % RING.  A chunk [hi, hi + CHUNK) overwrites the bytes of
 * [hi - RING, hi + CHUNK - RING); the oldest byte any running or unresolved segment can still read is
 * one window before the first position of the oldest segment that has not given its slot back
 * (sg_pipe_floor).  sg_pipe_may_load is that invariant, stated once; the host emulation asserts the
 * same predicate on every ring read and every chunk load (tests/emu_pipe).  Segment g may start when
 * its slot is free (g < p_released + NSLOT) and the ring holds everything up to the end of what its
 * parser can touch (sg_pipe_want).  The mirror behind the ring's end is rewritten by the load of the
 * chunk at ring offset 0, whose bytes it repeats (lz_load_chunk): what it held before lies a whole ring
 * back and is covered by the same invariant.
 *
 * The geometry (ring, chunk, slots) belongs to the type L the schedule is instantiated with (lz_parse_seg.h):
 * SgLds, the super-steps' own (45 056 / 2 048 / 32: the slots bound what is in flight), and SgLdsNarrow
 * (37 888 / 512 / 18: the ring does, and four workgroups fit a CU).  Progress, with rel = p_released and the
 * numbers of SgLdsNarrow in brackets; every statement is about RING, CHUNK, NSLOT and holds for both:
 *   - The loader may bring hi up to RING + floor(rel), in whole chunks: RING + rel SG_G - ZD_TILE once the
 *     window moves, less at most CHUNK - SG_G for the rounding (>= rel SG_G + 4 864).  Segment g wants
 *     (g + 1) SG_G + SG_OV + 2 ZD_MIN_LOOKAHEAD (rel SG_G + 1 292 for g = rel): the oldest segment that has
 *     not given its slot back can always be handed out, parsed and parsed again with the ring at its limit,
 *     whatever the others do -- RING >= ZD_TILE + SG_G + SG_OV + 2 ZD_MIN_LOOKAHEAD + CHUNK is all it takes.
 *     Its reads go no further back than max_dist (and 15 bytes for the sweep's aligned reads) from a position
 *     at or above rel SG_G, above the floor, and no further ahead than what it wanted.  [g <= rel + 14: fifteen
 *     segments in flight, fourteen while rel is odd.  Before the window moves and once the whole input is
 *     loaded the ring holds nobody back and the slots do.]
 *   - A parser that runs past its segment looks for a hand-over in the two segments behind its own, as far as
 *     their slots hold their own traces or none (sg_pipe_limit: below rel + NSLOT, read anew at every step
 *     past the end).  Beyond that it ends as SG_EXIT_LAST and the segment it stands in is parsed again from
 *     its exact state: slower, never different.  [rel + 14 + 2 < rel + 18: while the ring is the bound no
 *     parser ends that way.]
 *   - A segment to be parsed again (p_redo) waits for the speculative parse of the same segment, which may
 *     wait for a slot or for the ring: the resolver gives slots back while the redo is pending (the loop
 *     at the top of sg_pipe_resolve runs before `held` is looked at), rel reaches the chain's segment or the
 *     first segment not handed out yet, and that one is the oldest unreleased segment of the first point.
 * SG_PIPE_MAX_IDLE below is the last line of defence behind this argument, not a part of it.
 */
#ifndef ZSC_LZ_PARSE_PIPE_H
#define ZSC_LZ_PARSE_PIPE_H

#include "lz_parse_seg.h"

#ifndef SG_PIPE_HOOK_LOAD
#define SG_PIPE_HOOK_LOAD(hi, released) /* host emulation: a chunk is about to be loaded at hi */
#endif

#define SG_PIPE_DONE 0
#define SG_PIPE_WORKED 1
#define SG_PIPE_IDLE 2

#define SG_JOB_REDO 1u
#define SG_JOB_RESOLVE 2u
#define SG_JOB_LOAD 4u
#define SG_JOB_PARSE 8u
#define SG_JOB_ALL 15u

#define SG_PIPE_NOXP 0xffffffffu

/* the oldest byte a running or unresolved segment can still read */
DEV uint32_t sg_pipe_floor(uint32_t released)
{
    const uint32_t a = released * SG_G;
    return a > ZD_TILE ? a - ZD_TILE : 0u;
}
/* may the chunk at hi be loaded?  Not before everything it overwrites lies below that byte. */
template <class L>
DEV bool sg_pipe_may_load(uint32_t hi, uint32_t released)
{
    return (uint64_t)hi + L::CHUNK <= (uint64_t)L::RING + sg_pipe_floor(released);
}
/* the ring must hold [.., this) before segment g is handed out: its parser runs at most SG_OV past the
 * segment's end and reads a lookahead and what the register caches fetch ahead beyond that */
DEV uint32_t sg_pipe_want(uint32_t g, uint32_t ntot)
{
    const uint64_t e = ((uint64_t)g + 1u) * SG_G + SG_OV + 2u * ZD_MIN_LOOKAHEAD;
    return e < ntot ? (uint32_t)e : ntot;
}
DEV uint32_t sg_pipe_nseg(uint32_t n)
{
    return n == 0 ? 1u : (uint32_t)(((uint64_t)n + SG_G - 1u) / SG_G); /* (the empty buffer: segment 0 reports the end) */
}

/* claim a word in LDS for this wave: true if it went from `from` to `to` */
DEV bool sg_pipe_claim(uint32_t *word, uint32_t from, uint32_t to)
{
    LANEVAR(uint32_t, got);
    FOR_LANES
    {
        LV(got) = 0;
        if (LANE == 0)
            LV(got) = LDS_CAS_U32(word, from, to);
    }
    return READLANE(got, 0) == from;
}

/* before the first segment (wave 0; the caller puts a barrier behind it) */
template <class L>
DEV void sg_pipe_init(L *lds, int w)
{
    sg_init(lds, w);
    if (w != 0)
        return;
    FOR_LANES
    {
        for (uint32_t i = (uint32_t)LANE; i < L::NSLOT * (SG_TRACE / 32); i += WAVE)
            (&lds->trace[0][0])[i] = 0;
        for (uint32_t i = (uint32_t)LANE; i < L::NSLOT; i += WAVE)
            lds->p_done[i] = 0;
    }
    ON_LANE0
    {
        lds->p_next = 0;
        lds->p_released = 0;
        lds->p_res_busy = lds->p_load_busy = 0;
        lds->p_redo = 0;
        lds->p_rs[0] = lds->p_rs[1] = lds->p_rs[2] = lds->p_rs[3] = 0;
        lds->p_chain_xp = SG_PIPE_NOXP;
        lds->p_stuck = 0;
    }
    WAVE_SYNC();
}

/* the resolver, by the wave that holds p_res_busy: as far as complete segments allow, then it yields */
template <class L>
DEV void sg_pipe_resolve(const LzJob &job, L *lds, const SgScratch &scr)
{
    if (UNI(LDS_LOAD_ACQ(&lds->finished)) != 0u)
        return;
    /* (while a segment waits to be parsed again the chain stands still, but slots still go back: the
     * segment in question may itself be waiting for one) */
    const bool held = UNI(LDS_LOAD_ACQ(&lds->p_redo)) != 0u;
    uint32_t k = UNI(lds->chain), ft = UNI(lds->chain_ft), cxp = UNI(lds->p_chain_xp);
    uint32_t rel = UNI(lds->p_released);
    for (;;) {
        /* slots behind the chain whose parsers are through go back, trace cleared */
        const uint32_t rel0 = rel;
        while (rel < k && UNI(LDS_LOAD_ACQ(&lds->p_done[rel % L::NSLOT])) == rel + 1u) {
            FOR_LANES
            {
                if ((uint32_t)LANE < SG_TRACE / 32)
                    lds->trace[rel % L::NSLOT][LANE] = 0;
            }
            rel++;
        }
        if (rel != rel0) {
            WAVE_SYNC();
            ON_LANE0 { LDS_STORE_REL(&lds->p_released, rel); }
        }
        const uint32_t ks = k % L::NSLOT;
        if (held)
            return;
        if (UNI(LDS_LOAD_ACQ(&lds->p_done[ks])) != k + 1u)
            break;
        if (cxp != SG_PIPE_NOXP) {
            ft = UNI(scr.sidx[ks * SG_TRACE + cxp % SG_G]);
            cxp = SG_PIPE_NOXP;
        }
        const uint32_t kind = UNI(lds->wv[ks].exit_kind);
        const uint32_t xp = UNI(lds->wv[ks].exit_p);
        sg_append(job, &lds->out, scr.tok + ks * SG_TOKCAP, ft, UNI(lds->wv[ks].ntok), 1, 1u, ZD_MIN_LOOKAHEAD);
        if (kind == SG_EXIT_SYNCED) {
            SG_PATH(56);
            k = xp / SG_G; /* (beyond k: a parser only hands over past its own segment) */
            cxp = xp;
            ft = 0;
            continue;
        }
        if (kind == SG_EXIT_UNSYNCED || kind == SG_EXIT_LAST) {
            /* the parser gave up, or ran out of segments it could look into: the segment xp lies in is
             * parsed again from this exact state, once its own speculative parse is out of the way */
            const uint32_t xl = UNI(lds->wv[ks].exit_len), xa = UNI(lds->wv[ks].exit_at);
            const uint32_t xn = UNI(lds->wv[ks].exit_pending);
            SG_PATH(kind == SG_EXIT_UNSYNCED ? 57 : 58);
            k = xp / SG_G;
            ft = 0;
            ON_LANE0
            {
                lds->p_rs[0] = xp;
                lds->p_rs[1] = xl;
                lds->p_rs[2] = xa;
                lds->p_rs[3] = xn;
                lds->redo_seg = k;
                lds->chain = k;
                lds->chain_ft = 0;
                lds->p_chain_xp = SG_PIPE_NOXP;
                LDS_STORE_REL(&lds->p_redo, 1u);
            }
            WAVE_SYNC();
            return;
        }
        /* SG_EXIT_END: the parse reached the end of the input */
        SG_PATH(59);
        sg_end_of_input(job, lds, UNI(lds->wv[ks].exit_pending), xp);
        ON_LANE0 { LDS_STORE_REL(&lds->finished, 1u); }
        WAVE_SYNC();
        return;
    }
    ON_LANE0
    {
        lds->chain = k;
        lds->chain_ft = ft;
        lds->p_chain_xp = cxp;
    }
    WAVE_SYNC();
}

/* One job, if one is ready.  `allow` is SG_JOB_ALL in the product; the host emulation narrows it to
 * drive the same code through other schedules. */
template <bool TABLE, class L>
DEV int sg_pipe_step(const LzJob &job, L *lds, const SgScratch &scr, uint32_t allow)
{
    if (UNI(LDS_LOAD_ACQ(&lds->finished)) != 0u)
        return SG_PIPE_DONE;
    const uint32_t redo = UNI(LDS_LOAD_ACQ(&lds->p_redo));
    if ((allow & SG_JOB_REDO) && redo == 1u) {
        const uint32_t t = UNI(lds->redo_seg);
        if (UNI(LDS_LOAD_ACQ(&lds->p_done[t % L::NSLOT])) == t + 1u && sg_pipe_claim(&lds->p_redo, 1u, 2u)) {
            const uint32_t sp = UNI(lds->p_rs[0]), sl = UNI(lds->p_rs[1]), sa = UNI(lds->p_rs[2]);
            const uint32_t sn = UNI(lds->p_rs[3]);
            SG_COUNT(2, 0x10000 + t);
            sg_parse_segment<TABLE, true>(job, lds, scr, t, sp, sl, sa, (int)sn);
            SG_COUNT(3, 0);
            ON_LANE0 { LDS_STORE_REL(&lds->p_redo, 0u); }
            return SG_PIPE_WORKED;
        }
    }
    const uint32_t rel = UNI(LDS_LOAD_ACQ(&lds->p_released));
    if ((allow & SG_JOB_RESOLVE) && UNI(LDS_LOAD_ACQ(&lds->p_res_busy)) == 0u) {
        const uint32_t k = UNI(LDS_LOAD_ACQ(&lds->chain)); /* (a hint: the resolver looks again once it holds the word) */
        if (((redo == 0u && UNI(LDS_LOAD_ACQ(&lds->p_done[k % L::NSLOT])) == k + 1u) ||
             (rel < k && UNI(LDS_LOAD_ACQ(&lds->p_done[rel % L::NSLOT])) == rel + 1u)) &&
            sg_pipe_claim(&lds->p_res_busy, 0u, 1u)) {
            sg_pipe_resolve(job, lds, scr);
            ON_LANE0 { LDS_STORE_REL(&lds->p_res_busy, 0u); }
            return SG_PIPE_WORKED;
        }
    }
    uint32_t hi = UNI(LDS_LOAD_ACQ(&lds->hi));
    if ((allow & SG_JOB_LOAD) && hi < job.ntot && sg_pipe_may_load<L>(hi, rel) &&
        UNI(LDS_LOAD_ACQ(&lds->p_load_busy)) == 0u && sg_pipe_claim(&lds->p_load_busy, 0u, 1u)) {
        hi = UNI(LDS_LOAD_ACQ(&lds->hi)); /* (whoever held the loader before may have moved it) */
        if (hi < job.ntot && sg_pipe_may_load<L>(hi, rel)) {
            SG_PIPE_HOOK_LOAD(hi, rel);
            LzState st;
            st.hi = hi;
            st.lo = 0;
            st.wrap_base = hi / L::RING * L::RING;
            lz_load_chunk<L>(job, lds, st);
            ON_LANE0 { LDS_STORE_REL(&lds->hi, st.hi); }
        }
        ON_LANE0 { LDS_STORE_REL(&lds->p_load_busy, 0u); }
        return SG_PIPE_WORKED;
    }
    if (allow & SG_JOB_PARSE) {
        const uint32_t g = UNI(LDS_LOAD_ACQ(&lds->p_next));
        if (g < sg_pipe_nseg(job.n) && g < rel + L::NSLOT && hi >= sg_pipe_want(g, job.ntot) &&
            sg_pipe_claim(&lds->p_next, g, g + 1u)) {
            SG_COUNT(2, g);
            sg_parse_segment<TABLE, true>(job, lds, scr, g, g * SG_G, 2u, 0u, 0);
            SG_COUNT(3, 0);
            ON_LANE0 { LDS_STORE_REL(&lds->p_done[g % L::NSLOT], g + 1u); }
            return SG_PIPE_WORKED;
        }
    }
    return SG_PIPE_IDLE;
}

#ifndef ZSC_WAVE_EMU
/* how far the workgroup has got, as one number: every job that ends moves one of these */
template <class L>
DEV uint32_t sg_pipe_progress(L *lds)
{
    return UNI(LDS_LOAD_ACQ(&lds->p_next)) + UNI(LDS_LOAD_ACQ(&lds->p_released)) + UNI(LDS_LOAD_ACQ(&lds->hi)) +
           UNI(LDS_LOAD_ACQ(&lds->chain)) + UNI(LDS_LOAD_ACQ(&lds->p_redo));
}

/* Empty polls in a row, with nothing moving anywhere in the workgroup, after which a wave gives up.  The
 * longest a wave legitimately sees nothing move is one job of another wave, and the longest job is a
 * segment parsed at level 9 over data made for it: at most SG_G + SG_OV positions, each at most the chain
 * budget (4 096) of candidates that each ask for a long compare of some 40 cycles -- 1.3 x 10^8 cycles,
 * up to six times that when the five other waves of its SIMD are all busy.  A poll after back-off is a
 * sleep of 1 024 cycles and a few loads, so 2^20 of them are above 10^9 cycles: about half a second,
 * whatever the buffer's length. */
#define SG_PIPE_MAX_IDLE (1u << 20)

/* One wave's life in the pipeline.  All waiting happens here: a wave without a job sleeps a little
 * (longer when it keeps finding none) and asks again.  Waves only wait for waves of their own
 * workgroup, and the number of empty polls without any progress in the workgroup is bounded, so that a
 * logic error ends as Z_STREAM_ERROR (p_stuck) instead of hanging the device. */
template <bool TABLE, class L>
DEV void sg_pipe_run(const LzJob &job, L *lds, const SgScratch &scr)
{
    uint32_t idle = 0, row = 0, seen = 0;
    for (;;) {
        const int r = sg_pipe_step<TABLE>(job, lds, scr, SG_JOB_ALL);
        if (r == SG_PIPE_DONE)
            break;
        if (r == SG_PIPE_WORKED) {
            row = idle = 0;
            continue;
        }
        const uint32_t now = sg_pipe_progress(lds);
        if (now != seen) {
            seen = now;
            idle = 0;
        }
        if (++idle > SG_PIPE_MAX_IDLE) {
            ON_LANE0
            {
                lds->p_stuck = 1;
                LDS_STORE_REL(&lds->finished, 1u);
            }
            break;
        }
        WAVE_NAP(++row > 8u);
    }
}
#endif

#endif
