/*
 * emu_pipe.cpp -- TEST INFRASTRUCTURE ONLY.
 *
 * The pipeline schedule of the segmented parser (zsc_amd/csrc/lz_parse_pipe.h) in the lane emulation:
 * the kernel sources compiled with -DZSC_WAVE_EMU, as tests/emu does (whose driver is included whole, for
 * its chains, tables and the kernels behind the parser).  A job of the pipeline never waits inside, so
 * any order in which the waves of a workgroup ask for jobs is a legal schedule; the test chooses the
 * order, and every one of them must give the oracle's stream.
 *
 * Two hooks that are empty in the product check the window invariant (lz_parse_pipe.h):
 *   - every ring index a parser works out is for a position at or above sg_pipe_floor(p_released), whose
 *     byte has not been overwritten (position + RING >= hi) and has been loaded (position < hi, unless the
 *     whole input is in the ring), and within the two rings from the parser's base that lz_ridx can fold;
 *   - a chunk load overwrites nothing at or above the first position, less one window, of the oldest
 *     segment the resolver has not passed or whose parser is not through -- worked out here from the
 *     slots' own state, not from p_released.
 *
 * One source for both LDS geometries of the pipeline (lz_parse_seg.h): SgLds, and with -DPIPE_NARROW SgLdsNarrow
 * (tests/emu_pipe_narrow), which is built without the match table and without the kernels behind the parser, and
 * counts two figures the wide geometry never needed: the largest number of segments in flight (handed out and
 * not yet given back; once the window moves the ring bounds it here, not the slots) and the number of polls
 * that found no job.
 */
#include <stdint.h>
extern "C" void pipe_ring_read(uint32_t wrap_base, uint32_t pos);
extern "C" void pipe_chunk_load(uint32_t hi, uint32_t released);
#define LZ_RING_HOOK(st, pos) pipe_ring_read((st).wrap_base, (pos))
#define SG_PIPE_HOOK_LOAD(hi, released) pipe_chunk_load((hi), (released))
#include "../emu/emu_pipeline.cpp"
#include "../../zsc_amd/csrc/lz_parse_pipe.h"

#ifdef PIPE_NARROW
typedef SgLdsNarrow PL;
static const bool kPipeTable = false; /* (the narrow entry is built without the match table) */
#else
typedef SgLds PL;
static const bool kPipeTable = true;
#endif

struct PipeCtx {
    EmuBuf e; /* chains, table, the parser's job and what it writes (emu_pipeline.cpp) */
    std::vector<uint32_t> tok;
    std::vector<uint16_t> sidx;
    PL *lds;
    SgScratch scr;
    unsigned long long jobs[4]; /* redo, resolve, load, parse */
#ifdef PIPE_NARROW
    unsigned long long idle;     /* polls that found no job */
    uint32_t max_in_flight;      /* segments handed out and not yet given back */
    uint32_t max_in_flight_ring; /* ... while the ring is what bounds them: the window has begun to move
                                    (sg_pipe_floor above 0) and the input is not all loaded */
#endif
};

static PipeCtx *g_ctx;      /* the run the hooks look at */
static int g_in_load;       /* the loader works out ring indices of what it brings in */
extern "C" {
unsigned long long g_pipe_bad_reads, g_pipe_bad_loads, g_pipe_reads, g_pipe_reads_ahead;
#ifdef PIPE_NARROW
unsigned long long g_pipe_loads;
#endif
}

extern "C" void pipe_ring_read(uint32_t wrap_base, uint32_t pos)
{
    if (!g_ctx || g_in_load)
        return;
    const PL *lds = g_ctx->lds;
    g_pipe_reads++;
    /* the index itself: lz_ridx wraps once, so the position must lie within two rings of the parser's base */
    if (pos < wrap_base || pos - wrap_base >= 2u * PL::RING)
        g_pipe_bad_reads++;
    if (pos >= lds->hi) {
        /* Behind the ring's data.  A segment is handed out with everything its parser and the register
         * caches can touch in the ring (sg_pipe_want), unless the input ends before that: so this may only
         * happen once the whole input is loaded (the bytes there read as zero and are never used). */
        g_pipe_reads_ahead++;
        if (lds->hi < g_ctx->e.job.ntot)
            g_pipe_bad_reads++;
        return;
    }
    if (pos < sg_pipe_floor(lds->p_released) || (uint64_t)pos + PL::RING < lds->hi)
        g_pipe_bad_reads++;
}

extern "C" void pipe_chunk_load(uint32_t hi, uint32_t released)
{
    (void)released;
    g_in_load = 1;
#ifdef PIPE_NARROW
    g_pipe_loads++;
#endif
    const PL *lds = g_ctx->lds;
    /* the oldest segment somebody may still read the window for */
    uint32_t oldest = lds->chain;
    for (uint32_t g = lds->p_next > PL::NSLOT ? lds->p_next - PL::NSLOT : 0; g < lds->p_next; g++)
        if (lds->p_done[g % PL::NSLOT] != g + 1u && g < oldest)
            oldest = g;
    const uint64_t first = (uint64_t)oldest * SG_G;
    const uint64_t keep = first > ZD_TILE ? first - ZD_TILE : 0;
    if ((uint64_t)hi + PL::CHUNK > keep + PL::RING)
        g_pipe_bad_loads++;
}

#ifdef PIPE_NARROW
/* ring, chunk, slots, bytes of LDS */
extern "C" void emu_pipe_geometry(uint32_t *out4)
{
    out4[0] = PL::RING;
    out4[1] = PL::CHUNK;
    out4[2] = PL::NSLOT;
    out4[3] = (uint32_t)sizeof(PL);
}
#endif

extern "C" void *emu_pipe_open(const uint8_t *src, uint32_t n, int level, int strategy)
{
    if (level < 4 || level > 9)
        return nullptr;
    PipeCtx *x = new PipeCtx();
    /* g_link_in_parser: as the runtime runs a batch that goes to the segmented parser as a whole */
    x->e.open(src, n, level, 0, strategy, 0, nullptr, kPipeTable, g_link_in_parser != 0);
    x->lds = (PL *)malloc(sizeof(PL));
    memset(x->lds, 0x6B, sizeof(PL));
    /* the scratch as the kernel lays it out: SG_NS slots, of which a geometry uses the first NSLOT */
    x->tok.assign((size_t)SG_NS * SG_TOKCAP, 0xDDDDDDDD);
    x->sidx.assign((size_t)SG_NS * SG_TRACE, 0xDDDD);
    x->scr.tok = x->tok.data();
    x->scr.sidx = x->sidx.data();
    for (int w = 0; w < SG_W; w++)
        sg_pipe_init(x->lds, w);
    return x; /* (new PipeCtx() left the counters at 0) */
}

/* one call of wave w: a job of the kinds in `allow` if one is ready.  Returns SG_PIPE_DONE / WORKED / IDLE. */
extern "C" int emu_pipe_step(void *ctx, int w, uint32_t allow)
{
    (void)w; /* (a wave carries nothing from one job to the next: which one asks makes no difference) */
    PipeCtx *x = (PipeCtx *)ctx;
    g_ctx = x;
    g_in_load = 0;
    const uint32_t before[4] = {x->lds->p_redo, x->lds->chain + x->lds->out.nsyms + x->lds->p_released, x->lds->hi, x->lds->p_next};
    const int r = x->e.job.r2 ? sg_pipe_step<true>(x->e.job, x->lds, x->scr, allow)
                              : sg_pipe_step<false>(x->e.job, x->lds, x->scr, allow);
    g_ctx = nullptr;
    if (r == SG_PIPE_WORKED) {
        if (x->lds->p_next != before[3])
            x->jobs[3]++;
        else if (x->lds->hi != before[2])
            x->jobs[2]++;
        else if (before[0] == 1u)
            x->jobs[0]++;
        else
            x->jobs[1]++;
    }
#ifdef PIPE_NARROW
    if (r == SG_PIPE_IDLE)
        x->idle++;
    if (x->lds->p_next - x->lds->p_released > x->max_in_flight)
        x->max_in_flight = x->lds->p_next - x->lds->p_released;
    if (sg_pipe_floor(x->lds->p_released) > 0u && x->lds->hi < x->e.job.ntot &&
        x->lds->p_next - x->lds->p_released > x->max_in_flight_ring)
        x->max_in_flight_ring = x->lds->p_next - x->lds->p_released;
#endif
    return r;
}

/* The whole buffer under one of the schedules; returns 0, or -1 when no wave found a job although the
 * buffer is not finished (a deadlock of the design; on the GPU: the idle bound), -3 when it took absurdly many
 * steps, -4 p_stuck.
 *   mode 0  the waves ask in turn, each for any job, most urgent first (what the GPU's waves do)
 *   mode 1  the same, least urgent first: speculative parses run as far ahead as slots and window allow
 *   mode 2  wave 0 alone
 *   mode 3  every wave but wave 0
 *   mode 4  seeded random: a random wave asks for a random subset of the job kinds
 * In modes 0-3 wave w asks for its own kind of job first (w % 4: redo, resolve, load, parse), then for any. */
extern "C" int emu_pipe_run(void *ctx, int mode, uint32_t seed)
{
    PipeCtx *x = (PipeCtx *)ctx;
    uint64_t rng = 0x9E3779B97F4A7C15ull ^ ((uint64_t)seed * 0xD1342543DE82EF95ull + 1u);
    const uint64_t max_steps = 64ull + 64ull * (x->e.job.n / SG_G + 1u) * 8u;
    int w = 0;
    for (uint64_t it = 0; it < max_steps; it++) {
        int r = SG_PIPE_IDLE;
        if (mode == 4) {
            rng = rng * 6364136223846793005ull + 1442695040888963407ull;
            const uint32_t allow = (uint32_t)(rng >> 33) & SG_JOB_ALL;
            w = (int)((rng >> 40) % SG_W);
            r = allow ? emu_pipe_step(ctx, w, allow) : SG_PIPE_IDLE;
            if (r == SG_PIPE_IDLE)
                r = emu_pipe_step(ctx, w, SG_JOB_ALL);
        } else if (mode == 1) {
            for (uint32_t kind = SG_JOB_PARSE; kind != 0 && r == SG_PIPE_IDLE; kind >>= 1)
                r = emu_pipe_step(ctx, w, kind);
            w = (w + SG_W - 1) % SG_W;
        } else {
            if (mode == 2)
                w = 0;
            r = emu_pipe_step(ctx, w, 1u << (w % 4));
            if (r == SG_PIPE_IDLE)
                r = emu_pipe_step(ctx, w, SG_JOB_ALL);
            w = (w + 1) % SG_W;
            if (mode == 3 && w == 0)
                w = 1;
        }
        if (r == SG_PIPE_DONE)
            return x->lds->p_stuck ? -4 : 0;
        if (r == SG_PIPE_IDLE && mode != 4)
            return -1; /* every job kind was offered and none was ready */
        if (r == SG_PIPE_IDLE && emu_pipe_step(ctx, 0, SG_JOB_ALL) == SG_PIPE_IDLE)
            return -1;
    }
    return -3;
}

#ifdef PIPE_NARROW
/* redo, resolve, load, parse jobs; polls that found no job; the most segments ever in flight, and while the
 * ring bounds them */
extern "C" void emu_pipe_figures(void *ctx, unsigned long long *out7)
{
    PipeCtx *x = (PipeCtx *)ctx;
    memcpy(out7, x->jobs, sizeof(unsigned long long) * 4);
    out7[4] = x->idle;
    out7[5] = x->max_in_flight;
    out7[6] = x->max_in_flight_ring;
}
#else
extern "C" void emu_pipe_jobs(void *ctx, unsigned long long *out4)
{
    memcpy(out4, ((PipeCtx *)ctx)->jobs, sizeof(unsigned long long) * 4);
}

/* the kernels behind the parser on a finished run, as emu_compress (tests/emu) runs them: 64 lanes only */
extern "C" int emu_pipe_stream(void *ctx, int wrap, uint8_t *out, uint32_t out_cap, uint32_t *out_len)
{
    EmuBuf &e = ((PipeCtx *)ctx)->e;
    e.buf.wrap = (uint32_t)wrap;
    e.buf.out_cap = out_cap;
    e.emit();
    return e.give(out, out_len);
}
#endif

/* stage P of a finished run */
extern "C" void emu_pipe_parse_result(void *ctx, uint32_t *syms, uint32_t *nsyms, ZdBlockRec *blocks, uint32_t *nblocks)
{
    const EmuBuf &e = ((PipeCtx *)ctx)->e;
    *nsyms = e.po.nsyms;
    *nblocks = e.po.nblocks;
    memcpy(syms, e.syms.data(), (size_t)e.po.nsyms * 4);
    memcpy(blocks, e.recs.data(), (size_t)e.po.nblocks * sizeof(ZdBlockRec));
}

extern "C" void emu_pipe_close(void *ctx)
{
    PipeCtx *x = (PipeCtx *)ctx;
    free(x->lds);
    delete x;
}
