/*
 * emu_pipe_narrow.cpp -- TEST INFRASTRUCTURE ONLY.
 *
 * The pipeline schedule of the segmented parser (zsc_amd/csrc/lz_parse_pipe.h) in its own LDS geometry
 * (SgLdsNarrow, lz_parse_seg.h) in the lane emulation: what tests/emu_pipe does for the wide geometry, with
 * the same two hooks on the window invariant, stated for the narrow ring --
 *   - every ring index a parser works out is for a position at or above sg_pipe_floor(p_released), whose byte
 *     has not been overwritten (position + RING >= hi) and has been loaded (position < hi, unless the whole
 *     input is in the ring), and within the two rings from the parser's base that lz_ridx can fold;
 *   - a chunk load overwrites nothing at or above the first position, less one window, of the oldest segment
 *     the resolver has not passed or whose parser is not through -- worked out from the slots' own state,
 *     not from p_released --
 * and two figures the wide geometry never needed: the largest number of segments in flight (handed out and
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

typedef SgLdsNarrow PL;

struct PipeCtx {
    EmuChains c;
    std::vector<uint32_t> syms, tok;
    std::vector<uint16_t> sidx;
    std::vector<ZdBlockRec> recs;
    ZdParseOut po;
    LzJob job;
    PL *lds;
    SgScratch scr;
    int level, strategy;
    unsigned long long jobs[4]; /* redo, resolve, load, parse */
    unsigned long long idle;    /* polls that found no job */
    uint32_t max_in_flight;        /* segments handed out and not yet given back */
    uint32_t max_in_flight_ring;   /* ... while the ring is what bounds them: the window has begun to move
                                      (sg_pipe_floor above 0) and the input is not all loaded */
};

static PipeCtx *g_ctx; /* the run the hooks look at */
static int g_in_load;  /* the loader works out ring indices of what it brings in */
extern "C" {
unsigned long long g_pipe_bad_reads, g_pipe_bad_loads, g_pipe_reads, g_pipe_reads_ahead, g_pipe_loads;
}

extern "C" void pipe_ring_read(uint32_t wrap_base, uint32_t pos)
{
    if (!g_ctx || g_in_load)
        return;
    const PL *lds = g_ctx->lds;
    g_pipe_reads++;
    if (pos < wrap_base || pos - wrap_base >= 2u * PL::RING)
        g_pipe_bad_reads++;
    if (pos >= lds->hi) {
        /* behind the ring's data: only once the whole input is loaded (emu_pipe.cpp) */
        g_pipe_reads_ahead++;
        if (lds->hi < g_ctx->job.ntot)
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
    g_pipe_loads++;
    const PL *lds = g_ctx->lds;
    uint32_t oldest = lds->chain;
    for (uint32_t g = lds->p_next > PL::NSLOT ? lds->p_next - PL::NSLOT : 0; g < lds->p_next; g++)
        if (lds->p_done[g % PL::NSLOT] != g + 1u && g < oldest)
            oldest = g;
    const uint64_t first = (uint64_t)oldest * SG_G;
    const uint64_t keep = first > ZD_TILE ? first - ZD_TILE : 0;
    if ((uint64_t)hi + PL::CHUNK > keep + PL::RING)
        g_pipe_bad_loads++;
}

/* ring, chunk, slots, bytes of LDS */
extern "C" void emu_pipe_geometry(uint32_t *out4)
{
    out4[0] = PL::RING;
    out4[1] = PL::CHUNK;
    out4[2] = PL::NSLOT;
    out4[3] = (uint32_t)sizeof(PL);
}

extern "C" void *emu_pipe_open(const uint8_t *src, uint32_t n, int level, int strategy)
{
    if (level < 4 || level > 9)
        return nullptr;
    PipeCtx *x = new PipeCtx();
    x->level = level;
    x->strategy = strategy;
    build_chains(x->c, src, n);
    x->syms.assign((size_t)n + 64, 0);
    x->recs.resize(n / ((1u << (g_mem_level + 6)) - 1u) + 2);
    x->po.nsyms = x->po.nblocks = 0;
    LzJob &job = x->job;
    job.in = x->c.in.data();
    job.n = n;
    job.sorted = x->c.sorted.data();
    job.rank = x->c.rank.data();
    job.hib = x->c.hib.data();
    job.cnt = x->c.cnt.data();
    job.dir = nullptr;
    if (g_link_in_parser) { /* as the runtime runs a batch that goes to the segmented parser as a whole */
        job.dir = x->c.dir.data();
        job.hib = nullptr;
        job.cnt = nullptr;
    }
    job.r2 = nullptr; /* (the narrow entry is built without the match table) */
    job.stair_min = g_stair_min;
    job.syms = x->syms.data();
    job.blocks = x->recs.data();
    job.out = &x->po;
    job.cfg = level_cfg(level);
    job.strategy = (uint32_t)strategy;
    job.more = 0;
    job.sched = nullptr;
    job.nsched = 0;
    job.n0 = n;
    job.ntot = n;
    x->lds = (PL *)malloc(sizeof(PL));
    memset(x->lds, 0x6B, sizeof(PL));
    /* the scratch as the kernel lays it out: SG_NS slots, of which this geometry uses the first NSLOT */
    x->tok.assign((size_t)SG_NS * SG_TOKCAP, 0xDDDDDDDD);
    x->sidx.assign((size_t)SG_NS * SG_TRACE, 0xDDDD);
    x->scr.tok = x->tok.data();
    x->scr.sidx = x->sidx.data();
    for (int w = 0; w < SG_W; w++)
        sg_pipe_init(x->lds, w);
    memset(x->jobs, 0, sizeof x->jobs);
    x->idle = 0;
    x->max_in_flight = x->max_in_flight_ring = 0;
    return x;
}

/* one call of wave w: a job of the kinds in `allow` if one is ready.  Returns SG_PIPE_DONE / WORKED / IDLE. */
extern "C" int emu_pipe_step(void *ctx, int w, uint32_t allow)
{
    (void)w; /* (a wave carries nothing from one job to the next: which one asks makes no difference) */
    PipeCtx *x = (PipeCtx *)ctx;
    g_ctx = x;
    g_in_load = 0;
    const uint32_t before[4] = {x->lds->p_redo, x->lds->chain + x->lds->out.nsyms + x->lds->p_released, x->lds->hi, x->lds->p_next};
    const int r = sg_pipe_step<false>(x->job, x->lds, x->scr, allow);
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
    } else if (r == SG_PIPE_IDLE)
        x->idle++;
    if (x->lds->p_next - x->lds->p_released > x->max_in_flight)
        x->max_in_flight = x->lds->p_next - x->lds->p_released;
    if (sg_pipe_floor(x->lds->p_released) > 0u && x->lds->hi < x->job.ntot &&
        x->lds->p_next - x->lds->p_released > x->max_in_flight_ring)
        x->max_in_flight_ring = x->lds->p_next - x->lds->p_released;
    return r;
}

/* The whole buffer under one of the schedules of emu_pipe.cpp (0 round robin, 1 reverse: parses run as far
 * ahead as the ring allows, 2 wave 0 alone, 3 every wave but wave 0, 4 seeded random); 0, or -1 when no wave
 * found a job although the buffer is not finished (on the GPU: the idle bound), -3 absurdly many steps, -4
 * p_stuck. */
extern "C" int emu_pipe_run(void *ctx, int mode, uint32_t seed)
{
    PipeCtx *x = (PipeCtx *)ctx;
    uint64_t rng = 0x9E3779B97F4A7C15ull ^ ((uint64_t)seed * 0xD1342543DE82EF95ull + 1u);
    const uint64_t max_steps = 64ull + 64ull * (x->job.n / SG_G + 1u) * 8u;
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

/* stage P of a finished run */
extern "C" void emu_pipe_parse_result(void *ctx, uint32_t *syms, uint32_t *nsyms, ZdBlockRec *blocks, uint32_t *nblocks)
{
    PipeCtx *x = (PipeCtx *)ctx;
    *nsyms = x->po.nsyms;
    *nblocks = x->po.nblocks;
    memcpy(syms, x->syms.data(), (size_t)x->po.nsyms * 4);
    memcpy(blocks, x->recs.data(), (size_t)x->po.nblocks * sizeof(ZdBlockRec));
}

extern "C" void emu_pipe_close(void *ctx)
{
    PipeCtx *x = (PipeCtx *)ctx;
    free(x->lds);
    delete x;
}
