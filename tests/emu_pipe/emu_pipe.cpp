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
 */
#include <stdint.h>
extern "C" void pipe_ring_read(uint32_t wrap_base, uint32_t pos);
extern "C" void pipe_chunk_load(uint32_t hi, uint32_t released);
#define LZ_RING_HOOK(st, pos) pipe_ring_read((st).wrap_base, (pos))
#define SG_PIPE_HOOK_LOAD(hi, released) pipe_chunk_load((hi), (released))
#include "../emu/emu_pipeline.cpp"
#include "../../zsc_amd/csrc/lz_parse_pipe.h"

struct PipeCtx {
    EmuChains c;
    std::vector<uint32_t> syms, tok;
    std::vector<uint16_t> sidx;
    std::vector<ZdBlockRec> recs;
    ZdParseOut po;
    LzJob job;
    SgLds *lds;
    SgScratch scr;
    int level, strategy;
    bool table;
    unsigned long long jobs[4]; /* redo, resolve, load, parse */
};

static PipeCtx *g_ctx;      /* the run the hooks look at */
static int g_in_load;       /* the loader works out ring indices of what it brings in */
extern "C" {
unsigned long long g_pipe_bad_reads, g_pipe_bad_loads, g_pipe_reads, g_pipe_reads_ahead;
}

extern "C" void pipe_ring_read(uint32_t wrap_base, uint32_t pos)
{
    if (!g_ctx || g_in_load)
        return;
    const SgLds *lds = g_ctx->lds;
    g_pipe_reads++;
    /* the index itself: lz_ridx wraps once, so the position must lie within two rings of the parser's base */
    if (pos < wrap_base || pos - wrap_base >= 2u * SgLds::RING)
        g_pipe_bad_reads++;
    if (pos >= lds->hi) {
        /* Behind the ring's data.  A segment is handed out with everything its parser and the register
         * caches can touch in the ring (sg_pipe_want), unless the input ends before that: so this may only
         * happen once the whole input is loaded (the bytes there read as zero and are never used). */
        g_pipe_reads_ahead++;
        if (lds->hi < g_ctx->job.ntot)
            g_pipe_bad_reads++;
        return;
    }
    if (pos < sg_pipe_floor(lds->p_released) || (uint64_t)pos + SgLds::RING < lds->hi)
        g_pipe_bad_reads++;
}

extern "C" void pipe_chunk_load(uint32_t hi, uint32_t released)
{
    (void)released;
    g_in_load = 1;
    const SgLds *lds = g_ctx->lds;
    /* the oldest segment somebody may still read the window for */
    uint32_t oldest = lds->chain;
    for (uint32_t g = lds->p_next > SG_NS ? lds->p_next - SG_NS : 0; g < lds->p_next; g++)
        if (lds->p_done[g % SG_NS] != g + 1u && g < oldest)
            oldest = g;
    const uint64_t first = (uint64_t)oldest * SG_G;
    const uint64_t keep = first > ZD_TILE ? first - ZD_TILE : 0;
    if ((uint64_t)hi + SgLds::CHUNK > keep + SgLds::RING)
        g_pipe_bad_loads++;
}

extern "C" void *emu_pipe_open(const uint8_t *src, uint32_t n, int level, int strategy)
{
    if (level < 4 || level > 9)
        return nullptr;
    PipeCtx *x = new PipeCtx();
    x->level = level;
    x->strategy = strategy;
    build_chains(x->c, src, n);
    build_table(x->c, level, strategy);
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
    job.r2 = x->c.r2.empty() ? nullptr : x->c.r2.data();
    x->table = job.r2 != nullptr;
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
    x->lds = (SgLds *)malloc(sizeof(SgLds));
    memset(x->lds, 0x6B, sizeof(SgLds));
    x->tok.assign((size_t)SG_NS * SG_TOKCAP, 0xDDDDDDDD);
    x->sidx.assign((size_t)SG_NS * SG_TRACE, 0xDDDD);
    x->scr.tok = x->tok.data();
    x->scr.sidx = x->sidx.data();
    for (int w = 0; w < SG_W; w++)
        sg_pipe_init(x->lds, w);
    memset(x->jobs, 0, sizeof x->jobs);
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
    const int r = x->table ? sg_pipe_step<true>(x->job, x->lds, x->scr, allow)
                           : sg_pipe_step<false>(x->job, x->lds, x->scr, allow);
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
    return r;
}

/* The whole buffer under one of the schedules; returns 0, or -1 when no wave found a job although the
 * buffer is not finished (a deadlock of the design), -3 when it took absurdly many steps.
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

extern "C" void emu_pipe_jobs(void *ctx, unsigned long long *out4)
{
    memcpy(out4, ((PipeCtx *)ctx)->jobs, sizeof(unsigned long long) * 4);
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

/* the kernels behind the parser on a finished run, as emu_compress (tests/emu) runs them: 64 lanes only */
extern "C" int emu_pipe_stream(void *ctx, int wrap, uint8_t *out, uint32_t out_cap, uint32_t *out_len)
{
    PipeCtx *x = (PipeCtx *)ctx;
    const uint32_t n = x->job.n;
    std::vector<ZdBlockPlan> plans(x->recs.size());
    ZdBuf buf;
    memset(&buf, 0, sizeof buf);
    buf.in_len = n;
    buf.max_blocks = (uint32_t)x->recs.size();
    buf.out_cap = out_cap;
    buf.level = (uint32_t)x->level;
    buf.wrap = (uint32_t)wrap;
    buf.strategy = (uint32_t)x->strategy;
    buf.wbits = (uint32_t)g_wbits;
    ZdResult res;
    memset(&res, 0, sizeof res);
    CkLds ck;
    res.adler = wrap == 1 ? ck_adler32(x->c.in.data(), n) : wrap == 2 ? ck_crc32(x->c.in.data(), n, &ck) : 0;
    for (uint32_t b = 0; b < x->po.nblocks; b++) {
        HpLds hl;
        memset(&hl, 0x5A, sizeof hl);
        huff_plan_block(x->syms.data() + x->recs[b].sym_begin, &x->recs[b], (uint32_t)x->strategy, &plans[b], &hl);
    }
    std::vector<uint32_t> outw(((size_t)out_cap + 64) / 4 + 4, 0xCDCDCDCD);
    layout_buffer(&buf, &x->po, x->recs.data(), plans.data(), &res, (uint8_t *)outw.data());
    for (uint32_t b = 0; b < x->po.nblocks; b++) {
        BeLds bl;
        memset(&bl, 0x77, sizeof bl);
        emit_block(x->c.in.data(), x->syms.data() + x->recs[b].sym_begin, &x->recs[b], &plans[b], outw.data(), &bl);
    }
    *out_len = res.out_len;
    if (res.status == 0)
        memcpy(out, outw.data(), res.out_len);
    return res.status;
}

extern "C" void emu_pipe_close(void *ctx)
{
    PipeCtx *x = (PipeCtx *)ctx;
    free(x->lds);
    delete x;
}
