/*
 * emu_verify.cpp -- TEST INFRASTRUCTURE ONLY.
 *
 * The deflate pipeline of tests/emu with read-back verification on top (zsc_amd/csrc/deflate_verify.h), in
 * the lane emulation: what zsc_hip_deflate_plan_run enqueues for one buffer of a plan with verification
 * enabled, kernel by kernel (emu_verify_compress, which hands out the kept block facts), and what
 * zsc_hip_deflate_plan_verify enqueues (emu_verify_check), on a stream and an input the caller supplies,
 * so that a test can damage either.
 */
#include "../emu/emu_pipeline.cpp"
#include "../../zsc_amd/csrc/deflate_verify.h"

/* the runtime's offloadable(); 0 where the plan would not be made */
static int vf_params(int level, int window_bits, int mem_level, int *wrap, int *wb)
{
    *wrap = 1;
    *wb = window_bits;
    if (*wb < 0) {
        *wrap = 0;
        *wb = -*wb;
    } else if (*wb > 15) {
        *wrap = 2;
        *wb -= 16;
    }
    if (*wb == 8 && *wrap == 1)
        *wb = 9;
    return !(level < 1 || level > 9 || *wb < 9 || *wb > 15 || mem_level < 1 || mem_level > 9);
}

/* Returns the buffer's status.  window_bits as zsc_compress2 takes it (the wrapper folded in).
 *   out, *out_len        the stream (status 0); *out_len is the plan's result either way
 *   blocks, *nblocks     the facts k_verify_keep keeps (bit_off, in_begin, in_len, type | last << 8), at most
 *                        blocks_cap of them; none where the status is not 0 */
extern "C" int emu_verify_compress(const uint8_t *src, uint32_t n, int level, int window_bits, int mem_level,
                                   int strategy, uint32_t out_cap, uint8_t *out, uint32_t *out_len, uint32_t *blocks,
                                   uint32_t blocks_cap, uint32_t *nblocks)
{
    *out_len = 0;
    *nblocks = 0;
    int wrap, wb;
    if (!vf_params(level, window_bits, mem_level, &wrap, &wb))
        return -2;
    emu_set_params(wb, mem_level);

    EmuChains c;
    build_chains(c, src, n);
    build_table(c, level, strategy);
    std::vector<uint32_t> syms((size_t)n + 64);
    const uint32_t max_blocks = n / ((1u << (g_mem_level + 6)) - 1u) + 2;
    std::vector<ZdBlockRec> recs(max_blocks);
    std::vector<ZdBlockPlan> plans(max_blocks);
    ZdParseOut po = {0, 0};
    LzJob job;
    job.in = c.in.data();
    job.n = n;
    job.sorted = c.sorted.data();
    job.rank = c.rank.data();
    job.hib = c.hib.data();
    job.cnt = c.cnt.data();
    job.dir = nullptr;
    g_dir = c.dir.data();
    job.r2 = c.r2.empty() ? nullptr : c.r2.data();
    job.stair_min = g_stair_min;
    job.syms = syms.data();
    job.blocks = recs.data();
    job.out = &po;
    job.cfg = level_cfg(level);
    job.strategy = (uint32_t)strategy;
    job.more = 0;
    job.sched = nullptr;
    job.nsched = 0;
    job.n0 = n;
    job.ntot = n;
    run_parse(job);

    ZdBuf buf;
    memset(&buf, 0, sizeof buf);
    buf.in_len = n;
    buf.max_blocks = max_blocks;
    buf.out_cap = out_cap;
    buf.level = (uint32_t)level;
    buf.wrap = (uint32_t)wrap;
    buf.strategy = (uint32_t)strategy;
    buf.wbits = (uint32_t)wb;
    ZdResult res;
    memset(&res, 0, sizeof res);
    CkLds ck;
    res.adler = wrap == 1 ? ck_adler32(c.in.data(), n) : wrap == 2 ? ck_crc32(c.in.data(), n, &ck) : 0;
    for (uint32_t b = 0; b < po.nblocks && b < max_blocks; b++) {
        HpLds hl;
        memset(&hl, 0x5A, sizeof hl);
        huff_plan_block(syms.data() + recs[b].sym_begin, &recs[b], (uint32_t)strategy, &plans[b], &hl);
    }
    std::vector<uint32_t> outw(((size_t)out_cap + 64) / 4 + 4, 0xCDCDCDCD);
    layout_buffer(&buf, &po, recs.data(), plans.data(), &res, (uint8_t *)outw.data());
    for (uint32_t b = 0; b < po.nblocks && b < max_blocks; b++) {
        BeLds bl;
        memset(&bl, 0x77, sizeof bl);
        emit_block(c.in.data(), syms.data() + recs[b].sym_begin, &recs[b], &plans[b], outw.data(), &bl);
    }
    *out_len = res.out_len;
    if (res.status == 0)
        memcpy(out, outw.data(), res.out_len);

    /* k_verify_keep: one thread per block slot */
    std::vector<DvfBlock> facts(max_blocks);
    memset(facts.data(), 0xEE, sizeof(DvfBlock) * max_blocks);
    uint32_t nblk = 0xEEEEEEEEu;
    for (uint32_t j = 0; j < max_blocks; j++)
        dvf_keep(&buf, &po, recs.data(), plans.data(), &res, j, facts.data(), &nblk);
    for (uint32_t b = 0; b < nblk && b < blocks_cap; b++)
        memcpy(blocks + 4 * b, &facts[b], sizeof(DvfBlock));
    *nblocks = nblk;
    return res.status;
}

/* zsc_hip_deflate_plan_verify for one buffer: k_verify_blocks, then k_verify_finish.
 *   in, n                 the input to verify against
 *   stream, stream_cap    the stream and the room it lies in (the plan's out_caps[i]); both are copied to
 *                         allocations of exactly their size, so that a sanitizer sees any read outside
 *   out_len, status       the plan's result for the buffer
 *   blocks, nblocks       the kept facts
 *   result                verdict, block, bit_off, in_pos */
extern "C" void emu_verify_check(const uint8_t *in, uint32_t n, const uint8_t *stream, uint32_t stream_cap,
                                 uint32_t out_len, int status, int level, int window_bits, int mem_level, int strategy,
                                 const uint32_t *blocks, uint32_t nblocks, int32_t *result)
{
    int wrap, wb;
    DvfResult r;
    r.verdict = DVF_SKIPPED;
    r.block = DVF_NONE;
    r.bit_off = r.in_pos = 0;
    if (vf_params(level, window_bits, mem_level, &wrap, &wb)) {
        uint8_t *src_in = (uint8_t *)malloc(n ? n : 1), *src_out = (uint8_t *)malloc(stream_cap ? stream_cap : 1);
        if (n)
            memcpy(src_in, in, n);
        if (stream_cap)
            memcpy(src_out, stream, stream_cap);
        DvfBuf vb;
        vb.in_off = vb.out_off = 0;
        vb.in_len = n;
        vb.out_cap = stream_cap;
        vb.first = 0;
        vb.max_blocks = n / ((1u << (mem_level + 6)) - 1u) + 2;
        if (nblocks > vb.max_blocks)
            nblocks = 0; /* (k_verify_finish) */
        std::vector<DvfBlock> facts(nblocks ? nblocks : 1);
        if (nblocks)
            memcpy(facts.data(), blocks, sizeof(DvfBlock) * nblocks);
        std::vector<DvfVerdict> verd(nblocks ? nblocks : 1);
        memset(verd.data(), 0xEE, sizeof(DvfVerdict) * verd.size());
        ZdResult res;
        memset(&res, 0, sizeof res);
        res.status = status;
        res.out_len = out_len;
        res.adler = 0xDEADBEEFu; /* (not the verification's business) */
        for (uint32_t j = 0; j < nblocks; j++) {
            DvfLds *lds = (DvfLds *)malloc(sizeof(DvfLds));
            memset(lds, 0x5A, sizeof *lds);
            dvf_block_item(src_in, src_out, &vb, facts.data(), nblocks, j, res.out_len, (uint32_t)wrap, (uint32_t)wb, lds,
                           verd.data());
            free(lds);
        }
        dvf_finish(src_out, &vb, facts.data(), verd.data(), nblocks, &res, (uint32_t)wrap, (uint32_t)wb, (uint32_t)level,
                   (uint32_t)strategy, &r);
        free(src_in);
        free(src_out);
    }
    result[0] = r.verdict;
    result[1] = (int32_t)r.block;
    result[2] = (int32_t)r.bit_off;
    result[3] = (int32_t)r.in_pos;
}
