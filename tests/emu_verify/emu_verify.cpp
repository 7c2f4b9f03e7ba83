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

/* the runtime's parameter folding (a level must be said); 0 where the plan would not be made */
static int vf_params(int level, int window_bits, int mem_level, int strategy, int *wrap, int *wb)
{
    return level >= 1 && dpl_fold_params(&level, window_bits, mem_level, strategy, wrap, wb);
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
    if (!vf_params(level, window_bits, mem_level, strategy, &wrap, &wb))
        return -2;
    emu_set_params(wb, mem_level);

    EmuBuf e;
    e.open(src, n, level, wrap, strategy, out_cap);
    run_parse(e.job);
    e.emit();
    e.give(out, out_len);
    const uint32_t max_blocks = e.buf.max_blocks;

    /* k_verify_keep: one thread per block slot */
    std::vector<DvfBlock> facts(max_blocks);
    memset(facts.data(), 0xEE, sizeof(DvfBlock) * max_blocks);
    uint32_t nblk = 0xEEEEEEEEu;
    for (uint32_t j = 0; j < max_blocks; j++)
        dvf_keep(&e.buf, &e.po, e.recs.data(), e.plans.data(), &e.res, j, facts.data(), &nblk);
    for (uint32_t b = 0; b < nblk && b < blocks_cap; b++)
        memcpy(blocks + 4 * b, &facts[b], sizeof(DvfBlock));
    *nblocks = nblk;
    return e.res.status;
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
    if (vf_params(level, window_bits, mem_level, strategy, &wrap, &wb)) {
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
        vb.max_blocks = dpl_max_blocks(n, mem_level, 0);
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
