/*
 * emu_dindex.cpp -- TEST INFRASTRUCTURE ONLY.
 *
 * The deflate pipeline of tests/emu with the seek-point index on top (zsc_amd/csrc/deflate_index.h), in
 * the lane emulation: what zsc_hip_deflate_plan_run enqueues for one buffer of a plan with the index
 * enabled, kernel by kernel, and what zsc_hip_deflate_plan_index_export makes of it.  Of inflate_index.h
 * only the host half is compiled (the blob's format); the blobs are decoded by tests/emu_index.
 */
#define ZIDX_HOST_ONLY 1
#include "../emu/emu_pipeline.cpp"
#include "../../zsc_amd/csrc/deflate_index.h"

/* Returns the buffer's status.  window_bits as zsc_compress2 takes it (the wrapper folded in).
 *   out, *out_len        the stream (status 0)
 *   blob, *blob_len      the index; *blob_len = 0 where there is none, the bytes needed where blob_cap is short
 *   blocks, *nblocks     (bit_off, in_begin, in_len, type) of the stream's blocks, at most blocks_cap of them */
extern "C" int emu_dindex_compress(const uint8_t *src, uint32_t n, int level, int window_bits, int mem_level,
                                   int strategy, uint32_t chunk_bytes, uint32_t out_cap, uint8_t *out,
                                   uint32_t *out_len, uint8_t *blob, uint64_t blob_cap, uint64_t *blob_len,
                                   uint32_t *blocks, uint32_t blocks_cap, uint32_t *nblocks)
{
    *out_len = 0;
    *blob_len = 0;
    *nblocks = 0;
    /* the runtime's offloadable() */
    int wrap = 1, wb = window_bits;
    if (wb < 0) {
        wrap = 0;
        wb = -wb;
    } else if (wb > 15) {
        wrap = 2;
        wb -= 16;
    }
    if (wb == 8 && wrap == 1)
        wb = 9;
    if (level < 1 || level > 9 || wb < 9 || wb > 15 || mem_level < 1 || mem_level > 9)
        return -2;
    emu_set_params(wb, mem_level);
    chunk_bytes = dix_chunk_bytes(chunk_bytes);

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

    /* the index of the sub-batch: k_index_reach, k_index_points, k_index_check */
    const uint32_t nb = po.nblocks <= max_blocks ? po.nblocks : 0u;
    std::vector<uint32_t> reach(max_blocks, 0xDDDDDDDDu);
    for (uint32_t b = 0; b < nb; b++)
        reach[b] = dix_block_reach(syms.data() + recs[b].sym_begin, &recs[b], &plans[b]);
    const uint32_t cap = out_cap / chunk_bytes + 1u;
    std::vector<ZidxRec> pts(cap);
    memset(pts.data(), 0xEE, sizeof(ZidxRec) * cap);
    uint32_t npts = 0xEEEEEEEEu;
    dix_points(&buf, &po, recs.data(), plans.data(), reach.data(), &res, chunk_bytes, pts.data(), cap, &npts);
    for (uint32_t p = 0; p < npts; p++)
        pts[p].ck = dix_piece_check(c.in.data(), &pts[p], (uint32_t)wrap, &ck);

    for (uint32_t b = 0; b < nb && b < blocks_cap; b++) {
        blocks[4 * b + 0] = plans[b].bit_off;
        blocks[4 * b + 1] = recs[b].in_begin;
        blocks[4 * b + 2] = recs[b].in_len;
        blocks[4 * b + 3] = plans[b].type;
    }
    *nblocks = nb;

    /* zsc_hip_deflate_plan_index_export */
    if (res.status != 0 || npts == 0u)
        return res.status;
    uint64_t wbytes = 0;
    for (uint32_t p = 0; p < npts; p++) {
        pts[p].woff = wbytes;
        wbytes += pts[p].wlen;
    }
    const uint64_t bytes = zidx_blob_bytes(npts, wbytes);
    *blob_len = bytes;
    if (blob_cap < bytes)
        return res.status;
    /* (the export's input is a copy of exactly the buffer's bytes, so that a sanitizer sees a read outside) */
    std::vector<uint8_t> in(src, src + n);
    std::vector<uint8_t> wins(wbytes);
    for (uint32_t p = 0; p < npts; p++)
        for (uint32_t t = 0; t < 4; t++)
            dix_gather(in.data(), &pts[p], wins.data(), t, 4);
    if (wbytes)
        memcpy(blob + zidx_blob_bytes(npts, 0), wins.data(), wbytes);
    const ZidxInfo h = dix_blob_info((uint32_t)wrap, wb, chunk_bytes, res.out_len, n, npts);
    zidx_write_head(blob, &h, pts.data());
    zidx_seal(blob, bytes);
    return res.status;
}
