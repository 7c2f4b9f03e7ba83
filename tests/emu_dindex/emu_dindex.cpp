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
    int wrap, wb;
    if (level < 1 || !dpl_fold_params(&level, window_bits, mem_level, strategy, &wrap, &wb))
        return -2;
    emu_set_params(wb, mem_level);
    chunk_bytes = dix_chunk_bytes(chunk_bytes);

    EmuBuf e;
    e.open(src, n, level, wrap, strategy, out_cap);
    run_parse(e.job);
    e.emit();
    e.give(out, out_len);
    const ZdParseOut &po = e.po;
    const ZdBuf &buf = e.buf;
    const ZdResult &res = e.res;
    const uint32_t max_blocks = buf.max_blocks;
    CkLds ck;

    /* the index of the sub-batch: k_index_reach, k_index_points, k_index_check */
    const uint32_t nb = po.nblocks <= max_blocks ? po.nblocks : 0u;
    std::vector<uint32_t> reach(max_blocks, 0xDDDDDDDDu);
    for (uint32_t b = 0; b < nb; b++)
        reach[b] = dix_block_reach(e.syms.data() + e.recs[b].sym_begin, &e.recs[b], &e.plans[b]);
    const uint32_t cap = out_cap / chunk_bytes + 1u;
    std::vector<ZidxRec> pts(cap);
    memset(pts.data(), 0xEE, sizeof(ZidxRec) * cap);
    uint32_t npts = 0xEEEEEEEEu;
    dix_points(&buf, &po, e.recs.data(), e.plans.data(), reach.data(), &res, chunk_bytes, pts.data(), cap, &npts);
    for (uint32_t p = 0; p < npts; p++)
        pts[p].ck = dix_piece_check(e.c.in.data(), &pts[p], (uint32_t)wrap, &ck);

    for (uint32_t b = 0; b < nb && b < blocks_cap; b++) {
        blocks[4 * b + 0] = e.plans[b].bit_off;
        blocks[4 * b + 1] = e.recs[b].in_begin;
        blocks[4 * b + 2] = e.recs[b].in_len;
        blocks[4 * b + 3] = e.plans[b].type;
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
