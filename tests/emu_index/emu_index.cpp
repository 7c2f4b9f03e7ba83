/*
 * emu_index.cpp -- TEST INFRASTRUCTURE ONLY: the indexed inflate path of one stream on the lane
 * emulation (wave.h, -DZSC_WAVE_EMU).  emu_idx_build runs the chunks path with the index enabled
 * (setup -> scan -> count -> want -> retry -> resolve -> window -> write -> finish -> the serial decoder)
 * and exports the blob; emu_idx_uncompress runs the indexed path: k_idx_write's worker, finish, and the
 * serial decoder for what is left, as the runtime enqueues them (zsc_hip_runtime.hip).  Every buffer
 * the path may touch is allocated at its exact size, so that AddressSanitizer sees a stray access.
 */
#define ZSC_WAVE_EMU 1
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../../zsc_amd/csrc/inflate_index.h"
#include "../../zsc_amd/csrc/inflate_plan_layout.h"

static InfLds *new_lds()
{
    InfLds *lds = (InfLds *)malloc(sizeof(InfLds));
    memset(lds, 0x3C, sizeof(InfLds));
    static uint32_t crc_table[1][256];
    lds->cktab = crc_table;
    return lds;
}

extern "C" int emu_idx_validate(const uint8_t *blob, uint64_t len) { return zidx_validate(blob, len, nullptr); }

/* info[8]: window_bits, kind, head, chunk_bytes, consumed, total, trailer, npoints; 1 if the blob is valid */
extern "C" int emu_idx_info(const uint8_t *blob, uint64_t len, uint32_t *info)
{
    ZidxInfo h;
    if (!zidx_validate(blob, len, &h))
        return 0;
    const uint32_t v[8] = {(uint32_t)h.window_bits, h.kind, h.head, h.chunk_bytes, h.consumed, h.total, h.trailer, h.npoints};
    memcpy(info, v, sizeof v);
    return 1;
}

/* out[4]: first piece, piece count, piece_begin, piece_len; 1, 0 for a range outside the output, -1 for a bad blob */
extern "C" int emu_idx_range(const uint8_t *blob, uint64_t len, uint64_t begin, uint64_t n, uint32_t *out)
{
    ZidxInfo h;
    if (!zidx_validate(blob, len, &h))
        return -1;
    return zidx_range(blob, &h, begin, n, &out[0], &out[1], &out[2], &out[3]);
}

/* The chunks path with the index enabled, then the export.  Results as emu_chk_uncompress; *blob_len:
 * bytes of the blob (0: no index -- the serial decoder produced the stream), written to blob if
 * blob_cap holds it. */
extern "C" int emu_idx_build(const uint8_t *src, uint32_t n, int window_bits, uint8_t *dst, uint32_t cap,
                             uint32_t chunk_bytes, uint32_t *out_len, uint32_t *consumed, uint32_t *npieces,
                             uint8_t *blob, uint64_t blob_cap, uint64_t *blob_len)
{
    std::vector<uint8_t> in((size_t)n + 64, 0);
    memcpy(in.data(), src, n);
    std::vector<uint8_t> out((size_t)cap + 64, 0xEE);
    const uint32_t cb = chunk_bytes == 0 ? CHK_DEFAULT_BYTES : chunk_bytes;

    const uint64_t off0 = 0;
    InfLayout L; /* the runtime's layout of a batch of this one stream */
    chk_layout(1, &n, &off0, &off0, &cap, cb, [&](uint32_t) { return cap < 0x80000000u; }, L);
    const size_t ch = std::max<size_t>(1, L.pool);
    uint32_t nsec1 = 0, active = 0, q[4] = {0, 0, 0, 0};
    IsecStream st;
    memset(&st, 0x5a, sizeof st);
    std::vector<uint32_t> cstop(ch, 0x5a5a5a5au), clink(ch, 0x5a5a5a5au), clen(ch, 0x5a5a5a5au),
        chain_k(ch, 0x5a5a5a5au), chain_off(ch, 0x5a5a5a5au), chain_ck(ch, 0x5a5a5a5au), cused(ch, 0x5a5a5a5au),
        creach(ch, 0x5a5a5a5au), want(ch, 0x5a5a5a5au);
    std::vector<uint64_t> cand(ch * INF_PC_CANDS, 0x5a5a5a5a5a5a5a5aull);
    std::vector<uint16_t> ring(ch * INF_WIN, 0x5a5a);
    std::vector<uint8_t> win(ch * INF_WIN, 0x5a);
    IchkPlan P;
    memset(&P, 0, sizeof P);
    InfPlanMem m = {};
    m.items = L.items.data();
    m.tiles = L.tiles.data();
    m.nsec = &nsec1;
    m.st = &st;
    m.active = &active;
    m.q = q;
    m.cstop = cstop.data();
    m.clink = clink.data();
    m.clen = clen.data();
    m.chain_k = chain_k.data();
    m.chain_off = chain_off.data();
    m.chain_ck = chain_ck.data();
    m.cand = cand.data();
    m.cused = cused.data();
    m.creach = creach.data();
    m.want = want.data();
    m.ring = ring.data();
    m.win = win.data();
    chk_plan_view(P, m, L, window_bits, cb);
    P.keep_index = 1;

    InfLds *lds = new_lds();
    InfSecInfo si;
    InfPiece pc;
    InfResult res;
    memset(&res, 0, sizeof res);
    InfResume resume;
    memset(&resume, 0, sizeof resume);
    if (P.nactive) {
        chk_setup(P, 0);
        for (uint32_t t = 0; t < P.sp.ntiles; t++)
            chk_scan(P, in.data(), t);
        chk_count_worker<false>(P, in.data(), lds, &si, &pc);
        chk_want(P, 0);
        chk_count_worker<true>(P, in.data(), lds, &si, &pc);
        chk_resolve(P, in.data(), lds, &si, &pc, 0);
        chk_windows(P, 0, 0, 1, [] {});
        chk_write_worker(P, in.data(), out.data(), lds, &si, &pc);
        sec_finish(P.sp, in.data(), &res, &resume, 0);
    }
    if (resume.state != 2u) {
        InfJob job = {in.data(), n, out.data(), cap, window_bits};
        inflate_with_resync(job, lds, &res);
    }
    free(lds);
    *npieces = nsec1;
    *out_len = res.out_len;
    *consumed = res.consumed;
    memcpy(dst, out.data(), res.out_len <= cap ? res.out_len : cap);

    /* the export (zsc_hip_inflate_plan_index_export): records, a prefix sum of the window lengths,
     * the gather of the windows, the blob */
    *blob_len = 0;
    if (nsec1) {
        std::vector<ZidxRec> recs(nsec1);
        uint64_t wbytes = 0;
        for (uint32_t i = 0; i < nsec1; i++) {
            idx_record(P, 0, i, &recs[i]);
            recs[i].woff = wbytes;
            wbytes += recs[i].wlen;
        }
        const uint64_t len = zidx_blob_bytes(nsec1, wbytes);
        *blob_len = len;
        if (len <= blob_cap) {
            std::vector<uint8_t> wins((size_t)wbytes);
            for (uint32_t i = 0; i < nsec1; i++)
                idx_gather(P, 0, i, &recs[i], wins.data(), 0, 1);
            ZidxInfo h;
            h.window_bits = window_bits;
            h.kind = window_bits < 0 ? 0u : (st.head & 1u) ? 2u : 1u;
            h.head = st.head;
            h.chunk_bytes = cb;
            h.consumed = res.consumed;
            h.total = st.total;
            h.trailer = st.trailer;
            h.npoints = nsec1;
            zidx_write_head(blob, &h, recs.data());
            if (wbytes)
                memcpy(blob + zidx_blob_bytes(nsec1, 0), wins.data(), (size_t)wbytes);
            zidx_seal(blob, len);
        }
    }
    return res.status;
}

/* One stream through an indexed plan (blob may be NULL: no index).  has_range: a range item.  Returns
 * the item's status, or -100 where create refuses the plan (a range outside the output). */
extern "C" int emu_idx_uncompress(const uint8_t *src, uint32_t n, int window_bits, uint8_t *dst, uint32_t cap,
                                  const uint8_t *blob_in, uint64_t blob_len, int has_range, uint64_t rbegin,
                                  uint64_t rlen, uint32_t *out_len, uint32_t *consumed, uint32_t *npieces)
{
    /* exact-size copies: a read past the stream's 64 spare bytes, the blob or the output is a finding */
    uint8_t *in = (uint8_t *)calloc((size_t)n + 64, 1);
    memcpy(in, src, n);
    uint8_t *blob = blob_in ? (uint8_t *)malloc((size_t)blob_len + 1) : nullptr;
    if (blob)
        memcpy(blob, blob_in, (size_t)blob_len);
    uint8_t *out = (uint8_t *)malloc((size_t)cap + 64);
    memset(out, 0xEE, (size_t)cap + 64);

    IdxBuild B;
    const int rc = B.add(n, 0, cap, 0, window_bits, blob, blob_len, has_range != 0, rbegin, rlen);
    free(blob); /* (create uploads what it needs: nothing of the blob is read afterwards) */
    if (rc != 0) {
        free(in);
        free(out);
        return -100;
    }
    B.finish();
    uint32_t nsec1 = 0, done1 = 0, q[4] = {(uint32_t)B.active.size(), 0, 0, 0};
    std::vector<uint32_t> chain_ck(std::max<size_t>(1, B.pieces.size()), 0x5a5a5a5au);
    IidxPlan P;
    memset(&P, 0, sizeof P);
    P.sp.items = B.items.data();
    P.sp.nsec = &nsec1;
    P.sp.st = B.st.data();
    P.sp.active = B.active.data();
    P.sp.q = q;
    P.sp.clen = B.clen.data();
    P.sp.chain_k = B.chain_k.data();
    P.sp.chain_ck = chain_ck.data();
    P.sp.count = 1;
    P.sp.window_bits = window_bits;
    P.pieces = B.pieces.data();
    P.units = B.units.data();
    P.xs = B.xs.data();
    P.done = &done1;
    P.cand = B.cand.data();
    P.win = B.win.data();
    P.nunits = (uint32_t)B.units.size();

    InfLds *lds = new_lds();
    InfSecInfo si;
    InfPiece pc;
    InfResult res = B.res0[0];
    InfResume resume;
    memset(&resume, 0, sizeof resume);
    resume.state = B.state0[0];
    idx_write_worker(P, in, out, lds, &si, &pc, &res, &resume);
    for (uint32_t a = 0; a < B.active.size(); a++)
        sec_finish(P.sp, in, &res, &resume, a);
    if (resume.state != 2u) {
        InfJob job = {in, n, out, cap, window_bits};
        inflate_with_resync(job, lds, &res);
    }
    free(lds);
    *npieces = nsec1;
    *out_len = res.out_len;
    *consumed = res.consumed;
    memcpy(dst, out, res.out_len <= cap ? res.out_len : cap);
    free(in);
    free(out);
    return res.status;
}
