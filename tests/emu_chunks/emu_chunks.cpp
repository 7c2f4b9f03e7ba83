/*
 * emu_chunks.cpp -- TEST INFRASTRUCTURE ONLY: the chunks inflate path of one stream, kernel by kernel,
 * on the lane emulation (wave.h, -DZSC_WAVE_EMU): setup -> scan -> count -> resolve -> window -> write
 * -> finish -> the serial decoder for a stream that did not finish, as the runtime enqueues them
 * (zsc_hip_runtime.hip, chk_enqueue and inflate_launch).
 */
#define ZSC_WAVE_EMU 1
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../../zsc_amd/csrc/inflate_plan_layout.h"

static uint32_t g_work_mul = SEC_WORK_MUL, g_work_add = SEC_WORK_ADD;
/* the count pass's work bound (tests make it small to reach it with small streams) */
extern "C" void emu_chk_set_work_bound(uint32_t mul, uint32_t add)
{
    g_work_mul = mul;
    g_work_add = add;
}

static int g_retry = 1;
/* the want / retry pass on or off (off: resolve repairs every link into a chunk that took another
 * candidate) */
extern "C" void emu_chk_set_retry(int on) { g_retry = on; }

/* the scan's validator at one bit offset */
extern "C" int emu_chk_header_ok(const uint8_t *src, uint32_t n, uint64_t bit)
{
    return inf_dyn_header_ok(src, n, bit);
}

static InfLds *new_lds()
{
    InfLds *lds = (InfLds *)malloc(sizeof(InfLds));
    memset(lds, 0x3C, sizeof(InfLds));
    static uint32_t crc_table[1][256];
    lds->cktab = crc_table;
    return lds;
}

/* the decoder's verdict at one bit offset: decoding raw from there, was the first block a dynamic
 * block whose header passed? */
extern "C" int emu_chk_decoder_header_ok(const uint8_t *src, uint32_t n, uint64_t bit)
{
    std::vector<uint8_t> in((size_t)n + 64, 0);
    memcpy(in.data(), src, n);
    std::vector<uint16_t> ring(INF_WIN);
    const uint64_t none[INF_PC_CANDS] = {INF_PC_NONE, INF_PC_NONE, INF_PC_NONE, INF_PC_NONE};
    InfPiece pc = {};
    pc.base_bit = bit & ~7ull;
    pc.chunk_bits = 1ull << 40;
    pc.cand = none;
    pc.ring = ring.data();
    pc.skip = (uint32_t)(bit & 7u);
    pc.chunk = 0;
    pc.nchunks = 1;
    InfLds *lds = new_lds();
    InfSecInfo si;
    const uint32_t start = (uint32_t)(bit >> 3);
    InfJob job = {in.data() + start, n - start, nullptr, 1u << 20, -15};
    inflate_stream<INF_SEC_BITSTART | INF_SEC_SYM16 | INF_SEC_NOTRAIL>(job, lds, nullptr, nullptr, &si, &pc);
    free(lds);
    return (int)pc.hdr_ok;
}

/* one stream: status as zsc_uncompress2, *out_len, *consumed, *npieces (pieces decoded in parallel),
 * *ncand (candidates the scan found in all chunks) */
extern "C" int emu_chk_uncompress(const uint8_t *src, uint32_t n, int window_bits, uint8_t *dst, uint32_t cap,
                                  uint32_t chunk_bytes, uint32_t *out_len, uint32_t *consumed, uint32_t *npieces,
                                  uint32_t *ncand)
{
    std::vector<uint8_t> in((size_t)n + 64, 0);
    memcpy(in.data(), src, n);
    std::vector<uint8_t> out((size_t)cap + 64, 0xEE);
    const uint32_t cb = chunk_bytes == 0 ? CHK_DEFAULT_BYTES : chunk_bytes; /* (no CHK_MIN_BYTES: tests go smaller) */

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
    chk_plan_view(P, m, L, window_bits, cb, g_work_mul, g_work_add);

    InfLds *lds = new_lds();
    InfSecInfo si;
    InfPiece pc;
    InfResult res;
    memset(&res, 0, sizeof res);
    InfResume resume;
    memset(&resume, 0, sizeof resume);

    *ncand = 0;
    if (P.nactive) {
        chk_setup(P, 0);
        for (uint32_t t = 0; t < P.sp.ntiles; t++)
            chk_scan(P, in.data(), t);
        for (size_t c = 0; c < ch * INF_PC_CANDS; c++)
            *ncand += cand[c] != INF_PC_NONE;
        chk_count_worker<false>(P, in.data(), lds, &si, &pc);
        if (g_retry) {
            chk_want(P, 0);
            chk_count_worker<true>(P, in.data(), lds, &si, &pc);
        }
        chk_resolve(P, in.data(), lds, &si, &pc, 0);
        chk_windows(P, 0, 0, 1, [] {});
        chk_write_worker(P, in.data(), out.data(), lds, &si, &pc);
        sec_finish(P.sp, in.data(), &res, &resume, 0);
    }
    if (resume.state != 2u) {
        /* the serial decoder, from the start (k_inflate and its relaunches) */
        InfJob job = {in.data(), n, out.data(), cap, window_bits};
        inflate_with_resync(job, lds, &res);
    }
    free(lds);
    *npieces = nsec1;
    *out_len = res.out_len;
    *consumed = res.consumed;
    memcpy(dst, out.data(), res.out_len <= cap ? res.out_len : cap);
    return res.status;
}
