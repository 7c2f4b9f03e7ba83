/*
 * emu_sections.cpp -- TEST INFRASTRUCTURE ONLY: the sections inflate path of one stream, kernel by
 * kernel, on the lane emulation (wave.h, -DZSC_WAVE_EMU): scan -> setup -> scan -> count -> resolve
 * -> write -> finish -> the serial decoder for a stream that did not finish, as the runtime
 * enqueues them (zsc_hip_runtime.hip, sec_enqueue and k_inflate).
 */
#define ZSC_WAVE_EMU 1
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../../zsc_amd/csrc/inflate_sections.h"

static uint32_t g_work_mul = SEC_WORK_MUL, g_work_add = SEC_WORK_ADD;
/* the count pass's work bound (tests make it small to reach it with small streams) */
extern "C" void emu_sec_set_work_bound(uint32_t mul, uint32_t add)
{
    g_work_mul = mul;
    g_work_add = add;
}

static uint32_t g_pool = 0;
/* the candidate pool's size (0: what the runtime would give a plan of this one stream) */
extern "C" void emu_sec_set_pool(uint32_t slots) { g_pool = slots; }

extern "C" uint32_t emu_sec_crc32_combine(uint32_t c1, uint32_t c2, uint32_t len2)
{
    return sec_crc32_combine(c1, c2, len2);
}

extern "C" uint32_t emu_sec_adler32_combine(uint32_t a1, uint32_t a2, uint32_t len2)
{
    return sec_adler32_combine(a1, a2, len2);
}

/* one stream: status as zsc_uncompress2, *out_len, *consumed, *nsec (sections decoded in
 * parallel), *ncand (candidate starts found, 0 if the stream had none or too many) */
extern "C" int emu_sec_uncompress(const uint8_t *src, uint32_t n, int window_bits, uint8_t *dst, uint32_t cap,
                                  uint32_t *out_len, uint32_t *consumed, uint32_t *nsec, uint32_t *ncand)
{
    std::vector<uint8_t> in((size_t)n + 64, 0);
    memcpy(in.data(), src, n);
    std::vector<uint8_t> out((size_t)cap + 64, 0xEE);

    IsecItem it = {};
    it.src_off = 0;
    it.dst_off = 0;
    it.src_len = n;
    it.dst_cap = cap;
    it.cap = n / SEC_CAND_DIV + SEC_CAND_MIN;
    it.ntiles = (n + SEC_TILE - 1u) / SEC_TILE;
    std::vector<IsecTile> tiles(std::max(1u, it.ntiles));
    for (uint32_t t = 0; t < it.ntiles; t++)
        tiles[t] = IsecTile{0u, t * SEC_TILE};
    const size_t nt = tiles.size(), nc = g_pool ? g_pool : SEC_POOL_SLOTS((uint64_t)n);
    std::vector<uint32_t> tile_cnt(nt, 0x5a5a5a5au), tile_off(nt, 0x5a5a5a5au);
    uint32_t scount = 0, nsec1 = 0, active = 0x5a5a5a5au, q[4] = {0, 0, 0, 0};
    IsecStream st;
    memset(&st, 0x5a, sizeof st);
    std::vector<uint32_t> cstart(nc, 0x5a5a5a5au), cstop(nc, 0x5a5a5a5au), clink(nc, 0x5a5a5a5au),
        clen(nc, 0x5a5a5a5au), chain_k(nc, 0x5a5a5a5au), chain_off(nc, 0x5a5a5a5au), chain_ck(nc, 0x5a5a5a5au);
    IsecPlan P;
    P.items = &it;
    P.tiles = tiles.data();
    P.tile_cnt = tile_cnt.data();
    P.tile_off = tile_off.data();
    P.scount = &scount;
    P.nsec = &nsec1;
    P.st = &st;
    P.active = &active;
    P.q = q;
    P.cstart = cstart.data();
    P.cstop = cstop.data();
    P.clink = clink.data();
    P.clen = clen.data();
    P.chain_k = chain_k.data();
    P.chain_off = chain_off.data();
    P.chain_ck = chain_ck.data();
    P.count = 1;
    P.ntiles = it.ntiles;
    P.pool = (uint32_t)nc;
    P.window_bits = window_bits;
    P.work_mul = g_work_mul;
    P.work_add = g_work_add;

    InfLds *lds = (InfLds *)malloc(sizeof(InfLds));
    memset(lds, 0x3C, sizeof(InfLds));
    static uint32_t crc_table[1][256];
    lds->cktab = crc_table;
    InfSecInfo si;
    InfResult res;
    memset(&res, 0, sizeof res);
    InfResume resume;
    memset(&resume, 0, sizeof resume);

    for (uint32_t t = 0; t < P.ntiles; t++)
        sec_scan_tile(P, in.data(), t, 0);
    for (uint32_t a = 0; a < q[0]; a++)
        sec_setup(P, a);
    for (uint32_t t = 0; t < P.ntiles; t++)
        sec_scan_tile(P, in.data(), t, 1);
    sec_count_worker(P, in.data(), lds, &si);
    for (uint32_t a = 0; a < q[0]; a++)
        sec_resolve(P, a);
    sec_write_worker(P, in.data(), out.data(), lds, &si);
    for (uint32_t a = 0; a < q[0]; a++)
        sec_finish(P, in.data(), &res, &resume, a);
    *ncand = q[0] ? st.ncand : 0u;
    if (resume.state != 2u) {
        /* the serial decoder, from the start (k_inflate and its relaunches) */
        InfJob job = {in.data(), n, out.data(), cap, window_bits};
        inflate_with_resync(job, lds, &res);
    }
    free(lds);
    *nsec = nsec1;
    *out_len = res.out_len;
    *consumed = res.consumed;
    memcpy(dst, out.data(), res.out_len <= cap ? res.out_len : cap);
    return res.status;
}
