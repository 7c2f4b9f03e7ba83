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
#include "../../zsc_amd/csrc/inflate_plan_layout.h"

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

    const uint64_t off0 = 0;
    InfLayout L; /* the runtime's layout of a batch of this one stream */
    sec_layout(1, &n, &off0, &off0, &cap, L);
    if (g_pool)
        L.pool = g_pool;
    const size_t nt = std::max<size_t>(1, L.tiles.size()), nc = L.pool;
    std::vector<uint32_t> tile_cnt(nt, 0x5a5a5a5au), tile_off(nt, 0x5a5a5a5au);
    uint32_t scount = 0, nsec1 = 0, active = 0x5a5a5a5au, q[4] = {0, 0, 0, 0};
    IsecStream st;
    memset(&st, 0x5a, sizeof st);
    std::vector<uint32_t> cstart(nc, 0x5a5a5a5au), cstop(nc, 0x5a5a5a5au), clink(nc, 0x5a5a5a5au),
        clen(nc, 0x5a5a5a5au), chain_k(nc, 0x5a5a5a5au), chain_off(nc, 0x5a5a5a5au), chain_ck(nc, 0x5a5a5a5au);
    IsecPlan P;
    InfPlanMem m = {};
    m.items = L.items.data();
    m.tiles = L.tiles.data();
    m.tile_cnt = tile_cnt.data();
    m.tile_off = tile_off.data();
    m.scount = &scount;
    m.nsec = &nsec1;
    m.st = &st;
    m.active = &active;
    m.q = q;
    m.cstart = cstart.data();
    m.cstop = cstop.data();
    m.clink = clink.data();
    m.clen = clen.data();
    m.chain_k = chain_k.data();
    m.chain_off = chain_off.data();
    m.chain_ck = chain_ck.data();
    sec_plan_view(P, m, L, window_bits, g_work_mul, g_work_add);

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
