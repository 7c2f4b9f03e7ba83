/*
 * emu_resync.cpp -- TEST INFRASTRUCTURE ONLY: the resync inflate path of one stream, kernel by kernel,
 * on the lane emulation (wave.h, -DZSC_WAVE_EMU): scan -> setup -> scan -> count -> resolve -> write ->
 * finish -> the serial decoder for a stream that did not finish, as the runtime enqueues them
 * (zsc_hip_runtime.hip, sec_enqueue and k_inflate).  The serial decoder also runs on its own, so that
 * the two implementations' error counts can be compared.
 */
#define ZSC_WAVE_EMU 1
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../../zsc_amd/csrc/inflate_resync.h"
#include "../../zsc_amd/csrc/inflate_plan_layout.h"

static uint32_t g_work_mul = SEC_WORK_MUL, g_work_add = SEC_WORK_ADD;
/* the count pass's work bound (tests make it small to reach it with small streams) */
extern "C" void emu_rsy_set_work_bound(uint32_t mul, uint32_t add)
{
    g_work_mul = mul;
    g_work_add = add;
}

/* zsc_uncompress on the serial decoder, as k_inflate and its relaunches run it: the error count is
 * InfResume.errors */
static void serial(const InfJob &job, InfLds *lds, InfResult *res, InfResume *rs)
{
    for (uint32_t round = 0; round < job.n / 4u + 2u; round++)
        if (!inflate_stream(job, lds, res, rs))
            return;
}

/* one stream: status as zsc_uncompress2, *out_len, *consumed, *nsec (chain entries decoded in
 * parallel), *errors (InfResume.errors after the plan: the resync path's count, or the serial
 * decoder's for a stream it finished), *serial_errors (the serial decoder's count on its own) */
extern "C" int emu_rsy_uncompress(const uint8_t *src, uint32_t n, int window_bits, uint8_t *dst, uint32_t cap,
                                  uint32_t *out_len, uint32_t *consumed, uint32_t *nsec, uint32_t *errors,
                                  uint32_t *serial_errors)
{
    std::vector<uint8_t> in((size_t)n + 64, 0);
    memcpy(in.data(), src, n);
    std::vector<uint8_t> out((size_t)cap + 64, 0xEE);

    const uint64_t off0 = 0;
    InfLayout L; /* the runtime's layout of a batch of this one stream */
    sec_layout(1, &n, &off0, &off0, &cap, L);
    const size_t nt = std::max<size_t>(1, L.tiles.size()), nc = L.pool;
    std::vector<uint32_t> tile_cnt(nt, 0x5a5a5a5au), tile_off(nt, 0x5a5a5a5au);
    uint32_t scount = 0, nsec1 = 0, active = 0x5a5a5a5au, q[4] = {0, 0, 0, 0};
    IsecStream st;
    memset(&st, 0x5a, sizeof st);
    IrsyStream rst;
    memset(&rst, 0x5a, sizeof rst);
    std::vector<uint32_t> cstart(nc, 0x5a5a5a5au), cstop(nc, 0x5a5a5a5au), clink(nc, 0x5a5a5a5au),
        clen(nc, 0x5a5a5a5au), chain_k(nc, 0x5a5a5a5au), chain_off(nc, 0x5a5a5a5au), chain_ck(nc, 0x5a5a5a5au),
        chain_fl(nc, 0x5a5a5a5au);
    std::vector<uint64_t> cerr(nc, 0x5a5a5a5a5a5a5a5aull);
    IrsyPlan R;
    IsecPlan &P = R.sp;
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
    R.cerr = cerr.data();
    R.chain_fl = chain_fl.data();
    R.rst = &rst;

    InfLds *lds = (InfLds *)malloc(sizeof(InfLds));
    memset(lds, 0x3C, sizeof(InfLds));
    static uint32_t crc_table[1][256];
    lds->cktab = crc_table;
    InfSecErr si;
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
    rsy_count_worker(R, in.data(), lds, &si);
    for (uint32_t a = 0; a < q[0]; a++)
        rsy_resolve(R, in.data(), a);
    rsy_write_worker(R, in.data(), out.data(), lds, &si);
    for (uint32_t a = 0; a < q[0]; a++)
        rsy_finish(R, in.data(), &res, &resume, a);
    if (resume.state != 2u) {
        /* the serial decoder, from the start (k_inflate and its relaunches) */
        InfJob job = {in.data(), n, out.data(), cap, window_bits};
        serial(job, lds, &res, &resume);
    }
    *errors = resume.errors;
    /* and the serial decoder alone */
    {
        std::vector<uint8_t> out2((size_t)cap + 64, 0xEE);
        InfJob job = {in.data(), n, out2.data(), cap, window_bits};
        InfResult r2;
        InfResume rs2;
        memset(&r2, 0, sizeof r2);
        memset(&rs2, 0, sizeof rs2);
        serial(job, lds, &r2, &rs2);
        *serial_errors = rs2.errors;
    }
    free(lds);
    *nsec = nsec1;
    *out_len = res.out_len;
    *consumed = res.consumed;
    memcpy(dst, out.data(), res.out_len <= cap ? res.out_len : cap);
    return res.status;
}
