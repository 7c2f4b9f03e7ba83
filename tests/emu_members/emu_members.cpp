/*
 * emu_members.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone program that inflates multi-member gzip
 * files with the members path (zsc_amd/csrc/inflate_members.h) on the lane emulation (wave.h,
 * -DZSC_WAVE_EMU), step by step as the runtime enqueues them (zsc_hip_runtime.hip, mem_enqueue):
 * scan -> setup -> scan -> claims -> count -> resolve -> write -> finish -> serial.
 *
 * usage: emu_members CASES OUTPUT
 * CASES holds records of int32 window_bits, uint32 dest_cap, uint32 flags (1: size-only, 2: claims off),
 * uint32 pool (0: the runtime's), uint32 work_mul, uint32 work_add (both 0xFFFFFFFF: the runtime's),
 * uint32 n and the n bytes of the file.  One line per record:
 *     status out_len consumed members prefix claimed canary
 * (canary: the 64 bytes behind dest_cap are untouched) and the out_len output bytes appended to OUTPUT
 * (none in size-only mode).
 */
#define ZSC_WAVE_EMU 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "../../zsc_amd/csrc/inflate_members.h"
#include "../../zsc_amd/csrc/inflate_plan_layout.h"

struct Rec {
    int32_t window_bits;
    uint32_t cap, flags, pool, work_mul, work_add, n;
};

struct Out {
    int status;
    uint32_t out_len, consumed, members, prefix, claimed, canary;
};

static Out run_one(const Rec &h, const uint8_t *src, FILE *fo)
{
    const uint32_t n = h.n, cap = h.cap;
    const bool size_only = (h.flags & 1u) != 0;
    std::vector<uint8_t> in((size_t)n + 64, 0);
    if (n)
        memcpy(in.data(), src, n);
    std::vector<uint8_t> out(size_only ? 64 : (size_t)cap + 64, 0xEE);

    const uint64_t off0 = 0;
    InfLayout L; /* the runtime's layout of a batch of this one file */
    mem_layout(1, &n, &off0, &off0, &cap, L);
    if (h.pool)
        L.pool = h.pool;
    const size_t nt = std::max<size_t>(1, L.tiles.size()), nc = L.pool;
    std::vector<uint32_t> tile_cnt(nt, 0x5a5a5a5au), tile_off(nt, 0x5a5a5a5au);
    uint32_t scount = 0, nsec1 = 0, active = 0x5a5a5a5au, q[4] = {0, 0, 0, 0};
    IsecStream st;
    memset(&st, 0x5a, sizeof st);
    std::vector<uint32_t> cstart(nc, 0x5a5a5a5au), cstop(nc, 0x5a5a5a5au), clink(nc, 0x5a5a5a5au),
        clen(nc, 0x5a5a5a5au), chain_k(nc, 0x5a5a5a5au), chain_off(nc, 0x5a5a5a5au), chain_ck(nc, 0x5a5a5a5au);
    MemFile mf = {0, 0, 0, 0};
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
    MemPlan M;
    const bool dflt = h.work_mul == 0xffffffffu && h.work_add == 0xffffffffu;
    mem_plan_view(M, m, L, h.window_bits, &mf, size_only, (h.flags & 2u) == 0, dflt ? SEC_WORK_MUL : h.work_mul,
                  dflt ? SEC_WORK_ADD : h.work_add);
    const IsecPlan &P = M.sp;

    InfLds *lds = (InfLds *)malloc(sizeof(InfLds));
    memset(lds, 0x3C, sizeof(InfLds));
    static uint32_t crc_table[1][256];
    lds->cktab = crc_table;
    InfResult r, res;
    InfResume rs, resume;
    memset(&r, 0, sizeof r);
    memset(&res, 0, sizeof res);
    memset(&rs, 0, sizeof rs);
    memset(&resume, 0, sizeof resume);

    for (uint32_t t = 0; t < P.ntiles; t++)
        mem_scan_tile(M, in.data(), t, 0);
    for (uint32_t a = 0; a < q[0]; a++)
        sec_setup(P, a);
    for (uint32_t t = 0; t < P.ntiles; t++)
        mem_scan_tile(M, in.data(), t, 1);
    for (uint32_t a = 0; a < q[0]; a++)
        mem_claims(M, in.data(), a);
    mem_count_worker(M, in.data(), lds, &r, &rs);
    for (uint32_t a = 0; a < q[0]; a++)
        mem_resolve(M, a);
    if (!size_only)
        mem_write_worker(M, in.data(), out.data(), lds, &r, &rs);
    for (uint32_t a = 0; a < q[0]; a++)
        mem_finish(M, &res, &resume, a);
    if (size_only)
        mem_serial<true>(M, in.data(), nullptr, lds, &r, &rs, &res, &resume, 0);
    else
        mem_serial<false>(M, in.data(), out.data(), lds, &r, &rs, &res, &resume, 0);
    free(lds);

    Out o;
    o.status = res.status;
    o.out_len = res.out_len;
    o.consumed = res.consumed;
    o.members = mf.members;
    o.prefix = nsec1;
    o.claimed = mf.claimed;
    o.canary = 1;
    for (size_t i = out.size() - 64; i < out.size(); i++)
        if (out[i] != 0xEE)
            o.canary = 0;
    if (!size_only && res.out_len)
        fwrite(out.data(), 1, std::min<size_t>(res.out_len, cap), fo);
    return o;
}

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: %s CASES OUTPUT\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    FILE *fo = fopen(argv[2], "wb");
    if (!f || !fo) {
        perror(f ? argv[2] : argv[1]);
        return 2;
    }
    for (;;) {
        Rec h;
        const size_t got = fread(&h, 4, 7, f);
        if (got == 0)
            break;
        if (got != 7) {
            fprintf(stderr, "short record header\n");
            return 2;
        }
        std::vector<uint8_t> s((size_t)h.n + 1);
        if (h.n && fread(s.data(), 1, h.n, f) != h.n) {
            fprintf(stderr, "short record\n");
            return 2;
        }
        const Out o = run_one(h, s.data(), fo);
        printf("%d %u %u %u %u %u %u\n", o.status, o.out_len, o.consumed, o.members, o.prefix, o.claimed, o.canary);
    }
    fclose(f);
    fclose(fo);
    return 0;
}
