/*
 * emu_size.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone program that sizes streams with the size
 * path (zsc_amd/csrc/inflate_size.h) on the lane emulation (wave.h, -DZSC_WAVE_EMU), kernel by kernel
 * as the runtime enqueues them (zsc_hip_runtime.hip, chk_enqueue): setup -> scan -> count -> want ->
 * retry -> resolve -> finish for a stream longer than a chunk, then the whole-stream size decode for a
 * stream that did not finish.
 *
 * usage: emu_size CASES
 * CASES holds records of int32 window_bits, uint32 limit, uint32 chunk_bytes (0xFFFFFFFF: never cut),
 * uint32 n and the n bytes of the stream.  One line per record: status size consumed pieces.
 */
#define ZSC_WAVE_EMU 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "../../zsc_amd/csrc/inflate_size.h"
#include "../../zsc_amd/csrc/inflate_plan_layout.h"

static InfLds *new_lds()
{
    InfLds *lds = (InfLds *)malloc(sizeof(InfLds));
    memset(lds, 0x3C, sizeof(InfLds));
    static uint32_t crc_table[1][256];
    lds->cktab = crc_table;
    return lds;
}

static int size_one(const uint8_t *src, uint32_t n, int window_bits, uint32_t limit, uint32_t cb, uint32_t *out_len,
                    uint32_t *consumed, uint32_t *npieces)
{
    std::vector<uint8_t> in((size_t)n + 64, 0);
    if (n)
        memcpy(in.data(), src, n);
    const uint64_t off0 = 0;
    InfLayout L; /* the runtime's layout of a batch of this one stream */
    chk_layout(1, &n, &off0, nullptr, &limit, cb, [](uint32_t) { return true; }, L);
    const size_t ch = std::max<size_t>(1, L.pool);
    uint32_t nsec1 = 0, active = 0, q[4] = {0, 0, 0, 0};
    IsecStream st;
    memset(&st, 0x5a, sizeof st);
    std::vector<uint32_t> cstop(ch, 0x5a5a5a5au), clink(ch, 0x5a5a5a5au), clen(ch, 0x5a5a5a5au),
        chain_k(ch, 0x5a5a5a5au), chain_off(ch, 0x5a5a5a5au), cused(ch, 0x5a5a5a5au), creach(ch, 0x5a5a5a5au),
        want(ch, 0x5a5a5a5au);
    std::vector<uint64_t> cand(ch * INF_PC_CANDS, 0x5a5a5a5a5a5a5a5aull);
    IchkPlan P;
    memset(&P, 0, sizeof P); /* (no ring, no window, no slice check values) */
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
    m.cand = cand.data();
    m.cused = cused.data();
    m.creach = creach.data();
    m.want = want.data();
    chk_plan_view(P, m, L, window_bits, cb);

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
        chk_count_worker<false, true>(P, in.data(), lds, &si, &pc);
        chk_want(P, 0);
        chk_count_worker<true, true>(P, in.data(), lds, &si, &pc);
        chk_resolve<true>(P, in.data(), lds, &si, &pc, 0);
        size_finish(P, in.data(), &res, &resume, 0);
    }
    if (resume.state != 2u) {
        /* the whole-stream size decode, from the start (k_inflate_size and its relaunches) */
        InfJob job = {in.data(), n, nullptr, limit, window_bits};
        size_with_resync(job, lds, &res);
    }
    free(lds);
    *npieces = nsec1;
    *out_len = res.out_len;
    *consumed = res.consumed;
    return res.status;
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: %s CASES\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    for (;;) {
        uint32_t h[4];
        const size_t got = fread(h, 4, 4, f);
        if (got == 0)
            break;
        if (got != 4) {
            fprintf(stderr, "short record header\n");
            return 2;
        }
        std::vector<uint8_t> s((size_t)h[3] + 1);
        if (h[3] && fread(s.data(), 1, h[3], f) != h[3]) {
            fprintf(stderr, "short record\n");
            return 2;
        }
        uint32_t out_len = 0, consumed = 0, npieces = 0;
        const int rc = size_one(s.data(), h[3], (int32_t)h[0], h[1], h[2], &out_len, &consumed, &npieces);
        printf("%d %u %u %u\n", rc, out_len, consumed, npieces);
    }
    fclose(f);
    return 0;
}
