/*
 * emu_check.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone program that checks streams with the check
 * path (zsc_amd/csrc/inflate_check.h) on the lane emulation (wave.h, -DZSC_WAVE_EMU), kernel by kernel
 * as the runtime enqueues them (zsc_hip_runtime.hip, check_enqueue): setup -> scan -> count -> want ->
 * retry -> resolve -> window -> check-write -> finish for a stream longer than a chunk, then the
 * whole-stream ring decode for a stream that did not finish, with relaunches through the size decode.
 *
 * Every whole-stream decode of a run uses the same ring, as a lane group's streams do, and a shadow of
 * the ring (InfCheck::shadow) holds the output position last written to each slot: the decoder aborts
 * when a slot read does not hold the position asked for (so nothing of an earlier stream, and nothing
 * the ring has wrapped over, is ever read) or when a position is overwritten before it was folded.
 *
 * usage: emu_check CASES
 * CASES holds records of int32 window_bits, uint32 limit, uint32 chunk_bytes (0xFFFFFFFF: never cut),
 * uint32 n and the n bytes of the stream.  One line per record: status size consumed pieces errors value
 * (value: the check value computed, 0 unless the status is 0).
 */
#define ZSC_WAVE_EMU 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "../../zsc_amd/csrc/inflate_check.h"

static InfLds *new_lds()
{
    InfLds *lds = (InfLds *)malloc(sizeof(InfLds));
    memset(lds, 0x3C, sizeof(InfLds));
    static uint32_t crc_table[1][256];
    lds->cktab = crc_table;
    return lds;
}

/* the lane group's ring and its shadow: one for the whole run */
static std::vector<uint8_t> g_ring(CHK_RING, 0x77);
static std::vector<uint64_t> g_shadow(CHK_RING, 0);

static int check_one(const uint8_t *src, uint32_t n, int window_bits, uint32_t limit, uint32_t cb, uint32_t *out_len,
                     uint32_t *consumed, uint32_t *npieces, uint32_t *errors, uint32_t *value)
{
    std::vector<uint8_t> in((size_t)n + 64, 0);
    if (n)
        memcpy(in.data(), src, n);
    IsecItem it = {};
    it.src_len = n;
    it.dst_cap = std::min<uint32_t>(limit, 0x7fffffffu);
    it.tile0 = 0;
    const bool act = n > cb;
    it.ntiles = act ? (uint32_t)(((uint64_t)n + cb - 1u) / cb) : 0u;
    std::vector<IsecTile> scan;
    for (uint32_t k = 1; k < it.ntiles; k++)
        scan.push_back(IsecTile{0u, k});
    const size_t ch = std::max(1u, it.ntiles);
    uint32_t nsec1 = 0, active = 0, q[4] = {0, 0, 0, 0};
    IsecStream st;
    memset(&st, 0x5a, sizeof st);
    std::vector<uint32_t> cstop(ch, 0x5a5a5a5au), clink(ch, 0x5a5a5a5au), clen(ch, 0x5a5a5a5au),
        chain_k(ch, 0x5a5a5a5au), chain_off(ch, 0x5a5a5a5au), chain_ck(ch, 0x5a5a5a5au), cused(ch, 0x5a5a5a5au),
        creach(ch, 0x5a5a5a5au), want(ch, 0x5a5a5a5au);
    std::vector<uint64_t> cand(ch * INF_PC_CANDS, 0x5a5a5a5a5a5a5a5aull);
    std::vector<uint16_t> ring(act ? ch * INF_WIN : 0, 0x5a5a);
    std::vector<uint8_t> win(act ? ch * INF_WIN : 0, 0x5a);
    IchkPlan P;
    memset(&P, 0, sizeof P);
    P.sp.items = &it;
    P.sp.tiles = scan.data();
    P.sp.nsec = &nsec1;
    P.sp.st = &st;
    P.sp.active = &active;
    P.sp.q = q;
    P.sp.cstop = cstop.data();
    P.sp.clink = clink.data();
    P.sp.clen = clen.data();
    P.sp.chain_k = chain_k.data();
    P.sp.chain_off = chain_off.data();
    P.sp.chain_ck = chain_ck.data();
    P.sp.count = 1;
    P.sp.ntiles = (uint32_t)scan.size();
    P.sp.pool = (uint32_t)ch;
    P.sp.window_bits = window_bits;
    P.sp.work_mul = SEC_WORK_MUL;
    P.sp.work_add = SEC_WORK_ADD;
    P.cand = cand.data();
    P.cused = cused.data();
    P.creach = creach.data();
    P.want = want.data();
    P.ring = ring.data();
    P.win = win.data();
    P.nactive = act ? 1u : 0u;
    P.chunk_bytes = cb;

    InfLds *lds = new_lds();
    InfSecInfo si;
    InfPiece pc;
    InfResult res;
    memset(&res, 0, sizeof res);
    InfResume resume;
    memset(&resume, 0, sizeof resume);
    uint32_t val = 0;
    if (P.nactive) {
        std::vector<uint64_t> piece_shadow(CHK_RING, 0);
        chk_setup(P, 0);
        for (uint32_t t = 0; t < P.sp.ntiles; t++)
            chk_scan(P, in.data(), t);
        chk_count_worker<false>(P, in.data(), lds, &si, &pc);
        chk_want(P, 0);
        chk_count_worker<true>(P, in.data(), lds, &si, &pc);
        chk_resolve(P, in.data(), lds, &si, &pc, 0);
        chk_windows(P, 0, 0, 1, [] {});
        chk_check_worker(P, in.data(), lds, &si, &pc, piece_shadow.data());
        sec_finish(P.sp, in.data(), &res, &resume, 0);
        check_finish(P, &resume, &val, 0);
    }
    if (resume.state != 2u) {
        /* the whole-stream ring decode, from the start (k_inflate_check, then k_inflate_size's relaunches) */
        InfJob job = {in.data(), n, nullptr, limit, window_bits};
        InfCheck ck;
        ck.ring = g_ring.data();
        ck.shadow = g_shadow.data();
        check_with_resync(job, lds, &res, &resume, &ck, &val);
    }
    free(lds);
    *npieces = nsec1;
    *out_len = res.out_len;
    *consumed = res.consumed;
    *errors = resume.errors;
    *value = res.status == 0 ? val : 0u;
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
        uint32_t out_len = 0, consumed = 0, npieces = 0, errors = 0, value = 0;
        const int rc = check_one(s.data(), h[3], (int32_t)h[0], h[1], h[2], &out_len, &consumed, &npieces, &errors,
                                 &value);
        printf("%d %u %u %u %u %u\n", rc, out_len, consumed, npieces, errors, value);
    }
    fclose(f);
    return 0;
}
