/*
 * emu_pack.cpp -- TEST INFRASTRUCTURE ONLY.
 *
 * The packing kernels (zsc_amd/csrc/pack.h) in the lane emulation: the launches zsc_hip_*_plan_pack and
 * zsc_hip_unpack enqueue, wave by wave, on item lengths, statuses and slot offsets the caller supplies.  No
 * deflate is involved: the kernels move bytes whatever they are.
 *
 * Built with -DEMU_PACK_MAIN it is a program of its own (make asan: with AddressSanitizer and UBSan) that
 * packs and unpacks a seeded mix of items in allocations of exactly the bytes the kernels may touch.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../zsc_amd/csrc/pack.h"

extern "C" uint32_t emu_pack_wave(void) { return WAVE; }
extern "C" uint32_t emu_pack_scan_b(void) { return PK_SCAN_B; }
extern "C" uint64_t emu_pack_tile(void) { return PK_TILE; }

/* records as the plans keep them: { length, status } per item */
static PkLens make_lens(std::vector<uint32_t> &rec, const uint32_t *lens, const int32_t *status, uint64_t count)
{
    rec.resize(2 * (size_t)count + 2);
    for (uint64_t i = 0; i < count; i++) {
        rec[2 * i] = lens[i];
        rec[2 * i + 1] = status ? (uint32_t)status[i] : 0xEEEEEEEEu;
    }
    PkLens L;
    L.rec = rec.data();
    L.stride_w = 2;
    L.len_w = 0;
    L.st_w = status ? 1u : PK_NO_STATUS;
    return L;
}

/* The offsets of a pack: reduce per level, the scan of the top level's sums, apply per level, each a launch
 * of its own.  offsets: count + 1 values.  Returns the number of launches. */
static int scan_launches(const PkLens &L, uint64_t count, uint32_t align, uint64_t *offsets)
{
    uint64_t n[PK_MAX_LEVELS];
    const uint32_t levels = pk_scan_levels(count, n);
    std::vector<std::vector<uint64_t>> sums(levels);
    for (uint32_t k = 1; k < levels; k++)
        sums[k].assign((size_t)n[k] + 1, 0xEEEEEEEEEEEEEEEEull);
    int launches = 0;
    for (uint32_t k = 0; k + 1 < levels; k++, launches++)
        for (uint64_t g = 0; g < n[k + 1]; g++)
            pk_scan_block(L, align, k == 0 ? nullptr : sums[k].data(), n[k], g, nullptr, nullptr,
                          sums[k + 1].data());
    for (uint32_t k = levels; k-- > 0; launches++) {
        const uint64_t waves = k + 1 == levels ? 1 : n[k + 1];
        for (uint64_t g = 0; g < waves; g++)
            pk_scan_block(L, align, k == 0 ? nullptr : sums[k].data(), n[k], g,
                          k + 1 == levels ? nullptr : sums[k + 1].data(), k == 0 ? offsets : sums[k].data(), nullptr);
    }
    return launches;
}

extern "C" int emu_pack_scan(const uint32_t *lens, const int32_t *status, uint64_t count, uint32_t align,
                             uint64_t *offsets)
{
    std::vector<uint32_t> rec;
    const PkLens L = make_lens(rec, lens, status, count);
    return scan_launches(L, count, align, offsets);
}

/* The move launch: `tiles` waves.  dense / sparse: 16-byte aligned bases. */
extern "C" void emu_pack_move(int unpack, uint64_t count, const uint64_t *off, const uint32_t *lens,
                              const int32_t *status, const uint64_t *sparse_off, uint8_t *dense, uint8_t *sparse,
                              uint64_t cap, uint64_t tiles)
{
    std::vector<uint32_t> rec;
    PkMove M;
    M.off = off;
    M.sparse_off = sparse_off;
    M.lens = make_lens(rec, lens, status, count);
    M.count = (uint32_t)count;
    M.unpack = unpack ? 1u : 0u;
    M.cap = cap;
    for (uint64_t t = 0; t < tiles; t++)
        pk_move_tile(M, dense, sparse, t);
}

#ifdef EMU_PACK_MAIN
static uint32_t g_seed = 12345u;
static uint32_t rnd(void)
{
    g_seed = g_seed * 1664525u + 1013904223u;
    return g_seed >> 8;
}

static void *alloc16(size_t n) /* ends exactly n bytes behind a 16-byte aligned start */
{
    void *p = nullptr;
    if (posix_memalign(&p, 16, n ? n : 1) != 0)
        abort();
    return p;
}

int main(void)
{
    static const uint32_t kLens[] = {0, 1, 2, 8, 15, 16, 17, 20, 31, 33, (uint32_t)PK_TILE - 1, (uint32_t)PK_TILE,
                                     (uint32_t)PK_TILE + 1, 3 * (uint32_t)PK_TILE + 5};
    static const uint32_t kAligns[] = {1, 16, 256};
    int bad = 0;
    for (uint32_t round = 0; round < 3; round++) {
        const uint32_t align = kAligns[round];
        const uint64_t count = 300;
        std::vector<uint32_t> lens(count);
        std::vector<int32_t> status(count);
        std::vector<uint64_t> soff(count), off(count + 1);
        uint64_t sparse_end = 0, at = 0;
        for (uint64_t i = 0; i < count; i++) {
            lens[i] = rnd() % 4 ? kLens[rnd() % 10] : kLens[rnd() % 14];
            status[i] = rnd() % 16 ? 0 : -5;
            soff[i] = at;
            at += ((uint64_t)lens[i] + 15u) / 16u * 16u + 16u * (rnd() % 3);
            if (status[i] == 0 && lens[i])
                sparse_end = soff[i] + ((uint64_t)lens[i] + 15u) / 16u * 16u;
        }
        /* the sparse image ends at the last item's end rounded up to 16, the dense one at total */
        uint8_t *sparse = (uint8_t *)alloc16(sparse_end);
        for (uint64_t x = 0; x < sparse_end; x++)
            sparse[x] = (uint8_t)(rnd() | 1u);
        emu_pack_scan(lens.data(), status.data(), count, align, off.data());
        const uint64_t total = off[count];
        uint8_t *dense = (uint8_t *)alloc16(total);
        memset(dense, 0xA5, total);
        emu_pack_move(0, count, off.data(), lens.data(), status.data(), soff.data(), dense, sparse, total,
                      (total + PK_TILE - 1) / PK_TILE + 1);
        for (uint64_t i = 0; i < count; i++) {
            const uint64_t n = status[i] ? 0 : lens[i];
            if (memcmp(dense + off[i], sparse + soff[i], n) != 0)
                bad++;
            for (uint64_t x = off[i] + n; x < off[i + 1]; x++)
                bad += dense[x] != 0;
        }
        /* and back, into a fresh sparse image of the same extent */
        uint8_t *back = (uint8_t *)alloc16(sparse_end);
        memset(back, 0x5A, sparse_end);
        emu_pack_move(1, count, off.data(), lens.data(), status.data(), soff.data(), dense, back, ~0ull,
                      (total + PK_TILE - 1) / PK_TILE + 1);
        for (uint64_t i = 0; i < count; i++)
            if (memcmp(back + soff[i], sparse + soff[i], status[i] ? 0 : lens[i]) != 0)
                bad++;
        printf("align %u: %llu items, %llu bytes packed, %d mismatches\n", align, (unsigned long long)count,
               (unsigned long long)total, bad);
        free(sparse);
        free(dense);
        free(back);
    }
    return bad ? 1 : 0;
}
#endif
