/* layout_sanitize.cpp -- TEST INFRASTRUCTURE ONLY.  The batches of tests/test_deflate_layout_emu.py through
 * zsc_amd/csrc/deflate_plan_layout.h, for a build with sanitizers (one line per batch, returns 0):
 *   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all layout_sanitize.cpp -o layout_sanitize */
#include <stdio.h>
#include "../../zsc_amd/csrc/deflate_plan_layout.h"

static void one(const char *name, std::vector<uint32_t> lens, int level, int window_bits, uint64_t sub_limit, uint32_t cus,
                uint64_t off1 = 16)
{
    int wrap, wbits;
    const bool ok = dpl_fold_params(&level, window_bits, 8, 0, &wrap, &wbits);
    std::vector<uint64_t> off(lens.size(), 0);
    if (off.size() > 1)
        off[1] = off1;
    const std::vector<uint32_t> caps(lens.size(), 64);
    const DplKnobs K = {sub_limit, true, 3072u, false, 0, cus};
    DplLayout L;
    uint32_t bad = 0;
    const int rc = ok ? dpl_layout((uint32_t)lens.size(), lens.data(), off.data(), off.data(), caps.data(), level, wrap,
                                   wbits, 8, 0, nullptr, K, L, &bad) : DPL_STREAM_ERROR;
    uint64_t sum = 0; /* every entry of every array is read */
    for (const DplSub &sb : L.subs)
        for (const std::vector<uint32_t> *v : {&sb.tile_owner, &sb.blk_owner, &sb.order})
            for (uint32_t x : *v)
                sum += x;
    printf("%-12s rc %d bad %u subs %zu sum %llu\n", name, rc, bad, L.subs.size(), (unsigned long long)sum);
}

int main()
{
    const std::vector<uint32_t> edges = {10241, 0, 70000, 3072, 18433, 1, 6145, 40000, 3073, 18432, 6144, 10240};
    one("level 6", edges, 6, 15, ~0ull, 256);
    one("level 1", edges, 1, -15, ~0ull, 256);
    one("3 x 600 KiB", {600u << 10, 600u << 10, 600u << 10}, 6, 31, 1u << 20, 256);
    one("3 x 400 KiB", {400u << 10, 400u << 10, 400u << 10}, 6, 15, 1u << 20, 256);
    one("2 MiB alone", {1u << 10, 2u << 20, 1u << 10}, 6, 15, 1u << 20, 256);
    one("narrow", {100, 5000, 5000, 5000, 5000, 200}, 6, 15, ~0ull, 1);
    one("empty", {}, 6, 15, ~0ull, 256);
    one("too long", {100, 0x1ff00000u, 5}, 6, 15, ~0ull, 256);
    one("longest", {100, 0x1ff00000u - 1u}, 6, 15, ~0ull, 256);
    one("offset 8", {100, 100}, 6, 15, ~0ull, 256, 8);
    one("wbits 24", {100}, 6, 24, ~0ull, 256);
    return 0;
}
