/*
 * emu_sort.cpp -- TEST INFRASTRUCTURE ONLY.
 *
 * The tile sort (zsc_amd/csrc/hash_sort.h, kernel 1) alone in the lane emulation: the kernel source
 * compiled with -DZSC_WAVE_EMU, every tile of a buffer run as k_hash_sort runs it (its phases in order,
 * the waves of the workgroup one after the other inside a phase), and what it leaves in sorted[], rank[]
 * and dir[] handed back for a comparison with a plain stable sort.
 */
#define ZSC_WAVE_EMU 1
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

struct uint4 { uint32_t x, y, z, w; };

#include "../../zsc_amd/csrc/hash_sort.h"

extern "C" int emu_sort_batch(void) { return HS_SCATTER_BATCH; }
extern "C" int emu_sort_wave(void) { return WAVE; }
extern "C" int emu_sort_waves(void) { return HS_WAVES; }

/* sorted_out: tiles * ZD_TILE entries, rank_out: n entries, dir_out: tiles * ZD_DIR_STRIDE entries, all
 * filled with a pattern first so that what the sort does not write shows; returns the number of tiles */
extern "C" int emu_sort_tiles(const uint8_t *src, uint32_t n, uint32_t *sorted_out, uint16_t *rank_out,
                              uint16_t *dir_out)
{
    std::vector<uint8_t> in((size_t)n + 64, 0);
    memcpy(in.data(), src, n);
    const uint32_t ntiles = n == 0 ? 1 : (n + ZD_TILE - 1) / ZD_TILE;
    std::vector<uint32_t> tmp((size_t)ntiles * ZD_TILE, 0xdeadbeef);
    std::vector<uint16_t> rank((size_t)n + 64, 0xdead);
    for (size_t i = 0; i < (size_t)ntiles * ZD_TILE; i++)
        sorted_out[i] = 0xdeadbeef;
    for (size_t i = 0; i < (size_t)ntiles * ZD_DIR_STRIDE; i++)
        dir_out[i] = 0xdead;
    const uint32_t owners = n >= 3 ? n - 2 : 0; /* positions 0 .. n-3 own a 3-byte string */
    for (uint32_t t = 0; t < ntiles; t++) {
        HsTile tile;
        memset(&tile, 0, sizeof tile);
        tile.in = in.data();
        tile.n = n;
        tile.start = t * ZD_TILE;
        tile.m = owners > tile.start ? (owners - tile.start < ZD_TILE ? owners - tile.start : ZD_TILE) : 0;
        tile.sorted = sorted_out + (size_t)t * ZD_TILE;
        tile.tmp = tmp.data() + (size_t)t * ZD_TILE;
        tile.rank = rank.data();
        tile.dir = dir_out + (size_t)t * ZD_DIR_STRIDE;
        HsLds *lds = (HsLds *)malloc(sizeof(HsLds));
        memset(lds, 0x6B, sizeof(HsLds));
        for (int ph = 0; ph < HS_PHASES; ph++)
            for (int w = 0; w < HS_WAVES; w++)
                hash_sort_phase(tile, lds, w, ph);
        free(lds);
    }
    memcpy(rank_out, rank.data(), (size_t)n * 2);
    return (int)ntiles;
}
