/*
 * emu_bgzf.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone program that writes BGZF images with the kernels of
 * zsc_amd/csrc/bgzf.h on the lane emulation (wave.h, -DZSC_WAVE_EMU), launch by launch as the runtime enqueues
 * them (zsc_hip_runtime.hip, zsc_hip_deflate_plan_bgzf): file lengths -> scan (reduce, scan of the sums,
 * apply) -> member offsets -> move.  No deflate is involved: the result records and the slots' bytes are the
 * caller's, so every length is reachable.
 *
 * usage: emu_bgzf CASES OUTPUT [exact]
 * CASES holds records of uint32 count, nfiles, align, short_by, then nfiles + 1 uint32 file_first, then per
 * buffer int32 status, uint32 out_len, uint32 n and the n bytes of its slot.  The image's capacity is its length
 * - short_by.  Every slot is an allocation of its own of n rounded up to 16 bytes.
 * Without `exact` the image is allocated with 4096 bytes behind the capacity and the move runs twice, on an
 * image of 0xA5 and on one of 0x5A; with it (the sanitizer runs) the image is an allocation of exactly the
 * capacity and the move runs once.  Per record and move, appended to OUTPUT: uint64 total, uint64 launches of
 * the scan, nfiles + 1 uint64 file offsets, count + nfiles + 1 uint64 part offsets, uint64 n and the n bytes
 * of the image's allocation.  One line per record: total launches.
 */
#define ZSC_WAVE_EMU 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "../../zsc_amd/csrc/bgzf.h"

static void *alloc16(size_t n) /* ends exactly n bytes behind a 16-byte aligned start */
{
    void *p = nullptr;
    if (posix_memalign(&p, 16, n ? n : 1) != 0)
        abort();
    return p;
}

/* the scan of n values in place, as scan_enqueue launches it; returns the launches */
static uint64_t scan_launches(uint64_t *vals0, uint64_t count)
{
    const PkLens none = {nullptr, 0u, 0u, PK_NO_STATUS};
    uint64_t n[PK_MAX_LEVELS];
    const uint32_t levels = pk_scan_levels(count, n);
    std::vector<std::vector<uint64_t>> sums(levels);
    for (uint32_t k = 1; k < levels; k++)
        sums[k].assign((size_t)n[k] + 1, 0xEEEEEEEEEEEEEEEEull);
    auto vals = [&](uint32_t k) { return k == 0 ? vals0 : sums[k].data(); };
    uint64_t launches = 0;
    for (uint32_t k = 0; k + 1 < levels; k++, launches++)
        for (uint64_t g = 0; g < n[k + 1]; g++)
            pk_scan_block(none, 1u, vals(k), n[k], g, nullptr, nullptr, vals(k + 1));
    for (uint32_t k = levels; k-- > 0; launches++) {
        const uint64_t waves = k + 1 == levels ? 1 : n[k + 1];
        for (uint64_t g = 0; g < waves; g++)
            pk_scan_block(none, 1u, vals(k), n[k], g, k + 1 == levels ? nullptr : vals(k + 1), vals(k), nullptr);
    }
    return launches;
}

static void put64(FILE *f, uint64_t v) { fwrite(&v, 8, 1, f); }

int main(int argc, char **argv)
{
    if (argc < 3)
        return 2;
    const bool exact = argc > 3 && strcmp(argv[3], "exact") == 0;
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo)
        return 2;
    uint32_t h[4];
    while (fread(h, 4, 4, fi) == 4) {
        const uint32_t count = h[0], nfiles = h[1], align = h[2], short_by = h[3];
        std::vector<uint32_t> first((size_t)nfiles + 1);
        if (fread(first.data(), 4, first.size(), fi) != first.size())
            return 2;
        std::vector<uint32_t> rec(4 * (size_t)count + 4, 0xEEEEEEEEu);
        std::vector<uint8_t *> slots(count);
        uint8_t *lowest = nullptr;
        for (uint32_t i = 0; i < count; i++) {
            uint32_t b[3];
            if (fread(b, 4, 3, fi) != 3)
                return 2;
            rec[4 * (size_t)i] = b[1];
            rec[4 * (size_t)i + 1] = b[0];
            const size_t room = ((size_t)b[2] + 15u) & ~(size_t)15u;
            slots[i] = (uint8_t *)alloc16(room);
            memset(slots[i], 0xC3, room);
            if (b[2] && fread(slots[i], 1, b[2], fi) != b[2])
                return 2;
            lowest = !lowest || slots[i] < lowest ? slots[i] : lowest;
        }
        /* the plan's output is one base and offsets: the lowest slot is the base */
        std::vector<uint64_t> slot_off(std::max<uint32_t>(count, 1));
        for (uint32_t i = 0; i < count; i++)
            slot_off[i] = (uint64_t)(slots[i] - lowest);
        /* what _bgzf_enable uploads: what each part is */
        const uint32_t nparts = count + nfiles;
        std::vector<uint32_t> what(std::max<uint32_t>(nparts, 1));
        for (uint32_t f = 0; f < nfiles; f++) {
            for (uint32_t i = first[f]; i < first[f + 1]; i++)
                what[(size_t)i + f] = i;
            what[(size_t)first[f + 1] + f] = BZ_PART_TAIL;
        }
        BzFiles F;
        F.rec = rec.data();
        F.file_first = first.data();
        F.nfiles = nfiles;
        F.count = count;
        F.align = align;
        std::vector<uint64_t> file_off((size_t)nfiles + 1, 0xEEEEEEEEEEEEEEEEull), parts((size_t)nparts + 1,
                                                                                          0xEEEEEEEEEEEEEEEEull);
        for (uint32_t f = 0; f < nfiles; f++)
            bz_file_len(F, f, file_off.data());
        const uint64_t launches = scan_launches(file_off.data(), nfiles);
        for (uint32_t f = 0; f <= nfiles; f++)
            bz_member_off(F, f, file_off.data(), parts.data());
        const uint64_t total = parts[nparts];
        const uint64_t cap = total > short_by ? total - short_by : 0;
        const size_t room = exact ? (size_t)cap : (size_t)cap + 4096;
        BzMove M;
        M.parts = parts.data();
        M.what = what.data();
        M.slot = slot_off.data();
        M.nparts = nparts;
        M.cap = cap;
        uint8_t *image = (uint8_t *)alloc16(room);
        for (int pass = 0; pass < (exact ? 1 : 2); pass++) {
            memset(image, pass ? 0x5A : 0xA5, room);
            /* the grid comes from the capacity: a tile more than the image has */
            const uint64_t tiles = (cap + PK_TILE - 1) / PK_TILE + 1;
            for (uint64_t t = 0; t < tiles; t++)
                bz_move_tile(M, image, lowest, t);
            put64(fo, total);
            put64(fo, launches);
            fwrite(file_off.data(), 8, file_off.size(), fo);
            fwrite(parts.data(), 8, parts.size(), fo);
            put64(fo, room);
            fwrite(image, 1, room, fo);
        }
        printf("%llu %llu\n", (unsigned long long)total, (unsigned long long)launches);
        free(image);
        for (uint8_t *s : slots)
            free(s);
    }
    fclose(fi);
    fclose(fo);
    return 0;
}
