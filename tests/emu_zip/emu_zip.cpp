/*
 * emu_zip.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone program that writes ZIP images with the kernels of
 * zsc_amd/csrc/zip.h on the lane emulation (wave.h, -DZSC_WAVE_EMU), launch by launch as the runtime enqueues
 * them (zsc_hip_runtime.hip, zsc_hip_deflate_plan_zip): archive lengths -> scan (reduce, scan of the sums,
 * apply) -> part offsets -> move.  No deflate is involved: the result records and the slots' bytes are the
 * caller's, so every length is reachable.
 *
 * usage: emu_zip CASES OUTPUT [exact]
 * CASES holds records of uint32 count, narchives, align, short_by, flags, has_datetime, then narchives + 1
 * uint32 arch_first, count + 1 uint64 name offsets, the names' bytes, count uint32 dos_datetime where
 * has_datetime, then per buffer int32 status, uint32 out_len, uint32 n and the n bytes of its slot.  The
 * image's capacity is its length - short_by.  Every slot is an allocation of its own of n rounded up to 16
 * bytes, the names are one of exactly their size.
 * Without `exact` the image is allocated with 4096 bytes behind the capacity and the move runs twice, on an
 * image of 0xA5 and on one of 0x5A; with it (the sanitizer runs) the image is an allocation of exactly the
 * capacity and the move runs once.  Per record and move, appended to OUTPUT: uint64 total, uint64 launches of
 * the scan, narchives + 1 uint64 archive offsets, narchives uint64 archive states (ZP_ST_*), 2 * count +
 * narchives + 1 uint64 part offsets, uint64 n and the n bytes of the image's allocation.  One line per record:
 * total launches.
 */
#define ZSC_WAVE_EMU 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "../../zsc_amd/csrc/zip.h"

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
    uint32_t h[6];
    while (fread(h, 4, 6, fi) == 6) {
        const uint32_t count = h[0], narchives = h[1], align = h[2], short_by = h[3], flags = h[4], has_dt = h[5];
        std::vector<uint32_t> first((size_t)narchives + 1);
        std::vector<uint64_t> name_off((size_t)count + 1);
        if (fread(first.data(), 4, first.size(), fi) != first.size() ||
            fread(name_off.data(), 8, name_off.size(), fi) != name_off.size())
            return 2;
        const uint64_t names_len = name_off[count];
        uint8_t *names = (uint8_t *)alloc16((size_t)names_len);
        if (names_len && fread(names, 1, (size_t)names_len, fi) != names_len)
            return 2;
        std::vector<uint32_t> datetime(std::max<uint32_t>(count, 1));
        if (has_dt && count && fread(datetime.data(), 4, count, fi) != count)
            return 2;
        std::vector<uint32_t> rec(4 * (size_t)count + 4, 0xEEEEEEEEu), caps(std::max<uint32_t>(count, 1));
        std::vector<uint8_t *> slots(count);
        uint8_t *lowest = nullptr;
        for (uint32_t i = 0; i < count; i++) {
            uint32_t b[3];
            if (fread(b, 4, 3, fi) != 3)
                return 2;
            rec[4 * (size_t)i] = b[1];
            rec[4 * (size_t)i + 1] = b[0];
            caps[i] = b[1];
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
        /* what _zip_enable uploads */
        ZpLayout Z;
        if (!zp_layout(count, narchives, first.data(), name_off.data(), caps.data(), align, Z))
            return 3;
        const uint32_t nparts = (uint32_t)Z.nparts;
        ZpArchives A;
        A.rec = rec.data();
        A.arch_first = first.data();
        A.name_off = name_off.data();
        A.fixed = Z.fixed.data();
        A.narchives = narchives;
        A.count = count;
        A.align = align;
        std::vector<uint64_t> arch_off((size_t)narchives + 1, 0xEEEEEEEEEEEEEEEEull),
            parts((size_t)nparts + 1, 0xEEEEEEEEEEEEEEEEull);
        std::vector<uint32_t> arch_st(std::max<uint32_t>(narchives, 1), 0xEEEEEEEEu);
        for (uint32_t a = 0; a < narchives; a++)
            zp_arch_len(A, a, arch_off.data(), arch_st.data());
        const uint64_t launches = scan_launches(arch_off.data(), narchives);
        for (uint32_t a = 0; a <= narchives; a++)
            zp_part_off(A, a, arch_off.data(), parts.data());
        const uint64_t total = parts[nparts];
        const uint64_t cap = total > short_by ? total - short_by : 0;
        const size_t room = exact ? (size_t)cap : (size_t)cap + 4096;
        ZpMove M;
        M.parts = parts.data();
        M.kinds = Z.kinds.data();
        M.slot = slot_off.data();
        M.name_off = name_off.data();
        M.arch_first = first.data();
        M.arch_of = Z.arch_of.data();
        M.datetime = has_dt ? datetime.data() : nullptr;
        M.nparts = nparts;
        M.flags = flags;
        M.cap = cap;
        M.names_len = names_len;
        uint8_t *image = (uint8_t *)alloc16(room);
        for (int pass = 0; pass < (exact ? 1 : 2); pass++) {
            memset(image, pass ? 0x5A : 0xA5, room);
            /* the grid comes from the capacity: a tile more than the image has */
            const uint64_t tiles = (cap + PK_TILE - 1) / PK_TILE + 1;
            for (uint64_t t = 0; t < tiles; t++)
                zp_move_tile(M, image, lowest, names, t);
            put64(fo, total);
            put64(fo, launches);
            fwrite(arch_off.data(), 8, arch_off.size(), fo);
            for (uint32_t a = 0; a < narchives; a++)
                put64(fo, arch_st[a]);
            fwrite(parts.data(), 8, parts.size(), fo);
            put64(fo, room);
            fwrite(image, 1, room, fo);
        }
        printf("%llu %llu\n", (unsigned long long)total, (unsigned long long)launches);
        free(image);
        free(names);
        for (uint8_t *s : slots)
            free(s);
    }
    fclose(fi);
    fclose(fo);
    return 0;
}
