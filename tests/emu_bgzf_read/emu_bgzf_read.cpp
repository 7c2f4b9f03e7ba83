/*
 * emu_bgzf_read.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone program that indexes BGZF files and reads
 * ranges out of them with zsc_amd/csrc/bgzf_read.h on the lane emulation (wave.h, -DZSC_WAVE_EMU), step by
 * step as the runtime enqueues them (zsc_hip_runtime.hip, zsc_hip_bgzf_index_build, _import_gzi, bgr_enqueue):
 * scan -> setup -> scan -> claims -> chain;  verify -> tail;  range jobs -> finish.  The host side -- how
 * requests become jobs, the offsets, the .gzi image -- is the runtime's own (bgzf_read_host.h).
 *
 * usage: emu_bgzf_read CASE OUTPUT
 * CASE, all little-endian u32 unless said otherwise:
 *   pool (0: the runtime's candidate pool; small: files are walked header by header instead), nfiles,
 *   per file: n and its n bytes
 *   ngzi, per image: file, len and its len bytes          (imported against the file as it is now)
 *   nflips, per flip: file, position, xor                  (applied after the index is built, before the run)
 *   flags, count, per request: file, u64 begin, u64 len, cap
 * Lines written, in this order:
 *   index F members indexed_bytes total_out      and members + 1 lines "C U", per file; then, per file,
 *   vo U ok V ok2 BACK                           bgz_voffset of U and bgz_uoffset of what it gave, at every
 *                                                member start, every member's last byte, the end and one beyond
 *   gzihex HEX                                   bgz_gzi_export of the table
 *   gzi RC members                               per image, and members + 1 lines "C U" where RC is 0
 *   plan RC jobs edges decoded_bytes             (RC -2: an offset was refused; nothing follows then)
 *   req status dest_len consumed canaries tail   per request (canaries: the 64 bytes in front of and behind the
 *                                                destination are untouched; tail: so are the bytes of the
 *                                                destination behind dest_len, for a status that writes)
 * and of every request with status 0 the dest_len bytes, appended to OUTPUT.
 */
#define ZSC_WAVE_EMU 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "../../zsc_amd/csrc/inflate_plan_layout.h"
#include "../../zsc_amd/csrc/bgzf_read_host.h"

static FILE *g_in;

static uint32_t rd32()
{
    uint32_t v;
    if (fread(&v, 4, 1, g_in) != 1) {
        fprintf(stderr, "short case file\n");
        exit(2);
    }
    return v;
}

static uint64_t rd64()
{
    const uint64_t lo = rd32();
    return lo | (uint64_t)rd32() << 32;
}

static std::vector<uint8_t> rdbytes(uint32_t n)
{
    std::vector<uint8_t> b(n);
    if (n && fread(b.data(), 1, n, g_in) != n) {
        fprintf(stderr, "short case file\n");
        exit(2);
    }
    return b;
}

struct Index {
    std::vector<std::vector<uint64_t>> coff, uoff; /* per file: members + 1 entries */
    BgzTable table(uint32_t f) const { return {coff[f].data(), uoff[f].data(), (uint32_t)coff[f].size() - 1u}; }
};

/* zsc_hip_bgzf_index_build over the files of `src` */
static Index build_index(const std::vector<uint8_t> &src, const std::vector<uint32_t> &lens,
                         const std::vector<uint64_t> &offs, uint32_t pool)
{
    const uint32_t nfiles = (uint32_t)lens.size();
    std::vector<uint32_t> caps(nfiles, 0);
    std::vector<uint64_t> zero(nfiles, 0);
    InfLayout L;
    mem_layout(nfiles, lens.data(), offs.data(), zero.data(), caps.data(), L);
    if (pool)
        L.pool = pool;
    const size_t nt = std::max<size_t>(1, L.tiles.size()), nc = L.pool, nf = std::max(1u, nfiles);
    std::vector<uint32_t> tile_cnt(nt, 0x5a5a5a5au), tile_off(nt, 0x5a5a5a5au), scount(nf, 0), nsec(nf, 0),
        active(nf, 0x5a5a5a5au);
    uint32_t q[4] = {0, 0, 0, 0};
    std::vector<IsecStream> st(nf);
    memset(st.data(), 0x5a, sizeof(IsecStream) * nf);
    std::vector<uint32_t> cstart(nc, 0x5a5a5a5au), cstop(nc, 0x5a5a5a5au), clink(nc, 0x5a5a5a5au),
        clen(nc, 0x5a5a5a5au);
    InfPlanMem m = {};
    m.items = L.items.data();
    m.tiles = L.tiles.data();
    m.tile_cnt = tile_cnt.data();
    m.tile_off = tile_off.data();
    m.scount = scount.data();
    m.nsec = nsec.data();
    m.st = st.data();
    m.active = active.data();
    m.q = q;
    m.cstart = cstart.data();
    m.cstop = cstop.data();
    m.clink = clink.data();
    m.clen = clen.data();
    MemPlan M;
    mem_plan_view(M, m, L, 31, nullptr, false, true);
    const IsecPlan &P = M.sp;
    for (uint32_t t = 0; t < P.ntiles; t++)
        mem_scan_tile(M, src.data(), t, 0);
    for (uint32_t a = 0; a < q[0]; a++)
        sec_setup(P, a);
    for (uint32_t t = 0; t < P.ntiles; t++)
        mem_scan_tile(M, src.data(), t, 1);
    for (uint32_t a = 0; a < q[0]; a++)
        mem_claims(M, src.data(), a);
    Index ix;
    ix.coff.resize(nfiles);
    ix.uoff.resize(nfiles);
    for (uint32_t f = 0; f < nfiles; f++) {
        /* (exactly the room the runtime gives the file, so that the sanitizers see a walk that leaves it) */
        const uint64_t tcap = BGI_TABLE_CAP(lens[f]);
        std::vector<uint64_t> c(tcap, ~0ull), u(tcap, ~0ull);
        uint32_t members = 0;
        bgi_chain(M, src.data(), f, c.data(), u.data(), tcap, &members);
        ix.coff[f].assign(c.begin(), c.begin() + members + 1);
        ix.uoff[f].assign(u.begin(), u.begin() + members + 1);
    }
    return ix;
}

/* zsc_hip_bgzf_index_import_gzi; returns the status, the table in c / u */
static int import_gzi(const uint8_t *file, uint32_t n, const std::vector<uint8_t> &gzi, std::vector<uint64_t> &c,
                      std::vector<uint64_t> &u)
{
    if (!bgz_gzi_parse(gzi.data(), gzi.size(), c, u) || c.size() + 1u > BGI_TABLE_CAP(n))
        return -3;
    const uint32_t cnt = (uint32_t)c.size();
    const uint64_t tcap = bgz_import_room(c, n);
    c.resize(tcap, ~0ull);
    u.resize(tcap, ~0ull);
    uint32_t out[2] = {0, 0};
    for (uint32_t e0 = 0; e0 < cnt; e0 += WAVE)
        bgi_verify(file, n, c.data(), u.data(), cnt, e0, out);
    if (c[cnt - 1u] <= n)
        bgi_walk(file, n, (uint32_t)c[cnt - 1u], u[cnt - 1u], c.data() + (cnt - 1u), u.data() + (cnt - 1u),
                 tcap - (cnt - 1u), out + 1);
    if (out[0])
        return -3;
    c.resize(cnt + (size_t)out[1]);
    u.resize(cnt + (size_t)out[1]);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: %s CASE OUTPUT\n", argv[0]);
        return 2;
    }
    g_in = fopen(argv[1], "rb");
    FILE *fo = fopen(argv[2], "wb");
    if (!g_in || !fo) {
        perror(g_in ? argv[2] : argv[1]);
        return 2;
    }
    const uint32_t pool = rd32(), nfiles = rd32();
    /* the files as a batch has them: at 16-byte aligned offsets, 64 bytes behind each */
    std::vector<uint32_t> lens(nfiles);
    std::vector<uint64_t> offs(nfiles);
    std::vector<uint8_t> src;
    for (uint32_t f = 0; f < nfiles; f++) {
        lens[f] = rd32();
        const std::vector<uint8_t> b = rdbytes(lens[f]);
        offs[f] = src.size();
        src.insert(src.end(), b.begin(), b.end());
        src.resize((src.size() + 64u + 15u) & ~(size_t)15u, 0);
    }
    src.resize(src.size() + 64u, 0);

    const Index ix = build_index(src, lens, offs, pool);
    for (uint32_t f = 0; f < nfiles; f++) {
        const BgzTable T = ix.table(f);
        printf("index %u %u %llu %llu\n", f, T.members, (unsigned long long)T.coff[T.members],
               (unsigned long long)T.total_out());
        for (uint32_t k = 0; k <= T.members; k++)
            printf("%llu %llu\n", (unsigned long long)T.coff[k], (unsigned long long)T.uoff[k]);
        /* the host helpers: the offsets at every member start, every member's last byte, the end and one beyond */
        std::vector<uint64_t> us(T.uoff, T.uoff + T.members + 1u);
        for (uint32_t k = 0; k < T.members; k++)
            if (T.uoff[k + 1u] > T.uoff[k])
                us.push_back(T.uoff[k + 1u] - 1u);
        us.push_back(T.total_out() + 1u);
        for (uint64_t u : us) {
            uint64_t v = 0, back = 0;
            const int ok = bgz_voffset(T, u, &v);
            const int ok2 = ok && bgz_uoffset(T, v, &back);
            printf("vo %llu %d %llu %d %llu\n", (unsigned long long)u, ok, (unsigned long long)v, ok2,
                   (unsigned long long)back);
        }
        std::vector<uint8_t> image(bgz_gzi_bytes(T.members));
        bgz_gzi_export(T, image.data());
        printf("gzihex ");
        for (uint8_t b : image)
            printf("%02x", b);
        printf("\n");
    }

    const uint32_t ngzi = rd32();
    for (uint32_t g = 0; g < ngzi; g++) {
        const uint32_t f = rd32(), len = rd32();
        const std::vector<uint8_t> gzi = rdbytes(len);
        std::vector<uint64_t> c, u;
        const int rc = import_gzi(src.data() + offs[f], lens[f], gzi, c, u);
        printf("gzi %d %u\n", rc, rc == 0 ? (uint32_t)c.size() - 1u : 0u);
        for (size_t k = 0; rc == 0 && k < c.size(); k++)
            printf("%llu %llu\n", (unsigned long long)c[k], (unsigned long long)u[k]);
    }

    const uint32_t nflips = rd32();
    for (uint32_t k = 0; k < nflips; k++) {
        const uint32_t f = rd32(), pos = rd32(), x = rd32();
        src[offs[f] + pos] ^= (uint8_t)x;
    }

    /* zsc_hip_inflate_plan_create_bgzf_ranges: destinations one behind the other, 64 bytes of canary around each */
    const uint32_t flags = rd32(), count = rd32();
    std::vector<uint32_t> rfile(count), rcap(count);
    std::vector<uint64_t> rbegin(count), rlen(count), doff(count);
    uint64_t db = 64;
    for (uint32_t i = 0; i < count; i++) {
        rfile[i] = rd32();
        rbegin[i] = rd64();
        rlen[i] = rd64();
        rcap[i] = rd32();
        doff[i] = db;
        db += (((uint64_t)rcap[i] + 15u) & ~15ull) + 64u;
    }
    std::vector<BgrJob> jobs;
    std::vector<InfResult> res0(std::max(1u, count)), res(std::max(1u, count));
    std::vector<BgrFile> files(std::max(1u, nfiles));
    for (uint32_t f = 0; f < nfiles; f++)
        files[f] = BgrFile{offs[f], lens[f], 0};
    uint64_t edges = 0, decoded = 0;
    int rc = 0;
    for (uint32_t i = 0; i < count && rc == 0; i++) {
        if (rfile[i] >= nfiles) {
            rc = -2;
            break;
        }
        const BgzTable T = ix.table(rfile[i]);
        uint64_t b = rbegin[i], n = rlen[i];
        if ((flags & 1u) && !bgr_from_voffsets(T, rbegin[i], rlen[i], &b, &n)) {
            rc = -2;
            break;
        }
        bgr_cut(T, rfile[i], i, b, n, rcap[i], doff[i], jobs, res0[i], &edges);
    }
    bgr_order(jobs);
    for (const BgrJob &J : jobs)
        decoded += J.len;
    printf("plan %d %zu %llu %llu\n", rc, rc ? (size_t)0 : jobs.size(), (unsigned long long)(rc ? 0 : edges),
           (unsigned long long)(rc ? 0 : decoded));
    if (rc == 0) {
        std::vector<uint8_t> dst(db, 0xEE);
        std::vector<uint32_t> bad(std::max(1u, count), 0);
        uint32_t q[4] = {0, 0, 0, 0};
        BgrPlan B;
        B.files = files.data();
        B.jobs = jobs.data();
        B.bad = bad.data();
        B.q = q;
        B.njobs = (uint32_t)jobs.size();
        B.count = count;
        /* one lane group, so one staging slot that every edge job reuses (exactly BGR_SLOT bytes, 16-byte aligned) */
        uint8_t *slot = (uint8_t *)aligned_alloc(16, BGR_SLOT);
        memset(slot, 0xA5, BGR_SLOT);
        InfLds *lds = (InfLds *)malloc(sizeof(InfLds));
        memset(lds, 0x3C, sizeof(InfLds));
        static uint32_t crc_table[1][256];
        lds->cktab = crc_table;
        InfResult r;
        InfResume rs;
        memset(&r, 0, sizeof r);
        memset(&rs, 0, sizeof rs);
        bgr_worker(B, src.data(), dst.data(), slot, lds, &r, &rs);
        for (uint32_t i = 0; i < count; i++)
            bgr_finish(B, res0.data(), res.data(), i);
        free(lds);
        free(slot);
        for (uint32_t i = 0; i < count; i++) {
            const InfResult &v = res[i];
            const uint64_t room = ((uint64_t)rcap[i] + 15u) & ~15ull;
            uint32_t canaries = 1, tail = 1;
            for (uint64_t k = 0; k < 64; k++)
                if (dst[doff[i] - 64 + k] != 0xEE || dst[doff[i] + room + k] != 0xEE)
                    canaries = 0;
            for (uint64_t k = rcap[i]; k < room; k++)
                if (dst[doff[i] + k] != 0xEE)
                    canaries = 0;
            /* (a request that failed in its data may have written anywhere inside its own destination) */
            const uint64_t kept = v.status == 0 ? v.out_len : v.status == -5 ? 0 : rcap[i];
            for (uint64_t k = kept; k < rcap[i]; k++)
                if (dst[doff[i] + k] != 0xEE)
                    tail = 0;
            printf("req %d %u %u %u %u\n", v.status, v.out_len, v.consumed, canaries, tail);
            if (v.status == 0 && v.out_len)
                fwrite(dst.data() + doff[i], 1, v.out_len, fo);
        }
    }
    fclose(g_in);
    fclose(fo);
    return 0;
}
