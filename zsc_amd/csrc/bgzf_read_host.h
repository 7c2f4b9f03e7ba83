/*
 * bgzf_read_host.h -- the host side of the BGZF index and the ranges plan (bgzf_read.h): offsets in a table,
 * the .gzi image of a table, and how a request is cut into member jobs.  Host only: no device code and no HIP
 * call, so the runtime (zsc_hip_runtime.hip) and the lane emulation (tests/emu_bgzf_read) run the same code.
 *
 * A table is members + 1 ascending entries (coffset, uoffset), the last the end entry.
 *
 * .gzi, as bgzip -r writes it and htslib's bgzf_index_load reads it: a little-endian u64 count, then count
 * pairs (u64 compressed offset, u64 uncompressed offset), one for every member start after the first -- the
 * first member at (0, 0) is implicit, and there is no end entry.  That a file written by bgzip loads here
 * rests on that published layout, not on a test against one.
 */
#ifndef ZSC_BGZF_READ_HOST_H
#define ZSC_BGZF_READ_HOST_H

#include <stdint.h>
#include <algorithm>
#include <vector>

#include "bgzf_read.h"

struct BgzTable {
    const uint64_t *coff, *uoff;
    uint32_t members;
    uint64_t total_out() const { return uoff[members]; }
};

/* the member that holds byte u < total_out (never an empty one) */
inline uint32_t bgz_member_of(const BgzTable &T, uint64_t u)
{
    return (uint32_t)(std::upper_bound(T.uoff, T.uoff + T.members + 1u, u) - T.uoff) - 1u;
}

/* uncompressed offset -> virtual offset: the member that holds the byte and the offset within; total_out is
 * the end entry with 0 within.  0: u is beyond total_out. */
inline int bgz_voffset(const BgzTable &T, uint64_t u, uint64_t *v)
{
    if (u > T.total_out())
        return 0;
    if (u == T.total_out()) {
        *v = T.coff[T.members] << 16;
        return 1;
    }
    const uint32_t k = bgz_member_of(T, u);
    *v = T.coff[k] << 16 | (u - T.uoff[k]);
    return 1;
}

/* virtual offset -> uncompressed offset.  0: the compressed part is no member start of the table (nor its end
 * entry with 0 within), or the part within lies beyond the member's length. */
inline int bgz_uoffset(const BgzTable &T, uint64_t v, uint64_t *u)
{
    const uint64_t c = v >> 16, w = v & 0xffffu;
    const uint64_t *e = std::lower_bound(T.coff, T.coff + T.members + 1u, c);
    if (e == T.coff + T.members + 1u || *e != c)
        return 0;
    const uint32_t k = (uint32_t)(e - T.coff);
    if (k == T.members ? w != 0u : w > T.uoff[k + 1u] - T.uoff[k])
        return 0;
    *u = T.uoff[k] + w;
    return 1;
}

inline uint64_t bgz_gzi_bytes(uint32_t members)
{
    return 8u + 16ull * (members ? members - 1u : 0u);
}

inline void bgz_put64(uint8_t *p, uint64_t v)
{
    for (int k = 0; k < 8; k++)
        p[k] = (uint8_t)(v >> (8 * k));
}

inline uint64_t bgz_get64(const uint8_t *p)
{
    uint64_t v = 0;
    for (int k = 0; k < 8; k++)
        v |= (uint64_t)p[k] << (8 * k);
    return v;
}

/* out: bgz_gzi_bytes(T.members) bytes */
inline void bgz_gzi_export(const BgzTable &T, uint8_t *out)
{
    const uint32_t n = T.members ? T.members - 1u : 0u;
    bgz_put64(out, n);
    for (uint32_t k = 0; k < n; k++) {
        bgz_put64(out + 8u + 16ull * k, T.coff[k + 1u]);
        bgz_put64(out + 16u + 16ull * k, T.uoff[k + 1u]);
    }
}

/* the member starts a .gzi image names, the implicit first one in front: 0 where the image is not one */
inline int bgz_gzi_parse(const uint8_t *gzi, uint64_t len, std::vector<uint64_t> &coff, std::vector<uint64_t> &uoff)
{
    if (len < 8u)
        return 0;
    const uint64_t n = bgz_get64(gzi);
    if (n > (len - 8u) / 16u || 8u + 16u * n != len)
        return 0;
    coff.assign(1, 0);
    uoff.assign(1, 0);
    for (uint64_t k = 0; k < n; k++) {
        coff.push_back(bgz_get64(gzi + 8u + 16u * k));
        uoff.push_back(bgz_get64(gzi + 16u + 16u * k));
    }
    return 1;
}

/* the entries an import has to have room for: the cnt named starts (bgz_gzi_parse) and, from the last of them
 * on, what a walk over the rest of a file of n bytes can find with its end entry -- the walk rewrites the last
 * named entry, hence cnt - 1.  A last start outside the file is refused without a walk: its entry alone. */
inline uint64_t bgz_import_room(const std::vector<uint64_t> &coff, uint32_t n)
{
    const uint64_t last = coff.back();
    return (coff.size() - 1u) + (last <= n ? BGI_TABLE_CAP(n - last) : 1u);
}

/* a request given as a begin and an END virtual offset, as a begin and a length in uncompressed offsets;
 * 0: an offset is not of the table (bgz_uoffset), or the end lies in front of the begin */
inline int bgr_from_voffsets(const BgzTable &T, uint64_t vbegin, uint64_t vend, uint64_t *begin, uint64_t *len)
{
    uint64_t e = 0;
    if (vend < vbegin || !bgz_uoffset(T, vbegin, begin) || !bgz_uoffset(T, vend, &e) || e < *begin)
        return 0;
    *len = e - *begin;
    return 1;
}

/* Request `req`: bytes [begin, begin + len) of file `file`'s content, clipped to total_out, to dst_off with
 * room for cap bytes.  res0 takes what the request reports when its jobs are good; the jobs -- one per member
 * that contributes a byte -- are appended, and *edges counts those that do not cover their member whole. */
inline void bgr_cut(const BgzTable &T, uint32_t file, uint32_t req, uint64_t begin, uint64_t len, uint32_t cap,
                    uint64_t dst_off, std::vector<BgrJob> &jobs, InfResult &res0, uint64_t *edges)
{
    const uint64_t total = T.total_out();
    const uint64_t b = std::min(begin, total), e = len > total - b ? total : b + len;
    res0.status = 0;
    res0.out_len = res0.consumed = res0.pad = 0;
    if (e == b)
        return;
    if (e - b > cap) {
        res0.status = -5; /* Z_BUF_ERROR */
        res0.out_len = (uint32_t)std::min<uint64_t>(e - b, 0xffffffffu);
        return;
    }
    const uint32_t k0 = bgz_member_of(T, b), k1 = bgz_member_of(T, e - 1u);
    for (uint32_t k = k0; k <= k1; k++) {
        const uint64_t u0 = T.uoff[k], u1 = T.uoff[k + 1u];
        if (u1 == u0)
            continue;
        BgrJob J;
        J.file = file;
        J.req = req;
        J.start = (uint32_t)T.coff[k];
        J.stop = (uint32_t)T.coff[k + 1u];
        J.len = (uint32_t)(u1 - u0);
        J.clip0 = (uint32_t)(std::max(b, u0) - u0);
        J.clip1 = (uint32_t)(std::min(e, u1) - u0);
        J.dst = dst_off + (u0 + J.clip0 - b);
        J.pad = 0;
        if (J.clip0 != 0u || J.clip1 != J.len)
            ++*edges;
        jobs.push_back(J);
    }
    res0.out_len = (uint32_t)(e - b);
    res0.consumed = (uint32_t)T.coff[k1 + 1u];
}

/* the queue's order: longest member first */
inline void bgr_order(std::vector<BgrJob> &jobs)
{
    std::stable_sort(jobs.begin(), jobs.end(), [](const BgrJob &a, const BgrJob &b) { return a.len > b.len; });
}

#endif
