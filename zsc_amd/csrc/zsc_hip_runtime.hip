/*
 * zsc_hip_runtime.hip -- kernels and host runtime of libzsc_hip.so (gfx950 only).
 *
 * The __global__ functions are thin: each one finds its unit of work (tile,
 * buffer or block) and calls the wavefront code in the headers of this
 * directory.  The host half owns HBM scratch, builds the work descriptors and
 * enqueues the six kernels of a deflate pass on one HIP stream.
 *
 * Path and boundary: this file implements the batched extension declared in
 * include/zsc_hip.h; zsc_api.c puts the reference's own zsc_pub.h signatures on
 * top of it.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <map>
#include <vector>

#include "bit_emit.h"
#include "checksum.h"
#include "hash_sort.h"
#include "huff_plan.h"
#include "inflate.h"
#include "inflate_sections.h"
#include "inflate_chunks.h"
#include "inflate_resync.h"
#include "inflate_index.h"
#include "inflate_size.h"
#include "inflate_check.h"
#include "inflate_members.h"
#include "bgzf_read.h"
#include "deflate_index.h"
#include "deflate_verify.h"
#include "pack.h"
#include "bgzf.h"
#include "zip.h"
#include "lz_parse.h"
#include "lz_parse_seg.h"
#include "lz_parse_pipe.h"
#include "match_table.h"
#include "lz_parse_simple.h"
#include "sections.h"
#include "zsc_dev.h"
#include "deflate_plan_layout.h"

#include "zsc/zsc_conf_private.h"
#include "zsc_hip.h"

/* ------------------------------------------------------------------------ */
/* kernels                                                                  */
/* ------------------------------------------------------------------------ */

/* kernel 0: one wavefront per buffer */
__global__ __launch_bounds__(64) void k_checksum(const uint8_t *__restrict__ in,
                                                 const ZdBuf *__restrict__ bufs,
                                                 ZdResult *__restrict__ res, uint32_t nbuf)
{
    __shared__ CkLds lds;
    const uint32_t b = blockIdx.x;
    if (b >= nbuf)
        return;
    const ZdBuf buf = bufs[b];
    uint32_t v = 0;
    if (buf.wrap == 1)
        v = ck_adler32(in + buf.in_off, buf.in_len);
    else if (buf.wrap == 2)
        v = ck_crc32(in + buf.in_off, buf.in_len, &lds);
    if (threadIdx.x == 0)
        res[b].adler = v;
}

/* level 0: one piece of a stored stream -- a stored block (3-bit header in its own byte,
 * LEN, NLEN, the bytes), a flush marker, or the wrapper header / trailer; the host has laid
 * the pieces out (StoreSim), this only moves bytes */
typedef struct {
    uint64_t src_off; /* first input byte of a stored block (batch input) */
    uint64_t dst_off; /* first output byte of the piece (batch output) */
    uint32_t len;     /* stored bytes */
    uint32_t kind;    /* 0 stored block, 1 flush marker, 2 wrapper header, 3 trailer, 4 room for a caller's
                         gzip header; sections.h: 5 the marker's four bytes after a run, 6 plain bytes,
                         7 one byte AND arg, then len - 1 zero bytes (the end of a run) */
    uint32_t arg;     /* block: BFINAL; header: CMF<<8|FLG or the gzip XFL; trailer / header: owning buffer */
    uint32_t buf;     /* owning buffer (for the check value) */
} ZdStorePiece;

__global__ __launch_bounds__(256) void k_store(const uint8_t *__restrict__ in,
                                               uint8_t *__restrict__ out,
                                               const ZdStorePiece *__restrict__ pieces,
                                               const ZdBuf *__restrict__ bufs,
                                               const ZdResult *__restrict__ res, uint32_t npieces)
{
    if (blockIdx.x >= npieces)
        return;
    const ZdStorePiece pc = pieces[blockIdx.x];
    uint8_t *o = out + pc.dst_off;
    if (pc.kind == 0u) {
        /* reference _tr_stored_block, src/trees.c:838-849 */
        if (threadIdx.x == 0) {
            o[0] = (uint8_t)pc.arg;
            o[1] = (uint8_t)pc.len;
            o[2] = (uint8_t)(pc.len >> 8);
            o[3] = (uint8_t)~pc.len;
            o[4] = (uint8_t)(~pc.len >> 8);
        }
        const uint8_t *s = in + pc.src_off;
        for (uint32_t i = threadIdx.x; i < pc.len; i += blockDim.x)
            o[5u + i] = s[i];
    } else if (pc.kind == 6u) {
        const uint8_t *s = in + pc.src_off;
        for (uint32_t i = threadIdx.x; i < pc.len; i += blockDim.x)
            o[i] = s[i];
    } else if (threadIdx.x == 0) {
        if (pc.kind == 7u) {
            o[0] = in[pc.src_off] & (uint8_t)pc.arg;
            if (pc.len > 1u)
                o[1] = 0;
            return;
        }
        /* the small pieces; sections.h: only the first pc.len bytes when dest ends inside one */
        uint8_t t[10];
        uint32_t nt = 0;
        if (pc.kind == 5u) { /* LEN = 0, NLEN = ~0 of Z_FULL_FLUSH's empty stored block */
            t[0] = 0, t[1] = 0, t[2] = 0xff, t[3] = 0xff;
            nt = 4;
        } else if (pc.kind == 1u) { /* Z_FULL_FLUSH's empty stored block, src/deflate.c:1240-1243 */
            t[0] = 0, t[1] = 0, t[2] = 0, t[3] = 0xff, t[4] = 0xff;
            nt = 5;
        } else if (pc.kind == 2u) {
            if (bufs[pc.buf].wrap == 1u) { /* src/deflate.c:1031-1049 */
                t[0] = (uint8_t)(pc.arg >> 8), t[1] = (uint8_t)pc.arg;
                nt = 2;
            } else { /* :1068-1082 */
                t[0] = 31, t[1] = 139, t[2] = 8;
                t[3] = t[4] = t[5] = t[6] = t[7] = 0;
                t[8] = (uint8_t)pc.arg, t[9] = 3;
                nt = 10;
            }
        } else if (pc.kind == 3u) {
            const uint32_t c = res[pc.buf].adler, n = bufs[pc.buf].in_len;
            if (bufs[pc.buf].wrap == 1u) { /* :1282-1286 */
                t[0] = (uint8_t)(c >> 24), t[1] = (uint8_t)(c >> 16), t[2] = (uint8_t)(c >> 8), t[3] = (uint8_t)c;
                nt = 4;
            } else { /* :1272-1281 */
                for (uint32_t k = 0; k < 4; k++) {
                    t[k] = (uint8_t)(c >> (8 * k));
                    t[4 + k] = (uint8_t)(n >> (8 * k));
                }
                nt = 8;
            }
        }
        if (pc.len != 0u && pc.len < nt)
            nt = pc.len;
        for (uint32_t k = 0; k < nt; k++)
            o[k] = t[k];
    }
}

/* kernel 1: one workgroup (HS_WAVES wavefronts) per 32 KiB tile */
__global__ __launch_bounds__(HS_WAVES * 64) void k_hash_sort(
    const uint8_t *__restrict__ in, const ZdBuf *__restrict__ bufs,
    const uint32_t *__restrict__ tile_owner, uint32_t *__restrict__ sorted,
    uint32_t *__restrict__ tmp, uint16_t *__restrict__ rank, uint16_t *__restrict__ dir,
    uint32_t ntiles)
{
    __shared__ HsLds lds;
    const uint32_t tile = blockIdx.x;
    if (tile >= ntiles)
        return;
    const ZdBuf buf = bufs[tile_owner[tile]];
    const uint32_t t = tile - buf.tile0;
    HsTile job;
    job.in = in + buf.in_off;
    job.n = buf.in_len;
    job.start = t * ZD_TILE;
    const uint32_t owners = buf.in_len >= 3 ? buf.in_len - 2 : 0;
    job.m = owners > job.start ? min(owners - job.start, ZD_TILE) : 0u;
    job.sorted = sorted + (uint64_t)tile * ZD_TILE;
    job.tmp = tmp + (uint64_t)tile * ZD_TILE;
    job.rank = rank + buf.rank_off;
    job.dir = dir + (uint64_t)tile * ZD_DIR_STRIDE;
    job.dir_prev = nullptr;
    job.hib = nullptr;
    job.cnt = nullptr;
    const int w = (int)(threadIdx.x >> 6);
    for (int phase = 0; phase < HS_PHASES; phase++) {
        hash_sort_phase(job, &lds, w, phase);
        __syncthreads();
    }
}

/* kernel 1b: one workgroup per tile: chain lengths, and the link into the previous tile */
__global__ __launch_bounds__(HS_WAVES * 64) void k_link_prev(
    const uint8_t *__restrict__ in, const ZdBuf *__restrict__ bufs,
    const uint32_t *__restrict__ tile_owner, const uint16_t *__restrict__ dir,
    const uint16_t *__restrict__ rank, uint16_t *__restrict__ hib, uint32_t *__restrict__ cnt,
    uint32_t ntiles)
{
    const uint32_t tile = blockIdx.x;
    if (tile >= ntiles)
        return;
    const ZdBuf buf = bufs[tile_owner[tile]];
    const uint32_t t = tile - buf.tile0;
    HsTile job;
    job.in = in + buf.in_off;
    job.n = buf.in_len;
    job.start = t * ZD_TILE;
    const uint32_t owners = buf.in_len >= 3 ? buf.in_len - 2 : 0;
    job.m = owners > job.start ? min(owners - job.start, ZD_TILE) : 0u;
    job.sorted = nullptr;
    job.tmp = nullptr;
    job.rank = const_cast<uint16_t *>(rank) + buf.rank_off;
    job.dir = const_cast<uint16_t *>(dir) + (uint64_t)tile * ZD_DIR_STRIDE;
    job.dir_prev = t ? dir + (uint64_t)(tile - 1) * ZD_DIR_STRIDE : nullptr;
    job.hib = hib + buf.rank_off;
    job.cnt = cnt + buf.rank_off;
    hs_link_prev(job, (int)(threadIdx.x >> 6));
}

/* kernel 1c: one workgroup per tile: longest_match for every position of the tile, for the two
 * values of prev_length the lazy parse can ask with (match_table.h) */
#ifdef MT_EU
#define MT_ATTR __attribute__((amdgpu_waves_per_eu(MT_EU, MT_EU)))
#else
#define MT_ATTR
#endif
__global__ __launch_bounds__(MT_WAVES * 64) MT_ATTR void k_match_table(
    const uint8_t *__restrict__ in, const ZdBuf *__restrict__ bufs,
    const uint32_t *__restrict__ tile_owner, const uint32_t *__restrict__ sorted,
    const uint16_t *__restrict__ rank, const uint16_t *__restrict__ hib,
    const uint32_t *__restrict__ cnt, uint32_t *__restrict__ r2,
    const ZdLevel cfg, uint32_t min_len, uint32_t cap, uint32_t ntiles)
{
    __shared__ MtLds lds;
    const uint32_t tile = blockIdx.x;
    if (tile >= ntiles)
        return;
    const ZdBuf buf = bufs[tile_owner[tile]];
    /* only what the segmented parser takes without joints reads the table */
    if (buf.in_len <= min_len || buf.sched_n != 0)
        return;
    MtJob job;
    job.in = in + buf.in_off;
    job.n = buf.in_len;
    job.start = (tile - buf.tile0) * ZD_TILE;
    job.sorted = sorted + (uint64_t)buf.tile0 * ZD_TILE;
    job.rank = rank + buf.rank_off;
    job.hib = hib + buf.rank_off;
    job.cnt = cnt + buf.rank_off;
    job.r2 = r2 + buf.rank_off;
    job.cfg = cfg;
    job.cfg.wsize = ZD_TILE;
    job.cfg.max_dist = ZD_MAX_DIST;
    job.cfg.sym_cap = ZD_SYM_CAP;
    job.cfg.hbits = 15u;
    job.strategy = buf.strategy;
    job.cap = cap;
    const int w = (int)(threadIdx.x >> 6);
    mt_phase_load(job, &lds, w);
    __syncthreads();
    const uint32_t base0 = sg_base(job.cfg, job.start, job.n);
    mt_phase_search(job, &lds, w, base0);
}

/* kernel 2: one wavefront per buffer, longest buffers first.  L picks the LDS ring
 * size (and with it the number of waves a CU can hold); `first`/`nbuf` select the
 * slice of the length-sorted order this launch covers. */
template <class L>
__global__ __launch_bounds__(64) void k_parse(const uint8_t *__restrict__ in,
                                              const ZdBuf *__restrict__ bufs,
                                              const uint32_t *__restrict__ order,
                                              const uint32_t *__restrict__ sorted,
                                              const uint16_t *__restrict__ rank,
                                              const uint16_t *__restrict__ hib,
                                              uint32_t *__restrict__ syms,
                                              ZdBlockRec *__restrict__ recs,
                                              ZdParseOut *__restrict__ pout,
                                              const ZdSched *__restrict__ sched,
                                              const ZdLevel cfg, uint32_t first, uint32_t nbuf)
{
    __shared__ L lds;
    if (blockIdx.x >= nbuf)
        return;
    const uint32_t b = order[first + blockIdx.x];
    const ZdBuf buf = bufs[b];
    LzJob job;
    job.in = in + buf.in_off;
    job.n = buf.in_len;
    job.ntot = buf.in_len;
    job.sorted = sorted + (uint64_t)buf.tile0 * ZD_TILE;
    job.rank = rank + buf.rank_off;
    job.hib = hib + buf.rank_off;
    job.cnt = nullptr;
    job.dir = nullptr;
    job.r2 = nullptr;
    job.stair_min = 0xffffffffu;
    job.syms = syms + buf.sym_off;
    job.blocks = recs + buf.blk0;
    job.out = pout + b;
    job.cfg = cfg;
    job.strategy = buf.strategy;
    job.more = buf.more;
    job.sched = sched + buf.sched_off;
    job.nsched = buf.sched_n;
    job.n0 = buf.n0;
    lz_parse_lazy<L>(job, &lds);
}

/* kernel 2 for long buffers at levels 4-9: SG_W wavefronts share one window and parse
 * SG_W segments of the same buffer at once (lz_parse_seg.h) */
template <bool GENERIC, bool TABLE, int LEVEL> /* GENERIC false: window_bits 15 / mem_level 8, their constants folded in;
                                                  TABLE: the plan has a match table (only with GENERIC false);
                                                  LEVEL 6: the default level's search parameters folded in too (0: any) */
__global__ __launch_bounds__(SG_W * 64, SG_MIN_WAVES) void k_parse_seg(const uint8_t *__restrict__ in,
                                                         const ZdBuf *__restrict__ bufs,
                                                         const uint32_t *__restrict__ order,
                                                         const uint32_t *__restrict__ sorted,
                                                         const uint16_t *__restrict__ rank,
                                                         const uint16_t *__restrict__ hib,
                                                         const uint32_t *__restrict__ cnt,
                                                         const uint16_t *__restrict__ dir,
                                                         const uint32_t *__restrict__ r2,
                                                         uint32_t *__restrict__ syms,
                                                         ZdBlockRec *__restrict__ recs,
                                                         ZdParseOut *__restrict__ pout,
                                                         uint32_t *__restrict__ seg_tok,
                                                         const ZdSched *__restrict__ sched,
                                                         const ZdLevel cfg, uint32_t stair_min,
                                                         uint32_t pipe, uint32_t first, uint32_t nbuf)
{
    __shared__ SgLds lds;
    if (blockIdx.x >= nbuf)
        return;
    const uint32_t b = order[first + blockIdx.x];
    const ZdBuf buf = bufs[b];
    LzJob job;
    job.in = in + buf.in_off;
    job.n = buf.in_len;
    job.ntot = buf.in_len;
    job.sorted = sorted + (uint64_t)buf.tile0 * ZD_TILE;
    job.rank = rank + buf.rank_off;
    job.hib = hib + buf.rank_off;
    job.cnt = cnt + buf.rank_off;
    /* given the directories, the parser works hib / cnt out itself and k_link_prev has not run (sg_link) */
    job.dir = dir ? dir + (uint64_t)buf.tile0 * ZD_DIR_STRIDE : nullptr;
    /* the match table covers plain buffers (match_table.h); a run with joints is searched as before */
    job.r2 = r2 && buf.sched_n == 0 ? r2 + buf.rank_off : nullptr;
    job.stair_min = stair_min;
    job.syms = syms + buf.sym_off;
    job.blocks = recs + buf.blk0;
    job.out = pout + b;
    job.cfg = cfg;
    if (!GENERIC) {
        job.cfg.wsize = ZD_TILE;
        job.cfg.max_dist = ZD_MAX_DIST;
        job.cfg.sym_cap = ZD_SYM_CAP;
        job.cfg.hbits = 15u;
    }
    if (LEVEL == 6) { /* reference src/deflate.c:155: the fewer wave-uniform values the parser keeps, the fewer it spills */
        job.cfg.good = 8;
        job.cfg.lazy = 16;
        job.cfg.nice = 128;
        job.cfg.chain = 128;
        job.cfg.slow = 1;
    }
    job.strategy = LEVEL == 6 ? 0u : buf.strategy; /* (LEVEL 6 is only launched for plans without Z_FILTERED, the one strategy the lazy parse looks at) */
    job.more = buf.more;
    job.sched = sched + buf.sched_off;
    job.nsched = buf.sched_n;
    job.n0 = buf.n0;
    SgScratch scr;
    /* one area per workgroup: the segments' tokens, then their token indices (one pointer to keep) */
    scr.tok = seg_tok + (uint64_t)blockIdx.x * SG_SCRATCH_WORDS;
    scr.sidx = (uint16_t *)(scr.tok + SG_NS * SG_TOKCAP);
    const int w = (int)(threadIdx.x >> 6);
    if (pipe && buf.sched_n == 0) {
        /* a plain buffer: the segments as a pipeline, no barrier between the first and the last of them
         * (lz_parse_pipe.h); a run with joints keeps the super-steps below */
        sg_pipe_init(&lds, w);
        __syncthreads();
        if (TABLE && job.r2 != nullptr)
            sg_pipe_run<true>(job, &lds, scr);
        else
            sg_pipe_run<false>(job, &lds, scr);
        __syncthreads();
        if (lds.p_stuck && threadIdx.x == 0) {
            job.out->nsyms = 0;
            job.out->nblocks = 0xffffffffu; /* reported as Z_STREAM_ERROR by the layout kernel */
        }
        return;
    }
    sg_init(&lds, w);
    __syncthreads();
    /* every loop is bounded so that a logic error can never hang the device: a phase needs
     * n/SG_SPAN + 1 super-steps, a run has at most one phase per joint and one more */
    const uint32_t max_steps = buf.in_len / SG_SPAN + 2;
    bool stuck = false;
    uint32_t si = 0, nph = buf.sched_n ? buf.n0 : buf.in_len;
    for (uint32_t phase = 0; phase <= buf.sched_n && !stuck; phase++) {
        nph = sg_phase_end(job, nph, &si); /* joints of kind 0 only move the end (lz_parse_seg.h) */
        const bool goes_on = si < buf.sched_n;
        job.n = nph;
        job.more = goes_on ? 1u : buf.more;
        uint32_t steps = 0;
        while (!lds.finished) {
            if (++steps > max_steps) {
                stuck = true;
                break;
            }
            sg_phase_begin(job, &lds, w);
            __syncthreads();
            /* a redo round follows whenever a parser gave up before it met a successor's
             * tokens; each one moves the resolver at least one segment on */
            uint32_t rounds = 0;
            do {
                if (++rounds > SG_NS + 1) {
                    stuck = true;
                    break;
                }
                if (TABLE && job.r2 != nullptr)
                    sg_phase_parse<true>(job, &lds, scr, w);
                else
                    sg_phase_parse<false>(job, &lds, scr, w);
                __syncthreads();
                sg_phase_resolve(job, &lds, scr, w);
                __syncthreads();
            } while (lds.redo);
            if (stuck)
                break;
        }
        if (!goes_on)
            break;
        /* every wave must have seen lds.finished before wave 0 clears it for the next phase */
        __syncthreads();
        nph = sched[buf.sched_off + si].new_n;
        si++;
        sg_next_phase(&lds, w, job.n);
        __syncthreads();
    }
    if (stuck && threadIdx.x == 0) {
        job.out->nsyms = 0;
        job.out->nblocks = 0xffffffffu; /* reported as Z_STREAM_ERROR by the layout kernel */
    }
}

/* k_parse_seg for plain buffers in the pipeline schedule, in the pipeline's own LDS geometry (SgLdsNarrow,
 * lz_parse_seg.h): 40 712 bytes of LDS and registers for eight waves per SIMD put four workgroups on a CU.
 * Built without the match table and for window_bits 15 / mem_level 8 only; launched for plans without joints
 * (every buffer is a plain one), so there is no super-step path in it. */
template <int LEVEL>
__global__ __launch_bounds__(SG_W * 64, SG_NARROW_MIN_WAVES) void k_parse_seg_narrow(const uint8_t *__restrict__ in,
                                                         const ZdBuf *__restrict__ bufs,
                                                         const uint32_t *__restrict__ order,
                                                         const uint32_t *__restrict__ sorted,
                                                         const uint16_t *__restrict__ rank,
                                                         const uint16_t *__restrict__ hib,
                                                         const uint32_t *__restrict__ cnt,
                                                         const uint16_t *__restrict__ dir,
                                                         uint32_t *__restrict__ syms,
                                                         ZdBlockRec *__restrict__ recs,
                                                         ZdParseOut *__restrict__ pout,
                                                         uint32_t *__restrict__ seg_tok,
                                                         const ZdLevel cfg, uint32_t stair_min,
                                                         uint32_t first, uint32_t nbuf)
{
    __shared__ SgLdsNarrow lds;
    if (blockIdx.x >= nbuf)
        return;
    const uint32_t b = order[first + blockIdx.x];
    const ZdBuf buf = bufs[b];
    LzJob job;
    job.in = in + buf.in_off;
    job.n = buf.in_len;
    job.ntot = buf.in_len;
    job.sorted = sorted + (uint64_t)buf.tile0 * ZD_TILE;
    job.rank = rank + buf.rank_off;
    job.hib = hib + buf.rank_off;
    job.cnt = cnt + buf.rank_off;
    job.dir = dir ? dir + (uint64_t)buf.tile0 * ZD_DIR_STRIDE : nullptr;
    job.r2 = nullptr;
    job.stair_min = stair_min;
    job.syms = syms + buf.sym_off;
    job.blocks = recs + buf.blk0;
    job.out = pout + b;
    job.cfg = cfg;
    job.cfg.wsize = ZD_TILE;
    job.cfg.max_dist = ZD_MAX_DIST;
    job.cfg.sym_cap = ZD_SYM_CAP;
    job.cfg.hbits = 15u;
    if (LEVEL == 6) { /* (as k_parse_seg) */
        job.cfg.good = 8;
        job.cfg.lazy = 16;
        job.cfg.nice = 128;
        job.cfg.chain = 128;
        job.cfg.slow = 1;
    }
    job.strategy = LEVEL == 6 ? 0u : buf.strategy;
    job.more = buf.more;
    job.sched = nullptr;
    job.nsched = 0;
    job.n0 = buf.n0;
    SgScratch scr;
    /* (the scratch keeps the layout of SG_NS slots; this geometry uses the first SgLdsNarrow::NSLOT of each part) */
    scr.tok = seg_tok + (uint64_t)blockIdx.x * SG_SCRATCH_WORDS;
    scr.sidx = (uint16_t *)(scr.tok + SG_NS * SG_TOKCAP);
    sg_pipe_init(&lds, (int)(threadIdx.x >> 6));
    __syncthreads();
    sg_pipe_run<false>(job, &lds, scr);
    __syncthreads();
    if (lds.p_stuck && threadIdx.x == 0) {
        job.out->nsyms = 0;
        job.out->nblocks = 0xffffffffu; /* reported as Z_STREAM_ERROR by the layout kernel */
    }
}

/* kernel 2 for Z_HUFFMAN_ONLY and Z_RLE: no chains, no window (lz_parse_simple.h) */
__global__ __launch_bounds__(64) void k_parse_simple(const uint8_t *__restrict__ in,
                                                     const ZdBuf *__restrict__ bufs,
                                                     uint32_t *__restrict__ syms,
                                                     ZdBlockRec *__restrict__ recs,
                                                     ZdParseOut *__restrict__ pout,
                                                     const ZdSched *__restrict__ sched,
                                                     const ZdLevel cfg, uint32_t nbuf)
{
    __shared__ SpLds lds;
    const uint32_t b = blockIdx.x;
    if (b >= nbuf)
        return;
    const ZdBuf buf = bufs[b];
    LzJob job;
    job.in = in + buf.in_off;
    job.n = buf.in_len;
    job.ntot = buf.in_len;
    job.sorted = nullptr;
    job.rank = nullptr;
    job.hib = nullptr;
    job.cnt = nullptr;
    job.dir = nullptr;
    job.r2 = nullptr;
    job.stair_min = 0xffffffffu;
    job.syms = syms + buf.sym_off;
    job.blocks = recs + buf.blk0;
    job.out = pout + b;
    job.cfg = cfg;
    job.strategy = buf.strategy;
    job.more = buf.more;
    job.sched = sched + buf.sched_off;
    job.nsched = buf.sched_n;
    job.n0 = buf.n0;
    if (buf.sched_n)
        lz_parse_simple_joints(job, &lds);
    else if (buf.strategy == (uint32_t)Z_HUFFMAN_ONLY)
        lz_parse_huff(job, &lds);
    else
        lz_parse_rle(job, &lds);
}

/* kernel 2 for levels 1-3 (greedy parse) */
template <class L> /* LzLdsFastG: the window read from the input; LzLdsFast: an LDS ring (four waves per CU) */
__global__ __launch_bounds__(64) void k_parse_fast(const uint8_t *__restrict__ in,
                                                   const ZdBuf *__restrict__ bufs,
                                                   const uint32_t *__restrict__ order,
                                                   const uint32_t *__restrict__ sorted,
                                                   const uint16_t *__restrict__ rank,
                                                   const uint16_t *__restrict__ hib,
                                                   uint32_t *__restrict__ syms,
                                                   ZdBlockRec *__restrict__ recs,
                                                   ZdParseOut *__restrict__ pout,
                                                   const ZdSched *__restrict__ sched,
                                                   const ZdLevel cfg, uint32_t nbuf)
{
    __shared__ L lds;
    if (blockIdx.x >= nbuf)
        return;
    const uint32_t b = order[blockIdx.x];
    const ZdBuf buf = bufs[b];
    LzJob job;
    job.in = in + buf.in_off;
    job.n = buf.in_len;
    job.ntot = buf.in_len;
    job.sorted = sorted + (uint64_t)buf.tile0 * ZD_TILE;
    job.rank = rank + buf.rank_off;
    job.hib = hib + buf.rank_off;
    job.cnt = nullptr;
    job.dir = nullptr;
    job.r2 = nullptr;
    job.stair_min = 0xffffffffu;
    job.syms = syms + buf.sym_off;
    job.blocks = recs + buf.blk0;
    job.out = pout + b;
    job.cfg = cfg;
    job.strategy = buf.strategy;
    job.more = buf.more;
    job.sched = sched + buf.sched_off;
    job.nsched = buf.sched_n;
    job.n0 = buf.n0;
    lz_parse_greedy<L>(job, &lds);
}

/* kernel 3: one wavefront per (possible) block */
__global__ __launch_bounds__(64) void k_huff_plan(const ZdBuf *__restrict__ bufs,
                                                  const uint32_t *__restrict__ blk_owner,
                                                  const uint32_t *__restrict__ syms,
                                                  const ZdBlockRec *__restrict__ recs,
                                                  const ZdParseOut *__restrict__ pout,
                                                  ZdBlockPlan *__restrict__ plans, uint32_t nslots)
{
    __shared__ HpLds lds;
    const uint32_t slot = blockIdx.x;
    if (slot >= nslots)
        return;
    const uint32_t b = blk_owner[slot];
    const ZdBuf buf = bufs[b];
    if (slot - buf.blk0 >= pout[b].nblocks || pout[b].nblocks > buf.max_blocks)
        return;
    const ZdBlockRec *rec = &recs[slot];
    huff_plan_block(syms + buf.sym_off + rec->sym_begin, rec, buf.strategy, &plans[slot], &lds);
}

/* kernel 4a: one thread per buffer */
__global__ __launch_bounds__(64) void k_layout(const ZdBuf *__restrict__ bufs,
                                               const ZdParseOut *__restrict__ pout,
                                               const ZdBlockRec *__restrict__ recs,
                                               ZdBlockPlan *__restrict__ plans,
                                               ZdResult *__restrict__ res,
                                               uint8_t *__restrict__ out, uint32_t nbuf)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nbuf)
        return;
    layout_buffer(&bufs[b], &pout[b], recs + bufs[b].blk0, plans + bufs[b].blk0, &res[b],
                  out + bufs[b].out_off);
}

/* sections.h wants to know where every block ends: the bit_off column of the plans, packed */
__global__ __launch_bounds__(256) void k_bit_offs(const ZdBlockPlan *__restrict__ plans,
                                                  uint32_t *__restrict__ out, uint32_t nslots)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nslots)
        out[i] = plans[i].bit_off;
}

/* kernel 4b: one wavefront per block */
__global__ __launch_bounds__(64) void k_emit(const uint8_t *__restrict__ in,
                                             const ZdBuf *__restrict__ bufs,
                                             const uint32_t *__restrict__ blk_owner,
                                             const uint32_t *__restrict__ syms,
                                             const ZdBlockRec *__restrict__ recs,
                                             const ZdParseOut *__restrict__ pout,
                                             const ZdBlockPlan *__restrict__ plans,
                                             uint8_t *__restrict__ out, uint32_t nslots)
{
    __shared__ BeLds lds;
    const uint32_t slot = blockIdx.x;
    if (slot >= nslots)
        return;
    const uint32_t b = blk_owner[slot];
    const ZdBuf buf = bufs[b];
    if (slot - buf.blk0 >= pout[b].nblocks || pout[b].nblocks > buf.max_blocks)
        return;
    const ZdBlockRec *rec = &recs[slot];
    emit_block(in + buf.in_off, syms + buf.sym_off + rec->sym_begin, rec, &plans[slot],
               (uint32_t *)(out + buf.out_off), &lds);
}

/* kernels 4c-4e (deflate_index.h): the seek-point index of every stream of a sub-batch, only for a plan
 * with the index enabled.  4c: one wavefront per block */
__global__ __launch_bounds__(64) void k_index_reach(const ZdBuf *__restrict__ bufs,
                                                    const uint32_t *__restrict__ blk_owner,
                                                    const uint32_t *__restrict__ syms,
                                                    const ZdBlockRec *__restrict__ recs,
                                                    const ZdParseOut *__restrict__ pout,
                                                    const ZdBlockPlan *__restrict__ plans,
                                                    uint32_t *__restrict__ reach, uint32_t nslots)
{
    const uint32_t slot = blockIdx.x;
    if (slot >= nslots)
        return;
    const uint32_t b = blk_owner[slot];
    const ZdBuf buf = bufs[b];
    if (slot - buf.blk0 >= pout[b].nblocks || pout[b].nblocks > buf.max_blocks)
        return;
    const ZdBlockRec *rec = &recs[slot];
    const uint32_t r = dix_block_reach(syms + buf.sym_off + rec->sym_begin, rec, &plans[slot]);
    if (threadIdx.x == 0)
        reach[slot] = r;
}

/* 4d: one thread per buffer, like k_layout; rec_off / npts: the sub-batch's first buffer */
__global__ __launch_bounds__(64) void k_index_points(const ZdBuf *__restrict__ bufs,
                                                     const ZdParseOut *__restrict__ pout,
                                                     const ZdBlockRec *__restrict__ recs,
                                                     const ZdBlockPlan *__restrict__ plans,
                                                     const uint32_t *__restrict__ reach,
                                                     const ZdResult *__restrict__ res, uint32_t chunk_bytes,
                                                     ZidxRec *__restrict__ out,
                                                     const uint64_t *__restrict__ rec_off,
                                                     uint32_t *__restrict__ npts, uint32_t nbuf)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nbuf)
        return;
    dix_points(&bufs[b], &pout[b], recs + bufs[b].blk0, plans + bufs[b].blk0, reach + bufs[b].blk0, &res[b],
               chunk_bytes, out + rec_off[b], (uint32_t)(rec_off[b + 1] - rec_off[b]), &npts[b]);
}

/* 4e: blockIdx.x = the buffer; the gridDim.y wavefronts of a buffer share its pieces */
__global__ __launch_bounds__(64) void k_index_check(const uint8_t *__restrict__ in,
                                                    const ZdBuf *__restrict__ bufs, ZidxRec *__restrict__ out,
                                                    const uint64_t *__restrict__ rec_off,
                                                    const uint32_t *__restrict__ npts, uint32_t nbuf)
{
    __shared__ CkLds lds;
    const uint32_t b = blockIdx.x;
    if (b >= nbuf)
        return;
    const uint32_t n = npts[b], wrap = bufs[b].wrap;
    const uint8_t *src = in + bufs[b].in_off;
    ZidxRec *recs = out + rec_off[b];
    for (uint32_t p = blockIdx.y; p < n; p += gridDim.y) {
        const uint32_t v = dix_piece_check(src, &recs[p], wrap, &lds);
        if (threadIdx.x == 0)
            recs[p].ck = v;
        __syncthreads(); /* (one wave: orders the table's next rewrite after this piece's reads) */
    }
}

/* the export's windows: piece i of one buffer copied from its input to its place in the gathered buffer */
#define DIX_GATHER_THREADS 256
__global__ __launch_bounds__(DIX_GATHER_THREADS) void k_index_gather(const uint8_t *__restrict__ in, uint32_t n,
                                                                     const ZidxRec *__restrict__ recs,
                                                                     uint8_t *__restrict__ out)
{
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x)
        dix_gather(in, &recs[i], out, threadIdx.x, DIX_GATHER_THREADS);
}

/* kernels 4f-4h (deflate_verify.h): read-back verification, only for a plan with verification enabled.
 * 4f, per sub-batch: one thread per block slot keeps the block's facts; first / nblk: the sub-batch's
 * first buffer */
__global__ __launch_bounds__(256) void k_verify_keep(const ZdBuf *__restrict__ bufs,
                                                     const uint32_t *__restrict__ blk_owner,
                                                     const ZdParseOut *__restrict__ pout,
                                                     const ZdBlockRec *__restrict__ recs,
                                                     const ZdBlockPlan *__restrict__ plans,
                                                     const ZdResult *__restrict__ res,
                                                     const DvfBuf *__restrict__ vbufs, DvfBlock *__restrict__ facts,
                                                     uint32_t *__restrict__ nblk, uint32_t nslots)
{
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= nslots)
        return;
    const uint32_t b = blk_owner[slot];
    const uint32_t blk0 = bufs[b].blk0;
    dvf_keep(&bufs[b], &pout[b], recs + blk0, plans + blk0, &res[b], slot - blk0, facts + vbufs[b].first, &nblk[b]);
}

/* 4g, on request: one wavefront per kept block of the whole plan */
__global__ __launch_bounds__(64) void k_verify_blocks(const uint8_t *__restrict__ in,
                                                      const uint8_t *__restrict__ out,
                                                      const DvfBuf *__restrict__ vbufs,
                                                      const uint32_t *__restrict__ owner,
                                                      const DvfBlock *__restrict__ facts,
                                                      const uint32_t *__restrict__ nblk,
                                                      const ZdResult *__restrict__ res,
                                                      DvfVerdict *__restrict__ verd, uint32_t wrap, uint32_t wbits,
                                                      uint32_t nslots)
{
    __shared__ DvfLds lds;
    const uint32_t slot = blockIdx.x;
    if (slot >= nslots)
        return;
    const uint32_t b = owner[slot];
    const DvfBuf buf = vbufs[b];
    const uint32_t n = nblk[b], j = slot - buf.first;
    if (j >= n || n > buf.max_blocks)
        return;
    dvf_block_item(in + buf.in_off, out + buf.out_off, &buf, facts + buf.first, n, j, res[b].out_len, wrap, wbits,
                   &lds, verd + buf.first);
}

/* 4h: one thread per buffer */
__global__ __launch_bounds__(64) void k_verify_finish(const uint8_t *__restrict__ out,
                                                      const DvfBuf *__restrict__ vbufs,
                                                      const DvfBlock *__restrict__ facts,
                                                      const DvfVerdict *__restrict__ verd,
                                                      const uint32_t *__restrict__ nblk,
                                                      const ZdResult *__restrict__ res, uint32_t wrap,
                                                      uint32_t wbits, uint32_t level, uint32_t strategy,
                                                      DvfResult *__restrict__ results, uint32_t nbuf)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nbuf)
        return;
    const uint32_t n = nblk[b] <= vbufs[b].max_blocks ? nblk[b] : 0u;
    dvf_finish(out + vbufs[b].out_off, &vbufs[b], facts + vbufs[b].first, verd + vbufs[b].first, n, &res[b], wrap,
               wbits, level, strategy, &results[b]);
}

/* kernels 4i-4l (pack.h): a plan's results packed into one image, only for a plan with packing enabled, and
 * zsc_hip_unpack.  The offsets: one wavefront per PK_SCAN_B values of a level of the scan -- 4i the sums of a
 * level that one wavefront cannot take alone, 4j the scan of the top level by one wavefront, 4k the levels
 * below it with the bases from the level above.  vals == null: the values are the item lengths rounded up to
 * align; out may be vals */
__global__ __launch_bounds__(64) void k_pack_reduce(PkLens lens, uint32_t align, const uint64_t *vals, uint64_t n,
                                                    uint64_t *sums)
{
    pk_scan_block(lens, align, vals, n, blockIdx.x, nullptr, nullptr, sums);
}

__global__ __launch_bounds__(64) void k_pack_scan_sums(PkLens lens, uint32_t align, const uint64_t *vals, uint64_t n,
                                                       uint64_t *out)
{
    pk_scan_block(lens, align, vals, n, 0, nullptr, out, nullptr);
}

__global__ __launch_bounds__(64) void k_pack_apply(PkLens lens, uint32_t align, const uint64_t *vals, uint64_t n,
                                                   const uint64_t *base, uint64_t *out)
{
    pk_scan_block(lens, align, vals, n, blockIdx.x, base, out, nullptr);
}

/* 4l: one wavefront per tile of the dense image, in either direction */
__global__ __launch_bounds__(64) void k_pack_move(PkMove M, uint8_t *dense, uint8_t *sparse)
{
    pk_move_tile(M, dense, sparse, blockIdx.x);
}

/* kernels 4m-4o (bgzf.h): a gzip plan's streams as BGZF files, only for a plan with zsc_hip_deflate_plan_bgzf_enable.
 * 4m one wavefront per file: its length; the files' offsets are 4i-4k over those lengths; 4n one wavefront per
 * file (and one more): the offsets of the members and the tails; 4o one wavefront per tile of the image */
__global__ __launch_bounds__(64) void k_bgzf_file_len(BzFiles F, uint64_t *file_len)
{
    bz_file_len(F, blockIdx.x, file_len);
}

__global__ __launch_bounds__(64) void k_bgzf_member_off(BzFiles F, const uint64_t *file_off, uint64_t *parts)
{
    bz_member_off(F, blockIdx.x, file_off, parts);
}

__global__ __launch_bounds__(64) void k_bgzf_move(BzMove M, uint8_t *image, const uint8_t *out)
{
    bz_move_tile(M, image, out, blockIdx.x);
}

/* kernels 4p-4r (zip.h): a gzip plan's streams as ZIP archives, only for a plan with zsc_hip_deflate_plan_zip_enable.
 * 4p one wavefront per archive: its length and state; the archives' offsets are 4i-4k over those lengths; 4q one
 * wavefront per archive (and one more): the offsets of the entries, the directory records and the ends; 4r one
 * wavefront per tile of the image */
__global__ __launch_bounds__(64) void k_zip_arch_len(ZpArchives A, uint64_t *arch_len, uint32_t *arch_st)
{
    zp_arch_len(A, blockIdx.x, arch_len, arch_st);
}

__global__ __launch_bounds__(64) void k_zip_part_off(ZpArchives A, const uint64_t *arch_off, uint64_t *parts)
{
    zp_part_off(A, blockIdx.x, arch_off, parts);
}

__global__ __launch_bounds__(64) void k_zip_move(ZpMove M, uint8_t *image, const uint8_t *out, const uint8_t *names)
{
    zp_move_tile(M, image, out, names, blockIdx.x);
}

/* one stream of an inflate batch */
typedef struct {
    uint64_t src_off, dst_off;
    uint32_t src_len, dst_cap;
} ZdInfItem;

/* kernel 5: one group of INF_GROUP lanes per compressed stream, 64 / INF_GROUP streams per wavefront */
#define INF_PER_WAVE (64 / INF_GROUP)
#ifndef INF_WAVES_EU
#define INF_WAVES_EU 5 /* 96 VGPRs, with 8 KiB of LDS per wave (512-byte stages): 20 waves per CU */
#endif
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(INF_WAVES_EU, INF_WAVES_EU))) void k_inflate(const uint8_t *__restrict__ src,
                                                uint8_t *__restrict__ dst,
                                                const ZdInfItem *__restrict__ items,
                                                const uint32_t *__restrict__ order,
                                                InfResult *__restrict__ res,
                                                InfResume *__restrict__ resume,
                                                uint32_t *__restrict__ pending, int32_t window_bits,
                                                uint32_t count)
{
    __shared__ InfLds lds_all[INF_PER_WAVE];
    __shared__ uint32_t crc_table[1][256];
    const uint32_t grp = (threadIdx.x & 63u) / INF_GROUP;
    InfLds *lds = &lds_all[grp];
    if ((threadIdx.x & (INF_GROUP - 1u)) == 0)
        lds->cktab = crc_table;
    /* every group takes streams from one queue (pending[1], longest output first) until it is
     * empty: streams of one length still differ a lot in decoding time (a table-like member has
     * a third of a text member's symbols), and with a fixed four streams per wavefront the
     * groups that finish early idle until the slowest one is done */
    for (;;) {
        uint32_t slot = 0;
        if ((threadIdx.x & (INF_GROUP - 1u)) == 0)
            slot = atomicAdd(pending + 1, 1u);
        slot = (uint32_t)__shfl((int)slot, (int)(threadIdx.x & (64u - INF_GROUP)));
        if (slot >= count)
            break;
        const uint32_t i = order[slot];
        if (resume[i].state == 2u)
            continue; /* finished in an earlier launch (only streams that resynchronise come back) */
        const ZdInfItem it = items[i];
        InfJob job;
        job.src = src + it.src_off;
        job.n = it.src_len;
        job.dst = dst + it.dst_off;
        job.cap = it.dst_cap;
        job.window_bits = window_bits;
        if (inflate_stream(job, lds, &res[i], &resume[i])) {
            if ((threadIdx.x & (INF_GROUP - 1u)) == 0)
                atomicAdd(pending, 1u); /* the host launches once more for these */
        }
    }
}

/* kernel 5d: k_inflate for a plan with preset dictionaries (zsc_hip_inflate_plan_dict_enable): the same queue,
 * the dictionary variant of the decoder.  A stream's dictionary is one of the plan's window images (imgs,
 * INF_WIN bytes each: the INF_SEC_EXTWIN layout) or none; the images are shared by all the streams that use
 * them and stay in L2.  k_inflate itself never sees a dictionary: a plan without them launches it as ever. */
typedef struct {
    uint32_t len, id; /* the whole dictionary's length and Adler-32 */
} ZdInfDict;

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(INF_WAVES_EU, INF_WAVES_EU))) void k_inflate_dict(
    const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const ZdInfItem *__restrict__ items,
    const uint32_t *__restrict__ order, InfResult *__restrict__ res, InfResume *__restrict__ resume,
    uint32_t *__restrict__ pending, int32_t window_bits, uint32_t count, const uint8_t *__restrict__ imgs,
    const ZdInfDict *__restrict__ dicts, const uint32_t *__restrict__ dict_of)
{
    __shared__ InfLds lds_all[INF_PER_WAVE];
    __shared__ uint32_t crc_table[1][256];
    const uint32_t grp = (threadIdx.x & 63u) / INF_GROUP;
    InfLds *lds = &lds_all[grp];
    if ((threadIdx.x & (INF_GROUP - 1u)) == 0)
        lds->cktab = crc_table;
    for (;;) {
        uint32_t slot = 0;
        if ((threadIdx.x & (INF_GROUP - 1u)) == 0)
            slot = atomicAdd(pending + 1, 1u);
        slot = (uint32_t)__shfl((int)slot, (int)(threadIdx.x & (64u - INF_GROUP)));
        if (slot >= count)
            break;
        const uint32_t i = order[slot];
        if (resume[i].state == 2u)
            continue;
        const ZdInfItem it = items[i];
        InfJob job;
        job.src = src + it.src_off;
        job.n = it.src_len;
        job.dst = dst + it.dst_off;
        job.cap = it.dst_cap;
        job.window_bits = window_bits;
        const uint32_t d = dict_of[i];
        InfDict dc = {nullptr, 0u, 0u};
        if (d != ZSC_HIP_NO_DICT) {
            dc.win = imgs + (uint64_t)d * INF_WIN;
            dc.len = dicts[d].len;
            dc.id = dicts[d].id;
        }
        if (inflate_stream<INF_SEC_DICT>(job, lds, &res[i], &resume[i], nullptr, nullptr, (void *)nullptr, &dc)) {
            if ((threadIdx.x & (INF_GROUP - 1u)) == 0)
                atomicAdd(pending, 1u);
        }
    }
}

/* the plan's dictionaries made ready, one wavefront each: the id is the Adler-32 of the whole dictionary as
 * given (whole + at[d], 16-byte aligned), the image its last min(len, INF_WIN) bytes, right-aligned */
__global__ __launch_bounds__(64) void k_dict_setup(const uint8_t *__restrict__ whole, const uint64_t *__restrict__ at,
                                                   ZdInfDict *__restrict__ dicts, uint8_t *__restrict__ imgs)
{
    const uint32_t d = blockIdx.x;
    const uint8_t *in = whole + at[d];
    const uint32_t n = dicts[d].len;
    const uint32_t id = ck_adler32(in, n);
    if (threadIdx.x == 0)
        dicts[d].id = id;
    const uint32_t have = n < INF_WIN ? n : INF_WIN;
    uint8_t *img = imgs + (uint64_t)d * INF_WIN + (INF_WIN - have);
    for (uint32_t k = threadIdx.x; k < have; k += 64u)
        img[k] = in[n - have + k];
}

/* kernel 6 (inflate_sections.h): the full-flush sections of each stream inflated in parallel, in
 * six launches ahead of k_inflate */
__global__ __launch_bounds__(64) void k_sec_scan(const uint8_t *__restrict__ src, IsecPlan P, int write)
{
    for (uint32_t t = blockIdx.x; t < P.ntiles; t += gridDim.x)
        sec_scan_tile(P, src, t, write);
}

__global__ __launch_bounds__(64) void k_sec_setup(IsecPlan P)
{
    const uint32_t na = UNI(*P.q);
    for (uint32_t a = blockIdx.x; a < na; a += gridDim.x)
        sec_setup(P, a);
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(INF_WAVES_EU, INF_WAVES_EU))) void k_sec_count(
    const uint8_t *__restrict__ src, IsecPlan P)
{
    __shared__ InfLds lds_all[INF_PER_WAVE];
    __shared__ InfSecInfo info[INF_PER_WAVE];
    __shared__ uint32_t crc_table[1][256];
    const uint32_t grp = (threadIdx.x & 63u) / INF_GROUP;
    if ((threadIdx.x & (INF_GROUP - 1u)) == 0)
        lds_all[grp].cktab = crc_table;
    sec_count_worker(P, src, &lds_all[grp], &info[grp]);
}

__global__ __launch_bounds__(64) void k_sec_resolve(IsecPlan P)
{
    const uint32_t na = *P.q;
    for (uint32_t a = blockIdx.x * INF_PER_WAVE + (threadIdx.x & 63u) / INF_GROUP; a < na; a += gridDim.x * INF_PER_WAVE)
        sec_resolve(P, a);
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(INF_WAVES_EU, INF_WAVES_EU))) void k_sec_write(
    const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, IsecPlan P)
{
    __shared__ InfLds lds_all[INF_PER_WAVE];
    __shared__ InfSecInfo info[INF_PER_WAVE];
    __shared__ uint32_t crc_table[1][256];
    const uint32_t grp = (threadIdx.x & 63u) / INF_GROUP;
    if ((threadIdx.x & (INF_GROUP - 1u)) == 0)
        lds_all[grp].cktab = crc_table;
    sec_write_worker(P, src, dst, &lds_all[grp], &info[grp]);
}

__global__ __launch_bounds__(64) void k_sec_finish(const uint8_t *__restrict__ src, IsecPlan P,
                                                   InfResult *__restrict__ res, InfResume *__restrict__ resume)
{
    const uint32_t na = *P.q;
    for (uint32_t a = blockIdx.x * INF_PER_WAVE + (threadIdx.x & 63u) / INF_GROUP; a < na; a += gridDim.x * INF_PER_WAVE)
        sec_finish(P, src, res, resume, a);
}

/* kernel 12 (inflate_members.h): multi-member gzip files inflated member by member: the sections plan's
 * k_sec_setup between two scans for member headers, then claims, count, resolve, write, finish and the
 * serial step, which is the plan's whole-stream decode (k_inflate does not run on a members plan) */
__global__ __launch_bounds__(64) void k_mem_scan(const uint8_t *__restrict__ src, MemPlan M, int write)
{
    for (uint32_t t = blockIdx.x; t < M.sp.ntiles; t += gridDim.x)
        mem_scan_tile(M, src, t, write);
}

__global__ __launch_bounds__(64) void k_mem_claims(const uint8_t *__restrict__ src, MemPlan M)
{
    const uint32_t na = UNI(*M.sp.q);
    for (uint32_t a = blockIdx.x; a < na; a += gridDim.x)
        mem_claims(M, src, a);
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(INF_WAVES_EU, INF_WAVES_EU))) void k_mem_count(
    const uint8_t *__restrict__ src, MemPlan M)
{
    __shared__ InfLds lds_all[INF_PER_WAVE];
    __shared__ InfResult r[INF_PER_WAVE];
    __shared__ InfResume rs[INF_PER_WAVE];
    __shared__ uint32_t crc_table[1][256];
    const uint32_t grp = (threadIdx.x & 63u) / INF_GROUP;
    if ((threadIdx.x & (INF_GROUP - 1u)) == 0)
        lds_all[grp].cktab = crc_table;
    mem_count_worker(M, src, &lds_all[grp], &r[grp], &rs[grp]);
}

__global__ __launch_bounds__(64) void k_mem_resolve(MemPlan M)
{
    const uint32_t na = *M.sp.q;
    for (uint32_t a = blockIdx.x * INF_PER_WAVE + (threadIdx.x & 63u) / INF_GROUP; a < na; a += gridDim.x * INF_PER_WAVE)
        mem_resolve(M, a);
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(INF_WAVES_EU, INF_WAVES_EU))) void k_mem_write(
    const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, MemPlan M)
{
    __shared__ InfLds lds_all[INF_PER_WAVE];
    __shared__ InfResult r[INF_PER_WAVE];
    __shared__ InfResume rs[INF_PER_WAVE];
    __shared__ uint32_t crc_table[1][256];
    const uint32_t grp = (threadIdx.x & 63u) / INF_GROUP;
    if ((threadIdx.x & (INF_GROUP - 1u)) == 0)
        lds_all[grp].cktab = crc_table;
    mem_write_worker(M, src, dst, &lds_all[grp], &r[grp], &rs[grp]);
}

__global__ __launch_bounds__(64) void k_mem_finish(MemPlan M, InfResult *__restrict__ res, InfResume *__restrict__ resume)
{
    const uint32_t na = *M.sp.q;
    for (uint32_t a = blockIdx.x * INF_PER_WAVE + (threadIdx.x & 63u) / INF_GROUP; a < na; a += gridDim.x * INF_PER_WAVE)
        mem_finish(M, res, resume, a);
}

/* (the serial step loops over members and over re-entries around the decoder, which costs registers
 * (inflate.h, at inflate_stream): it is left to the occupancy the compiler finds, not held to k_inflate's) */
template <bool SIZE>
__global__ __launch_bounds__(64) void k_mem_serial(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, MemPlan M,
                                                   InfResult *__restrict__ res, InfResume *__restrict__ resume)
{
    __shared__ InfLds lds_all[INF_PER_WAVE];
    __shared__ InfResult r[INF_PER_WAVE];
    __shared__ InfResume rs[INF_PER_WAVE];
    __shared__ uint32_t crc_table[1][256];
    const uint32_t grp = (threadIdx.x & 63u) / INF_GROUP;
    if ((threadIdx.x & (INF_GROUP - 1u)) == 0)
        lds_all[grp].cktab = crc_table;
    for (uint32_t s = blockIdx.x * INF_PER_WAVE + grp; s < M.sp.count; s += gridDim.x * INF_PER_WAVE)
        mem_serial<SIZE>(M, src, dst, &lds_all[grp], &r[grp], &rs[grp], res, resume, s);
}

/* kernel 14 (bgzf_read.h): BGZF ranges.  The index: the members plan's scan, setup and claims launches as they
 * are, then k_bgi_chain, a lane group per file, and k_bgi_gather, a wavefront per file, which moves the tables
 * from the room a file might have needed to the room it needs.  A ranges plan: k_bgr_range, lane groups taking
 * member jobs from one queue, each group with BGR_SLOT bytes of `stage`, and k_bgr_finish, a lane per request. */
__global__ __launch_bounds__(64) void k_bgi_chain(const uint8_t *__restrict__ src, MemPlan M,
                                                  const uint64_t *__restrict__ tbase, uint64_t *__restrict__ coff,
                                                  uint64_t *__restrict__ uoff, uint32_t *__restrict__ members)
{
    for (uint32_t s = blockIdx.x * INF_PER_WAVE + (threadIdx.x & 63u) / INF_GROUP; s < M.sp.count;
         s += gridDim.x * INF_PER_WAVE)
        bgi_chain(M, src, s, coff + tbase[s], uoff + tbase[s], tbase[s + 1u] - tbase[s], &members[s]);
}

__global__ __launch_bounds__(64) void k_bgi_gather(const uint64_t *__restrict__ tbase, const uint64_t *__restrict__ first,
                                                   const uint64_t *__restrict__ coff, const uint64_t *__restrict__ uoff,
                                                   uint64_t *__restrict__ table, uint64_t total, uint32_t nfiles)
{
    for (uint32_t f = blockIdx.x; f < nfiles; f += gridDim.x) {
        const uint64_t n = first[f + 1u] - first[f];
        for (uint64_t k = threadIdx.x; k < n; k += 64u) {
            table[first[f] + k] = coff[tbase[f] + k];
            table[total + first[f] + k] = uoff[tbase[f] + k];
        }
    }
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(INF_WAVES_EU, INF_WAVES_EU))) void k_bgr_range(
    const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, uint8_t *__restrict__ stage, BgrPlan B)
{
    __shared__ InfLds lds_all[INF_PER_WAVE];
    __shared__ InfResult r[INF_PER_WAVE];
    __shared__ InfResume rs[INF_PER_WAVE];
    __shared__ uint32_t crc_table[1][256];
    const uint32_t grp = (threadIdx.x & 63u) / INF_GROUP;
    if ((threadIdx.x & (INF_GROUP - 1u)) == 0)
        lds_all[grp].cktab = crc_table;
    bgr_worker(B, src, dst, stage + (uint64_t)(blockIdx.x * INF_PER_WAVE + grp) * BGR_SLOT, &lds_all[grp], &r[grp],
               &rs[grp]);
}

__global__ __launch_bounds__(64) void k_bgr_finish(BgrPlan B, const InfResult *__restrict__ res0,
                                                   InfResult *__restrict__ res)
{
    for (uint32_t i = blockIdx.x * 64u + threadIdx.x; i < B.count; i += gridDim.x * 64u)
        bgr_finish(B, res0, res, i);
}

/* kernel 7 (inflate_chunks.h): any stream inflated in parallel from block starts found by trial, in
 * six launches ahead of k_sec_finish and k_inflate */
__global__ __launch_bounds__(64) void k_chk_setup(IchkPlan P)
{
    for (uint32_t a = blockIdx.x; a < P.nactive; a += gridDim.x)
        chk_setup(P, a);
}

__global__ __launch_bounds__(64) void k_chk_scan(const uint8_t *__restrict__ src, IchkPlan P)
{
    for (uint32_t t = blockIdx.x; t < P.sp.ntiles; t += gridDim.x)
        chk_scan(P, src, t);
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(INF_WAVES_EU, INF_WAVES_EU))) void k_chk_count(
    const uint8_t *__restrict__ src, IchkPlan P)
{
    __shared__ InfLds lds_all[INF_PER_WAVE];
    __shared__ InfSecInfo info[INF_PER_WAVE];
    __shared__ InfPiece piece[INF_PER_WAVE];
    __shared__ uint32_t crc_table[1][256];
    const uint32_t grp = (threadIdx.x & 63u) / INF_GROUP;
    if ((threadIdx.x & (INF_GROUP - 1u)) == 0)
        lds_all[grp].cktab = crc_table;
    chk_count_worker<false>(P, src, &lds_all[grp], &info[grp], &piece[grp]);
}

__global__ __launch_bounds__(64) void k_chk_want(IchkPlan P)
{
    for (uint32_t a = blockIdx.x; a < P.nactive; a += gridDim.x)
        chk_want(P, a);
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(INF_WAVES_EU, INF_WAVES_EU))) void k_chk_retry(
    const uint8_t *__restrict__ src, IchkPlan P)
{
    __shared__ InfLds lds_all[INF_PER_WAVE];
    __shared__ InfSecInfo info[INF_PER_WAVE];
    __shared__ InfPiece piece[INF_PER_WAVE];
    __shared__ uint32_t crc_table[1][256];
    const uint32_t grp = (threadIdx.x & 63u) / INF_GROUP;
    if ((threadIdx.x & (INF_GROUP - 1u)) == 0)
        lds_all[grp].cktab = crc_table;
    chk_count_worker<true>(P, src, &lds_all[grp], &info[grp], &piece[grp]);
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(INF_WAVES_EU, INF_WAVES_EU))) void k_chk_resolve(
    const uint8_t *__restrict__ src, IchkPlan P)
{
    __shared__ InfLds lds_all[INF_PER_WAVE];
    __shared__ InfSecInfo info[INF_PER_WAVE];
    __shared__ InfPiece piece[INF_PER_WAVE];
    __shared__ uint32_t crc_table[1][256];
    const uint32_t grp = (threadIdx.x & 63u) / INF_GROUP;
    if ((threadIdx.x & (INF_GROUP - 1u)) == 0)
        lds_all[grp].cktab = crc_table;
    for (uint32_t a = blockIdx.x * INF_PER_WAVE + grp; a < P.nactive; a += gridDim.x * INF_PER_WAVE)
        chk_resolve(P, src, &lds_all[grp], &info[grp], &piece[grp], a);
}

#define CHK_WINDOW_THREADS 1024
__global__ __launch_bounds__(CHK_WINDOW_THREADS) void k_chk_window(IchkPlan P)
{
    for (uint32_t a = blockIdx.x; a < P.nactive; a += gridDim.x)
        chk_windows(P, P.sp.active[a], threadIdx.x, CHK_WINDOW_THREADS, [] { __syncthreads(); });
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(INF_WAVES_EU, INF_WAVES_EU))) void k_chk_write(
    const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, IchkPlan P)
{
    __shared__ InfLds lds_all[INF_PER_WAVE];
    __shared__ InfSecInfo info[INF_PER_WAVE];
    __shared__ InfPiece piece[INF_PER_WAVE];
    __shared__ uint32_t crc_table[1][256];
    const uint32_t grp = (threadIdx.x & 63u) / INF_GROUP;
    if ((threadIdx.x & (INF_GROUP - 1u)) == 0)
        lds_all[grp].cktab = crc_table;
    chk_write_worker(P, src, dst, &lds_all[grp], &info[grp], &piece[grp]);
}

/* kernel 9 (inflate_index.h): streams inflated from a seek-point index -- one launch ahead of
 * k_sec_finish and k_inflate */
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(INF_WAVES_EU, INF_WAVES_EU))) void k_idx_write(
    const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, IidxPlan P, InfResult *__restrict__ res,
    InfResume *__restrict__ resume)
{
    __shared__ InfLds lds_all[INF_PER_WAVE];
    __shared__ InfSecInfo info[INF_PER_WAVE];
    __shared__ InfPiece piece[INF_PER_WAVE];
    __shared__ uint32_t crc_table[1][256];
    const uint32_t grp = (threadIdx.x & 63u) / INF_GROUP;
    if ((threadIdx.x & (INF_GROUP - 1u)) == 0)
        lds_all[grp].cktab = crc_table;
    idx_write_worker(P, src, dst, &lds_all[grp], &info[grp], &piece[grp], res, resume);
}

/* kernel 10 (inflate_size.h): the output lengths of the streams, nothing stored.  k_inflate_size is
 * k_inflate's launch over the size decode; ahead of it a size plan with chunks runs k_chk_setup, k_chk_scan
 * and k_chk_want unchanged and these over the piece count variant */
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(INF_WAVES_EU, INF_WAVES_EU))) void k_inflate_size(
    const uint8_t *__restrict__ src, const ZdInfItem *__restrict__ items, const uint32_t *__restrict__ order,
    InfResult *__restrict__ res, InfResume *__restrict__ resume, uint32_t *__restrict__ pending, int32_t window_bits,
    uint32_t count)
{
    __shared__ InfLds lds_all[INF_PER_WAVE];
    __shared__ uint32_t crc_table[1][256]; /* (the header CRC of a gzip member is over input bytes: it stays) */
    const uint32_t grp = (threadIdx.x & 63u) / INF_GROUP;
    InfLds *lds = &lds_all[grp];
    if ((threadIdx.x & (INF_GROUP - 1u)) == 0)
        lds->cktab = crc_table;
    /* one queue, as k_inflate (pending[1]; longest input first) */
    for (;;) {
        uint32_t slot = 0;
        if ((threadIdx.x & (INF_GROUP - 1u)) == 0)
            slot = atomicAdd(pending + 1, 1u);
        slot = (uint32_t)__shfl((int)slot, (int)(threadIdx.x & (64u - INF_GROUP)));
        if (slot >= count)
            break;
        const uint32_t i = order[slot];
        if (resume[i].state == 2u)
            continue; /* finished by the chunked path, or in an earlier launch */
        const ZdInfItem it = items[i];
        InfJob job;
        job.src = src + it.src_off;
        job.n = it.src_len;
        job.dst = nullptr;
        job.cap = it.dst_cap; /* the limit */
        job.window_bits = window_bits;
        if (size_stream(job, lds, &res[i], &resume[i])) {
            if ((threadIdx.x & (INF_GROUP - 1u)) == 0)
                atomicAdd(pending, 1u); /* the host launches once more for these */
        }
    }
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(INF_WAVES_EU, INF_WAVES_EU))) void k_size_count(
    const uint8_t *__restrict__ src, IchkPlan P)
{
    __shared__ InfLds lds_all[INF_PER_WAVE];
    __shared__ InfSecInfo info[INF_PER_WAVE];
    __shared__ InfPiece piece[INF_PER_WAVE];
    __shared__ uint32_t crc_table[1][256];
    const uint32_t grp = (threadIdx.x & 63u) / INF_GROUP;
    if ((threadIdx.x & (INF_GROUP - 1u)) == 0)
        lds_all[grp].cktab = crc_table;
    chk_count_worker<false, true>(P, src, &lds_all[grp], &info[grp], &piece[grp]);
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(INF_WAVES_EU, INF_WAVES_EU))) void k_size_retry(
    const uint8_t *__restrict__ src, IchkPlan P)
{
    __shared__ InfLds lds_all[INF_PER_WAVE];
    __shared__ InfSecInfo info[INF_PER_WAVE];
    __shared__ InfPiece piece[INF_PER_WAVE];
    __shared__ uint32_t crc_table[1][256];
    const uint32_t grp = (threadIdx.x & 63u) / INF_GROUP;
    if ((threadIdx.x & (INF_GROUP - 1u)) == 0)
        lds_all[grp].cktab = crc_table;
    chk_count_worker<true, true>(P, src, &lds_all[grp], &info[grp], &piece[grp]);
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(INF_WAVES_EU, INF_WAVES_EU))) void k_size_resolve(
    const uint8_t *__restrict__ src, IchkPlan P)
{
    __shared__ InfLds lds_all[INF_PER_WAVE];
    __shared__ InfSecInfo info[INF_PER_WAVE];
    __shared__ InfPiece piece[INF_PER_WAVE];
    __shared__ uint32_t crc_table[1][256];
    const uint32_t grp = (threadIdx.x & 63u) / INF_GROUP;
    if ((threadIdx.x & (INF_GROUP - 1u)) == 0)
        lds_all[grp].cktab = crc_table;
    for (uint32_t a = blockIdx.x * INF_PER_WAVE + grp; a < P.nactive; a += gridDim.x * INF_PER_WAVE)
        chk_resolve<true>(P, src, &lds_all[grp], &info[grp], &piece[grp], a);
}

__global__ __launch_bounds__(64) void k_size_finish(const uint8_t *__restrict__ src, IchkPlan P,
                                                    InfResult *__restrict__ res, InfResume *__restrict__ resume)
{
    for (uint32_t a = blockIdx.x * INF_PER_WAVE + (threadIdx.x & 63u) / INF_GROUP; a < P.nactive;
         a += gridDim.x * INF_PER_WAVE)
        size_finish(P, src, res, resume, a);
}

/* kernel 11 (inflate_check.h): the streams checked, nothing stored.  k_inflate_check is k_inflate's queue
 * loop over the ring variant, each lane group with CHK_RING bytes of `rings`; ahead of it a check plan with
 * chunks runs the chunks plan's launches with k_check_write in place of k_chk_write, and k_check_finish
 * behind k_sec_finish */
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(INF_WAVES_EU, INF_WAVES_EU))) void k_inflate_check(
    const uint8_t *__restrict__ src, uint8_t *__restrict__ rings, const ZdInfItem *__restrict__ items,
    const uint32_t *__restrict__ order, InfResult *__restrict__ res, InfResume *__restrict__ resume,
    uint32_t *__restrict__ values, uint32_t *__restrict__ pending, int32_t window_bits, uint32_t count)
{
    __shared__ InfLds lds_all[INF_PER_WAVE];
    __shared__ uint32_t crc_table[1][256];
    const uint32_t grp = (threadIdx.x & 63u) / INF_GROUP;
    InfLds *lds = &lds_all[grp];
    if ((threadIdx.x & (INF_GROUP - 1u)) == 0)
        lds->cktab = crc_table;
    InfCheck ck;
    ck.ring = rings + (uint64_t)(blockIdx.x * INF_PER_WAVE + grp) * CHK_RING;
    /* one queue, as k_inflate (pending[1]; longest input first); the next stream reuses the ring */
    for (;;) {
        uint32_t slot = 0;
        if ((threadIdx.x & (INF_GROUP - 1u)) == 0)
            slot = atomicAdd(pending + 1, 1u);
        slot = (uint32_t)__shfl((int)slot, (int)(threadIdx.x & (64u - INF_GROUP)));
        if (slot >= count)
            break;
        const uint32_t i = order[slot];
        if (resume[i].state == 2u)
            continue; /* finished by the chunked path */
        const ZdInfItem it = items[i];
        InfJob job;
        job.src = src + it.src_off;
        job.n = it.src_len;
        job.dst = nullptr;
        job.cap = it.dst_cap; /* the limit */
        job.window_bits = window_bits;
        if (check_stream(job, lds, &res[i], &resume[i], &ck, &values[i])) {
            if ((threadIdx.x & (INF_GROUP - 1u)) == 0)
                atomicAdd(pending, 1u); /* the host launches k_inflate_size for these */
        }
    }
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(INF_WAVES_EU, INF_WAVES_EU))) void k_check_write(
    const uint8_t *__restrict__ src, IchkPlan P)
{
    __shared__ InfLds lds_all[INF_PER_WAVE];
    __shared__ InfSecInfo info[INF_PER_WAVE];
    __shared__ InfPiece piece[INF_PER_WAVE];
    __shared__ uint32_t crc_table[1][256];
    const uint32_t grp = (threadIdx.x & 63u) / INF_GROUP;
    if ((threadIdx.x & (INF_GROUP - 1u)) == 0)
        lds_all[grp].cktab = crc_table;
    chk_check_worker(P, src, &lds_all[grp], &info[grp], &piece[grp]);
}

__global__ __launch_bounds__(64) void k_check_finish(IchkPlan P, const InfResume *__restrict__ resume,
                                                     uint32_t *__restrict__ values)
{
    for (uint32_t a = blockIdx.x * INF_PER_WAVE + (threadIdx.x & 63u) / INF_GROUP; a < P.nactive;
         a += gridDim.x * INF_PER_WAVE)
        check_finish(P, resume, values, a);
}

/* the export of a chunks plan's index: the records of stream s's chain, each window's place in the
 * gathered buffer by a prefix sum of the window lengths (one workgroup, IDX_REC_THREADS records a step);
 * then the windows, cut down to what their pieces reach, copied to their places */
#define IDX_REC_THREADS 1024
__global__ __launch_bounds__(IDX_REC_THREADS) void k_idx_records(IchkPlan P, uint32_t s, uint32_t n, ZidxRec *recs,
                                                                 uint64_t *total)
{
    __shared__ uint32_t sc[IDX_REC_THREADS];
    __shared__ uint64_t carry;
    const uint32_t tid = threadIdx.x;
    if (tid == 0)
        carry = 0;
    __syncthreads();
    for (uint32_t b = 0; b < n; b += IDX_REC_THREADS) {
        const uint32_t i = b + tid;
        ZidxRec r = {};
        if (i < n)
            idx_record(P, s, i, &r);
        sc[tid] = r.wlen;
        __syncthreads();
        for (uint32_t d = 1; d < IDX_REC_THREADS; d <<= 1) {
            const uint32_t v = tid >= d ? sc[tid - d] : 0u;
            __syncthreads();
            sc[tid] += v;
            __syncthreads();
        }
        if (i < n) {
            r.woff = carry + (sc[tid] - r.wlen);
            recs[i] = r;
        }
        __syncthreads();
        if (tid == IDX_REC_THREADS - 1u)
            carry += sc[tid];
        __syncthreads();
    }
    if (tid == 0)
        *total = carry;
}

#define IDX_GATHER_THREADS 256
__global__ __launch_bounds__(IDX_GATHER_THREADS) void k_idx_gather(IchkPlan P, uint32_t s, uint32_t n,
                                                                   const ZidxRec *__restrict__ recs,
                                                                   uint8_t *__restrict__ out)
{
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x)
        idx_gather(P, s, i, &recs[i], out, threadIdx.x, IDX_GATHER_THREADS);
}

/* kernel 8 (inflate_resync.h): damaged full-flush streams inflated in parallel, with inflateSync's
 * resynchronisation; k_sec_scan and k_sec_setup, then these four, ahead of k_inflate */
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(INF_WAVES_EU, INF_WAVES_EU))) void k_rsy_count(
    const uint8_t *__restrict__ src, IrsyPlan R)
{
    __shared__ InfLds lds_all[INF_PER_WAVE];
    __shared__ InfSecErr info[INF_PER_WAVE];
    __shared__ uint32_t crc_table[1][256];
    const uint32_t grp = (threadIdx.x & 63u) / INF_GROUP;
    if ((threadIdx.x & (INF_GROUP - 1u)) == 0)
        lds_all[grp].cktab = crc_table;
    rsy_count_worker(R, src, &lds_all[grp], &info[grp]);
}

__global__ __launch_bounds__(64) void k_rsy_resolve(const uint8_t *__restrict__ src, IrsyPlan R)
{
    const uint32_t na = *R.sp.q;
    for (uint32_t a = blockIdx.x * INF_PER_WAVE + (threadIdx.x & 63u) / INF_GROUP; a < na; a += gridDim.x * INF_PER_WAVE)
        rsy_resolve(R, src, a);
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(INF_WAVES_EU, INF_WAVES_EU))) void k_rsy_write(
    const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, IrsyPlan R)
{
    __shared__ InfLds lds_all[INF_PER_WAVE];
    __shared__ InfSecInfo info[INF_PER_WAVE];
    __shared__ uint32_t crc_table[1][256];
    const uint32_t grp = (threadIdx.x & 63u) / INF_GROUP;
    if ((threadIdx.x & (INF_GROUP - 1u)) == 0)
        lds_all[grp].cktab = crc_table;
    rsy_write_worker(R, src, dst, &lds_all[grp], &info[grp]);
}

__global__ __launch_bounds__(64) void k_rsy_finish(const uint8_t *__restrict__ src, IrsyPlan R,
                                                   InfResult *__restrict__ res, InfResume *__restrict__ resume)
{
    const uint32_t na = *R.sp.q;
    for (uint32_t a = blockIdx.x * INF_PER_WAVE + (threadIdx.x & 63u) / INF_GROUP; a < na; a += gridDim.x * INF_PER_WAVE)
        rsy_finish(R, src, res, resume, a);
}

/* ------------------------------------------------------------------------ */
/* host runtime                                                             */
/* ------------------------------------------------------------------------ */

namespace {

std::once_flag g_init_once;
int g_init_status = Z_STREAM_ERROR;
int g_device = -1; /* the device this process's plans, scratch and kernels live on */
int g_cus = 256;    /* its compute units */
char g_device_info[256] = "uninitialised";

#define HIP_TRY(expr, fail)                                                              \
    do {                                                                                 \
        hipError_t _e = (expr);                                                          \
        if (_e != hipSuccess) {                                                          \
            ZSC_WARN2("zsc_hip: %s failed: %s", #expr, hipGetErrorString(_e));           \
            fail;                                                                        \
        }                                                                                \
    } while (0)

size_t g_dev_cache_cap = 4ull << 30; /* DevCache: bytes of freed device memory kept at most */

void do_init(int ordinal)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) {
        ZSC_WARN("zsc_hip: no HIP device is visible; this library has no CPU path.");
        g_init_status = Z_STREAM_ERROR;
        return;
    }
    if (ordinal < 0) {
        /* one process per GPU: LOCAL_RANK names it; without it, the device the calling thread
         * works on already (never silently device 0 under somebody else's feet) */
        const char *lr = getenv("LOCAL_RANK");
        int cur = 0;
        if (lr)
            ordinal = atoi(lr) % count;
        else
            ordinal = hipGetDevice(&cur) == hipSuccess ? cur : 0;
    }
    if (hipSetDevice(ordinal) != hipSuccess) {
        ZSC_WARN1("zsc_hip: cannot select device %d.", ordinal);
        g_init_status = Z_STREAM_ERROR;
        return;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, ordinal) != hipSuccess) {
        g_init_status = Z_STREAM_ERROR;
        return;
    }
    g_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    snprintf(g_device_info, sizeof g_device_info, "%s | %s | %d CUs | %.1f GiB", prop.name,
             prop.gcnArchName, prop.multiProcessorCount,
             (double)prop.totalGlobalMem / (1024.0 * 1024.0 * 1024.0));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        ZSC_WARN1("zsc_hip: built for gfx950 only, found %s.", prop.gcnArchName);
        g_init_status = Z_STREAM_ERROR;
        return;
    }
    g_dev_cache_cap = prop.totalGlobalMem / 4;
    if (const char *e = getenv("ZSC_HIP_CACHE_MB"))
        g_dev_cache_cap = (size_t)atoll(e) << 20;
    g_device = ordinal;
    g_init_status = Z_OK;
}

/* HIP's current device is a property of the calling THREAD.  Every entry point that touches
 * the device runs inside one of these: it selects the library's device for the call and puts
 * the thread's own choice back afterwards, so a caller (or another library) that works on a
 * different GPU is not disturbed, and a second thread does not launch on its default device
 * against memory that lives on ours. */
void ensure_init();
struct DeviceScope {
    int prev = -1;
    bool changed = false;
    DeviceScope()
    {
        ensure_init();
        if (g_device >= 0 && hipGetDevice(&prev) == hipSuccess && prev != g_device)
            changed = hipSetDevice(g_device) == hipSuccess;
    }
    ~DeviceScope()
    {
        if (changed)
            (void)hipSetDevice(prev);
    }
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
};

/* Freed device blocks, kept for the next plan.  The one-shot entry points (zsc_compress ...)
 * build and drop a plan per call and the sections path one per round; hipMalloc / hipFree cost
 * a tenth of a millisecond each, hipFree waits for the device and takes ~30 ms per GB it
 * unmaps -- with ~16 B of scratch per input byte that was two thirds of a sections call.  At
 * most g_dev_cache_cap bytes (a quarter of the device's memory; ZSC_HIP_CACHE_MB) in kMaxBlocks blocks
 * are kept (ZSC_HIP_NO_CACHE: none); a block serves a request of at least half its size. */
struct DevCache {
    static constexpr size_t kMaxBlocks = 96;
    std::mutex mu;
    std::vector<std::pair<size_t, void *>> blocks;
    size_t held = 0;
    bool off = getenv("ZSC_HIP_NO_CACHE") != nullptr;

    void *take(size_t need, size_t *got)
    {
        std::lock_guard<std::mutex> lock(mu);
        size_t best = blocks.size();
        for (size_t i = 0; i < blocks.size(); i++)
            if (blocks[i].first >= need && blocks[i].first <= 2 * need + (1u << 16) &&
                (best == blocks.size() || blocks[i].first < blocks[best].first))
                best = i;
        if (best == blocks.size())
            return nullptr;
        void *p = blocks[best].second;
        *got = blocks[best].first;
        held -= blocks[best].first;
        blocks[best] = blocks.back();
        blocks.pop_back();
        return p;
    }
    bool give(void *p, size_t bytes)
    {
        std::lock_guard<std::mutex> lock(mu);
        if (off || blocks.size() >= kMaxBlocks || held + bytes > g_dev_cache_cap)
            return false;
        blocks.push_back(std::make_pair(bytes, p));
        held += bytes;
        return true;
    }
    void trim()
    {
        std::lock_guard<std::mutex> lock(mu);
        for (auto &b : blocks)
            (void)hipFree(b.second);
        blocks.clear();
        held = 0;
    }
};
DevCache g_dev_cache;

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    bool ensure(size_t need)
    {
        if (need <= bytes)
            return true;
        release();
        if (need == 0)
            need = 16;
        p = g_dev_cache.take(need, &bytes);
        if (p)
            return true;
        if (hipMalloc(&p, need) != hipSuccess) {
            (void)hipGetLastError(); /* (the error is sticky: it must not be charged to the next launch) */
            g_dev_cache.trim(); /* what is kept may be what is missing */
            if (hipMalloc(&p, need) != hipSuccess) {
                (void)hipGetLastError();
                p = nullptr;
                ZSC_WARN1("zsc_hip: hipMalloc of %zu bytes failed.", need);
                return false;
            }
        }
        bytes = need;
        return true;
    }
    /* the caller has waited for the work that used the block */
    void release()
    {
        if (p && !g_dev_cache.give(p, bytes))
            (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};

/* The streams rule (zsc_hip.h, "Streams"): a plan has one set of scratch, so what it enqueues is ordered on the
 * device whatever streams it is given, and the host waits only in _results, the accessors and _destroy.  One of
 * these per kind of work -- a plan's runs, its verifications, its packs: the stream the last enqueue of the kind
 * went to and an event (hipEventDisableTiming) recorded behind it.  A plan that only ever sees one stream pays
 * one event record per enqueue and never a hipStreamWaitEvent. */
struct Enqueued {
    hipEvent_t done = nullptr;
    hipStream_t stream = nullptr;
    bool pending = false;          /* enqueued since the host last waited for this kind */
    std::vector<hipStream_t> left; /* streams a chain of runs has left behind since then (work_chain) */
};

/* the host waits for the work of the kind: before its results are read or its blocks go back to the cache */
hipError_t work_wait(Enqueued &w)
{
    if (!w.pending)
        return hipSuccess;
    hipError_t rc = hipSuccess;
    for (hipStream_t s : w.left) {
        const hipError_t e = hipStreamSynchronize(s);
        rc = rc == hipSuccess ? e : rc;
    }
    w.left.clear();
    const hipError_t e = hipStreamSynchronize(w.stream);
    w.pending = false;
    return rc == hipSuccess ? e : rc;
}

/* what is enqueued on `st` from here on comes after the work of the kind, wherever that went: a wait on the
 * device where it went to another stream (the same stream orders it by itself) */
void work_order(Enqueued &w, hipStream_t st)
{
    if (!w.pending || w.stream == st)
        return;
    if (w.done == nullptr || hipStreamWaitEvent(st, w.done, 0) != hipSuccess) {
        (void)hipGetLastError();
        (void)work_wait(w); /* no event to wait for: the host waits */
    }
}

/* the same before a run that follows the plan's earlier run: the runs form a chain, so the end of the last one
 * is the end of them all; the stream the chain leaves is kept for work_wait, which waits for it too */
void work_chain(Enqueued &w, hipStream_t st)
{
    work_order(w, st);
    if (w.pending && w.stream != st && std::find(w.left.begin(), w.left.end(), w.stream) == w.left.end())
        w.left.push_back(w.stream);
}

/* behind the last launch of an enqueue on `st` */
void work_note(Enqueued &w, hipStream_t st)
{
    if (w.done == nullptr && hipEventCreateWithFlags(&w.done, hipEventDisableTiming) != hipSuccess)
        w.done = nullptr; /* (the error stays for the caller's hipGetLastError; work_order then waits on the host) */
    if (w.done)
        (void)hipEventRecord(w.done, st);
    w.stream = st;
    w.pending = true;
}

void work_release(Enqueued &w)
{
    if (w.done)
        (void)hipEventDestroy(w.done);
    w = Enqueued();
}

/* a group of buffers that shares one set of scratch arrays (deflate_plan_layout.h), and its descriptors on the device */
struct SubBatch : DplSubShape {
    DevBuf d_bufs, d_tile_owner, d_blk_owner, d_order;
};

/* Packing (pack.h): what a plan of either kind holds for it, and the launches */
struct PackState {
    bool on = false, ran = false;
    uint32_t count = 0, align = 0;
    std::vector<uint32_t> caps; /* the most each item takes */
    uint64_t max_total = 0;     /* ... and the image */
    uint64_t cap = 0;           /* packed_cap of the last pack */
    DevBuf d_off;               /* count + 1 dense offsets, written by every pack */
    DevBuf d_sparse;            /* count slot offsets */
    DevBuf d_sums;              /* the scan's levels above the items: n[k] + 1 values each */
    uint32_t levels = 1;
    uint64_t level_n[PK_MAX_LEVELS] = {0}, level_at[PK_MAX_LEVELS] = {0};
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipStream_t stream = nullptr;
    Enqueued work; /* the packs, for the plan's next run and its destroy */
    uint64_t scratch = 0;
};

bool pack_align_ok(U32 align)
{
    return align >= 1u && align <= 4096u && (align & (align - 1u)) == 0u;
}

void pack_set_align(PackState &ps, U32 align)
{
    ps.align = align;
    ps.max_total = 0;
    for (uint32_t c : ps.caps)
        ps.max_total += ((uint64_t)c + (align - 1u)) & ~(uint64_t)(align - 1u);
}

void pack_release(PackState &ps, uint64_t *scratch_bytes)
{
    ps.d_off.release();
    ps.d_sparse.release();
    ps.d_sums.release();
    for (hipEvent_t &e : ps.ev) {
        if (e)
            (void)hipEventDestroy(e);
        e = nullptr;
    }
    work_release(ps.work);
    if (scratch_bytes)
        *scratch_bytes -= ps.scratch;
    ps.scratch = 0;
    ps.on = ps.ran = false;
}

ZlibReturn pack_setup(PackState &ps, uint32_t count, U32 align, const uint64_t *sparse_off, const U32 *caps,
                      uint64_t *scratch_bytes)
{
    ps.count = count;
    ps.caps.assign(caps, caps + count);
    pack_set_align(ps, align);
    ps.levels = pk_scan_levels(count, ps.level_n);
    uint64_t nsums = 0;
    for (uint32_t k = 1; k < ps.levels; k++) {
        ps.level_at[k] = nsums;
        nsums += ps.level_n[k] + 1u;
    }
    bool ok = ps.d_off.ensure(((uint64_t)count + 1u) * 8u) && ps.d_sparse.ensure(std::max<uint64_t>(count, 1) * 8u) &&
              ps.d_sums.ensure(std::max<uint64_t>(nsums, 1) * 8u);
    ok = ok && (count == 0 || hipMemcpy(ps.d_sparse.p, sparse_off, 8ull * count, hipMemcpyHostToDevice) == hipSuccess) &&
         hipEventCreate(&ps.ev[0]) == hipSuccess && hipEventCreate(&ps.ev[1]) == hipSuccess;
    ps.scratch = ps.d_off.bytes + ps.d_sparse.bytes + ps.d_sums.bytes;
    *scratch_bytes += ps.scratch;
    if (!ok) {
        (void)hipGetLastError();
        pack_release(ps, scratch_bytes);
        return Z_MEM_ERROR;
    }
    ps.on = true;
    return Z_OK;
}

/* An exclusive prefix sum of level_n[0] values into out0 (one more entry: the sum): reduce up the levels, scan the
 * top one, apply down.  The values are vals0[] or, without vals0, the lengths `lens` names rounded up to align;
 * out0 may be vals0.  sums: the levels above, level k at level_at[k]. */
void scan_enqueue(uint32_t levels, const uint64_t *level_n, const uint64_t *level_at, uint64_t *sums,
                  const PkLens &lens, uint32_t align, uint64_t *vals0, uint64_t *out0, hipStream_t st)
{
    auto vals = [&](uint32_t k) { return k == 0 ? vals0 : sums + level_at[k]; };
    auto out = [&](uint32_t k) { return k == 0 ? out0 : sums + level_at[k]; };
    for (uint32_t k = 0; k + 1u < levels; k++)
        hipLaunchKernelGGL(k_pack_reduce, dim3((uint32_t)level_n[k + 1u]), dim3(64), 0, st, lens, align,
                           (const uint64_t *)vals(k), level_n[k], vals(k + 1u));
    const uint32_t top = levels - 1u;
    hipLaunchKernelGGL(k_pack_scan_sums, dim3(1), dim3(64), 0, st, lens, align, (const uint64_t *)vals(top),
                       level_n[top], out(top));
    for (uint32_t k = top; k-- > 0;)
        hipLaunchKernelGGL(k_pack_apply, dim3((uint32_t)level_n[k + 1u]), dim3(64), 0, st, lens, align,
                           (const uint64_t *)vals(k), level_n[k], (const uint64_t *)vals(k + 1u), out(k));
}

/* the dense offsets of the items whose lengths `lens` names */
void pack_scan_enqueue(const PackState &ps, const PkLens &lens, hipStream_t st)
{
    scan_enqueue(ps.levels, ps.level_n, ps.level_at, (uint64_t *)ps.d_sums.p, lens, ps.align, nullptr,
                 (uint64_t *)ps.d_off.p, st);
}

ZlibReturn pack_enqueue(PackState &ps, const PkLens &lens, const void *d_sparse_image, void *d_packed,
                        uint64_t packed_cap, hipStream_t st)
{
    if (!ps.on || ((uintptr_t)d_packed & 15u) || ((uintptr_t)d_sparse_image & 15u))
        return Z_STREAM_ERROR;
    /* the grid comes from the capacity; what the image can be at the most bounds it */
    const uint64_t tiles = (std::min(packed_cap, ps.max_total) + PK_TILE - 1u) / PK_TILE;
    if (tiles > 0x7fffffffull)
        return Z_MEM_ERROR;
    if (tiles && (d_packed == Z_NULL || d_sparse_image == Z_NULL))
        return Z_STREAM_ERROR;
    (void)hipGetLastError();
    if (ps.ran && ps.stream != st) /* the offsets of the one before may still be in use */
        HIP_TRY(hipStreamSynchronize(ps.stream), return Z_STREAM_ERROR);
    ps.stream = st;
    ps.ran = true;
    ps.cap = packed_cap;
    (void)hipEventRecord(ps.ev[0], st);
    pack_scan_enqueue(ps, lens, st);
    if (tiles) {
        PkMove M;
        M.off = (const uint64_t *)ps.d_off.p;
        M.sparse_off = (const uint64_t *)ps.d_sparse.p;
        M.lens = lens;
        M.count = ps.count;
        M.unpack = 0;
        M.cap = packed_cap;
        hipLaunchKernelGGL(k_pack_move, dim3((uint32_t)tiles), dim3(64), 0, st, M, (uint8_t *)d_packed,
                           (uint8_t *)const_cast<void *>(d_sparse_image));
    }
    (void)hipEventRecord(ps.ev[1], st);
    work_note(ps.work, st);
    HIP_TRY(hipGetLastError(), return Z_STREAM_ERROR);
    return Z_OK;
}

ZlibReturn pack_fetch(PackState &ps, uint64_t *offsets, uint64_t *total, float *ms)
{
    if (ms)
        *ms = 0.f;
    if (total)
        *total = 0;
    if (!ps.on || !ps.ran)
        return Z_STREAM_ERROR;
    HIP_TRY(hipStreamSynchronize(ps.stream), return Z_STREAM_ERROR);
    uint64_t tot = 0;
    if (offsets) {
        HIP_TRY(hipMemcpy(offsets, ps.d_off.p, ((size_t)ps.count + 1u) * 8u, hipMemcpyDeviceToHost), return Z_STREAM_ERROR);
        tot = offsets[ps.count];
    } else {
        HIP_TRY(hipMemcpy(&tot, (const uint64_t *)ps.d_off.p + ps.count, 8, hipMemcpyDeviceToHost), return Z_STREAM_ERROR);
    }
    if (total)
        *total = tot;
    if (ms)
        (void)hipEventElapsedTime(ms, ps.ev[0], ps.ev[1]);
    return tot > ps.cap ? Z_BUF_ERROR : Z_OK;
}

/* dense image -> slots: the offsets are the caller's, so no scan; d_table: count + 1 dense offsets, d_lens: count
 * lengths, d_slots: count slot offsets, all on the device already */
void unpack_enqueue(uint32_t count, uint64_t total, const void *d_packed, const void *d_table, const void *d_lens,
                    void *d_dst, const void *d_slots, hipStream_t st)
{
    const uint64_t tiles = (total + PK_TILE - 1u) / PK_TILE;
    if (!tiles)
        return;
    PkMove M;
    M.off = (const uint64_t *)d_table;
    M.sparse_off = (const uint64_t *)d_slots;
    M.lens.rec = (const uint32_t *)d_lens;
    M.lens.stride_w = 1;
    M.lens.len_w = 0;
    M.lens.st_w = PK_NO_STATUS;
    M.count = count;
    M.unpack = 1;
    M.cap = ~0ull;
    hipLaunchKernelGGL(k_pack_move, dim3((uint32_t)tiles), dim3(64), 0, st, M,
                       (uint8_t *)const_cast<void *>(d_packed), (uint8_t *)d_dst);
}

/* the host side of an unpack: the table of count + 1 offsets from the caller's; false where the items do not
 * lie in ascending order without overlap, or a slot is not 16-byte aligned */
bool unpack_table(uint32_t count, const uint64_t *packed_offsets, const U32 *lens, const uint64_t *dst_offsets,
                  std::vector<uint64_t> &table)
{
    table.assign((size_t)count + 1u, 0);
    for (uint32_t i = 0; i < count; i++) {
        table[i] = packed_offsets[i];
        const uint64_t end = packed_offsets[i] + lens[i];
        if ((dst_offsets[i] & 15u) || end < packed_offsets[i] || (i + 1u < count && end > packed_offsets[i + 1u]))
            return false;
        table[i + 1u] = end;
    }
    return true;
}

/* BGZF files (bgzf.h): what a gzip deflate plan holds for them */
struct BgzfState {
    bool on = false, ran = false;
    uint32_t count = 0, nfiles = 0, align = 0;
    std::vector<uint32_t> file_first; /* nfiles + 1 */
    uint64_t max_total = 0;           /* the most the image takes */
    uint64_t cap = 0;                 /* image_cap of the last _bgzf */
    DevBuf d_first;                   /* file_first */
    DevBuf d_file_off;                /* nfiles + 1: the files' lengths, scanned in place into their offsets */
    DevBuf d_parts;                   /* count + nfiles + 1 offsets of the members and the tails */
    DevBuf d_what;                    /* count + nfiles: what each part is */
    DevBuf d_slots;                   /* count slot offsets */
    DevBuf d_sums;                    /* the scan's levels above the files */
    uint32_t levels = 1;
    uint64_t level_n[PK_MAX_LEVELS] = {0}, level_at[PK_MAX_LEVELS] = {0};
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipStream_t stream = nullptr;
    Enqueued work; /* the _bgzf calls, for the plan's next run and its destroy */
    uint64_t scratch = 0;
};

/* (the caller has waited for the work) */
void bgzf_release(BgzfState &bs, uint64_t *scratch_bytes)
{
    for (DevBuf *b : {&bs.d_first, &bs.d_file_off, &bs.d_parts, &bs.d_what, &bs.d_slots, &bs.d_sums})
        b->release();
    for (hipEvent_t &e : bs.ev) {
        if (e)
            (void)hipEventDestroy(e);
        e = nullptr;
    }
    work_release(bs.work);
    if (scratch_bytes)
        *scratch_bytes -= bs.scratch;
    bs.scratch = 0;
    bs.on = bs.ran = false;
}

/* ZIP archives (zip.h): what a gzip deflate plan holds for them */
struct ZipState {
    bool on = false, ran = false, has_datetime = false;
    uint32_t count = 0, narchives = 0, align = 0, flags = 0;
    std::vector<uint32_t> arch_first; /* narchives + 1 */
    std::vector<uint64_t> name_off;   /* count + 1 */
    uint64_t nparts = 0;
    uint64_t max_total = 0;           /* the most the image takes */
    uint64_t cap = 0;                 /* image_cap of the last _zip */
    DevBuf d_first;                   /* arch_first */
    DevBuf d_fixed;                   /* narchives: ZpLayout.fixed */
    DevBuf d_arch_off;                /* narchives + 1: the archives' lengths, scanned in place into their offsets */
    DevBuf d_arch_st;                 /* narchives: ZP_ST_* */
    DevBuf d_parts;                   /* nparts + 1 offsets */
    DevBuf d_kinds;                   /* nparts: what each part is */
    DevBuf d_arch_of;                 /* count */
    DevBuf d_slots;                   /* count slot offsets */
    DevBuf d_name_off;                /* count + 1 */
    DevBuf d_names;                   /* the names */
    DevBuf d_datetime;                /* count, where the caller gave them */
    DevBuf d_sums;                    /* the scan's levels above the archives */
    uint32_t levels = 1;
    uint64_t level_n[PK_MAX_LEVELS] = {0}, level_at[PK_MAX_LEVELS] = {0};
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipStream_t stream = nullptr;
    Enqueued work; /* the _zip calls, for the plan's next run and its destroy */
    uint64_t scratch = 0;
};

/* (the caller has waited for the work) */
void zip_release(ZipState &zs, uint64_t *scratch_bytes)
{
    for (DevBuf *b : {&zs.d_first, &zs.d_fixed, &zs.d_arch_off, &zs.d_arch_st, &zs.d_parts, &zs.d_kinds, &zs.d_arch_of,
                      &zs.d_slots, &zs.d_name_off, &zs.d_names, &zs.d_datetime, &zs.d_sums})
        b->release();
    for (hipEvent_t &e : zs.ev) {
        if (e)
            (void)hipEventDestroy(e);
        e = nullptr;
    }
    work_release(zs.work);
    if (scratch_bytes)
        *scratch_bytes -= zs.scratch;
    zs.scratch = 0;
    zs.on = zs.ran = false;
}

} // namespace

struct zsc_hip_deflate_plan {
    uint32_t count = 0;
    int level = 6, wrap = 1, wbits = 15, mem_level = 8;
    uint32_t strategy = 0;
    std::vector<ZdBuf> bufs; /* in_off / out_off are absolute in the caller's buffers */
    std::vector<SubBatch> subs;
    /* scratch shared by all sub-batches (sized for the largest) */
    DevBuf d_sorted, d_tmp_syms, d_rank, d_hib, d_cnt, d_dir, d_recs, d_plans, d_pout;
    DevBuf d_seg_tok; /* per long buffer: token staging of the segmented parser (tokens, then token indices) */
    DevBuf d_r2; /* the match table (match_table.h): one entry per input position */
    bool use_table = false;
    uint32_t table_min = 0; /* buffers longer than this have a table (those the segmented parser takes) */
    uint32_t table_cap = MT_CAP;
    uint32_t stair_min = SG_STAIR_MIN; /* chains at least this long are searched as a staircase (lz_parse_seg.h) */
    DevBuf d_sched;               /* joints of runs of sections (sections.h) */
    bool use_seg = true;
    /* read from the environment once, when the plan is made (A/B and debugging): a plan cannot get a mixed
     * configuration and the launch path looks nothing up */
    bool seg_pipe = true;     /* ZSC_HIP_SEG_PIPE=0: plain buffers in super-steps too (lz_parse_seg.h) */
    int seg_ring_said = 0;    /* ZSC_HIP_SEG_RING: 1 wide, 2 narrow, 0 nothing said -- each sub-batch goes by the workgroups
                                 it offers a CU (SubBatch::seg_narrow) */
    bool link_kernel = false; /* ZSC_HIP_LINK_KERNEL: k_link_prev runs even where the parser could do without */
    bool fast_ring = false;   /* ZSC_HIP_FAST_RING: levels 1-3 with the window in an LDS ring */
    DevBuf d_res; /* one ZdResult per buffer of the whole plan */
    uint64_t rank_base_off = 0;
    bool profile = false;
    float times[ZSC_HIP_NKERNELS] = {0};
    std::vector<hipEvent_t> events; /* ZSC_HIP_NKERNELS per sub-batch per profiled run */
    size_t events_used = 0;
    uint32_t profiled_runs = 0;
    hipStream_t last_stream = nullptr;
    Enqueued ran; /* the runs; the verifications and packs keep their own (vf_work, pack.work) */
    uint64_t scratch_bytes = 0;
    /* the seek-point index (deflate_index.h), off unless zsc_hip_deflate_plan_index_enable was called */
    bool idx_on = false;
    bool sectioned = false;       /* a plan of runs of sections: takes no index */
    uint32_t idx_chunk = 0;       /* chunk_bytes of the blobs */
    DevBuf d_idx_reach;           /* per block slot of a sub-batch: R_b (shared by the sub-batches) */
    DevBuf d_idx_recs;            /* per buffer of the plan: out_cap / chunk_bytes + 1 records */
    DevBuf d_idx_rec_off;         /* count + 1 first records (u64) */
    DevBuf d_idx_npts;            /* per buffer: records written by the last run */
    std::vector<uint64_t> idx_rec_off;
    uint64_t idx_scratch = 0;     /* what of scratch_bytes the index holds */
    bool idx_valid = false;       /* between _results and the next _run */
    std::vector<ZdResult> idx_res;   /* the last run's results */
    std::vector<uint32_t> idx_npts;  /* ... and point counts */
    std::map<uint32_t, std::pair<std::vector<ZidxRec>, uint64_t>> idx_cache; /* records (woff set), window bytes */
    std::vector<hipEvent_t> idx_events; /* 2 per sub-batch per profiled run */
    size_t idx_events_used = 0;
    /* read-back verification (deflate_verify.h), off unless zsc_hip_deflate_plan_verify_enable was called */
    bool vf_on = false;
    bool vf_valid = false;        /* between _results and the next _run */
    bool vf_ran = false;          /* a _verify since then */
    uint32_t vf_slots = 0;        /* block slots of the whole plan */
    DevBuf d_vf_bufs;             /* DvfBuf per buffer */
    DevBuf d_vf_owner;            /* per block slot: its buffer */
    DevBuf d_vf_facts;            /* per block slot: DvfBlock, kept by every run */
    DevBuf d_vf_verd;             /* per block slot: DvfVerdict of the last _verify */
    DevBuf d_vf_nblk;             /* per buffer: blocks kept by the last run */
    DevBuf d_vf_res;              /* per buffer: DvfResult of the last _verify */
    std::vector<DvfBuf> vf_bufs;
    std::vector<ZdResult> vf_run_res; /* the last run's results */
    uint64_t vf_scratch = 0;      /* what of scratch_bytes verification holds */
    hipEvent_t vf_ev[2] = {nullptr, nullptr};
    hipStream_t vf_stream = nullptr;
    Enqueued vf_work;
    /* packing (pack.h), off unless zsc_hip_deflate_plan_pack_enable was called */
    PackState pack;
    /* BGZF files (bgzf.h), off unless zsc_hip_deflate_plan_bgzf_enable was called */
    BgzfState bgzf;
    /* ZIP archives (zip.h), off unless zsc_hip_deflate_plan_zip_enable was called */
    ZipState zip;
};

/* is the plan one k_parse_seg_narrow is built for?  Plain buffers in the pipeline schedule that would otherwise
 * take k_parse_seg<false, false, 6 or 0> */
static bool zsc_plan_narrow_able(const zsc_hip_deflate_plan *pl)
{
    return pl->use_seg && pl->seg_pipe && pl->d_sched.p == nullptr && !pl->use_table && pl->wbits == 15 &&
           pl->mem_level == 8;
}
/* sub-batches of the plan whose segmented parser runs in the narrow geometry, and in the wide one */
static void zsc_plan_seg_rings(const zsc_hip_deflate_plan *pl, uint32_t *wide, uint32_t *narrow)
{
    *wide = *narrow = 0;
    for (const SubBatch &sb : pl->subs)
        if (pl->use_seg && sb.cseg > 0)
            (sb.seg_narrow && zsc_plan_narrow_able(pl) ? *narrow : *wide)++;
}

namespace {
void ensure_init()
{
    int before = -1;
    (void)hipGetDevice(&before);
    std::call_once(g_init_once, do_init, -1);
    if (before >= 0 && getenv("LOCAL_RANK") == nullptr)
        (void)hipSetDevice(before); /* (do_init selects the device it adopts; a no-op here) */
}
} // namespace

extern "C" I32 zsc_hip_init(I32 device_ordinal)
{
    int before = -1;
    (void)hipGetDevice(&before);
    std::call_once(g_init_once, do_init, (int)device_ordinal);
    if (g_init_status == Z_OK && device_ordinal >= 0 && device_ordinal != g_device) {
        ZSC_WARN2("zsc_hip: already initialised on device %d, cannot move to device %d.", g_device,
                  (int)device_ordinal);
        return Z_STREAM_ERROR;
    }
    /* the calling thread keeps the device it had unless it asked for this one by number */
    if (device_ordinal < 0 && before >= 0 && getenv("LOCAL_RANK") == nullptr)
        (void)hipSetDevice(before);
    return g_init_status;
}

extern "C" void zsc_hip_release_cached_memory(void)
{
    DeviceScope scope;
    g_dev_cache.trim();
}

extern "C" const char *zsc_hip_device_info(void)
{
    (void)zsc_hip_init(-1);
    return g_device_info;
}

/* reference deflateBoundNoStream + zsc_compress_get_max_output_size2; defined in zsc_api.c */
extern "C" ZlibReturn zsc_compress_get_max_output_size2(U32, U32, I32, I32, I32, U32 *);

extern "C" ZlibReturn zsc_hip_deflate_plan_layout(U32 count, const U32 *source_lens, I32 level,
                                                  I32 window_bits, I32 mem_level,
                                                  uint64_t *in_offsets, uint64_t *out_offsets,
                                                  U32 *out_caps, uint64_t *in_bytes,
                                                  uint64_t *out_bytes)
{
    ZSC_ASSERT(source_lens != Z_NULL);
    ZSC_ASSERT(in_offsets != Z_NULL);
    ZSC_ASSERT(out_offsets != Z_NULL);
    ZSC_ASSERT(out_caps != Z_NULL);
    uint64_t io = 0, oo = 0;
    for (U32 i = 0; i < count; i++) {
        U32 cap = 0;
        const U32 n = source_lens[i];
        ZlibReturn rc = zsc_compress_get_max_output_size2(n, n ? n : 1, level, window_bits,
                                                          mem_level, &cap);
        if (rc != Z_OK)
            return rc;
        in_offsets[i] = io;
        out_offsets[i] = oo;
        out_caps[i] = cap;
        io += ((uint64_t)n + 15u) & ~15ull;
        oo += ((uint64_t)cap + 16u + 15u) & ~15ull;
    }
    if (in_bytes)
        *in_bytes = io + 64;
    if (out_bytes)
        *out_bytes = oo + 64;
    return Z_OK;
}

static ZlibReturn plan_create(zsc_hip_deflate_plan **plan_out, U32 count, const U32 *source_lens,
                              const uint64_t *in_offsets, const uint64_t *out_offsets,
                              const U32 *out_caps, I32 level, I32 window_bits, I32 mem_level,
                              ZlibStrategy strategy, const PlanRuns *runs);

/* the host waits for everything the plan has enqueued, whatever streams it went to */
static hipError_t plan_wait_all(zsc_hip_deflate_plan *pl)
{
    const hipError_t a = work_wait(pl->ran), b = work_wait(pl->vf_work), c = work_wait(pl->pack.work),
                     d = work_wait(pl->bgzf.work), e = work_wait(pl->zip.work);
    return a != hipSuccess ? a : b != hipSuccess ? b : c != hipSuccess ? c : d != hipSuccess ? d : e;
}

/* gives back what zsc_hip_deflate_plan_index_enable took (the caller has waited for the plan's work) */
static void index_release(zsc_hip_deflate_plan *pl)
{
    pl->d_idx_reach.release();
    pl->d_idx_recs.release();
    pl->d_idx_rec_off.release();
    pl->d_idx_npts.release();
    pl->scratch_bytes -= pl->idx_scratch;
    pl->idx_scratch = 0;
    pl->idx_on = false;
    pl->idx_valid = false;
    pl->idx_cache.clear();
}

/* the same for zsc_hip_deflate_plan_verify_enable */
static void verify_release(zsc_hip_deflate_plan *pl)
{
    pl->d_vf_bufs.release();
    pl->d_vf_owner.release();
    pl->d_vf_facts.release();
    pl->d_vf_verd.release();
    pl->d_vf_nblk.release();
    pl->d_vf_res.release();
    pl->scratch_bytes -= pl->vf_scratch;
    pl->vf_scratch = 0;
    pl->vf_on = false;
    pl->vf_valid = false;
    pl->vf_ran = false;
    work_release(pl->vf_work);
    for (hipEvent_t &e : pl->vf_ev) {
        if (e)
            (void)hipEventDestroy(e);
        e = nullptr;
    }
}

extern "C" ZlibReturn zsc_hip_deflate_plan_create(zsc_hip_deflate_plan **plan_out, U32 count,
                                                  const U32 *source_lens,
                                                  const uint64_t *in_offsets,
                                                  const uint64_t *out_offsets, const U32 *out_caps,
                                                  I32 level, I32 window_bits, I32 mem_level,
                                                  ZlibStrategy strategy)
{
    return plan_create(plan_out, count, source_lens, in_offsets, out_offsets, out_caps, level,
                       window_bits, mem_level, strategy, nullptr);
}

static ZlibReturn plan_create(zsc_hip_deflate_plan **plan_out, U32 count, const U32 *source_lens,
                              const uint64_t *in_offsets, const uint64_t *out_offsets,
                              const U32 *out_caps, I32 level, I32 window_bits, I32 mem_level,
                              ZlibStrategy strategy, const PlanRuns *runs)
{
    DeviceScope scope;
    ZSC_ASSERT(plan_out != Z_NULL);
    *plan_out = nullptr;
    if (zsc_hip_init(-1) != Z_OK)
        return Z_STREAM_ERROR;
    int wrap = 1, wbits = 15;
    if (!dpl_fold_params(&level, window_bits, mem_level, (int)strategy, &wrap, &wbits)) {
        ZSC_WARN4("zsc_hip: level %d / window_bits %d / mem_level %d / strategy %d is not "
                  "offloaded to the GPU yet (DESIGN.md, out of scope).",
                  level, window_bits, mem_level, (int)strategy);
        return Z_STREAM_ERROR;
    }

    DplKnobs knobs;
    /* input bytes per sub-batch; the scratch is ~14 B per input byte OF ONE SUB-BATCH.  Measured on
     * the x4096 batch (11.5 GB): 8 GiB sub-batches 3 641 MB/s with 165 GB of scratch, 4 GiB 3 631 MB/s
     * with 83 GB, 2 GiB 3 552 MB/s with 41 GB (the tail of every sub-batch's parse is idle time) */
    knobs.sub_limit = 4096ull << 20;
    if (const char *e = getenv("ZSC_HIP_SUBBATCH_MB"))
        knobs.sub_limit = (uint64_t)atoll(e) << 20;
    if (knobs.sub_limit < (1ull << 20))
        knobs.sub_limit = 1ull << 20;
    if (runs)
        knobs.sub_limit = ~0ull; /* the caller reads the block records back: one set of scratch arrays */
    knobs.use_seg = getenv("ZSC_HIP_NO_SEG") == nullptr;
    /* buffers longer than this go to the segmented parser.  Measured on the x4096 batch: 18 432
     * (round 1: what fits the small rings stays with the wave-per-buffer parser) 2 843 + 37 ms of
     * parsing, 8 192: 2 853 + 13 ms, 3 072: 2 853 + 0 ms -- a workgroup per 4 KiB file still
     * beats a wave per file */
    static const uint32_t seg_min = getenv("ZSC_HIP_SEG_MIN") ? (uint32_t)atoi(getenv("ZSC_HIP_SEG_MIN")) : 3072u;
    knobs.seg_min = seg_min;
    knobs.full_ring_only = getenv("ZSC_HIP_FULL_RING") != nullptr;
    if (const char *e = getenv("ZSC_HIP_SEG_RING"))
        knobs.ring_said = strcmp(e, "narrow") == 0 ? 2 : strcmp(e, "wide") == 0 ? 1 : 0;
    knobs.cus = (uint32_t)g_cus;

    DplLayout L;
    uint32_t bad = 0;
    const int lrc = dpl_layout(count, source_lens, in_offsets, out_offsets, out_caps, level, wrap, wbits, mem_level,
                               (int)strategy, runs, knobs, L, &bad);
    if (lrc == DPL_MEM_ERROR) {
        ZSC_WARN2("zsc_hip: buffer %u has %u bytes; one buffer (or one run of sections) is limited "
                  "to 535 822 335 bytes.", bad, source_lens[bad]);
        return Z_MEM_ERROR;
    }
    if (lrc != DPL_OK) {
        ZSC_WARN1("zsc_hip: buffer %u is not 16-byte aligned in the batch.", bad);
        return Z_STREAM_ERROR;
    }

    auto *pl = new zsc_hip_deflate_plan();
    pl->count = count;
    pl->level = level;
    pl->wrap = wrap;
    pl->wbits = wbits;
    pl->mem_level = mem_level;
    pl->strategy = (uint32_t)strategy;
    pl->sectioned = runs != nullptr;
    pl->bufs = std::move(L.bufs);
    pl->use_seg = L.use_seg;
    pl->table_min = knobs.seg_min;
    pl->seg_ring_said = knobs.ring_said;
    if (const char *e = getenv("ZSC_HIP_SEG_PIPE"))
        pl->seg_pipe = atoi(e) != 0;
    pl->link_kernel = getenv("ZSC_HIP_LINK_KERNEL") != nullptr;
    pl->fast_ring = getenv("ZSC_HIP_FAST_RING") != nullptr;
    /* per-sub-batch descriptor arrays */
    pl->subs.resize(L.subs.size());
    for (size_t j = 0; j < L.subs.size(); j++) {
        const DplSub &ls = L.subs[j];
        SubBatch &sb = pl->subs[j];
        static_cast<DplSubShape &>(sb) = ls;
        const struct {
            DevBuf *d;
            const void *src;
            uint64_t bytes;
        } up[4] = {{&sb.d_bufs, &pl->bufs[sb.first], sizeof(ZdBuf) * sb.count},
                   {&sb.d_tile_owner, ls.tile_owner.data(), 4ull * sb.ntiles},
                   {&sb.d_blk_owner, ls.blk_owner.data(), 4ull * sb.nslots},
                   {&sb.d_order, ls.order.data(), 4ull * sb.count}};
        for (const auto &u : up) {
            if (!u.d->ensure(u.bytes)) {
                zsc_hip_deflate_plan_destroy(pl);
                return Z_MEM_ERROR;
            }
            HIP_TRY(hipMemcpy(u.d->p, u.src, u.bytes, hipMemcpyHostToDevice),
                    { zsc_hip_deflate_plan_destroy(pl); return Z_MEM_ERROR; });
            pl->scratch_bytes += u.d->bytes;
        }
    }

    if (runs && runs->nsched) {
        if (!pl->d_sched.ensure(sizeof(ZdSched) * runs->nsched) ||
            hipMemcpy(pl->d_sched.p, runs->sched, sizeof(ZdSched) * runs->nsched,
                      hipMemcpyHostToDevice) != hipSuccess) {
            zsc_hip_deflate_plan_destroy(pl);
            return Z_MEM_ERROR;
        }
        pl->scratch_bytes += pl->d_sched.bytes;
    }
    if (pl->use_seg && L.max_seg) {
        if (!pl->d_seg_tok.ensure(L.max_seg * SG_SCRATCH_WORDS * 4ull)) {
            zsc_hip_deflate_plan_destroy(pl);
            return Z_MEM_ERROR;
        }
        pl->scratch_bytes += pl->d_seg_tok.bytes;
    }

    /* shared scratch: sorted (4 B/position), tmp aliased with the symbol stream
     * (4 B/position, tmp is dead once the sort kernel ends), rank (2 B/position,
     * indexed by input offset), dir (2 B/position), block records + plans */
    const uint64_t tile_words = L.max_tiles * ZD_TILE;
    bool ok = pl->d_sorted.ensure(tile_words * 4) &&
              pl->d_tmp_syms.ensure(std::max<uint64_t>(tile_words, L.max_syms) * 4) &&
              pl->d_rank.ensure(L.max_rank_span * 2) && pl->d_hib.ensure(L.max_rank_span * 2) &&
              pl->d_cnt.ensure(L.max_rank_span * 4) &&
              pl->d_dir.ensure(L.max_tiles * ZD_DIR_STRIDE * 2) &&
              pl->d_recs.ensure(L.max_slots * sizeof(ZdBlockRec)) &&
              pl->d_plans.ensure(L.max_slots * sizeof(ZdBlockPlan)) &&
              pl->d_pout.ensure(L.max_count * sizeof(ZdParseOut)) &&
              pl->d_res.ensure((uint64_t)std::max(1u, count) * sizeof(ZdResult));
    /* the match table: levels 4-9 with the default window and hash size, for the buffers the
     * segmented parser takes; the match-finding strategies (default, filtered, fixed) share it */
    /* Off unless asked for (ZSC_HIP_TABLE=1): measured on the MI355X the table
     * kernel costs what the hops it buys save -- 23 ms per 403 MB of text for 40 % of the loop tops. */
    pl->use_table = getenv("ZSC_HIP_TABLE") != nullptr && pl->use_seg && L.max_seg != 0 && wbits == 15 &&
                    mem_level == 8 && strategy != Z_HUFFMAN_ONLY && strategy != Z_RLE;
    if (const char *e = getenv("ZSC_HIP_STAIR_MIN")) /* (debugging / tuning aid) */
        pl->stair_min = (uint32_t)atoi(e);
    if (const char *e = getenv("ZSC_HIP_TABLE_CAP")) /* (debugging / tuning aid) */
        pl->table_cap = (uint32_t)atoi(e);
    if (ok && pl->use_table)
        ok = pl->d_r2.ensure(L.max_rank_span * 4);
    if (!ok) {
        zsc_hip_deflate_plan_destroy(pl);
        return Z_MEM_ERROR;
    }
    pl->scratch_bytes += pl->d_r2.bytes;
    pl->scratch_bytes += pl->d_sorted.bytes + pl->d_tmp_syms.bytes + pl->d_rank.bytes + pl->d_hib.bytes + pl->d_cnt.bytes +
                         pl->d_dir.bytes + pl->d_recs.bytes + pl->d_plans.bytes +
                         pl->d_pout.bytes + pl->d_res.bytes;
    *plan_out = pl;
    return Z_OK;
}

extern "C" void zsc_hip_deflate_plan_profile(zsc_hip_deflate_plan *plan, I32 enable)
{
    ZSC_ASSERT(plan != Z_NULL);
    plan->profile = enable != 0;
    plan->events_used = 0; /* a new measurement window starts */
    plan->idx_events_used = 0;
    plan->profiled_runs = 0;
}

/* the index of one sub-batch (deflate_index.h): reach per block, points per buffer, check value per piece */
static void index_enqueue(zsc_hip_deflate_plan *pl, const SubBatch &sb, const uint8_t *in, hipStream_t st)
{
    const ZdBuf *bufs = (const ZdBuf *)sb.d_bufs.p;
    uint32_t *reach = (uint32_t *)pl->d_idx_reach.p;
    ZidxRec *out = (ZidxRec *)pl->d_idx_recs.p;
    const uint64_t *rec_off = (const uint64_t *)pl->d_idx_rec_off.p + sb.first;
    uint32_t *npts = (uint32_t *)pl->d_idx_npts.p + sb.first;
    if (pl->profile)
        (void)hipEventRecord(pl->idx_events[pl->idx_events_used++], st);
    hipLaunchKernelGGL(k_index_reach, dim3(sb.nslots), dim3(64), 0, st, bufs, (const uint32_t *)sb.d_blk_owner.p,
                       (const uint32_t *)pl->d_tmp_syms.p, (const ZdBlockRec *)pl->d_recs.p,
                       (const ZdParseOut *)pl->d_pout.p, (const ZdBlockPlan *)pl->d_plans.p, reach, sb.nslots);
    hipLaunchKernelGGL(k_index_points, dim3((sb.count + 63) / 64), dim3(64), 0, st, bufs,
                       (const ZdParseOut *)pl->d_pout.p, (const ZdBlockRec *)pl->d_recs.p,
                       (const ZdBlockPlan *)pl->d_plans.p, (const uint32_t *)reach,
                       (const ZdResult *)pl->d_res.p + sb.first, pl->idx_chunk, out, rec_off, npts, sb.count);
    /* enough wavefronts to fill the device where the buffers are few and long */
    uint64_t most = 1;
    for (uint32_t k = 0; k < sb.count; k++)
        most = std::max(most, pl->idx_rec_off[sb.first + k + 1] - pl->idx_rec_off[sb.first + k]);
    const uint64_t want = ((uint64_t)g_cus * 16u + sb.count - 1u) / sb.count;
    const uint32_t per_buf = (uint32_t)std::min<uint64_t>(std::min(most, std::max<uint64_t>(want, 1)), 65535u);
    hipLaunchKernelGGL(k_index_check, dim3(sb.count, per_buf), dim3(64), 0, st, in, bufs, out, rec_off,
                       (const uint32_t *)npts, sb.count);
    if (pl->profile)
        (void)hipEventRecord(pl->idx_events[pl->idx_events_used++], st);
}

extern "C" ZlibReturn zsc_hip_deflate_plan_run(zsc_hip_deflate_plan *pl, const void *d_input,
                                               void *d_output, void *hip_stream)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    ZSC_ASSERT(d_input != Z_NULL);
    ZSC_ASSERT(d_output != Z_NULL);
    hipStream_t st = (hipStream_t)hip_stream;
    (void)hipGetLastError(); /* an error some earlier call on this thread left behind is not this run's */
    /* one set of scratch: behind the plan's earlier run, and behind a verification or a pack that still reads the
     * results and the block facts this run writes -- on the device, and only where they went to another stream */
    work_chain(pl->ran, st);
    work_order(pl->vf_work, st);
    work_order(pl->pack.work, st);
    work_order(pl->bgzf.work, st);
    work_order(pl->zip.work, st);
    pl->last_stream = st;
    const uint8_t *in = (const uint8_t *)d_input;
    uint8_t *out = (uint8_t *)d_output;
    const ZdLevel cfg = dpl_level(pl->level, pl->wbits, pl->mem_level);

    const size_t nev = pl->events_used + pl->subs.size() * ZSC_HIP_NKERNELS;
    if (pl->profile) {
        while (pl->events.size() < nev) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e), return Z_MEM_ERROR);
            pl->events.push_back(e);
        }
        pl->profiled_runs++;
    }
    if (pl->vf_on) {
        pl->vf_valid = false;
        pl->vf_ran = false;
    }
    if (pl->idx_on) {
        pl->idx_valid = false;
        pl->idx_cache.clear();
        if (pl->profile)
            while (pl->idx_events.size() < pl->idx_events_used + pl->subs.size() * 2) {
                hipEvent_t e;
                HIP_TRY(hipEventCreate(&e), return Z_MEM_ERROR);
                pl->idx_events.push_back(e);
            }
    }
    auto mark = [&]() {
        if (pl->profile)
            (void)hipEventRecord(pl->events[pl->events_used++], st);
    };

    for (SubBatch &sb : pl->subs) {
        const ZdBuf *bufs = (const ZdBuf *)sb.d_bufs.p;
        ZdResult *res = (ZdResult *)pl->d_res.p + sb.first;
        uint32_t *sorted = (uint32_t *)pl->d_sorted.p;
        uint32_t *tmp_syms = (uint32_t *)pl->d_tmp_syms.p;
        uint16_t *rank = (uint16_t *)pl->d_rank.p;
        uint16_t *hib = (uint16_t *)pl->d_hib.p;
        uint32_t *cnt = (uint32_t *)pl->d_cnt.p;
        uint16_t *dir = (uint16_t *)pl->d_dir.p;
        ZdBlockRec *recs = (ZdBlockRec *)pl->d_recs.p;
        ZdBlockPlan *plans = (ZdBlockPlan *)pl->d_plans.p;
        ZdParseOut *pout = (ZdParseOut *)pl->d_pout.p;

        mark();
        hipLaunchKernelGGL(k_checksum, dim3(sb.count), dim3(64), 0, st, in, bufs, res, sb.count);
        mark();
        /* Z_HUFFMAN_ONLY / Z_RLE look at no earlier data than the previous byte: no chains */
        const bool simple = pl->strategy == (uint32_t)Z_HUFFMAN_ONLY || pl->strategy == (uint32_t)Z_RLE;
        const bool link_in_parser = !simple && cfg.slow && sb.cseg == sb.count && !pl->use_table &&
                                    !pl->link_kernel;
        if (!simple) {
            hipLaunchKernelGGL(k_hash_sort, dim3(sb.ntiles), dim3(HS_WAVES * 64), 0, st, in, bufs,
                               (const uint32_t *)sb.d_tile_owner.p, sorted, tmp_syms, rank, dir,
                               sb.ntiles);
            /* chain lengths and the links into the previous tile, for every position -- unless every buffer of
             * the batch goes to the segmented parser, which works them out for the positions it visits */
            if (!link_in_parser)
                hipLaunchKernelGGL(k_link_prev, dim3(sb.ntiles), dim3(HS_WAVES * 64), 0, st, in, bufs,
                                   (const uint32_t *)sb.d_tile_owner.p, (const uint16_t *)dir,
                                   (const uint16_t *)rank, hib, cnt, sb.ntiles);
        }
        mark();
        if (!simple) {
            if (pl->use_table && sb.cseg > 0)
                hipLaunchKernelGGL(k_match_table, dim3(sb.ntiles), dim3(MT_WAVES * 64), 0, st, in, bufs,
                                   (const uint32_t *)sb.d_tile_owner.p, (const uint32_t *)sorted,
                                   (const uint16_t *)rank, (const uint16_t *)hib, (const uint32_t *)cnt,
                                   (uint32_t *)pl->d_r2.p, cfg, pl->table_min,
                                   pl->table_cap, sb.ntiles);
        }
        mark();
        if (simple) {
            hipLaunchKernelGGL(k_parse_simple, dim3(sb.count), dim3(64), 0, st, in, bufs, tmp_syms,
                               recs, pout, (const ZdSched *)pl->d_sched.p, cfg, sb.count);
            mark();
        } else if (cfg.slow) {
#define ZSC_LAUNCH_PARSE(LT, FIRST, COUNT)                                                       \
    if ((COUNT) > 0)                                                                             \
    hipLaunchKernelGGL(k_parse<LT>, dim3(COUNT), dim3(64), 0, st, in, bufs,                      \
                       (const uint32_t *)sb.d_order.p, (const uint32_t *)sorted,                 \
                       (const uint16_t *)rank, (const uint16_t *)hib, tmp_syms, recs, pout,      \
                       (const ZdSched *)pl->d_sched.p, cfg, (uint32_t)(FIRST), (uint32_t)(COUNT))
            if (sb.cseg > 0 && sb.seg_narrow && zsc_plan_narrow_able(pl)) {
                hipLaunchKernelGGL(pl->level == 6 && pl->strategy != (uint32_t)Z_FILTERED ? k_parse_seg_narrow<6> : k_parse_seg_narrow<0>,
                                   dim3(sb.cseg), dim3(SG_W * 64), 0, st, in, bufs,
                                   (const uint32_t *)sb.d_order.p, (const uint32_t *)sorted,
                                   (const uint16_t *)rank, (const uint16_t *)hib,
                                   (const uint32_t *)cnt, link_in_parser ? (const uint16_t *)dir : nullptr, tmp_syms, recs,
                                   pout, (uint32_t *)pl->d_seg_tok.p, cfg, pl->stair_min, 0u, sb.cseg);
            } else if (sb.cseg > 0) {
                auto kern = (pl->wbits == 15 && pl->mem_level == 8)
                                ? (pl->use_table ? k_parse_seg<false, true, 0>
                                                 : pl->level == 6 && pl->strategy != (uint32_t)Z_FILTERED ? k_parse_seg<false, false, 6>
                                                                                                          : k_parse_seg<false, false, 0>)
                                : k_parse_seg<true, false, 0>;
                hipLaunchKernelGGL(kern, dim3(sb.cseg), dim3(SG_W * 64), 0, st, in, bufs,
                                   (const uint32_t *)sb.d_order.p, (const uint32_t *)sorted,
                                   (const uint16_t *)rank, (const uint16_t *)hib,
                                   (const uint32_t *)cnt, link_in_parser ? (const uint16_t *)dir : nullptr,
                                   pl->use_table ? (const uint32_t *)pl->d_r2.p : nullptr, tmp_syms, recs,
                                   pout, (uint32_t *)pl->d_seg_tok.p,
                                   (const ZdSched *)pl->d_sched.p, cfg, pl->stair_min, pl->seg_pipe ? 1u : 0u, 0u,
                                   sb.cseg);
            }
            if (pl->d_sched.p) { /* runs with joints: the parsers keep a hole map (lz_parse.h) */
                ZSC_LAUNCH_PARSE(LzLdsJ, sb.cseg, sb.c36 - sb.cseg);
                mark();
                ZSC_LAUNCH_PARSE(LzLdsJ16k, sb.c36, sb.c16 - sb.c36);
                ZSC_LAUNCH_PARSE(LzLdsJ8k, sb.c16, sb.c8 - sb.c16);
                ZSC_LAUNCH_PARSE(LzLdsJ4k, sb.c8, sb.count - sb.c8);
            } else {
                ZSC_LAUNCH_PARSE(LzLds, sb.cseg, sb.c36 - sb.cseg);
                mark();
                ZSC_LAUNCH_PARSE(LzLds16k, sb.c36, sb.c16 - sb.c36);
                ZSC_LAUNCH_PARSE(LzLds8k, sb.c16, sb.c8 - sb.c16);
                ZSC_LAUNCH_PARSE(LzLds4k, sb.c8, sb.count - sb.c8);
            }
#undef ZSC_LAUNCH_PARSE
        } else
            hipLaunchKernelGGL(pl->fast_ring ? k_parse_fast<LzLdsFast> : k_parse_fast<LzLdsFastG>,
                               dim3(sb.count), dim3(64), 0, st, in, bufs,
                               (const uint32_t *)sb.d_order.p, (const uint32_t *)sorted,
                               (const uint16_t *)rank, (const uint16_t *)hib, tmp_syms, recs,
                               pout, (const ZdSched *)pl->d_sched.p, cfg, sb.count);
        if (!simple && !cfg.slow)
            mark(); /* levels 1-3: one parse kernel for every length, the short-buffer slot stays empty */
        mark();
        hipLaunchKernelGGL(k_huff_plan, dim3(sb.nslots), dim3(64), 0, st, bufs,
                           (const uint32_t *)sb.d_blk_owner.p, (const uint32_t *)tmp_syms,
                           (const ZdBlockRec *)recs, (const ZdParseOut *)pout, plans, sb.nslots);
        mark();
        hipLaunchKernelGGL(k_layout, dim3((sb.count + 63) / 64), dim3(64), 0, st, bufs,
                           (const ZdParseOut *)pout, (const ZdBlockRec *)recs, plans, res, out,
                           sb.count);
        mark();
        hipLaunchKernelGGL(k_emit, dim3(sb.nslots), dim3(64), 0, st, in, bufs,
                           (const uint32_t *)sb.d_blk_owner.p, (const uint32_t *)tmp_syms,
                           (const ZdBlockRec *)recs, (const ZdParseOut *)pout,
                           (const ZdBlockPlan *)plans, out, sb.nslots);
        mark();
        if (pl->idx_on) /* before the next sub-batch reuses recs, plans and tmp_syms */
            index_enqueue(pl, sb, in, st);
        if (pl->vf_on) /* the same: the block facts of this sub-batch, out of recs and plans */
            hipLaunchKernelGGL(k_verify_keep, dim3((sb.nslots + 255) / 256), dim3(256), 0, st, bufs,
                               (const uint32_t *)sb.d_blk_owner.p, (const ZdParseOut *)pout, (const ZdBlockRec *)recs,
                               (const ZdBlockPlan *)plans, (const ZdResult *)res,
                               (const DvfBuf *)pl->d_vf_bufs.p + sb.first, (DvfBlock *)pl->d_vf_facts.p,
                               (uint32_t *)pl->d_vf_nblk.p + sb.first, sb.nslots);
    }
    work_note(pl->ran, st);
    HIP_TRY(hipGetLastError(), return Z_STREAM_ERROR);
    return Z_OK;
}

extern "C" ZlibReturn zsc_hip_deflate_plan_results(zsc_hip_deflate_plan *pl, U32 *dest_lens,
                                                   I32 *statuses)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    HIP_TRY(plan_wait_all(pl), return Z_STREAM_ERROR);
    std::vector<ZdResult> res(pl->count);
    if (pl->count)
        HIP_TRY(hipMemcpy(res.data(), pl->d_res.p, sizeof(ZdResult) * pl->count,
                          hipMemcpyDeviceToHost),
                return Z_STREAM_ERROR);
    for (uint32_t i = 0; i < pl->count; i++) {
        if (dest_lens)
            dest_lens[i] = res[i].out_len;
        if (statuses)
            statuses[i] = res[i].status;
    }
    if (pl->vf_on && !pl->vf_valid) {
        pl->vf_run_res = res;
        pl->vf_valid = true;
    }
    if (pl->idx_on && !pl->idx_valid) {
        pl->idx_npts.assign(pl->count, 0u);
        if (pl->count)
            HIP_TRY(hipMemcpy(pl->idx_npts.data(), pl->d_idx_npts.p, 4ull * pl->count, hipMemcpyDeviceToHost),
                    return Z_STREAM_ERROR);
        pl->idx_res = res;
        pl->idx_valid = true;
    }
    if (pl->profile && pl->profiled_runs) {
        /* mean per run over every run since profiling was switched on */
        for (int k = 0; k < ZSC_HIP_NKERNELS; k++)
            pl->times[k] = 0.f;
        const int NE = ZSC_HIP_NKERNELS; /* marks per sub-batch: NE-1 intervals + the whole pass */
        const size_t per_run = pl->subs.size() * NE;
        for (uint32_t r = 0; r < pl->profiled_runs; r++) {
            const size_t e0 = (size_t)r * per_run;
            for (size_t s = 0; s < pl->subs.size(); s++) {
                for (int k = 0; k < NE - 1; k++) {
                    float ms = 0.f;
                    (void)hipEventElapsedTime(&ms, pl->events[e0 + s * NE + k],
                                              pl->events[e0 + s * NE + k + 1]);
                    pl->times[k] += ms;
                }
            }
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, pl->events[e0], pl->events[e0 + per_run - 1]);
            pl->times[NE - 1] += ms;
        }
        for (int k = 0; k < ZSC_HIP_NKERNELS; k++)
            pl->times[k] /= (float)pl->profiled_runs;
    }
    return Z_OK;
}

extern "C" ZlibReturn zsc_hip_deflate_plan_times(zsc_hip_deflate_plan *pl, float *ms_out)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    ZSC_ASSERT(ms_out != Z_NULL);
    for (int k = 0; k < ZSC_HIP_NKERNELS; k++)
        ms_out[k] = pl->times[k];
    return pl->profile ? Z_OK : Z_STREAM_ERROR;
}

extern "C" uint64_t zsc_hip_deflate_plan_scratch_bytes(const zsc_hip_deflate_plan *pl)
{
    return pl ? pl->scratch_bytes : 0;
}

extern "C" U32 zsc_hip_deflate_plan_sub_batches(const zsc_hip_deflate_plan *pl)
{
    return pl ? (U32)pl->subs.size() : 0;
}

extern "C" I32 zsc_hip_deflate_plan_seg_ring(const zsc_hip_deflate_plan *pl)
{
    if (!pl || !pl->use_seg)
        return 0;
    uint32_t wide, narrow;
    zsc_plan_seg_rings(pl, &wide, &narrow);
    return narrow == 0 ? 1 : wide == 0 ? 2 : 3;
}

extern "C" I32 zsc_hip_deflate_plan_seg_schedule(const zsc_hip_deflate_plan *pl)
{
    if (!pl || !pl->use_seg)
        return 0;
    return pl->seg_pipe ? 2 : 1;
}

extern "C" void zsc_hip_deflate_plan_destroy(zsc_hip_deflate_plan *pl)
{
    DeviceScope scope;
    if (!pl)
        return;
    /* the blocks go back to the cache, not to hipFree: the runs, the verifications and the packs are waited for */
    (void)plan_wait_all(pl);
    for (SubBatch &sb : pl->subs) {
        sb.d_bufs.release();
        sb.d_tile_owner.release();
        sb.d_blk_owner.release();
        sb.d_order.release();
    }
    pl->d_sorted.release();
    pl->d_tmp_syms.release();
    pl->d_rank.release();
    pl->d_hib.release();
    pl->d_cnt.release();
    pl->d_seg_tok.release();
    pl->d_r2.release();
    pl->d_sched.release();
    pl->d_dir.release();
    pl->d_recs.release();
    pl->d_plans.release();
    pl->d_pout.release();
    pl->d_res.release();
    index_release(pl);
    verify_release(pl);
    pack_release(pl->pack, &pl->scratch_bytes);
    bgzf_release(pl->bgzf, &pl->scratch_bytes);
    zip_release(pl->zip, &pl->scratch_bytes);
    for (hipEvent_t e : pl->events)
        (void)hipEventDestroy(e);
    for (hipEvent_t e : pl->idx_events)
        (void)hipEventDestroy(e);
    work_release(pl->ran);
    delete pl;
}

/* ---- the seek-point index of a deflate plan (deflate_index.h) ------------------------------- */

extern "C" ZlibReturn zsc_hip_deflate_plan_index_enable(zsc_hip_deflate_plan *pl, U32 chunk_bytes)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    if (pl->sectioned)
        return Z_STREAM_ERROR;
    static_assert(DIX_DEFAULT_CHUNK == CHK_DEFAULT_BYTES, "one default for both sides");
    chunk_bytes = dix_chunk_bytes(chunk_bytes);
    if (pl->idx_on && pl->idx_chunk == chunk_bytes)
        return Z_OK;
    (void)plan_wait_all(pl);
    index_release(pl);
    pl->idx_rec_off.assign((size_t)pl->count + 1u, 0);
    uint64_t max_slots = 1;
    for (uint32_t i = 0; i < pl->count; i++)
        pl->idx_rec_off[i + 1u] = pl->idx_rec_off[i] + pl->bufs[i].out_cap / chunk_bytes + 1u;
    for (const SubBatch &sb : pl->subs)
        max_slots = std::max<uint64_t>(max_slots, sb.nslots);
    const uint64_t nrec = pl->idx_rec_off[pl->count];
    bool ok = pl->d_idx_reach.ensure(max_slots * 4u) && pl->d_idx_recs.ensure(std::max<uint64_t>(nrec, 1) * sizeof(ZidxRec)) &&
              pl->d_idx_rec_off.ensure(((uint64_t)pl->count + 1u) * 8u) &&
              pl->d_idx_npts.ensure(std::max(pl->count, 1u) * 4ull);
    ok = ok && hipMemcpy(pl->d_idx_rec_off.p, pl->idx_rec_off.data(), ((size_t)pl->count + 1u) * 8u,
                         hipMemcpyHostToDevice) == hipSuccess &&
         hipMemset(pl->d_idx_npts.p, 0, std::max(pl->count, 1u) * 4ull) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        index_release(pl);
        return Z_MEM_ERROR;
    }
    pl->idx_scratch = pl->d_idx_reach.bytes + pl->d_idx_recs.bytes + pl->d_idx_rec_off.bytes + pl->d_idx_npts.bytes;
    pl->scratch_bytes += pl->idx_scratch;
    pl->idx_chunk = chunk_bytes;
    pl->idx_on = true;
    return Z_OK;
}

/* the records of `buffer` from the last run, woff set by a prefix sum of the window lengths (kept until the
 * next run); Z_DATA_ERROR: the buffer has no stream, so no index */
static ZlibReturn dix_records(zsc_hip_deflate_plan *pl, U32 buffer, const std::vector<ZidxRec> **recs,
                              uint64_t *wbytes)
{
    if (!pl->idx_on || !pl->idx_valid || buffer >= pl->count)
        return Z_STREAM_ERROR;
    const uint32_t n = pl->idx_npts[buffer];
    if (pl->idx_res[buffer].status != Z_OK || n == 0u)
        return Z_DATA_ERROR;
    auto hit = pl->idx_cache.find(buffer);
    if (hit == pl->idx_cache.end()) {
        if (n > pl->idx_rec_off[buffer + 1u] - pl->idx_rec_off[buffer])
            return Z_STREAM_ERROR;
        std::vector<ZidxRec> r(n);
        HIP_TRY(hipMemcpy(r.data(), (const ZidxRec *)pl->d_idx_recs.p + pl->idx_rec_off[buffer], sizeof(ZidxRec) * n,
                          hipMemcpyDeviceToHost),
                return Z_STREAM_ERROR);
        uint64_t total = 0;
        for (ZidxRec &x : r) {
            /* (the kernels' own output; checked all the same, so that the gather stays inside the input) */
            if (x.wlen > ZIDX_WIN || x.wlen > x.off || (uint64_t)x.off + x.len > pl->bufs[buffer].in_len)
                return Z_STREAM_ERROR;
            x.woff = total;
            total += x.wlen;
        }
        hit = pl->idx_cache.emplace(buffer, std::make_pair(std::move(r), total)).first;
    }
    *recs = &hit->second.first;
    *wbytes = hit->second.second;
    return Z_OK;
}

extern "C" ZlibReturn zsc_hip_deflate_plan_index_size(zsc_hip_deflate_plan *pl, U32 buffer, uint64_t *bytes)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    ZSC_ASSERT(bytes != Z_NULL);
    *bytes = 0;
    const std::vector<ZidxRec> *recs = nullptr;
    uint64_t wbytes = 0;
    const ZlibReturn rc = dix_records(pl, buffer, &recs, &wbytes);
    if (rc == Z_OK)
        *bytes = zidx_blob_bytes((uint32_t)recs->size(), wbytes);
    return rc;
}

extern "C" ZlibReturn zsc_hip_deflate_plan_index_export(zsc_hip_deflate_plan *pl, U32 buffer, const void *d_input,
                                                        U8 *blob, uint64_t cap, uint64_t *len)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    ZSC_ASSERT(len != Z_NULL);
    *len = 0;
    const std::vector<ZidxRec> *recs = nullptr;
    uint64_t wbytes = 0;
    const ZlibReturn rc = dix_records(pl, buffer, &recs, &wbytes);
    if (rc != Z_OK)
        return rc;
    const uint32_t n = (uint32_t)recs->size();
    const uint64_t bytes = zidx_blob_bytes(n, wbytes);
    *len = bytes;
    if (cap < bytes || blob == Z_NULL)
        return Z_BUF_ERROR;
    if (wbytes) {
        if (d_input == Z_NULL)
            return Z_STREAM_ERROR;
        /* the windows, gathered from the input on the device, in one copy */
        DevBuf d_recs, d_wins;
        bool ok = d_recs.ensure(sizeof(ZidxRec) * n) && d_wins.ensure(wbytes) &&
                  hipMemcpy(d_recs.p, recs->data(), sizeof(ZidxRec) * n, hipMemcpyHostToDevice) == hipSuccess;
        if (ok) {
            const uint32_t blocks = std::max(1u, std::min(n, (uint32_t)g_cus * 8u));
            hipLaunchKernelGGL(k_index_gather, dim3(blocks), dim3(DIX_GATHER_THREADS), 0, pl->last_stream,
                               (const uint8_t *)d_input + pl->bufs[buffer].in_off, n, (const ZidxRec *)d_recs.p,
                               (uint8_t *)d_wins.p);
            ok = hipStreamSynchronize(pl->last_stream) == hipSuccess &&
                 hipMemcpy(blob + zidx_blob_bytes(n, 0), d_wins.p, wbytes, hipMemcpyDeviceToHost) == hipSuccess;
        }
        d_recs.release();
        d_wins.release();
        if (!ok)
            return Z_MEM_ERROR;
    }
    const ZidxInfo h = dix_blob_info((uint32_t)pl->wrap, pl->wbits, pl->idx_chunk, pl->idx_res[buffer].out_len,
                                     pl->bufs[buffer].in_len, n);
    zidx_write_head(blob, &h, recs->data());
    zidx_seal(blob, bytes);
    return Z_OK;
}

extern "C" ZlibReturn zsc_hip_deflate_plan_index_ms(zsc_hip_deflate_plan *pl, float *ms)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    ZSC_ASSERT(ms != Z_NULL);
    *ms = 0.f;
    if (!pl->idx_on || !pl->profile || !pl->profiled_runs || !pl->idx_valid)
        return Z_STREAM_ERROR;
    float sum = 0.f;
    for (size_t k = 0; k + 1 < pl->idx_events_used; k += 2) {
        float t = 0.f;
        (void)hipEventElapsedTime(&t, pl->idx_events[k], pl->idx_events[k + 1]);
        sum += t;
    }
    *ms = sum / (float)pl->profiled_runs;
    return Z_OK;
}

/* ---- read-back verification of a deflate plan (deflate_verify.h) ---------------------------- */

static_assert(ZSC_HIP_VERIFY_OK == DVF_OK && ZSC_HIP_VERIFY_SKIPPED == DVF_SKIPPED && ZSC_HIP_VERIFY_HEADER == DVF_HEADER &&
                  ZSC_HIP_VERIFY_BLOCK_HDR == DVF_BLOCK_HDR && ZSC_HIP_VERIFY_CODES == DVF_CODES &&
                  ZSC_HIP_VERIFY_LITERAL == DVF_LITERAL && ZSC_HIP_VERIFY_DISTANCE == DVF_DISTANCE &&
                  ZSC_HIP_VERIFY_MATCH == DVF_MATCH && ZSC_HIP_VERIFY_LENGTH == DVF_LENGTH &&
                  ZSC_HIP_VERIFY_BIT_END == DVF_BIT_END && ZSC_HIP_VERIFY_TRAILER == DVF_TRAILER,
              "the kernels' verdicts are the header's");
static_assert(sizeof(zsc_hip_verify_result) == sizeof(DvfResult) && sizeof(zsc_hip_verify_block) == sizeof(DvfBlock),
              "copied out as they are");

extern "C" ZlibReturn zsc_hip_deflate_plan_verify_enable(zsc_hip_deflate_plan *pl)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    if (pl->sectioned)
        return Z_STREAM_ERROR;
    if (pl->vf_on)
        return Z_OK;
    (void)plan_wait_all(pl);
    uint64_t slots = 0;
    pl->vf_bufs.assign(pl->count, DvfBuf());
    for (uint32_t i = 0; i < pl->count; i++) {
        const ZdBuf &b = pl->bufs[i];
        DvfBuf &v = pl->vf_bufs[i];
        v.in_off = b.in_off;
        v.out_off = b.out_off;
        v.in_len = b.in_len;
        v.out_cap = b.out_cap;
        v.first = (uint32_t)slots;
        v.max_blocks = b.max_blocks;
        slots += b.max_blocks;
        if (slots >= 0x7fffffffull) /* one launch takes a wavefront per slot */
            return Z_MEM_ERROR;
    }
    std::vector<uint32_t> owner((size_t)slots);
    for (uint32_t i = 0; i < pl->count; i++)
        std::fill(owner.begin() + pl->vf_bufs[i].first, owner.begin() + pl->vf_bufs[i].first + pl->vf_bufs[i].max_blocks, i);
    const uint64_t nb = std::max(pl->count, 1u), ns = std::max<uint64_t>(slots, 1);
    bool ok = pl->d_vf_bufs.ensure(nb * sizeof(DvfBuf)) && pl->d_vf_owner.ensure(ns * 4u) &&
              pl->d_vf_facts.ensure(ns * sizeof(DvfBlock)) && pl->d_vf_verd.ensure(ns * sizeof(DvfVerdict)) &&
              pl->d_vf_nblk.ensure(nb * 4u) && pl->d_vf_res.ensure(nb * sizeof(DvfResult));
    ok = ok && hipMemcpy(pl->d_vf_bufs.p, pl->vf_bufs.data(), sizeof(DvfBuf) * pl->count, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(pl->d_vf_owner.p, owner.data(), 4ull * slots, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemset(pl->d_vf_nblk.p, 0, nb * 4u) == hipSuccess && hipEventCreate(&pl->vf_ev[0]) == hipSuccess &&
         hipEventCreate(&pl->vf_ev[1]) == hipSuccess;
    pl->vf_scratch = pl->d_vf_bufs.bytes + pl->d_vf_owner.bytes + pl->d_vf_facts.bytes + pl->d_vf_verd.bytes +
                     pl->d_vf_nblk.bytes + pl->d_vf_res.bytes;
    pl->scratch_bytes += pl->vf_scratch;
    if (!ok) {
        (void)hipGetLastError();
        verify_release(pl);
        return Z_MEM_ERROR;
    }
    pl->vf_slots = (uint32_t)slots;
    pl->vf_on = true;
    return Z_OK;
}

extern "C" ZlibReturn zsc_hip_deflate_plan_verify(zsc_hip_deflate_plan *pl, const void *d_input, const void *d_output,
                                                  void *hip_stream)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    if (!pl->vf_on || !pl->vf_valid || (pl->count != 0 && (d_input == Z_NULL || d_output == Z_NULL)))
        return Z_STREAM_ERROR;
    hipStream_t st = (hipStream_t)hip_stream;
    (void)hipGetLastError();
    if (pl->vf_ran && pl->vf_stream != st) /* the verdicts of the one before are still being written */
        HIP_TRY(hipStreamSynchronize(pl->vf_stream), return Z_STREAM_ERROR);
    pl->vf_stream = st;
    pl->vf_ran = true;
    (void)hipEventRecord(pl->vf_ev[0], st);
    if (pl->vf_slots)
        hipLaunchKernelGGL(k_verify_blocks, dim3(pl->vf_slots), dim3(64), 0, st, (const uint8_t *)d_input,
                           (const uint8_t *)d_output, (const DvfBuf *)pl->d_vf_bufs.p,
                           (const uint32_t *)pl->d_vf_owner.p, (const DvfBlock *)pl->d_vf_facts.p,
                           (const uint32_t *)pl->d_vf_nblk.p, (const ZdResult *)pl->d_res.p,
                           (DvfVerdict *)pl->d_vf_verd.p, (uint32_t)pl->wrap, (uint32_t)pl->wbits, pl->vf_slots);
    if (pl->count)
        hipLaunchKernelGGL(k_verify_finish, dim3((pl->count + 63) / 64), dim3(64), 0, st, (const uint8_t *)d_output,
                           (const DvfBuf *)pl->d_vf_bufs.p, (const DvfBlock *)pl->d_vf_facts.p,
                           (const DvfVerdict *)pl->d_vf_verd.p, (const uint32_t *)pl->d_vf_nblk.p,
                           (const ZdResult *)pl->d_res.p, (uint32_t)pl->wrap, (uint32_t)pl->wbits, (uint32_t)pl->level,
                           pl->strategy, (DvfResult *)pl->d_vf_res.p, pl->count);
    (void)hipEventRecord(pl->vf_ev[1], st);
    work_note(pl->vf_work, st);
    HIP_TRY(hipGetLastError(), return Z_STREAM_ERROR);
    return Z_OK;
}

extern "C" ZlibReturn zsc_hip_deflate_plan_verify_results(zsc_hip_deflate_plan *pl, zsc_hip_verify_result *results,
                                                          float *ms)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    if (ms)
        *ms = 0.f;
    if (!pl->vf_on || !pl->vf_valid || !pl->vf_ran)
        return Z_STREAM_ERROR;
    HIP_TRY(hipStreamSynchronize(pl->vf_stream), return Z_STREAM_ERROR);
    if (pl->count && results)
        HIP_TRY(hipMemcpy(results, pl->d_vf_res.p, sizeof(DvfResult) * pl->count, hipMemcpyDeviceToHost),
                return Z_STREAM_ERROR);
    if (ms)
        (void)hipEventElapsedTime(ms, pl->vf_ev[0], pl->vf_ev[1]);
    return Z_OK;
}

extern "C" ZlibReturn zsc_hip_deflate_plan_verify_blocks(zsc_hip_deflate_plan *pl, U32 buffer,
                                                         zsc_hip_verify_block *blocks, U32 cap, U32 *count)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    ZSC_ASSERT(count != Z_NULL);
    *count = 0;
    if (!pl->vf_on || !pl->vf_valid || buffer >= pl->count)
        return Z_STREAM_ERROR;
    if (pl->vf_run_res[buffer].status != Z_OK)
        return Z_DATA_ERROR;
    uint32_t n = 0;
    HIP_TRY(hipMemcpy(&n, (const uint32_t *)pl->d_vf_nblk.p + buffer, 4, hipMemcpyDeviceToHost), return Z_STREAM_ERROR);
    if (n > pl->vf_bufs[buffer].max_blocks)
        return Z_STREAM_ERROR;
    *count = n;
    if (cap < n || (n != 0 && blocks == Z_NULL))
        return Z_BUF_ERROR;
    if (n)
        HIP_TRY(hipMemcpy(blocks, (const DvfBlock *)pl->d_vf_facts.p + pl->vf_bufs[buffer].first, sizeof(DvfBlock) * n,
                          hipMemcpyDeviceToHost),
                return Z_STREAM_ERROR);
    return Z_OK;
}

/* ---- packing a deflate plan's streams (pack.h) ------------------------------------------------ */

static_assert(sizeof(ZdResult) == 16 && offsetof(ZdResult, out_len) == 0 && offsetof(ZdResult, status) == 4 &&
                  sizeof(InfResult) == 16 && offsetof(InfResult, status) == 0 && offsetof(InfResult, out_len) == 4,
              "the pack reads the lengths where the plans' results keep them");
static_assert(PK_TILE % (16u * 64u) == 0, "a tile is whole steps of a wavefront");

extern "C" ZlibReturn zsc_hip_deflate_plan_pack_enable(zsc_hip_deflate_plan *pl, U32 align)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    if (pl->sectioned || !pack_align_ok(align))
        return Z_STREAM_ERROR;
    if (pl->pack.on) {
        pack_set_align(pl->pack, align);
        return Z_OK;
    }
    std::vector<uint64_t> slots(pl->count);
    std::vector<U32> caps(pl->count);
    for (uint32_t i = 0; i < pl->count; i++) {
        slots[i] = pl->bufs[i].out_off;
        caps[i] = pl->bufs[i].out_cap;
    }
    return pack_setup(pl->pack, pl->count, align, slots.data(), caps.data(), &pl->scratch_bytes);
}

extern "C" ZlibReturn zsc_hip_deflate_plan_pack(zsc_hip_deflate_plan *pl, const void *d_output, void *d_packed,
                                                uint64_t packed_cap, void *hip_stream)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    /* a stream's length where its status is Z_OK, else 0 */
    const PkLens lens = {(const uint32_t *)pl->d_res.p, 4u, 0u, 1u};
    return pack_enqueue(pl->pack, lens, d_output, d_packed, packed_cap, (hipStream_t)hip_stream);
}

extern "C" ZlibReturn zsc_hip_deflate_plan_pack_results(zsc_hip_deflate_plan *pl, uint64_t *offsets, uint64_t *total,
                                                        float *ms)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    return pack_fetch(pl->pack, offsets, total, ms);
}

/* ---- BGZF files from a gzip deflate plan (bgzf.h) --------------------------------------------- */

extern "C" ZlibReturn zsc_hip_deflate_plan_bgzf_enable(zsc_hip_deflate_plan *pl, U32 nfiles, const U32 *file_first,
                                                       U32 align)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    ZSC_ASSERT(file_first != Z_NULL);
    if (pl->wrap != 2 || pl->sectioned || !pack_align_ok(align) || file_first[0] != 0u ||
        file_first[nfiles] != pl->count)
        return Z_STREAM_ERROR;
    for (U32 f = 0; f < nfiles; f++)
        if (file_first[f + 1u] < file_first[f])
            return Z_STREAM_ERROR;
    for (uint32_t i = 0; i < pl->count; i++)
        if (pl->bufs[i].in_len > BZ_MAX_MEMBER)
            return Z_STREAM_ERROR;
    /* the new partition beside the old one, which stays where anything fails */
    BgzfState nb;
    nb.count = pl->count;
    nb.nfiles = nfiles;
    nb.align = align;
    nb.file_first.assign(file_first, file_first + nfiles + 1u);
    const uint64_t nparts = (uint64_t)pl->count + nfiles;
    if (nparts > 0x7fffffffull)
        return Z_MEM_ERROR;
    std::vector<uint32_t> what((size_t)std::max<uint64_t>(nparts, 1));
    std::vector<uint64_t> slots(std::max<uint32_t>(pl->count, 1));
    for (U32 f = 0; f < nfiles; f++) {
        uint64_t most = BZ_TAIL;
        for (uint32_t i = file_first[f]; i < file_first[f + 1u]; i++) {
            what[(size_t)i + f] = i;
            most += std::min<uint64_t>((uint64_t)pl->bufs[i].out_cap + (BZ_HEAD - BZ_SKIP), BZ_MAX_MEMBER);
        }
        what[(size_t)file_first[f + 1u] + f] = BZ_PART_TAIL;
        nb.max_total += (most + (align - 1u)) & ~(uint64_t)(align - 1u);
    }
    for (uint32_t i = 0; i < pl->count; i++)
        slots[i] = pl->bufs[i].out_off;
    nb.levels = pk_scan_levels(nfiles, nb.level_n);
    uint64_t nsums = 0;
    for (uint32_t k = 1; k < nb.levels; k++) {
        nb.level_at[k] = nsums;
        nsums += nb.level_n[k] + 1u;
    }
    bool ok = nb.d_first.ensure(((uint64_t)nfiles + 1u) * 4u) && nb.d_file_off.ensure(((uint64_t)nfiles + 1u) * 8u) &&
              nb.d_parts.ensure((nparts + 1u) * 8u) && nb.d_what.ensure(what.size() * 4u) &&
              nb.d_slots.ensure(slots.size() * 8u) && nb.d_sums.ensure(std::max<uint64_t>(nsums, 1) * 8u);
    ok = ok && hipMemcpy(nb.d_first.p, file_first, ((size_t)nfiles + 1u) * 4u, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(nb.d_what.p, what.data(), what.size() * 4u, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(nb.d_slots.p, slots.data(), slots.size() * 8u, hipMemcpyHostToDevice) == hipSuccess &&
         hipEventCreate(&nb.ev[0]) == hipSuccess && hipEventCreate(&nb.ev[1]) == hipSuccess;
    nb.scratch = nb.d_first.bytes + nb.d_file_off.bytes + nb.d_parts.bytes + nb.d_what.bytes + nb.d_slots.bytes +
                 nb.d_sums.bytes;
    if (!ok) {
        (void)hipGetLastError();
        bgzf_release(nb, nullptr);
        return Z_MEM_ERROR;
    }
    if (pl->bgzf.on) { /* the partition of before goes, once what was enqueued with it has run */
        (void)work_wait(pl->bgzf.work);
        bgzf_release(pl->bgzf, &pl->scratch_bytes);
    }
    pl->bgzf = nb;
    pl->bgzf.on = true;
    pl->scratch_bytes += nb.scratch;
    return Z_OK;
}

extern "C" ZlibReturn zsc_hip_deflate_plan_bgzf(zsc_hip_deflate_plan *pl, const void *d_output, void *d_image,
                                                uint64_t image_cap, void *hip_stream)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    BgzfState &bs = pl->bgzf;
    hipStream_t st = (hipStream_t)hip_stream;
    if (!bs.on || ((uintptr_t)d_image & 15u) || ((uintptr_t)d_output & 15u))
        return Z_STREAM_ERROR;
    /* the grid comes from the capacity; what the image can be at the most bounds it */
    const uint64_t tiles = (std::min(image_cap, bs.max_total) + PK_TILE - 1u) / PK_TILE;
    if (tiles > 0x7fffffffull)
        return Z_MEM_ERROR;
    if (tiles && (d_image == Z_NULL || d_output == Z_NULL))
        return Z_STREAM_ERROR;
    (void)hipGetLastError();
    if (bs.ran && bs.stream != st) /* the tables of the one before may still be in use */
        HIP_TRY(hipStreamSynchronize(bs.stream), return Z_STREAM_ERROR);
    bs.stream = st;
    bs.ran = true;
    bs.cap = image_cap;
    (void)hipEventRecord(bs.ev[0], st);
    BzFiles F;
    F.rec = (const uint32_t *)pl->d_res.p;
    F.file_first = (const uint32_t *)bs.d_first.p;
    F.nfiles = bs.nfiles;
    F.count = bs.count;
    F.align = bs.align;
    uint64_t *const file_off = (uint64_t *)bs.d_file_off.p;
    if (bs.nfiles)
        hipLaunchKernelGGL(k_bgzf_file_len, dim3(bs.nfiles), dim3(64), 0, st, F, file_off);
    const PkLens none = {nullptr, 0u, 0u, PK_NO_STATUS};
    scan_enqueue(bs.levels, bs.level_n, bs.level_at, (uint64_t *)bs.d_sums.p, none, 1u, file_off, file_off, st);
    hipLaunchKernelGGL(k_bgzf_member_off, dim3(bs.nfiles + 1u), dim3(64), 0, st, F, (const uint64_t *)file_off,
                       (uint64_t *)bs.d_parts.p);
    if (tiles) {
        BzMove M;
        M.parts = (const uint64_t *)bs.d_parts.p;
        M.what = (const uint32_t *)bs.d_what.p;
        M.slot = (const uint64_t *)bs.d_slots.p;
        M.nparts = bs.count + bs.nfiles;
        M.cap = image_cap;
        hipLaunchKernelGGL(k_bgzf_move, dim3((uint32_t)tiles), dim3(64), 0, st, M, (uint8_t *)d_image,
                           (const uint8_t *)d_output);
    }
    (void)hipEventRecord(bs.ev[1], st);
    work_note(bs.work, st);
    HIP_TRY(hipGetLastError(), return Z_STREAM_ERROR);
    return Z_OK;
}

extern "C" ZlibReturn zsc_hip_deflate_plan_bgzf_results(zsc_hip_deflate_plan *pl, uint64_t *file_offsets,
                                                        uint64_t *file_lens, I32 *file_statuses,
                                                        uint64_t *member_offsets, uint64_t *total, float *ms)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    BgzfState &bs = pl->bgzf;
    if (ms)
        *ms = 0.f;
    if (total)
        *total = 0;
    if (!bs.on || !bs.ran)
        return Z_STREAM_ERROR;
    HIP_TRY(hipStreamSynchronize(bs.stream), return Z_STREAM_ERROR);
    const size_t nparts = (size_t)bs.count + bs.nfiles;
    std::vector<uint64_t> parts(nparts + 1u);
    HIP_TRY(hipMemcpy(parts.data(), bs.d_parts.p, parts.size() * 8u, hipMemcpyDeviceToHost), return Z_STREAM_ERROR);
    const uint64_t tot = parts[nparts];
    for (uint32_t f = 0; f < bs.nfiles; f++) {
        const uint32_t first = bs.file_first[f], end = bs.file_first[f + 1u];
        /* a sound file has its tail; a failed one has nothing */
        const uint64_t at = parts[(size_t)first + f], tail = parts[(size_t)end + f];
        const bool sound = parts[(size_t)end + f + 1u] > tail;
        if (file_offsets)
            file_offsets[f] = at;
        if (file_lens)
            file_lens[f] = sound ? tail + BZ_TAIL - at : 0u;
        if (file_statuses)
            file_statuses[f] = sound ? Z_OK : Z_BUF_ERROR;
        if (member_offsets)
            for (uint32_t i = first; i < end; i++)
                member_offsets[i] = parts[(size_t)i + f];
    }
    if (file_offsets)
        file_offsets[bs.nfiles] = tot;
    if (total)
        *total = tot;
    if (ms)
        (void)hipEventElapsedTime(ms, bs.ev[0], bs.ev[1]);
    return tot > bs.cap ? Z_BUF_ERROR : Z_OK;
}

/* ---- ZIP archives from a gzip deflate plan (zip.h) ---------------------------------------------- */

extern "C" ZlibReturn zsc_hip_deflate_plan_zip_enable(zsc_hip_deflate_plan *pl, U32 narchives, const U32 *arch_first,
                                                      const U8 *names, const uint64_t *name_offsets,
                                                      const U32 *dos_datetime, U32 flags, U32 align)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    ZSC_ASSERT(arch_first != Z_NULL);
    ZSC_ASSERT(name_offsets != Z_NULL);
    if (pl->wrap != 2 || pl->sectioned || !pack_align_ok(align) || (flags & ~ZSC_HIP_ZIP_UTF8))
        return Z_STREAM_ERROR;
    const uint32_t count = pl->count;
    std::vector<uint32_t> caps(std::max<uint32_t>(count, 1));
    std::vector<uint64_t> slots(std::max<uint32_t>(count, 1));
    for (uint32_t i = 0; i < count; i++) {
        caps[i] = pl->bufs[i].out_cap;
        slots[i] = pl->bufs[i].out_off;
    }
    ZpLayout Z;
    if (name_offsets[0] > name_offsets[count] || !zp_layout(count, narchives, arch_first, name_offsets, caps.data(), align, Z))
        return Z_STREAM_ERROR;
    const uint64_t names_at = name_offsets[0], names_len = name_offsets[count] - names_at;
    ZSC_ASSERT(names_len == 0 || names != Z_NULL);
    /* the new partition beside the old one, which stays where anything fails */
    ZipState nz;
    nz.count = count;
    nz.narchives = narchives;
    nz.align = align;
    nz.flags = (flags & ZSC_HIP_ZIP_UTF8) ? 0x0800u : 0u;
    nz.has_datetime = dos_datetime != Z_NULL;
    nz.arch_first.assign(arch_first, arch_first + narchives + 1u);
    nz.name_off.resize((size_t)count + 1u);
    for (uint32_t i = 0; i <= count; i++) /* (the device's names start at 0) */
        nz.name_off[i] = name_offsets[i] - names_at;
    nz.nparts = Z.nparts;
    nz.max_total = Z.max_total;
    nz.levels = pk_scan_levels(narchives, nz.level_n);
    uint64_t nsums = 0;
    for (uint32_t k = 1; k < nz.levels; k++) {
        nz.level_at[k] = nsums;
        nsums += nz.level_n[k] + 1u;
    }
    auto up = [](DevBuf &b, const void *src, uint64_t bytes) {
        return b.ensure(bytes) && (bytes == 0 || hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice) == hipSuccess);
    };
    bool ok = up(nz.d_first, arch_first, ((uint64_t)narchives + 1u) * 4u) && up(nz.d_fixed, Z.fixed.data(), Z.fixed.size() * 8u) &&
              up(nz.d_kinds, Z.kinds.data(), Z.kinds.size() * 4u) && up(nz.d_arch_of, Z.arch_of.data(), Z.arch_of.size() * 4u) &&
              up(nz.d_slots, slots.data(), slots.size() * 8u) && up(nz.d_name_off, nz.name_off.data(), nz.name_off.size() * 8u) &&
              up(nz.d_names, names_len ? names + names_at : Z_NULL, names_len) &&
              (!nz.has_datetime || up(nz.d_datetime, dos_datetime, (uint64_t)count * 4u)) &&
              nz.d_arch_off.ensure(((uint64_t)narchives + 1u) * 8u) && nz.d_arch_st.ensure(std::max<uint64_t>(narchives, 1) * 4u) &&
              nz.d_parts.ensure((Z.nparts + 1u) * 8u) && nz.d_sums.ensure(std::max<uint64_t>(nsums, 1) * 8u);
    ok = ok && hipEventCreate(&nz.ev[0]) == hipSuccess && hipEventCreate(&nz.ev[1]) == hipSuccess;
    for (const DevBuf *b : {&nz.d_first, &nz.d_fixed, &nz.d_arch_off, &nz.d_arch_st, &nz.d_parts, &nz.d_kinds, &nz.d_arch_of,
                            &nz.d_slots, &nz.d_name_off, &nz.d_names, &nz.d_datetime, &nz.d_sums})
        nz.scratch += b->bytes;
    if (!ok) {
        (void)hipGetLastError();
        zip_release(nz, nullptr);
        return Z_MEM_ERROR;
    }
    if (pl->zip.on) { /* what was there before goes, once what was enqueued with it has run */
        (void)work_wait(pl->zip.work);
        zip_release(pl->zip, &pl->scratch_bytes);
    }
    pl->zip = nz;
    pl->zip.on = true;
    pl->scratch_bytes += nz.scratch;
    return Z_OK;
}

extern "C" ZlibReturn zsc_hip_deflate_plan_zip(zsc_hip_deflate_plan *pl, const void *d_output, void *d_image,
                                               uint64_t image_cap, void *hip_stream)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    ZipState &zs = pl->zip;
    hipStream_t st = (hipStream_t)hip_stream;
    if (!zs.on || ((uintptr_t)d_image & 15u) || ((uintptr_t)d_output & 15u))
        return Z_STREAM_ERROR;
    /* the grid comes from the capacity; what the image can be at the most bounds it */
    const uint64_t tiles = (std::min(image_cap, zs.max_total) + PK_TILE - 1u) / PK_TILE;
    if (tiles > 0x7fffffffull)
        return Z_MEM_ERROR;
    if (tiles && (d_image == Z_NULL || (zs.count && d_output == Z_NULL)))
        return Z_STREAM_ERROR;
    (void)hipGetLastError();
    if (zs.ran && zs.stream != st) /* the tables of the one before may still be in use */
        HIP_TRY(hipStreamSynchronize(zs.stream), return Z_STREAM_ERROR);
    zs.stream = st;
    zs.ran = true;
    zs.cap = image_cap;
    (void)hipEventRecord(zs.ev[0], st);
    ZpArchives A;
    A.rec = (const uint32_t *)pl->d_res.p;
    A.arch_first = (const uint32_t *)zs.d_first.p;
    A.name_off = (const uint64_t *)zs.d_name_off.p;
    A.fixed = (const uint64_t *)zs.d_fixed.p;
    A.narchives = zs.narchives;
    A.count = zs.count;
    A.align = zs.align;
    uint64_t *const arch_off = (uint64_t *)zs.d_arch_off.p;
    if (zs.narchives)
        hipLaunchKernelGGL(k_zip_arch_len, dim3(zs.narchives), dim3(64), 0, st, A, arch_off, (uint32_t *)zs.d_arch_st.p);
    const PkLens none = {nullptr, 0u, 0u, PK_NO_STATUS};
    scan_enqueue(zs.levels, zs.level_n, zs.level_at, (uint64_t *)zs.d_sums.p, none, 1u, arch_off, arch_off, st);
    hipLaunchKernelGGL(k_zip_part_off, dim3(zs.narchives + 1u), dim3(64), 0, st, A, (const uint64_t *)arch_off,
                       (uint64_t *)zs.d_parts.p);
    if (tiles) {
        ZpMove M;
        M.parts = (const uint64_t *)zs.d_parts.p;
        M.kinds = (const uint32_t *)zs.d_kinds.p;
        M.slot = (const uint64_t *)zs.d_slots.p;
        M.name_off = (const uint64_t *)zs.d_name_off.p;
        M.arch_first = (const uint32_t *)zs.d_first.p;
        M.arch_of = (const uint32_t *)zs.d_arch_of.p;
        M.datetime = zs.has_datetime ? (const uint32_t *)zs.d_datetime.p : nullptr;
        M.nparts = (uint32_t)zs.nparts;
        M.flags = zs.flags;
        M.cap = image_cap;
        M.names_len = zs.name_off[zs.count];
        hipLaunchKernelGGL(k_zip_move, dim3((uint32_t)tiles), dim3(64), 0, st, M, (uint8_t *)d_image,
                           (const uint8_t *)d_output, (const uint8_t *)zs.d_names.p);
    }
    (void)hipEventRecord(zs.ev[1], st);
    work_note(zs.work, st);
    HIP_TRY(hipGetLastError(), return Z_STREAM_ERROR);
    return Z_OK;
}

extern "C" ZlibReturn zsc_hip_deflate_plan_zip_results(zsc_hip_deflate_plan *pl, uint64_t *arch_offsets,
                                                       uint64_t *arch_lens, I32 *arch_statuses, uint64_t *entry_offsets,
                                                       uint64_t *data_offsets, uint64_t *dir_offsets, uint64_t *total,
                                                       float *ms)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    ZipState &zs = pl->zip;
    if (ms)
        *ms = 0.f;
    if (total)
        *total = 0;
    if (!zs.on || !zs.ran)
        return Z_STREAM_ERROR;
    HIP_TRY(hipStreamSynchronize(zs.stream), return Z_STREAM_ERROR);
    std::vector<uint64_t> parts((size_t)zs.nparts + 1u);
    std::vector<uint32_t> states(std::max<uint32_t>(zs.narchives, 1));
    HIP_TRY(hipMemcpy(parts.data(), zs.d_parts.p, parts.size() * 8u, hipMemcpyDeviceToHost), return Z_STREAM_ERROR);
    if (zs.narchives)
        HIP_TRY(hipMemcpy(states.data(), zs.d_arch_st.p, (size_t)zs.narchives * 4u, hipMemcpyDeviceToHost),
                return Z_STREAM_ERROR);
    const uint64_t tot = parts[(size_t)zs.nparts];
    for (uint32_t a = 0; a < zs.narchives; a++) {
        const uint32_t first = zs.arch_first[a], end = zs.arch_first[a + 1u];
        const uint64_t at = parts[2u * (size_t)first + a], end_at = parts[2u * (size_t)end + a];
        const bool sound = states[a] == ZP_ST_OK;
        if (arch_offsets)
            arch_offsets[a] = at;
        if (arch_lens)
            arch_lens[a] = sound ? end_at + zp_end_len(end - first) - at : 0u;
        if (arch_statuses)
            arch_statuses[a] = sound ? Z_OK : states[a] == ZP_ST_MEM ? Z_MEM_ERROR : Z_BUF_ERROR;
        if (dir_offsets)
            dir_offsets[a] = parts[(size_t)a + end + first]; /* (an empty directory lies where the end does) */
        for (uint32_t i = first; i < end; i++) {
            const uint64_t e = parts[(size_t)first + a + i];
            if (entry_offsets)
                entry_offsets[i] = e;
            if (data_offsets)
                data_offsets[i] = sound ? e + ZP_LOCAL + (zs.name_off[i + 1u] - zs.name_off[i]) : e;
        }
    }
    if (arch_offsets)
        arch_offsets[zs.narchives] = tot;
    if (total)
        *total = tot;
    if (ms)
        (void)hipEventElapsedTime(ms, zs.ev[0], zs.ev[1]);
    return tot > zs.cap ? Z_BUF_ERROR : Z_OK;
}

/* ---- level 0 --------------------------------------------------------------------- */

namespace {

/* Where the pieces of a level-0 stream go.  deflate_stored (reference src/deflate.c:1679-1880)
 * sizes its stored blocks by the output space of the moment, and zsc_compress hands that
 * space out in slices of max_block_len next to input sections of max_block_len
 * (src/zsc_compress.c:121-138), so the layout is found by following those calls -- pure
 * arithmetic on lengths, the bytes themselves never matter.  One StoreSim per buffer. */
struct StoreSim {
    uint32_t w_size = 0, pending_buf_size = 0, max_block_len = 0, source_len = 0;
    int wrap = 1;
    std::vector<ZdStorePiece> *pieces = nullptr;
    uint64_t in_base = 0, out_base = 0;
    uint32_t buf = 0, hdr_arg = 0;
    uint32_t hdr_len = 0; /* a caller-supplied gzip member header of this length (0: the plain one) */
    /* the stream */
    uint32_t produced = 0, delivered = 0, avail_out = 0;
    uint32_t given = 0, st_read = 0, st_emit = 0, st_strstart = 0, st_block_start = 0;
    bool header_done = false, finishing = false, trailer_done = false;

    void piece(uint32_t kind, uint32_t len, uint32_t arg, uint32_t bytes)
    {
        ZdStorePiece pc;
        pc.src_off = in_base + st_emit;
        pc.dst_off = out_base + produced;
        pc.len = len;
        pc.kind = kind;
        pc.arg = arg;
        pc.buf = buf;
        pieces->push_back(pc);
        produced += bytes;
    }
    void stored_block(uint32_t len, int last)
    {
        piece(0, len, (uint32_t)last, 5u + len);
        st_emit += len;
    }
    void flush_pending()
    {
        const uint32_t have = produced - delivered, len = have < avail_out ? have : avail_out;
        delivered += len;
        avail_out -= len;
    }
    /* 0 need_more, 1 block_done, 2 finish_started, 3 finish_done */
    int deflate_stored(bool finish)
    {
        const uint32_t window_size = 2u * w_size;
        uint32_t min_block = std::min(pending_buf_size - 5u, w_size);
        uint32_t avail_in = given - st_read;
        const uint32_t used0 = avail_in;
        uint32_t len, left, have;
        int last = 0;
        do {
            len = 65535u;
            have = 5u;
            if (avail_out < have)
                break;
            have = avail_out - have;
            left = st_strstart - st_block_start;
            len = std::min(len, left + avail_in);
            len = std::min(len, have);
            if (len < min_block && ((len == 0 && !finish) || len != left + avail_in))
                break;
            last = finish && len == left + avail_in;
            const uint32_t from_window = std::min(left, len);
            stored_block(len, last);
            st_block_start += from_window;
            st_read += len - from_window;
            avail_in -= len - from_window;
            delivered += 5u + len; /* header through pending, bytes straight to next_out */
            avail_out -= 5u + len;
        } while (!last);
        const uint32_t used = used0 - avail_in;
        if (used) {
            if (used >= w_size) {
                st_strstart = w_size;
            } else {
                if (window_size - st_strstart <= used)
                    st_strstart -= w_size;
                st_strstart += used;
            }
            st_block_start = st_strstart;
        }
        if (last)
            return 3;
        if (!finish && avail_in == 0 && st_strstart == st_block_start)
            return 1;
        have = window_size - st_strstart - 1u;
        if (avail_in > have && st_block_start >= w_size) {
            st_block_start -= w_size;
            st_strstart -= w_size;
            have += w_size;
        }
        have = std::min(have, avail_in);
        if (have) {
            st_read += have;
            avail_in -= have;
            st_strstart += have;
        }
        have = std::min(pending_buf_size - 5u, 65535u);
        min_block = std::min(have, w_size);
        left = st_strstart - st_block_start;
        if (left >= min_block || ((left || finish) && avail_in == 0 && left <= have)) {
            len = std::min(left, have);
            last = finish && avail_in == 0 && len == left;
            stored_block(len, last);
            st_block_start += len;
            flush_pending();
        }
        return last ? 2 : 0;
    }
    /* one deflate() call: Z_OK, 1 = Z_STREAM_END, Z_BUF_ERROR (src/deflate.c:964-1295) */
    int deflate(bool finish)
    {
        if (avail_out == 0)
            return Z_BUF_ERROR;
        if (produced != delivered) {
            flush_pending();
            if (avail_out == 0)
                return Z_OK;
        }
        if (!header_done) {
            header_done = true;
            if (wrap) {
                if (hdr_len)
                    piece(4, 0, 0, hdr_len); /* room only: zsc_api.c writes the caller's header */
                else
                    piece(2, 0, hdr_arg, wrap == 1 ? 2u : 10u);
                flush_pending();
                if (produced != delivered)
                    return Z_OK;
            }
        }
        if (!finishing) {
            const int bs = deflate_stored(finish);
            if (bs == 2 || bs == 3)
                finishing = true;
            if (bs == 0 || bs == 2)
                return Z_OK;
            if (bs == 1) {
                piece(1, 0, 0, 5u);
                st_strstart = st_block_start = 0;
                flush_pending();
                return Z_OK;
            }
        }
        if (!finish)
            return Z_OK;
        if (wrap == 0)
            return 1;
        if (!trailer_done) {
            trailer_done = true;
            piece(3, 0, 0, wrap == 1 ? 4u : 8u);
            flush_pending();
            return produced != delivered ? Z_OK : 1;
        }
        return 1;
    }
    /* the wrapper's loop, src/zsc_compress.c:121-138; returns the call's ZlibReturn */
    int run(uint32_t dest_cap)
    {
        uint32_t left_dest = dest_cap, left_src = source_len;
        int err = Z_OK;
        while (err == Z_OK) {
            if (avail_out == 0) {
                avail_out = std::min(left_dest, max_block_len);
                left_dest -= avail_out;
            }
            if (st_read == given) {
                const uint32_t take = std::min(left_src, max_block_len);
                given += take;
                left_src -= take;
            }
            err = deflate(left_src == 0);
        }
        return err == 1 ? Z_OK : err;
    }
};

} // namespace

extern "C" ZlibReturn zsc_hip_store_batch(U32 count, const U8 *const *sources, const U32 *source_lens,
                                          const U32 *max_block_lens, U8 *const *dests,
                                          U32 *dest_lens, I32 *statuses, I32 window_bits,
                                          I32 mem_level, U32 gzip_header_len)
{
    DeviceScope scope;
    ZSC_ASSERT(sources != Z_NULL);
    ZSC_ASSERT(source_lens != Z_NULL);
    ZSC_ASSERT(max_block_lens != Z_NULL);
    ZSC_ASSERT(dests != Z_NULL);
    ZSC_ASSERT(dest_lens != Z_NULL);
    if (count == 0)
        return Z_OK;
    if (zsc_hip_init(-1) != Z_OK)
        return Z_STREAM_ERROR;
    int wrap = 1, wbits = 15, level = 1;
    if (!dpl_fold_params(&level, window_bits, mem_level, Z_DEFAULT_STRATEGY, &wrap, &wbits))
        return Z_STREAM_ERROR;
    /* zlib header of level 0: level_flags 0 (src/deflate.c:1031-1049); gzip XFL 4 (:1075-1078) */
    uint32_t zh = (8u + (((uint32_t)wbits - 8u) << 4)) << 8;
    zh += 31u - zh % 31u;
    std::vector<ZdStorePiece> pieces;
    std::vector<ZdBuf> bufs(count);
    std::vector<uint32_t> give(count), stat(count);
    uint64_t in_bytes = 0, out_bytes = 0;
    for (U32 i = 0; i < count; i++) {
        ZSC_ASSERT(max_block_lens[i] != 0);
        StoreSim sim;
        sim.w_size = 1u << wbits;
        sim.pending_buf_size = (1u << (mem_level + 6)) * 4u; /* lit_bufsize * 4, src/deflate.c:362 */
        sim.max_block_len = max_block_lens[i];
        sim.source_len = source_lens[i];
        sim.wrap = wrap;
        sim.pieces = &pieces;
        sim.in_base = in_bytes;
        sim.out_base = out_bytes;
        sim.buf = i;
        sim.hdr_arg = wrap == 1 ? zh : 4u;
        sim.hdr_len = wrap == 2 ? gzip_header_len : 0u;
        stat[i] = (uint32_t)sim.run(dest_lens[i]);
        give[i] = sim.delivered;
        memset(&bufs[i], 0, sizeof(ZdBuf));
        bufs[i].in_off = in_bytes;
        bufs[i].out_off = out_bytes;
        bufs[i].in_len = source_lens[i];
        bufs[i].wrap = (uint32_t)wrap;
        in_bytes += ((uint64_t)source_lens[i] + 15u) & ~15ull;
        out_bytes += ((uint64_t)sim.produced + 15u) & ~15ull;
    }
    DevBuf d_in, d_out, d_pieces, d_bufs, d_res;
    ZlibReturn rc = Z_OK;
    if (!d_in.ensure(in_bytes + 64) || !d_out.ensure(out_bytes + 64) ||
        !d_pieces.ensure(sizeof(ZdStorePiece) * std::max<size_t>(1, pieces.size())) ||
        !d_bufs.ensure(sizeof(ZdBuf) * count) || !d_res.ensure(sizeof(ZdResult) * count))
        rc = Z_MEM_ERROR;
    for (U32 i = 0; i < count && rc == Z_OK; i++) {
        ZSC_ASSERT(sources[i] != Z_NULL);
        if (source_lens[i] && hipMemcpy((uint8_t *)d_in.p + bufs[i].in_off, sources[i], source_lens[i],
                                        hipMemcpyHostToDevice) != hipSuccess)
            rc = Z_STREAM_ERROR;
    }
    if (rc == Z_OK &&
        (hipMemcpy(d_bufs.p, bufs.data(), sizeof(ZdBuf) * count, hipMemcpyHostToDevice) != hipSuccess ||
         (!pieces.empty() && hipMemcpy(d_pieces.p, pieces.data(), sizeof(ZdStorePiece) * pieces.size(),
                                       hipMemcpyHostToDevice) != hipSuccess)))
        rc = Z_STREAM_ERROR;
    if (rc == Z_OK) {
        hipLaunchKernelGGL(k_checksum, dim3(count), dim3(64), 0, nullptr, (const uint8_t *)d_in.p,
                           (const ZdBuf *)d_bufs.p, (ZdResult *)d_res.p, count);
        if (!pieces.empty())
            hipLaunchKernelGGL(k_store, dim3((uint32_t)pieces.size()), dim3(256), 0, nullptr,
                               (const uint8_t *)d_in.p, (uint8_t *)d_out.p,
                               (const ZdStorePiece *)d_pieces.p, (const ZdBuf *)d_bufs.p,
                               (const ZdResult *)d_res.p, (uint32_t)pieces.size());
        if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess)
            rc = Z_STREAM_ERROR;
    }
    for (U32 i = 0; i < count && rc == Z_OK; i++) {
        ZSC_ASSERT(dests[i] != Z_NULL);
        if (give[i] && hipMemcpy(dests[i], (uint8_t *)d_out.p + bufs[i].out_off, give[i],
                                 hipMemcpyDeviceToHost) != hipSuccess)
            rc = Z_STREAM_ERROR;
        dest_lens[i] = give[i];
        if (statuses)
            statuses[i] = (I32)stat[i];
    }
    d_in.release();
    d_out.release();
    d_pieces.release();
    d_bufs.release();
    d_res.release();
    return rc;
}

/* ---- levels 1-9 with source_len > max_block_len (sections.h) ----------------------- */

namespace {

/* runs the kernels for the runs sections.h wants parsed (one plan per round) and keeps every
 * round's compressed bytes until the streams are put together */
/* the last sections call of this process: sub-batches parsed in the wide and in the narrow LDS geometry */
static std::atomic<uint32_t> g_sections_last_rings[2];

struct HipSecRunner {
    const uint8_t *d_src = nullptr; /* the streams' input, stream i at src_off[i] */
    const uint64_t *src_off = nullptr;
    I32 level = 6, mem_level = 8;
    int wbits = 15;
    ZlibStrategy strategy = Z_DEFAULT_STRATEGY;
    struct Round {
        DevBuf d_in, d_out;
        std::vector<uint64_t> out_off;
    };
    std::vector<Round *> rounds;
    uint32_t parses = 0;
    uint32_t subs_wide = 0, subs_narrow = 0; /* the rounds' sub-batches by the LDS geometry of their segmented parser */
    ZlibReturn error = Z_OK;
    const std::vector<SecStream> *streams = nullptr; /* whose runs say which rounds' bytes are still in use */
    uint64_t parsed_bytes = 0, budget_bytes = ~0ull;  /* work budget: input bytes parsed over all rounds */
    uint64_t held_bytes = 0, held_peak = 0;           /* compressed bytes of the rounds kept */

    /* Bytes of a round are in use while a run that was parsed in it is still part of its stream (not
     * about to be parsed again: `jobs`, and not swallowed by the run before it) or a finished stream
     * is made of them.  Everything else is given back before the next round allocates: without this
     * a stream that needs many rounds (short sections, tiny blocks, incompressible data: every
     * section end a joint) held rounds x run bytes, hundreds of GB for a few MiB of input. */
    void release_dead_rounds(const std::vector<SecRun *> &jobs)
    {
        if (!streams)
            return;
        std::vector<uint8_t> live(rounds.size(), 0);
        for (const SecStream &st : *streams) {
            if (st.done) {
                for (const SecPiece &pc : st.pieces)
                    if ((pc.kind == SEC_PIECE_RUN || pc.kind == SEC_PIECE_TAIL) && pc.round < live.size())
                        live[pc.round] = 1;
                continue;
            }
            for (const auto &kv : st.runs) {
                const SecRun &r = kv.second;
                if (r.blocks.empty() || std::find(jobs.begin(), jobs.end(), &r) != jobs.end())
                    continue; /* never parsed yet, or about to be parsed again */
                if (r.round < live.size())
                    live[r.round] = 1;
            }
        }
        for (size_t k = 0; k < rounds.size(); k++) {
            if (rounds[k] && !live[k] && rounds[k]->d_out.p) {
                held_bytes -= rounds[k]->d_out.bytes;
                rounds[k]->d_out.release();
            }
        }
    }

    ~HipSecRunner()
    {
        for (Round *r : rounds) {
            r->d_in.release();
            r->d_out.release();
            delete r;
        }
    }

    int operator()(std::vector<SecRun *> &jobs, uint32_t round)
    {
        const auto t_begin = std::chrono::steady_clock::now();
        const U32 count = (U32)jobs.size();
        release_dead_rounds(jobs);
        for (const SecRun *r : jobs)
            parsed_bytes += r->n;
        if (parsed_bytes > budget_bytes) {
            ZSC_WARN3("zsc_hip: compressing these streams of sections needs more than %llu MB of parsing for "
                      "%u runs in round %u (sections so short, or blocks so small, that nearly every section end "
                      "lets the next section in): refused.",
                      (unsigned long long)(budget_bytes >> 20), count, round);
            return error = Z_STREAM_ERROR;
        }
        std::vector<U32> lens(count), caps(count), more(count), n0(count), soff(count), scnt(count), segok(count);
        std::vector<uint64_t> in_off(count), out_off(count);
        std::vector<ZdSched> sched;
        for (U32 j = 0; j < count; j++) {
            const SecRun &r = *jobs[j];
            lens[j] = r.n;
            more[j] = r.more ? 1u : 0u;
            n0[j] = r.n0;
            soff[j] = (U32)sched.size();
            scnt[j] = (U32)r.sched.size();
            segok[j] = sec_seg_ok(r) ? 1u : 0u;
            sched.insert(sched.end(), r.sched.begin(), r.sched.end());
        }
        uint64_t in_bytes = 0, out_bytes = 0;
        ZlibReturn rc = zsc_hip_deflate_plan_layout(count, lens.data(), level, -wbits, mem_level,
                                                    in_off.data(), out_off.data(), caps.data(),
                                                    &in_bytes, &out_bytes);
        if (rc != Z_OK)
            return error = rc;
        /* every joint can cut a block, a cut costs a few bytes; room for the marker's bits */
        out_bytes = 0;
        for (U32 j = 0; j < count; j++) {
            caps[j] += 16u * (scnt[j] + 1u) + 64u;
            out_off[j] = out_bytes;
            out_bytes += ((uint64_t)caps[j] + 16u + 15u) & ~15ull;
        }
        out_bytes += 64;
        Round *rd = new Round();
        rounds.resize(round + 1, nullptr);
        rounds[round] = rd;
        rd->out_off = out_off;
        if (!rd->d_out.ensure(out_bytes))
            return error = Z_MEM_ERROR;
        held_bytes += rd->d_out.bytes;
        held_peak = std::max(held_peak, held_bytes);

        /* the scratch arrays of a plan are ~16 bytes per input byte: groups of jobs, one plan each,
         * all writing into the round's output */
        uint64_t group_limit = 2048ull << 20;
        if (const char *e = getenv("ZSC_HIP_SECTIONS_GROUP_MB"))
            group_limit = std::max<uint64_t>(1, (uint64_t)atoll(e)) << 20;
        for (U32 g0 = 0; g0 < count && rc == Z_OK;) {
            U32 g1 = g0;
            uint64_t bytes = 0;
            while (g1 < count && (g1 == g0 || bytes + lens[g1] <= group_limit))
                bytes += lens[g1++];
            rc = run_group(jobs, round, g0, g1, lens, caps, more, n0, soff, scnt, segok, sched, out_off, rd);
            g0 = g1;
        }
        parses += count;
        if (getenv("ZSC_HIP_SECTIONS_LOG")) {
            uint64_t bytes = 0, joints = 0;
            for (U32 j = 0; j < count; j++)
                bytes += lens[j], joints += scnt[j];
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
            fprintf(stderr, "zsc_hip sections: round %u: %u runs, %llu bytes, %llu joints, %.2f ms\n", round, count,
                    (unsigned long long)bytes, (unsigned long long)joints, ms);
        }
        return error = rc;
    }

    /* jobs [g0, g1) of a round: gather their input, run the kernels, read the block records back */
    ZlibReturn run_group(std::vector<SecRun *> &jobs, uint32_t round, U32 g0, U32 g1,
                         const std::vector<U32> &lens, const std::vector<U32> &caps,
                         const std::vector<U32> &more, const std::vector<U32> &n0,
                         const std::vector<U32> &soff, const std::vector<U32> &scnt,
                         const std::vector<U32> &segok, const std::vector<ZdSched> &sched,
                         const std::vector<uint64_t> &out_off, Round *rd)
    {
        const U32 count = g1 - g0;
        std::vector<uint64_t> in_off(count);
        uint64_t in_bytes = 0;
        for (U32 j = 0; j < count; j++) {
            in_off[j] = in_bytes;
            in_bytes += ((uint64_t)lens[g0 + j] + 15u) & ~15ull;
        }
        in_bytes += 64;
        PlanRuns pr = {more.data() + g0, n0.data() + g0, soff.data() + g0, scnt.data() + g0, segok.data() + g0,
                       sched.data(), (uint32_t)sched.size()};
        zsc_hip_deflate_plan *pl = nullptr;
        ZlibReturn rc = plan_create(&pl, count, lens.data() + g0, in_off.data(), out_off.data() + g0,
                                    caps.data() + g0, level, -wbits, mem_level, strategy, &pr);
        if (rc != Z_OK)
            return rc;
        {
            uint32_t wide, narrow;
            zsc_plan_seg_rings(pl, &wide, &narrow);
            subs_wide += wide;
            subs_narrow += narrow;
        }
        DevBuf d_pieces;
        std::vector<ZdStorePiece> gather(count);
        for (U32 j = 0; j < count; j++) {
            ZdStorePiece &pc = gather[j];
            memset(&pc, 0, sizeof pc);
            pc.src_off = src_off[jobs[g0 + j]->stream] + jobs[g0 + j]->start;
            pc.dst_off = in_off[j];
            pc.len = lens[g0 + j];
            pc.kind = 6u;
        }
        if (!rd->d_in.ensure(in_bytes) || !d_pieces.ensure(sizeof(ZdStorePiece) * count))
            rc = Z_MEM_ERROR;
        if (rc == Z_OK && hipMemcpy(d_pieces.p, gather.data(), sizeof(ZdStorePiece) * count,
                                    hipMemcpyHostToDevice) != hipSuccess)
            rc = Z_STREAM_ERROR;
        if (rc == Z_OK) {
            hipLaunchKernelGGL(k_store, dim3(count), dim3(256), 0, nullptr, d_src, (uint8_t *)rd->d_in.p,
                               (const ZdStorePiece *)d_pieces.p, (const ZdBuf *)nullptr,
                               (const ZdResult *)nullptr, count);
            rc = zsc_hip_deflate_plan_run(pl, rd->d_in.p, rd->d_out.p, nullptr);
        }
        std::vector<U32> out_lens(count);
        std::vector<I32> stat(count);
        if (rc == Z_OK)
            rc = zsc_hip_deflate_plan_results(pl, out_lens.data(), stat.data());
        /* what the simulation needs of every block: where it ends, in input and in bits */
        const SubBatch &sb = pl->subs[0];
        std::vector<ZdBlockRec> recs(sb.nslots);
        std::vector<uint32_t> bit_off(sb.nslots);
        std::vector<ZdParseOut> pout(count);
        std::vector<ZdResult> res(count);
        DevBuf d_bits;
        if (rc == Z_OK && !d_bits.ensure(4ull * std::max(1u, sb.nslots)))
            rc = Z_MEM_ERROR;
        if (rc == Z_OK && sb.nslots)
            hipLaunchKernelGGL(k_bit_offs, dim3((sb.nslots + 255) / 256), dim3(256), 0, nullptr,
                               (const ZdBlockPlan *)pl->d_plans.p, (uint32_t *)d_bits.p, sb.nslots);
        if (rc == Z_OK &&
            (hipMemcpy(recs.data(), pl->d_recs.p, sizeof(ZdBlockRec) * sb.nslots, hipMemcpyDeviceToHost) != hipSuccess ||
             hipMemcpy(bit_off.data(), d_bits.p, 4ull * sb.nslots, hipMemcpyDeviceToHost) != hipSuccess ||
             hipMemcpy(pout.data(), pl->d_pout.p, sizeof(ZdParseOut) * count, hipMemcpyDeviceToHost) != hipSuccess ||
             hipMemcpy(res.data(), pl->d_res.p, sizeof(ZdResult) * count, hipMemcpyDeviceToHost) != hipSuccess))
            rc = Z_STREAM_ERROR;
        for (U32 j = 0; j < count && rc == Z_OK; j++) {
            SecRun &r = *jobs[g0 + j];
            const ZdBuf &b = pl->bufs[j];
            if (stat[j] != Z_OK || pout[j].nblocks > b.max_blocks) {
                ZSC_WARN2("zsc_hip: a run of sections came back with status %d (%u blocks).",
                          (int)stat[j], pout[j].nblocks);
                rc = Z_STREAM_ERROR;
                break;
            }
            r.blocks.clear();
            for (uint32_t k = 0; k < pout[j].nblocks; k++) {
                const ZdBlockRec &rec = recs[b.blk0 + k];
                SecBlock blk;
                blk.upto = rec.in_begin + rec.in_len;
                blk.end_bit = k + 1 < pout[j].nblocks ? bit_off[b.blk0 + k + 1] : res[j].bits;
                blk.wend = rec.wend;
                blk.at = rec.at;
                blk.cut = rec.cut;
                blk.last = rec.last;
                r.blocks.push_back(blk);
            }
            r.round = round;
            r.job = g0 + j;
        }
        d_pieces.release();
        d_bits.release();
        rd->d_in.release(); /* only the compressed bytes are needed later */
        zsc_hip_deflate_plan_destroy(pl);
        return rc;
    }
};

} // namespace

/* the streams are in device memory, stream i at d_src + src_off[i] (16-byte aligned); the finished
 * streams go to d_dst + dst_off[i], of which dest_caps[i] bytes may be used */
static ZlibReturn sections_on_device(U32 count, const uint8_t *d_src, const uint64_t *src_off,
                                     const U32 *source_lens, const U32 *max_block_lens,
                                     uint8_t *d_dst, const uint64_t *dst_off, const U32 *dest_caps,
                                     U32 *dest_lens, I32 *statuses, I32 level, I32 window_bits,
                                     I32 mem_level, ZlibStrategy strategy, U32 gzip_header_len)
{
    DeviceScope scope;
    if (zsc_hip_init(-1) != Z_OK)
        return Z_STREAM_ERROR;
    int wrap = 1, wbits = 15;
    if (!dpl_fold_params(&level, window_bits, mem_level, (int)strategy, &wrap, &wbits)) {
        ZSC_WARN4("zsc_hip: level %d / window_bits %d / mem_level %d / strategy %d is not "
                  "offloaded to the GPU yet (DESIGN.md, out of scope).",
                  level, window_bits, mem_level, (int)strategy);
        return Z_STREAM_ERROR;
    }

    /* wrapper header as deflate() writes it (src/deflate.c:1031-1049, :1068-1082) */
    uint32_t zh = (8u + (((uint32_t)wbits - 8u) << 4)) << 8;
    const uint32_t lf = (strategy >= Z_HUFFMAN_ONLY || level < 2) ? 0u : level < 6 ? 1u : level == 6 ? 2u : 3u;
    zh |= lf << 6;
    zh += 31u - zh % 31u;
    const uint32_t xfl = level == 9 ? 2u : (strategy >= Z_HUFFMAN_ONLY || level < 2) ? 4u : 0u;

    /* the host keeps a record per section: refuse what would not fit there, loudly */
    uint64_t nsections = 0;
    for (U32 i = 0; i < count; i++) {
        ZSC_ASSERT(max_block_lens[i] != 0);
        nsections += source_lens[i] / max_block_lens[i] + 1u;
    }
    if (nsections > (64ull << 20)) {
        ZSC_WARN1("zsc_hip: %llu sections in one call are more than the host side keeps track of.",
                  (unsigned long long)nsections);
        return Z_MEM_ERROR;
    }
    std::vector<SecStream> streams(count);
    std::vector<ZdBuf> sbufs(count);
    for (U32 i = 0; i < count; i++) {
        ZSC_ASSERT(max_block_lens[i] != 0);
        if (src_off[i] & 15u) {
            ZSC_WARN1("zsc_hip: stream %u is not 16-byte aligned in the batch.", i);
            return Z_STREAM_ERROR;
        }
        SecStream &s = streams[i];
        s.source_len = source_lens[i];
        s.max_block_len = max_block_lens[i];
        s.dest_cap = dest_caps[i];
        s.wrap = wrap;
        s.hdr_len = wrap == 1 ? 2u : wrap == 2 ? (gzip_header_len ? gzip_header_len : 10u) : 0u;
        s.need = strategy == Z_HUFFMAN_ONLY ? 1u : strategy == Z_RLE ? ZD_MAX_MATCH + 1u : ZD_MIN_LOOKAHEAD;
        memset(&sbufs[i], 0, sizeof(ZdBuf));
        sbufs[i].in_off = src_off[i];
        sbufs[i].in_len = source_lens[i];
        sbufs[i].wrap = (uint32_t)wrap;
    }
    DevBuf d_sbufs, d_sres, d_pieces;
    ZlibReturn rc = Z_OK;
    if (!d_sbufs.ensure(sizeof(ZdBuf) * count) || !d_sres.ensure(sizeof(ZdResult) * count))
        rc = Z_MEM_ERROR;
    if (rc == Z_OK && hipMemcpy(d_sbufs.p, sbufs.data(), sizeof(ZdBuf) * count, hipMemcpyHostToDevice) != hipSuccess)
        rc = Z_STREAM_ERROR;

    HipSecRunner runner;
    runner.d_src = d_src;
    runner.src_off = src_off;
    runner.level = level;
    runner.mem_level = mem_level;
    runner.wbits = wbits;
    runner.strategy = strategy;
    runner.streams = &streams;
    {
        /* a run is parsed again from its start whenever a joint turns up behind it; 64 times the input
         * (and 256 MB for small calls) is far beyond what any sensible call needs and bounds the rest */
        uint64_t total = 0;
        for (U32 i = 0; i < count; i++)
            total += source_lens[i];
        runner.budget_bytes = 64ull * total + (256ull << 20);
        if (const char *e = getenv("ZSC_HIP_SECTIONS_BUDGET_MB")) /* (test hook) */
            runner.budget_bytes = (uint64_t)atoll(e) << 20;
    }
    const auto t_begin = std::chrono::steady_clock::now();
    if (rc == Z_OK) {
        const int e = sec_compress(streams, runner);
        if (e != 0)
            rc = runner.error != Z_OK ? runner.error : Z_STREAM_ERROR;
    }
    const auto t_parsed = std::chrono::steady_clock::now();

    /* put the streams together: per round one launch that copies the runs' bytes, one for the
     * headers / markers / trailers */
    std::vector<std::vector<ZdStorePiece>> by_round(runner.rounds.size());
    std::vector<ZdStorePiece> small;
    for (U32 i = 0; i < count && rc == Z_OK; i++) {
        if (streams[i].status == SEC_Z_STREAM_ERROR) {
            ZSC_WARN1("zsc_hip: stream %u: the runs of sections do not fit together (a bug).", i);
            rc = Z_STREAM_ERROR;
            break;
        }
        for (const SecPiece &sp : streams[i].pieces) {
            if (sp.dst >= streams[i].delivered)
                continue; /* behind what the caller gets (dest too small) */
            ZdStorePiece pc;
            memset(&pc, 0, sizeof pc);
            pc.dst_off = dst_off[i] + sp.dst;
            pc.len = std::min(sp.len, streams[i].delivered - sp.dst);
            pc.buf = i;
            if (sp.kind == SEC_PIECE_RUN || sp.kind == SEC_PIECE_TAIL) {
                pc.kind = sp.kind == SEC_PIECE_RUN ? 6u : 7u;
                pc.src_off = runner.rounds[sp.round]->out_off[sp.job] + sp.src;
                pc.arg = sp.mask;
                by_round[sp.round].push_back(pc);
                continue;
            }
            /* a header / marker / trailer: k_store writes the first pc.len bytes of it */
            if (sp.kind == SEC_PIECE_HEADER) {
                pc.kind = wrap == 2 && gzip_header_len ? 4u : 2u; /* 4: zsc_api.c writes the caller's header */
                pc.arg = wrap == 1 ? zh : xfl;
            } else {
                pc.kind = sp.kind == SEC_PIECE_MARKER ? 5u : 3u;
            }
            small.push_back(pc);
        }
    }
    size_t most = small.size();
    for (const std::vector<ZdStorePiece> &v : by_round)
        most = std::max(most, v.size());
    if (rc == Z_OK && !d_pieces.ensure(sizeof(ZdStorePiece) * std::max<size_t>(1, most)))
        rc = Z_MEM_ERROR;
    if (rc == Z_OK)
        hipLaunchKernelGGL(k_checksum, dim3(count), dim3(64), 0, nullptr, d_src,
                           (const ZdBuf *)d_sbufs.p, (ZdResult *)d_sres.p, count);
    for (size_t r = 0; r <= by_round.size() && rc == Z_OK; r++) {
        const std::vector<ZdStorePiece> &v = r < by_round.size() ? by_round[r] : small;
        if (v.empty())
            continue;
        if (hipMemcpy(d_pieces.p, v.data(), sizeof(ZdStorePiece) * v.size(), hipMemcpyHostToDevice) != hipSuccess) {
            rc = Z_STREAM_ERROR;
            break;
        }
        const uint8_t *from = r < by_round.size() ? (const uint8_t *)runner.rounds[r]->d_out.p : d_src;
        hipLaunchKernelGGL(k_store, dim3((uint32_t)v.size()), dim3(256), 0, nullptr, from, d_dst,
                           (const ZdStorePiece *)d_pieces.p, (const ZdBuf *)d_sbufs.p,
                           (const ZdResult *)d_sres.p, (uint32_t)v.size());
        if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess)
            rc = Z_STREAM_ERROR; /* d_pieces is reused by the next launch */
    }
    for (U32 i = 0; i < count && rc == Z_OK; i++) {
        dest_lens[i] = streams[i].delivered;
        if (statuses)
            statuses[i] = (I32)streams[i].status;
    }
    if (getenv("ZSC_HIP_SECTIONS_LOG")) {
        const auto t_end = std::chrono::steady_clock::now();
        fprintf(stderr, "zsc_hip sections: %u streams, rounds + simulation %.2f ms, putting together %.2f ms; %u rounds, "
                        "%llu input bytes parsed, compressed bytes of rounds peak held %llu\n", count,
                std::chrono::duration<double, std::milli>(t_parsed - t_begin).count(),
                std::chrono::duration<double, std::milli>(t_end - t_parsed).count(), (unsigned)runner.rounds.size(),
                (unsigned long long)runner.parsed_bytes, (unsigned long long)runner.held_peak);
    }
    g_sections_last_rings[0] = runner.subs_wide;
    g_sections_last_rings[1] = runner.subs_narrow;
    d_sbufs.release();
    d_sres.release();
    d_pieces.release();
    return rc;
}

extern "C" void zsc_hip_compress_sections_last_rings(U32 *wide, U32 *narrow)
{
    if (wide)
        *wide = g_sections_last_rings[0];
    if (narrow)
        *narrow = g_sections_last_rings[1];
}

extern "C" ZlibReturn zsc_hip_compress_sections_device(U32 count, const void *d_input,
                                                       const uint64_t *in_offsets, const U32 *source_lens,
                                                       const U32 *max_block_lens, void *d_output,
                                                       const uint64_t *out_offsets, const U32 *out_caps,
                                                       U32 *dest_lens, I32 *statuses, I32 level,
                                                       I32 window_bits, I32 mem_level, ZlibStrategy strategy)
{
    DeviceScope scope;
    ZSC_ASSERT(d_input != Z_NULL);
    ZSC_ASSERT(in_offsets != Z_NULL);
    ZSC_ASSERT(source_lens != Z_NULL);
    ZSC_ASSERT(max_block_lens != Z_NULL);
    ZSC_ASSERT(d_output != Z_NULL);
    ZSC_ASSERT(out_offsets != Z_NULL);
    ZSC_ASSERT(out_caps != Z_NULL);
    ZSC_ASSERT(dest_lens != Z_NULL);
    if (count == 0)
        return Z_OK;
    return sections_on_device(count, (const uint8_t *)d_input, in_offsets, source_lens, max_block_lens,
                              (uint8_t *)d_output, out_offsets, out_caps, dest_lens, statuses, level,
                              window_bits, mem_level, strategy, 0);
}

extern "C" ZlibReturn zsc_hip_compress_sections_batch(U32 count, const U8 *const *sources,
                                                      const U32 *source_lens, const U32 *max_block_lens,
                                                      U8 *const *dests, U32 *dest_lens, I32 *statuses,
                                                      I32 level, I32 window_bits, I32 mem_level,
                                                      ZlibStrategy strategy, U32 gzip_header_len)
{
    DeviceScope scope;
    ZSC_ASSERT(sources != Z_NULL);
    ZSC_ASSERT(source_lens != Z_NULL);
    ZSC_ASSERT(max_block_lens != Z_NULL);
    ZSC_ASSERT(dests != Z_NULL);
    ZSC_ASSERT(dest_lens != Z_NULL);
    if (count == 0)
        return Z_OK;
    if (zsc_hip_init(-1) != Z_OK)
        return Z_STREAM_ERROR;
    std::vector<uint64_t> src_off(count), dst_off(count);
    std::vector<U32> caps(count), got(count);
    uint64_t in_bytes = 0, out_bytes = 0;
    for (U32 i = 0; i < count; i++) {
        ZSC_ASSERT(sources[i] != Z_NULL);
        ZSC_ASSERT(dests[i] != Z_NULL);
        src_off[i] = in_bytes;
        dst_off[i] = out_bytes;
        caps[i] = dest_lens[i];
        in_bytes += ((uint64_t)source_lens[i] + 15u) & ~15ull;
        /* a stream never grows past its bound by much, whatever dest the caller has */
        U32 bound = 0;
        if (zsc_compress_get_max_output_size2(source_lens[i], max_block_lens[i], level, window_bits,
                                              mem_level, &bound) != Z_OK)
            bound = dest_lens[i];
        const uint64_t room = std::min<uint64_t>(dest_lens[i], (uint64_t)bound + gzip_header_len +
                                                                   source_lens[i] / max_block_lens[i] * 8ull + 4096u);
        out_bytes += (room + 15u) & ~15ull;
    }
    DevBuf d_src, d_dst;
    ZlibReturn rc = Z_OK;
    if (!d_src.ensure(in_bytes + 64) || !d_dst.ensure(out_bytes + 64))
        rc = Z_MEM_ERROR;
    for (U32 i = 0; i < count && rc == Z_OK; i++)
        if (source_lens[i] && hipMemcpy((uint8_t *)d_src.p + src_off[i], sources[i], source_lens[i],
                                        hipMemcpyHostToDevice) != hipSuccess)
            rc = Z_STREAM_ERROR;
    if (rc == Z_OK)
        rc = sections_on_device(count, (const uint8_t *)d_src.p, src_off.data(), source_lens, max_block_lens,
                                (uint8_t *)d_dst.p, dst_off.data(), caps.data(), got.data(), statuses, level,
                                window_bits, mem_level, strategy, gzip_header_len);
    for (U32 i = 0; i < count && rc == Z_OK; i++) {
        if (got[i] && hipMemcpy(dests[i], (uint8_t *)d_dst.p + dst_off[i], got[i], hipMemcpyDeviceToHost) != hipSuccess)
            rc = Z_STREAM_ERROR;
        dest_lens[i] = got[i];
    }
    d_src.release();
    d_dst.release();
    return rc;
}

/* host-pointer batch: stage through one pair of device buffers */
extern "C" ZlibReturn zsc_hip_compress_batch(U32 count, const U8 *const *sources,
                                             const U32 *source_lens, U8 *const *dests,
                                             U32 *dest_lens, I32 *statuses, I32 level,
                                             I32 window_bits, I32 mem_level,
                                             ZlibStrategy strategy)
{
    DeviceScope scope;
    ZSC_ASSERT(sources != Z_NULL);
    ZSC_ASSERT(source_lens != Z_NULL);
    ZSC_ASSERT(dests != Z_NULL);
    ZSC_ASSERT(dest_lens != Z_NULL);
    if (count == 0)
        return Z_OK;
    if (level == Z_NO_COMPRESSION) {
        /* level 0: stored blocks; max_block_len = source_len, the smallest a single section allows */
        std::vector<U32> mbl(count);
        for (U32 i = 0; i < count; i++)
            mbl[i] = source_lens[i] ? source_lens[i] : 1u;
        return zsc_hip_store_batch(count, sources, source_lens, mbl.data(), dests, dest_lens, statuses,
                                   window_bits, mem_level, 0);
    }
    std::vector<uint64_t> in_off(count), out_off(count);
    std::vector<U32> caps(count), lens(count);
    std::vector<I32> stat(count);
    uint64_t in_bytes = 0, out_bytes = 0;
    ZlibReturn rc = zsc_hip_deflate_plan_layout(count, source_lens, level, window_bits, mem_level,
                                                in_off.data(), out_off.data(), caps.data(),
                                                &in_bytes, &out_bytes);
    if (rc != Z_OK)
        return rc;
    zsc_hip_deflate_plan *pl = nullptr;
    rc = zsc_hip_deflate_plan_create(&pl, count, source_lens, in_off.data(), out_off.data(),
                                     caps.data(), level, window_bits, mem_level, strategy);
    if (rc != Z_OK)
        return rc;
    DevBuf d_in, d_out;
    if (!d_in.ensure(in_bytes) || !d_out.ensure(out_bytes)) {
        d_in.release();
        d_out.release();
        zsc_hip_deflate_plan_destroy(pl);
        return Z_MEM_ERROR;
    }
    rc = Z_OK;
    for (U32 i = 0; i < count && rc == Z_OK; i++) {
        ZSC_ASSERT(sources[i] != Z_NULL);
        if (source_lens[i] &&
            hipMemcpy((uint8_t *)d_in.p + in_off[i], sources[i], source_lens[i],
                      hipMemcpyHostToDevice) != hipSuccess)
            rc = Z_STREAM_ERROR;
    }
    if (rc == Z_OK)
        rc = zsc_hip_deflate_plan_run(pl, d_in.p, d_out.p, nullptr);
    if (rc == Z_OK)
        rc = zsc_hip_deflate_plan_results(pl, lens.data(), stat.data());
    for (U32 i = 0; i < count && rc == Z_OK; i++) {
        ZSC_ASSERT(dests[i] != Z_NULL);
        const U32 cap = dest_lens[i];
        I32 s = stat[i];
        U32 give = lens[i];
        if (s == Z_OK && give > cap) {
            /* the reference hands out dest in slices and fails once it is used up:
             * the caller keeps the prefix that fitted (src/zsc_compress.c:126-140) */
            give = cap;
            s = Z_BUF_ERROR;
        } else if (s != Z_OK) {
            give = 0;
        }
        if (give && hipMemcpy(dests[i], (uint8_t *)d_out.p + out_off[i], give,
                              hipMemcpyDeviceToHost) != hipSuccess)
            rc = Z_STREAM_ERROR;
        dest_lens[i] = give;
        if (statuses)
            statuses[i] = s;
    }
    d_in.release();
    d_out.release();
    zsc_hip_deflate_plan_destroy(pl);
    return rc;
}

/* wavefronts of k_inflate: enough to fill every CU at its occupancy, never more than the streams need */
static uint32_t inflate_grid(uint32_t count)
{
    const uint32_t need = (count + INF_PER_WAVE - 1) / INF_PER_WAVE;
    const uint32_t fill = (uint32_t)g_cus * 4u * INF_WAVES_EU;
    return std::max(1u, std::min(need, fill));
}

#include "inflate_plan_layout.h"

enum InfPlanKind { INF_PLAIN, INF_SECTIONS, INF_RESYNC, INF_CHUNKS, INF_INDEXED, INF_SIZE, INF_CHECK, INF_MEMBERS, INF_BGZF_RANGES };

struct zsc_hip_inflate_plan {
    /* a device buffer of the plan: it cannot be declared without joining `owned`, which destroy releases */
    struct Buf : DevBuf {
        explicit Buf(std::vector<DevBuf *> &owned) { owned.push_back(this); }
    };
    std::vector<DevBuf *> owned;
    InfPlanKind kind = INF_PLAIN;
    /* what a kind has, and with it which entry points serve it */
    bool has_sections() const { return kind == INF_SECTIONS || kind == INF_RESYNC; } /* resync: a sections plan with more */
    bool writes_nothing() const /* check: a size plan with more; members: in size-only mode */
    {
        return kind == INF_SIZE || kind == INF_CHECK || (kind == INF_MEMBERS && mp.size_only);
    }
    bool has_chunks() const { return kind == INF_CHUNKS || kind == INF_SIZE || kind == INF_CHECK; } /* cp and the chunk records */
    bool has_rings() const { return kind == INF_CHECK; }                             /* a ring per lane group, a value per stream */
    bool counts_pieces() const { return kind != INF_PLAIN && kind != INF_BGZF_RANGES; } /* the others keep d_nsec, a sections plan's */
    uint32_t count = 0;
    int32_t window_bits = 15;
    Buf d_items{owned}, d_order{owned}, d_res{owned}, d_resume{owned}, d_pending{owned};
    /* sections plans (inflate_sections.h) */
    IsecPlan sp = {};
    uint64_t ncand_total = 0, scratch_bytes = 0;
    Buf d_sitems{owned}, d_tiles{owned}, d_tile_cnt{owned}, d_tile_off{owned}, d_scount{owned}, d_nsec{owned},
        d_sst{owned}, d_active{owned}, d_q{owned};
    Buf d_cstart{owned}, d_cstop{owned}, d_clink{owned}, d_clen{owned}, d_chain_k{owned}, d_chain_off{owned},
        d_chain_ck{owned};
    /* chunks plans (inflate_chunks.h; they also use the sections plan's buffers above) */
    IchkPlan cp = {};
    Buf d_cand{owned}, d_cused{owned}, d_creach{owned}, d_want{owned}, d_ring{owned}, d_win{owned};
    /* resync plans (inflate_resync.h; sections plans with these buffers besides) */
    IrsyPlan rp = {};
    Buf d_cerr{owned}, d_chain_fl{owned}, d_rst{owned};
    /* members plans (inflate_members.h; sections plans' buffers, scanned for another pattern, and this one) */
    MemPlan mp = {};
    Buf d_mfiles{owned};
    /* BGZF ranges plans (bgzf_read.h): a plain plan's buffers (d_items for the packs, d_res, and d_resume and
     * d_pending, which a run zeroes so that _results relaunches nothing) and none of the kinds' above; bgr_waves: wavefronts of k_bgr_range, with
     * BGR_SLOT bytes of d_bstage for each lane group where the plan has an edge job */
    BgrPlan bp = {};
    uint32_t bgr_waves = 0;
    Buf d_bfiles{owned}, d_bjobs{owned}, d_bbad{owned}, d_bq{owned}, d_bstage{owned}, d_bres0{owned};
    /* size plans (inflate_size.h; with chunks they use cp and the chunks plan's record buffers, never
     * d_ring, d_win or d_chain_ck) */
    bool size_ran = false;
    /* check plans (inflate_check.h): size plans (relaunches are the size decode) whose first launch decodes
     * into rings; with chunks they use every buffer of a chunks plan */
    uint32_t check_waves = 0; /* wavefronts of k_inflate_check: d_rings holds CHK_RING bytes for each lane group */
    Buf d_rings{owned}, d_ckval{owned};
    /* indexed plans (inflate_index.h; they also use d_sitems, d_sst, d_active, d_q, d_nsec, d_clen,
     * d_chain_k, d_chain_ck, d_cand and d_win) */
    bool idx_fixed = false;
    IidxPlan ip = {};
    uint32_t idx_active = 0;
    Buf d_sst0{owned}, d_q0{owned}, d_ipieces{owned}, d_iunits{owned}, d_ixs{owned}, d_idone{owned}, d_res0{owned},
        d_resume0{owned};
    /* chunks plans with the index enabled: the records of the streams asked for since the last run */
    std::map<uint32_t, std::pair<std::vector<ZidxRec>, uint64_t>> idx_recs;
    const void *last_src = nullptr;
    void *last_dst = nullptr;
    hipStream_t last_stream = nullptr;
    Enqueued ran; /* the runs; the packs keep their own (pack.work) */
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    /* packing (pack.h), off unless zsc_hip_inflate_plan_pack_enable was called */
    PackState pack;
    /* preset dictionaries, off unless zsc_hip_inflate_plan_dict_enable was called (plain plans only): the window
     * images, a ZdInfDict per dictionary and every stream's index */
    bool dict_on = false;
    uint64_t dict_scratch = 0; /* what of scratch_bytes they hold */
    std::vector<U32> dict_ids;
    Buf d_dict_img{owned}, d_dict_tab{owned}, d_dict_of{owned};

    /* a buffer beyond a plain plan's: its bytes are the plan's scratch */
    bool scratch(DevBuf &b, uint64_t bytes)
    {
        scratch_bytes += bytes;
        return b.ensure(bytes);
    }
    /* what sp and cp point into (null where the kind has no such buffer) */
    InfPlanMem mem() const
    {
        return {d_sitems.p, d_tiles.p, d_tile_cnt.p, d_tile_off.p, d_scount.p, d_nsec.p, d_sst.p, d_active.p,
                d_q.p, d_cstart.p, d_cstop.p, d_clink.p, d_clen.p, d_chain_k.p, d_chain_off.p, d_chain_ck.p,
                d_cand.p, d_cused.p, d_creach.p, d_want.p, d_ring.p, d_win.p};
    }
};

/* the host waits for everything the plan has enqueued, whatever streams it went to */
static hipError_t inflate_wait_all(zsc_hip_inflate_plan *pl)
{
    const hipError_t a = work_wait(pl->ran), b = work_wait(pl->pack.work);
    return a != hipSuccess ? a : b;
}

static void inflate_plan_release(zsc_hip_inflate_plan *pl)
{
    for (DevBuf *b : pl->owned)
        b->release();
}

/* the error exit of the create functions once the plain plan exists */
static ZlibReturn inflate_plan_fail(zsc_hip_inflate_plan **plan_out, ZlibReturn rc = Z_MEM_ERROR)
{
    zsc_hip_inflate_plan_destroy(*plan_out);
    *plan_out = nullptr;
    return rc;
}

/* the items, the tiles the scan visits and the active streams of a layout, uploaded */
static bool inflate_layout_upload(zsc_hip_inflate_plan *pl, const InfLayout &L)
{
    bool ok = true;
    if (!L.items.empty())
        ok = hipMemcpy(pl->d_sitems.p, L.items.data(), sizeof(IsecItem) * L.items.size(), hipMemcpyHostToDevice) ==
             hipSuccess;
    if (ok && !L.tiles.empty())
        ok = hipMemcpy(pl->d_tiles.p, L.tiles.data(), sizeof(IsecTile) * L.tiles.size(), hipMemcpyHostToDevice) ==
             hipSuccess;
    if (ok && !L.active.empty())
        ok = hipMemcpy(pl->d_active.p, L.active.data(), 4 * L.active.size(), hipMemcpyHostToDevice) == hipSuccess;
    return ok;
}

extern "C" ZlibReturn zsc_hip_inflate_plan_create_ordered(zsc_hip_inflate_plan **plan_out, U32 count,
                                                  const U32 *source_lens,
                                                  const uint64_t *src_offsets,
                                                  const U32 *dest_caps,
                                                  const uint64_t *dst_offsets, I32 window_bits,
                                                       const U32 *decode_order)
{
    DeviceScope scope;
    ZSC_ASSERT(plan_out != Z_NULL);
    *plan_out = nullptr;
    if (zsc_hip_init(-1) != Z_OK)
        return Z_STREAM_ERROR;
    auto *pl = new zsc_hip_inflate_plan();
    pl->count = count;
    pl->window_bits = window_bits;
    std::vector<ZdInfItem> items(count);
    std::vector<uint32_t> order(count);
    for (U32 i = 0; i < count; i++) {
        items[i].src_off = src_offsets[i];
        items[i].dst_off = dst_offsets[i];
        items[i].src_len = source_lens[i];
        items[i].dst_cap = dest_caps[i];
        order[i] = i;
        if ((src_offsets[i] | dst_offsets[i]) & 15u) {
            /* (the decoder reads a stream's last, partial dword whole: it must not straddle a page) */
            ZSC_WARN1("zsc_hip: stream %u is not 16-byte aligned in the batch.", i);
            delete pl;
            return Z_STREAM_ERROR;
        }
    }
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t a, uint32_t b) { return items[a].dst_cap > items[b].dst_cap; });
    if (decode_order) {
        /* the caller's order: a permutation of the streams (checked), e.g. to keep the replicas of one
         * stream of a benchmark batch from sharing wavefronts (bench.py) */
        std::vector<uint8_t> seen(count, 0);
        for (uint32_t k = 0; k < count; k++) {
            if (decode_order[k] >= count || seen[decode_order[k]]) {
                ZSC_WARN1("zsc_hip: decode_order is not a permutation (entry %u).", k);
                delete pl;
                return Z_STREAM_ERROR;
            }
            seen[decode_order[k]] = 1;
            order[k] = decode_order[k];
        }
    }
    bool ok = pl->d_items.ensure(sizeof(ZdInfItem) * std::max(1u, count)) &&
              pl->d_order.ensure(4ull * std::max(1u, count)) &&
              pl->d_res.ensure(sizeof(InfResult) * std::max(1u, count)) &&
              pl->d_resume.ensure(sizeof(InfResume) * std::max(1u, count)) && pl->d_pending.ensure(8);
    if (ok && count) {
        ok = hipMemcpy(pl->d_items.p, items.data(), sizeof(ZdInfItem) * count,
                       hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(pl->d_order.p, order.data(), 4ull * count, hipMemcpyHostToDevice) ==
                 hipSuccess;
    }
    if (!ok) {
        inflate_plan_release(pl);
        delete pl;
        return Z_MEM_ERROR;
    }
    (void)hipEventCreate(&pl->ev0);
    (void)hipEventCreate(&pl->ev1);
    *plan_out = pl;
    return Z_OK;
}

extern "C" ZlibReturn zsc_hip_inflate_plan_create(zsc_hip_inflate_plan **plan_out, U32 count,
                                                  const U32 *source_lens,
                                                  const uint64_t *src_offsets,
                                                  const U32 *dest_caps,
                                                  const uint64_t *dst_offsets, I32 window_bits)
{
    return zsc_hip_inflate_plan_create_ordered(plan_out, count, source_lens, src_offsets, dest_caps, dst_offsets,
                                               window_bits, Z_NULL);
}

extern "C" ZlibReturn zsc_hip_inflate_plan_create_sections(zsc_hip_inflate_plan **plan_out, U32 count,
                                                           const U32 *source_lens,
                                                           const uint64_t *src_offsets,
                                                           const U32 *dest_caps,
                                                           const uint64_t *dst_offsets, I32 window_bits)
{
    ZlibReturn rc = zsc_hip_inflate_plan_create(plan_out, count, source_lens, src_offsets, dest_caps, dst_offsets,
                                                window_bits);
    if (rc != Z_OK)
        return rc;
    DeviceScope scope;
    zsc_hip_inflate_plan *pl = *plan_out;
    pl->kind = INF_SECTIONS;
    InfLayout L;
    sec_layout(count, source_lens, src_offsets, dst_offsets, dest_caps, L);
    if (L.tiles.size() >= 0xffffffffull)
        return inflate_plan_fail(plan_out);
    const uint64_t nt = std::max<uint64_t>(1, L.tiles.size()), nc = std::max<uint64_t>(1, count), cand = L.pool;
    pl->ncand_total = cand;
    bool ok = pl->scratch(pl->d_sitems, sizeof(IsecItem) * nc) && pl->scratch(pl->d_tiles, sizeof(IsecTile) * nt) &&
              pl->scratch(pl->d_tile_cnt, 4 * nt) && pl->scratch(pl->d_tile_off, 4 * nt) &&
              pl->scratch(pl->d_scount, 4 * nc) && pl->scratch(pl->d_nsec, 4 * nc) &&
              pl->scratch(pl->d_sst, sizeof(IsecStream) * nc) && pl->scratch(pl->d_active, 4 * nc) &&
              pl->scratch(pl->d_q, 16) && pl->scratch(pl->d_cstart, 4 * cand) && pl->scratch(pl->d_cstop, 4 * cand) &&
              pl->scratch(pl->d_clink, 4 * cand) && pl->scratch(pl->d_clen, 4 * cand) &&
              pl->scratch(pl->d_chain_k, 4 * cand) && pl->scratch(pl->d_chain_off, 4 * cand) &&
              pl->scratch(pl->d_chain_ck, 4 * cand);
    if (!ok || !inflate_layout_upload(pl, L))
        return inflate_plan_fail(plan_out);
    sec_plan_view(pl->sp, pl->mem(), L, window_bits);
    return Z_OK;
}

/* a sections plan's buffers over files, the candidate cap of mem_layout, and a MemFile per file */
extern "C" ZlibReturn zsc_hip_inflate_plan_create_members(zsc_hip_inflate_plan **plan_out, U32 count,
                                                          const U32 *source_lens, const uint64_t *src_offsets,
                                                          const U32 *dest_caps, const uint64_t *dst_offsets,
                                                          I32 window_bits, U32 flags)
{
    ZSC_ASSERT(plan_out != Z_NULL);
    *plan_out = nullptr;
    const bool size_only = (flags & ZSC_HIP_MEMBERS_SIZE_ONLY) != 0;
    if (window_bits < 16 + 8 || window_bits > 16 + 15 || (flags & ~(U32)ZSC_HIP_MEMBERS_SIZE_ONLY) ||
        (!size_only && (dest_caps == Z_NULL || dst_offsets == Z_NULL))) {
        ZSC_WARN("zsc_hip: a members plan takes window_bits 24..31 (the gzip wrapper) and, unless size-only, destinations.");
        return Z_STREAM_ERROR;
    }
    InfLayout L;
    mem_layout(count, source_lens, src_offsets, size_only ? Z_NULL : dst_offsets, dest_caps, L);
    std::vector<uint64_t> doff(count);
    std::vector<U32> caps(count);
    for (U32 i = 0; i < count; i++) {
        doff[i] = L.items[i].dst_off;
        caps[i] = L.items[i].dst_cap;
    }
    ZlibReturn rc = zsc_hip_inflate_plan_create(plan_out, count, source_lens, src_offsets, caps.data(), doff.data(),
                                                window_bits);
    if (rc != Z_OK)
        return rc;
    DeviceScope scope;
    zsc_hip_inflate_plan *pl = *plan_out;
    pl->kind = INF_MEMBERS;
    if (L.tiles.size() >= 0xffffffffull)
        return inflate_plan_fail(plan_out);
    const uint64_t nt = std::max<uint64_t>(1, L.tiles.size()), nc = std::max<uint64_t>(1, count), cand = L.pool;
    pl->ncand_total = cand;
    bool ok = pl->scratch(pl->d_sitems, sizeof(IsecItem) * nc) && pl->scratch(pl->d_tiles, sizeof(IsecTile) * nt) &&
              pl->scratch(pl->d_tile_cnt, 4 * nt) && pl->scratch(pl->d_tile_off, 4 * nt) &&
              pl->scratch(pl->d_scount, 4 * nc) && pl->scratch(pl->d_nsec, 4 * nc) &&
              pl->scratch(pl->d_sst, sizeof(IsecStream) * nc) && pl->scratch(pl->d_active, 4 * nc) &&
              pl->scratch(pl->d_q, 16) && pl->scratch(pl->d_cstart, 4 * cand) && pl->scratch(pl->d_cstop, 4 * cand) &&
              pl->scratch(pl->d_clink, 4 * cand) && pl->scratch(pl->d_clen, 4 * cand) &&
              pl->scratch(pl->d_chain_k, 4 * cand) && pl->scratch(pl->d_chain_off, 4 * cand) &&
              (size_only || pl->scratch(pl->d_chain_ck, 4 * cand)) && pl->scratch(pl->d_mfiles, sizeof(MemFile) * nc);
    if (!ok || !inflate_layout_upload(pl, L))
        return inflate_plan_fail(plan_out);
    bool claims = true;
    if (const char *e = getenv("ZSC_HIP_MEMBERS_CLAIMS")) /* (a test hook, and the A/B switch of the claims step) */
        claims = atoi(e) != 0;
    mem_plan_view(pl->mp, pl->mem(), L, window_bits, pl->d_mfiles.p, size_only, claims);
    return Z_OK;
}

/* what the chunk family (chunks, size and check plans) has beyond the plain plan, over the layout L of chunks
 * of cb bytes: the sections plan's per-stream buffers, the candidates and the records of a chunk, and
 * by kind the buffers of pieces that produce bytes */
static ZlibReturn chunk_records_create(zsc_hip_inflate_plan **plan_out, U32 count, const InfLayout &L, uint32_t cb)
{
    zsc_hip_inflate_plan *pl = *plan_out;
    const uint64_t nchunks = L.pool;
    if (nchunks >= 0x03ffffffull) /* (links hold chunk * 4 + candidate in 28 bits) */
        return inflate_plan_fail(plan_out);
    const uint64_t nt = std::max<uint64_t>(1, L.tiles.size()), nc = std::max<uint64_t>(1, count);
    const uint64_t ch = std::max<uint64_t>(1, nchunks);
    /* the candidates and the records of a chunk */
    bool ok = pl->scratch(pl->d_sitems, sizeof(IsecItem) * nc) && pl->scratch(pl->d_tiles, sizeof(IsecTile) * nt) &&
              pl->scratch(pl->d_nsec, 4 * nc) && pl->scratch(pl->d_sst, sizeof(IsecStream) * nc) &&
              pl->scratch(pl->d_active, 4 * nc) && pl->scratch(pl->d_q, 16) && pl->scratch(pl->d_cstop, 4 * ch) &&
              pl->scratch(pl->d_clink, 4 * ch) && pl->scratch(pl->d_clen, 4 * ch) &&
              pl->scratch(pl->d_chain_k, 4 * ch) && pl->scratch(pl->d_chain_off, 4 * ch) &&
              pl->scratch(pl->d_cand, 8ull * INF_PC_CANDS * ch) && pl->scratch(pl->d_cused, 4 * ch) &&
              pl->scratch(pl->d_creach, 4 * ch) && pl->scratch(pl->d_want, 4 * ch);
    /* a size plan: no ring, no window, no slice check values.  A check plan has rings and windows for the
     * streams with chunks only, 16 bytes behind each */
    if (pl->kind == INF_CHUNKS)
        ok = ok && pl->scratch(pl->d_chain_ck, 4 * ch) && pl->scratch(pl->d_ring, 2ull * INF_WIN * ch) &&
             pl->scratch(pl->d_win, (uint64_t)INF_WIN * ch);
    if (pl->has_rings()) {
        /* ZSC_HIP_CHECK_GROUPS (a test hook): fewer lane groups, so that every ring is reused by several streams */
        pl->check_waves = inflate_grid(count);
        if (const char *e = getenv("ZSC_HIP_CHECK_GROUPS")) {
            const long long g = atoll(e);
            if (g > 0)
                pl->check_waves = (uint32_t)std::min<long long>(pl->check_waves, (g + INF_PER_WAVE - 1) / INF_PER_WAVE);
        }
        ok = ok && pl->scratch(pl->d_chain_ck, 4 * ch) &&
             pl->scratch(pl->d_ring, 2ull * INF_WIN * (nchunks ? ch : 0) + 16) &&
             pl->scratch(pl->d_win, (uint64_t)INF_WIN * (nchunks ? ch : 0) + 16) &&
             pl->scratch(pl->d_rings, (uint64_t)CHK_RING * pl->check_waves * INF_PER_WAVE) &&
             pl->scratch(pl->d_ckval, 4 * nc);
    }
    if (!ok || !inflate_layout_upload(pl, L))
        return inflate_plan_fail(plan_out);
    chk_plan_view(pl->cp, pl->mem(), L, pl->window_bits, cb);
    pl->ncand_total = nchunks;
    if (pl->has_rings()) {
        /* the one figure that is not the sum of the allocations: a chunks plan's scratch for the streams with
         * chunks (the chunks there are, not the one record allocated when there is none, and without the 16
         * bytes behind the rings and windows), a ring per lane group, a value per stream */
        pl->scratch_bytes = (sizeof(IsecItem) + sizeof(IsecStream) + 8) * nc + 16 + sizeof(IsecTile) * nt +
                            (8ull * INF_PC_CANDS + 36 + 3ull * INF_WIN) * nchunks +
                            (uint64_t)CHK_RING * pl->check_waves * INF_PER_WAVE + 4 * nc;
    }
    return Z_OK;
}

extern "C" ZlibReturn zsc_hip_inflate_plan_create_chunks(zsc_hip_inflate_plan **plan_out, U32 count,
                                                         const U32 *source_lens, const uint64_t *src_offsets,
                                                         const U32 *dest_caps, const uint64_t *dst_offsets,
                                                         I32 window_bits, U32 chunk_bytes)
{
    ZlibReturn rc = zsc_hip_inflate_plan_create(plan_out, count, source_lens, src_offsets, dest_caps, dst_offsets,
                                                window_bits);
    if (rc != Z_OK)
        return rc;
    DeviceScope scope;
    (*plan_out)->kind = INF_CHUNKS;
    const uint32_t cb = chunk_bytes == 0 ? CHK_DEFAULT_BYTES : std::max<uint32_t>(chunk_bytes, CHK_MIN_BYTES);
    /* per stream longer than a chunk (and with less than 2 GiB of output: positions inside a piece
     * are signed 32-bit): its chunks; the scan visits every chunk but the first */
    InfLayout L;
    chk_layout(count, source_lens, src_offsets, dst_offsets, dest_caps, cb,
               [&](U32 i) { return dest_caps[i] < 0x80000000u; }, L);
    return chunk_records_create(plan_out, count, L, cb);
}

/* a size plan, or (check) a check plan: the same items, queue order and chunk records, and for a check plan
 * the chunks plan's rings, windows and slice check values, the lane groups' rings and the values */
static ZlibReturn size_plan_create(zsc_hip_inflate_plan **plan_out, U32 count, const U32 *source_lens,
                                   const uint64_t *src_offsets, const U32 *dest_limits, I32 window_bits,
                                   U32 chunk_bytes, bool check)
{
    ZSC_ASSERT(plan_out != Z_NULL);
    *plan_out = nullptr;
    /* a plain plan's items with the limits for capacities and no destination; the queue hands out the
     * longest inputs first (the capacities, all alike by default, say nothing about the decoding time) */
    std::vector<U32> limits(count), order(count);
    std::vector<uint64_t> dof(count, 0);
    for (U32 i = 0; i < count; i++) {
        limits[i] = dest_limits ? dest_limits[i] : 0xffffffffu;
        order[i] = i;
    }
    std::stable_sort(order.begin(), order.end(), [&](U32 a, U32 b) { return source_lens[a] > source_lens[b]; });
    ZlibReturn rc = zsc_hip_inflate_plan_create_ordered(plan_out, count, source_lens, src_offsets, limits.data(),
                                                        dof.data(), window_bits, order.data());
    if (rc != Z_OK)
        return rc;
    DeviceScope scope;
    (*plan_out)->kind = check ? INF_CHECK : INF_SIZE;
    const uint32_t cb = chunk_bytes == 0 ? CHK_DEFAULT_BYTES : std::max<uint32_t>(chunk_bytes, CHK_MIN_BYTES);
    /* per stream longer than a chunk: its chunks; the scan visits every chunk but the first (any limit
     * will do: a piece is only counted, no position inside it is ever signed) */
    InfLayout L;
    chk_layout(count, source_lens, src_offsets, nullptr, limits.data(), cb,
               [&](U32) { return chunk_bytes != 0xffffffffu; }, L);
    /* (a check plan's pieces sign positions in 32 bits, as a chunks plan's: a stream of 2 GiB or more is
     * left to the whole-stream decode by this limit) */
    if (check)
        for (IsecItem &it : L.items)
            it.dst_cap = std::min<uint32_t>(it.dst_cap, 0x7fffffffu);
    return chunk_records_create(plan_out, count, L, cb);
}

extern "C" ZlibReturn zsc_hip_inflate_plan_create_size(zsc_hip_inflate_plan **plan_out, U32 count,
                                                       const U32 *source_lens, const uint64_t *src_offsets,
                                                       const U32 *dest_limits, I32 window_bits, U32 chunk_bytes)
{
    return size_plan_create(plan_out, count, source_lens, src_offsets, dest_limits, window_bits, chunk_bytes, false);
}

extern "C" ZlibReturn zsc_hip_inflate_plan_create_check(zsc_hip_inflate_plan **plan_out, U32 count,
                                                        const U32 *source_lens, const uint64_t *src_offsets,
                                                        const U32 *dest_limits, I32 window_bits, U32 chunk_bytes)
{
    return size_plan_create(plan_out, count, source_lens, src_offsets, dest_limits, window_bits, chunk_bytes, true);
}

extern "C" ZlibReturn zsc_hip_inflate_plan_create_resync(zsc_hip_inflate_plan **plan_out, U32 count,
                                                         const U32 *source_lens, const uint64_t *src_offsets,
                                                         const U32 *dest_caps, const uint64_t *dst_offsets,
                                                         I32 window_bits)
{
    ZlibReturn rc = zsc_hip_inflate_plan_create_sections(plan_out, count, source_lens, src_offsets, dest_caps,
                                                         dst_offsets, window_bits);
    if (rc != Z_OK)
        return rc;
    DeviceScope scope;
    zsc_hip_inflate_plan *pl = *plan_out;
    pl->kind = INF_RESYNC;
    const uint64_t cand = pl->ncand_total, nc = std::max(1u, count);
    if (!pl->scratch(pl->d_cerr, 8 * cand) || !pl->scratch(pl->d_chain_fl, 4 * cand) ||
        !pl->scratch(pl->d_rst, sizeof(IrsyStream) * nc))
        return inflate_plan_fail(plan_out);
    IrsyPlan &R = pl->rp;
    R.sp = pl->sp;
    R.cerr = (uint64_t *)pl->d_cerr.p;
    R.chain_fl = (uint32_t *)pl->d_chain_fl.p;
    R.rst = (IrsyStream *)pl->d_rst.p;
    return Z_OK;
}

extern "C" ZlibReturn zsc_hip_inflate_plan_create_indexed(zsc_hip_inflate_plan **plan_out, U32 count,
                                                          const U32 *source_lens, const uint64_t *src_offsets,
                                                          const U32 *dest_caps, const uint64_t *dst_offsets,
                                                          I32 window_bits, const U8 *const *indexes,
                                                          const uint64_t *index_lens, const uint64_t *range_begins,
                                                          const uint64_t *range_lens)
{
    ZSC_ASSERT(plan_out != Z_NULL);
    *plan_out = nullptr;
    /* the blobs are checked and the tables built on the host before anything is allocated */
    IdxBuild B;
    for (U32 i = 0; i < count; i++) {
        const bool ranged = range_begins && range_lens && range_lens[i] != ~0ull;
        const U8 *blob = indexes && index_lens ? indexes[i] : Z_NULL;
        if (B.add(source_lens[i], src_offsets[i], dest_caps[i], dst_offsets[i], window_bits, blob,
                  blob ? index_lens[i] : 0, ranged, ranged ? range_begins[i] : 0, ranged ? range_lens[i] : 0) != 0) {
            ZSC_WARN1("zsc_hip: the range of stream %u is not inside its output.", i);
            return Z_STREAM_ERROR;
        }
    }
    B.finish();
    if (B.pieces.size() >= 0xffffffffull)
        return Z_MEM_ERROR;
    ZlibReturn rc = zsc_hip_inflate_plan_create(plan_out, count, source_lens, src_offsets, dest_caps, dst_offsets,
                                                window_bits);
    if (rc != Z_OK)
        return rc;
    DeviceScope scope;
    zsc_hip_inflate_plan *pl = *plan_out;
    pl->kind = INF_INDEXED;
    pl->idx_fixed = B.any_fixed;
    pl->idx_active = (uint32_t)B.active.size();
    const uint64_t nc = std::max<uint64_t>(1, count), np = std::max<uint64_t>(1, B.pieces.size());
    const uint64_t ncand = std::max<uint64_t>(1, B.cand.size());
    const uint32_t q0[4] = {pl->idx_active, 0, 0, 0};
    std::vector<InfResume> resume0(nc);
    memset(resume0.data(), 0, sizeof(InfResume) * nc);
    for (U32 i = 0; i < count; i++)
        resume0[i].state = B.state0[i];
    struct Up {
        DevBuf *buf;
        const void *from;
        uint64_t bytes, have;
    };
    const Up ups[] = {
        {&pl->d_sitems, B.items.data(), sizeof(IsecItem) * nc, sizeof(IsecItem) * count},
        {&pl->d_sst0, B.st.data(), sizeof(IsecStream) * nc, sizeof(IsecStream) * count},
        {&pl->d_sst, nullptr, sizeof(IsecStream) * nc, 0},
        {&pl->d_ixs, B.xs.data(), sizeof(IdxStream) * nc, sizeof(IdxStream) * count},
        {&pl->d_active, B.active.data(), 4 * nc, 4ull * B.active.size()},
        {&pl->d_q0, q0, 16, 16},
        {&pl->d_q, nullptr, 16, 0},
        {&pl->d_nsec, nullptr, 4 * nc, 0},
        {&pl->d_idone, nullptr, 4 * nc, 0},
        {&pl->d_res0, B.res0.data(), sizeof(InfResult) * nc, sizeof(InfResult) * count},
        {&pl->d_resume0, resume0.data(), sizeof(InfResume) * nc, sizeof(InfResume) * count},
        {&pl->d_ipieces, B.pieces.data(), sizeof(IdxPiece) * np, sizeof(IdxPiece) * B.pieces.size()},
        {&pl->d_iunits, B.units.data(), 4 * np, 4ull * B.units.size()},
        {&pl->d_clen, B.clen.data(), 4 * np, 4ull * B.clen.size()},
        {&pl->d_chain_k, B.chain_k.data(), 4 * np, 4ull * B.chain_k.size()},
        {&pl->d_chain_ck, nullptr, 4 * np, 0},
        {&pl->d_cand, B.cand.data(), 8 * ncand, 8ull * B.cand.size()},
        {&pl->d_win, B.win.data(), B.win.size(), B.win.size()},
    };
    bool ok = true;
    for (const Up &u : ups) {
        ok = ok && pl->scratch(*u.buf, u.bytes);
        if (ok && u.have)
            ok = hipMemcpy(u.buf->p, u.from, u.have, hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok)
        return inflate_plan_fail(plan_out);
    IidxPlan &P = pl->ip;
    P.sp.items = (const IsecItem *)pl->d_sitems.p;
    P.sp.nsec = (uint32_t *)pl->d_nsec.p;
    P.sp.st = (IsecStream *)pl->d_sst.p;
    P.sp.active = (uint32_t *)pl->d_active.p;
    P.sp.q = (uint32_t *)pl->d_q.p;
    P.sp.clen = (uint32_t *)pl->d_clen.p;
    P.sp.chain_k = (uint32_t *)pl->d_chain_k.p;
    P.sp.chain_ck = (uint32_t *)pl->d_chain_ck.p;
    P.sp.count = count;
    P.sp.window_bits = window_bits;
    P.pieces = (const IdxPiece *)pl->d_ipieces.p;
    P.units = (const uint32_t *)pl->d_iunits.p;
    P.xs = (const IdxStream *)pl->d_ixs.p;
    P.done = (uint32_t *)pl->d_idone.p;
    P.cand = (const uint64_t *)pl->d_cand.p;
    P.win = (const uint8_t *)pl->d_win.p;
    P.nunits = (uint32_t)B.units.size();
    pl->ncand_total = B.units.size();
    return Z_OK;
}

/* the grids of a plan's launches ahead of the whole-stream decode, worked out once per run from the streams
 * that may take part, the records (candidates, chunks or units) lane groups take from a queue, and the
 * tiles the scan visits */
struct InfGrid {
    uint32_t fill;       /* wavefronts that fill the device */
    uint32_t per_stream; /* a wavefront for each stream */
    uint32_t per_group;  /* a lane group for each stream */
    uint32_t groups;     /* a lane group for each record */
    uint32_t scans;      /* a wavefront for each tile */
    InfGrid(uint32_t streams, uint64_t records, uint32_t tiles)
        : fill((uint32_t)g_cus * 4u * INF_WAVES_EU), per_stream(std::max(1u, std::min(streams, fill))),
          per_group((per_stream + INF_PER_WAVE - 1) / INF_PER_WAVE),
          groups((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(fill, (records + INF_PER_WAVE - 1) / INF_PER_WAVE))),
          scans(std::max(1u, std::min(tiles, fill * 4u)))
    {
    }
};

/* the launches of an indexed plan, ahead of k_inflate: the state every run starts from, the write
 * pass, finish */
static ZlibReturn idx_enqueue(zsc_hip_inflate_plan *pl, const void *d_src, void *d_dst, hipStream_t st)
{
    const IidxPlan &P = pl->ip;
    HIP_TRY(hipMemsetAsync(pl->d_nsec.p, 0, 4ull * pl->count, st), return Z_STREAM_ERROR);
    if (pl->idx_fixed) {
        HIP_TRY(hipMemcpyAsync(pl->d_res.p, pl->d_res0.p, sizeof(InfResult) * pl->count, hipMemcpyDeviceToDevice, st),
                return Z_STREAM_ERROR);
        HIP_TRY(hipMemcpyAsync(pl->d_resume.p, pl->d_resume0.p, sizeof(InfResume) * pl->count,
                               hipMemcpyDeviceToDevice, st),
                return Z_STREAM_ERROR);
    }
    if (P.nunits == 0)
        return Z_OK;
    HIP_TRY(hipMemsetAsync(pl->d_idone.p, 0, 4ull * pl->count, st), return Z_STREAM_ERROR);
    HIP_TRY(hipMemcpyAsync(pl->d_sst.p, pl->d_sst0.p, sizeof(IsecStream) * pl->count, hipMemcpyDeviceToDevice, st),
            return Z_STREAM_ERROR);
    HIP_TRY(hipMemcpyAsync(pl->d_q.p, pl->d_q0.p, 16, hipMemcpyDeviceToDevice, st), return Z_STREAM_ERROR);
    const InfGrid g(pl->idx_active, P.nunits, 0);
    hipLaunchKernelGGL(k_idx_write, dim3(g.groups), dim3(64), 0, st, (const uint8_t *)d_src, (uint8_t *)d_dst, P,
                       (InfResult *)pl->d_res.p, (InfResume *)pl->d_resume.p);
    if (pl->idx_active)
        hipLaunchKernelGGL(k_sec_finish, dim3(g.per_group), dim3(64), 0, st, (const uint8_t *)d_src, P.sp,
                           (InfResult *)pl->d_res.p, (InfResume *)pl->d_resume.p);
    return Z_OK;
}

/* the launches of the chunk family ahead of the whole-stream decode (none when no stream is longer than a
 * chunk).  A chunks plan: setup, scan, count, want, retry, resolve, window, write, finish.  A size plan: the
 * same without the window and write passes, with its own count, retry, resolve and finish.  A check plan: a
 * chunks plan's with the check-write pass for the write pass and the values copied out behind finish. */
static void chk_enqueue(zsc_hip_inflate_plan *pl, const void *d_src, void *d_dst, hipStream_t st)
{
    const IchkPlan &P = pl->cp;
    if (P.nactive == 0)
        return;
    const uint8_t *src = (const uint8_t *)d_src;
    InfResult *res = (InfResult *)pl->d_res.p;
    InfResume *resume = (InfResume *)pl->d_resume.p;
    const bool size = pl->kind == INF_SIZE;
    const InfGrid g(P.nactive, pl->ncand_total, P.sp.ntiles);
    hipLaunchKernelGGL(k_chk_setup, dim3(g.per_stream), dim3(64), 0, st, P);
    hipLaunchKernelGGL(k_chk_scan, dim3(g.scans), dim3(64), 0, st, src, P);
    hipLaunchKernelGGL(size ? k_size_count : k_chk_count, dim3(g.groups), dim3(64), 0, st, src, P);
    hipLaunchKernelGGL(k_chk_want, dim3(g.per_stream), dim3(64), 0, st, P);
    hipLaunchKernelGGL(size ? k_size_retry : k_chk_retry, dim3(g.groups), dim3(64), 0, st, src, P);
    hipLaunchKernelGGL(size ? k_size_resolve : k_chk_resolve, dim3(g.per_group), dim3(64), 0, st, src, P);
    if (size) {
        hipLaunchKernelGGL(k_size_finish, dim3(g.per_group), dim3(64), 0, st, src, P, res, resume);
        return;
    }
    hipLaunchKernelGGL(k_chk_window, dim3(std::min<uint32_t>(P.nactive, (uint32_t)g_cus * 4u)), dim3(CHK_WINDOW_THREADS), 0, st, P);
    if (pl->has_rings())
        hipLaunchKernelGGL(k_check_write, dim3(g.groups), dim3(64), 0, st, src, P);
    else
        hipLaunchKernelGGL(k_chk_write, dim3(g.groups), dim3(64), 0, st, src, (uint8_t *)d_dst, P);
    hipLaunchKernelGGL(k_sec_finish, dim3(g.per_group), dim3(64), 0, st, src, P.sp, res, resume);
    if (pl->has_rings())
        hipLaunchKernelGGL(k_check_finish, dim3(g.per_group), dim3(64), 0, st, P, (const InfResume *)resume,
                           (uint32_t *)pl->d_ckval.p);
}

/* the launches of a sections plan, ahead of k_inflate: scan, setup, scan again, then count, resolve, write and
 * finish -- a resync plan's own (which take R), or the sections plan's */
static void sec_enqueue(zsc_hip_inflate_plan *pl, const void *d_src, void *d_dst, hipStream_t st)
{
    const IrsyPlan &R = pl->rp;
    const IsecPlan &P = pl->sp;
    const uint8_t *src = (const uint8_t *)d_src;
    InfResult *res = (InfResult *)pl->d_res.p;
    InfResume *resume = (InfResume *)pl->d_resume.p;
    const InfGrid g(pl->count, pl->ncand_total, P.ntiles);
    hipLaunchKernelGGL(k_sec_scan, dim3(g.scans), dim3(64), 0, st, src, P, 0);
    hipLaunchKernelGGL(k_sec_setup, dim3(g.per_stream), dim3(64), 0, st, P);
    hipLaunchKernelGGL(k_sec_scan, dim3(g.scans), dim3(64), 0, st, src, P, 1);
    if (pl->kind == INF_RESYNC) {
        hipLaunchKernelGGL(k_rsy_count, dim3(g.groups), dim3(64), 0, st, src, R);
        hipLaunchKernelGGL(k_rsy_resolve, dim3(g.per_group), dim3(64), 0, st, src, R);
        hipLaunchKernelGGL(k_rsy_write, dim3(g.groups), dim3(64), 0, st, src, (uint8_t *)d_dst, R);
        hipLaunchKernelGGL(k_rsy_finish, dim3(g.per_group), dim3(64), 0, st, src, R, res, resume);
    } else {
        hipLaunchKernelGGL(k_sec_count, dim3(g.groups), dim3(64), 0, st, src, P);
        hipLaunchKernelGGL(k_sec_resolve, dim3(g.per_group), dim3(64), 0, st, P);
        hipLaunchKernelGGL(k_sec_write, dim3(g.groups), dim3(64), 0, st, src, (uint8_t *)d_dst, P);
        hipLaunchKernelGGL(k_sec_finish, dim3(g.per_group), dim3(64), 0, st, src, P, res, resume);
    }
}

/* the launches of a members plan, all of its run: scan, setup, scan again, claims, count, resolve, write (not in
 * size-only mode), finish and the serial step over the files finish left open */
static void mem_enqueue(zsc_hip_inflate_plan *pl, const void *d_src, void *d_dst, hipStream_t st)
{
    const MemPlan &M = pl->mp;
    const uint8_t *src = (const uint8_t *)d_src;
    InfResult *res = (InfResult *)pl->d_res.p;
    InfResume *resume = (InfResume *)pl->d_resume.p;
    const InfGrid g(pl->count, pl->ncand_total, M.sp.ntiles);
    hipLaunchKernelGGL(k_mem_scan, dim3(g.scans), dim3(64), 0, st, src, M, 0);
    hipLaunchKernelGGL(k_sec_setup, dim3(g.per_stream), dim3(64), 0, st, M.sp);
    hipLaunchKernelGGL(k_mem_scan, dim3(g.scans), dim3(64), 0, st, src, M, 1);
    hipLaunchKernelGGL(k_mem_claims, dim3(g.per_stream), dim3(64), 0, st, src, M);
    hipLaunchKernelGGL(k_mem_count, dim3(g.groups), dim3(64), 0, st, src, M);
    hipLaunchKernelGGL(k_mem_resolve, dim3(g.per_group), dim3(64), 0, st, M);
    if (!M.size_only)
        hipLaunchKernelGGL(k_mem_write, dim3(g.groups), dim3(64), 0, st, src, (uint8_t *)d_dst, M);
    hipLaunchKernelGGL(k_mem_finish, dim3(g.per_group), dim3(64), 0, st, M, res, resume);
    if (M.size_only)
        hipLaunchKernelGGL(k_mem_serial<true>, dim3(g.per_group), dim3(64), 0, st, src, (uint8_t *)nullptr, M, res, resume);
    else
        hipLaunchKernelGGL(k_mem_serial<false>, dim3(g.per_group), dim3(64), 0, st, src, (uint8_t *)d_dst, M, res, resume);
}

/* the launches of a BGZF ranges plan, all of its run: the member jobs, then a result per request */
static ZlibReturn bgr_enqueue(zsc_hip_inflate_plan *pl, const void *d_src, void *d_dst, hipStream_t st)
{
    const BgrPlan &B = pl->bp;
    HIP_TRY(hipMemsetAsync(pl->d_bbad.p, 0, 4ull * pl->count, st), return Z_STREAM_ERROR);
    HIP_TRY(hipMemsetAsync(pl->d_bq.p, 0, 16, st), return Z_STREAM_ERROR);
    if (B.njobs)
        hipLaunchKernelGGL(k_bgr_range, dim3(pl->bgr_waves), dim3(64), 0, st, (const uint8_t *)d_src, (uint8_t *)d_dst,
                           (uint8_t *)pl->d_bstage.p, B);
    hipLaunchKernelGGL(k_bgr_finish, dim3(std::max(1u, std::min((pl->count + 63u) / 64u, (uint32_t)g_cus * 8u))),
                       dim3(64), 0, st, B, (const InfResult *)pl->d_bres0.p, (InfResult *)pl->d_res.p);
    return Z_OK;
}

/* the whole-stream decode of what the launches above left: the first launch of a run, and every relaunch of
 * _results.  A check plan's first launch decodes into the rings; its relaunches are the size decode. */
static void inflate_launch(zsc_hip_inflate_plan *pl, const void *d_src, void *d_dst, hipStream_t st, bool first)
{
    const uint8_t *src = (const uint8_t *)d_src;
    const ZdInfItem *items = (const ZdInfItem *)pl->d_items.p;
    const uint32_t *order = (const uint32_t *)pl->d_order.p;
    InfResult *res = (InfResult *)pl->d_res.p;
    InfResume *resume = (InfResume *)pl->d_resume.p;
    uint32_t *pending = (uint32_t *)pl->d_pending.p;
    if (pl->has_rings() && first)
        hipLaunchKernelGGL(k_inflate_check, dim3(pl->check_waves), dim3(64), 0, st, src, (uint8_t *)pl->d_rings.p, items,
                           order, res, resume, (uint32_t *)pl->d_ckval.p, pending, pl->window_bits, pl->count);
    else if (pl->writes_nothing())
        hipLaunchKernelGGL(k_inflate_size, dim3(inflate_grid(pl->count)), dim3(64), 0, st, src, items, order, res,
                           resume, pending, pl->window_bits, pl->count);
    else if (pl->dict_on)
        hipLaunchKernelGGL(k_inflate_dict, dim3(inflate_grid(pl->count)), dim3(64), 0, st, src, (uint8_t *)d_dst, items,
                           order, res, resume, pending, pl->window_bits, pl->count, (const uint8_t *)pl->d_dict_img.p,
                           (const ZdInfDict *)pl->d_dict_tab.p, (const uint32_t *)pl->d_dict_of.p);
    else
        hipLaunchKernelGGL(k_inflate, dim3(inflate_grid(pl->count)), dim3(64), 0, st, src, (uint8_t *)d_dst, items, order,
                           res, resume, pending, pl->window_bits, pl->count);
}

extern "C" ZlibReturn zsc_hip_inflate_plan_run(zsc_hip_inflate_plan *pl, const void *d_src,
                                               void *d_dst, void *hip_stream)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    hipStream_t st = (hipStream_t)hip_stream;
    if (pl->count == 0) {
        pl->last_stream = st;
        return Z_OK;
    }
    (void)hipGetLastError(); /* (see zsc_hip_deflate_plan_run) */
    work_chain(pl->ran, st); /* (the same: one set of scratch, and a pack reads the results this run writes) */
    work_order(pl->pack.work, st);
    pl->last_stream = st;
    pl->last_src = d_src;
    pl->last_dst = d_dst;
    HIP_TRY(hipMemsetAsync(pl->d_resume.p, 0, sizeof(InfResume) * pl->count, st), return Z_STREAM_ERROR);
    HIP_TRY(hipMemsetAsync(pl->d_pending.p, 0, 8, st), return Z_STREAM_ERROR); /* [0] streams to relaunch, [1] the queue */
    if (pl->has_sections() || pl->kind == INF_MEMBERS)
        HIP_TRY(hipMemsetAsync(pl->d_scount.p, 0, 4ull * pl->count, st), return Z_STREAM_ERROR);
    if (pl->kind == INF_MEMBERS)
        HIP_TRY(hipMemsetAsync(pl->d_mfiles.p, 0, sizeof(MemFile) * pl->count, st), return Z_STREAM_ERROR);
    if (pl->has_sections() || pl->has_chunks() || pl->kind == INF_MEMBERS) { /* (an indexed plan sets these up itself) */
        HIP_TRY(hipMemsetAsync(pl->d_nsec.p, 0, 4ull * pl->count, st), return Z_STREAM_ERROR);
        HIP_TRY(hipMemsetAsync(pl->d_q.p, 0, 16, st), return Z_STREAM_ERROR);
    }
    if (pl->writes_nothing()) {
        /* nothing is written through d_dst: it is not looked at */
        pl->last_dst = nullptr;
        pl->size_ran = true;
    }
    if (pl->has_rings())
        HIP_TRY(hipMemsetAsync(pl->d_ckval.p, 0, 4ull * pl->count, st), return Z_STREAM_ERROR);
    (void)hipEventRecord(pl->ev0, st);
    if (pl->has_sections())
        sec_enqueue(pl, d_src, d_dst, st);
    if (pl->kind == INF_CHUNKS)
        pl->idx_recs.clear();
    if (pl->has_chunks())
        chk_enqueue(pl, d_src, d_dst, st);
    if (pl->kind == INF_INDEXED && idx_enqueue(pl, d_src, d_dst, st) != Z_OK)
        return Z_STREAM_ERROR;
    if (pl->kind == INF_BGZF_RANGES) {
        if (bgr_enqueue(pl, d_src, d_dst, st) != Z_OK)
            return Z_STREAM_ERROR;
    } else if (pl->kind == INF_MEMBERS)
        mem_enqueue(pl, d_src, d_dst, st); /* (its serial step is its whole-stream decode: nothing is relaunched) */
    else
        inflate_launch(pl, d_src, d_dst, st, true);
    (void)hipEventRecord(pl->ev1, st);
    pl->timed = true;
    work_note(pl->ran, st);
    HIP_TRY(hipGetLastError(), return Z_STREAM_ERROR);
    return Z_OK;
}

extern "C" ZlibReturn zsc_hip_inflate_plan_results(zsc_hip_inflate_plan *pl, U32 *dest_lens,
                                                   U32 *consumed, I32 *statuses, float *kernel_ms)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    HIP_TRY(inflate_wait_all(pl), return Z_STREAM_ERROR);
    /* streams that hit a data error and found a flush marker behind it (inflateSync) are
     * inflated again from there, as zsc_uncompress's loop does (src/zsc_uncompr.c:104-125);
     * every round consumes at least the marker, so this ends */
    for (uint32_t round = 0; pl->count && (pl->last_dst || pl->size_ran); round++) {
        uint32_t pending = 0;
        HIP_TRY(hipMemcpy(&pending, pl->d_pending.p, 4, hipMemcpyDeviceToHost), return Z_STREAM_ERROR);
        if (pending == 0 || round > (1u << 30))
            break;
        HIP_TRY(hipMemsetAsync(pl->d_pending.p, 0, 8, pl->last_stream), return Z_STREAM_ERROR);
        inflate_launch(pl, pl->last_src, pl->last_dst, pl->last_stream, false);
        HIP_TRY(hipStreamSynchronize(pl->last_stream), return Z_STREAM_ERROR);
    }
    std::vector<InfResult> res(pl->count);
    if (pl->count)
        HIP_TRY(hipMemcpy(res.data(), pl->d_res.p, sizeof(InfResult) * pl->count,
                          hipMemcpyDeviceToHost),
                return Z_STREAM_ERROR);
    for (uint32_t i = 0; i < pl->count; i++) {
        if (dest_lens)
            dest_lens[i] = res[i].out_len;
        if (consumed)
            consumed[i] = res[i].consumed;
        if (statuses)
            statuses[i] = res[i].status;
        if (res[i].status == Z_DATA_ERROR && getenv("ZSC_HIP_DEBUG"))
            fprintf(stderr, "zsc_hip: stream %u rejected at inflate.h:%u\n", i, res[i].pad);
    }
    if (kernel_ms) {
        *kernel_ms = 0.f;
        if (pl->timed)
            (void)hipEventElapsedTime(kernel_ms, pl->ev0, pl->ev1);
    }
    return Z_OK;
}

extern "C" void zsc_hip_inflate_plan_destroy(zsc_hip_inflate_plan *pl)
{
    DeviceScope scope;
    if (!pl)
        return;
    (void)inflate_wait_all(pl); /* the blocks go back to the cache: the runs and the packs are waited for */
    inflate_plan_release(pl);
    pack_release(pl->pack, &pl->scratch_bytes);
    work_release(pl->ran);
    if (pl->ev0)
        (void)hipEventDestroy(pl->ev0);
    if (pl->ev1)
        (void)hipEventDestroy(pl->ev1);
    delete pl;
}

extern "C" ZlibReturn zsc_hip_inflate_plan_sections(zsc_hip_inflate_plan *pl, U32 *sections)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    ZSC_ASSERT(sections != Z_NULL);
    if (!pl->counts_pieces() || !(pl->last_dst || pl->size_ran) ||
        pl->count == 0) {
        for (uint32_t i = 0; i < pl->count; i++)
            sections[i] = 0;
        return Z_OK;
    }
    HIP_TRY(inflate_wait_all(pl), return Z_STREAM_ERROR);
    HIP_TRY(hipMemcpy(sections, pl->d_nsec.p, 4ull * pl->count, hipMemcpyDeviceToHost), return Z_STREAM_ERROR);
    return Z_OK;
}

extern "C" ZlibReturn zsc_hip_inflate_plan_members(zsc_hip_inflate_plan *pl, U32 *members, U32 *claimed)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    if (pl->kind != INF_MEMBERS)
        return Z_STREAM_ERROR;
    std::vector<MemFile> mf(pl->count, MemFile{0, 0, 0, 0});
    if ((pl->last_dst || pl->size_ran) && pl->count) {
        HIP_TRY(inflate_wait_all(pl), return Z_STREAM_ERROR);
        HIP_TRY(hipMemcpy(mf.data(), pl->d_mfiles.p, sizeof(MemFile) * pl->count, hipMemcpyDeviceToHost),
                return Z_STREAM_ERROR);
    }
    for (uint32_t i = 0; i < pl->count; i++) {
        if (members)
            members[i] = mf[i].members;
        if (claimed)
            claimed[i] = mf[i].claimed;
    }
    return Z_OK;
}

extern "C" ZlibReturn zsc_hip_inflate_plan_data_errors(zsc_hip_inflate_plan *pl, U32 *errors)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    ZSC_ASSERT(errors != Z_NULL);
    if (!(pl->last_dst || pl->size_ran) || pl->count == 0) {
        for (uint32_t i = 0; i < pl->count; i++)
            errors[i] = 0;
        return Z_OK;
    }
    HIP_TRY(inflate_wait_all(pl), return Z_STREAM_ERROR);
    std::vector<InfResume> rs(pl->count);
    HIP_TRY(hipMemcpy(rs.data(), pl->d_resume.p, sizeof(InfResume) * pl->count, hipMemcpyDeviceToHost),
            return Z_STREAM_ERROR);
    for (uint32_t i = 0; i < pl->count; i++)
        errors[i] = rs[i].errors;
    return Z_OK;
}

extern "C" ZlibReturn zsc_hip_inflate_plan_index_enable(zsc_hip_inflate_plan *pl, I32 enable)
{
    ZSC_ASSERT(pl != Z_NULL);
    if (pl->kind != INF_CHUNKS)
        return Z_STREAM_ERROR;
    pl->cp.keep_index = enable ? 1u : 0u;
    return Z_OK;
}

/* the records of stream `stream` of the last run (kept until the next one); Z_DATA_ERROR: no index */
static ZlibReturn idx_records(zsc_hip_inflate_plan *pl, U32 stream, const std::vector<ZidxRec> **recs,
                              uint64_t *wbytes)
{
    if (pl->kind != INF_CHUNKS || !pl->cp.keep_index || stream >= pl->count || !pl->last_dst)
        return Z_STREAM_ERROR;
    auto hit = pl->idx_recs.find(stream);
    if (hit == pl->idx_recs.end()) {
        HIP_TRY(inflate_wait_all(pl), return Z_STREAM_ERROR);
        uint32_t n = 0;
        HIP_TRY(hipMemcpy(&n, (const uint32_t *)pl->d_nsec.p + stream, 4, hipMemcpyDeviceToHost), return Z_STREAM_ERROR);
        std::vector<ZidxRec> r(n);
        uint64_t total = 0;
        if (n) {
            DevBuf d_recs, d_total;
            bool ok = d_recs.ensure(sizeof(ZidxRec) * n) && d_total.ensure(8);
            if (ok) {
                hipLaunchKernelGGL(k_idx_records, dim3(1), dim3(IDX_REC_THREADS), 0, pl->last_stream, pl->cp, stream, n,
                                   (ZidxRec *)d_recs.p, (uint64_t *)d_total.p);
                ok = hipStreamSynchronize(pl->last_stream) == hipSuccess &&
                     hipMemcpy(r.data(), d_recs.p, sizeof(ZidxRec) * n, hipMemcpyDeviceToHost) == hipSuccess &&
                     hipMemcpy(&total, d_total.p, 8, hipMemcpyDeviceToHost) == hipSuccess;
            }
            d_recs.release();
            d_total.release();
            if (!ok)
                return Z_MEM_ERROR;
        }
        hit = pl->idx_recs.emplace(stream, std::make_pair(std::move(r), total)).first;
    }
    *recs = &hit->second.first;
    *wbytes = hit->second.second;
    return (*recs)->empty() ? Z_DATA_ERROR : Z_OK;
}

extern "C" ZlibReturn zsc_hip_inflate_plan_index_size(zsc_hip_inflate_plan *pl, U32 stream, uint64_t *bytes)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    ZSC_ASSERT(bytes != Z_NULL);
    *bytes = 0;
    const std::vector<ZidxRec> *recs = nullptr;
    uint64_t wbytes = 0;
    const ZlibReturn rc = idx_records(pl, stream, &recs, &wbytes);
    if (rc == Z_OK)
        *bytes = zidx_blob_bytes((uint32_t)recs->size(), wbytes);
    return rc;
}

extern "C" ZlibReturn zsc_hip_inflate_plan_index_export(zsc_hip_inflate_plan *pl, U32 stream, U8 *blob, uint64_t cap,
                                                        uint64_t *len)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    ZSC_ASSERT(len != Z_NULL);
    *len = 0;
    const std::vector<ZidxRec> *recs = nullptr;
    uint64_t wbytes = 0;
    const ZlibReturn rc = idx_records(pl, stream, &recs, &wbytes);
    if (rc != Z_OK)
        return rc;
    const uint32_t n = (uint32_t)recs->size();
    const uint64_t bytes = zidx_blob_bytes(n, wbytes);
    *len = bytes;
    if (cap < bytes || blob == Z_NULL)
        return Z_BUF_ERROR;
    IsecStream S;
    InfResult res;
    HIP_TRY(hipMemcpy(&S, (const IsecStream *)pl->d_sst.p + stream, sizeof S, hipMemcpyDeviceToHost), return Z_STREAM_ERROR);
    HIP_TRY(hipMemcpy(&res, (const InfResult *)pl->d_res.p + stream, sizeof res, hipMemcpyDeviceToHost), return Z_STREAM_ERROR);
    if (wbytes) {
        /* the windows, gathered on the device, in one copy */
        DevBuf d_recs, d_wins;
        bool ok = d_recs.ensure(sizeof(ZidxRec) * n) && d_wins.ensure(wbytes) &&
                  hipMemcpy(d_recs.p, recs->data(), sizeof(ZidxRec) * n, hipMemcpyHostToDevice) == hipSuccess;
        if (ok) {
            const uint32_t blocks = std::max(1u, std::min(n, (uint32_t)g_cus * 8u));
            hipLaunchKernelGGL(k_idx_gather, dim3(blocks), dim3(IDX_GATHER_THREADS), 0, pl->last_stream, pl->cp, stream, n,
                               (const ZidxRec *)d_recs.p, (uint8_t *)d_wins.p);
            ok = hipStreamSynchronize(pl->last_stream) == hipSuccess &&
                 hipMemcpy(blob + zidx_blob_bytes(n, 0), d_wins.p, wbytes, hipMemcpyDeviceToHost) == hipSuccess;
        }
        d_recs.release();
        d_wins.release();
        if (!ok)
            return Z_MEM_ERROR;
    }
    ZidxInfo h;
    h.window_bits = pl->window_bits;
    h.kind = pl->window_bits < 0 ? 0u : (S.head & 1u) ? 2u : 1u;
    h.head = S.head;
    h.chunk_bytes = pl->cp.chunk_bytes;
    h.consumed = res.consumed;
    h.total = S.total;
    h.trailer = S.trailer;
    h.npoints = n;
    zidx_write_head(blob, &h, recs->data());
    zidx_seal(blob, bytes);
    return Z_OK;
}

extern "C" ZlibReturn zsc_hip_index_validate(const U8 *blob, uint64_t len)
{
    return zidx_validate(blob, len, nullptr) ? Z_OK : Z_DATA_ERROR;
}

extern "C" ZlibReturn zsc_hip_index_info(const U8 *blob, uint64_t len, zsc_hip_index_header *info)
{
    ZSC_ASSERT(info != Z_NULL);
    ZidxInfo h;
    if (!zidx_validate(blob, len, &h))
        return Z_DATA_ERROR;
    info->window_bits = h.window_bits;
    info->wrapper = h.kind;
    info->gzip = h.head & 1u;
    info->dist_limit = 1u << ((h.head >> 8) & 31u);
    info->chunk_bytes = h.chunk_bytes;
    info->consumed = h.consumed;
    info->total_out = h.total;
    info->trailer_offset = h.trailer;
    info->points = h.npoints;
    return Z_OK;
}

extern "C" ZlibReturn zsc_hip_index_range(const U8 *blob, uint64_t len, uint64_t out_begin, uint64_t out_len,
                                          U32 *first_piece, U32 *piece_count, U32 *piece_begin, U32 *piece_len)
{
    ZidxInfo h;
    if (!zidx_validate(blob, len, &h))
        return Z_DATA_ERROR;
    U32 f = 0, c = 0, b = 0, l = 0;
    if (!zidx_range(blob, &h, out_begin, out_len, &f, &c, &b, &l))
        return Z_STREAM_ERROR;
    if (first_piece)
        *first_piece = f;
    if (piece_count)
        *piece_count = c;
    if (piece_begin)
        *piece_begin = b;
    if (piece_len)
        *piece_len = l;
    return Z_OK;
}

extern "C" uint64_t zsc_hip_inflate_plan_scratch_bytes(const zsc_hip_inflate_plan *pl)
{
    return pl ? pl->scratch_bytes : 0;
}

/* ---- preset dictionaries of a plain inflate plan (inflate.h, InfDict) ---------------------------- */

extern "C" ZlibReturn zsc_hip_inflate_plan_dict_enable(zsc_hip_inflate_plan *pl, U32 ndicts, const U8 *const *dicts,
                                                       const U32 *dict_lens, const U32 *stream_dict)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    if (pl->kind != INF_PLAIN || (ndicts && (dicts == Z_NULL || dict_lens == Z_NULL)))
        return Z_STREAM_ERROR;
    std::vector<U32> of(std::max(1u, pl->count), ZSC_HIP_NO_DICT);
    for (uint32_t i = 0; i < pl->count; i++) {
        of[i] = stream_dict ? stream_dict[i] : 0u;
        if (of[i] != ZSC_HIP_NO_DICT && of[i] >= ndicts)
            return Z_STREAM_ERROR;
    }
    /* the whole dictionaries go up once, for their ids; the plan keeps the images (k_dict_setup) */
    std::vector<uint64_t> at(std::max(1u, ndicts), 0);
    std::vector<ZdInfDict> tab(std::max(1u, ndicts), ZdInfDict{0u, 0u});
    uint64_t total = 0;
    for (uint32_t d = 0; d < ndicts; d++) {
        if (dict_lens[d] && dicts[d] == Z_NULL)
            return Z_STREAM_ERROR;
        at[d] = total;
        tab[d].len = dict_lens[d];
        total += ((uint64_t)dict_lens[d] + 15u) & ~15ull;
    }
    DevBuf whole, d_at, img, d_tab, d_of;
    const uint64_t img_bytes = (uint64_t)INF_WIN * std::max(1u, ndicts);
    bool ok = whole.ensure(total + 16) && d_at.ensure(8ull * at.size()) && img.ensure(img_bytes) &&
              d_tab.ensure(sizeof(ZdInfDict) * tab.size()) && d_of.ensure(4ull * of.size());
    ok = ok && hipMemset(img.p, 0, img_bytes) == hipSuccess &&
         hipMemcpy(d_at.p, at.data(), 8ull * at.size(), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d_tab.p, tab.data(), sizeof(ZdInfDict) * tab.size(), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d_of.p, of.data(), 4ull * of.size(), hipMemcpyHostToDevice) == hipSuccess;
    for (uint32_t d = 0; d < ndicts && ok; d++)
        if (dict_lens[d])
            ok = hipMemcpy((uint8_t *)whole.p + at[d], dicts[d], dict_lens[d], hipMemcpyHostToDevice) == hipSuccess;
    if (ok && ndicts) {
        hipLaunchKernelGGL(k_dict_setup, dim3(ndicts), dim3(64), 0, nullptr, (const uint8_t *)whole.p,
                           (const uint64_t *)d_at.p, (ZdInfDict *)d_tab.p, (uint8_t *)img.p);
        ok = hipStreamSynchronize(nullptr) == hipSuccess &&
             hipMemcpy(tab.data(), d_tab.p, sizeof(ZdInfDict) * ndicts, hipMemcpyDeviceToHost) == hipSuccess;
    }
    whole.release();
    d_at.release();
    if (!ok) {
        img.release();
        d_tab.release();
        d_of.release();
        return Z_MEM_ERROR;
    }
    /* the set the plan had, if any, is replaced (its last run may still be reading it) */
    (void)inflate_wait_all(pl);
    std::swap(static_cast<DevBuf &>(pl->d_dict_img), img);
    std::swap(static_cast<DevBuf &>(pl->d_dict_tab), d_tab);
    std::swap(static_cast<DevBuf &>(pl->d_dict_of), d_of);
    img.release();
    d_tab.release();
    d_of.release();
    pl->scratch_bytes -= pl->dict_scratch;
    pl->dict_scratch = img_bytes + sizeof(ZdInfDict) * tab.size() + 4ull * of.size();
    pl->scratch_bytes += pl->dict_scratch;
    pl->dict_ids.resize(ndicts);
    for (uint32_t d = 0; d < ndicts; d++)
        pl->dict_ids[d] = tab[d].id;
    pl->dict_on = true;
    return Z_OK;
}

extern "C" ZlibReturn zsc_hip_inflate_plan_dict_ids(zsc_hip_inflate_plan *pl, U32 *ids)
{
    ZSC_ASSERT(pl != Z_NULL);
    if (!pl->dict_on)
        return Z_STREAM_ERROR;
    ZSC_ASSERT(ids != Z_NULL || pl->dict_ids.empty());
    for (size_t d = 0; d < pl->dict_ids.size(); d++)
        ids[d] = pl->dict_ids[d];
    return Z_OK;
}

/* host-pointer batch: lay the streams out one behind the other, make the plan (create(&plan, source offsets,
 * destination offsets)), stage the sources through one device buffer, run, fetch the results, copy the
 * outputs back (dests; null for a plan that writes nothing) and, of a check plan, the values, of a members plan
 * the member counts if asked for; tear down */
template <class Create>
static ZlibReturn uncompress_batch_host(U32 count, const U8 *const *sources, U32 *source_lens, U8 *const *dests,
                                        U32 *dest_lens, I32 *statuses, U32 *check_values, Create create,
                                        U32 *members = Z_NULL)
{
    DeviceScope scope;
    ZSC_ASSERT(sources != Z_NULL);
    ZSC_ASSERT(source_lens != Z_NULL);
    ZSC_ASSERT(dest_lens != Z_NULL);
    if (count == 0)
        return Z_OK;
    if (zsc_hip_init(-1) != Z_OK)
        return Z_STREAM_ERROR;
    std::vector<uint64_t> so(count), dof(count);
    uint64_t sb = 0, db = 0;
    for (U32 i = 0; i < count; i++) {
        so[i] = sb;
        dof[i] = db;
        sb += ((uint64_t)source_lens[i] + 64u + 15u) & ~15ull;
        db += ((uint64_t)dest_lens[i] + 64u + 15u) & ~15ull;
    }
    zsc_hip_inflate_plan *pl = nullptr;
    ZlibReturn rc = create(&pl, so.data(), dof.data());
    if (rc != Z_OK)
        return rc;
    DevBuf d_src, d_dst;
    if (!d_src.ensure(sb + 64) || (dests && !d_dst.ensure(db + 64)))
        rc = Z_MEM_ERROR;
    for (U32 i = 0; i < count && rc == Z_OK; i++) {
        ZSC_ASSERT(sources[i] != Z_NULL);
        if (source_lens[i] && hipMemcpy((uint8_t *)d_src.p + so[i], sources[i], source_lens[i],
                                        hipMemcpyHostToDevice) != hipSuccess)
            rc = Z_STREAM_ERROR;
    }
    std::vector<U32> outl(count), used(count), vals(count);
    std::vector<I32> stat(count);
    if (rc == Z_OK)
        rc = zsc_hip_inflate_plan_run(pl, d_src.p, d_dst.p, nullptr);
    if (rc == Z_OK)
        rc = zsc_hip_inflate_plan_results(pl, outl.data(), used.data(), stat.data(), nullptr);
    if (rc == Z_OK && pl->has_rings())
        rc = zsc_hip_inflate_plan_check_values(pl, vals.data());
    if (rc == Z_OK && members)
        rc = zsc_hip_inflate_plan_members(pl, members, Z_NULL);
    for (U32 i = 0; i < count && rc == Z_OK; i++) {
        if (dests) {
            ZSC_ASSERT(dests[i] != Z_NULL);
            if (outl[i] && hipMemcpy(dests[i], (uint8_t *)d_dst.p + dof[i], outl[i],
                                     hipMemcpyDeviceToHost) != hipSuccess)
                rc = Z_STREAM_ERROR;
        }
        dest_lens[i] = outl[i];
        source_lens[i] = used[i];
        if (statuses)
            statuses[i] = stat[i];
        if (check_values)
            check_values[i] = vals[i];
    }
    d_src.release();
    d_dst.release();
    zsc_hip_inflate_plan_destroy(pl);
    return rc;
}

/* the batches that write their outputs: a plain (0), sections (1), chunks (2), resync (3) or indexed (4) plan */
static ZlibReturn uncompress_batch_impl(U32 count, const U8 *const *sources, U32 *source_lens, U8 *const *dests,
                                        U32 *dest_lens, I32 *statuses, I32 window_bits, int kind,
                                        const U8 *const *indexes = Z_NULL, const uint64_t *index_lens = Z_NULL)
{
    ZSC_ASSERT(dests != Z_NULL);
    return uncompress_batch_host(
        count, sources, source_lens, dests, dest_lens, statuses, Z_NULL,
        [&](zsc_hip_inflate_plan **pl, const uint64_t *so, const uint64_t *dof) {
            return kind == 1 ? zsc_hip_inflate_plan_create_sections(pl, count, source_lens, so, dest_lens, dof,
                                                                    window_bits)
                   : kind == 2 ? zsc_hip_inflate_plan_create_chunks(pl, count, source_lens, so, dest_lens, dof,
                                                                    window_bits, 0)
                   : kind == 3 ? zsc_hip_inflate_plan_create_resync(pl, count, source_lens, so, dest_lens, dof,
                                                                    window_bits)
                   : kind == 4 ? zsc_hip_inflate_plan_create_indexed(pl, count, source_lens, so, dest_lens, dof,
                                                                     window_bits, indexes, index_lens, Z_NULL, Z_NULL)
                               : zsc_hip_inflate_plan_create(pl, count, source_lens, so, dest_lens, dof, window_bits);
        });
}

/* host-pointer batch: stage through one pair of device buffers */
extern "C" ZlibReturn zsc_hip_uncompress_batch(U32 count, const U8 *const *sources,
                                               U32 *source_lens, U8 *const *dests,
                                               U32 *dest_lens, I32 *statuses, I32 window_bits)
{
    return uncompress_batch_impl(count, sources, source_lens, dests, dest_lens, statuses, window_bits, 0);
}

extern "C" ZlibReturn zsc_hip_uncompress_sections_batch(U32 count, const U8 *const *sources,
                                                        U32 *source_lens, U8 *const *dests,
                                                        U32 *dest_lens, I32 *statuses, I32 window_bits)
{
    return uncompress_batch_impl(count, sources, source_lens, dests, dest_lens, statuses, window_bits, 1);
}

extern "C" ZlibReturn zsc_hip_uncompress_chunks_batch(U32 count, const U8 *const *sources, U32 *source_lens,
                                                      U8 *const *dests, U32 *dest_lens, I32 *statuses,
                                                      I32 window_bits)
{
    return uncompress_batch_impl(count, sources, source_lens, dests, dest_lens, statuses, window_bits, 2);
}

extern "C" ZlibReturn zsc_hip_uncompress_resync_batch(U32 count, const U8 *const *sources, U32 *source_lens,
                                                      U8 *const *dests, U32 *dest_lens, I32 *statuses,
                                                      I32 window_bits)
{
    return uncompress_batch_impl(count, sources, source_lens, dests, dest_lens, statuses, window_bits, 3);
}

extern "C" ZlibReturn zsc_hip_uncompress_indexed_batch(U32 count, const U8 *const *sources, U32 *source_lens,
                                                       U8 *const *dests, U32 *dest_lens, I32 *statuses,
                                                       I32 window_bits, const U8 *const *indexes,
                                                       const uint64_t *index_lens)
{
    return uncompress_batch_impl(count, sources, source_lens, dests, dest_lens, statuses, window_bits, 4, indexes,
                                 index_lens);
}

/* host-pointer batch through a plain plan with preset dictionaries */
extern "C" ZlibReturn zsc_hip_uncompress_dict_batch(U32 count, const U8 *const *sources, U32 *source_lens,
                                                    U8 *const *dests, U32 *dest_lens, I32 *statuses, I32 window_bits,
                                                    U32 ndicts, const U8 *const *dicts, const U32 *dict_lens,
                                                    const U32 *stream_dict)
{
    ZSC_ASSERT(dests != Z_NULL);
    return uncompress_batch_host(
        count, sources, source_lens, dests, dest_lens, statuses, Z_NULL,
        [&](zsc_hip_inflate_plan **pl, const uint64_t *so, const uint64_t *dof) {
            ZlibReturn rc = zsc_hip_inflate_plan_create(pl, count, source_lens, so, dest_lens, dof, window_bits);
            if (rc == Z_OK) {
                rc = zsc_hip_inflate_plan_dict_enable(*pl, ndicts, dicts, dict_lens, stream_dict);
                if (rc != Z_OK)
                    inflate_plan_fail(pl, rc);
            }
            return rc;
        });
}

/* host-pointer batch through a size plan (default chunk_bytes): the sources staged in one device buffer */
extern "C" ZlibReturn zsc_hip_uncompress_sizes_batch(U32 count, const U8 *const *sources, U32 *source_lens,
                                                     U32 *dest_lens, I32 *statuses, I32 window_bits)
{
    return uncompress_batch_host(count, sources, source_lens, Z_NULL, dest_lens, statuses, Z_NULL,
                                 [&](zsc_hip_inflate_plan **pl, const uint64_t *so, const uint64_t *) {
                                     return zsc_hip_inflate_plan_create_size(pl, count, source_lens, so, dest_lens,
                                                                             window_bits, 0);
                                 });
}

/* host-pointer batch through a members plan: every source a multi-member gzip file */
extern "C" ZlibReturn zsc_hip_uncompress_members_batch(U32 count, const U8 *const *sources, U32 *source_lens,
                                                       U8 *const *dests, U32 *dest_lens, I32 *statuses,
                                                       I32 window_bits, U32 *members)
{
    ZSC_ASSERT(dests != Z_NULL);
    return uncompress_batch_host(
        count, sources, source_lens, dests, dest_lens, statuses, Z_NULL,
        [&](zsc_hip_inflate_plan **pl, const uint64_t *so, const uint64_t *dof) {
            return zsc_hip_inflate_plan_create_members(pl, count, source_lens, so, dest_lens, dof, window_bits, 0);
        },
        members);
}

extern "C" ZlibReturn zsc_hip_inflate_plan_check_values(zsc_hip_inflate_plan *pl, U32 *values)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    ZSC_ASSERT(values != Z_NULL);
    if (!pl->has_rings() || !pl->size_ran)
        return Z_STREAM_ERROR;
    if (pl->count == 0)
        return Z_OK;
    /* (the statuses are final once _results has relaunched what had to be) */
    std::vector<I32> stat(pl->count);
    ZlibReturn rc = zsc_hip_inflate_plan_results(pl, nullptr, nullptr, stat.data(), nullptr);
    if (rc != Z_OK)
        return rc;
    HIP_TRY(hipMemcpy(values, pl->d_ckval.p, 4ull * pl->count, hipMemcpyDeviceToHost), return Z_STREAM_ERROR);
    for (uint32_t i = 0; i < pl->count; i++)
        if (stat[i] != Z_OK)
            values[i] = 0;
    return Z_OK;
}

/* host-pointer batch through a check plan (default chunk_bytes): the sources staged in one device buffer */
extern "C" ZlibReturn zsc_hip_uncompress_check_batch(U32 count, const U8 *const *sources, U32 *source_lens,
                                                     U32 *dest_lens, I32 *statuses, U32 *check_values,
                                                     I32 window_bits)
{
    return uncompress_batch_host(count, sources, source_lens, Z_NULL, dest_lens, statuses, check_values,
                                 [&](zsc_hip_inflate_plan **pl, const uint64_t *so, const uint64_t *) {
                                     return zsc_hip_inflate_plan_create_check(pl, count, source_lens, so, dest_lens,
                                                                              window_bits, 0);
                                 });
}

/* ---- packing an inflate plan's outputs, unpacking, and the host images (pack.h) ----------------- */

extern "C" ZlibReturn zsc_hip_inflate_plan_pack_enable(zsc_hip_inflate_plan *pl, U32 align)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    if (!pack_align_ok(align) || pl->writes_nothing()) /* (a size plan has no outputs to pack) */
        return Z_STREAM_ERROR;
    if (pl->pack.on) {
        pack_set_align(pl->pack, align);
        return Z_OK;
    }
    /* where the outputs go and how long they get at the most: the plan's own items */
    std::vector<ZdInfItem> items(pl->count);
    if (pl->count)
        HIP_TRY(hipMemcpy(items.data(), pl->d_items.p, sizeof(ZdInfItem) * pl->count, hipMemcpyDeviceToHost),
                return Z_STREAM_ERROR);
    std::vector<uint64_t> slots(pl->count);
    std::vector<U32> caps(pl->count);
    for (uint32_t i = 0; i < pl->count; i++) {
        slots[i] = items[i].dst_off;
        caps[i] = items[i].dst_cap;
    }
    return pack_setup(pl->pack, pl->count, align, slots.data(), caps.data(), &pl->scratch_bytes);
}

extern "C" ZlibReturn zsc_hip_inflate_plan_pack(zsc_hip_inflate_plan *pl, const void *d_output, void *d_packed,
                                                uint64_t packed_cap, void *hip_stream)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    /* the bytes written, whatever the status: what a damaged stream gave is kept */
    const PkLens lens = {(const uint32_t *)pl->d_res.p, 4u, 1u, PK_NO_STATUS};
    /* (of a ranges plan the bytes of the Z_OK requests: another status wrote nothing it stands for) */
    const PkLens ok_lens = {(const uint32_t *)pl->d_res.p, 4u, 1u, 0u};
    return pack_enqueue(pl->pack, pl->kind == INF_BGZF_RANGES ? ok_lens : lens, d_output, d_packed, packed_cap,
                        (hipStream_t)hip_stream);
}

extern "C" ZlibReturn zsc_hip_inflate_plan_pack_results(zsc_hip_inflate_plan *pl, uint64_t *offsets, uint64_t *total,
                                                        float *ms)
{
    DeviceScope scope;
    ZSC_ASSERT(pl != Z_NULL);
    return pack_fetch(pl->pack, offsets, total, ms);
}

namespace {
/* the device arrays of zsc_hip_unpack calls whose launch may still be running */
struct UnpackPending {
    hipEvent_t done;
    DevBuf table, lens, slots;
};
std::mutex g_unpack_mu;
std::vector<UnpackPending> g_unpack_pending;

void unpack_reap(bool wait)
{
    std::lock_guard<std::mutex> lock(g_unpack_mu);
    for (size_t k = 0; k < g_unpack_pending.size();) {
        UnpackPending &u = g_unpack_pending[k];
        if (wait)
            (void)hipEventSynchronize(u.done);
        else if (hipEventQuery(u.done) != hipSuccess) {
            (void)hipGetLastError();
            k++;
            continue;
        }
        (void)hipEventDestroy(u.done);
        u.table.release();
        u.lens.release();
        u.slots.release();
        g_unpack_pending[k] = g_unpack_pending.back();
        g_unpack_pending.pop_back();
    }
}
} // namespace

extern "C" ZlibReturn zsc_hip_unpack(U32 count, const void *d_packed, const uint64_t *packed_offsets, const U32 *lens,
                                     void *d_dst, const uint64_t *dst_offsets, void *hip_stream)
{
    DeviceScope scope;
    if (zsc_hip_init(-1) != Z_OK)
        return Z_STREAM_ERROR;
    unpack_reap(false);
    if (count == 0)
        return Z_OK;
    ZSC_ASSERT(packed_offsets != Z_NULL);
    ZSC_ASSERT(lens != Z_NULL);
    ZSC_ASSERT(dst_offsets != Z_NULL);
    std::vector<uint64_t> table;
    if (!unpack_table(count, packed_offsets, lens, dst_offsets, table) || ((uintptr_t)d_packed & 15u) ||
        ((uintptr_t)d_dst & 15u))
        return Z_STREAM_ERROR;
    const uint64_t total = table[count];
    if ((total + PK_TILE - 1u) / PK_TILE > 0x7fffffffull)
        return Z_MEM_ERROR;
    if (total == 0)
        return Z_OK;
    if (d_packed == Z_NULL || d_dst == Z_NULL)
        return Z_STREAM_ERROR;
    UnpackPending u;
    bool ok = u.table.ensure(8ull * (count + 1ull)) && u.lens.ensure(4ull * count) && u.slots.ensure(8ull * count) &&
              hipMemcpy(u.table.p, table.data(), 8ull * (count + 1ull), hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(u.lens.p, lens, 4ull * count, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(u.slots.p, dst_offsets, 8ull * count, hipMemcpyHostToDevice) == hipSuccess &&
              hipEventCreate(&u.done) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        u.table.release();
        u.lens.release();
        u.slots.release();
        return Z_MEM_ERROR;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    unpack_enqueue(count, total, d_packed, u.table.p, u.lens.p, d_dst, u.slots.p, st);
    (void)hipEventRecord(u.done, st);
    const bool launched = hipGetLastError() == hipSuccess;
    {
        std::lock_guard<std::mutex> lock(g_unpack_mu);
        g_unpack_pending.push_back(u);
    }
    return launched ? Z_OK : Z_STREAM_ERROR;
}

extern "C" ZlibReturn zsc_hip_compress_batch_packed(U32 count, const U8 *sources, const uint64_t *source_offsets,
                                                    U8 *dest, uint64_t dest_cap, uint64_t *dest_offsets,
                                                    I32 *statuses, I32 level, I32 window_bits, I32 mem_level,
                                                    ZlibStrategy strategy, U32 align)
{
    DeviceScope scope;
    ZSC_ASSERT(source_offsets != Z_NULL);
    ZSC_ASSERT(dest_offsets != Z_NULL);
    if (level == Z_NO_COMPRESSION || !pack_align_ok(align))
        return Z_STREAM_ERROR;
    dest_offsets[0] = 0;
    if (count == 0)
        return Z_OK;
    std::vector<U32> lens(count), caps(count);
    for (U32 i = 0; i < count; i++) {
        if (source_offsets[i + 1u] < source_offsets[i] || source_offsets[i + 1u] - source_offsets[i] > 0xffffffffull)
            return Z_STREAM_ERROR;
        lens[i] = (U32)(source_offsets[i + 1u] - source_offsets[i]);
    }
    const uint64_t image = source_offsets[count];
    ZSC_ASSERT(image == 0 || sources != Z_NULL);
    std::vector<uint64_t> in_off(count), out_off(count);
    uint64_t in_bytes = 0, out_bytes = 0;
    ZlibReturn rc = zsc_hip_deflate_plan_layout(count, lens.data(), level, window_bits, mem_level, in_off.data(),
                                                out_off.data(), caps.data(), &in_bytes, &out_bytes);
    if (rc != Z_OK)
        return rc;
    zsc_hip_deflate_plan *pl = nullptr;
    rc = zsc_hip_deflate_plan_create(&pl, count, lens.data(), in_off.data(), out_off.data(), caps.data(), level,
                                     window_bits, mem_level, strategy);
    if (rc != Z_OK)
        return rc;
    rc = zsc_hip_deflate_plan_pack_enable(pl, align);
    DevBuf d_img, d_in, d_out, d_packed, d_table, d_lens, d_slots;
    const uint64_t pcap = std::min(dest_cap, pl->pack.max_total);
    if (rc == Z_OK &&
        !(d_img.ensure(image) && d_in.ensure(in_bytes) && d_out.ensure(out_bytes) && d_packed.ensure(pcap) &&
          d_table.ensure(8ull * (count + 1ull)) && d_lens.ensure(4ull * count) && d_slots.ensure(8ull * count)))
        rc = Z_MEM_ERROR;
    /* one copy in, then the image is cut into the plan's layout on the device */
    if (rc == Z_OK &&
        !((image == 0 || hipMemcpy(d_img.p, sources + source_offsets[0], image - source_offsets[0],
                                   hipMemcpyHostToDevice) == hipSuccess) &&
          hipMemcpy(d_lens.p, lens.data(), 4ull * count, hipMemcpyHostToDevice) == hipSuccess &&
          hipMemcpy(d_slots.p, in_off.data(), 8ull * count, hipMemcpyHostToDevice) == hipSuccess))
        rc = Z_STREAM_ERROR;
    if (rc == Z_OK) {
        std::vector<uint64_t> table(source_offsets, source_offsets + count + 1u);
        for (uint64_t &t : table)
            t -= source_offsets[0];
        if (hipMemcpy(d_table.p, table.data(), 8ull * (count + 1ull), hipMemcpyHostToDevice) != hipSuccess)
            rc = Z_STREAM_ERROR;
        else
            unpack_enqueue(count, table[count], d_img.p, d_table.p, d_lens.p, d_in.p, d_slots.p, nullptr);
    }
    if (rc == Z_OK)
        rc = zsc_hip_deflate_plan_run(pl, d_in.p, d_out.p, nullptr);
    if (rc == Z_OK)
        rc = zsc_hip_deflate_plan_pack(pl, d_out.p, d_packed.p, pcap, nullptr);
    if (rc == Z_OK)
        rc = zsc_hip_deflate_plan_results(pl, Z_NULL, statuses);
    if (rc == Z_OK) {
        uint64_t total = 0;
        rc = zsc_hip_deflate_plan_pack_results(pl, dest_offsets, &total, Z_NULL);
        /* ... and one copy out */
        if (rc == Z_OK && total && hipMemcpy(dest, d_packed.p, total, hipMemcpyDeviceToHost) != hipSuccess)
            rc = Z_STREAM_ERROR;
    }
    (void)hipDeviceSynchronize();
    for (DevBuf *b : {&d_img, &d_in, &d_out, &d_packed, &d_table, &d_lens, &d_slots})
        b->release();
    zsc_hip_deflate_plan_destroy(pl);
    return rc;
}

extern "C" ZlibReturn zsc_hip_bgzf_compress_batch(U32 nfiles, const U8 *const *sources, const uint64_t *source_lens,
                                                  U8 *const *dests, uint64_t *dest_lens, I32 *statuses, I32 level,
                                                  I32 mem_level, ZlibStrategy strategy, U32 block_bytes)
{
    DeviceScope scope;
    ZSC_ASSERT(nfiles == 0 || (sources != Z_NULL && source_lens != Z_NULL && dests != Z_NULL && dest_lens != Z_NULL));
    if (block_bytes == 0)
        block_bytes = 65280u;
    if (level == Z_NO_COMPRESSION || (block_bytes & 15u) || block_bytes > BZ_MAX_MEMBER)
        return Z_STREAM_ERROR;
    /* file f lies at base[f], a multiple of 16, and is cut where it lies: block_bytes is one too, so every
     * buffer starts at one, and the plan compresses a buffer as if nothing lay before or behind it */
    std::vector<uint64_t> base((size_t)nfiles + 1u, 0);
    std::vector<U32> first((size_t)nfiles + 1u, 0);
    for (U32 f = 0; f < nfiles; f++) {
        const uint64_t nb = (source_lens[f] + block_bytes - 1u) / block_bytes;
        if (source_lens[f] > (1ull << 46) || first[f] + nb > 0x7fffffffull - nfiles)
            return Z_MEM_ERROR;
        first[f + 1u] = first[f] + (U32)nb;
        base[f + 1u] = base[f] + ((source_lens[f] + 15u) & ~15ull);
    }
    const U32 count = first[nfiles];
    if (count == 0) { /* nothing to compress: every file is the 28 bytes that end one */
        static const U8 kEof[BZ_TAIL] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0};
        for (U32 f = 0; f < nfiles; f++) {
            const bool room = dest_lens[f] >= BZ_TAIL;
            if (room)
                memcpy(dests[f], kEof, BZ_TAIL);
            dest_lens[f] = BZ_TAIL;
            if (statuses)
                statuses[f] = room ? Z_OK : Z_BUF_ERROR;
        }
        return Z_OK;
    }
    std::vector<U32> lens(std::max<U32>(count, 1)), caps(std::max<U32>(count, 1));
    std::vector<uint64_t> in_off(std::max<U32>(count, 1)), out_off(std::max<U32>(count, 1));
    uint64_t out_bytes = 0;
    for (U32 f = 0; f < nfiles; f++)
        for (U32 i = first[f]; i < first[f + 1u]; i++) {
            const uint64_t at = (uint64_t)(i - first[f]) * block_bytes;
            lens[i] = (U32)std::min<uint64_t>(block_bytes, source_lens[f] - at);
        }
    ZlibReturn rc = zsc_hip_deflate_plan_layout(count, lens.data(), level, 31, mem_level, in_off.data(), out_off.data(),
                                                caps.data(), Z_NULL, &out_bytes);
    if (rc != Z_OK)
        return rc;
    for (U32 f = 0; f < nfiles; f++)
        for (U32 i = first[f]; i < first[f + 1u]; i++)
            in_off[i] = base[f] + (uint64_t)(i - first[f]) * block_bytes;
    zsc_hip_deflate_plan *pl = nullptr;
    rc = zsc_hip_deflate_plan_create(&pl, count, lens.data(), in_off.data(), out_off.data(), caps.data(), level, 31,
                                     mem_level, strategy);
    if (rc != Z_OK)
        return rc;
    rc = zsc_hip_deflate_plan_bgzf_enable(pl, nfiles, first.data(), 16u);
    DevBuf d_in, d_out, d_image;
    const uint64_t icap = rc == Z_OK ? pl->bgzf.max_total : 0;
    if (rc == Z_OK && !(d_in.ensure(base[nfiles] + 64u) && d_out.ensure(out_bytes) && d_image.ensure(icap)))
        rc = Z_MEM_ERROR;
    for (U32 f = 0; rc == Z_OK && f < nfiles; f++) /* one copy in per file */
        if (source_lens[f] && hipMemcpy((uint8_t *)d_in.p + base[f], sources[f], source_lens[f],
                                        hipMemcpyHostToDevice) != hipSuccess)
            rc = Z_STREAM_ERROR;
    if (rc == Z_OK)
        rc = zsc_hip_deflate_plan_run(pl, d_in.p, d_out.p, nullptr);
    if (rc == Z_OK)
        rc = zsc_hip_deflate_plan_bgzf(pl, d_out.p, d_image.p, icap, nullptr);
    if (rc == Z_OK)
        rc = zsc_hip_deflate_plan_results(pl, Z_NULL, Z_NULL);
    if (rc == Z_OK) {
        std::vector<uint64_t> off((size_t)nfiles + 1u), flen(std::max<U32>(nfiles, 1));
        std::vector<I32> fst(std::max<U32>(nfiles, 1));
        rc = zsc_hip_deflate_plan_bgzf_results(pl, off.data(), flen.data(), fst.data(), Z_NULL, Z_NULL, Z_NULL);
        for (U32 f = 0; rc == Z_OK && f < nfiles; f++) { /* ... and one out */
            const uint64_t room = dest_lens[f];
            dest_lens[f] = flen[f];
            I32 s = fst[f];
            if (s == Z_OK && flen[f] > room)
                s = Z_BUF_ERROR;
            else if (s == Z_OK &&
                     hipMemcpy(dests[f], (const uint8_t *)d_image.p + off[f], flen[f], hipMemcpyDeviceToHost) != hipSuccess)
                rc = Z_STREAM_ERROR;
            if (statuses)
                statuses[f] = s;
        }
    }
    (void)hipDeviceSynchronize();
    for (DevBuf *b : {&d_in, &d_out, &d_image})
        b->release();
    zsc_hip_deflate_plan_destroy(pl);
    return rc;
}

extern "C" ZlibReturn zsc_hip_zip_compress_batch(U32 narchives, const U32 *arch_first, const U8 *const *sources,
                                                 const U32 *source_lens, const U8 *names, const uint64_t *name_offsets,
                                                 const U32 *dos_datetime, U32 flags, U8 *const *dests,
                                                 uint64_t *dest_lens, I32 *statuses, I32 level, I32 mem_level,
                                                 ZlibStrategy strategy)
{
    DeviceScope scope;
    ZSC_ASSERT(arch_first != Z_NULL && name_offsets != Z_NULL);
    ZSC_ASSERT(narchives == 0 || (dests != Z_NULL && dest_lens != Z_NULL));
    if (level == Z_NO_COMPRESSION)
        return Z_STREAM_ERROR;
    const U32 count = arch_first[narchives];
    ZSC_ASSERT(count == 0 || (sources != Z_NULL && source_lens != Z_NULL));
    if (count == 0) { /* nothing to compress: every archive is an end record alone */
        static const U8 kEnd[ZP_END] = {0x50, 0x4b, 5, 6};
        if (flags & ~ZSC_HIP_ZIP_UTF8)
            return Z_STREAM_ERROR;
        for (U32 a = 0; a < narchives; a++)
            if (arch_first[a] != 0u)
                return Z_STREAM_ERROR;
        for (U32 a = 0; a < narchives; a++) {
            const bool room = dest_lens[a] >= ZP_END;
            if (room)
                memcpy(dests[a], kEnd, ZP_END);
            dest_lens[a] = ZP_END;
            if (statuses)
                statuses[a] = room ? Z_OK : Z_BUF_ERROR;
        }
        return Z_OK;
    }
    if (zsc_hip_init(-1) != Z_OK)
        return Z_STREAM_ERROR;
    std::vector<U32> caps(std::max<U32>(count, 1));
    std::vector<uint64_t> in_off(std::max<U32>(count, 1)), out_off(std::max<U32>(count, 1));
    uint64_t in_bytes = 0, out_bytes = 0;
    ZlibReturn rc = zsc_hip_deflate_plan_layout(count, source_lens, level, 31, mem_level, in_off.data(), out_off.data(),
                                                caps.data(), &in_bytes, &out_bytes);
    if (rc != Z_OK)
        return rc;
    zsc_hip_deflate_plan *pl = nullptr;
    rc = zsc_hip_deflate_plan_create(&pl, count, source_lens, in_off.data(), out_off.data(), caps.data(), level, 31,
                                     mem_level, strategy);
    if (rc != Z_OK)
        return rc;
    rc = zsc_hip_deflate_plan_zip_enable(pl, narchives, arch_first, names, name_offsets, dos_datetime, flags, 16u);
    DevBuf d_in, d_out, d_image;
    const uint64_t icap = rc == Z_OK ? pl->zip.max_total : 0;
    if (rc == Z_OK && !(d_in.ensure(in_bytes) && d_out.ensure(out_bytes) && d_image.ensure(icap)))
        rc = Z_MEM_ERROR;
    if (rc == Z_OK) { /* one upload: the buffers gathered at the plan's offsets */
        std::vector<U8> stage((size_t)in_bytes, 0);
        for (U32 i = 0; i < count; i++)
            if (source_lens[i])
                memcpy(stage.data() + in_off[i], sources[i], source_lens[i]);
        if (in_bytes && hipMemcpy(d_in.p, stage.data(), in_bytes, hipMemcpyHostToDevice) != hipSuccess)
            rc = Z_STREAM_ERROR;
    }
    if (rc == Z_OK)
        rc = zsc_hip_deflate_plan_run(pl, d_in.p, d_out.p, nullptr);
    if (rc == Z_OK)
        rc = zsc_hip_deflate_plan_zip(pl, d_out.p, d_image.p, icap, nullptr);
    if (rc == Z_OK)
        rc = zsc_hip_deflate_plan_results(pl, Z_NULL, Z_NULL);
    if (rc == Z_OK) {
        std::vector<uint64_t> off((size_t)narchives + 1u), alen(std::max<U32>(narchives, 1));
        std::vector<I32> ast(std::max<U32>(narchives, 1));
        rc = zsc_hip_deflate_plan_zip_results(pl, off.data(), alen.data(), ast.data(), Z_NULL, Z_NULL, Z_NULL, Z_NULL,
                                              Z_NULL);
        for (U32 a = 0; rc == Z_OK && a < narchives; a++) { /* ... and one copy out per archive */
            const uint64_t room = dest_lens[a];
            dest_lens[a] = alen[a];
            I32 s = ast[a];
            if (s == Z_OK && alen[a] > room)
                s = Z_BUF_ERROR;
            else if (s == Z_OK &&
                     hipMemcpy(dests[a], (const uint8_t *)d_image.p + off[a], alen[a], hipMemcpyDeviceToHost) != hipSuccess)
                rc = Z_STREAM_ERROR;
            if (statuses)
                statuses[a] = s;
        }
    }
    (void)hipDeviceSynchronize();
    for (DevBuf *b : {&d_in, &d_out, &d_image})
        b->release();
    zsc_hip_deflate_plan_destroy(pl);
    return rc;
}

extern "C" ZlibReturn zsc_hip_uncompress_batch_packed(U32 count, const U8 *sources, const uint64_t *source_offsets,
                                                      const U32 *source_lens, const U32 *dest_caps, U8 *dest,
                                                      uint64_t dest_cap, uint64_t *dest_offsets, U32 *dest_lens,
                                                      U32 *consumed, I32 *statuses, I32 window_bits, U32 align)
{
    DeviceScope scope;
    ZSC_ASSERT(dest_offsets != Z_NULL);
    if (!pack_align_ok(align))
        return Z_STREAM_ERROR;
    dest_offsets[0] = 0;
    if (count == 0)
        return Z_OK;
    ZSC_ASSERT(source_offsets != Z_NULL);
    ZSC_ASSERT(source_lens != Z_NULL);
    ZSC_ASSERT(dest_caps != Z_NULL);
    if (zsc_hip_init(-1) != Z_OK)
        return Z_STREAM_ERROR;
    /* the layout of zsc_hip_uncompress_batch */
    std::vector<uint64_t> so(count), dof(count), table;
    uint64_t sb = 0, db = 0;
    for (U32 i = 0; i < count; i++) {
        so[i] = sb;
        dof[i] = db;
        sb += ((uint64_t)source_lens[i] + 64u + 15u) & ~15ull;
        db += ((uint64_t)dest_caps[i] + 64u + 15u) & ~15ull;
    }
    if (!unpack_table(count, source_offsets, source_lens, so.data(), table))
        return Z_STREAM_ERROR;
    const uint64_t first = table[0], image = table[count] - first;
    for (uint64_t &t : table)
        t -= first;
    ZSC_ASSERT(image == 0 || sources != Z_NULL);
    zsc_hip_inflate_plan *pl = nullptr;
    ZlibReturn rc = zsc_hip_inflate_plan_create(&pl, count, source_lens, so.data(), dest_caps, dof.data(), window_bits);
    if (rc != Z_OK)
        return rc;
    rc = zsc_hip_inflate_plan_pack_enable(pl, align);
    DevBuf d_img, d_src, d_dst, d_packed, d_table, d_lens, d_slots;
    const uint64_t pcap = std::min(dest_cap, pl->pack.max_total);
    if (rc == Z_OK &&
        !(d_img.ensure(image) && d_src.ensure(sb + 64) && d_dst.ensure(db + 64) && d_packed.ensure(pcap) &&
          d_table.ensure(8ull * (count + 1ull)) && d_lens.ensure(4ull * count) && d_slots.ensure(8ull * count)))
        rc = Z_MEM_ERROR;
    if (rc == Z_OK &&
        !((image == 0 || hipMemcpy(d_img.p, sources + first, image, hipMemcpyHostToDevice) == hipSuccess) &&
          hipMemcpy(d_table.p, table.data(), 8ull * (count + 1ull), hipMemcpyHostToDevice) == hipSuccess &&
          hipMemcpy(d_lens.p, source_lens, 4ull * count, hipMemcpyHostToDevice) == hipSuccess &&
          hipMemcpy(d_slots.p, so.data(), 8ull * count, hipMemcpyHostToDevice) == hipSuccess))
        rc = Z_STREAM_ERROR;
    if (rc == Z_OK) {
        unpack_enqueue(count, image, d_img.p, d_table.p, d_lens.p, d_src.p, d_slots.p, nullptr);
        rc = zsc_hip_inflate_plan_run(pl, d_src.p, d_dst.p, nullptr);
    }
    /* (the results first: a damaged stream that resynchronises is finished there) */
    if (rc == Z_OK)
        rc = zsc_hip_inflate_plan_results(pl, dest_lens, consumed, statuses, nullptr);
    if (rc == Z_OK)
        rc = zsc_hip_inflate_plan_pack(pl, d_dst.p, d_packed.p, pcap, nullptr);
    if (rc == Z_OK) {
        uint64_t total = 0;
        rc = zsc_hip_inflate_plan_pack_results(pl, dest_offsets, &total, Z_NULL);
        if (rc == Z_OK && total && hipMemcpy(dest, d_packed.p, total, hipMemcpyDeviceToHost) != hipSuccess)
            rc = Z_STREAM_ERROR;
    }
    (void)hipDeviceSynchronize();
    for (DevBuf *b : {&d_img, &d_src, &d_dst, &d_packed, &d_table, &d_lens, &d_slots})
        b->release();
    zsc_hip_inflate_plan_destroy(pl);
    return rc;
}

/* ---- BGZF ranges: the member index and the ranges plan (bgzf_read.h, bgzf_read_host.h) ------------------ */

#include "bgzf_read_host.h"

struct zsc_hip_bgzf_index {
    uint32_t nfiles = 0;
    std::vector<BgrFile> files;
    std::vector<uint64_t> first; /* nfiles + 1: where a file's members + 1 entries start in the tables */
    std::vector<uint64_t> coff, uoff;
    DevBuf d_table;              /* the same on the device: every coffset, then every uoffset */
    float build_ms = 0.f;

    BgzTable table(uint32_t f) const
    {
        return {coff.data() + first[f], uoff.data() + first[f], (uint32_t)(first[f + 1] - first[f] - 1u)};
    }
};

extern "C" void zsc_hip_bgzf_index_destroy(zsc_hip_bgzf_index *ix)
{
    DeviceScope scope;
    if (!ix)
        return;
    ix->d_table.release();
    delete ix;
}

/* the tables of an index whose `first` is set, from the device (every coffset, then every uoffset) */
static bool bgi_download(zsc_hip_bgzf_index *ix)
{
    const uint64_t total = ix->first[ix->nfiles];
    ix->coff.resize(total);
    ix->uoff.resize(total);
    return hipMemcpy(ix->coff.data(), ix->d_table.p, 8 * total, hipMemcpyDeviceToHost) == hipSuccess &&
           hipMemcpy(ix->uoff.data(), (const uint64_t *)ix->d_table.p + total, 8 * total, hipMemcpyDeviceToHost) ==
               hipSuccess;
}

extern "C" ZlibReturn zsc_hip_bgzf_index_build(zsc_hip_bgzf_index **index_out, U32 nfiles, const void *d_src,
                                               const U32 *source_lens, const uint64_t *src_offsets, void *hip_stream)
{
    ZSC_ASSERT(index_out != Z_NULL);
    *index_out = nullptr;
    ZSC_ASSERT(nfiles == 0 || (source_lens != Z_NULL && src_offsets != Z_NULL));
    /* the buffers, the layout and the view of a members plan over the files: its first four launches are the
     * index's (claims on, whatever the plan's switch says) */
    std::vector<U32> caps(nfiles, 0);
    std::vector<uint64_t> zero(nfiles, 0);
    zsc_hip_inflate_plan *mp = nullptr;
    ZlibReturn rc = zsc_hip_inflate_plan_create_members(&mp, nfiles, source_lens, src_offsets, caps.data(), zero.data(),
                                                        31, 0);
    if (rc != Z_OK)
        return rc;
    DeviceScope scope;
    mp->mp.claims = 1;
    hipStream_t st = (hipStream_t)hip_stream;
    auto *ix = new zsc_hip_bgzf_index();
    ix->nfiles = nfiles;
    ix->files.resize(nfiles);
    ix->first.assign(nfiles + 1ull, 0);
    std::vector<uint64_t> tbase(nfiles + 1ull, 0);
    for (U32 f = 0; f < nfiles; f++) {
        ix->files[f] = BgrFile{src_offsets[f], source_lens[f], 0};
        tbase[f + 1] = tbase[f] + BGI_TABLE_CAP(source_lens[f]);
    }
    DevBuf d_tbase, d_first, d_coff, d_uoff, d_members;
    std::vector<U32> members(nfiles);
    /* (mem: every allocation was had -- what failed otherwise was a copy, a launch or the wait) */
    bool mem = d_tbase.ensure(8 * (nfiles + 1ull)) && d_first.ensure(8 * (nfiles + 1ull)) &&
               d_coff.ensure(8 * std::max<uint64_t>(1, tbase[nfiles])) &&
               d_uoff.ensure(8 * std::max<uint64_t>(1, tbase[nfiles])) && d_members.ensure(4 * std::max(1u, nfiles));
    bool ok = mem && hipMemcpy(d_tbase.p, tbase.data(), 8 * (nfiles + 1ull), hipMemcpyHostToDevice) == hipSuccess;
    if (ok && nfiles) {
        const MemPlan &M = mp->mp;
        const uint8_t *src = (const uint8_t *)d_src;
        const InfGrid g(nfiles, mp->ncand_total, M.sp.ntiles);
        (void)hipGetLastError();
        ok = hipMemsetAsync(mp->d_scount.p, 0, 4ull * nfiles, st) == hipSuccess &&
             hipMemsetAsync(mp->d_q.p, 0, 16, st) == hipSuccess;
        (void)hipEventRecord(mp->ev0, st);
        hipLaunchKernelGGL(k_mem_scan, dim3(g.scans), dim3(64), 0, st, src, M, 0);
        hipLaunchKernelGGL(k_sec_setup, dim3(g.per_stream), dim3(64), 0, st, M.sp);
        hipLaunchKernelGGL(k_mem_scan, dim3(g.scans), dim3(64), 0, st, src, M, 1);
        hipLaunchKernelGGL(k_mem_claims, dim3(g.per_stream), dim3(64), 0, st, src, M);
        hipLaunchKernelGGL(k_bgi_chain, dim3(g.per_group), dim3(64), 0, st, src, M, (const uint64_t *)d_tbase.p,
                           (uint64_t *)d_coff.p, (uint64_t *)d_uoff.p, (uint32_t *)d_members.p);
        (void)hipEventRecord(mp->ev1, st);
        /* the counts come back, and the tables move to the room they need */
        ok = ok && hipStreamSynchronize(st) == hipSuccess && hipGetLastError() == hipSuccess &&
             hipMemcpy(members.data(), d_members.p, 4ull * nfiles, hipMemcpyDeviceToHost) == hipSuccess;
        if (ok)
            (void)hipEventElapsedTime(&ix->build_ms, mp->ev0, mp->ev1);
    }
    for (U32 f = 0; ok && f < nfiles; f++)
        ix->first[f + 1] = ix->first[f] + members[f] + 1ull;
    const uint64_t total = ix->first[nfiles];
    if (ok && !ix->d_table.ensure(16 * std::max<uint64_t>(1, total)))
        ok = mem = false;
    if (ok && nfiles) {
        ok = hipMemcpyAsync(d_first.p, ix->first.data(), 8 * (nfiles + 1ull), hipMemcpyHostToDevice, st) == hipSuccess;
        hipLaunchKernelGGL(k_bgi_gather, dim3(std::min(nfiles, (uint32_t)g_cus * 8u)), dim3(64), 0, st,
                           (const uint64_t *)d_tbase.p, (const uint64_t *)d_first.p, (const uint64_t *)d_coff.p,
                           (const uint64_t *)d_uoff.p, (uint64_t *)ix->d_table.p, total, nfiles);
        ok = ok && hipStreamSynchronize(st) == hipSuccess && hipGetLastError() == hipSuccess && bgi_download(ix);
    }
    if (!ok) {
        (void)hipStreamSynchronize(st); /* (what was enqueued before the failure may still use the buffers) */
        (void)hipGetLastError();
    }
    for (DevBuf *b : {&d_tbase, &d_first, &d_coff, &d_uoff, &d_members})
        b->release();
    zsc_hip_inflate_plan_destroy(mp);
    if (!ok) {
        zsc_hip_bgzf_index_destroy(ix);
        return mem ? Z_STREAM_ERROR : Z_MEM_ERROR;
    }
    *index_out = ix;
    return Z_OK;
}

__global__ __launch_bounds__(64) void k_bgi_verify(const uint8_t *__restrict__ src, uint32_t n,
                                                   const uint64_t *__restrict__ coff, const uint64_t *__restrict__ uoff,
                                                   uint32_t cnt, uint32_t *__restrict__ out)
{
    for (uint32_t e0 = blockIdx.x * 64u; e0 < cnt; e0 += gridDim.x * 64u)
        bgi_verify(src, n, coff, uoff, cnt, e0, out);
}

/* (one lane group: the walk behind the last named member start, over that entry) */
__global__ __launch_bounds__(INF_GROUP) void k_bgi_tail(const uint8_t *__restrict__ src, uint32_t n, uint64_t *coff,
                                                        uint64_t *uoff, uint32_t cnt, uint64_t tcap, uint32_t *out)
{
    const uint64_t at = coff[cnt - 1u];
    if (at <= n)
        bgi_walk(src, n, (uint32_t)at, uoff[cnt - 1u], coff + (cnt - 1u), uoff + (cnt - 1u), tcap - (cnt - 1u), out + 1);
}

extern "C" ZlibReturn zsc_hip_bgzf_index_import_gzi(zsc_hip_bgzf_index **index_out, const U8 *gzi, uint64_t gzi_len,
                                                    const void *d_src, U32 source_len, uint64_t src_offset,
                                                    void *hip_stream)
{
    DeviceScope scope;
    ZSC_ASSERT(index_out != Z_NULL);
    *index_out = nullptr;
    if (zsc_hip_init(-1) != Z_OK || (src_offset & 15u))
        return Z_STREAM_ERROR;
    std::vector<uint64_t> c, u;
    if (gzi == Z_NULL || !bgz_gzi_parse(gzi, gzi_len, c, u) || c.size() + 1u > BGI_TABLE_CAP(source_len))
        return Z_DATA_ERROR;
    const uint32_t cnt = (uint32_t)c.size();
    const uint64_t tcap = bgz_import_room(c, source_len);
    hipStream_t st = (hipStream_t)hip_stream;
    auto *ix = new zsc_hip_bgzf_index();
    ix->nfiles = 1;
    ix->files.assign(1, BgrFile{src_offset, source_len, 0});
    /* the table's room on the device: the named entries and what the walk behind the last of them can find
     * (bgz_import_room); out[0]: an entry does not fit
     * the file, out[1]: the members the walk found from the last entry on */
    DevBuf d_out;
    uint32_t out[2] = {0, 0};
    const uint8_t *src = (const uint8_t *)d_src + src_offset;
    uint64_t *dc = nullptr, *du = nullptr;
    bool mem = ix->d_table.ensure(16 * tcap) && d_out.ensure(8), ok = mem;
    if (ok) {
        dc = (uint64_t *)ix->d_table.p;
        du = dc + tcap;
        (void)hipGetLastError();
        ok = hipMemsetAsync(d_out.p, 0, 8, st) == hipSuccess &&
             hipMemcpyAsync(dc, c.data(), 8ull * cnt, hipMemcpyHostToDevice, st) == hipSuccess &&
             hipMemcpyAsync(du, u.data(), 8ull * cnt, hipMemcpyHostToDevice, st) == hipSuccess;
        hipLaunchKernelGGL(k_bgi_verify, dim3(std::min((cnt + 63u) / 64u, (uint32_t)g_cus * 8u)), dim3(64), 0, st, src,
                           source_len, (const uint64_t *)dc, (const uint64_t *)du, cnt, (uint32_t *)d_out.p);
        hipLaunchKernelGGL(k_bgi_tail, dim3(1), dim3(INF_GROUP), 0, st, src, source_len, dc, du, cnt, tcap,
                           (uint32_t *)d_out.p);
        ok = ok && hipStreamSynchronize(st) == hipSuccess && hipGetLastError() == hipSuccess &&
             hipMemcpy(out, d_out.p, 8, hipMemcpyDeviceToHost) == hipSuccess;
    }
    if (!ok) {
        (void)hipStreamSynchronize(st); /* (what was enqueued before the failure may still use the buffers) */
        (void)hipGetLastError();
    }
    d_out.release();
    ZlibReturn rc = !ok ? (mem ? Z_STREAM_ERROR : Z_MEM_ERROR) : out[0] ? Z_DATA_ERROR : Z_OK;
    if (rc == Z_OK) {
        /* (the uoffsets move up behind the coffsets: the layout of a built index) */
        const uint64_t total = cnt + (uint64_t)out[1];
        ix->first = {0, total};
        ix->coff.resize(total);
        ix->uoff.resize(total);
        DevBuf exact;
        mem = exact.ensure(16 * total);
        ok = mem && hipMemcpy(exact.p, dc, 8 * total, hipMemcpyDeviceToDevice) == hipSuccess &&
             hipMemcpy((uint64_t *)exact.p + total, du, 8 * total, hipMemcpyDeviceToDevice) == hipSuccess;
        ix->d_table.release();
        ix->d_table = exact;
        ok = ok && bgi_download(ix);
        rc = ok ? Z_OK : mem ? Z_STREAM_ERROR : Z_MEM_ERROR;
    }
    if (rc != Z_OK) {
        zsc_hip_bgzf_index_destroy(ix);
        return rc;
    }
    *index_out = ix;
    return Z_OK;
}

extern "C" ZlibReturn zsc_hip_bgzf_index_info(const zsc_hip_bgzf_index *ix, U32 file, U32 *members,
                                              uint64_t *indexed_bytes, uint64_t *total_out)
{
    ZSC_ASSERT(ix != Z_NULL);
    if (file >= ix->nfiles)
        return Z_STREAM_ERROR;
    const BgzTable T = ix->table(file);
    if (members)
        *members = T.members;
    if (indexed_bytes)
        *indexed_bytes = T.coff[T.members];
    if (total_out)
        *total_out = T.total_out();
    return Z_OK;
}

extern "C" ZlibReturn zsc_hip_bgzf_index_table(const zsc_hip_bgzf_index *ix, U32 file, uint64_t *coffsets,
                                               uint64_t *uoffsets, U32 cap)
{
    ZSC_ASSERT(ix != Z_NULL);
    if (file >= ix->nfiles)
        return Z_STREAM_ERROR;
    const BgzTable T = ix->table(file);
    if (cap < T.members + 1u)
        return Z_BUF_ERROR;
    if (coffsets)
        std::copy(T.coff, T.coff + T.members + 1u, coffsets);
    if (uoffsets)
        std::copy(T.uoff, T.uoff + T.members + 1u, uoffsets);
    return Z_OK;
}

extern "C" uint64_t zsc_hip_bgzf_index_scratch_bytes(const zsc_hip_bgzf_index *ix)
{
    return ix ? 16 * std::max<uint64_t>(1, ix->first[ix->nfiles]) : 0;
}

extern "C" float zsc_hip_bgzf_index_build_ms(const zsc_hip_bgzf_index *ix)
{
    return ix ? ix->build_ms : 0.f;
}

extern "C" ZlibReturn zsc_hip_bgzf_index_voffset(const zsc_hip_bgzf_index *ix, U32 file, uint64_t uoffset,
                                                 uint64_t *voffset)
{
    ZSC_ASSERT(ix != Z_NULL);
    ZSC_ASSERT(voffset != Z_NULL);
    return file < ix->nfiles && bgz_voffset(ix->table(file), uoffset, voffset) ? Z_OK : Z_STREAM_ERROR;
}

extern "C" ZlibReturn zsc_hip_bgzf_index_uoffset(const zsc_hip_bgzf_index *ix, U32 file, uint64_t voffset,
                                                 uint64_t *uoffset)
{
    ZSC_ASSERT(ix != Z_NULL);
    ZSC_ASSERT(uoffset != Z_NULL);
    return file < ix->nfiles && bgz_uoffset(ix->table(file), voffset, uoffset) ? Z_OK : Z_STREAM_ERROR;
}

extern "C" ZlibReturn zsc_hip_bgzf_index_export_gzi(const zsc_hip_bgzf_index *ix, U32 file, U8 *gzi, uint64_t *gzi_len)
{
    ZSC_ASSERT(ix != Z_NULL);
    ZSC_ASSERT(gzi_len != Z_NULL);
    if (file >= ix->nfiles)
        return Z_STREAM_ERROR;
    const BgzTable T = ix->table(file);
    const uint64_t room = *gzi_len;
    *gzi_len = bgz_gzi_bytes(T.members);
    if (gzi == Z_NULL || room < *gzi_len)
        return Z_BUF_ERROR;
    bgz_gzi_export(T, gzi);
    return Z_OK;
}

extern "C" ZlibReturn zsc_hip_inflate_plan_create_bgzf_ranges(zsc_hip_inflate_plan **plan_out,
                                                              const zsc_hip_bgzf_index *ix, U32 count, const U32 *files,
                                                              const uint64_t *begins, const uint64_t *lens,
                                                              const U32 *dest_caps, const uint64_t *dst_offsets,
                                                              U32 flags)
{
    ZSC_ASSERT(plan_out != Z_NULL);
    *plan_out = nullptr;
    if (ix == Z_NULL || (flags & ~(U32)ZSC_HIP_BGZF_VOFFSETS) ||
        (count && (files == Z_NULL || begins == Z_NULL || lens == Z_NULL || dest_caps == Z_NULL || dst_offsets == Z_NULL)))
        return Z_STREAM_ERROR;
    /* the requests cut into member jobs on the host, before anything is allocated */
    std::vector<BgrJob> jobs;
    std::vector<InfResult> res0(std::max(1u, count));
    std::vector<U32> slen(count);
    std::vector<uint64_t> soff(count);
    uint64_t edges = 0;
    for (U32 i = 0; i < count; i++) {
        if (files[i] >= ix->nfiles) {
            ZSC_WARN1("zsc_hip: request %u names a file the index does not have.", i);
            return Z_STREAM_ERROR;
        }
        const BgzTable T = ix->table(files[i]);
        uint64_t b = begins[i], n = lens[i];
        if ((flags & ZSC_HIP_BGZF_VOFFSETS) && !bgr_from_voffsets(T, begins[i], lens[i], &b, &n)) {
            ZSC_WARN1("zsc_hip: the virtual offsets of request %u are not of the index.", i);
            return Z_STREAM_ERROR;
        }
        bgr_cut(T, files[i], i, b, n, dest_caps[i], dst_offsets[i], jobs, res0[i], &edges);
        slen[i] = ix->files[files[i]].src_len;
        soff[i] = ix->files[files[i]].src_off;
    }
    if (jobs.size() >= 0xffffffffull)
        return Z_MEM_ERROR;
    bgr_order(jobs);
    ZlibReturn rc = zsc_hip_inflate_plan_create(plan_out, count, slen.data(), soff.data(), dest_caps, dst_offsets, 31);
    if (rc != Z_OK)
        return rc;
    DeviceScope scope;
    zsc_hip_inflate_plan *pl = *plan_out;
    pl->kind = INF_BGZF_RANGES;
    /* ZSC_HIP_BGZF_GROUPS (a test hook): fewer lane groups, so that every staging slot is reused by several jobs */
    pl->bgr_waves = inflate_grid((uint32_t)jobs.size());
    if (const char *e = getenv("ZSC_HIP_BGZF_GROUPS")) {
        const long long g = atoll(e);
        if (g > 0)
            pl->bgr_waves = (uint32_t)std::min<long long>(pl->bgr_waves, (g + INF_PER_WAVE - 1) / INF_PER_WAVE);
    }
    const uint64_t nc = std::max(1u, count), nj = std::max<uint64_t>(1, jobs.size());
    bool ok = pl->scratch(pl->d_bfiles, sizeof(BgrFile) * std::max(1u, ix->nfiles)) &&
              pl->scratch(pl->d_bjobs, sizeof(BgrJob) * nj) && pl->scratch(pl->d_bbad, 4 * nc) &&
              pl->scratch(pl->d_bq, 16) && pl->scratch(pl->d_bres0, sizeof(InfResult) * nc) &&
              (edges == 0 || pl->scratch(pl->d_bstage, (uint64_t)BGR_SLOT * pl->bgr_waves * INF_PER_WAVE));
    ok = ok && hipMemcpy(pl->d_bres0.p, res0.data(), sizeof(InfResult) * nc, hipMemcpyHostToDevice) == hipSuccess &&
         (ix->nfiles == 0 || hipMemcpy(pl->d_bfiles.p, ix->files.data(), sizeof(BgrFile) * ix->nfiles,
                                       hipMemcpyHostToDevice) == hipSuccess) &&
         (jobs.empty() || hipMemcpy(pl->d_bjobs.p, jobs.data(), sizeof(BgrJob) * jobs.size(), hipMemcpyHostToDevice) ==
                              hipSuccess);
    if (!ok)
        return inflate_plan_fail(plan_out);
    BgrPlan &B = pl->bp;
    B.files = (const BgrFile *)pl->d_bfiles.p;
    B.jobs = (const BgrJob *)pl->d_bjobs.p;
    B.bad = (uint32_t *)pl->d_bbad.p;
    B.q = (uint32_t *)pl->d_bq.p;
    B.njobs = (uint32_t)jobs.size();
    B.count = count;
    return Z_OK;
}

extern "C" ZlibReturn zsc_hip_inflate_plan_bgzf_jobs(zsc_hip_inflate_plan *pl, uint64_t *jobs, uint64_t *decoded_bytes)
{
    ZSC_ASSERT(pl != Z_NULL);
    if (pl->kind != INF_BGZF_RANGES)
        return Z_STREAM_ERROR;
    std::vector<BgrJob> j(pl->bp.njobs);
    DeviceScope scope;
    if (!j.empty())
        HIP_TRY(hipMemcpy(j.data(), pl->d_bjobs.p, sizeof(BgrJob) * j.size(), hipMemcpyDeviceToHost), return Z_STREAM_ERROR);
    uint64_t sum = 0;
    for (const BgrJob &x : j)
        sum += x.len;
    if (jobs)
        *jobs = j.size();
    if (decoded_bytes)
        *decoded_bytes = sum;
    return Z_OK;
}

/* Host memory: the files go up once each, an index and a ranges plan are made over them, and the requests'
 * bytes come back as one packed image that is dealt out to dests */
extern "C" ZlibReturn zsc_hip_bgzf_read_ranges_batch(U32 nfiles, const U8 *const *sources, const U32 *source_lens,
                                                     U32 count, const U32 *files, const uint64_t *begins,
                                                     const uint64_t *lens, U8 *const *dests, U32 *dest_lens,
                                                     I32 *statuses, U32 flags)
{
    DeviceScope scope;
    if (count == 0)
        return Z_OK;
    ZSC_ASSERT(nfiles == 0 || (sources != Z_NULL && source_lens != Z_NULL));
    ZSC_ASSERT(dests != Z_NULL);
    ZSC_ASSERT(dest_lens != Z_NULL);
    if (zsc_hip_init(-1) != Z_OK)
        return Z_STREAM_ERROR;
    std::vector<uint64_t> so(nfiles), dof(count), offs(count + 1ull);
    uint64_t sb = 0, db = 0;
    for (U32 f = 0; f < nfiles; f++) {
        so[f] = sb;
        sb += ((uint64_t)source_lens[f] + 64u + 15u) & ~15ull;
    }
    for (U32 i = 0; i < count; i++) {
        dof[i] = db;
        db += ((uint64_t)dest_lens[i] + 15u) & ~15ull;
    }
    DevBuf d_src, d_dst, d_packed;
    zsc_hip_bgzf_index *ix = nullptr;
    zsc_hip_inflate_plan *pl = nullptr;
    ZlibReturn rc = d_src.ensure(sb + 64) ? Z_OK : Z_MEM_ERROR;
    for (U32 f = 0; f < nfiles && rc == Z_OK; f++) {
        ZSC_ASSERT(sources[f] != Z_NULL);
        if (source_lens[f] &&
            hipMemcpy((uint8_t *)d_src.p + so[f], sources[f], source_lens[f], hipMemcpyHostToDevice) != hipSuccess)
            rc = Z_STREAM_ERROR;
    }
    if (rc == Z_OK)
        rc = zsc_hip_bgzf_index_build(&ix, nfiles, d_src.p, source_lens, so.data(), nullptr);
    if (rc == Z_OK)
        rc = zsc_hip_inflate_plan_create_bgzf_ranges(&pl, ix, count, files, begins, lens, dest_lens, dof.data(), flags);
    if (rc == Z_OK)
        rc = zsc_hip_inflate_plan_pack_enable(pl, 1);
    uint64_t pcap = 0;
    if (rc == Z_OK) {
        pcap = pl->pack.max_total;
        if (!d_dst.ensure(db + 64) || !d_packed.ensure(pcap + 16))
            rc = Z_MEM_ERROR;
    }
    std::vector<U32> outl(count);
    std::vector<I32> stat(count);
    std::vector<uint8_t> image;
    if (rc == Z_OK)
        rc = zsc_hip_inflate_plan_run(pl, d_src.p, d_dst.p, nullptr);
    if (rc == Z_OK)
        rc = zsc_hip_inflate_plan_results(pl, outl.data(), nullptr, stat.data(), nullptr);
    if (rc == Z_OK)
        rc = zsc_hip_inflate_plan_pack(pl, d_dst.p, d_packed.p, pcap, nullptr);
    if (rc == Z_OK) {
        uint64_t total = 0;
        rc = zsc_hip_inflate_plan_pack_results(pl, offs.data(), &total, Z_NULL);
        image.resize(total);
        if (rc == Z_OK && total && hipMemcpy(image.data(), d_packed.p, total, hipMemcpyDeviceToHost) != hipSuccess)
            rc = Z_STREAM_ERROR;
    }
    for (U32 i = 0; i < count && rc == Z_OK; i++) {
        if (stat[i] == Z_OK && outl[i]) {
            ZSC_ASSERT(dests[i] != Z_NULL);
            memcpy(dests[i], image.data() + offs[i], outl[i]);
        }
        dest_lens[i] = outl[i];
        if (statuses)
            statuses[i] = stat[i];
    }
    (void)hipDeviceSynchronize();
    for (DevBuf *b : {&d_src, &d_dst, &d_packed})
        b->release();
    zsc_hip_inflate_plan_destroy(pl);
    zsc_hip_bgzf_index_destroy(ix);
    return rc;
}
