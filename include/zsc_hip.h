/*
 * zsc_hip.h -- batched / device-resident entry points of libzsc_hip.so.
 *
 * Extension of the reference API (SURVEY.md 8b "extension we add"): one
 * zsc_compress() call cannot amortise a kernel launch, so the library also
 * accepts MANY independent buffers per call.  Every item has exactly the
 * semantics of one reference zsc_compress2()/zsc_uncompress2() call
 * (src/zsc_compress.c:50-160, src/zsc_uncompr.c:44-154) with
 * max_block_len >= source_len: the stream produced for an item is byte-identical
 * to the reference's, and its status is the ZlibReturn the reference returns.
 *
 * C ABI only: plain pointers and sizes, no C++/torch types.  The reference-side
 * binding a maintainer would add is shown in INTEGRATION.md.
 */
#ifndef ZSC_HIP_H
#define ZSC_HIP_H

#include <stdint.h>

#include "zsc/zlib_types_pub.h"

#ifdef __cplusplus
extern "C" {
#endif

/* library / device -------------------------------------------------------- */

/* 0 when a gfx950 device is usable; otherwise a negative ZlibReturn and a message
 * through ZSC_WARN.  Called implicitly by every other entry point. */
I32 zsc_hip_init(I32 device_ordinal);

/* human readable "device name | arch | CUs", valid until the next call */
const char *zsc_hip_device_info(void);

/* Device memory of finished calls and destroyed plans is kept for the next ones (at most a
 * quarter of the device's memory, or ZSC_HIP_CACHE_MB from the environment), which saves the
 * one-shot entry points their hipMalloc/hipFree time -- unmapping the scratch arrays was two
 * thirds of a sections call; this gives it back.  ZSC_HIP_NO_CACHE=1 keeps nothing. */
void zsc_hip_release_cached_memory(void);

/* host-pointer batches ---------------------------------------------------- */

/* Compress `count` independent buffers (host memory).  Item i:
 *   sources[i], source_lens[i]          input
 *   dests[i], dest_lens[i]              in: capacity of dests[i]; out: bytes written
 *   statuses[i]                         ZlibReturn of the item (Z_OK, Z_BUF_ERROR ...)
 * level / window_bits / mem_level / strategy as zsc_compress2 (reference
 * include/zsc/zsc_pub.h:258).  Returns Z_OK when the batch ran (look at statuses
 * for the items), or the error that stopped the whole batch. */
ZlibReturn zsc_hip_compress_batch(U32 count, const U8 *const *sources, const U32 *source_lens,
                                  U8 *const *dests, U32 *dest_lens, I32 *statuses, I32 level,
                                  I32 window_bits, I32 mem_level, ZlibStrategy strategy);

/* Level 0 (reference deflate_stored, src/deflate.c:1679-1880): `count` buffers stored, item i
 * like zsc_compress2(level 0, max_block_lens[i]) -- the lengths of the stored blocks follow the
 * output slices of max_block_len the wrapper hands out, and max_block_len < source_len gives
 * the sections their flush markers (src/zsc_compress.c:121-138). */
ZlibReturn zsc_hip_store_batch(U32 count, const U8 *const *sources, const U32 *source_lens,
                               const U32 *max_block_lens, U8 *const *dests, U32 *dest_lens,
                               I32 *statuses, I32 window_bits, I32 mem_level, U32 gzip_header_len);
/* gzip_header_len: 0, or the length of a caller-supplied gzip member header that the caller
 * writes over the start of each stream afterwards (zsc_compress_gzip with a gz_header) */

/* Levels 1-9 with source_lens[i] > max_block_lens[i]: item i like zsc_compress2(max_block_lens[i])
 * (reference src/zsc_compress.c:121-138) -- the input goes to deflate() in sections of
 * max_block_len with Z_FULL_FLUSH, the output in slices of max_block_len.  All sections of all
 * items are parsed at once; where an output slice ran out at a place that lets the next section
 * in early (SURVEY finding 2) the run is parsed again with the history (zsc_amd/csrc/sections.h).
 * gzip_header_len as in zsc_hip_store_batch. */
ZlibReturn zsc_hip_compress_sections_batch(U32 count, const U8 *const *sources,
                                           const U32 *source_lens, const U32 *max_block_lens,
                                           U8 *const *dests, U32 *dest_lens, I32 *statuses,
                                           I32 level, I32 window_bits, I32 mem_level,
                                           ZlibStrategy strategy, U32 gzip_header_len);

/* the last zsc_hip_compress_sections_* call of this process: how many sub-batches of its rounds' plans ran
 * the segmented parser in the wide and in the narrow LDS geometry (runs with joints are always wide) */
void zsc_hip_compress_sections_last_rings(U32 *wide, U32 *narrow);

/* The same with the streams in device memory: stream i is source_lens[i] bytes at d_input +
 * in_offsets[i] (16-byte aligned) and its compressed stream goes to d_output + out_offsets[i],
 * of which out_caps[i] bytes may be used (the capacity is part of the result: the wrapper hands
 * it out in slices of max_block_len).  Synchronous: returns when the streams are in place. */
ZlibReturn zsc_hip_compress_sections_device(U32 count, const void *d_input,
                                            const uint64_t *in_offsets, const U32 *source_lens,
                                            const U32 *max_block_lens, void *d_output,
                                            const uint64_t *out_offsets, const U32 *out_caps,
                                            U32 *dest_lens, I32 *statuses, I32 level,
                                            I32 window_bits, I32 mem_level, ZlibStrategy strategy);

/* Decompress `count` independent streams (host memory).  source_lens[i]: in bytes
 * available, out bytes consumed (reference zsc_uncompress2, zsc_pub.h:385). */
ZlibReturn zsc_hip_uncompress_batch(U32 count, const U8 *const *sources, U32 *source_lens,
                                    U8 *const *dests, U32 *dest_lens, I32 *statuses,
                                    I32 window_bits);

/* device-resident plans --------------------------------------------------- */

/* What a run reads, writes and remembers -- for every plan below, deflate and inflate, of every kind,
 * and for zsc_hip_compress_sections_device:
 *   reads     the bytes of the items, [offset, + length) each, and behind an item at the most 64 bytes
 *             (which is why 64 readable bytes must follow the last item of an input).  What those bytes
 *             hold has no influence on any result: a stream that ends at source_lens[i] has ended there,
 *             whatever lies behind it -- its own continuation, the next item, 0xFF -- and a buffer is
 *             compressed as if nothing lay before or behind it.
 *   writes    nothing outside the slots [offset, + capacity) of the output.  Inside a slot the bytes
 *             behind the reported length are undefined (a parallel path and its serial fallback may both
 *             have written there); the bytes behind the capacity are never written, not even the rest of
 *             the 32-bit word the capacity ends in.  The output need not be cleared before a run.
 *   remembers nothing: a plan can be run many times, on the same input or on another of the same shape,
 *             and every run gives what a freshly created plan gives.  What the accessors report
 *             (sections, members, data errors, check values, indexes) is the last run's.
 * tests/test_gpu_inflate_surroundings.py, test_gpu_deflate_surroundings.py and test_gpu_plan_rerun.py
 * hold the plans to it.
 *
 * Streams -- for the same plans:
 *   - what _run, _verify and _pack enqueue is ordered after everything enqueued earlier on the stream they
 *     are given and before everything enqueued later on it, like a kernel launched there: the input may come
 *     from a copy or a kernel still pending on that stream, and a consumer enqueued behind the call reads the
 *     finished output.  None of the three waits on the host for device work.
 *   - a clean batch is complete in stream order at the end of _run.  The inflate plans' resynchronisation of
 *     damaged streams (relaunches from the flush marker behind a data error) finishes in _results, and only
 *     for the plan's last run: a run that another _run follows before _results is left where its first pass
 *     got to.
 *   - a plan has ONE set of scratch.  A _run enqueued on another stream than the plan's unfinished earlier
 *     work -- a run, a verification, a pack, a _bgzf or a _zip -- waits for that work on the device (an event
 *     behind each enqueue, hipStreamWaitEvent only where the streams differ); the host does not wait.  A plan
 *     that only ever sees one stream enqueues nothing for this but one event record per call.
 *   - _results, every accessor and _destroy wait, on the host, for all of the plan's work, whatever streams
 *     it went to: every stream the plan was given since the last such wait is synchronised, so it must still
 *     exist then.
 *   - the caller keeps the input unchanged until _results: an inflate plan's relaunches and the index exports
 *     read it again.
 * One plan is used from one host thread at a time.  tests/test_gpu_streams.py holds the plans to it. */

/* A plan fixes the shape of a batch (how many buffers, how long each one is, the
 * codec parameters), owns all scratch memory in HBM and can be run many times on
 * inputs that already live in device memory.  Layout of the device buffers:
 *   input   buffer i occupies [in_offsets[i], in_offsets[i] + source_lens[i]);
 *           offsets are multiples of 16; 64 readable bytes must follow the last buffer
 *   output  stream i is written at out_offsets[i] (multiple of 16), capacity
 *           out_caps[i] >= zsc_compress_get_max_output_size(source_lens[i], ...)
 * zsc_hip_deflate_plan_layout() fills offsets/capacities with the tightest legal
 * layout and returns the two buffer sizes to allocate. */
typedef struct zsc_hip_deflate_plan zsc_hip_deflate_plan;

ZlibReturn zsc_hip_deflate_plan_layout(U32 count, const U32 *source_lens, I32 level,
                                       I32 window_bits, I32 mem_level, uint64_t *in_offsets,
                                       uint64_t *out_offsets, U32 *out_caps,
                                       uint64_t *in_bytes, uint64_t *out_bytes);

ZlibReturn zsc_hip_deflate_plan_create(zsc_hip_deflate_plan **plan, U32 count,
                                       const U32 *source_lens, const uint64_t *in_offsets,
                                       const uint64_t *out_offsets, const U32 *out_caps,
                                       I32 level, I32 window_bits, I32 mem_level,
                                       ZlibStrategy strategy);

/* Enqueue one full pass (checksum, hash sort, parse, Huffman plan, layout, bit
 * packing) on `hip_stream` (a hipStream_t, or NULL for the default stream).
 * Asynchronous: results are read with zsc_hip_deflate_plan_results(). */
ZlibReturn zsc_hip_deflate_plan_run(zsc_hip_deflate_plan *plan, const void *d_input,
                                    void *d_output, void *hip_stream);

/* Wait for the last run and fetch per-buffer sizes and statuses (either may be NULL). */
ZlibReturn zsc_hip_deflate_plan_results(zsc_hip_deflate_plan *plan, U32 *dest_lens,
                                        I32 *statuses);

/* Per-kernel device time in milliseconds, measured with HIP events recorded on the
 * run's stream and averaged over every run since profiling was switched on:
 * index 0 checksum, 1 hash sort, 2 match table (levels 4-9), 3 parse (the segmented multi-wave
 * kernel at levels 4-9, the greedy kernel at levels 1-3), 4 parse of short buffers (wave-per-buffer
 * kernels, levels 4-9), 5 huffman plan, 6 layout, 7 bit emit, 8 whole pass.  A plan that had to be
 * cut into sub-batches (zsc_hip_deflate_plan_sub_batches) launches every kernel once per
 * sub-batch; the times are sums over them.  Read after zsc_hip_deflate_plan_results(). */
#define ZSC_HIP_NKERNELS 9
void zsc_hip_deflate_plan_profile(zsc_hip_deflate_plan *plan, I32 enable);
ZlibReturn zsc_hip_deflate_plan_times(zsc_hip_deflate_plan *plan, float *ms_out);

/* bytes of HBM scratch the plan holds */
uint64_t zsc_hip_deflate_plan_scratch_bytes(const zsc_hip_deflate_plan *plan);

/* number of sub-batches (kernel launch sets) one run of the plan issues */
U32 zsc_hip_deflate_plan_sub_batches(const zsc_hip_deflate_plan *plan);

/* how the plan's long buffers without joints are parsed at levels 4-9: 0 the segmented parser is not
 * used, 1 in super-steps, 2 as a pipeline of segments (the default); fixed when the plan is created */
I32 zsc_hip_deflate_plan_seg_schedule(const zsc_hip_deflate_plan *plan);

/* the LDS geometry that parser runs in: 0 the segmented parser is not used, 1 the wide ring (the
 * super-steps' geometry, three workgroups on a CU), 2 the narrow ring of the pipeline alone (four), 3 some
 * sub-batches the one and some the other.  In plans the narrow ring is built for -- no joints, the
 * pipeline schedule, window_bits 15, mem_level 8, no match table -- each sub-batch takes it when it has more
 * long buffers than three per CU; ZSC_HIP_SEG_RING=narrow or =wide, set while the plan is created, says it
 * for all of them.  Fixed when the plan is created */
I32 zsc_hip_deflate_plan_seg_ring(const zsc_hip_deflate_plan *plan);

void zsc_hip_deflate_plan_destroy(zsc_hip_deflate_plan *plan);

/* The seek-point index, written with the stream (zsc_amd/csrc/deflate_index.h, DESIGN.md section 11;
 * the blob is described under "seek-point indexes" below).  With the index enabled a run also works out,
 * per stream, one seek point at the stream's start and one at the first block that holds input in every
 * later chunk of chunk_bytes compressed bytes, how far each piece reads before its start, and the check
 * value of each piece -- three launches per sub-batch after the bit packing.  An indexed inflate plan
 * (zsc_hip_inflate_plan_create_indexed) decodes the stream from such a blob; no chunks plan is needed.
 *
 * Scope: plans made by zsc_hip_deflate_plan_create -- levels 1-9, every strategy, all three wrappers.
 * Not covered: level 0 (zsc_hip_store_batch), the sections entry points (max_block_len < source_len)
 * and the zsc_* one-shot functions, none of which hands out a plan.  A plan that never enables the
 * index allocates, launches and returns exactly what it did without these functions.
 *
 * _index_enable: before _run.  chunk_bytes 0: the chunks plans' default, 128 KiB; values below 256 are
 *   taken as 256.  Calling it again with another chunk_bytes re-sizes the storage (out_caps[i] /
 *   chunk_bytes + 1 records of 32 bytes per buffer, 4 bytes per block slot of the largest sub-batch, 12
 *   bytes per buffer; counted in zsc_hip_deflate_plan_scratch_bytes).
 * _index_size, _index_export: valid after _results and before the next _run.  Z_STREAM_ERROR on a plan
 *   that never enabled the index; Z_DATA_ERROR and 0 bytes for a buffer whose status is not Z_OK (a
 *   short out_caps[i]); Z_BUF_ERROR, with *len the bytes needed -- what _index_size reports --, for a
 *   short cap.  d_input is the device input the run read, UNCHANGED since the run: the windows of the
 *   blob are gathered from it.  Given another input the blob is still well-formed but its windows are
 *   wrong, and an indexed plan sends the stream to its serial decoder.  Nothing is read outside the
 *   plan's buffers and bytes [in_offsets[buffer], + source_lens[buffer]) of d_input.
 *   The blob's header: chunk_bytes as enabled; window_bits the value an inflate plan must be given
 *   (the plan's own for zlib and raw streams, 16 + the window size for gzip); consumed the stream's
 *   length; total source_lens[buffer].
 * _index_ms: the summed device time of the three index launches over the sub-batches, averaged over
 *   the runs since profiling was switched on like zsc_hip_deflate_plan_times (which they are not part
 *   of: its whole-pass slot ends before the last sub-batch's index launches).  Valid after _results
 *   while profiling is on. */
ZlibReturn zsc_hip_deflate_plan_index_enable(zsc_hip_deflate_plan *plan, U32 chunk_bytes);
ZlibReturn zsc_hip_deflate_plan_index_size(zsc_hip_deflate_plan *plan, U32 buffer, uint64_t *bytes);
ZlibReturn zsc_hip_deflate_plan_index_export(zsc_hip_deflate_plan *plan, U32 buffer, const void *d_input,
                                             U8 *blob, uint64_t cap, uint64_t *len);
ZlibReturn zsc_hip_deflate_plan_index_ms(zsc_hip_deflate_plan *plan, float *ms);

/* Read-back verification: a plan's streams checked against their input on the device, where they lie
 * (zsc_amd/csrc/deflate_verify.h).  With verification enabled a run keeps, for
 * every block of every stream, where it starts and which input bytes it stands for; _verify then decodes
 * every block from the emitted bits, one wave per block in one launch, and compares it with the input --
 * a literal with its byte, a match as input[p + i] == input[p + i - dist] -- with no second output image;
 * a second launch, one thread per buffer, checks that the blocks tile the input, the stream's header
 * bytes, and the trailer as read from the stream against the blocks' own check values combined.  It guards
 * against soft errors, a bad copy of the output to its resting place, and a bug in the Huffman plan,
 * layout or emit kernels, none of whose results it reads.
 *
 * Scope: plans made by zsc_hip_deflate_plan_create -- levels 1-9, every strategy, window_bits 9-15, all
 * three wrappers.  Not covered: level 0 (zsc_hip_store_batch), the sections entry points and the zsc_*
 * one-shot functions.  A plan that never enables verification allocates, launches and returns exactly
 * what it did without these functions.
 *
 * Storage, held from _verify_enable to destroy and counted in zsc_hip_deflate_plan_scratch_bytes: per
 * block slot of the plan (source_lens[i] / ((1 << (mem_level + 6)) - 1) + 2 per buffer, all sub-batches)
 * 16 bytes of block facts (zsc_hip_verify_block), 16 bytes of per-block verdict and check value and 4
 * bytes naming its buffer; 52 bytes per buffer.
 *
 * The verdict of a buffer is that of its LOWEST-NUMBERED failing block (a later block may well fail too,
 * e.g. one that copies from bytes the first one got wrong); header and trailer failures are reported
 * only when no block failed.  Verification is stricter than a decoder where a decoder does not care:
 * non-zero padding bits and a gzip header other than the plan's are failures.
 *
 * What an OK does not rest on: the symbol buffers, the Huffman plans, the plan's own check value of the
 * input (the trailer is read from the stream, the value it must hold is computed anew per block).  What
 * it does rest on: the kept block facts and the input, and -- the one dependence that remains -- for a
 * RAW plan (window_bits < 0) the block compares alone, since a raw stream has no trailer to check.
 *
 * _verify_enable: before _run.  Z_STREAM_ERROR for a plan of sections.  The index may be enabled too.
 * _verify: asynchronous on hip_stream; valid after _results and before the next _run, any number of
 *   times; Z_STREAM_ERROR otherwise and on a plan that never enabled verification.  d_input is the input
 *   the run read; d_output need not be the buffer the run wrote: a copy of it, with the plan's
 *   out_offsets, is verified just the same -- this is how a caller checks the stream where it finally
 *   rests.  Nothing is read outside [out_offsets[i], + out_caps[i]) (and the 64 readable bytes the layout
 *   guarantees) and [in_offsets[i], + source_lens[i]), whatever the bits say: a block whose decode would
 *   run past either fails with a reason.
 * _verify_results: waits for the last _verify; one result per buffer.  ms (may be NULL): the device time
 *   of that verification's launches, from HIP events on its stream.
 * _verify_blocks: the kept block map of one buffer of the last run, in stream order.  Z_BUF_ERROR, with
 *   *count the number needed, for a short cap; Z_DATA_ERROR and a count of 0 for a buffer whose status
 *   is not Z_OK. */
#define ZSC_HIP_VERIFY_OK          0
#define ZSC_HIP_VERIFY_SKIPPED    -1  /* the buffer's status was not Z_OK: nothing to verify */
#define ZSC_HIP_VERIFY_HEADER      1  /* stream header is not the plan's */
#define ZSC_HIP_VERIFY_BLOCK_HDR   2  /* BFINAL / BTYPE / LEN / NLEN / padding */
#define ZSC_HIP_VERIFY_CODES       3  /* dynamic header: invalid code set */
#define ZSC_HIP_VERIFY_LITERAL     4  /* a literal or stored byte differs from the input */
#define ZSC_HIP_VERIFY_DISTANCE    5  /* distance 0, before the input's start, or beyond the window */
#define ZSC_HIP_VERIFY_MATCH       6  /* the bytes a match copies are not the input's */
#define ZSC_HIP_VERIFY_LENGTH      7  /* the block passes or misses its input end, or an invalid symbol */
#define ZSC_HIP_VERIFY_BIT_END     8  /* the block does not end at the next block's first bit / the trailer */
#define ZSC_HIP_VERIFY_TRAILER     9  /* check value or ISIZE */

typedef struct { I32 verdict; U32 block; U32 bit_off; U32 in_pos; } zsc_hip_verify_result;
/* block: the failing block in stream order, 0xFFFFFFFF for OK / SKIPPED / HEADER / TRAILER;
 * bit_off: the block's first bit; in_pos: the input offset the check had reached */
typedef struct { U32 bit_off, in_begin, in_len, type_last; } zsc_hip_verify_block; /* type | last << 8 */

ZlibReturn zsc_hip_deflate_plan_verify_enable(zsc_hip_deflate_plan *plan);
ZlibReturn zsc_hip_deflate_plan_verify(zsc_hip_deflate_plan *plan, const void *d_input,
                                       const void *d_output, void *hip_stream);
ZlibReturn zsc_hip_deflate_plan_verify_results(zsc_hip_deflate_plan *plan,
                                               zsc_hip_verify_result *results, float *ms);
ZlibReturn zsc_hip_deflate_plan_verify_blocks(zsc_hip_deflate_plan *plan, U32 buffer,
                                              zsc_hip_verify_block *blocks, U32 cap, U32 *count);

/* device-resident inflate batches ------------------------------------------ */

/* Stream i occupies [src_offsets[i], +source_lens[i]) of the device input (offsets
 * multiples of 16, 64 readable bytes after the last stream) and decodes into
 * [dst_offsets[i], +dest_caps[i]) of the device output (offsets multiples of 16).
 * Results per stream as zsc_uncompress2 reports them: status, bytes written,
 * bytes consumed.  kernel_ms (may be NULL): device time of the last run from HIP
 * events on the run's stream. */
typedef struct zsc_hip_inflate_plan zsc_hip_inflate_plan;

ZlibReturn zsc_hip_inflate_plan_create(zsc_hip_inflate_plan **plan, U32 count,
                                       const U32 *source_lens, const uint64_t *src_offsets,
                                       const U32 *dest_caps, const uint64_t *dst_offsets,
                                       I32 window_bits);
/* The same with the order in which the streams are handed to the wavefronts given by the caller:
 * decode_order is a permutation of 0 .. count-1 (Z_STREAM_ERROR if it is not), NULL = the library's
 * own order (longest output first).  Four streams share a wavefront, so a caller that knows which
 * streams resemble each other can keep them apart or together; bench.py uses it to keep the replicas
 * of one member of its replicated batch from sharing wavefronts. */
ZlibReturn zsc_hip_inflate_plan_create_ordered(zsc_hip_inflate_plan **plan, U32 count,
                                               const U32 *source_lens, const uint64_t *src_offsets,
                                               const U32 *dest_caps, const uint64_t *dst_offsets,
                                               I32 window_bits, const U32 *decode_order);
ZlibReturn zsc_hip_inflate_plan_run(zsc_hip_inflate_plan *plan, const void *d_src, void *d_dst,
                                    void *hip_stream);
ZlibReturn zsc_hip_inflate_plan_results(zsc_hip_inflate_plan *plan, U32 *dest_lens,
                                        U32 *consumed, I32 *statuses, float *kernel_ms);
void zsc_hip_inflate_plan_destroy(zsc_hip_inflate_plan *plan);

/* Sections plans: the same arguments and plan type as zsc_hip_inflate_plan_create (_run, _results
 * and _destroy work unchanged), for streams written with Z_FULL_FLUSH every max_block_len bytes
 * (zsc_compress2 with max_block_len < source_len, or any encoder's full flushes).  A run first finds
 * each stream's byte-aligned 00 00 FF FF flush markers, decodes every section between them in a
 * lane group of its own, places the outputs at their offsets and checks the trailer by combining
 * the sections' Adler-32 / CRC-32 (zsc_amd/csrc/inflate_sections.h); then the serial decoder runs
 * over the plan as usual.  The parallel path only ever reports a clean Z_OK.  Every stream it cannot
 * finish that way is decoded serially from its start, exactly as zsc_hip_inflate_plan_create's plan
 * decodes it: a stream with no marker, a section that needs the output of an earlier one (e.g.
 * Z_SYNC_FLUSH), a data error anywhere (with its inflateSync resynchronisation), Z_NEED_DICT,
 * truncation, a short dest_caps[i], a trailer or ISIZE mismatch, more than source_len / 32 + 8
 * candidate markers, a used-up candidate pool (below), or a count pass that has decoded more than 4 * source_len + 64 KiB input bytes
 * from the stream's candidates (false markers inside stored data or a gzip header are decoded and
 * thrown away; this bounds the work they cause; groups already decoding when the bound is reached
 * finish their candidate).  So status, output bytes and consumed equal the plain plan's for every
 * input.  kernel_ms of _results covers all launches of a run.  Scratch, held from create to destroy
 * (zsc_hip_inflate_plan_scratch_bytes): 28 bytes per slot of one candidate pool of
 * (sum of source_lens) / 256 + 65 536 slots, taken at run time only by streams that have markers
 * (a stream that finds the pool used up is decoded serially), 16 bytes per 4 KiB of input and
 * 100 bytes per stream. */
ZlibReturn zsc_hip_inflate_plan_create_sections(zsc_hip_inflate_plan **plan, U32 count,
                                                const U32 *source_lens, const uint64_t *src_offsets,
                                                const U32 *dest_caps, const uint64_t *dst_offsets,
                                                I32 window_bits);
/* after _results: per stream, the number of sections (or pieces, of a chunks plan) decoded in parallel;
 * 0 for streams the serial decoder produced (and for every stream of a plain plan) */
ZlibReturn zsc_hip_inflate_plan_sections(zsc_hip_inflate_plan *plan, U32 *sections);
/* bytes of device scratch a sections, chunks, resync or indexed plan holds beyond a plain plan's (0 for a
 * plain plan) */
uint64_t zsc_hip_inflate_plan_scratch_bytes(const zsc_hip_inflate_plan *plan);

/* zsc_hip_uncompress_batch through a sections plan: the same signature and per-item semantics */
ZlibReturn zsc_hip_uncompress_sections_batch(U32 count, const U8 *const *sources, U32 *source_lens,
                                             U8 *const *dests, U32 *dest_lens, I32 *statuses,
                                             I32 window_bits);

/* Chunks plans: the arguments of zsc_hip_inflate_plan_create_sections plus chunk_bytes, the compressed
 * bytes per piece the plan aims at (0: the default, 128 KiB, chosen from a sweep over 32 KiB to 1 MiB
 * on one 1 GiB-output stream; values below 4 KiB are taken as 4 KiB).  For any stream, whoever
 * wrote it: each stream longer than chunk_bytes (with dest_caps[i] < 2 GiB) is cut into chunks of
 * chunk_bytes input bytes; a run finds candidate block starts in each chunk by trial (dynamic-Huffman
 * headers at any bit offset, ends of stored blocks), decodes from them with placeholders for the
 * unknown window before each piece, chains the pieces from the stream's start, passes the 32 KiB
 * windows from piece to piece and decodes every chained piece again into place
 * (zsc_amd/csrc/inflate_chunks.h); then the serial decoder runs over the plan as usual.  _run,
 * _results, _destroy, zsc_hip_inflate_plan_sections (pieces decoded in parallel per stream, 0 for
 * serial) and zsc_hip_inflate_plan_scratch_bytes work on it.  As with sections plans the parallel path
 * only ever reports a clean Z_OK; every stream it cannot finish that way -- a data error anywhere,
 * Z_NEED_DICT, truncation, a short dest_caps[i], a trailer or ISIZE mismatch, a chain broken by a
 * missed or false candidate, a reach before the output or beyond the header's window, a count pass
 * that has decoded more than 4 * source_len + 64 KiB input bytes -- is decoded serially from its
 * start, so status, output bytes and consumed equal the plain plan's for every input.  Scratch, held
 * from create to destroy: 98 372 bytes per chunk of the streams longer than chunk_bytes (a 64 KiB
 * ring of 16-bit symbols, a 32 KiB window, 32 bytes of candidates, 36 bytes of records), 8 bytes per
 * chunk after a stream's first, and 96 bytes per stream plus 16. */
ZlibReturn zsc_hip_inflate_plan_create_chunks(zsc_hip_inflate_plan **plan, U32 count,
                                              const U32 *source_lens, const uint64_t *src_offsets,
                                              const U32 *dest_caps, const uint64_t *dst_offsets,
                                              I32 window_bits, U32 chunk_bytes);
/* zsc_hip_uncompress_batch through a chunks plan (default chunk_bytes): the same signature and
 * per-item semantics */
ZlibReturn zsc_hip_uncompress_chunks_batch(U32 count, const U8 *const *sources, U32 *source_lens,
                                           U8 *const *dests, U32 *dest_lens, I32 *statuses,
                                           I32 window_bits);

/* Resync plans: the same arguments as zsc_hip_inflate_plan_create_sections; a sections plan that also
 * finishes damaged streams in parallel.  Where a section ends in a data error, the run does what
 * zsc_uncompress does (inflateSync): it looks for the next 00 00 FF FF -- in what the bit buffer held,
 * then in the input -- and goes on decoding behind it, so the stream ends with Z_DATA_ERROR, the
 * output salvaged, the reference's consumed count and its number of data errors
 * (zsc_amd/csrc/inflate_resync.h).  Every stream the path cannot finish that way is decoded serially
 * from its start: everything a sections plan sends there except the data errors and their
 * resynchronisation, and besides an error in the zlib / gzip header, a data error where the output has
 * reached dest_caps[i], a resynchronisation that lands where no section was decoded, a distance beyond the
 * output of a section entered at a marker, a pattern inside or behind a failing trailer, and more data
 * errors than the reference's loop allows (max(dest_caps[i], 10) inflate() calls).  So status, output
 * bytes and consumed equal the plain plan's for every input.  _run, _results, _destroy,
 * zsc_hip_inflate_plan_sections (chain entries decoded in parallel, a damaged section's partial one
 * included; 0 for serial) and zsc_hip_inflate_plan_scratch_bytes work on it.  Scratch: a sections
 * plan's, plus 12 bytes per candidate pool slot and 16 bytes per stream. */
ZlibReturn zsc_hip_inflate_plan_create_resync(zsc_hip_inflate_plan **plan, U32 count,
                                              const U32 *source_lens, const uint64_t *src_offsets,
                                              const U32 *dest_caps, const uint64_t *dst_offsets,
                                              I32 window_bits);
/* zsc_hip_uncompress_batch through a resync plan: the same signature and per-item semantics */
ZlibReturn zsc_hip_uncompress_resync_batch(U32 count, const U8 *const *sources, U32 *source_lens,
                                           U8 *const *dests, U32 *dest_lens, I32 *statuses,
                                           I32 window_bits);
/* after _results, for every plan kind: per stream, the data errors the reference's zsc_uncompress loop
 * counts (one per inflate() call that returned Z_DATA_ERROR; it only warns of them).  0 for a stream
 * that decoded cleanly. */
ZlibReturn zsc_hip_inflate_plan_data_errors(zsc_hip_inflate_plan *plan, U32 *errors);

/* Size plans: what dest_caps[i] has to be, found on the device without writing any output
 * (zsc_amd/csrc/inflate_size.h).  A zlib or raw stream does not carry its length, and a gzip ISIZE is a
 * number modulo 2^32 at the end of a file not yet trusted; a size plan decodes the streams as a plain
 * plan does and stores nothing.  source_lens, src_offsets and window_bits as zsc_hip_inflate_plan_create.
 * dest_limits[i] is the most stream i may inflate to (NULL: 0xFFFFFFFF for every stream).  chunk_bytes
 * as zsc_hip_inflate_plan_create_chunks (0: the default; below 4 KiB: 4 KiB): a stream longer than that
 * is sized in pieces, in parallel; 0xFFFFFFFF never cuts a stream.
 *
 * The contract.  Status, dest_len and consumed of stream i (_results) are those a plain plan
 * (zsc_hip_inflate_plan_create) reports with dest_caps[i] = dest_limits[i], for every input, damaged and
 * truncated ones included: header rules, invalid code sets and symbols, a distance beyond the output so
 * far or beyond the header's window, truncation (Z_BUF_ERROR), Z_NEED_DICT, data errors survived through
 * inflateSync (Z_DATA_ERROR, zsc_hip_inflate_plan_data_errors) and a gzip ISIZE that is not the length
 * are all found.  A stream longer than its limit is Z_BUF_ERROR with dest_len equal to the limit, as the
 * plain plan gives it: the limit is a guard against decompression bombs.
 *   The one exception: the check value in a zlib or gzip trailer is not compared, because there are no
 *   bytes to take it over.  A stream whose only fault is its Adler-32 or CRC-32 is reported Z_OK with
 *   its full length, and consumed is the trailer's end; inflating it afterwards reports the fault.
 *   (Where a data error has been survived, the salvaged output cannot match the writer's check value, and
 *   the check is taken as failed, as a plain plan finds it.)  A check plan (below) compares the check value
 *   too, and hands it out.
 *
 * _run (d_dst is ignored and may be NULL: nothing is ever written through it), _results, _destroy,
 * zsc_hip_inflate_plan_sections (the pieces a stream was sized in, in parallel, or 0),
 * zsc_hip_inflate_plan_data_errors and zsc_hip_inflate_plan_scratch_bytes work on it;
 * zsc_hip_inflate_plan_pack_enable and zsc_hip_inflate_plan_index_enable return Z_STREAM_ERROR.  As with
 * chunks plans the parallel path only ever reports a clean Z_OK; a stream it cannot finish -- a broken
 * chain, a reach before the output or beyond the header's window, the 4 * source_len + 64 KiB work
 * bound, a total above the limit, an ISIZE mismatch, any error -- is sized by the whole-stream decode
 * from its start.  Scratch: 64 bytes per chunk of the streams longer than chunk_bytes (32 bytes of
 * candidates, 32 bytes of records; no ring and no window), 8 bytes per chunk after a stream's first, and
 * 96 bytes per stream plus 16.  A plan of any other kind allocates, launches and returns what it did
 * without size plans. */
ZlibReturn zsc_hip_inflate_plan_create_size(zsc_hip_inflate_plan **plan, U32 count,
                                            const U32 *source_lens, const uint64_t *src_offsets,
                                            const U32 *dest_limits, I32 window_bits, U32 chunk_bytes);
/* host-pointer batch through a size plan (default chunk_bytes).  dest_lens: in, the limits; out, the
 * sizes.  source_lens: out, the bytes consumed.  statuses may be NULL. */
ZlibReturn zsc_hip_uncompress_sizes_batch(U32 count, const U8 *const *sources, U32 *source_lens,
                                          U32 *dest_lens, I32 *statuses, I32 window_bits);

/* Check plans: "is this archive intact?" answered on the device without writing any output
 * (zsc_amd/csrc/inflate_check.h) -- gzip -t for a batch.  A check plan decodes the streams as a plain plan
 * does, keeps only the last window of each output in a 64 KiB ring owned by the lane group that decodes it,
 * and folds the output into the running Adler-32 / CRC-32 before the ring wraps over it.  Arguments as
 * zsc_hip_inflate_plan_create_size: dest_limits[i] is the most stream i may inflate to (NULL: 0xFFFFFFFF
 * for every stream), a stream longer than chunk_bytes is checked in pieces, in parallel (0: the default;
 * below 4 KiB: 4 KiB; 0xFFFFFFFF never cuts a stream).
 *
 * The contract.  Status, dest_len and consumed of stream i (_results) are exactly those a plain plan
 * (zsc_hip_inflate_plan_create) reports with dest_caps[i] = dest_limits[i], for every input: a wrong
 * Adler-32 or CRC-32 is Z_DATA_ERROR as a wrong ISIZE is, and a stream longer than its limit is
 * Z_BUF_ERROR with dest_len equal to the limit.
 *
 * _run (d_dst is ignored and may be NULL: nothing is ever written through it), _results, _destroy,
 * zsc_hip_inflate_plan_sections (the pieces a stream was checked in, in parallel, or 0),
 * zsc_hip_inflate_plan_data_errors and zsc_hip_inflate_plan_scratch_bytes work on it;
 * zsc_hip_inflate_plan_pack_enable and zsc_hip_inflate_plan_index_enable return Z_STREAM_ERROR.  As with
 * chunks plans the parallel path only ever reports a clean Z_OK; a stream it cannot finish -- a check value
 * that does not match, a broken chain, a limit passed, the work bound, any error -- is checked by the
 * whole-stream decode from its start.  (A stream of 2 GiB or more of output is always left to that decode.)
 * Scratch does not depend on dest_limits: 65 536 bytes per lane group of the launch -- four to a wavefront;
 * wavefronts: a quarter of count, rounded up, and no more than fill the device -- a chunks plan's scratch
 * for the streams longer than chunk_bytes (98 372 bytes per chunk; 8 per chunk after a stream's first,
 * and at least 8), 4 bytes per stream for the check values, and 96 bytes per stream plus 16.  The
 * environment variable
 * ZSC_HIP_CHECK_GROUPS, read when the plan is created, caps the lane groups (rounded up to a whole
 * wavefront): a test hook that makes every ring serve several streams.  A plan of any other kind
 * allocates, launches and returns what it did without check plans. */
ZlibReturn zsc_hip_inflate_plan_create_check(zsc_hip_inflate_plan **plan, U32 count,
                                             const U32 *source_lens, const uint64_t *src_offsets,
                                             const U32 *dest_limits, I32 window_bits, U32 chunk_bytes);
/* The check value computed over the output of every stream of a check plan whose status is Z_OK -- CRC-32
 * for a gzip stream, Adler-32 for a zlib or a raw one (the index blob's convention) -- and 0 for every
 * other stream.  After _run; it waits for the run as _results does.  Z_STREAM_ERROR for a plan of any other
 * kind and before the first run. */
ZlibReturn zsc_hip_inflate_plan_check_values(zsc_hip_inflate_plan *plan, U32 *values);
/* host-pointer batch through a check plan (default chunk_bytes).  dest_lens: in, the limits; out, the
 * lengths.  source_lens: out, the bytes consumed.  statuses and check_values may be NULL. */
ZlibReturn zsc_hip_uncompress_check_batch(U32 count, const U8 *const *sources, U32 *source_lens,
                                          U32 *dest_lens, I32 *statuses, U32 *check_values, I32 window_bits);

/* Members plans: multi-member gzip files -- the output of zsc_hip_deflate_plan_pack with align 1 over a gzip
 * plan, BGZF, `cat a.gz b.gz`, pigz -i -- inflated member by member, in parallel
 * (zsc_amd/csrc/inflate_members.h).  Every other inflate plan, like zsc_uncompress, stops at the end of the
 * first member.  Arguments as zsc_hip_inflate_plan_create; item i is one file, source_lens[i] bytes at
 * src_offsets[i], decoded to [dst_offsets[i], + dest_caps[i]).  window_bits must select the gzip wrapper
 * (16 + 8 .. 16 + 15); anything else, and an unknown flag, is Z_STREAM_ERROR.  Files above 4 GiB of input or
 * output are not served (the lengths are U32).
 *
 * The contract.  The result of file i is that of this walk:
 *     at = 0; out = 0; members = 0
 *     loop: (rc, len, used) = what a plain plan (zsc_hip_inflate_plan_create) reports for the stream
 *                             file[at:] with dest cap dest_caps[i] - out and the plan's window_bits
 *           out += len; at += used
 *           if rc != Z_OK: return (rc, out, at, members)
 *           members += 1
 *           if fewer than 2 bytes remain at `at`, or they are not 1f 8b: return (Z_OK, out, at, members)
 * Status, dest_len and consumed (_results) are the walk's rc, out and at.  A file stops at its first member
 * that is not Z_OK; that member's salvaged bytes are counted, and its inflateSync resynchronisation is what
 * the plain plan does on file[at:] (zsc_hip_inflate_plan_data_errors reports that member's count).  Zero
 * padding or other bytes behind the last member end the file with Z_OK; consumed says where.  Nothing outside
 * a file's own [dst_offsets[i], + dest_caps[i]) is written, whatever the file holds, and nothing is read
 * outside [src_offsets[i], + source_lens[i]) plus the 64 readable bytes every inflate input has behind it.
 *
 * A run scans the files for 1f 8b 08 with the reserved FLG bits clear (candidate member starts), decodes
 * every candidate as one whole member with nothing stored, follows the chain of clean members from offset 0
 * while it stays inside dest_caps[i], decodes every chained member again into its place with the plain
 * decode, and keeps the verified prefix: the chain entries before the first one whose second decode did not
 * give Z_OK with exactly the counted length and end.  A file whose prefix reaches the walk's end is finished;
 * every other file -- a member that is not Z_OK, a short dest_caps[i], a header the scan does not take for
 * one (a method other than 8, reserved FLG bits), more than source_len / 16 + 8 candidates or a used-up
 * candidate pool (prefix 0), a count pass that has decoded more than 4 * source_len + 64 KiB input bytes of
 * the file's candidates (prefix 0; a gzip file stored inside a gzip member makes candidates off the chain) --
 * is taken up by one lane group at the end of its verified prefix and walked serially to its end.
 *   Claims.  A member whose FEXTRA holds a subfield `B` `C` of length 2 says how long it is (BSIZE + 1, the
 *   BGZF convention).  Where that end lies inside the file and the ISIZE in front of it is at most 65 536,
 *   the first decode is skipped and stop and length are taken from the header and trailer.  A claim is never
 *   trusted: the second decode runs in a slice of exactly the claimed length and must reproduce length and
 *   end, or the verified prefix ends in front of that member.  So a BGZF file is decoded once, any other file
 *   twice.  The environment variable ZSC_HIP_MEMBERS_CLAIMS=0, read when the plan is created, switches
 *   claims off (a test hook and the A/B switch); results do not depend on it.
 *
 * flags: 0, or ZSC_HIP_MEMBERS_SIZE_ONLY: nothing is written and d_dst is ignored (it may be NULL), as are
 * dst_offsets; dest_caps are limits (NULL: 0xFFFFFFFF for every file).  Each member of the walk then follows
 * the size plan's contract instead of the plain plan's, with its one exception: the CRC-32 is not compared, so
 * a member whose only fault is its CRC-32 is Z_OK and the walk goes on.  Size-only mode does not use claims:
 * every member is decoded (once), never trusted -- there is no second decode to hold a claim against.
 *
 * _run, _results, _destroy, zsc_hip_inflate_plan_scratch_bytes, zsc_hip_inflate_plan_data_errors and
 * zsc_hip_inflate_plan_pack_enable / _pack (not in size-only mode) work on it;
 * zsc_hip_inflate_plan_index_enable returns Z_STREAM_ERROR.  zsc_hip_inflate_plan_sections reports the
 * verified prefix: the members decoded by the parallel path.  kernel_ms of _results covers all launches of
 * a run; _results relaunches nothing.  Scratch, held from create to destroy: 28 bytes (size-only: 24) per
 * slot of one candidate pool of (sum of source_lens) / 256 + 65 536 slots, taken at run time by the files'
 * candidates, 16 bytes per 4 KiB of input, and 116 bytes per file plus 16.  A plan of any other kind
 * allocates, launches and returns what it did without members plans. */
#define ZSC_HIP_MEMBERS_SIZE_ONLY 1u
ZlibReturn zsc_hip_inflate_plan_create_members(zsc_hip_inflate_plan **plan, U32 count,
                                               const U32 *source_lens, const uint64_t *src_offsets,
                                               const U32 *dest_caps, const uint64_t *dst_offsets,
                                               I32 window_bits, U32 flags);
/* after _results, of a members plan (Z_STREAM_ERROR for any other): per file, the walk's member count (the
 * members that were Z_OK) and how many members of the verified prefix were claimed.  Either may be NULL. */
ZlibReturn zsc_hip_inflate_plan_members(zsc_hip_inflate_plan *plan, U32 *members, U32 *claimed);
/* zsc_hip_uncompress_batch through a members plan: the same signature and per-item semantics, every source
 * a multi-member file; members (may be NULL): out, the walk's member count per file */
ZlibReturn zsc_hip_uncompress_members_batch(U32 count, const U8 *const *sources, U32 *source_lens,
                                            U8 *const *dests, U32 *dest_lens, I32 *statuses,
                                            I32 window_bits, U32 *members);

/* seek-point indexes -------------------------------------------------------- */

/* A chunks plan finds, on every run, where the chained pieces of a stream start, how long each one's
 * output is and which bytes before its start it reads.  With the index enabled it can hand these facts
 * out as one blob per stream, to be kept beside the archive; an indexed plan decodes from the blob with
 * none of the discovery, and can decode a range out of the middle (zsc_amd/csrc/inflate_index.h,
 * DESIGN.md section 10).
 *
 * The blob.  Little-endian, self-contained, version 1.  The density of the index is the exporting plan's
 * chunk_bytes: one point per chained piece.
 *   header, 48 bytes
 *      0  u32  magic 0x4943535A ("ZSCI")
 *      4  u32  format version, 1
 *      8  u32  CRC-32 (the gzip polynomial) of blob[12 .. length)
 *     12  i32  window_bits the stream was decoded with
 *     16  u32  wrapper kind: 0 raw, 1 zlib, 2 gzip
 *     20  u32  bit 0: the header is a gzip header; bits 8-12: log2 of the header's distance limit
 *     24  u32  chunk_bytes of the exporting plan (at least 256)
 *     28  u32  consumed: the trailer's end, as the plain plan reports it
 *     32  u32  total output bytes
 *     36  u32  byte offset of the trailer (consumed less 0 / 4 / 8 bytes for raw / zlib / gzip)
 *     40  u32  number of points, at least 1
 *     44  u32  reserved, 0
 *   points, 32 bytes each, from offset 48, in chain order; the first is the stream's start
 *      0  u64  where the piece starts, as a bit offset into the stream (0 for the first)
 *      8  u64  where its window lies, as a byte offset into the blob
 *     16  u32  output offset
 *     20  u32  output length
 *     24  u32  check value of the piece's own output: CRC-32 for gzip streams, Adler-32 for zlib and raw ones
 *     28  u32  length of its window: how far the piece reaches before its start, at most 32 768 (0 for the first)
 *   windows, from the end of the points to the end of the blob, in point order without gaps: the last
 *   `window length` output bytes before each piece.
 * A blob is valid if magic, version and CRC are right; the wrapper kind fits window_bits and the gzip bit;
 * the points ascend strictly in bit offset and in chunk (bit offset / (8 * chunk_bytes)), so at most one
 * lies in a chunk; the output offsets are the running sum of the lengths and end at the total; each window
 * is no longer than 32 KiB or than the output before its piece, and lies where the layout above puts it;
 * and the trailer's offset lies at or behind the last point. */
typedef struct {
    I32 window_bits;
    U32 wrapper;        /* 0 raw, 1 zlib, 2 gzip */
    U32 gzip;           /* the header is a gzip header */
    U32 dist_limit;     /* the header's distance limit in bytes */
    U32 chunk_bytes;
    U32 consumed;
    U32 total_out;
    U32 trailer_offset;
    U32 points;
} zsc_hip_index_header;

/* Host functions; none needs a device.  Z_OK, or Z_DATA_ERROR for a blob that is not valid. */
ZlibReturn zsc_hip_index_validate(const U8 *blob, uint64_t len);
ZlibReturn zsc_hip_index_info(const U8 *blob, uint64_t len, zsc_hip_index_header *info);
/* The smallest run of whole pieces that covers output bytes [out_begin, out_begin + out_len): its first
 * piece, the number of pieces, and the output range [piece_begin, piece_begin + piece_len) they produce
 * (any of the four may be NULL).  Z_STREAM_ERROR for an empty range or one not inside the output. */
ZlibReturn zsc_hip_index_range(const U8 *blob, uint64_t len, uint64_t out_begin, uint64_t out_len,
                               U32 *first_piece, U32 *piece_count, U32 *piece_begin, U32 *piece_len);

/* Export.  zsc_hip_inflate_plan_index_enable: chunks plans only (Z_STREAM_ERROR for any other kind),
 * before _run.  A plan that never enables it launches, holds and returns what it always did; with it
 * enabled the write pass takes the slice check values of raw streams too, and nothing else changes.
 * _index_size and _index_export are valid after _results and before the next _run: Z_OK and the blob for
 * a stream the run finished in parallel (zsc_hip_inflate_plan_sections > 0); Z_DATA_ERROR and 0 bytes for
 * a stream the serial decoder produced; Z_BUF_ERROR (and *len the bytes needed) for a short cap.  The
 * windows are gathered on the device into one buffer (temporary, sized by a prefix sum of their lengths),
 * so a blob costs one device-to-host copy of records and one of windows. */
ZlibReturn zsc_hip_inflate_plan_index_enable(zsc_hip_inflate_plan *plan, I32 enable);
ZlibReturn zsc_hip_inflate_plan_index_size(zsc_hip_inflate_plan *plan, U32 stream, uint64_t *bytes);
ZlibReturn zsc_hip_inflate_plan_index_export(zsc_hip_inflate_plan *plan, U32 stream, U8 *blob, uint64_t cap,
                                             uint64_t *len);

/* Indexed plans: the arguments of zsc_hip_inflate_plan_create, plus per stream a blob (indexes[i],
 * index_lens[i]; indexes == NULL or indexes[i] == NULL: no index) and optionally a range of the output
 * (range_begins[i], range_lens[i]; a NULL array or a length of all ones: the whole stream).  _run,
 * _results, _destroy, zsc_hip_inflate_plan_sections (the pieces decoded from the index, or 0) and
 * zsc_hip_inflate_plan_scratch_bytes work on it.  Create validates every blob on the host, uploads points
 * and windows once and orders the pieces of all streams by output length, longest first.  A run decodes
 * every piece into place from its point with its window (k_idx_write), combines the pieces' check values
 * and compares them with the stream's trailer and ISIZE (k_sec_finish), and then runs the serial decoder
 * over the plan (k_inflate): no scan, count, retry, resolve or window launch.
 *
 * Whole streams follow the rule of the sections and chunks plans: the path only ever reports a clean
 * Z_OK, and every other stream is decoded serially from its start -- a blob that is not valid or belongs
 * to another stream, source_lens[i] below the index's consumed, a window_bits other than the index's, a
 * short dest_caps[i], a piece that does not stop exactly at the next point (the last: at the indexed
 * trailer offset), produces another length or check value, reaches back further or less far than its
 * window is long or beyond the header's distance limit, a header other than the index says, a trailer or
 * ISIZE mismatch.  So status, output bytes and consumed equal the plain plan's for every stream and every
 * blob, with one exception: a raw stream has no trailer, and a range is checked against the index alone,
 * so for them an index whose windows and piece check values were altered consistently cannot be told
 * from a true one.  For a raw stream or a range the index is trusted as the stream's source is; the
 * blob's CRC guards against accidents, not against intent.
 *
 * Ranges: the item decodes only the pieces zsc_hip_index_range names, to dst_offsets[i]; dest_caps[i]
 * must hold piece_len.  On success Z_OK, dest_len = piece_len, consumed = the byte behind the last bit
 * read.  There is no serial fallback (the destination is not sized for one): any disagreement, or a
 * stream without a valid index, gives Z_DATA_ERROR (Z_BUF_ERROR for a dest_caps[i] below piece_len) with
 * dest_len 0 and consumed 0.  A range that is empty or not inside the output: Z_STREAM_ERROR at create.
 *
 * Whatever a blob holds, the device reads nothing outside the plan's own allocations: every offset is
 * checked at create, and the windows lie packed in one buffer behind 32 KiB of zeros, each ending where
 * a full window would, so a piece that reaches beyond its window's length (a distance is at most 32 768)
 * reads that buffer's earlier bytes and fails.  Scratch, held from create to destroy: 64 bytes per piece,
 * the windows' bytes plus 32 KiB, 32 bytes per chunk up to the last point a stream's pieces stop at, and
 * 232 bytes per stream plus 32. */
ZlibReturn zsc_hip_inflate_plan_create_indexed(zsc_hip_inflate_plan **plan, U32 count,
                                               const U32 *source_lens, const uint64_t *src_offsets,
                                               const U32 *dest_caps, const uint64_t *dst_offsets,
                                               I32 window_bits, const U8 *const *indexes,
                                               const uint64_t *index_lens, const uint64_t *range_begins,
                                               const uint64_t *range_lens);
/* zsc_hip_uncompress_batch through an indexed plan (whole streams only): the same signature and per-item
 * semantics, plus the blobs */
ZlibReturn zsc_hip_uncompress_indexed_batch(U32 count, const U8 *const *sources, U32 *source_lens,
                                            U8 *const *dests, U32 *dest_lens, I32 *statuses,
                                            I32 window_bits, const U8 *const *indexes,
                                            const uint64_t *index_lens);

/* packed images ---------------------------------------------------------------- */

/* A plan leaves item i where its layout put it: at out_offsets[i] (deflate) or dst_offsets[i] (inflate), in a
 * slot sized for the worst case, and how long each item is, is known on the device only.  Packing moves the
 * items of the last run into ONE dense image, item after item, with a table of offsets, without a trip to the
 * host in between (zsc_amd/csrc/pack.h): an exclusive prefix sum of the lengths on the
 * device -- reduce, scan of the sums and apply as launches of their own, one to seven of them by count -- and
 * one launch that moves the bytes, a wavefront per ZSC_HIP_PACK_TILE bytes of the image.
 *
 * The length of an item is read from the plan's result records on the device: of a deflate plan out_len where
 * the status is Z_OK and 0 otherwise; of an inflate plan the dest_len that _results reports, whatever the
 * status, so that the salvaged output of a damaged stream is kept.
 *
 * align: a power of two from 1 to 4096 (anything else: Z_STREAM_ERROR); every item starts at a multiple of it
 *   and the bytes between an item's end and the next start are written as zeros, so the image is a function
 *   of the items alone.  16 or more gives offsets an inflate plan takes as its src_offsets (the image then
 *   needs 64 readable bytes behind it, as every inflate input does); 1 gives an archive -- gzip streams packed
 *   with align 1 are a valid multi-member gzip file.
 *
 * _pack_enable: before _run, for plans of every kind (deflate: Z_STREAM_ERROR for a plan of sections).
 *   Allocates 16 bytes per item (the dense offsets and the slots' offsets), 8 more for the total and 8 per
 *   1 024 items for the scan's partial sums, counted in _scratch_bytes.  Calling it again with another align
 *   only changes the align.  A plan that never enables packing allocates, launches and returns exactly what
 *   it did without these functions.  The index and verification of a deflate plan may be enabled too; they
 *   keep referring to the plan's own out_offsets, that is to the stream where the run wrote it, not to the
 *   packed image.
 * _pack: asynchronous on hip_stream; enqueues kernels only -- no allocation, no synchronisation, no copy from
 *   or to the host.  Valid after a _run on the same stream or after _results, any number of times (an inflate
 *   plan that resynchronises damaged streams finishes them in _results: pack such a plan after _results).
 *   d_output is the run's output or a copy of it at the plan's offsets, as with _verify; of each item the
 *   pack reads the whole 16-byte granules that hold one of its bytes, so never before its slot and at most 15
 *   bytes behind its end.  d_packed is 16-byte aligned and packed_cap bytes long: bytes [0, total) are each
 *   written exactly once and nothing at or behind total; with total > packed_cap nothing is written at all.
 * _pack_results: waits for the last _pack.  offsets[i] (may be NULL): where item i starts, offsets[count] ==
 *   *total; ms (may be NULL): the device time of that pack's launches, from HIP events on its stream.
 *   Z_BUF_ERROR where total > packed_cap -- offsets and total are filled all the same, so that the caller can
 *   size another _pack --; Z_STREAM_ERROR on a plan that never enabled packing or never packed. */
#define ZSC_HIP_PACK_TILE 16384 /* bytes of the image one wavefront moves */

ZlibReturn zsc_hip_deflate_plan_pack_enable(zsc_hip_deflate_plan *plan, U32 align);
ZlibReturn zsc_hip_deflate_plan_pack(zsc_hip_deflate_plan *plan, const void *d_output, void *d_packed,
                                     uint64_t packed_cap, void *hip_stream);
ZlibReturn zsc_hip_deflate_plan_pack_results(zsc_hip_deflate_plan *plan, uint64_t *offsets, uint64_t *total,
                                             float *ms);
ZlibReturn zsc_hip_inflate_plan_pack_enable(zsc_hip_inflate_plan *plan, U32 align);
ZlibReturn zsc_hip_inflate_plan_pack(zsc_hip_inflate_plan *plan, const void *d_output, void *d_packed,
                                     uint64_t packed_cap, void *hip_stream);
ZlibReturn zsc_hip_inflate_plan_pack_results(zsc_hip_inflate_plan *plan, uint64_t *offsets, uint64_t *total,
                                             float *ms);

/* The other way, without a plan: item i, lens[i] bytes at packed_offsets[i] of the image d_packed (16-byte
 * aligned base, offsets of any alignment), goes to [dst_offsets[i], + lens[i]) of d_dst, and no other byte of
 * d_dst is written.  The items lie in the image in ascending order without overlap (packed_offsets[i] +
 * lens[i] <= packed_offsets[i + 1]; what lies between them is skipped) and dst_offsets are multiples of 16:
 * Z_STREAM_ERROR otherwise.  Nothing of the image is read at or behind the last item's end.  The three host
 * arrays are uploaded before the call returns; the launch is asynchronous on hip_stream. */
ZlibReturn zsc_hip_unpack(U32 count, const void *d_packed, const uint64_t *packed_offsets, const U32 *lens,
                          void *d_dst, const uint64_t *dst_offsets, void *hip_stream);

/* Host images: zsc_hip_compress_batch / zsc_hip_uncompress_batch for a caller whose items lie in one host
 * buffer -- one copy to the device and one back, whatever count is, where the pointer batches do one per item
 * each way.  The image is uploaded with one hipMemcpy, unpacked into a plan's layout, the same plan as the
 * pointer batch's runs, its results are packed and bytes [0, total) come back with one hipMemcpy.  Statuses
 * (and consumed) are those of the pointer batches given enough room.
 *
 * zsc_hip_compress_batch_packed: buffer i is sources[source_offsets[i] .. source_offsets[i + 1]); stream i is
 *   dest[dest_offsets[i] ...], dest_offsets[count] the image's length.  There is no capacity per item: the call
 *   returns Z_BUF_ERROR where dest_cap is less than the image's length, with dest_offsets filled and dest
 *   untouched.  Level 0 is Z_STREAM_ERROR (the store path hands out no plan).
 * zsc_hip_uncompress_batch_packed: stream i is source_lens[i] bytes at sources[source_offsets[i]] (ascending,
 *   no overlap); dest_caps[i] is the most it may decode to, as dest_lens[i] on entry of
 *   zsc_hip_uncompress_batch; output i is dest_lens[i] bytes at dest[dest_offsets[i]]. */
ZlibReturn zsc_hip_compress_batch_packed(U32 count, const U8 *sources, const uint64_t *source_offsets, U8 *dest,
                                         uint64_t dest_cap, uint64_t *dest_offsets, I32 *statuses, I32 level,
                                         I32 window_bits, I32 mem_level, ZlibStrategy strategy, U32 align);
ZlibReturn zsc_hip_uncompress_batch_packed(U32 count, const U8 *sources, const uint64_t *source_offsets,
                                           const U32 *source_lens, const U32 *dest_caps, U8 *dest,
                                           uint64_t dest_cap, uint64_t *dest_offsets, U32 *dest_lens,
                                           U32 *consumed, I32 *statuses, I32 window_bits, U32 align);

/* BGZF files --------------------------------------------------------------------
 *
 * A gzip deflate plan's streams written out as BGZF files -- the block-gzip container of bgzip, BAM and tabix --
 * on the device (zsc_amd/csrc/bgzf.h).  A file is a run of consecutive buffers of the
 * plan, file_first[f] .. file_first[f + 1] (a run may be empty); its image is one member per buffer, in buffer
 * order, and the 28 bytes that end a BGZF file:
 *
 *   member header (18): 1f 8b 08 04 | 00 00 00 00 | XFL | ff | 06 00 | 42 43 02 00 | BSIZE lo, hi
 *      XFL   = byte 8 of the plan's own stream for that buffer
 *      BSIZE = the member's length - 1; the member of a stream of out_len bytes is L = out_len + 8 bytes long
 *   member body:        the plan's stream from byte 10 to its end (deflate data, CRC-32, ISIZE), unchanged
 *   end of file (28):   1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43 02 00 1b 00 03 00 00 00 00 00 00 00 00 00
 *
 * which is byte for byte what the reference writes when it is given that FEXTRA field in a gz_header.  Files
 * start at multiples of align (a power of two from 1 to 4096, as with _pack) and the bytes from a file's end to
 * the next file's start are zeros.  A file FAILS with Z_BUF_ERROR where one of its buffers has a status other
 * than Z_OK or an L above 65 536 (BSIZE has 16 bits; the caller picks shorter buffers): it takes no room in the
 * image, like a failed item of _pack, and the other files are what they are without it.  A members plan
 * (zsc_hip_inflate_plan_create_members) reads such a file by its BSIZE fields, each member decoded once.
 *
 * _bgzf_enable: before _run.  Z_STREAM_ERROR, with the plan left as it was, for a plan whose wrapper is not
 *   gzip, a plan of sections, a source_lens[i] above 65 536, a file_first that does not ascend from 0 to count,
 *   or a bad align.  Calling it again replaces the partition.  Allocates 20 bytes per buffer and 24 per file,
 *   and 8 per 1 024 files for the scan's partial sums, counted in _scratch_bytes.  Independent of _pack_enable,
 *   _index_enable and _verify_enable: all may be on.  A plan that never calls it allocates and launches exactly
 *   what it did without these functions.
 * _bgzf: asynchronous on hip_stream; enqueues kernels only -- no allocation, no synchronisation, no copy from
 *   or to the host.  Valid after a _run on the same stream or after _results, any number of times.  d_output is
 *   the run's output or a copy of it at the plan's offsets; of each stream the whole 16-byte granules that hold
 *   one of its bytes are read.  d_image is 16-byte aligned and image_cap bytes long: bytes [0, total) are each
 *   written exactly once and nothing at or behind total; with total > image_cap nothing is written at all.
 *   Ordered against the plan's runs like a pack (see "Streams").
 * _bgzf_results: waits for the last _bgzf.  Every pointer may be NULL.  file_offsets[f]: where file f starts,
 *   file_offsets[nfiles] == *total; file_lens[f]: its length without the zeros behind it, 0 for a failed file;
 *   file_statuses[f]: Z_OK or Z_BUF_ERROR; member_offsets[i]: where buffer i's member starts -- for a member of
 *   a failed file the file's offset --, which with source_lens gives a caller BGZF virtual offsets; ms: the
 *   device time of that _bgzf's launches.  Z_BUF_ERROR where total > image_cap, the tables filled all the
 *   same; Z_STREAM_ERROR on a plan that never enabled this or never called _bgzf. */
ZlibReturn zsc_hip_deflate_plan_bgzf_enable(zsc_hip_deflate_plan *plan, U32 nfiles, const U32 *file_first,
                                            U32 align);
ZlibReturn zsc_hip_deflate_plan_bgzf(zsc_hip_deflate_plan *plan, const void *d_output, void *d_image,
                                     uint64_t image_cap, void *hip_stream);
ZlibReturn zsc_hip_deflate_plan_bgzf_results(zsc_hip_deflate_plan *plan, uint64_t *file_offsets,
                                             uint64_t *file_lens, I32 *file_statuses, uint64_t *member_offsets,
                                             uint64_t *total, float *ms);

/* Host memory: nfiles files compressed into nfiles BGZF files.  File f (sources[f], source_lens[f] bytes) is
 * uploaded once, at a 16-byte aligned offset, and cut where it lies into buffers of block_bytes -- a multiple
 * of 16 from 16 to 65 536; 0 means 65 280, bgzip's value -- then one plan, one run, one _bgzf and one copy back
 * per file.  dest_lens[f]: in, the room at dests[f]; out, the file's length.  statuses[f] (may be NULL): Z_OK;
 * Z_BUF_ERROR where the file failed (a block that does not fit a member: pick a smaller block_bytes; the
 * length is then 0) or where the room is too small (nothing is copied, the length says what it takes).  An
 * empty file is the 28 end-of-file bytes.  Returns Z_OK when the batch ran.  Level 0 is Z_STREAM_ERROR, as in
 * the packed batch. */
ZlibReturn zsc_hip_bgzf_compress_batch(U32 nfiles, const U8 *const *sources, const uint64_t *source_lens,
                                       U8 *const *dests, uint64_t *dest_lens, I32 *statuses, I32 level,
                                       I32 mem_level, ZlibStrategy strategy, U32 block_bytes);

/* ZIP archives -------------------------------------------------------------------
 *
 * A gzip deflate plan's streams written out as ZIP archives -- the container of .npz, wheels, jars and OOXML / ODF
 * documents -- on the device (zsc_amd/csrc/zip.h).  An archive is a run of consecutive
 * buffers of the plan, arch_first[a] .. arch_first[a + 1] (a run may be empty).  Its image, all little-endian,
 * with n the buffer's name length and S the plan's stream for the buffer (out_len bytes):
 *
 *   entry, one per buffer in buffer order:
 *     local header (30): 50 4b 03 04 | version needed 20 | flags | method 8 | DOS time | DOS date | CRC-32 |
 *                        compressed size = out_len - 18 | uncompressed size | n | extra length 0
 *     the name (n bytes), then S[10 : out_len - 8], unchanged.  CRC-32 and the uncompressed size are S's last 8
 *     bytes.
 *   central directory, one record per buffer in the same order:
 *     record (46):       50 4b 01 02 | made by 20 (system 0) | version needed 20 | flags, method, time, date,
 *                        CRC-32 and sizes as in the local header | n | extra length 0 | comment length 0 |
 *                        disk 0 | internal attributes 0 | external attributes 0 | the local header's offset from
 *                        the archive's start
 *     the name again.
 *   end:
 *     with 65 535 entries or more, first the ZIP64 end record (56): 50 4b 06 06 | size 44 (8 bytes) | made by 45 |
 *                        needed 45 | disk 0 | directory's disk 0 | the count twice (8 bytes each) | the
 *                        directory's size | its offset (8 bytes each)
 *     and its locator (20): 50 4b 06 07 | disk 0 | the ZIP64 end record's offset (8 bytes) | 1 disk
 *     then always the end record (22): 50 4b 05 06 | disk 0 | directory's disk 0 | the count twice, saturated at
 *                        0xFFFF | the directory's size | its offset | comment length 0
 *
 * flags is 0x0800 with ZSC_HIP_ZIP_UTF8, else 0; there is no data descriptor: every size is known before a header
 * is written.  dos_datetime[i] is date << 16 | time; NULL means 0x00210000, 1980-01-01 00:00:00.  Names are bytes
 * the library does not interpret, 0 to 65 535 of them; buffer i's are names[name_offsets[i] .. name_offsets[i+1]).
 * Archives start at multiples of align (a power of two from 1 to 4096, as with _pack) and the bytes from an
 * archive's end to the next one's start are zeros.  An archive FAILS alone -- it takes no room in the image and
 * the others are what they are without it -- with Z_BUF_ERROR where one of its buffers has a status other than
 * Z_OK, and with Z_MEM_ERROR where it would be longer than 4 294 967 295 bytes (no ZIP64 offsets or sizes: the
 * caller splits).  Entry sizes always fit 32 bits.  CPython's zipfile reads these archives; a raw plain inflate
 * plan over data_offsets and the compressed sizes reads the entries back on the device.
 *
 * _zip_enable: before _run.  Z_STREAM_ERROR, with the plan left as it was, for a plan whose wrapper is not gzip, a
 *   plan of sections, an arch_first that does not ascend from 0 to count, a name above 65 535 bytes or
 *   descending name_offsets, unknown flags, or a bad align.  Calling it again replaces everything.  names,
 *   name_offsets (count + 1) and dos_datetime (count, or NULL) are host memory, copied.  Allocates the names, 44
 *   bytes per buffer (48 with dos_datetime), 36 per archive and 8 per 1 024 archives for the scan's partial sums,
 *   counted in _scratch_bytes.  Independent of _pack_enable, _bgzf_enable, _index_enable and _verify_enable: all
 *   may be on.  A plan that never calls it allocates and launches exactly what it did without these functions.
 * _zip: asynchronous on hip_stream; enqueues kernels only -- no allocation, no synchronisation, no copy from or
 *   to the host.  Valid after a _run on the same stream or after _results, any number of times.  d_output is the
 *   run's output or a copy of it at the plan's offsets; of each stream the whole 16-byte granules that hold one
 *   of its bytes are read.  d_image is 16-byte aligned and image_cap bytes long: bytes [0, total) are each
 *   written exactly once and nothing at or behind total; with total > image_cap nothing is written at all.
 *   Ordered against the plan's runs like a pack (see "Streams").
 * _zip_results: waits for the last _zip.  Every pointer may be NULL.  arch_offsets[a]: where archive a starts,
 *   arch_offsets[narchives] == *total; arch_lens[a]: its length without the zeros behind it, 0 for a failed one;
 *   arch_statuses[a]: Z_OK, Z_BUF_ERROR or Z_MEM_ERROR; entry_offsets[i] and data_offsets[i]: where buffer i's
 *   local header and its DEFLATE body start in the image; dir_offsets[a]: where archive a's central directory
 *   starts -- all three the archive's offset for a failed archive --; ms: the device time of that _zip's
 *   launches.  Z_BUF_ERROR where total > image_cap, the tables filled all the same; Z_STREAM_ERROR on a plan that
 *   never enabled this or never called _zip. */
#define ZSC_HIP_ZIP_UTF8 1u /* names are UTF-8: general purpose bit 11 */
ZlibReturn zsc_hip_deflate_plan_zip_enable(zsc_hip_deflate_plan *plan, U32 narchives, const U32 *arch_first,
                                           const U8 *names, const uint64_t *name_offsets, const U32 *dos_datetime,
                                           U32 flags, U32 align);
ZlibReturn zsc_hip_deflate_plan_zip(zsc_hip_deflate_plan *plan, const void *d_output, void *d_image,
                                    uint64_t image_cap, void *hip_stream);
ZlibReturn zsc_hip_deflate_plan_zip_results(zsc_hip_deflate_plan *plan, uint64_t *arch_offsets, uint64_t *arch_lens,
                                            I32 *arch_statuses, uint64_t *entry_offsets, uint64_t *data_offsets,
                                            uint64_t *dir_offsets, uint64_t *total, float *ms);

/* Host memory: narchives archives of named buffers compressed into narchives ZIP files.  Archive a is the buffers
 * arch_first[a] .. arch_first[a + 1] of count = arch_first[narchives]; buffer i is sources[i], source_lens[i]
 * bytes, named names[name_offsets[i] .. name_offsets[i + 1]).  One upload, one plan, one run, one _zip and one
 * copy back per archive.  dest_lens[a]: in, the room at dests[a]; out, the archive's length.  statuses[a] (may be
 * NULL): Z_OK; Z_BUF_ERROR or Z_MEM_ERROR where the archive failed (the length is then 0); Z_BUF_ERROR where the
 * room is too small (nothing is copied, the length says what it takes).  An empty archive is the 22 bytes of an
 * end record.  Returns Z_OK when the batch ran; Z_STREAM_ERROR for what _zip_enable refuses.  Level 0 is
 * Z_STREAM_ERROR, as in the packed batch. */
ZlibReturn zsc_hip_zip_compress_batch(U32 narchives, const U32 *arch_first, const U8 *const *sources,
                                      const U32 *source_lens, const U8 *names, const uint64_t *name_offsets,
                                      const U32 *dos_datetime, U32 flags, U8 *const *dests, uint64_t *dest_lens,
                                      I32 *statuses, I32 level, I32 mem_level, ZlibStrategy strategy);

/* BGZF ranges ---------------------------------------------------------------
 *
 * BGZF's seek points are its member starts, and they cost no decode to find.  An INDEX keeps them for a batch
 * of device-resident files; a RANGES plan decodes only the members its requests touch
 * (zsc_amd/csrc/bgzf_read.h).  The counterpart of the seek-point indexes above, which
 * give points INSIDE one stream.
 *
 * The index of a file of n bytes is the table of this walk:
 *     at = 0; out = 0; k = 0
 *     loop: the header at `at` must be a BGZF member's: 1f 8b 08, FEXTRA set and the reserved FLG bits clear, a
 *           `B` `C` subfield of length 2 whose BSIZE + 1 = L keeps the member inside the file with room for the
 *           extra field and a trailer, and an ISIZE (the last four bytes of those L) of at most 65 536; else stop
 *           coffset[k] = at; uoffset[k] = out; k += 1;  at += L; out += ISIZE
 *     coffset[k] = at; uoffset[k] = out                                                  (the end entry)
 * members = k, indexed_bytes = at, total_out = out.  A file that is not BGZF has 0 members, which is no error;
 * bytes behind the last member (padding, anything) are not indexed.  Nothing is decoded: the table is a set of
 * claims, each verified when a range is read.  Files are up to 4 GiB - 1 long (U32, as in a members plan) at
 * 16-byte aligned offsets with 64 readable bytes behind each; the tables are u64, as in .gzi.
 *
 * zsc_hip_bgzf_index_build is synchronous, like a plan's create: it enqueues on hip_stream a members plan's scan
 *   and claims launches and a walk over the claims' links, waits, reads the counts back and keeps the exact table
 *   on the device (every file's coffsets, then every file's uoffsets; no call hands it out yet) and on the host.
 *   Its scratch is a members plan's plus 16 bytes per 26 bytes of input -- the room every file's table could need,
 *   0.6 of the input -- all released before it returns; what it keeps is _scratch_bytes, 16 bytes per entry.
 *   _build_ms: the device time of its launches up to the walk.  Z_MEM_ERROR where an allocation failed,
 *   Z_STREAM_ERROR where a copy, a launch or the wait did; the same holds for _import_gzi.
 * _info, _table (cap: the entries coffsets and uoffsets have room for; Z_BUF_ERROR below members + 1; either
 *   may be NULL), _voffset and _uoffset need no device.  A virtual offset is coffset << 16 | offset within the
 *   member.  _voffset gives the one of the member that HOLDS byte uoffset (never an empty member's), and for
 *   total_out the end entry's with 0 within; Z_STREAM_ERROR beyond total_out.  _uoffset takes any virtual offset
 *   whose compressed part is a member start of the table (or its end entry, with 0 within) and whose part within
 *   is at most that member's length; Z_STREAM_ERROR otherwise.
 * _export_gzi / _import_gzi: the .gzi layout of bgzip -r -- a little-endian u64 count, then (u64 compressed,
 *   u64 uncompressed) for every member start after the first; the first member at (0, 0) is implicit and there
 *   is no end entry.  No htslib was at hand: that a file bgzip wrote loads here rests on that published layout,
 *   not on a test against one.  _export_gzi: *gzi_len is the room in, the length out (Z_BUF_ERROR where it does
 *   not fit or gzi is NULL).  _import_gzi makes a one-file index from an image and the file on the device: every
 *   entry is checked there, one per lane -- it must be a member start whose claim ends at the next entry with the
 *   length the uncompressed offsets differ by -- and the walk goes on behind the last entry to the end entry.
 *   Its room on the device is 16 bytes per named entry and per 26 bytes of the file behind the last named start.
 *   An image that does not fit the file is Z_DATA_ERROR, so an imported index is exactly what _build gives for
 *   that file, or it is refused.
 *
 * zsc_hip_inflate_plan_create_bgzf_ranges: item i asks for bytes [begins[i], begins[i] + lens[i]) of the
 *   uncompressed content of file files[i], written to [dst_offsets[i], + dest_caps[i]) of the run's d_dst
 *   (16-byte aligned offsets).  With ZSC_HIP_BGZF_VOFFSETS, begins[i] and lens[i] are a begin and an END virtual
 *   offset, converted with _uoffset: Z_STREAM_ERROR where either is refused there or end < begin.  The plan
 *   copies what it needs: the index may be destroyed before the run.  Create clips each range to total_out and
 *   makes one job per member that contributes a byte, longest member first.  In a run a lane group takes a
 *   job, evaluates the member's claim again -- it must give the index's end and length -- and decodes the member
 *   with the plain decode, which must return Z_OK with exactly that length and consumed count.  A member the
 *   range covers whole is decoded in place; an edge member (two per range at the most) goes whole into the
 *   group's staging slot, and the group copies the slice out.  Per item, by _results:
 *     Z_OK          dest_len is the clipped length (0 for a range at or behind total_out or of length 0: no job
 *                   runs), consumed the compressed offset behind the last member decoded (0 if none); bytes of
 *                   the destination behind dest_len are untouched
 *     Z_BUF_ERROR   dest_caps[i] is below the clipped length: nothing is written, dest_len says what it takes
 *     Z_DATA_ERROR  a job of the item was not good: dest_len and consumed are 0, the bytes in the item's own
 *                   destination unspecified.  One damaged member fails only the requests that touch it.
 *   Whatever the files or the index hold, nothing is written outside [dst_offsets[i], + dest_caps[i]) and the
 *   staging slots, and nothing is read outside a file and the 64 bytes behind it.  Coordinates are the index's:
 *   a member whose ISIZE field was altered shifts everything behind it, as for every BGZF reader.
 *   _run, _results, _destroy, _scratch_bytes and _pack_enable / _pack (which packs the Z_OK items) work as on any
 *   inflate plan; _index_enable and _dict_enable return Z_STREAM_ERROR; _results relaunches nothing.  Scratch:
 *   40 bytes per job, 20 per request, 16 per file, and -- where the plan has an edge job -- 65 552 bytes of
 *   staging for each lane group of the launch (four per wavefront, at most 20 wavefronts per CU, never more
 *   wavefronts than jobs / 4), whatever the number of requests -- on an MI355X 20 480 slots, 1.34 GB, for any
 *   plan of 81 920 jobs or more of which one is an edge; a plan of whole members has none.  That is beyond a
 *   plain plan's own buffers (items, queue order, results, resume records: 72 bytes per request), which a ranges plan has as
 *   well and _scratch_bytes does not count.  The environment variable ZSC_HIP_BGZF_GROUPS,
 *   read at create, caps the lane groups (a test hook: staging slots are then reused by many jobs).
 * _bgzf_jobs: the jobs of a ranges plan and the bytes they decode (either may be NULL).
 * zsc_hip_bgzf_read_ranges_batch: host memory.  Every file goes up once, an index and a ranges plan are made,
 *   and the Z_OK items come back as one packed image, dealt out to dests.  dest_lens[i]: in, the room at
 *   dests[i]; out, the item's dest_len.  A process that calls none of these allocates and launches what it did. */
#define ZSC_HIP_BGZF_VOFFSETS 1u
typedef struct zsc_hip_bgzf_index zsc_hip_bgzf_index;
ZlibReturn zsc_hip_bgzf_index_build(zsc_hip_bgzf_index **index, U32 nfiles, const void *d_src, const U32 *source_lens,
                                    const uint64_t *src_offsets, void *hip_stream);
ZlibReturn zsc_hip_bgzf_index_import_gzi(zsc_hip_bgzf_index **index, const U8 *gzi, uint64_t gzi_len,
                                         const void *d_src, U32 source_len, uint64_t src_offset, void *hip_stream);
ZlibReturn zsc_hip_bgzf_index_export_gzi(const zsc_hip_bgzf_index *index, U32 file, U8 *gzi, uint64_t *gzi_len);
ZlibReturn zsc_hip_bgzf_index_info(const zsc_hip_bgzf_index *index, U32 file, U32 *members, uint64_t *indexed_bytes,
                                   uint64_t *total_out);
ZlibReturn zsc_hip_bgzf_index_table(const zsc_hip_bgzf_index *index, U32 file, uint64_t *coffsets, uint64_t *uoffsets,
                                    U32 cap);
ZlibReturn zsc_hip_bgzf_index_voffset(const zsc_hip_bgzf_index *index, U32 file, uint64_t uoffset, uint64_t *voffset);
ZlibReturn zsc_hip_bgzf_index_uoffset(const zsc_hip_bgzf_index *index, U32 file, uint64_t voffset, uint64_t *uoffset);
uint64_t zsc_hip_bgzf_index_scratch_bytes(const zsc_hip_bgzf_index *index);
float zsc_hip_bgzf_index_build_ms(const zsc_hip_bgzf_index *index);
void zsc_hip_bgzf_index_destroy(zsc_hip_bgzf_index *index);
ZlibReturn zsc_hip_inflate_plan_create_bgzf_ranges(zsc_hip_inflate_plan **plan, const zsc_hip_bgzf_index *index,
                                                   U32 count, const U32 *files, const uint64_t *begins,
                                                   const uint64_t *lens, const U32 *dest_caps,
                                                   const uint64_t *dst_offsets, U32 flags);
ZlibReturn zsc_hip_inflate_plan_bgzf_jobs(zsc_hip_inflate_plan *plan, uint64_t *jobs, uint64_t *decoded_bytes);
ZlibReturn zsc_hip_bgzf_read_ranges_batch(U32 nfiles, const U8 *const *sources, const U32 *source_lens, U32 count,
                                          const U32 *files, const uint64_t *begins, const uint64_t *lens,
                                          U8 *const *dests, U32 *dest_lens, I32 *statuses, U32 flags);

/* preset dictionaries (decompression only) ---------------------------------
 *
 * zsc_hip_inflate_plan_dict_enable gives every stream of a PLAIN plan (zsc_hip_inflate_plan_create,
 * _create_ordered) one of ndicts dictionaries or none: stream_dict[i] is an index or ZSC_HIP_NO_DICT, and
 * stream_dict == NULL means dictionary 0 for every stream.  A run then reports what a caller of the
 * reference gets who answers Z_NEED_DICT with inflateSetDictionary inside zsc_uncompress's loop
 * (reference src/inflate.c:1446-1486, the DICTID / DICT states :955-968; zsc_amd/csrc/inflate.h, InfDict):
 *   - a raw plan (window_bits -9 .. -15) applies the stream's dictionary from the start; a zlib-wrapped
 *     stream (a zlib plan, or the zlib case of an auto-detecting one) only if its header sets FDICT.  A zlib
 *     stream without FDICT and a gzip member ignore it: a distance past the start of their output is the
 *     data error it always was;
 *   - the four big-endian bytes behind a zlib header with FDICT are compared with the Adler-32 of the WHOLE
 *     dictionary as given.  FDICT with ZSC_HIP_NO_DICT is the plain plan's answer, Z_NEED_DICT with 0 bytes
 *     out and 0 consumed; another id is Z_DATA_ERROR, 0 bytes out, 0 consumed, nothing resynchronised.  The
 *     trailer's Adler-32 covers the output alone;
 *   - with wsize = 1 << window bits (the plan's, or the header's where the plan's are 0) and
 *     have = min(dict_len, wsize), the stream decodes as if the last `have` bytes of the dictionary lay
 *     directly before byte 0 of its output: a distance is valid up to pos + have (and, as ever, up to the
 *     limit the header sets, 32 768 for raw), one more is the plain decoder's "too far back", with its
 *     resynchronisation;
 *   - after a data error nothing before the point of resynchronisation can be reached (inflateSync ends in
 *     inflateReset, :1593-1602), the dictionary included;
 *   - consumed counts the bytes of the source really used, the two header bytes and the four of the id
 *     included.  (The one departure: the reference's total_in would miss those six, but it has no one-shot
 *     call with a dictionary to be equal to, and consumed is how a caller finds a stream's end.)
 * The dictionaries are host memory of any length; the last 32 KiB of each go to the device once, and the
 * ids are taken over the whole of each there.  Calling it again replaces the set.  Z_STREAM_ERROR, with the
 * plan left as it was: an index >= ndicts, and every plan kind but the plain one (_create_sections, _chunks,
 * _resync, _indexed, _members, _size, _check).  zsc_hip_inflate_plan_pack_enable and runs with other device
 * buffers work as on any plain plan.  A plan that never enabled dictionaries launches exactly what it
 * launched before there were any.  zsc_hip_inflate_plan_scratch_bytes counts 32 KiB per dictionary, 8 bytes
 * per dictionary and 4 bytes per stream.
 * zsc_hip_inflate_plan_dict_ids: ids[d] = the Adler-32 of dictionary d (Z_STREAM_ERROR on a plan without).
 * zsc_hip_uncompress_dict_batch: zsc_hip_uncompress_batch through such a plan. */
#define ZSC_HIP_NO_DICT 0xffffffffu

ZlibReturn zsc_hip_inflate_plan_dict_enable(zsc_hip_inflate_plan *plan, U32 ndicts, const U8 *const *dicts,
                                            const U32 *dict_lens, const U32 *stream_dict);
ZlibReturn zsc_hip_inflate_plan_dict_ids(zsc_hip_inflate_plan *plan, U32 *ids);
ZlibReturn zsc_hip_uncompress_dict_batch(U32 count, const U8 *const *sources, U32 *source_lens, U8 *const *dests,
                                         U32 *dest_lens, I32 *statuses, I32 window_bits, U32 ndicts,
                                         const U8 *const *dicts, const U32 *dict_lens, const U32 *stream_dict);

#ifdef __cplusplus
}
#endif
#endif
