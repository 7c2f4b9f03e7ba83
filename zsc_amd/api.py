"""ctypes binding of libzsc_hip.so -- the host-side mirror of the reference API.

Function names follow ``include/zsc/zsc_pub.h`` with the ``zsc_`` prefix dropped;
arguments keep their reference meaning (``max_block_len``, caller-sized work buffer,
``window_bits`` wrapper encoding).  Return values are ``(ZlibReturn, bytes, ...)``
tuples instead of out-parameters.

The library is built in-tree by ``make -C zsc_amd/csrc`` (``__graft_entry__.build``)
and must exist: this module never falls back to a CPU codec.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import List, Optional, Sequence, Tuple

Z_OK, Z_STREAM_END, Z_NEED_DICT = 0, 1, 2
Z_ERRNO, Z_STREAM_ERROR, Z_DATA_ERROR, Z_MEM_ERROR, Z_BUF_ERROR, Z_VERSION_ERROR = -1, -2, -3, -4, -5, -6
Z_DEFAULT_STRATEGY, Z_FILTERED, Z_HUFFMAN_ONLY, Z_RLE, Z_FIXED = 0, 1, 2, 3, 4
GZIP_CODE, DEF_WBITS, DEF_MEM_LEVEL = 16, 15, 8
NKERNELS = 9
PACK_TILE = 16384  # ZSC_HIP_PACK_TILE: bytes of a packed image one wavefront moves
KERNEL_NAMES = ("checksum", "hash_sort", "match_table", "parse", "parse_short", "huff_plan", "layout", "emit", "total")

_HERE = os.path.dirname(os.path.abspath(__file__))
lib_path = os.environ.get("ZSC_HIP_LIB") or os.path.join(_HERE, "libzsc_hip.so")  # env: experiments only


def build_library() -> None:
    """Compile every HIP source for gfx950 into zsc_amd/libzsc_hip.so (hipcc, no GPU needed)."""
    subprocess.run(["make", "-s", "-C", os.path.join(_HERE, "csrc")], check=True)


class IndexHeader(C.Structure):
    """zsc_hip_index_header (include/zsc_hip.h)"""
    _fields_ = [("window_bits", C.c_int32), ("wrapper", C.c_uint32), ("gzip", C.c_uint32),
                ("dist_limit", C.c_uint32), ("chunk_bytes", C.c_uint32), ("consumed", C.c_uint32),
                ("total_out", C.c_uint32), ("trailer_offset", C.c_uint32), ("points", C.c_uint32)]


class VerifyResult(C.Structure):
    """zsc_hip_verify_result (include/zsc_hip.h)"""
    _fields_ = [("verdict", C.c_int32), ("block", C.c_uint32), ("bit_off", C.c_uint32), ("in_pos", C.c_uint32)]


class VerifyBlock(C.Structure):
    """zsc_hip_verify_block (include/zsc_hip.h)"""
    _fields_ = [("bit_off", C.c_uint32), ("in_begin", C.c_uint32), ("in_len", C.c_uint32), ("type_last", C.c_uint32)]


# ZSC_HIP_VERIFY_*: the verdict of verifying one buffer's stream against its input
VERIFY_OK, VERIFY_SKIPPED = 0, -1
(VERIFY_HEADER, VERIFY_BLOCK_HDR, VERIFY_CODES, VERIFY_LITERAL, VERIFY_DISTANCE, VERIFY_MATCH, VERIFY_LENGTH,
 VERIFY_BIT_END, VERIFY_TRAILER) = range(1, 10)


def _load() -> C.CDLL:
    # PyTorch-ROCm wheels bundle their own libamdhip64 (SONAME libamdhip64.so.7, the same
    # as /opt/rocm's).  Two HIP runtimes in one process cannot both own the GPU, so when
    # torch is installed it is imported FIRST: the loader then resolves libzsc_hip.so's
    # NEEDED libamdhip64.so.7 to the copy torch already mapped, and tensors, streams and
    # our kernels share one runtime.  Without torch the system ROCm runtime is used.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    if not os.path.exists(lib_path):
        raise ImportError(
            f"{lib_path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or make -C zsc_amd/csrc). zsc_amd has no CPU fallback.")
    L = C.CDLL(lib_path)
    u8p, u32p, i32p, u64p = C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
    L.zsc_hip_init.argtypes = [C.c_int32]
    L.zsc_hip_device_info.restype = C.c_char_p
    L.zsc_compress_get_min_work_buf_size.argtypes = [u32p]
    L.zsc_compress_get_min_work_buf_size2.argtypes = [C.c_int32, C.c_int32, u32p]
    L.zsc_compress_get_max_output_size.argtypes = [C.c_uint32, C.c_uint32, C.c_int32, u32p]
    L.zsc_compress_get_max_output_size2.argtypes = [C.c_uint32, C.c_uint32, C.c_int32, C.c_int32,
                                                    C.c_int32, u32p]
    L.zsc_uncompress_get_min_work_buf_size.argtypes = [u32p]
    L.zsc_uncompress_get_min_work_buf_size2.argtypes = [C.c_int32, u32p]
    L.zsc_compress_gzip2.argtypes = [u8p, u32p, C.c_char_p, C.c_uint32, C.c_uint32, u8p, C.c_uint32,
                                     C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    L.zsc_uncompress_gzip2.argtypes = [u8p, u32p, C.c_char_p, u32p, u8p, C.c_uint32, C.c_int32,
                                       C.c_void_p]
    L.zsc_hip_compress_batch.argtypes = [C.c_uint32, C.POINTER(C.c_char_p), u32p,
                                         C.POINTER(C.c_void_p), u32p, i32p, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_int32]
    L.zsc_hip_compress_sections_batch.argtypes = [C.c_uint32, C.POINTER(C.c_char_p), u32p, u32p,
                                                  C.POINTER(C.c_void_p), u32p, i32p, C.c_int32,
                                                  C.c_int32, C.c_int32, C.c_int32, C.c_uint32]
    L.zsc_hip_compress_sections_device.argtypes = [C.c_uint32, C.c_void_p, u64p, u32p, u32p, C.c_void_p,
                                                   u64p, u32p, u32p, i32p, C.c_int32, C.c_int32,
                                                   C.c_int32, C.c_int32]
    L.zsc_hip_uncompress_batch.argtypes = [C.c_uint32, C.POINTER(C.c_char_p), u32p,
                                           C.POINTER(C.c_void_p), u32p, i32p, C.c_int32]
    L.zsc_hip_inflate_plan_create.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, u32p, u64p, u32p,
                                              u64p, C.c_int32]
    L.zsc_hip_inflate_plan_create_ordered.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, u32p, u64p, u32p,
                                                      u64p, C.c_int32, u32p]
    L.zsc_hip_inflate_plan_create_sections.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, u32p, u64p, u32p,
                                                       u64p, C.c_int32]
    L.zsc_hip_inflate_plan_sections.argtypes = [C.c_void_p, u32p]
    L.zsc_hip_inflate_plan_scratch_bytes.argtypes = [C.c_void_p]
    L.zsc_hip_inflate_plan_scratch_bytes.restype = C.c_uint64
    L.zsc_hip_uncompress_sections_batch.argtypes = L.zsc_hip_uncompress_batch.argtypes
    L.zsc_hip_inflate_plan_create_chunks.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, u32p, u64p, u32p, u64p,
                                                     C.c_int32, C.c_uint32]
    L.zsc_hip_uncompress_chunks_batch.argtypes = L.zsc_hip_uncompress_batch.argtypes
    L.zsc_hip_inflate_plan_create_resync.argtypes = L.zsc_hip_inflate_plan_create_sections.argtypes
    L.zsc_hip_uncompress_resync_batch.argtypes = L.zsc_hip_uncompress_batch.argtypes
    L.zsc_hip_inflate_plan_data_errors.argtypes = [C.c_void_p, u32p]
    L.zsc_hip_inflate_plan_create_size.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, u32p, u64p, u32p, C.c_int32,
                                                   C.c_uint32]
    L.zsc_hip_uncompress_sizes_batch.argtypes = [C.c_uint32, C.POINTER(C.c_char_p), u32p, u32p, i32p, C.c_int32]
    L.zsc_hip_inflate_plan_create_check.argtypes = L.zsc_hip_inflate_plan_create_size.argtypes
    L.zsc_hip_inflate_plan_create_members.argtypes = L.zsc_hip_inflate_plan_create_sections.argtypes + [C.c_uint32]
    L.zsc_hip_inflate_plan_members.argtypes = [C.c_void_p, u32p, u32p]
    L.zsc_hip_uncompress_members_batch.argtypes = L.zsc_hip_uncompress_batch.argtypes + [u32p]
    L.zsc_hip_inflate_plan_check_values.argtypes = [C.c_void_p, u32p]
    L.zsc_hip_uncompress_check_batch.argtypes = [C.c_uint32, C.POINTER(C.c_char_p), u32p, u32p, i32p, u32p,
                                                 C.c_int32]
    L.zsc_hip_index_validate.argtypes = [C.c_char_p, C.c_uint64]
    L.zsc_hip_index_info.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(IndexHeader)]
    L.zsc_hip_index_range.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, u32p, u32p, u32p, u32p]
    L.zsc_hip_inflate_plan_index_enable.argtypes = [C.c_void_p, C.c_int32]
    L.zsc_hip_inflate_plan_dict_enable.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.zsc_hip_inflate_plan_dict_ids.argtypes = [C.c_void_p, C.c_void_p]
    L.zsc_hip_uncompress_dict_batch.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p,
                                                C.c_void_p]
    L.zsc_hip_inflate_plan_index_size.argtypes = [C.c_void_p, C.c_uint32, u64p]
    L.zsc_hip_inflate_plan_index_export.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_uint64, u64p]
    L.zsc_hip_inflate_plan_create_indexed.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, u32p, u64p, u32p, u64p,
                                                      C.c_int32, C.POINTER(C.c_char_p), u64p, u64p, u64p]
    L.zsc_hip_uncompress_indexed_batch.argtypes = L.zsc_hip_uncompress_batch.argtypes + [C.POINTER(C.c_char_p), u64p]
    L.zsc_hip_inflate_plan_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.zsc_hip_inflate_plan_results.argtypes = [C.c_void_p, u32p, u32p, i32p, C.POINTER(C.c_float)]
    L.zsc_hip_inflate_plan_destroy.argtypes = [C.c_void_p]
    L.zsc_hip_inflate_plan_destroy.restype = None
    L.zsc_hip_deflate_plan_layout.argtypes = [C.c_uint32, u32p, C.c_int32, C.c_int32, C.c_int32,
                                              u64p, u64p, u32p, u64p, u64p]
    L.zsc_hip_deflate_plan_create.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, u32p, u64p, u64p,
                                              u32p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    L.zsc_hip_deflate_plan_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.zsc_hip_deflate_plan_results.argtypes = [C.c_void_p, u32p, i32p]
    L.zsc_hip_deflate_plan_profile.argtypes = [C.c_void_p, C.c_int32]
    L.zsc_hip_deflate_plan_profile.restype = None
    L.zsc_hip_deflate_plan_times.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.zsc_hip_deflate_plan_scratch_bytes.argtypes = [C.c_void_p]
    L.zsc_hip_deflate_plan_scratch_bytes.restype = C.c_uint64
    L.zsc_hip_deflate_plan_sub_batches.argtypes = [C.c_void_p]
    L.zsc_hip_deflate_plan_sub_batches.restype = C.c_uint32
    L.zsc_hip_deflate_plan_seg_schedule.argtypes = [C.c_void_p]
    L.zsc_hip_deflate_plan_seg_schedule.restype = C.c_int32
    L.zsc_hip_deflate_plan_seg_ring.argtypes = [C.c_void_p]
    L.zsc_hip_deflate_plan_seg_ring.restype = C.c_int32
    L.zsc_hip_compress_sections_last_rings.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.zsc_hip_compress_sections_last_rings.restype = None
    L.zsc_hip_deflate_plan_destroy.argtypes = [C.c_void_p]
    L.zsc_hip_deflate_plan_destroy.restype = None
    L.zsc_hip_deflate_plan_index_enable.argtypes = [C.c_void_p, C.c_uint32]
    L.zsc_hip_deflate_plan_index_size.argtypes = [C.c_void_p, C.c_uint32, u64p]
    L.zsc_hip_deflate_plan_index_export.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_char_p, C.c_uint64, u64p]
    L.zsc_hip_deflate_plan_index_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.zsc_hip_deflate_plan_verify_enable.argtypes = [C.c_void_p]
    L.zsc_hip_deflate_plan_verify.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.zsc_hip_deflate_plan_verify_results.argtypes = [C.c_void_p, C.POINTER(VerifyResult), C.POINTER(C.c_float)]
    L.zsc_hip_deflate_plan_verify_blocks.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(VerifyBlock), C.c_uint32, u32p]
    for kind in ("deflate", "inflate"):
        getattr(L, f"zsc_hip_{kind}_plan_pack_enable").argtypes = [C.c_void_p, C.c_uint32]
        getattr(L, f"zsc_hip_{kind}_plan_pack").argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        getattr(L, f"zsc_hip_{kind}_plan_pack_results").argtypes = [C.c_void_p, u64p, u64p, C.POINTER(C.c_float)]
    L.zsc_hip_deflate_plan_bgzf_enable.argtypes = [C.c_void_p, C.c_uint32, u32p, C.c_uint32]
    L.zsc_hip_deflate_plan_bgzf.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.zsc_hip_deflate_plan_bgzf_results.argtypes = [C.c_void_p, u64p, u64p, i32p, u64p, u64p, C.POINTER(C.c_float)]
    L.zsc_hip_bgzf_compress_batch.argtypes = [C.c_uint32, C.POINTER(C.c_char_p), u64p, C.POINTER(C.c_void_p), u64p,
                                              i32p, C.c_int32, C.c_int32, C.c_int32, C.c_uint32]
    L.zsc_hip_deflate_plan_zip_enable.argtypes = [C.c_void_p, C.c_uint32, u32p, C.c_char_p, u64p, u32p, C.c_uint32,
                                                  C.c_uint32]
    L.zsc_hip_deflate_plan_zip.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.zsc_hip_deflate_plan_zip_results.argtypes = [C.c_void_p, u64p, u64p, i32p, u64p, u64p, u64p, u64p,
                                                   C.POINTER(C.c_float)]
    L.zsc_hip_zip_compress_batch.argtypes = [C.c_uint32, u32p, C.POINTER(C.c_char_p), u32p, C.c_char_p, u64p, u32p,
                                             C.c_uint32, C.POINTER(C.c_void_p), u64p, i32p, C.c_int32, C.c_int32,
                                             C.c_int32]
    L.zsc_hip_bgzf_index_build.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.c_void_p, u32p, u64p, C.c_void_p]
    L.zsc_hip_bgzf_index_import_gzi.argtypes = [C.POINTER(C.c_void_p), C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint32,
                                                C.c_uint64, C.c_void_p]
    L.zsc_hip_bgzf_index_export_gzi.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, u64p]
    L.zsc_hip_bgzf_index_info.argtypes = [C.c_void_p, C.c_uint32, u32p, u64p, u64p]
    L.zsc_hip_bgzf_index_table.argtypes = [C.c_void_p, C.c_uint32, u64p, u64p, C.c_uint32]
    L.zsc_hip_bgzf_index_voffset.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, u64p]
    L.zsc_hip_bgzf_index_uoffset.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, u64p]
    L.zsc_hip_bgzf_index_scratch_bytes.argtypes = [C.c_void_p]
    L.zsc_hip_bgzf_index_scratch_bytes.restype = C.c_uint64
    L.zsc_hip_bgzf_index_build_ms.argtypes = [C.c_void_p]
    L.zsc_hip_bgzf_index_build_ms.restype = C.c_float
    L.zsc_hip_bgzf_index_destroy.argtypes = [C.c_void_p]
    L.zsc_hip_bgzf_index_destroy.restype = None
    L.zsc_hip_inflate_plan_create_bgzf_ranges.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_uint32, u32p, u64p,
                                                          u64p, u32p, u64p, C.c_uint32]
    L.zsc_hip_inflate_plan_bgzf_jobs.argtypes = [C.c_void_p, u64p, u64p]
    L.zsc_hip_bgzf_read_ranges_batch.argtypes = [C.c_uint32, C.POINTER(C.c_char_p), u32p, C.c_uint32, u32p, u64p, u64p,
                                                 C.POINTER(C.c_void_p), u32p, i32p, C.c_uint32]
    L.zsc_hip_unpack.argtypes = [C.c_uint32, C.c_void_p, u64p, u32p, C.c_void_p, u64p, C.c_void_p]
    L.zsc_hip_compress_batch_packed.argtypes = [C.c_uint32, C.c_char_p, u64p, C.c_void_p, C.c_uint64, u64p, i32p,
                                                C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint32]
    L.zsc_hip_uncompress_batch_packed.argtypes = [C.c_uint32, C.c_char_p, u64p, u32p, u32p, C.c_void_p, C.c_uint64,
                                                  u64p, u32p, u32p, i32p, C.c_int32, C.c_uint32]
    return L


lib = _load()


def device_info() -> str:
    return lib.zsc_hip_device_info().decode()


# ---- sizing helpers ------------------------------------------------------------

def compress_get_min_work_buf_size(window_bits: int = DEF_WBITS, mem_level: int = DEF_MEM_LEVEL):
    out = C.c_uint32()
    rc = lib.zsc_compress_get_min_work_buf_size2(window_bits, mem_level, C.byref(out))
    return rc, out.value


def compress_get_max_output_size2(source_len: int, max_block_len: int, level: int,
                                  window_bits: int = DEF_WBITS, mem_level: int = DEF_MEM_LEVEL):
    out = C.c_uint32()
    rc = lib.zsc_compress_get_max_output_size2(source_len, max_block_len, level, window_bits,
                                               mem_level, C.byref(out))
    return rc, out.value


def compress_get_max_output_size(source_len: int, max_block_len: int, level: int):
    return compress_get_max_output_size2(source_len, max_block_len, level)


def uncompress_get_min_work_buf_size(window_bits: int = DEF_WBITS):
    out = C.c_uint32()
    rc = lib.zsc_uncompress_get_min_work_buf_size2(window_bits, C.byref(out))
    return rc, out.value


# ---- one-shot calls (reference zsc_pub.h:201-411) ---------------------------------

class GzHeader(C.Structure):
    """gz_header, reference include/zsc/zlib_types_pub.h:281-296"""
    _fields_ = [("text", C.c_int32), ("time", C.c_uint32), ("xflags", C.c_int32), ("os", C.c_int32),
                ("extra", C.c_void_p), ("extra_len", C.c_uint32), ("extra_max", C.c_uint32),
                ("name", C.c_void_p), ("name_max", C.c_uint32),
                ("comment", C.c_void_p), ("comm_max", C.c_uint32),
                ("hcrc", C.c_int32), ("done", C.c_int32)]


def gz_header_for_writing(text=0, time=0, os=3, extra: Optional[bytes] = None, name: Optional[bytes] = None,
                          comment: Optional[bytes] = None, hcrc=0):
    """A gz_header for zsc_compress_gzip*; returns (struct, buffers to keep alive)."""
    h = GzHeader()
    h.text, h.time, h.os, h.hcrc = text, time, os, hcrc
    keep = []
    if extra is not None:
        b = C.create_string_buffer(extra, max(len(extra), 1))
        keep.append(b)
        h.extra, h.extra_len = C.addressof(b), len(extra)
    if name is not None:
        b = C.create_string_buffer(name + b"\0")
        keep.append(b)
        h.name = C.addressof(b)
    if comment is not None:
        b = C.create_string_buffer(comment + b"\0")
        keep.append(b)
        h.comment = C.addressof(b)
    return h, keep


def gz_header_for_reading(extra_max=0, name_max=0, comm_max=0):
    """A gz_header for zsc_uncompress_gzip*; returns (struct, (extra, name, comment) buffers)."""
    h = GzHeader()
    bufs = []
    for cap, ptr, mx in ((extra_max, "extra", "extra_max"), (name_max, "name", "name_max"),
                         (comm_max, "comment", "comm_max")):
        b = C.create_string_buffer(max(cap, 1)) if cap else None
        bufs.append(b)
        if b is not None:
            setattr(h, ptr, C.addressof(b))
            setattr(h, mx, cap)
    return h, tuple(bufs)


def gz_header_fields(h: GzHeader, bufs) -> dict:
    """What a reader finds in the struct afterwards (buffers cut at their capacity)."""
    extra, name, comment = bufs
    return {"text": h.text, "time": h.time, "xflags": h.xflags, "os": h.os, "hcrc": h.hcrc, "done": h.done,
            "extra_len": h.extra_len,
            "extra": None if not h.extra or extra is None else extra.raw[:min(h.extra_len, h.extra_max)].hex(),
            "name": None if not h.name or name is None else name.raw.split(b"\0")[0].hex(),
            "comment": None if not h.comment or comment is None else comment.raw.split(b"\0")[0].hex()}


def compress2(source: bytes, max_block_len: Optional[int] = None, level: int = 6,
              window_bits: int = DEF_WBITS, mem_level: int = DEF_MEM_LEVEL,
              strategy: int = Z_DEFAULT_STRATEGY, dest_len: Optional[int] = None,
              work_len: Optional[int] = None, gz_header: Optional[GzHeader] = None) -> Tuple[int, bytes]:
    """zsc_compress2 / zsc_compress_gzip2 (reference zsc_pub.h:258,290).  Returns (ZlibReturn, stream bytes)."""
    n = len(source)
    mbl = max(n, 1) if max_block_len is None else max_block_len
    if dest_len is None:
        rc, dest_len = compress_get_max_output_size2(n, mbl, level, window_bits, mem_level)
        if rc != Z_OK:
            dest_len = n + (n >> 3) + 128
        if gz_header is not None:
            dest_len += 70000 * 3  # extra + name + comment at their largest
    if work_len is None:
        rc, work_len = compress_get_min_work_buf_size(window_bits, mem_level)
        if rc != Z_OK:
            work_len = 400000
    dst = C.create_string_buffer(max(dest_len, 1))
    work = C.create_string_buffer(max(work_len, 1))
    dl = C.c_uint32(dest_len)
    rc = lib.zsc_compress_gzip2(dst, C.byref(dl), source, n, mbl, work, work_len, level,
                                window_bits, mem_level, strategy,
                                None if gz_header is None else C.byref(gz_header))
    return rc, dst.raw[:dl.value]


def compress(source: bytes, max_block_len: Optional[int] = None, level: int = 6, **kw):
    """zsc_compress (reference zsc_pub.h:201): zlib wrapper, default window and memory."""
    return compress2(source, max_block_len, level, DEF_WBITS, DEF_MEM_LEVEL, Z_DEFAULT_STRATEGY, **kw)


def compress_gzip(source: bytes, max_block_len: Optional[int] = None, level: int = 6, **kw):
    """zsc_compress_gzip (reference zsc_pub.h:227) with gz_header == NULL."""
    return compress2(source, max_block_len, level, DEF_WBITS + GZIP_CODE, DEF_MEM_LEVEL,
                     Z_DEFAULT_STRATEGY, **kw)


def uncompress2(source: bytes, dest_len: int, window_bits: int = DEF_WBITS,
                work_len: Optional[int] = None, gz_header: Optional[GzHeader] = None) -> Tuple[int, bytes, int]:
    """zsc_uncompress2 (reference zsc_pub.h:385).  Returns (ZlibReturn, bytes, consumed)."""
    if work_len is None:
        rc, work_len = uncompress_get_min_work_buf_size(window_bits)
        if rc != Z_OK:
            work_len = 40000
    dst = C.create_string_buffer(max(dest_len, 1))
    work = C.create_string_buffer(max(work_len, 1))
    dl, sl = C.c_uint32(dest_len), C.c_uint32(len(source))
    rc = lib.zsc_uncompress_gzip2(dst, C.byref(dl), source, C.byref(sl), work, work_len,
                                  window_bits, None if gz_header is None else C.byref(gz_header))
    return rc, dst.raw[:dl.value], sl.value


def uncompress(source: bytes, dest_len: int, **kw):
    return uncompress2(source, dest_len, DEF_WBITS, **kw)


def uncompress_gzip(source: bytes, dest_len: int, **kw):
    return uncompress2(source, dest_len, DEF_WBITS + GZIP_CODE, **kw)


# ---- batches ---------------------------------------------------------------------

def compress_batch(sources: Sequence[bytes], level: int = 6, window_bits: int = DEF_WBITS,
                   mem_level: int = DEF_MEM_LEVEL, strategy: int = Z_DEFAULT_STRATEGY,
                   dest_caps: Optional[Sequence[int]] = None) -> Tuple[int, List[bytes], List[int]]:
    """zsc_hip_compress_batch: every item behaves like one zsc_compress2 call."""
    count = len(sources)
    if dest_caps is None:
        dest_caps = [compress_get_max_output_size2(len(s), max(len(s), 1), level, window_bits,
                                                   mem_level)[1] for s in sources]
    srcs = (C.c_char_p * count)(*sources)
    slen = (C.c_uint32 * count)(*[len(s) for s in sources])
    bufs = [C.create_string_buffer(max(c, 1)) for c in dest_caps]
    dsts = (C.c_void_p * count)(*[C.addressof(b) for b in bufs])
    dlen = (C.c_uint32 * count)(*dest_caps)
    stat = (C.c_int32 * count)()
    rc = lib.zsc_hip_compress_batch(count, srcs, slen, dsts, dlen, stat, level, window_bits,
                                    mem_level, strategy)
    outs = [bufs[i].raw[:dlen[i]] for i in range(count)] if rc == Z_OK else []
    return rc, outs, list(stat)


def compress_sections_batch(sources: Sequence[bytes], max_block_lens: Sequence[int], level: int = 6,
                            window_bits: int = DEF_WBITS, mem_level: int = DEF_MEM_LEVEL,
                            strategy: int = Z_DEFAULT_STRATEGY,
                            dest_caps: Optional[Sequence[int]] = None) -> Tuple[int, List[bytes], List[int]]:
    """zsc_hip_compress_sections_batch: item i behaves like zsc_compress2 with
    max_block_lens[i] < len(sources[i]) at levels 1-9 (sections, flush markers, output slices)."""
    count = len(sources)
    if dest_caps is None:
        dest_caps = [compress_get_max_output_size2(len(s), m, level, window_bits, mem_level)[1]
                     for s, m in zip(sources, max_block_lens)]
    srcs = (C.c_char_p * count)(*sources)
    slen = (C.c_uint32 * count)(*[len(s) for s in sources])
    mbls = (C.c_uint32 * count)(*max_block_lens)
    bufs = [C.create_string_buffer(max(c, 1)) for c in dest_caps]
    dsts = (C.c_void_p * count)(*[C.addressof(b) for b in bufs])
    dlen = (C.c_uint32 * count)(*dest_caps)
    stat = (C.c_int32 * count)()
    rc = lib.zsc_hip_compress_sections_batch(count, srcs, slen, mbls, dsts, dlen, stat, level,
                                             window_bits, mem_level, strategy, 0)
    outs = [bufs[i].raw[:dlen[i]] for i in range(count)] if rc == Z_OK else []
    return rc, outs, list(stat)


def compress_sections_last_rings() -> Tuple[int, int]:
    """(wide, narrow): sub-batches of the last compress_sections_* call by the LDS geometry of their parser."""
    w, n = C.c_uint32(), C.c_uint32()
    lib.zsc_hip_compress_sections_last_rings(C.byref(w), C.byref(n))
    return w.value, n.value


def compress_sections_device(d_input: int, in_offsets: Sequence[int], source_lens: Sequence[int],
                             max_block_lens: Sequence[int], d_output: int, out_offsets: Sequence[int],
                             out_caps: Sequence[int], level: int = 6, window_bits: int = DEF_WBITS,
                             mem_level: int = DEF_MEM_LEVEL,
                             strategy: int = Z_DEFAULT_STRATEGY) -> Tuple[int, List[int], List[int]]:
    """zsc_hip_compress_sections_device: streams and results stay in device memory
    (d_input / d_output are device pointers).  Returns (rc, stream lengths, statuses)."""
    count = len(source_lens)
    ioff = (C.c_uint64 * count)(*in_offsets)
    slen = (C.c_uint32 * count)(*source_lens)
    mbls = (C.c_uint32 * count)(*max_block_lens)
    ooff = (C.c_uint64 * count)(*out_offsets)
    caps = (C.c_uint32 * count)(*out_caps)
    dlen = (C.c_uint32 * count)()
    stat = (C.c_int32 * count)()
    rc = lib.zsc_hip_compress_sections_device(count, d_input, ioff, slen, mbls, d_output, ooff, caps,
                                              dlen, stat, level, window_bits, mem_level, strategy)
    return rc, list(dlen), list(stat)


def uncompress_batch(sources: Sequence[bytes], dest_caps: Sequence[int],
                     window_bits: int = DEF_WBITS) -> Tuple[int, List[bytes], List[int], List[int]]:
    """zsc_hip_uncompress_batch: every item behaves like one zsc_uncompress2 call.
    Returns (rc, outputs, consumed, statuses)."""
    return _uncompress_batch(lib.zsc_hip_uncompress_batch, sources, dest_caps, window_bits)


def uncompress_sections_batch(sources: Sequence[bytes], dest_caps: Sequence[int],
                              window_bits: int = DEF_WBITS) -> Tuple[int, List[bytes], List[int], List[int]]:
    """zsc_hip_uncompress_sections_batch: as uncompress_batch, with the full-flush sections of
    each stream decoded in parallel (results identical to uncompress_batch for every input)."""
    return _uncompress_batch(lib.zsc_hip_uncompress_sections_batch, sources, dest_caps, window_bits)


def uncompress_chunks_batch(sources: Sequence[bytes], dest_caps: Sequence[int],
                            window_bits: int = DEF_WBITS):
    """zsc_hip_uncompress_chunks_batch: as uncompress_batch, with every stream longer than a chunk
    decoded in parallel pieces from block starts found by trial (results identical to uncompress_batch
    for every input)."""
    return _uncompress_batch(lib.zsc_hip_uncompress_chunks_batch, sources, dest_caps, window_bits)


def uncompress_resync_batch(sources: Sequence[bytes], dest_caps: Sequence[int],
                            window_bits: int = DEF_WBITS):
    """zsc_hip_uncompress_resync_batch: as uncompress_batch, with the full-flush sections of each
    stream decoded in parallel, damaged streams included: a data error resynchronises at the next
    flush marker as zsc_uncompress does (results identical to uncompress_batch for every input)."""
    return _uncompress_batch(lib.zsc_hip_uncompress_resync_batch, sources, dest_caps, window_bits)


NO_LIMIT = 0xFFFFFFFF
NO_DICT = 0xFFFFFFFF  # ZSC_HIP_NO_DICT: a stream of a plan with preset dictionaries that has none


def uncompress_sizes_batch(sources: Sequence[bytes], limits: Sequence[int] | None = None,
                           window_bits: int = DEF_WBITS) -> Tuple[int, List[int], List[int], List[int]]:
    """zsc_hip_uncompress_sizes_batch: what every stream inflates to, found on the device without writing
    any output.  limits[i] is the most stream i may inflate to (None: no limit); a stream longer than its
    limit is Z_BUF_ERROR with its size equal to the limit.  Status, size and consumed are uncompress_batch's
    with dest_caps = limits, except that the check value of a zlib / gzip trailer is not compared.
    Returns (rc, sizes, consumed, statuses)."""
    count = len(sources)
    srcs = (C.c_char_p * count)(*sources)
    slen = (C.c_uint32 * count)(*[len(s) for s in sources])
    dlen = (C.c_uint32 * count)(*([NO_LIMIT] * count if limits is None else limits))
    stat = (C.c_int32 * count)()
    rc = lib.zsc_hip_uncompress_sizes_batch(count, srcs, slen, dlen, stat, window_bits)
    return rc, list(dlen) if rc == Z_OK else [], list(slen), list(stat)


MEMBERS_SIZE_ONLY = 1
GZIP_WBITS = 31


def uncompress_members_batch(sources: Sequence[bytes], dest_caps: Sequence[int] | None, window_bits: int = GZIP_WBITS,
                             size_only: bool = False):
    """zsc_hip_uncompress_members_batch: every source is a multi-member gzip file (a packed archive of gzip
    streams, BGZF, `cat a.gz b.gz`), inflated member by member in parallel.  The result of a file is that of
    walking it with uncompress_batch, one member after the other in what is left of dest_caps[i], up to the
    first member that is not Z_OK or to where no 1f 8b follows.  Returns (rc, outputs, consumed, statuses,
    members).  size_only=True writes nothing (a members plan in size-only mode: dest_caps are limits, None:
    no limit; the CRC-32 is not compared) and returns the sizes in place of the outputs."""
    count = len(sources)
    if size_only:
        plan = InflatePlan([len(s) for s in sources], dest_caps, window_bits=window_bits, members=True, size_only=True)
        try:
            import torch
            image = bytearray(plan.src_bytes)
            for s, o in zip(sources, plan.src_offsets):
                image[o:o + len(s)] = s
            d_src = torch.frombuffer(image, dtype=torch.uint8).cuda()
            plan.run(d_src.data_ptr())
            sizes, used, stat, _ = plan.results()
            return Z_OK, sizes, used, stat, plan.members()[0]
        finally:
            plan.close()
    if dest_caps is None:
        raise ValueError("dest_caps are needed")
    srcs = (C.c_char_p * count)(*sources)
    slen = (C.c_uint32 * count)(*[len(s) for s in sources])
    bufs = [C.create_string_buffer(max(c, 1)) for c in dest_caps]
    dsts = (C.c_void_p * count)(*[C.addressof(b) for b in bufs])
    dlen = (C.c_uint32 * count)(*dest_caps)
    stat = (C.c_int32 * count)()
    memb = (C.c_uint32 * max(count, 1))()
    rc = lib.zsc_hip_uncompress_members_batch(count, srcs, slen, dsts, dlen, stat, window_bits, memb)
    outs = [bufs[i].raw[:dlen[i]] for i in range(count)] if rc == Z_OK else []
    return rc, outs, list(slen), list(stat), list(memb)[:count]


def uncompress_check_batch(sources: Sequence[bytes], limits: Sequence[int] | None = None,
                           window_bits: int = DEF_WBITS) -> Tuple[int, List[int], List[int], List[int], List[int]]:
    """zsc_hip_uncompress_check_batch: is every stream intact?  Found on the device without writing any
    output (gzip -t for a batch).  limits as uncompress_sizes_batch.  Status, size and consumed are exactly
    uncompress_batch's with dest_caps = limits: a wrong Adler-32 / CRC-32 is Z_DATA_ERROR.  check_values[i]
    is the value computed over the output of a stream whose status is Z_OK (CRC-32 for gzip, Adler-32 for
    zlib and raw streams) and 0 otherwise.  Returns (rc, sizes, consumed, statuses, check_values)."""
    count = len(sources)
    srcs = (C.c_char_p * count)(*sources)
    slen = (C.c_uint32 * count)(*[len(s) for s in sources])
    dlen = (C.c_uint32 * count)(*([NO_LIMIT] * count if limits is None else limits))
    stat = (C.c_int32 * count)()
    vals = (C.c_uint32 * count)()
    rc = lib.zsc_hip_uncompress_check_batch(count, srcs, slen, dlen, stat, vals, window_bits)
    return rc, list(dlen) if rc == Z_OK else [], list(slen), list(stat), list(vals)


def uncompress_batch_auto(sources: Sequence[bytes], window_bits: int = DEF_WBITS, limit: int | None = None):
    """Inflate streams of unknown length: size them (uncompress_sizes_batch, every stream under `limit`
    if one is given), then run uncompress_chunks_batch with dest_caps[i] set to the reported size, so no
    byte of capacity is allocated beyond it.  Returns what that call returns and the sizes:
    (rc, outputs, consumed, statuses, sizes).  The statuses are the inflate's: a stream cut off at the
    limit comes back Z_BUF_ERROR with `limit` bytes, one whose check value is wrong Z_DATA_ERROR."""
    count = len(sources)
    rc, sizes, _, _ = uncompress_sizes_batch(sources, None if limit is None else [limit] * count, window_bits)
    if rc != Z_OK:
        return rc, [], [], [], []
    rc, outs, used, stat = uncompress_chunks_batch(sources, sizes, window_bits)
    return rc, outs, used, stat, sizes


def uncompress_indexed_batch(sources: Sequence[bytes], dest_caps: Sequence[int],
                             indexes: Sequence[Optional[bytes]], window_bits: int = DEF_WBITS):
    """zsc_hip_uncompress_indexed_batch: as uncompress_batch, with every stream that has a valid index
    (export_index / build_indexes; None: no index) decoded in parallel from its seek points, without the
    chunks plan's discovery (results identical to uncompress_batch for every input and every blob, but
    see include/zsc_hip.h on raw streams)."""
    count = len(sources)
    blobs = (C.c_char_p * count)(*indexes)
    blens = (C.c_uint64 * count)(*[len(b) if b is not None else 0 for b in indexes])
    return _uncompress_batch(lambda *a: lib.zsc_hip_uncompress_indexed_batch(*a, blobs, blens), sources, dest_caps,
                             window_bits)


def index_info(blob: bytes) -> dict:
    """zsc_hip_index_info: the header of a seek-point index as a dict (ValueError for a blob that is not
    a valid index).  No device needed."""
    h = IndexHeader()
    if lib.zsc_hip_index_info(blob, len(blob), C.byref(h)) != Z_OK:
        raise ValueError("not a valid seek-point index")
    return {name: getattr(h, name) for name, _ in IndexHeader._fields_}


def index_range(blob: bytes, begin: int, length: int) -> Tuple[int, int, int, int]:
    """zsc_hip_index_range: (first piece, piece count, piece_begin, piece_len) of the smallest run of whole
    pieces that covers output bytes [begin, begin + length).  ValueError for a blob that is not valid or a
    range that is empty or not inside the output.  No device needed."""
    f, c, b, n = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    rc = lib.zsc_hip_index_range(blob, len(blob), begin, length, C.byref(f), C.byref(c), C.byref(b), C.byref(n))
    if rc != Z_OK:
        raise ValueError("not a valid seek-point index" if rc == Z_DATA_ERROR else "range outside the output")
    return f.value, c.value, b.value, n.value


def build_indexes(sources: Sequence[bytes], dest_caps: Sequence[int], window_bits: int = DEF_WBITS,
                  chunk_bytes: int = 0) -> List[Optional[bytes]]:
    """The seek-point index of every stream, from one run of a chunks plan with keep_index (None for a
    stream the serial decoder produced: too short, damaged, or not split)."""
    import torch
    plan = InflatePlan([len(s) for s in sources], dest_caps, window_bits=window_bits, chunks=True,
                       chunk_bytes=chunk_bytes, keep_index=True)
    try:
        src = torch.zeros(plan.src_bytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty(plan.dst_bytes, dtype=torch.uint8, device="cuda")
        for s, off in zip(sources, plan.src_offsets):
            if s:
                src[off:off + len(s)] = torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda()
        plan.run(src.data_ptr(), dst.data_ptr())
        plan.results()
        return [plan.export_index(i) for i in range(len(sources))]
    finally:
        plan.close()


def compress_batch_indexed(sources: Sequence[bytes], level: int = 6, window_bits: int = DEF_WBITS,
                           mem_level: int = DEF_MEM_LEVEL, strategy: int = Z_DEFAULT_STRATEGY,
                           chunk_bytes: int = 0) -> Tuple[List[bytes], List[int], List[Optional[bytes]]]:
    """Every stream of compress_batch with its seek-point index, from one run of a DeflatePlan with
    index_enable: (streams, statuses, blobs).  A blob goes to uncompress_indexed_batch or
    InflatePlan(indexes=...) beside its stream; no chunks plan is needed to make it."""
    import torch
    plan = DeflatePlan([len(s) for s in sources], level, window_bits, mem_level, strategy)
    try:
        plan.index_enable(chunk_bytes)
        src = torch.zeros(plan.in_bytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty(plan.out_bytes, dtype=torch.uint8, device="cuda")
        for s, off in zip(sources, plan.in_offsets):
            if s:
                src[off:off + len(s)] = torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda()
        plan.run(src.data_ptr(), dst.data_ptr())
        lens, stat = plan.results()
        host = dst.cpu().numpy().tobytes()
        streams = [host[off:off + n] if st == Z_OK else b"" for off, n, st in zip(plan.out_offsets, lens, stat)]
        return streams, stat, plan.export_indexes(src.data_ptr())
    finally:
        plan.close()


def compress_batch_verified(sources: Sequence[bytes], level: int = 6, window_bits: int = DEF_WBITS,
                            mem_level: int = DEF_MEM_LEVEL, strategy: int = Z_DEFAULT_STRATEGY
                            ) -> Tuple[int, List[bytes], List[int], List[dict]]:
    """compress_batch with every stream verified against its input on the device before it is copied to the
    host, from one run of a DeflatePlan with verify_enable: (rc, streams, statuses, verdicts).  verdicts are
    DeflatePlan.verify_results(); rc is Z_OK when the batch ran and no stream failed its verification,
    Z_DATA_ERROR when one did (its bytes are returned all the same)."""
    import torch
    plan = DeflatePlan([len(s) for s in sources], level, window_bits, mem_level, strategy)
    try:
        plan.verify_enable()
        src = torch.zeros(plan.in_bytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty(plan.out_bytes, dtype=torch.uint8, device="cuda")
        for s, off in zip(sources, plan.in_offsets):
            if s:
                src[off:off + len(s)] = torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda()
        plan.run(src.data_ptr(), dst.data_ptr())
        lens, stat = plan.results()
        rc = plan.verify(src.data_ptr(), dst.data_ptr())
        if rc != Z_OK:
            return rc, [], stat, []
        verdicts = plan.verify_results()
        host = dst.cpu().numpy().tobytes()
        streams = [host[off:off + n] if st == Z_OK else b"" for off, n, st in zip(plan.out_offsets, lens, stat)]
        bad = any(v["verdict"] not in (VERIFY_OK, VERIFY_SKIPPED) for v in verdicts)
        return (Z_DATA_ERROR if bad else Z_OK), streams, stat, verdicts
    finally:
        plan.close()


def _round_up(n: int, align: int) -> int:
    return (n + align - 1) // align * align if align > 1 else n  # (an align the library refuses: no matter)


class PackedCallError(RuntimeError):
    """A *_batch_packed call that did not run: .rc is the ZlibReturn (Z_STREAM_ERROR: level 0, an align that is
    no power of two from 1 to 4096, offsets out of order; Z_BUF_ERROR: dest_cap is too small, and .offsets[-1]
    says what the image takes)."""

    def __init__(self, what: str, rc: int, offsets: List[int]):
        super().__init__(f"{what} failed: {rc}")
        self.rc, self.offsets = rc, offsets


class _Packing:
    """pack_enable / pack / pack_results / pack_ms of both plan classes (zsc_hip_*_plan_pack*)."""
    _pack_kind = ""

    def pack_enable(self, align: int = 16) -> None:
        """Before run(): the plan can pack the items of a run into one image, item i at a multiple of align (a
        power of two from 1 to 4096; 16 or more feeds InflatePlan(src_offsets=...), 1 gives an archive)."""
        rc = getattr(lib, f"zsc_hip_{self._pack_kind}_plan_pack_enable")(self._h, align)
        if rc != Z_OK:
            raise ValueError(f"zsc_hip_{self._pack_kind}_plan_pack_enable failed: {rc}")

    def pack(self, d_output: int, d_packed: int, cap: int, stream: int = 0) -> int:
        """After run() on the same stream, or after results(), any number of times: enqueue the pack of the
        items at d_output (the run's output or a copy of it at the plan's offsets) into the cap bytes at
        d_packed (16-byte aligned).  Returns the ZlibReturn: Z_STREAM_ERROR on a plan without pack_enable().
        stream: the pack is ordered in it like a kernel; the plan's next run, results() and close() wait for it."""
        return getattr(lib, f"zsc_hip_{self._pack_kind}_plan_pack")(self._h, C.c_void_p(d_output), C.c_void_p(d_packed),
                                                                     cap, C.c_void_p(stream))

    def pack_results(self) -> Tuple[List[int], int]:
        """Waits for the last pack(): (offsets, total) -- count + 1 offsets, the last one the total.  BufferError,
        with .offsets and .total to size another pack() by, where the image was longer than cap (nothing was
        written then)."""
        off = (C.c_uint64 * (self.count + 1))()
        total, ms = C.c_uint64(), C.c_float()
        rc = getattr(lib, f"zsc_hip_{self._pack_kind}_plan_pack_results")(self._h, off, C.byref(total), C.byref(ms))
        self._pack_ms = ms.value
        if rc == Z_BUF_ERROR:
            err = BufferError(f"the packed image takes {total.value} bytes")
            err.offsets, err.total = list(off), total.value
            raise err
        if rc != Z_OK:
            raise RuntimeError(f"zsc_hip_{self._pack_kind}_plan_pack_results failed: {rc}")
        return list(off), total.value

    def pack_ms(self) -> float:
        """After pack_results(): device time of that pack's launches, in milliseconds."""
        if getattr(self, "_pack_ms", None) is None:
            raise RuntimeError("no pack_results() yet")
        return self._pack_ms


def unpack(d_packed: int, packed_offsets: Sequence[int], lens: Sequence[int], d_dst: int,
           dst_offsets: Sequence[int], stream: int = 0) -> int:
    """zsc_hip_unpack: item i, lens[i] bytes at packed_offsets[i] of the device image d_packed (ascending, any
    alignment; a count + 1 table as pack_results() returns it will do), to dst_offsets[i] (multiples of 16) of
    d_dst; no other byte of d_dst is written.  Asynchronous on stream.  Returns the ZlibReturn.
    stream: the three tables are uploaded before the call returns, the launch is ordered in the stream like a kernel."""
    n = len(lens)
    return lib.zsc_hip_unpack(n, C.c_void_p(d_packed), (C.c_uint64 * n)(*packed_offsets[:n]), (C.c_uint32 * n)(*lens),
                              C.c_void_p(d_dst), (C.c_uint64 * n)(*dst_offsets), C.c_void_p(stream))


def compress_batch_packed(sources, level: int = 6, window_bits: int = DEF_WBITS, mem_level: int = DEF_MEM_LEVEL,
                          strategy: int = Z_DEFAULT_STRATEGY, align: int = 1, source_offsets: Sequence[int] | None = None,
                          dest_cap: Optional[int] = None) -> Tuple[bytes, List[int], List[int]]:
    """zsc_hip_compress_batch_packed: compress_batch with one copy to the device and one back.  sources: a
    sequence of buffers, or one bytes object with source_offsets (count + 1).  Returns (image, offsets,
    statuses): stream i is image[offsets[i]:offsets[i + 1]] less its padding up to align; with align 1 the
    image is the streams one after the other.  PackedCallError where the call as a whole fails."""
    if source_offsets is None:
        source_offsets = [0]
        for s_ in sources:
            source_offsets.append(source_offsets[-1] + len(s_))
        sources = b"".join(sources)
    n = len(source_offsets) - 1
    if dest_cap is None:
        dest_cap = sum(_round_up(compress_get_max_output_size2(source_offsets[i + 1] - source_offsets[i],
                                                               max(source_offsets[i + 1] - source_offsets[i], 1), level,
                                                               window_bits, mem_level)[1], align) for i in range(n))
    dst = C.create_string_buffer(max(dest_cap, 1))
    off = (C.c_uint64 * (n + 1))()
    stat = (C.c_int32 * max(n, 1))()
    rc = lib.zsc_hip_compress_batch_packed(n, sources, (C.c_uint64 * (n + 1))(*source_offsets), dst, dest_cap, off,
                                           stat, level, window_bits, mem_level, strategy, align)
    if rc != Z_OK:
        raise PackedCallError("zsc_hip_compress_batch_packed", rc, list(off))
    return dst.raw[:off[n]], list(off), list(stat)[:n]


def bgzf_compress_batch(files: Sequence[bytes], level: int = 6, block_bytes: int = 65280,
                        mem_level: int = DEF_MEM_LEVEL, strategy: int = Z_DEFAULT_STRATEGY,
                        dest_caps: Sequence[int] | None = None) -> Tuple[List[bytes], List[int]]:
    """zsc_hip_bgzf_compress_batch: every file compressed into a BGZF file of its own, cut into members of
    block_bytes of input (a multiple of 16 up to 65 536; 65 280 is bgzip's).  Returns (files, statuses): a file
    whose status is Z_BUF_ERROR is b"" -- one of its blocks did not fit a member (pick a smaller block_bytes),
    or dest_caps[f] (default: the worst case) was too small.  PackedCallError where the call as a whole fails."""
    n = len(files)
    bb = block_bytes or 65280
    if dest_caps is None:
        dest_caps = [((len(f) + bb - 1) // bb) * 65536 + 28 for f in files]
    bufs = [C.create_string_buffer(max(c, 1)) for c in dest_caps]
    srcs = (C.c_char_p * max(n, 1))(*files)
    slen = (C.c_uint64 * max(n, 1))(*[len(f) for f in files])
    dsts = (C.c_void_p * max(n, 1))(*[C.addressof(b) for b in bufs])
    dlen = (C.c_uint64 * max(n, 1))(*dest_caps)
    stat = (C.c_int32 * max(n, 1))()
    rc = lib.zsc_hip_bgzf_compress_batch(n, srcs, slen, dsts, dlen, stat, level, mem_level, strategy, block_bytes)
    if rc != Z_OK:
        raise PackedCallError("zsc_hip_bgzf_compress_batch", rc, [])
    return [b.raw[:dlen[f]] if stat[f] == Z_OK else b"" for f, b in enumerate(bufs)], list(stat)[:n]


ZIP_UTF8 = 1


def zip_compress_batch(archives: Sequence[Sequence[Tuple[bytes, bytes]]], level: int = 6,
                       mem_level: int = DEF_MEM_LEVEL, strategy: int = Z_DEFAULT_STRATEGY,
                       dos_datetime: Sequence[int] | None = None, utf8: bool = False,
                       dest_caps: Sequence[int] | None = None) -> Tuple[List[bytes], List[int]]:
    """zsc_hip_zip_compress_batch: archives[a] is a list of (name_bytes, data); every archive comes back as a ZIP
    file of its own, its entries in that order (method 8, no data descriptors; the ZIP64 end records from 65 535
    entries on).  dos_datetime: one date << 16 | time per entry over all archives (default 1980-01-01 00:00:00);
    utf8 sets the entries' UTF-8 flag.  Returns (files, statuses): an archive whose status is not Z_OK is b"" --
    it would pass 4 294 967 295 bytes (Z_MEM_ERROR), or dest_caps[a] (default: the worst case) was too small
    (Z_BUF_ERROR).  PackedCallError where the call as a whole fails."""
    na = len(archives)
    first, names, datas = [0], [], []
    for arch in archives:
        for nm, data in arch:
            names.append(bytes(nm))
            datas.append(bytes(data))
        first.append(len(datas))
    n = len(datas)
    if dest_caps is None:  # (zlib's conservative bound on a deflate body)
        dest_caps = [sum(76 + 2 * len(names[i]) + len(datas[i]) + (len(datas[i]) >> 3) + (len(datas[i]) >> 8) +
                         (len(datas[i]) >> 9) + 64 for i in range(first[a], first[a + 1])) + 98 for a in range(na)]
    offs = [0]
    for nm in names:
        offs.append(offs[-1] + len(nm))
    bufs = [C.create_string_buffer(max(c, 1)) for c in dest_caps]
    srcs = (C.c_char_p * max(n, 1))(*datas)
    slen = (C.c_uint32 * max(n, 1))(*[len(d) for d in datas])
    dsts = (C.c_void_p * max(na, 1))(*[C.addressof(b) for b in bufs])
    dlen = (C.c_uint64 * max(na, 1))(*dest_caps)
    stat = (C.c_int32 * max(na, 1))()
    dt = None if dos_datetime is None else (C.c_uint32 * max(n, 1))(*dos_datetime)
    rc = lib.zsc_hip_zip_compress_batch(na, (C.c_uint32 * (na + 1))(*first), srcs, slen, b"".join(names),
                                        (C.c_uint64 * (n + 1))(*offs), dt, ZIP_UTF8 if utf8 else 0, dsts, dlen, stat,
                                        level, mem_level, strategy)
    if rc != Z_OK:
        raise PackedCallError("zsc_hip_zip_compress_batch", rc, [])
    return [b.raw[:dlen[a]] if stat[a] == Z_OK else b"" for a, b in enumerate(bufs)], list(stat)[:na]


def uncompress_batch_packed(image: bytes, offsets: Sequence[int], lens: Sequence[int], dest_caps: Sequence[int],
                            window_bits: int = DEF_WBITS, align: int = 1, dest_cap: Optional[int] = None):
    """zsc_hip_uncompress_batch_packed: uncompress_batch with one copy to the device and one back.  Stream i is
    lens[i] bytes at image[offsets[i]] (ascending; a count + 1 table will do) and may decode to dest_caps[i]
    bytes.  Returns (image, offsets, dest_lens, consumed, statuses): output i is dest_lens[i] bytes at
    offsets[i] of the returned image.  PackedCallError where the call as a whole fails."""
    n = len(lens)
    if dest_cap is None:
        dest_cap = sum(_round_up(c, align) for c in dest_caps)
    dst = C.create_string_buffer(max(dest_cap, 1))
    off = (C.c_uint64 * (n + 1))()
    dlen, used, stat = (C.c_uint32 * max(n, 1))(), (C.c_uint32 * max(n, 1))(), (C.c_int32 * max(n, 1))()
    rc = lib.zsc_hip_uncompress_batch_packed(n, image, (C.c_uint64 * max(n, 1))(*offsets[:n]), (C.c_uint32 * max(n, 1))(*lens),
                                             (C.c_uint32 * max(n, 1))(*dest_caps), dst, dest_cap, off, dlen, used, stat,
                                             window_bits, align)
    if rc != Z_OK:
        raise PackedCallError("zsc_hip_uncompress_batch_packed", rc, list(off))
    return dst.raw[:off[n]], list(off), list(dlen)[:n], list(used)[:n], list(stat)[:n]


def _uncompress_batch(fn, sources, dest_caps, window_bits):
    count = len(sources)
    srcs = (C.c_char_p * count)(*sources)
    slen = (C.c_uint32 * count)(*[len(s) for s in sources])
    bufs = [C.create_string_buffer(max(c, 1)) for c in dest_caps]
    dsts = (C.c_void_p * count)(*[C.addressof(b) for b in bufs])
    dlen = (C.c_uint32 * count)(*dest_caps)
    stat = (C.c_int32 * count)()
    rc = fn(count, srcs, slen, dsts, dlen, stat, window_bits)
    outs = [bufs[i].raw[:dlen[i]] for i in range(count)] if rc == Z_OK else []
    return rc, outs, list(slen), list(stat)


def _dict_arrays(dicts):
    """(pointers, lengths) of a list of dictionaries for the C ABI; the pointers keep the bytes alive"""
    n = len(dicts)
    keep = [bytes(d) for d in dicts]
    ptrs = (C.c_char_p * max(n, 1))(*keep)
    ptrs._keep = keep
    return ptrs, (C.c_uint32 * max(n, 1))(*[len(d) for d in keep])


def uncompress_dict_batch(sources: Sequence[bytes], dest_caps: Sequence[int], dicts: Sequence[bytes],
                          stream_dict: Sequence[int] | None = None, window_bits: int = DEF_WBITS):
    """uncompress_batch for streams that use zlib preset dictionaries (zsc_hip_uncompress_dict_batch):
    stream_dict[i] is the index of stream i's dictionary in dicts or NO_DICT; None: dictionary 0 for all.
    -> (rc, outputs, consumed, statuses)."""
    if stream_dict is not None and len(stream_dict) != len(sources):
        raise ValueError("one dictionary index per stream")
    ptrs, lens = _dict_arrays(dicts)
    sd = None if stream_dict is None else (C.c_uint32 * max(len(sources), 1))(*stream_dict)

    def fn(count, srcs, slen, dsts, dlen, stat, wbits):
        return lib.zsc_hip_uncompress_dict_batch(count, srcs, slen, dsts, dlen, stat, wbits, len(dicts), ptrs, lens, sd)

    return _uncompress_batch(fn, sources, dest_caps, window_bits)


class InflatePlan(_Packing):
    """Device-resident inflate batch (see include/zsc_hip.h).  sections=True makes a sections plan
    (zsc_hip_inflate_plan_create_sections: full-flush sections decoded in parallel; it takes no
    decode_order).  chunks=True makes a chunks plan (zsc_hip_inflate_plan_create_chunks: any stream longer
    than chunk_bytes decoded in parallel pieces; chunk_bytes 0 = the library's default; no decode_order
    either).  resync=True makes a resync plan (zsc_hip_inflate_plan_create_resync: a sections plan that
    also decodes damaged streams in parallel, resynchronising at the next flush marker after a data
    error); it implies sections.  keep_index=True (chunks plans only) keeps what a run finds out, for
    export_index().  indexes=[blob or None, ...] makes an indexed plan (zsc_hip_inflate_plan_create_indexed:
    every stream with a valid index decoded in parallel from its seek points); with it, ranges=[(begin,
    length) or None, ...] decodes only the whole pieces that cover that range of the stream's output
    (index_range), to the start of the stream's destination.  src_offsets=[...] (multiples of 16) puts the
    streams where the caller has them instead of one behind the other -- the offsets of an image packed with
    align 16 or more, say, which then is the plan's input as it lies; src_bytes is not meaningful then.
    size_only=True makes a size plan (zsc_hip_inflate_plan_create_size): dest_caps are the limits (None: no
    limit), nothing is written, run() takes d_dst 0, and results() gives the sizes; a stream longer than
    chunk_bytes is sized in parallel pieces (chunk_bytes 0 = the default, NO_LIMIT = never cut a stream).
    check_only=True makes a check plan (zsc_hip_inflate_plan_create_check) with the same arguments: the
    streams are decoded into 64 KiB rings, so the check value of the trailer is compared as well -- results()
    is a plain plan's at dest_caps = limits -- and check_values() hands out the values computed.
    members=True makes a members plan (zsc_hip_inflate_plan_create_members): every item is a multi-member gzip
    file, inflated member by member in parallel (window_bits must select the gzip wrapper, 24..31); members()
    gives the member counts and sections() the members the parallel path decoded.  It may be combined with
    size_only=True (nothing written, dest_caps are limits or None, the CRC-32 is not compared) and with nothing
    else.
    dicts=[bytes, ...] gives the streams of a plain plan zlib preset dictionaries
    (zsc_hip_inflate_plan_dict_enable): stream_dict[i] is the index of stream i's dictionary or NO_DICT, None
    means dictionary 0 for every stream.  dict_enable() replaces the set later; dict_ids() hands out the
    dictionaries' Adler-32 values."""
    _pack_kind = "inflate"

    def __init__(self, source_lens: Sequence[int], dest_caps: Sequence[int] | None,
                 window_bits: int = DEF_WBITS, decode_order: Sequence[int] | None = None,
                 sections: bool = False, chunks: bool = False, chunk_bytes: int = 0, resync: bool = False,
                 keep_index: bool = False, indexes: Sequence[Optional[bytes]] | None = None,
                 ranges: Sequence[Optional[Tuple[int, int]]] | None = None,
                 src_offsets: Sequence[int] | None = None, size_only: bool = False,
                 check_only: bool = False, members: bool = False, dicts: Sequence[bytes] | None = None,
                 stream_dict: Sequence[int] | None = None):
        self.count = n = len(source_lens)
        if stream_dict is not None and dicts is None:
            raise ValueError("stream_dict needs dicts")
        if members and (check_only or sections or chunks or resync or keep_index or indexes is not None or
                        decode_order is not None or chunk_bytes):
            raise ValueError("a members plan may be size-only and is no other kind of plan")
        members_size_only = members and size_only
        if members_size_only and dest_caps is None:
            dest_caps = [NO_LIMIT] * n
        size_only = size_only and not members
        if size_only and check_only:
            raise ValueError("a plan is a size plan or a check plan, not both")
        size_only = size_only or check_only  # (a check plan is laid out as a size plan)
        if size_only:
            if sections or chunks or resync or keep_index or indexes is not None or decode_order is not None:
                raise ValueError("a size or check plan is no other kind of plan and takes no decode_order")
            if dest_caps is None:
                dest_caps = [NO_LIMIT] * n
        elif dest_caps is None:
            raise ValueError("dest_caps are needed")
        if keep_index and not chunks:
            raise ValueError("keep_index needs a chunks plan")
        if ranges is not None and indexes is None:
            raise ValueError("ranges need indexes")
        if indexes is not None and (sections or chunks or resync or decode_order is not None):
            raise ValueError("an indexed plan is no sections, chunks or resync plan and takes no decode_order")
        so, do, sb, db = [], [], 0, 0
        for sl, dc in zip(source_lens, dest_caps):
            so.append(sb)
            do.append(db)
            sb += (sl + 64 + 15) & ~15
            db += 0 if size_only or members_size_only else (dc + 64 + 15) & ~15
        if src_offsets is not None:
            if len(src_offsets) != n:
                raise ValueError("one source offset per stream")
            so = list(src_offsets)
            sb = max([o + l for o, l in zip(so, source_lens)], default=0)
        self.src_offsets, self.dst_offsets = so, do
        self.src_bytes, self.dst_bytes = sb + 64, db + 64
        self._h = C.c_void_p()
        if resync and chunks:
            raise ValueError("a resync plan is a sections plan, not a chunks plan")
        if sections and chunks:
            raise ValueError("a plan is a sections plan or a chunks plan, not both")
        if members:
            rc = lib.zsc_hip_inflate_plan_create_members(C.byref(self._h), n, (C.c_uint32 * n)(*source_lens),
                                                         (C.c_uint64 * n)(*so), (C.c_uint32 * n)(*dest_caps),
                                                         (C.c_uint64 * n)(*do), window_bits,
                                                         MEMBERS_SIZE_ONLY if members_size_only else 0)
        elif size_only:
            create = lib.zsc_hip_inflate_plan_create_check if check_only else lib.zsc_hip_inflate_plan_create_size
            rc = create(C.byref(self._h), n, (C.c_uint32 * n)(*source_lens), (C.c_uint64 * n)(*so),
                        (C.c_uint32 * n)(*dest_caps), window_bits, chunk_bytes)
        elif indexes is not None:
            if len(indexes) != n or (ranges is not None and len(ranges) != n):
                raise ValueError("one index (and one range) per stream")
            blobs = (C.c_char_p * n)(*indexes)
            blens = (C.c_uint64 * n)(*[len(b) if b is not None else 0 for b in indexes])
            rb = rl = None
            if ranges is not None:
                rb = (C.c_uint64 * n)(*[r[0] if r is not None else 0 for r in ranges])
                rl = (C.c_uint64 * n)(*[r[1] if r is not None else 0xffffffffffffffff for r in ranges])
            rc = lib.zsc_hip_inflate_plan_create_indexed(C.byref(self._h), n, (C.c_uint32 * n)(*source_lens),
                                                         (C.c_uint64 * n)(*so), (C.c_uint32 * n)(*dest_caps),
                                                         (C.c_uint64 * n)(*do), window_bits, blobs, blens, rb, rl)
        elif chunks:
            if decode_order is not None:
                raise ValueError("a chunks plan takes no decode_order")
            rc = lib.zsc_hip_inflate_plan_create_chunks(C.byref(self._h), n, (C.c_uint32 * n)(*source_lens),
                                                        (C.c_uint64 * n)(*so), (C.c_uint32 * n)(*dest_caps),
                                                        (C.c_uint64 * n)(*do), window_bits, chunk_bytes)
        elif sections or resync:
            if decode_order is not None:
                raise ValueError("a sections plan takes no decode_order")
            create = lib.zsc_hip_inflate_plan_create_resync if resync else lib.zsc_hip_inflate_plan_create_sections
            rc = create(C.byref(self._h), n, (C.c_uint32 * n)(*source_lens),
                                                          (C.c_uint64 * n)(*so), (C.c_uint32 * n)(*dest_caps),
                                                          (C.c_uint64 * n)(*do), window_bits)
        else:
            order = None if decode_order is None else (C.c_uint32 * n)(*decode_order)
            rc = lib.zsc_hip_inflate_plan_create_ordered(C.byref(self._h), n, (C.c_uint32 * n)(*source_lens),
                                                         (C.c_uint64 * n)(*so), (C.c_uint32 * n)(*dest_caps),
                                                         (C.c_uint64 * n)(*do), window_bits, order)
        if rc != Z_OK:
            raise RuntimeError(f"zsc_hip_inflate_plan_create failed: {rc}")
        if keep_index and lib.zsc_hip_inflate_plan_index_enable(self._h, 1) != Z_OK:
            raise RuntimeError("zsc_hip_inflate_plan_index_enable failed")
        if dicts is not None:
            rc = self.dict_enable(dicts, stream_dict)
            if rc != Z_OK:
                self.close()
                raise ValueError(f"zsc_hip_inflate_plan_dict_enable failed: {rc}")

    def dict_enable(self, dicts: Sequence[bytes], stream_dict: Sequence[int] | None = None) -> int:
        """Gives the streams these preset dictionaries (replacing the ones the plan had).  Returns the
        ZlibReturn: Z_STREAM_ERROR, with the plan as it was, for an index out of range and for every plan kind
        but the plain one."""
        if stream_dict is not None and len(stream_dict) != self.count:
            raise ValueError("one dictionary index per stream")
        ptrs, lens = _dict_arrays(dicts)
        sd = None if stream_dict is None else (C.c_uint32 * max(self.count, 1))(*stream_dict)
        rc = lib.zsc_hip_inflate_plan_dict_enable(self._h, len(dicts), ptrs, lens, sd)
        if rc == Z_OK:
            self._ndicts = len(dicts)
        return rc

    def dict_ids(self) -> List[int]:
        """The Adler-32 of each of the plan's dictionaries, taken over the whole of it."""
        n = getattr(self, "_ndicts", None)
        if n is None:
            raise ValueError("the plan has no dictionaries")
        out = (C.c_uint32 * max(n, 1))()
        rc = lib.zsc_hip_inflate_plan_dict_ids(self._h, out)
        if rc != Z_OK:
            raise RuntimeError(f"zsc_hip_inflate_plan_dict_ids failed: {rc}")
        return list(out)[:n]

    def export_index(self, i: int) -> Optional[bytes]:
        """After results() of a chunks plan made with keep_index: the seek-point index of stream i, or
        None for a stream the serial decoder produced."""
        need = C.c_uint64()
        rc = lib.zsc_hip_inflate_plan_index_size(self._h, i, C.byref(need))
        if rc == Z_DATA_ERROR:
            return None
        if rc != Z_OK:
            raise RuntimeError(f"zsc_hip_inflate_plan_index_size failed: {rc}")
        buf = C.create_string_buffer(need.value)
        got = C.c_uint64()
        rc = lib.zsc_hip_inflate_plan_index_export(self._h, i, buf, need.value, C.byref(got))
        if rc != Z_OK:
            raise RuntimeError(f"zsc_hip_inflate_plan_index_export failed: {rc}")
        return buf.raw[:got.value]

    def run(self, d_src: int, d_dst: int = 0, stream: int = 0) -> None:
        """stream (a hipStream_t as an int, e.g. torch.cuda.Stream().cuda_stream): the run is ordered in it like a
        kernel, and on another stream than the plan's unfinished run or pack it waits for that on the device."""
        rc = lib.zsc_hip_inflate_plan_run(self._h, C.c_void_p(d_src), C.c_void_p(d_dst),
                                          C.c_void_p(stream))
        if rc != Z_OK:
            raise RuntimeError(f"zsc_hip_inflate_plan_run failed: {rc}")

    def results(self):
        n = self.count
        lens, used, stat, ms = (C.c_uint32 * n)(), (C.c_uint32 * n)(), (C.c_int32 * n)(), C.c_float()
        rc = lib.zsc_hip_inflate_plan_results(self._h, lens, used, stat, C.byref(ms))
        if rc != Z_OK:
            raise RuntimeError(f"zsc_hip_inflate_plan_results failed: {rc}")
        return list(lens), list(used), list(stat), ms.value

    def sections(self) -> List[int]:
        """After results(): per stream, the sections (or pieces, of a chunks plan) decoded in parallel
        (0: decoded serially)."""
        n = self.count
        out = (C.c_uint32 * max(n, 1))()
        rc = lib.zsc_hip_inflate_plan_sections(self._h, out)
        if rc != Z_OK:
            raise RuntimeError(f"zsc_hip_inflate_plan_sections failed: {rc}")
        return list(out)[:n]

    def members(self) -> Tuple[List[int], List[int]]:
        """After results() of a members plan: per file, the members of the walk that were Z_OK, and how many
        members of the verified prefix (sections()) were claimed by their headers."""
        n = self.count
        memb, claimed = (C.c_uint32 * max(n, 1))(), (C.c_uint32 * max(n, 1))()
        rc = lib.zsc_hip_inflate_plan_members(self._h, memb, claimed)
        if rc != Z_OK:
            raise RuntimeError(f"zsc_hip_inflate_plan_members failed: {rc}")
        return list(memb)[:n], list(claimed)[:n]

    def data_errors(self) -> List[int]:
        """After results(), for every plan kind: per stream, the data errors zsc_uncompress's loop counts
        (0 for a stream that decoded cleanly)."""
        n = self.count
        out = (C.c_uint32 * max(n, 1))()
        rc = lib.zsc_hip_inflate_plan_data_errors(self._h, out)
        if rc != Z_OK:
            raise RuntimeError(f"zsc_hip_inflate_plan_data_errors failed: {rc}")
        return list(out)[:n]

    def check_values(self) -> List[int]:
        """After run() of a check plan: per stream whose status is Z_OK, the check value computed over its
        output (CRC-32 for gzip, Adler-32 for zlib and raw streams); 0 for every other stream."""
        n = self.count
        out = (C.c_uint32 * max(n, 1))()
        rc = lib.zsc_hip_inflate_plan_check_values(self._h, out)
        if rc != Z_OK:
            raise RuntimeError(f"zsc_hip_inflate_plan_check_values failed: {rc}")
        return list(out)[:n]

    def scratch_bytes(self) -> int:
        """Device scratch of a sections, chunks or resync plan beyond a plain plan's (0 for a plain plan)."""
        return int(lib.zsc_hip_inflate_plan_scratch_bytes(self._h))

    def close(self) -> None:
        if self._h:
            lib.zsc_hip_inflate_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


BGZF_VOFFSETS = 1


class BgzfIndex:
    """The member index of a batch of BGZF files on the device (zsc_hip_bgzf_index_build, include/zsc_hip.h
    "BGZF ranges"): per file the compressed and uncompressed offset of every member start and of the end, found
    from the headers alone.  d_src is the device pointer of the batch, file f at src_offsets[f] (multiples of 16,
    64 readable bytes behind each; None: one behind the other as InflatePlan lays sources out, see src_offsets
    and src_bytes).  A file that is not BGZF has 0 members."""

    def __init__(self, d_src: int, source_lens: Sequence[int], src_offsets: Sequence[int] | None = None,
                 stream: int = 0, _handle=None):
        self.nfiles = n = len(source_lens)
        self.source_lens = list(source_lens)
        self.src_offsets, self.src_bytes = self.layout(source_lens) if src_offsets is None else (list(src_offsets), 0)
        self._h = C.c_void_p()
        if _handle is not None:
            self._h = _handle
            return
        rc = lib.zsc_hip_bgzf_index_build(C.byref(self._h), n, C.c_void_p(d_src), (C.c_uint32 * max(n, 1))(*source_lens),
                                          (C.c_uint64 * max(n, 1))(*self.src_offsets), C.c_void_p(stream))
        if rc != Z_OK:
            raise RuntimeError(f"zsc_hip_bgzf_index_build failed: {rc}")

    @staticmethod
    def layout(source_lens: Sequence[int]) -> Tuple[List[int], int]:
        """(src_offsets, src_bytes) of files laid out one behind the other, as InflatePlan lays sources out"""
        so, sb = [], 0
        for sl in source_lens:
            so.append(sb)
            sb += (sl + 64 + 15) & ~15
        return so, sb + 64

    @classmethod
    def from_gzi(cls, gzi: bytes, d_src: int, source_len: int, src_offset: int = 0, stream: int = 0) -> "BgzfIndex":
        """A one-file index from a .gzi image (bgzip -r) and the file on the device.  Every entry is checked
        against the file there; ValueError (Z_DATA_ERROR) where the image does not fit it, so what comes back is
        exactly what building the index gives."""
        h = C.c_void_p()
        rc = lib.zsc_hip_bgzf_index_import_gzi(C.byref(h), gzi, len(gzi), C.c_void_p(d_src), source_len, src_offset,
                                               C.c_void_p(stream))
        if rc == Z_DATA_ERROR:
            raise ValueError("the .gzi image does not fit the file")
        if rc != Z_OK:
            raise RuntimeError(f"zsc_hip_bgzf_index_import_gzi failed: {rc}")
        return cls(d_src, [source_len], [src_offset], _handle=h)

    def info(self, file: int = 0) -> Tuple[int, int, int]:
        """(members, indexed_bytes, total_out) of a file"""
        m, ib, to = C.c_uint32(), C.c_uint64(), C.c_uint64()
        rc = lib.zsc_hip_bgzf_index_info(self._h, file, C.byref(m), C.byref(ib), C.byref(to))
        if rc != Z_OK:
            raise ValueError(f"zsc_hip_bgzf_index_info failed: {rc}")
        return m.value, ib.value, to.value

    def table(self, file: int = 0) -> Tuple[List[int], List[int]]:
        """(coffsets, uoffsets) of a file: members + 1 entries each, the last the end entry"""
        n = self.info(file)[0] + 1
        c, u = (C.c_uint64 * n)(), (C.c_uint64 * n)()
        rc = lib.zsc_hip_bgzf_index_table(self._h, file, c, u, n)
        if rc != Z_OK:
            raise RuntimeError(f"zsc_hip_bgzf_index_table failed: {rc}")
        return list(c), list(u)

    def voffset(self, uoffset: int, file: int = 0) -> int:
        """the virtual offset (coffset << 16 | offset within the member) of uncompressed offset uoffset"""
        v = C.c_uint64()
        if lib.zsc_hip_bgzf_index_voffset(self._h, file, uoffset, C.byref(v)) != Z_OK:
            raise ValueError(f"uncompressed offset {uoffset} is beyond the end of file {file}")
        return v.value

    def uoffset(self, voffset: int, file: int = 0) -> int:
        """the uncompressed offset of a virtual offset of the index"""
        u = C.c_uint64()
        if lib.zsc_hip_bgzf_index_uoffset(self._h, file, voffset, C.byref(u)) != Z_OK:
            raise ValueError(f"virtual offset {voffset:#x} is not of the index of file {file}")
        return u.value

    def to_gzi(self, file: int = 0) -> bytes:
        """the index of a file as a .gzi image"""
        need = C.c_uint64(0)
        lib.zsc_hip_bgzf_index_export_gzi(self._h, file, None, C.byref(need))
        buf = C.create_string_buffer(need.value)
        rc = lib.zsc_hip_bgzf_index_export_gzi(self._h, file, buf, C.byref(need))
        if rc != Z_OK:
            raise RuntimeError(f"zsc_hip_bgzf_index_export_gzi failed: {rc}")
        return buf.raw[:need.value]

    def build_ms(self) -> float:
        """device time of the build's launches"""
        return float(lib.zsc_hip_bgzf_index_build_ms(self._h))

    def scratch_bytes(self) -> int:
        return int(lib.zsc_hip_bgzf_index_scratch_bytes(self._h))

    def close(self) -> None:
        if self._h:
            lib.zsc_hip_bgzf_index_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BgzfRangesPlan(InflatePlan):
    """A ranges plan (zsc_hip_inflate_plan_create_bgzf_ranges): request i is bytes [begins[i], begins[i] + lens[i])
    of the uncompressed content of file files[i] of the index, decoded from the members it touches alone into
    [dst_offsets[i], + dest_caps[i]) of run()'s d_dst; d_src is the batch the index was built over.  With
    voffsets=True begins and lens are begin and END virtual offsets (ValueError where one is not of the index).
    run, results, pack_enable / pack, scratch_bytes and close are InflatePlan's; the index may be closed before
    the run.  Also made by InflatePlan.bgzf_ranges(...)."""

    def __init__(self, index: BgzfIndex, files: Sequence[int], begins: Sequence[int], lens: Sequence[int],
                 dest_caps: Sequence[int], voffsets: bool = False, dst_offsets: Sequence[int] | None = None):
        self.count = n = len(files)
        if not (len(begins) == len(lens) == len(dest_caps) == n):
            raise ValueError("one file, begin, length and capacity per request")
        do, db = [], 0
        for dc in dest_caps:
            do.append(db)
            db += (dc + 64 + 15) & ~15
        if dst_offsets is not None:
            do = list(dst_offsets)
            db = max([o + c for o, c in zip(do, dest_caps)], default=0)
        self.src_offsets, self.src_bytes = index.src_offsets, index.src_bytes
        self.dst_offsets, self.dst_bytes = do, db + 64
        self._h = C.c_void_p()
        m = max(n, 1)
        rc = lib.zsc_hip_inflate_plan_create_bgzf_ranges(C.byref(self._h), index._h, n, (C.c_uint32 * m)(*files),
                                                         (C.c_uint64 * m)(*begins), (C.c_uint64 * m)(*lens),
                                                         (C.c_uint32 * m)(*dest_caps), (C.c_uint64 * m)(*do),
                                                         BGZF_VOFFSETS if voffsets else 0)
        if rc == Z_STREAM_ERROR:
            raise ValueError("a request names no file of the index, an offset that is not of it, or an end before its begin")
        if rc != Z_OK:
            raise RuntimeError(f"zsc_hip_inflate_plan_create_bgzf_ranges failed: {rc}")

    def jobs(self) -> Tuple[int, int]:
        """(member jobs of the plan, the bytes they decode in a run)"""
        j, b = C.c_uint64(), C.c_uint64()
        rc = lib.zsc_hip_inflate_plan_bgzf_jobs(self._h, C.byref(j), C.byref(b))
        if rc != Z_OK:
            raise RuntimeError(f"zsc_hip_inflate_plan_bgzf_jobs failed: {rc}")
        return j.value, b.value

    def index_enable(self, enable: bool = True) -> int:
        """(zsc_hip_inflate_plan_index_enable: Z_STREAM_ERROR on a ranges plan)"""
        return lib.zsc_hip_inflate_plan_index_enable(self._h, 1 if enable else 0)


InflatePlan.bgzf_ranges = staticmethod(BgzfRangesPlan)


def bgzf_read_ranges(files: Sequence[bytes], requests: Sequence[Tuple[int, int, int]],
                     dest_caps: Sequence[int] | None = None, voffsets: bool = False):
    """zsc_hip_bgzf_read_ranges_batch: requests[i] = (file, begin, length) -- with voffsets=True (file, begin
    virtual offset, end virtual offset) -- read out of BGZF files in host memory: one upload per file, an index, a
    ranges plan, one download.  dest_caps: the room per request (None: the length asked for, capped at 4 GiB - 1;
    needed with voffsets).  Returns (rc, [bytes], [dest_len], [status]); the bytes of a request that is not Z_OK
    are empty."""
    nf, n = len(files), len(requests)
    if dest_caps is None:
        if voffsets:
            raise ValueError("dest_caps are needed with virtual offsets")
        dest_caps = [min(r[2], 0xffffffff) for r in requests]
    srcs = (C.c_char_p * max(nf, 1))(*files)
    slen = (C.c_uint32 * max(nf, 1))(*[len(f) for f in files])
    bufs = [C.create_string_buffer(max(c, 1)) for c in dest_caps]
    dsts = (C.c_void_p * max(n, 1))(*[C.cast(b, C.c_void_p) for b in bufs])
    dlen = (C.c_uint32 * max(n, 1))(*dest_caps)
    stat = (C.c_int32 * max(n, 1))()
    rc = lib.zsc_hip_bgzf_read_ranges_batch(nf, srcs, slen, n, (C.c_uint32 * max(n, 1))(*[r[0] for r in requests]),
                                            (C.c_uint64 * max(n, 1))(*[r[1] for r in requests]),
                                            (C.c_uint64 * max(n, 1))(*[r[2] for r in requests]), dsts, dlen, stat,
                                            BGZF_VOFFSETS if voffsets else 0)
    if rc != Z_OK:
        return rc, [], [], []
    outs = [bufs[i].raw[:dlen[i]] if stat[i] == Z_OK else b"" for i in range(n)]
    return rc, outs, list(dlen)[:n], list(stat)[:n]


class DeflatePlan(_Packing):
    """A device-resident batch: fixed buffer lengths, inputs/outputs stay in HBM.

    ``layout`` gives the byte offsets of every buffer inside one input and one output
    allocation; ``run`` takes raw device pointers (e.g. ``tensor.data_ptr()``), so the
    binding itself needs neither torch nor numpy.  ``out_caps`` (default: the layout's own, the worst case)
    gives stream i less room than that: a stream that does not fit ends in Z_BUF_ERROR.
    """
    _pack_kind = "deflate"

    def __init__(self, source_lens: Sequence[int], level: int = 6, window_bits: int = DEF_WBITS,
                 mem_level: int = DEF_MEM_LEVEL, strategy: int = Z_DEFAULT_STRATEGY,
                 out_caps: Sequence[int] | None = None):
        self.count = n = len(source_lens)
        self.source_lens = list(source_lens)
        lens = (C.c_uint32 * n)(*source_lens)
        self._in_off = (C.c_uint64 * n)()
        self._out_off = (C.c_uint64 * n)()
        self._caps = (C.c_uint32 * n)()
        ib, ob = C.c_uint64(), C.c_uint64()
        rc = lib.zsc_hip_deflate_plan_layout(n, lens, level, window_bits, mem_level, self._in_off,
                                             self._out_off, self._caps, C.byref(ib), C.byref(ob))
        if rc != Z_OK:
            raise ValueError(f"zsc_hip_deflate_plan_layout failed: {rc}")
        self.in_bytes, self.out_bytes = ib.value, ob.value
        if out_caps is not None:
            if len(out_caps) != n or any(c > full for c, full in zip(out_caps, self._caps)):
                raise ValueError("one capacity per buffer, none above the layout's")
            self._caps = (C.c_uint32 * n)(*out_caps)
        self.in_offsets = list(self._in_off)
        self.out_offsets = list(self._out_off)
        self.out_caps = list(self._caps)
        self._h = C.c_void_p()
        rc = lib.zsc_hip_deflate_plan_create(C.byref(self._h), n, lens, self._in_off, self._out_off,
                                             self._caps, level, window_bits, mem_level, strategy)
        if rc != Z_OK:
            raise RuntimeError(f"zsc_hip_deflate_plan_create failed: {rc}")

    @property
    def scratch_bytes(self) -> int:
        return lib.zsc_hip_deflate_plan_scratch_bytes(self._h)

    @property
    def sub_batches(self) -> int:
        return lib.zsc_hip_deflate_plan_sub_batches(self._h)

    @property
    def seg_schedule(self) -> str:
        """How long plain buffers are parsed at levels 4-9: "none", "super-steps" or "pipeline"."""
        return ("none", "super-steps", "pipeline")[lib.zsc_hip_deflate_plan_seg_schedule(self._h)]

    @property
    def seg_ring(self) -> str:
        """The LDS geometry that parser runs in: "none", "wide", "narrow", or "mixed" when the plan's sub-batches
        differ (each goes by the long buffers it has per CU unless ZSC_HIP_SEG_RING says it at plan creation)."""
        return ("none", "wide", "narrow", "mixed")[lib.zsc_hip_deflate_plan_seg_ring(self._h)]

    def profile(self, enable: bool = True) -> None:
        lib.zsc_hip_deflate_plan_profile(self._h, 1 if enable else 0)

    def run(self, d_input: int, d_output: int, stream: int = 0) -> None:
        """stream (a hipStream_t as an int, e.g. torch.cuda.Stream().cuda_stream): the run is ordered in it like a
        kernel, and on another stream than the plan's unfinished run, verify or pack it waits for that on the device."""
        rc = lib.zsc_hip_deflate_plan_run(self._h, C.c_void_p(d_input), C.c_void_p(d_output),
                                          C.c_void_p(stream))
        if rc != Z_OK:
            raise RuntimeError(f"zsc_hip_deflate_plan_run failed: {rc}")

    def results(self) -> Tuple[List[int], List[int]]:
        lens = (C.c_uint32 * self.count)()
        stat = (C.c_int32 * self.count)()
        rc = lib.zsc_hip_deflate_plan_results(self._h, lens, stat)
        if rc != Z_OK:
            raise RuntimeError(f"zsc_hip_deflate_plan_results failed: {rc}")
        return list(lens), list(stat)

    def kernel_times_ms(self) -> dict:
        t = (C.c_float * NKERNELS)()
        rc = lib.zsc_hip_deflate_plan_times(self._h, t)
        if rc != Z_OK:
            raise RuntimeError("profiling was not enabled before the run")
        return dict(zip(KERNEL_NAMES, list(t)))

    def index_enable(self, chunk_bytes: int = 0) -> None:
        """Before run(): every run also writes the seek-point index of every stream, one point per
        chunk_bytes compressed bytes at the most (0: the library's default, 128 KiB)."""
        rc = lib.zsc_hip_deflate_plan_index_enable(self._h, chunk_bytes)
        if rc != Z_OK:
            raise RuntimeError(f"zsc_hip_deflate_plan_index_enable failed: {rc}")

    def export_indexes(self, d_input_ptr: int) -> List[Optional[bytes]]:
        """After results() of a plan with index_enable: the blob of every buffer, None for a buffer whose
        status is not Z_OK.  d_input_ptr is the device input the run read, unchanged since."""
        out: List[Optional[bytes]] = []
        for i in range(self.count):
            need = C.c_uint64()
            rc = lib.zsc_hip_deflate_plan_index_size(self._h, i, C.byref(need))
            if rc == Z_DATA_ERROR:
                out.append(None)
                continue
            if rc != Z_OK:
                raise RuntimeError(f"zsc_hip_deflate_plan_index_size failed: {rc}")
            buf = C.create_string_buffer(need.value)
            got = C.c_uint64()
            rc = lib.zsc_hip_deflate_plan_index_export(self._h, i, C.c_void_p(d_input_ptr), buf, need.value,
                                                       C.byref(got))
            if rc != Z_OK:
                raise RuntimeError(f"zsc_hip_deflate_plan_index_export failed: {rc}")
            out.append(buf.raw[:got.value])
        return out

    def index_ms(self) -> float:
        """After results(), with profile() on: device time of the index launches per run, in milliseconds."""
        ms = C.c_float()
        if lib.zsc_hip_deflate_plan_index_ms(self._h, C.byref(ms)) != Z_OK:
            raise RuntimeError("the index or profiling was not enabled before the run")
        return ms.value

    def verify_enable(self) -> None:
        """Before run(): every run also keeps where each block of each stream starts and which input bytes
        it stands for, so that verify() can check the streams against the input on the device."""
        rc = lib.zsc_hip_deflate_plan_verify_enable(self._h)
        if rc != Z_OK:
            raise RuntimeError(f"zsc_hip_deflate_plan_verify_enable failed: {rc}")

    def verify(self, d_input: int, d_output: int, stream: int = 0) -> int:
        """After results(), any number of times: enqueue the verification of the streams at d_output (the
        run's output or a copy of it, with the plan's out_offsets) against the input at d_input.  Returns
        the ZlibReturn: Z_STREAM_ERROR on a plan without verify_enable().
        stream: the verification is ordered in it like a kernel; the plan's next run, results() and close() wait for it."""
        return lib.zsc_hip_deflate_plan_verify(self._h, C.c_void_p(d_input), C.c_void_p(d_output), C.c_void_p(stream))

    def verify_results(self) -> List[dict]:
        """Waits for the last verify(): per buffer {"verdict", "block", "bit_off", "in_pos"} -- verdict one of
        VERIFY_*, block the lowest-numbered failing block (0xFFFFFFFF where the verdict names none)."""
        res = (VerifyResult * max(self.count, 1))()
        ms = C.c_float()
        rc = lib.zsc_hip_deflate_plan_verify_results(self._h, res, C.byref(ms))
        if rc != Z_OK:
            raise RuntimeError(f"zsc_hip_deflate_plan_verify_results failed: {rc}")
        self._verify_ms = ms.value
        return [{"verdict": r.verdict, "block": r.block, "bit_off": r.bit_off, "in_pos": r.in_pos}
                for r in res[:self.count]]

    def verify_ms(self) -> float:
        """After verify_results(): device time of that verification's launches, in milliseconds."""
        if getattr(self, "_verify_ms", None) is None:
            raise RuntimeError("no verify_results() yet")
        return self._verify_ms

    def verify_blocks(self, i: int) -> List[Tuple[int, int, int, int, int]]:
        """After results() of a plan with verify_enable(): the block map of buffer i, in stream order:
        (bit_off, in_begin, in_len, type, last) -- type 0 stored, 1 static, 2 dynamic.  [] for a buffer whose
        status is not Z_OK."""
        n = C.c_uint32()
        rc = lib.zsc_hip_deflate_plan_verify_blocks(self._h, i, None, 0, C.byref(n))
        if rc == Z_DATA_ERROR:
            return []
        if rc not in (Z_OK, Z_BUF_ERROR):
            raise RuntimeError(f"zsc_hip_deflate_plan_verify_blocks failed: {rc}")
        blocks = (VerifyBlock * max(n.value, 1))()
        rc = lib.zsc_hip_deflate_plan_verify_blocks(self._h, i, blocks, n.value, C.byref(n))
        if rc != Z_OK:
            raise RuntimeError(f"zsc_hip_deflate_plan_verify_blocks failed: {rc}")
        return [(b.bit_off, b.in_begin, b.in_len, b.type_last & 0xff, b.type_last >> 8) for b in blocks[:n.value]]

    def bgzf_enable(self, file_first: Sequence[int], align: int = 1) -> None:
        """Before run(), on a gzip plan (window_bits 31) whose buffers are 65 536 bytes at the most: the plan can
        write its streams as BGZF files, file f the buffers file_first[f] .. file_first[f + 1] (nfiles + 1
        values ascending from 0 to count), each file at a multiple of align.  Calling it again replaces the
        partition.  ValueError, the plan as it was, where the library refuses."""
        nfiles = len(file_first) - 1
        if nfiles < 0:
            raise ValueError("file_first holds nfiles + 1 values")
        rc = lib.zsc_hip_deflate_plan_bgzf_enable(self._h, nfiles, (C.c_uint32 * (nfiles + 1))(*file_first), align)
        if rc != Z_OK:
            raise ValueError(f"zsc_hip_deflate_plan_bgzf_enable failed: {rc}")
        self._bgzf_files = nfiles

    def bgzf(self, d_output: int, d_image: int, cap: int, stream: int = 0) -> int:
        """After run() on the same stream, or after results(), any number of times: enqueue the writing of the
        files from the streams at d_output (the run's output or a copy of it, with the plan's out_offsets) into
        the cap bytes at d_image (16-byte aligned).  Returns the ZlibReturn: Z_STREAM_ERROR on a plan without
        bgzf_enable().  stream: ordered in it like a kernel; the plan's next run, results() and close() wait."""
        return lib.zsc_hip_deflate_plan_bgzf(self._h, C.c_void_p(d_output), C.c_void_p(d_image), cap, C.c_void_p(stream))

    def bgzf_results(self) -> dict:
        """Waits for the last bgzf(): {"file_offsets" (nfiles + 1), "file_lens", "file_statuses", "member_offsets"
        (count), "total"}.  A failed file (Z_BUF_ERROR: a buffer that is not Z_OK or whose member would pass
        65 536 bytes) has length 0.  BufferError, with .tables, where the image was longer than cap (nothing was
        written)."""
        nf = getattr(self, "_bgzf_files", 0)
        foff, flen = (C.c_uint64 * (nf + 1))(), (C.c_uint64 * max(nf, 1))()
        fst, moff = (C.c_int32 * max(nf, 1))(), (C.c_uint64 * max(self.count, 1))()
        total, ms = C.c_uint64(), C.c_float()
        rc = lib.zsc_hip_deflate_plan_bgzf_results(self._h, foff, flen, fst, moff, C.byref(total), C.byref(ms))
        self._bgzf_ms = ms.value
        tables = {"file_offsets": list(foff), "file_lens": list(flen)[:nf], "file_statuses": list(fst)[:nf],
                  "member_offsets": list(moff)[:self.count], "total": total.value}
        if rc == Z_BUF_ERROR:
            err = BufferError(f"the BGZF image takes {total.value} bytes")
            err.tables = tables
            raise err
        if rc != Z_OK:
            raise RuntimeError(f"zsc_hip_deflate_plan_bgzf_results failed: {rc}")
        return tables

    def bgzf_ms(self) -> float:
        """After bgzf_results(): device time of that bgzf()'s launches, in milliseconds."""
        if getattr(self, "_bgzf_ms", None) is None:
            raise RuntimeError("no bgzf_results() yet")
        return self._bgzf_ms

    def zip_enable(self, arch_first: Sequence[int], names: Sequence[bytes],
                   dos_datetime: Optional[Sequence[int]] = None, utf8: bool = False, align: int = 1) -> None:
        """Before run(), on a gzip plan (window_bits 31): the plan can write its streams as ZIP archives, archive a
        the buffers arch_first[a] .. arch_first[a + 1] (narchives + 1 values ascending from 0 to count), buffer i
        named names[i] (bytes, 65 535 at the most), each archive at a multiple of align.  dos_datetime[i] is
        date << 16 | time (default 1980-01-01 00:00:00); utf8 sets the entries' UTF-8 flag.  Calling it again
        replaces everything.  ValueError, the plan as it was, where the library refuses."""
        na = len(arch_first) - 1
        if na < 0 or len(names) != self.count or (dos_datetime is not None and len(dos_datetime) != self.count):
            raise ValueError("arch_first holds narchives + 1 values; names and dos_datetime one per buffer")
        offs = [0]
        for nm in names:
            offs.append(offs[-1] + len(nm))
        dt = None if dos_datetime is None else (C.c_uint32 * max(self.count, 1))(*dos_datetime)
        rc = lib.zsc_hip_deflate_plan_zip_enable(self._h, na, (C.c_uint32 * (na + 1))(*arch_first), b"".join(names),
                                                 (C.c_uint64 * (self.count + 1))(*offs), dt, ZIP_UTF8 if utf8 else 0,
                                                 align)
        if rc != Z_OK:
            raise ValueError(f"zsc_hip_deflate_plan_zip_enable failed: {rc}")
        self._zip_archives = na

    def zip(self, d_output: int, d_image: int, cap: int, stream: int = 0) -> int:
        """After run() on the same stream, or after results(), any number of times: enqueue the writing of the
        archives from the streams at d_output (the run's output or a copy of it, with the plan's out_offsets) into
        the cap bytes at d_image (16-byte aligned).  Returns the ZlibReturn: Z_STREAM_ERROR on a plan without
        zip_enable().  stream: ordered in it like a kernel; the plan's next run, results() and close() wait."""
        return lib.zsc_hip_deflate_plan_zip(self._h, C.c_void_p(d_output), C.c_void_p(d_image), cap, C.c_void_p(stream))

    def zip_results(self) -> dict:
        """Waits for the last zip(): {"arch_offsets" (narchives + 1), "arch_lens", "arch_statuses", "entry_offsets"
        and "data_offsets" (count: where a buffer's local header and its DEFLATE body start), "dir_offsets"
        (narchives), "total"}.  A failed archive (Z_BUF_ERROR: a buffer that is not Z_OK; Z_MEM_ERROR: longer than
        4 294 967 295 bytes) has length 0.  BufferError, with .tables, where the image was longer than cap
        (nothing was written)."""
        na = getattr(self, "_zip_archives", 0)
        aoff, alen, ast = (C.c_uint64 * (na + 1))(), (C.c_uint64 * max(na, 1))(), (C.c_int32 * max(na, 1))()
        eoff, doff = (C.c_uint64 * max(self.count, 1))(), (C.c_uint64 * max(self.count, 1))()
        diro, total, ms = (C.c_uint64 * max(na, 1))(), C.c_uint64(), C.c_float()
        rc = lib.zsc_hip_deflate_plan_zip_results(self._h, aoff, alen, ast, eoff, doff, diro, C.byref(total), C.byref(ms))
        self._zip_ms = ms.value
        tables = {"arch_offsets": list(aoff), "arch_lens": list(alen)[:na], "arch_statuses": list(ast)[:na],
                  "entry_offsets": list(eoff)[:self.count], "data_offsets": list(doff)[:self.count],
                  "dir_offsets": list(diro)[:na], "total": total.value}
        if rc == Z_BUF_ERROR:
            err = BufferError(f"the ZIP image takes {total.value} bytes")
            err.tables = tables
            raise err
        if rc != Z_OK:
            raise RuntimeError(f"zsc_hip_deflate_plan_zip_results failed: {rc}")
        return tables

    def zip_ms(self) -> float:
        """After zip_results(): device time of that zip()'s launches, in milliseconds."""
        if getattr(self, "_zip_ms", None) is None:
            raise RuntimeError("no zip_results() yet")
        return self._zip_ms

    def close(self) -> None:
        if self._h:
            lib.zsc_hip_deflate_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
