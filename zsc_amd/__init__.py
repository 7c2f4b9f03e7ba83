"""zsc_amd -- MI355X-native DEFLATE hot path behind zsc's own API.

Host-side mirror (Python, ctypes) of the C ABI exported by ``libzsc_hip.so``:

* :func:`compress`, :func:`compress2`, :func:`compress_gzip`, :func:`uncompress` ... --
  the reference's one-shot functions (``include/zsc/zsc_pub.h``), same argument
  meaning and ``ZlibReturn`` codes;
* :func:`compress_batch` -- many independent buffers per call;
* :func:`uncompress_sections_batch` -- the full-flush sections of each stream inflated in parallel;
* :func:`uncompress_chunks_batch` -- any long stream inflated in parallel pieces from block starts
  found by trial;
* :func:`uncompress_resync_batch` -- full-flush sections inflated in parallel, damaged streams
  resynchronised at the next flush marker as zsc_uncompress does;
* :func:`uncompress_sizes_batch`, :func:`uncompress_batch_auto` -- what streams of unknown length inflate
  to, found on the device without writing any output (``InflatePlan(..., size_only=True)``), and the
  size-allocate-inflate sequence in one call;
* :func:`uncompress_check_batch` -- are the streams intact?  Status, length, consumed and the check value of
  every stream, found on the device without writing any output (``InflatePlan(..., check_only=True)``);
* :func:`uncompress_members_batch` -- multi-member gzip files (packed archives of gzip streams, BGZF,
  concatenated .gz files) inflated member by member in parallel (``InflatePlan(..., members=True)``);
* :func:`uncompress_dict_batch` -- streams that use zlib preset dictionaries, each with one of a set of
  shared dictionaries or none (``InflatePlan(..., dicts=[...], stream_dict=[...])``); decompression only;
* :func:`build_indexes`, :func:`uncompress_indexed_batch`, :func:`index_info`, :func:`index_range` --
  seek-point indexes: exported once from a chunks plan, then every later decode (or a range out of the
  middle) without the discovery;
* :func:`compress_batch_indexed` -- streams written together with their seek-point indexes
  (``DeflatePlan.index_enable`` / ``export_indexes``): no chunks plan is ever needed for them;
* :func:`compress_batch_verified` -- streams checked against their input on the device, block by block,
  before they leave it (``DeflatePlan.verify_enable`` / ``verify`` / ``verify_results``);
* :func:`compress_batch_packed`, :func:`uncompress_batch_packed`, :func:`unpack` -- batches as ONE image with a
  table of offsets: one copy to the device and one back whatever the count (``DeflatePlan.pack_enable`` /
  ``pack`` / ``pack_results``, the same on :class:`InflatePlan`);
* :func:`bgzf_compress_batch` -- files written as BGZF, the block-gzip container of bgzip, BAM and tabix, which a
  members plan reads back member by member (``DeflatePlan.bgzf_enable`` / ``bgzf`` / ``bgzf_results``);
* :class:`BgzfIndex`, :class:`BgzfRangesPlan` (``InflatePlan.bgzf_ranges``), :func:`bgzf_read_ranges` -- ranges read out
  of BGZF files by uncompressed or virtual offset: a member index built from the headers alone (``to_gzi`` /
  ``from_gzi``), and a plan that decodes only the members its requests touch;
* :func:`zip_compress_batch` -- lists of named buffers written as ZIP archives (``.npz``, wheels, jars, OOXML), which
  CPython's ``zipfile`` reads (``DeflatePlan.zip_enable`` / ``zip`` / ``zip_results``);
* :class:`DeflatePlan` -- device-resident batches (inputs and outputs stay in HBM).

There is no CPU codec here: if the HIP library is missing, import fails loudly.
"""
from .api import (  # noqa: F401
    Z_OK, Z_STREAM_END, Z_STREAM_ERROR, Z_DATA_ERROR, Z_MEM_ERROR, Z_BUF_ERROR,
    Z_DEFAULT_STRATEGY, Z_FILTERED, Z_FIXED, GZIP_CODE, DEF_WBITS, DEF_MEM_LEVEL,
    lib, lib_path, build_library, device_info,
    compress_get_min_work_buf_size, compress_get_max_output_size, compress_get_max_output_size2,
    uncompress_get_min_work_buf_size,
    compress, compress2, compress_gzip, uncompress, uncompress2, uncompress_gzip,
    compress_batch, compress_sections_batch, compress_sections_device, compress_sections_last_rings, uncompress_batch, uncompress_sections_batch,
    uncompress_chunks_batch, uncompress_resync_batch, DeflatePlan, InflatePlan,
    uncompress_sizes_batch, uncompress_batch_auto, NO_LIMIT, uncompress_check_batch,
    uncompress_members_batch, MEMBERS_SIZE_ONLY,
    uncompress_dict_batch, NO_DICT,
    uncompress_indexed_batch, build_indexes, index_info, index_range, compress_batch_indexed,
    compress_batch_verified, VERIFY_OK, VERIFY_SKIPPED, VERIFY_HEADER, VERIFY_BLOCK_HDR, VERIFY_CODES, VERIFY_LITERAL,
    VERIFY_DISTANCE, VERIFY_MATCH, VERIFY_LENGTH, VERIFY_BIT_END, VERIFY_TRAILER,
    PACK_TILE, unpack, compress_batch_packed, uncompress_batch_packed, PackedCallError,
    bgzf_compress_batch, BgzfIndex, BgzfRangesPlan, bgzf_read_ranges, BGZF_VOFFSETS,
    zip_compress_batch, ZIP_UTF8,
    GzHeader, gz_header_for_writing, gz_header_for_reading, gz_header_fields,
)
