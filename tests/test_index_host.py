"""The host functions of the seek-point index through libzsc_hip.so (no device needed): validate, info and
range on blobs made by the lane emulation of the export."""
import pytest

import zsc_amd
from zsc_amd import corpus
from test_inflate_chunks_emu import CHUNK, zlib_stream
from test_inflate_index_emu import build, covering_run, flip, idx, points, reseal  # noqa: F401  (idx: the fixture)


def test_info_and_range_agree_with_the_blob(idx):
    text = corpus.make_buffer("text", 300000, 31)
    for wbits in (15, 31, -15):
        s = zlib_stream(text, 6, wbits)
        rc, out, used, npieces, blob = build(idx, s, len(text), wbits)
        assert rc == 0 and npieces > 1
        assert zsc_amd.lib.zsc_hip_index_validate(blob, len(blob)) == 0
        h = zsc_amd.index_info(blob)
        assert h == {"window_bits": wbits, "wrapper": {15: 1, 31: 2, -15: 0}[wbits], "gzip": int(wbits == 31),
                     "dist_limit": 32768, "chunk_bytes": CHUNK, "consumed": len(s), "total_out": len(text),
                     "trailer_offset": len(s) - {15: 4, 31: 8, -15: 0}[wbits], "points": npieces}
        pts = points(blob)
        for b, n in ((0, 1), (len(text) - 1, 1), (0, len(text)), (pts[2]["off"] - 1, 2), (123456, 50000)):
            assert zsc_amd.index_range(blob, b, n) == covering_run(pts, b, n)
        for bad in (blob[:-1], flip(blob, 30, 0), reseal(flip(blob, 44, 5)), b""):
            assert zsc_amd.lib.zsc_hip_index_validate(bad, len(bad)) == zsc_amd.Z_DATA_ERROR
            with pytest.raises(ValueError):
                zsc_amd.index_info(bad)
            with pytest.raises(ValueError):
                zsc_amd.index_range(bad, 0, 1)
        with pytest.raises(ValueError):
            zsc_amd.index_range(blob, len(text), 1)
