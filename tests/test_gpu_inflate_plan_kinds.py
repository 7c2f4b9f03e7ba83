"""Every kind of inflate plan through the whole host interface (create, run, results, sections(), data_errors(),
scratch_bytes(), run again, results again, close) on three small batches: what the plans' shared host code has to
keep for each kind, where the other GPU tests look at one kind at a time."""
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNK = 4096  # CHK_MIN_BYTES
KINDS = ("plain", "sections", "chunks", "resync", "indexed", "size", "check")

# structure sizes (inflate.h, inflate_sections.h, inflate_resync.h, inflate_index.h) and constants
ITEM, TILE, STREAM, RSY_STREAM, IDX_STREAM, IDX_PIECE, RESULT, RESUME = 40, 8, 48, 16, 40, 48, 16, 28
SEC_TILE, PC_CANDS, WIN, RING, PER_WAVE = 4096, 4, 32768, 65536, 4


def _inflate(s):
    d = zlib.decompressobj(15)
    out = d.decompress(s)
    return out, len(s) - len(d.unused_data)


def batches():
    """count == 0; outputs of 0, 1 and 300 bytes; those and incompressible bytes, a full flush in their middle,
    whose stream is a little longer than three chunks of the least size"""
    small = [zlib.compress(b""), zlib.compress(b"z"), zlib.compress(bytes(range(100)) * 3)]
    noise = np.random.default_rng(77).integers(0, 256, 12400, dtype=np.uint8).tobytes()
    co = zlib.compressobj(6, zlib.DEFLATED, 15)
    big = co.compress(noise[:6200]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(noise[6200:]) + co.flush()
    assert 3 * CHUNK < len(big) < 3 * CHUNK + 256
    return [[], small, small + [big]]


def parent_scratch(kind, lens, caps, blobs):
    """the scratch figure of the plans' host code before it was built from shared parts, term by term"""
    count = len(lens)
    nc = max(1, count)
    if kind == "plain":
        return 0
    if kind in ("sections", "resync"):
        nt = max(1, sum((n + SEC_TILE - 1) // SEC_TILE for n in lens))
        cand = min(sum(lens) // 256 + 65536, 0x0ffffff0)
        own = ITEM * nc + (TILE + 8) * nt + (8 + STREAM + 4) * nc + 16 + 28 * cand
        return own + (12 * cand + RSY_STREAM * nc if kind == "resync" else 0)
    if kind == "indexed":
        np_, ncand, win = 0, 0, WIN
        for b in blobs:
            if b is None:
                continue
            (n,) = struct.unpack_from("<I", b, 40)
            (cb,) = struct.unpack_from("<I", b, 24)
            (last_bit,) = struct.unpack_from("<Q", b, 48 + 32 * (n - 1))
            np_ += n
            ncand += (last_bit // (8 * cb) + 1) * PC_CANDS if n > 1 else 0
            win += sum(struct.unpack_from("<I", b, 48 + 32 * j + 28)[0] for j in range(n))
        np_, ncand = max(1, np_), max(1, ncand)
        return ((ITEM + 2 * STREAM + IDX_STREAM + 4 + 4 + 4 + RESULT + RESUME) * nc + 16 + 16 + (IDX_PIECE + 16) * np_ +
                8 * ncand + win)
    cut = [(n + CHUNK - 1) // CHUNK for n, c in zip(lens, caps) if n > CHUNK and (kind != "chunks" or c < 1 << 31)]
    nchunks = sum(cut)
    nt, ch = max(1, nchunks - len(cut)), max(1, nchunks)
    base = (ITEM + STREAM + 8) * nc + 16 + TILE * nt
    if kind == "chunks":
        return base + (8 * PC_CANDS + 36 + 3 * WIN) * ch
    if kind == "size":
        return base + (8 * PC_CANDS + 32) * ch
    waves = max(1, (count + PER_WAVE - 1) // PER_WAVE)  # (far below what fills the device)
    return base + (8 * PC_CANDS + 36 + 3 * WIN) * nchunks + RING * waves * PER_WAVE + 4 * nc


def make_plan(kind, lens, caps, blobs=None):
    import zsc_amd
    if kind == "plain":
        return zsc_amd.InflatePlan(lens, caps)
    if kind == "sections":
        return zsc_amd.InflatePlan(lens, caps, sections=True)
    if kind == "resync":
        return zsc_amd.InflatePlan(lens, caps, resync=True)
    if kind == "chunks":
        return zsc_amd.InflatePlan(lens, caps, chunks=True, chunk_bytes=CHUNK)
    if kind == "indexed":
        return zsc_amd.InflatePlan(lens, caps, indexes=blobs)
    return zsc_amd.InflatePlan(lens, caps, size_only=kind == "size", check_only=kind == "check", chunk_bytes=CHUNK)


def upload(torch, plan, streams):
    src = torch.zeros(plan.src_bytes, dtype=torch.uint8, device="cuda")
    for s, off in zip(streams, plan.src_offsets):
        src[off:off + len(s)] = torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda()
    return src


def build_blobs(torch, streams, caps):
    """the indexes of the batch, from a chunks plan that keeps them (None for a stream decoded serially)"""
    import zsc_amd
    plan = zsc_amd.InflatePlan([len(s) for s in streams], caps, chunks=True, chunk_bytes=CHUNK, keep_index=True)
    src = upload(torch, plan, streams)
    dst = torch.zeros(plan.dst_bytes, dtype=torch.uint8, device="cuda")
    plan.run(src.data_ptr(), dst.data_ptr(), 0)
    plan.results()
    blobs = [plan.export_index(i) for i in range(len(streams))]
    plan.close()
    return blobs


@pytest.fixture(scope="module")
def cases():
    import torch
    out = []
    for streams in batches():
        want = [_inflate(s) for s in streams]
        caps = [len(w[0]) for w in want]
        out.append((streams, want, caps, build_blobs(torch, streams, caps)))
    assert [b is not None for b in out[2][3]] == [False, False, False, True]
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_every_entry_point_of_a_kind(cases, kind):
    import torch
    for streams, want, caps, blobs in cases:
        count = len(streams)
        lens = [len(s) for s in streams]
        plan = make_plan(kind, lens, caps, blobs)
        assert plan.sections() == [0] * count and plan.data_errors() == [0] * count
        src = upload(torch, plan, streams)
        writes = kind not in ("size", "check")
        dst = torch.zeros(plan.dst_bytes, dtype=torch.uint8, device="cuda") if writes else None
        seen = []
        for _ in range(2):
            if writes:
                dst.zero_()
            plan.run(src.data_ptr(), dst.data_ptr() if writes else 0, 0)
            got_lens, used, stat, _ = plan.results()
            assert stat == [0] * count
            assert got_lens == caps and used == [w[1] for w in want]
            if writes:
                host = dst.cpu().numpy()
                assert [bytes(host[o:o + n]) for o, n in zip(plan.dst_offsets, got_lens)] == [w[0] for w in want]
            if kind == "check" and count:  # (a run of no streams is none: the values stay refused)
                assert plan.check_values() == [zlib.adler32(w[0]) for w in want]
            pieces = plan.sections()
            print(kind, count, pieces, plan.scratch_bytes())
            assert plan.data_errors() == [0] * count
            assert plan.scratch_bytes() == parent_scratch(kind, lens, caps, blobs)
            assert pieces[:3] == [0] * min(count, 3) and (kind != "plain" or pieces == [0] * count)
            if count == 4 and kind in ("sections", "resync"):
                assert pieces[3] >= 2  # (the full flush cuts it)
            seen.append(pieces)
        assert seen[0] == seen[1]
        plan.close()


def test_create_refuses_bad_arguments():
    import zsc_amd
    with pytest.raises(RuntimeError):
        zsc_amd.InflatePlan([10, 10, 10], [10, 10, 10], src_offsets=[0, 8, 96])
    with pytest.raises(RuntimeError):
        zsc_amd.InflatePlan([10, 10, 10], [10, 10, 10], decode_order=[0, 0, 1])
