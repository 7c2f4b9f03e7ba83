"""The two schedules of the segmented parser on a real MI355X: the pipeline of segments
(lz_parse_pipe.h, the default for plain buffers) and the super-steps (ZSC_HIP_SEG_PIPE=0, read when
a plan is created).  Every stream equals the oracle's and the two schedules equal each other."""
import os

import pytest

pytestmark = pytest.mark.gpu

from zsc_amd import corpus  # noqa: E402

KINDS = ("text", "bitmap", "zero", "runs", "table", "random", "token", "object")
SIZES = (3073, 4095, 4097, 8191, 8193, 16384, 45056, 45057, 65536, 90113, 135169, 200001, 524288, 1048576)


def run_plan(zsc_amd, torch, bufs, level, schedule):
    """One batch through a DeflatePlan, which must have chosen `schedule`; returns the streams."""
    plan = zsc_amd.DeflatePlan([len(b) for b in bufs], level=level)
    try:
        assert plan.seg_schedule == schedule
        host = torch.zeros(plan.in_bytes, dtype=torch.uint8)
        for off, b in zip(plan.in_offsets, bufs):
            host[off:off + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8)
        d_in = host.to("cuda")
        d_out = torch.zeros(plan.out_bytes, dtype=torch.uint8, device="cuda")
        plan.run(d_in.data_ptr(), d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        lens, stats = plan.results()
        assert all(s == 0 for s in stats), [(i, s) for i, s in enumerate(stats) if s]
        out = d_out.cpu()
        return [bytes(out[o:o + n].numpy()) for o, n in zip(plan.out_offsets, lens)]
    finally:
        plan.close()


def test_pipeline_and_super_steps_give_the_oracle_streams(oracle):
    import torch
    import zsc_amd
    assert zsc_amd.lib.zsc_hip_init(-1) == 0, "no usable gfx950 device: " + zsc_amd.device_info()
    bufs = []
    for n in SIZES:
        for kind in KINDS:
            if n > 200001 and kind not in ("text", "bitmap", "table", "random", "zero"):
                continue
            bufs.append(corpus.make_buffer(kind, n, n + 29))
    keep = os.environ.get("ZSC_HIP_SEG_PIPE")
    try:
        for level in (6, 4, 9):
            want = [oracle.compress(b, level)[1] for b in bufs]
            got = {}
            for pipe in ("1", "0"):
                os.environ["ZSC_HIP_SEG_PIPE"] = pipe  # read by plan creation
                got[pipe] = run_plan(zsc_amd, torch, bufs, level, "pipeline" if pipe == "1" else "super-steps")
            os.environ.pop("ZSC_HIP_SEG_PIPE", None)
            default = run_plan(zsc_amd, torch, bufs, level, "pipeline")
            for i, b in enumerate(bufs):
                assert got["1"][i] == want[i], ("pipeline", level, i, len(b))
                assert got["0"][i] == want[i], ("super-steps", level, i, len(b))
                assert default[i] == got["1"][i] == got["0"][i], (level, i, len(b))
    finally:
        os.environ.pop("ZSC_HIP_SEG_PIPE", None)
        if keep is not None:
            os.environ["ZSC_HIP_SEG_PIPE"] = keep
