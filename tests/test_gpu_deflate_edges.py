"""The deflate block coder on inputs built to reach its edge paths (tests/deflate_cases.py), on a real MI355X,
through the C ABI of libzsc_hip.so.

One batch per parameter set holds all of that set's cases between ordinary corpus buffers.  Every stream must
be the oracle's and the compiled reference's (tests/golden/deflate_edges_golden.json), the same wherever the
case sits in the batch (the batch runs again in reverse order: state left in LDS by the block before would
show), inflate back to the input, and pass the device-side verification, whose decoder reads 15-bit codes
after a repair and 10-bit blocks here as the packer writes them.  tests/test_deflate_edges_emu.py proves on the
CPU that each case reaches the path it was built for.
"""
import pytest

import deflate_cases as D

pytestmark = pytest.mark.gpu

VERIFY_OK = 0


@pytest.fixture(scope="module")
def z():
    import zsc_amd
    assert zsc_amd.lib.zsc_hip_init(-1) == 0, "no usable gfx950 device: " + zsc_amd.device_info()
    return zsc_amd


@pytest.fixture(scope="module")
def groups():
    """{(level, window_bits, mem_level, strategy): cases}"""
    out = {}
    for c in D.cases():
        out.setdefault(c.params, []).append(c)
    assert 12 <= len(out) <= 20
    return out


@pytest.fixture(scope="module")
def wanted(oracle, groups):
    """{case name: (rc, the oracle's stream)}, and the same for the corpus buffers that pad a batch"""
    want = {}
    for params, cases in groups.items():
        level, wbits, ml, strat = params
        for name, data in [(c.name, c.data) for c in cases] + list(padding(params)):
            rc, s, _ = oracle.compress(data, level, window_bits=wbits, mem_level=ml, strategy=strat, work_len=1 << 20)
            want[(params, name)] = (rc, s)
    return want


_PAD = {}


def padding(params):
    """ordinary buffers that go around and between the cases: short text, a table of several blocks, zeros"""
    if not _PAD:
        from zsc_amd import corpus
        _PAD["pad"] = [("pad-text", corpus.make_buffer("text", 3000, 41)),
                       ("pad-table", corpus.make_buffer("table", 40000, 42)),
                       ("pad-zero", corpus.make_buffer("zero", 700, 43)),
                       ("pad-object", corpus.make_buffer("object", 9000, 44))]
    return _PAD["pad"]


def batch_of(params, cases):
    """[(name, data)]: a corpus buffer in front, one after every fourth case, and one at the end"""
    pad = padding(params)
    out = [pad[0]]
    for k, c in enumerate(cases):
        out.append((c.name, c.data))
        if k % 4 == 3:
            out.append(pad[(k // 4) % len(pad)])
    out.append(pad[1])
    return out


def test_streams_equal_oracle_and_golden_wherever_they_sit(z, groups, wanted):
    results = {}
    for params, cases in groups.items():
        level, wbits, ml, strat = params
        batch = batch_of(params, cases)
        rc, outs, stats = z.compress_batch([d for _, d in batch], level=level, window_bits=wbits, mem_level=ml,
                                           strategy=strat)
        assert rc == 0 and len(outs) == len(batch), params
        for (name, data), out, st in zip(batch, outs, stats):
            assert (st, out) == wanted[(params, name)], (params, name, st, len(out))
        back = batch[::-1]
        rc, outs2, stats2 = z.compress_batch([d for _, d in back], level=level, window_bits=wbits, mem_level=ml,
                                             strategy=strat)
        assert rc == 0 and outs2[::-1] == outs and stats2[::-1] == stats, params
        for (name, _), out, st in zip(batch, outs, stats):
            if not name.startswith("pad-"):
                results[name] = (st, out)
    D.check_against_golden(D.load_golden(), D.cases(), results, "compress_batch")


def test_streams_inflate_back_and_verify_on_the_device(z, groups, wanted):
    for params, cases in groups.items():
        level, wbits, ml, strat = params
        batch = batch_of(params, cases)
        datas = [d for _, d in batch]
        rc, streams, stats, verdicts = z.compress_batch_verified(datas, level=level, window_bits=wbits, mem_level=ml,
                                                                 strategy=strat)
        assert rc == 0 and stats == [0] * len(batch), params
        for (name, _), s, v in zip(batch, streams, verdicts):
            assert s == wanted[(params, name)][1], (params, name)
            assert v["verdict"] == VERIFY_OK, (params, name, v)
        rc, outs, used, stat = z.uncompress_batch(streams, [len(d) for d in datas], window_bits=wbits)
        assert rc == 0 and stat == [0] * len(batch), params
        assert used == [len(s) for s in streams], params
        for (name, data), out in zip(batch, outs):
            assert out == data, (params, name)
