"""The members inflate path (zsc_amd/csrc/inflate_members.h) on the lane emulation, against the oracle walk.

tests/emu_members builds the path's kernel sources with -DZSC_WAVE_EMU into a stand-alone program at 64, 16
(the decoder's group width on the GPU) and 8 lanes; it runs scan -> setup -> scan -> claims -> count ->
resolve -> write -> finish -> serial, as the runtime enqueues them.

The reference is the walk of the contract (include/zsc_hip.h) built from oracle.uncompress(file[at:],
cap - out, window_bits=31): every case must give its (status, bytes, consumed, members).  Every case also
states the verified prefix it expects (the members the parallel path decoded); for the clean files and the
clean BGZF files that is the number of members they were built from, exactly.  In size-only mode the walk is
built from the size contract (expect() of tests/test_inflate_size_emu.py: a member whose only fault is its
CRC-32 is Z_OK and the walk goes on); there only the clean files' prefix is stated, because claims are not
used and a wrong CRC-32 is not seen.

Two things the case list cannot hold.  A member start at offsets 15, 16 or 17: the shortest gzip member has
20 bytes (10 of header, 2 of deflate data, 8 of trailer), so no member but the first starts before offset 20.
The lane edges are taken at 32 and 48 instead (starts at 30-33 and 46-49), and the pattern itself is placed
at 14-17 inside an FNAME, where it is a false candidate.  And FDICT / Z_NEED_DICT: a gzip header has no such
flag, so that status does not arise in a members plan and no case fakes it.

make_member_cases() is shared with tests/test_gpu_inflate_members.py.
"""
import collections
import os
import struct
import subprocess
import zlib

import pytest

from zsc_amd import corpus

HERE = os.path.dirname(os.path.abspath(__file__))
LANES = (64, 16, 8)
GZ = 31
Z_OK, Z_DATA_ERROR, Z_BUF_ERROR = 0, -3, -5
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
SIZE_ONLY, CLAIMS_OFF = 1, 2
DEFAULT = 0xFFFFFFFF

# kind: "clean" / "bgzf" (built sound: prefix == members == built, no exceptions) or "other"
Case = collections.namedtuple("Case", "name data cap kind built prefix claimed")


def gz(oracle, data, level=6, **kw):
    rc, comp, _ = oracle.compress(data, level, window_bits=GZ, **kw)
    assert rc == 0
    return comp


def raw(oracle, data, level=6):
    rc, comp, _ = oracle.compress(data, level, window_bits=-15)
    assert rc == 0
    return comp


def gz_by_hand(oracle, data, level=6, extra=None, name=None, comment=None, hcrc=False):
    """a gzip member with the header fields given (name and comment without their NUL)"""
    flg = (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | \
          (2 if hcrc else 0)
    h = b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\0\xff"
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\0"
    if comment is not None:
        h += comment + b"\0"
    if hcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xffff)
    return h + raw(oracle, data, level) + struct.pack("<II", zlib.crc32(data), len(data))


def bgzf(oracle, data, level=6, before=b"", slen=2, bsize_delta=0, isize_delta=0):
    """a BGZF member: FEXTRA with the `BC` subfield (behind `before`), BSIZE = its length - 1"""
    body = raw(oracle, data, level)
    sub = b"BC" + struct.pack("<H", slen) + b"\0" * slen
    extra = before + sub
    total = 12 + len(extra) + len(body) + 8
    sub = b"BC" + struct.pack("<H", slen) + struct.pack("<H", total - 1 + bsize_delta) + b"\0" * (slen - 2)
    extra = before + sub
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", len(extra)) + extra + body +
            struct.pack("<II", zlib.crc32(data), len(data) + isize_delta))


def set_bsize(member, bsize):
    """a BGZF member made by bgzf() with no `before`, its BSIZE replaced"""
    assert member[12:16] == b"BC\x02\x00"
    return member[:16] + struct.pack("<H", bsize) + member[18:]


def walk(oracle, data, cap, size_only=False):
    """the contract's walk: (status, output bytes or their count, consumed, members)"""
    if size_only:
        from test_inflate_size_emu import expect
    at = out_len = members = 0
    outs = []
    while True:
        if size_only:
            (rc, n, used), _ = expect(oracle, data[at:], cap - out_len, GZ)
        else:
            rc, o, used = oracle.uncompress(data[at:], cap - out_len, window_bits=GZ)
            outs.append(o)
            n = len(o)
        out_len += n
        at += used
        if rc != Z_OK:
            break
        members += 1
        if len(data) - at < 2 or data[at:at + 2] != b"\x1f\x8b":
            break
    return rc, (out_len if size_only else b"".join(outs)), at, members


_cases_memo = {}


def make_member_cases(oracle):
    """[Case]; built once per oracle and not changed by anyone"""
    if id(oracle) in _cases_memo:
        return _cases_memo[id(oracle)]
    cases = []
    kinds = ("text", "table", "token", "bitmap", "object")

    def buf(n, seed):
        return corpus.make_buffer(kinds[seed % len(kinds)], n, 900 + seed)

    def clean(name, members, datas, kind="clean", claimed=0):
        f = b"".join(members)
        cases.append(Case(name, f, sum(len(d) for d in datas), kind, len(members), len(members), claimed))

    # ---- clean files of 1, 2, 5 and 300 members: outputs of 0, 1, 300, ~5 KB and over 64 KiB; levels 0, 1, 6, 9
    sizes = [0, 1, 300, 5000, 70000]
    for level in (0, 1, 6, 9):
        for count in (1, 2, 5):
            datas = [buf(sizes[(j + count + level) % 5], 10 * level + j) for j in range(count)]
            clean(f"clean-{count}-l{level}", [gz(oracle, d, level) for d in datas], datas)
    for j, n in enumerate(sizes):
        d = buf(n, 70 + j)
        clean(f"clean-single-{n}", [gz(oracle, d, 6)], [d])
    datas = [buf((37 * j) % 700, j) for j in range(300)]
    clean("clean-300", [gz(oracle, d, (0, 1, 6, 9)[j % 4]) for j, d in enumerate(datas)], datas)
    empty = gz(oracle, b"", 6)
    assert len(empty) == 20
    clean("clean-300-empty", [empty] * 300, [b""] * 300)
    # a full-flushed member (the reference's max_block_len) between plain ones
    d3 = [buf(3000, 1), buf(9000, 2), buf(200, 3)]
    clean("clean-flushed-middle", [gz(oracle, d3[0]), gz(oracle, d3[1], 6, max_block_len=2048), gz(oracle, d3[2])], d3)

    # ---- scan edges: member 1 starts at `at`, placed by the length of member 0's FNAME
    a, b = buf(40, 5), buf(500, 6)
    for at in (30, 31, 32, 33, 46, 47, 48, 49, 254, 255, 256, 257, 1022, 1023, 1024, 1025, 4093, 4094, 4095, 4096, 4097):
        a0 = b"" if at < 100 else a  # (an empty member 0 leaves room for a name in front of offset 30)
        m0 = gz_by_hand(oracle, a0, 6, name=b"n" * (at - len(gz_by_hand(oracle, a0, 6, name=b""))))
        assert len(m0) == at
        clean(f"edge-{at}", [m0, gz(oracle, b, 6)], [a0, b])
    # the pattern at 14-17 (inside an FNAME): a false candidate at a lane edge
    for at in (14, 15, 16, 17):
        name = b"n" * (at - 10) + b"\x1f\x8b\x08" + b"n" * 20
        clean(f"edge-false-{at}", [gz_by_hand(oracle, a, 6, name=name), gz(oracle, b, 6)], [a, b])

    # ---- false candidates
    inner = gz(oracle, buf(2000, 7), 6) + gz(oracle, buf(1500, 8), 9)
    clean("gzip-in-stored-gzip", [gz(oracle, inner, 0)], [inner])
    clean("gzip-in-stored-gzip-then-one", [gz(oracle, inner, 0), gz(oracle, a, 6)], [inner, a])
    sprinkled = bytearray(buf(30000, 9))
    for p in range(50, len(sprinkled) - 8, 97):
        sprinkled[p:p + 4] = b"\x1f\x8b\x08\x00"
    sprinkled = bytes(sprinkled)
    clean("magic-every-97-stored", [gz(oracle, sprinkled, 0), gz(oracle, a, 6)], [sprinkled, a])
    clean("magic-every-97-deflated", [gz(oracle, sprinkled, 6), gz(oracle, a, 6)], [sprinkled, a])
    magic = b"\x1f\x8b\x08\x00"
    # stored data that is nothing but the pattern: more candidates than a file may have, so it goes serial
    dense = magic * 3000
    cases.append(Case("magic-dense-overflows", gz(oracle, dense, 0) + gz(oracle, a, 6), len(dense) + len(a), "other",
                      None, 0, 0))
    fields = gz_by_hand(oracle, b, 6, extra=b"AB" + struct.pack("<H", 8) + magic * 2, name=b"x" + magic[:3] + b"y",
                        comment=magic[:3] * 3)
    clean("magic-in-header-fields", [fields, gz(oracle, a, 6)], [b, a])
    fh = gz_by_hand(oracle, b, 6, extra=b"AB" + struct.pack("<H", 4) + magic, name=b"file", hcrc=True)
    clean("magic-in-fextra-fhcrc", [gz(oracle, a, 1), fh, fh], [a, b, b])

    # ---- ends
    d5 = [buf(n, 20 + j) for j, n in enumerate((123, 81, 0, 384, 2000))]
    m5 = [gz(oracle, d, 6) for d in d5]
    f5, n5 = b"".join(m5), sum(len(d) for d in d5)
    for pad in (1, 7, 4096):
        cases.append(Case(f"zero-pad-{pad}", f5 + b"\0" * pad, n5, "clean", 5, 5, 0))
    cases.append(Case("junk-after", f5 + b"junk \x8b\x1f junk", n5, "clean", 5, 5, 0))
    cases.append(Case("trailing-1f", f5 + b"\x1f", n5, "clean", 5, 5, 0))
    # (the chain ends at a link to nowhere: the serial step meets the truncated / bad header)
    cases.append(Case("magic-then-truncated", f5 + b"\x1f\x8b", n5, "other", None, 5, 0))
    cases.append(Case("bad-method-after", f5 + b"\x1f\x8b\x07\x00 junk", n5, "other", None, 5, 0))
    for cut in (1, 4, 8):
        cases.append(Case(f"trailer-cut-{cut}", f5[:-cut], n5, "other", None, 4, 0))
    cases.append(Case("empty-input", b"", 100, "other", None, 0, 0))

    # ---- caps
    s5 = [len(d) for d in d5]
    cases.append(Case("cap-plus-100", f5, n5 + 100, "clean", 5, 5, 0))
    cases.append(Case("cap-one-short", f5, n5 - 1, "other", None, 4, 0))
    inside = s5[0] + s5[1] // 2  # ends inside member 2 of 5
    cases.append(Case("cap-inside-member-2", f5, inside, "other", None, 1, 0))
    cases.append(Case("cap-0", f5, 0, "other", None, 0, 0))
    cases.append(Case("cap-0-empty-members", empty * 3, 0, "clean", 3, 3, 0))

    # ---- damage: member 3 of 6 (the prefix is the 2 before it)
    d6 = [buf(n, 30 + j) for j, n in enumerate((700, 1, 4000, 300, 0, 900))]
    m6 = [gz(oracle, d, 6) for d in d6]
    n6 = sum(len(d) for d in d6)
    start3 = len(m6[0]) + len(m6[1])

    def flipped(pos):
        f = bytearray(b"".join(m6))
        f[pos] ^= 0x40
        return bytes(f)

    cases.append(Case("flip-body", flipped(start3 + len(m6[2]) // 2), n6, "other", None, 2, 0))
    cases.append(Case("flip-crc", flipped(start3 + len(m6[2]) - 7), n6, "other", None, 2, 0))
    cases.append(Case("flip-isize", flipped(start3 + len(m6[2]) - 3), n6, "other", None, 2, 0))
    cases.append(Case("flip-member-0", flipped(14), n6, "other", None, 0, 0))
    # a damaged member with full-flush markers and members behind it: the resynchronisation runs on into them
    big = buf(30000, 40)
    fl = bytearray(gz(oracle, big, 6, max_block_len=2048))
    assert fl.count(b"\x00\x00\xff\xff") >= 4, fl.count(b"\x00\x00\xff\xff")
    for j in range(300, 306):
        fl[j] ^= 0x5a
    cases.append(Case("damaged-flushed-then-more", m6[0] + bytes(fl) + m6[2] + m6[3], n6 + len(big), "other", None, 1, 0))

    # ---- claims: clean BGZF files of 1, 3 and 40 members and the EOF member
    for count in (1, 3, 40):
        datas = [buf(1 + (977 * j) % 9000, 50 + j) for j in range(count)]
        if count == 3:
            datas[1] = buf(65536, 49)  # the largest output a claim may have
        ms = [bgzf(oracle, d, (1, 6, 9)[j % 3]) for j, d in enumerate(datas)] + [BGZF_EOF]
        clean(f"bgzf-{count}", ms, datas + [b""], "bgzf", count + 1)
    c4 = [buf(n, 60 + j) for j, n in enumerate((100, 200, 150, 120))]
    g4 = [bgzf(oracle, d) for d in c4]
    n4 = sum(len(d) for d in c4)
    other = b"XY" + struct.pack("<H", 3) + b"abc"
    clean("bgzf-bc-behind-another", [g4[0], bgzf(oracle, c4[1], before=other), g4[2]], c4[:3], "bgzf", 3)
    # not claimed, decoded like any member: SLEN other than 2, an ISIZE above 64 KiB, a BSIZE past the file
    clean("bgzf-slen-4-ignored", [g4[0], bgzf(oracle, c4[1], slen=4), g4[2]], c4[:3], "clean", 2)
    d65537 = buf(65537, 48)
    clean("bgzf-isize-65537", [g4[0], bgzf(oracle, d65537), g4[2]], [c4[0], d65537, c4[2]], "clean", 2)
    past = set_bsize(g4[3], len(g4[3]) + 5)
    cases.append(Case("lie-bsize-past-file", g4[0] + g4[1] + g4[2] + past, n4, "clean", 4, 4, 3))
    # lying claims that are taken: the verified prefix ends before the liar (member 2 of 4, or the last)
    # BSIZE one too small: the ISIZE read one byte early is (crc >> 24) | 200 << 8, below 64 KiB
    small = set_bsize(g4[1], len(g4[1]) - 2)
    cases.append(Case("lie-bsize-small", g4[0] + small + g4[2] + g4[3], n4, "other", None, 1, None))
    # BSIZE one too large, on the last member with a zero byte behind it: the ISIZE read is 120 >> 8
    large = set_bsize(g4[3], len(g4[3]))
    cases.append(Case("lie-bsize-large", g4[0] + g4[1] + g4[2] + large + b"\0", n4, "other", None, 3, None))
    # BSIZE spanning two members, the ISIZE at the claimed end set to the sum of the two
    span = set_bsize(g4[1], len(g4[1]) + len(g4[2]) - 1)
    sum2 = g4[2][:-4] + struct.pack("<I", len(c4[1]) + len(c4[2]))
    cases.append(Case("lie-bsize-spans-two", g4[0] + span + sum2 + g4[3], n4, "other", None, 1, None))
    cases.append(Case("lie-isize-plus-1", g4[0] + bgzf(oracle, c4[1], isize_delta=1) + g4[2] + g4[3], n4 + 1,
                      "other", None, 1, None))
    cases.append(Case("lie-isize-minus-1", g4[0] + bgzf(oracle, c4[1], isize_delta=-1) + g4[2] + g4[3], n4,
                      "other", None, 1, None))
    _cases_memo[id(oracle)] = cases
    return cases


def run_emu(tmp_path, lanes, jobs):
    """jobs: [(file, cap, flags, pool, work_mul, work_add)] -> [(status, bytes or None, consumed, members,
    prefix, claimed, canary)]"""
    cpath = os.path.join(str(tmp_path), f"cases{lanes}.bin")
    opath = os.path.join(str(tmp_path), f"out{lanes}.bin")
    with open(cpath, "wb") as f:
        for s, cap, flags, pool, wm, wa in jobs:
            f.write(struct.pack("<iIIIIII", GZ, cap, flags, pool, wm, wa, len(s)) + s)
    r = subprocess.run([os.path.join(HERE, "emu_members", f"emu_members{lanes}"), cpath, opath], check=True,
                       stdout=subprocess.PIPE)
    lines = r.stdout.decode().split("\n")[:-1]
    assert len(lines) == len(jobs)
    blob = open(opath, "rb").read()
    res, at = [], 0
    for line, job in zip(lines, jobs):
        st, ol, used, members, prefix, claimed, canary = (int(x) for x in line.split())
        out = None
        if not job[2] & SIZE_ONLY:
            out = blob[at:at + min(ol, job[1])]
            at += len(out)
        res.append((st, ol, out, used, members, prefix, claimed, canary))
    assert at == len(blob)
    return res


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu_members")], check=True)


@pytest.fixture(scope="module")
def walks(oracle):
    """the reference side: the oracle walk of every case, once"""
    return {c.name: walk(oracle, c.data, c.cap) for c in make_member_cases(oracle)}


def test_the_case_set_is_what_its_names_say(oracle, walks):
    """the reference side alone: every case gives the outcome its name says, before any kernel is asked"""
    cases = make_member_cases(oracle)
    assert len({c.name for c in cases}) == len(cases)
    sound = [c for c in cases if c.kind in ("clean", "bgzf")]
    assert len(sound) >= 40
    for c in sound:
        rc, out, used, members = walks[c.name]
        assert (rc, members) == (Z_OK, c.built), c.name
        assert c.prefix == c.built, c.name
        assert len(out) <= c.cap
        if used == len(c.data):
            import gzip
            assert gzip.decompress(c.data) == out, c.name
    w = {c.name: walks[c.name] for c in cases}
    by = {c.name: c for c in cases}
    for pad in (1, 7, 4096):
        assert w[f"zero-pad-{pad}"][2] == len(by[f"zero-pad-{pad}"].data) - pad
    assert w["junk-after"][0] == Z_OK and w["trailing-1f"][0] == Z_OK
    assert w["magic-then-truncated"][0::3] == (Z_BUF_ERROR, 5)
    assert w["bad-method-after"][0::3] == (Z_DATA_ERROR, 5)
    for cut in (1, 4, 8):
        assert w[f"trailer-cut-{cut}"][0::3] == (Z_BUF_ERROR, 4)
    assert w["empty-input"] == (Z_BUF_ERROR, b"", 0, 0)
    assert w["cap-one-short"][0::3] == (Z_BUF_ERROR, 4) and len(w["cap-one-short"][1]) == by["cap-one-short"].cap
    assert w["cap-inside-member-2"][0::3] == (Z_BUF_ERROR, 1)
    assert w["cap-0"][0::3] == (Z_BUF_ERROR, 0)
    for name in ("flip-body", "flip-crc", "flip-isize"):
        assert w[name][0::3] == (Z_DATA_ERROR, 2), name
    assert w["flip-member-0"][0::3] == (Z_DATA_ERROR, 0)
    # the resynchronisation salvaged output beyond the damaged member's start and ran to the file's end
    rc, out, used, members = w["damaged-flushed-then-more"]
    assert (rc, members, used) == (Z_DATA_ERROR, 1, len(by["damaged-flushed-then-more"].data)) and len(out) > 700 + 2048
    assert w["gzip-in-stored-gzip"][3] == 1
    assert w["magic-dense-overflows"][0::3] == (Z_OK, 2)
    assert w["lie-bsize-past-file"][0::3] == (Z_OK, 4)
    assert w["lie-bsize-small"][0::3] == (Z_OK, 4)
    assert w["lie-bsize-large"][0::3] == (Z_OK, 4)
    assert w["lie-bsize-spans-two"][0::3] == (Z_DATA_ERROR, 2)
    assert w["lie-isize-plus-1"][0::3] == (Z_DATA_ERROR, 1)
    assert w["lie-isize-minus-1"][0::3] == (Z_DATA_ERROR, 1)


def check_case(c, want, got, claims=True):
    """one result against the walk and the case's stated prefix"""
    st, ol, out, used, members, prefix, claimed, canary = got
    rc, wout, wused, wmembers = want
    assert (st, ol, used, members) == (rc, len(wout), wused, wmembers), (c.name, got[:2], got[3:])
    assert out == wout, c.name
    assert canary == 1, c.name
    assert prefix == c.prefix, (c.name, prefix, c.prefix)
    if not claims:
        assert claimed == 0, c.name
    elif c.claimed is not None:
        assert claimed == c.claimed, (c.name, claimed)
    else:
        assert claimed <= prefix, c.name


@pytest.mark.parametrize("lanes", LANES)
def test_members_equal_the_oracle_walk(built, oracle, walks, tmp_path, lanes):
    cases = make_member_cases(oracle)
    res = run_emu(tmp_path, lanes, [(c.data, c.cap, 0, 0, DEFAULT, DEFAULT) for c in cases])
    for c, got in zip(cases, res):
        check_case(c, walks[c.name], got)


@pytest.mark.parametrize("lanes", LANES)
def test_claims_switched_off_give_the_same_results(built, oracle, walks, tmp_path, lanes):
    """without claims the count pass decodes every member, liars included: a lying header is then just a header"""
    cases = [c for c in make_member_cases(oracle) if c.kind == "bgzf" or c.name.startswith(("lie-", "bgzf-"))]
    assert len(cases) >= 12
    res = run_emu(tmp_path, lanes, [(c.data, c.cap, CLAIMS_OFF, 0, DEFAULT, DEFAULT) for c in cases])
    for c, got in zip(cases, res):
        want = walks[c.name]
        # (unclaimed, a liar is counted by decoding it: the prefix runs to the first member that is not Z_OK)
        check_case(c._replace(prefix=want[3]), want, got, claims=False)


@pytest.mark.parametrize("lanes", LANES)
def test_size_only_equals_the_size_walk(built, oracle, tmp_path, lanes):
    cases = make_member_cases(oracle)
    res = run_emu(tmp_path, lanes, [(c.data, c.cap, SIZE_ONLY, 0, DEFAULT, DEFAULT) for c in cases])
    crc_only = 0
    for c, got in zip(cases, res):
        st, ol, out, used, members, prefix, claimed, canary = got
        want = walk(oracle, c.data, c.cap, size_only=True)
        assert (st, ol, used, members) == want, (c.name, got, want)
        assert claimed == 0 and canary == 1
        if c.kind in ("clean", "bgzf"):
            assert prefix == members == c.built, c.name
        crc_only += c.name == "flip-crc" and want[0] == Z_OK and want[3] == 6
    assert crc_only == 1  # the one exception of the size contract took effect where it should


@pytest.mark.parametrize("lanes", LANES)
def test_no_limit_in_size_only_mode(built, oracle, tmp_path, lanes):
    cases = [c for c in make_member_cases(oracle) if c.name in ("clean-5-l6", "bgzf-40", "flip-body", "cap-0")]
    res = run_emu(tmp_path, lanes, [(c.data, DEFAULT, SIZE_ONLY, 0, DEFAULT, DEFAULT) for c in cases])
    for c, got in zip(cases, res):
        want = walk(oracle, c.data, 1 << 20, size_only=True)  # (a limit the output does not reach is no limit)
        assert want[1] < 1 << 20
        assert (got[0], got[1], got[3], got[4]) == want, c.name


@pytest.mark.parametrize("lanes", LANES)
def test_pool_and_work_bound_send_the_file_serial(built, oracle, walks, tmp_path, lanes):
    by = {c.name: c for c in make_member_cases(oracle)}
    five, forty = by["clean-5-l6"], by["bgzf-40"]
    jobs = [(five.data, five.cap, 0, 5, DEFAULT, DEFAULT),   # the file needs 5 slots
            (five.data, five.cap, 0, 4, DEFAULT, DEFAULT),   # one short
            (five.data, five.cap, 0, 0, 0, 64),              # the work bound passed after the first member
            (five.data, five.cap, SIZE_ONLY, 4, DEFAULT, DEFAULT),
            (five.data, five.cap, SIZE_ONLY, 0, 0, 64),
            (forty.data, forty.cap, 0, 40, DEFAULT, DEFAULT),
            (forty.data, forty.cap, 0, 0, 0, 64)]            # claimed members cost the count pass nothing
    res = run_emu(tmp_path, lanes, jobs)
    for (data, cap, flags, *_), got, prefix in zip(jobs, res, (5, 0, 0, 0, 0, 0, 41)):
        c = five if data is five.data else forty
        if flags & SIZE_ONLY:
            assert (got[0], got[1], got[3], got[4]) == walk(oracle, data, cap, size_only=True)
            assert got[5] == prefix
        else:
            check_case(c._replace(prefix=prefix, claimed=None), walks[c.name], got)
