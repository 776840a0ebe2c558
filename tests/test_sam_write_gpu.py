"""SAM output on the GPU (row f8): dq_sam_write* against the plain-Python oracle
tests/samwriteutil.py -- lines byte for byte, the first error by record index and class -- over
record sizes that cross every seam of the kernels, then the round trips with the SAM reader and
the storage layer."""
import os
import re
import struct

import numpy as np
import pytest

from disq_amd import _lib
from disq_amd import parallel as P
from disq_amd.storage import HtsjdkReadsRddStorage
import bamutil as B
import samcases as K
import samutil as S
import samwriteutil as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = W.bam_header()
CORE = open(os.path.join(ROOT, "disq_amd", "csrc", "dq_samw_core.h")).read()
TILE = int(re.search(r"SAMW_TILE = (\d+);", CORE).group(1))
RUN = int(re.search(r"SAMW_RUN = (\d+);", CORE).group(1))
LONG = int(re.search(r"SAMW_LONG = (\d+);", CORE).group(1))


def offsets(recs):
    return np.cumsum([0] + [len(r) for r in recs[:-1]], dtype=np.int64) if recs else np.zeros(0, np.int64)


def check(recs, header=HDR, ctx=None):
    """dq_sam_write of the records, with raw_offset given and with NULL, equals the oracle: the
    text, or the first failing record and its class."""
    want, err = W.records_to_sam_text(recs, W.header_ref_names(header))
    raw = b"".join(recs)
    c = ctx or _lib.Context()
    try:
        for off in (offsets(recs), None):
            if err is None:
                assert c.sam_write(header, raw, off) == want
            else:
                with pytest.raises(_lib.DqError) as e:
                    c.sam_write(header, raw, off)
                assert e.value.code == _lib.DQ_EFORMAT and str(e.value).endswith("] " + err), (str(e.value), err)
    finally:
        if ctx is None:
            c.close()
    return want


@pytest.fixture(scope="module")
def bam1(golden):
    """1.bam read whole: header, raw bytes, offsets, hashes, and the oracle's text of its records
    (computed once)."""
    data = open(os.path.join(golden, "1.bam"), "rb").read()
    with _lib.Context() as c:
        c.open_bytes(data)
        _, hdr = c.header()
        b = c.read(with_raw=True)
    raw = bytes(b["raw"])
    text, err = W.records_to_sam_text(W.split_records(raw), W.header_ref_names(hdr))
    assert err is None and text.count(b"\n") == 4917
    return {"data": data, "hdr": hdr, "raw": raw, "off": b["raw_offset"].copy(), "hash": b["hash"].copy(),
            "text": text}


def test_rule_records():
    text = K.HEADER + b"".join(l + b"\n" for l in K.good_lines())
    hdr, names = S.sam_header_to_bam(text)
    recs = [r for _, _, r in S.sam_records(text, names)]
    assert len(recs) == 76
    check(recs, hdr)
    check(W.trim_cases())


def test_1bam_host_input(bam1):
    with _lib.Context() as c:
        assert c.sam_write(bam1["hdr"], bam1["raw"], bam1["off"]) == bam1["text"]
        assert c.sam_write(bam1["hdr"], bam1["raw"], None) == bam1["text"]


def test_error_cases():
    good = W.make_record()
    with _lib.Context() as c:
        for rec, what in W.error_cases():
            want, err = W.records_to_sam_text([good, good, good, rec, good], W.REFS)
            assert err == "record 3: " + what
            check([good, good, good, rec, good], ctx=c)
        bad = [r for r, _ in W.error_cases()]
        check([good] * 70 + [bad[20]] + [good] * 70 + [bad[12]], ctx=c)   # two records: the first
        check([bad[15], bad[4]], ctx=c)
        # a chain that does not end at raw_len, or breaks
        for raw, n, msg in ((good + good[:-1], 2, "record 1: fields"), (good + b"\0", 2, "record 1: fields"),
                            (good + good, 1, "record 1: fields"), (good[:20], 1, "record 0: fields")):
            hdr = np.frombuffer(HDR, np.uint8)
            buf = np.frombuffer(raw, np.uint8)
            out, m = _lib.C.c_void_p(), _lib.C.c_int64()
            rc = _lib.lib().dq_sam_write(c._h, hdr.ctypes.data, len(hdr), buf.ctypes.data, len(buf), None, n,
                                         _lib.C.byref(out), _lib.C.byref(m))
            assert rc == _lib.DQ_EFORMAT and _lib.lib().dq_last_error(c._h).decode() == msg
        # an earlier malformed record outranks the broken chain
        with pytest.raises(_lib.DqError, match="record 0: QUAL"):
            c.sam_write(HDR, bad[12] + good[:-1], None)


def sized_record(total, l_seq=1000, tags=b"", **kw):
    """A record of exactly `total` bytes (block_size word included), padded by a Z tag."""
    seq = bytes((17 * i) & 0xff or 0x11 for i in range((l_seq + 1) // 2))
    kw.setdefault("qual", bytes((i * 7) % 94 for i in range(l_seq)))

    def mk(pad):
        return W.make_record(seq=seq, l_seq=l_seq, cigar=(l_seq << 4,),
                             tags=b"XZZ" + b"p" * pad + b"\0" + tags, **kw)
    pad = total - len(mk(0))
    assert pad >= 0
    return mk(pad)


def test_thread_wave_threshold():
    assert LONG == 2048
    recs = [sized_record(n) for n in (2047, 2048, 2049, 2050, 2047, 4001)]
    assert [len(r) for r in recs] == [2047, 2048, 2049, 2050, 2047, 4001]
    check(recs)
    check([sized_record(2049, qual=b"\xff" * 1000), sized_record(3000, l_seq=1001, qual=b"\xff" * 1001)])
    # the wave's QUAL check and its rank between the fixed columns and the tags
    bad_q = bytes(94 if i == 777 else 30 for i in range(1000))
    check([sized_record(2049), sized_record(2500, qual=bad_q)])
    check([sized_record(2500, qual=bad_q, tags=b"XQq\x01")])
    check([sized_record(2500, qual=bad_q, nref=9)])
    check([sized_record(2500, tags=b"XQq\x01"), sized_record(2500, qual=bad_q)])
    check([sized_record(2500, qual=b"\xff" * 999 + b"\x05")])


def test_long_read():
    n = 70000
    rng = np.random.default_rng(5)
    seq = rng.integers(0, 256, (n + 1) // 2, dtype=np.uint8).tobytes()
    qual = rng.integers(0, 94, n, dtype=np.uint8).tobytes()
    cigar = tuple(((i % 250) + 1) << 4 | (i % 9) for i in range(300))
    fl = W.float_set(0)[:1000]
    tags = b"NMC\x07XBBf" + struct.pack("<i", len(fl)) + struct.pack("<%dI" % len(fl), *fl) + b"XZZtail  \0"
    rec = W.make_record(qname=b"long/1", seq=seq, l_seq=n, qual=qual, cigar=cigar, tags=tags, ref=2, nref=2)
    text = check([W.make_record(), rec, W.make_record(), rec[:], W.make_record()])
    assert len(text) > 2 * 140000


def line_sized(size):
    """A short record whose line (LF included) is exactly `size` bytes."""
    base = len(W.record_to_sam_line(W.make_record(tags=b"XZZ\0"), W.REFS)) + 1
    assert size >= base
    return W.make_record(tags=b"XZZ" + b"z" * (size - base) + b"\0")


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_lds_tile_boundary(delta):
    """A run of RUN short records whose lines sum to just under, exactly at and just over the LDS
    tile, after a first run that leaves the text at an odd offset, before a short last run."""
    each = TILE // RUN
    sizes = [each] * (RUN - 1)
    sizes.append(TILE + delta - sum(sizes))
    first = [line_sized(50 + (i % 7)) for i in range(RUN)]
    recs = first + [line_sized(s) for s in sizes] + [line_sized(60 + i) for i in range(9)]
    text = check(recs)
    lines = text.split(b"\n")
    assert sum(len(l) + 1 for l in lines[RUN:2 * RUN]) == TILE + delta


def test_zero_and_one_record():
    with _lib.Context() as c:
        assert c.sam_write(HDR, b"", None) == b""
        assert c.sam_write(HDR, b"", np.zeros(0, np.int64)) == b""
    check([W.make_record()])


def _float_tag(name, v):
    return name + b"Bf" + struct.pack("<i", len(v)) + struct.pack("<%dI" % len(v), *v)


def float_array_records(vals, per_record):
    """Unmapped records (what the SAM reader makes of their lines, bin included) with one B:f array
    of per_record values each; a last group of fewer than half as many joins the one before it."""
    groups = [vals[i:i + per_record] for i in range(0, len(vals), per_record)]
    if len(groups) > 1 and 2 * len(groups[-1]) < per_record:
        groups[-2:] = [groups[-2] + groups[-1]]
    return [W.make_record(qname=b"f%d" % i, flag=4, ref=-1, pos=-1, mapq=0, cigar=(), seq=b"", l_seq=0, qual=b"",
                          tags=_float_tag(b"XB", g)) for i, g in enumerate(groups)]


def finite_floats(n_random):
    """float_set(n_random) and the binade edges of both signs, the finite ones."""
    edges = W.binade_edges()
    return [b for b in W.float_set(n_random) + edges + [0x80000000 | b for b in edges] if (b >> 23) & 0xff != 0xff]


def test_floats():
    edges = W.binade_edges()
    edges = edges + [0x80000000 | b for b in edges]
    tag = _float_tag
    check([W.make_record(tags=tag(b"XA", edges[:900]) + tag(b"XB", edges[900:])),
           W.make_record(tags=tag(b"XC", edges[:100])), W.make_record(tags=tag(b"XD", []))])
    singles = (W.float_set(0) + edges)[:2000]
    assert len(singles) == 2000
    check([W.make_record(tags=b"XFf" + struct.pack("<I", b)) for b in singles])
    # at scale, a hundred values a record (a thread per record) and a thousand (a wave per record);
    # the oracle works out each value's text once (samwriteutil.float_text keeps its results)
    vals = finite_floats(20000) + [0x7f800000, 0xff800000, 0x7fc00000]
    assert len(vals) > 24000
    with _lib.Context() as c:
        for per, long in ((100, False), (1000, True)):
            recs = float_array_records(vals, per)
            assert all((len(r) > LONG) == long for r in recs) and len(recs) >= len(vals) // per
            check(recs, ctx=c)


def test_float_round_trip_on_device():
    """Every finite value the writer prints is read back to itself by the SAM reader's own
    conversion: the records and their hashes return unchanged, through the thread and the wave
    path of both."""
    from oracle import oracle as O
    vals = finite_floats(20000)
    assert len(vals) > 24000
    for per in (100, 1000):
        recs = float_array_records(vals, per)
        raw = b"".join(recs)
        with _lib.Context() as c:
            text = c.sam_write(HDR, raw, offsets(recs))
        lines = text.split(b"\n")[:-1]
        assert len(lines) == len(recs) and all((len(l) > 2048) == (per == 1000) for l in lines)
        with _lib.Context() as c:
            c.sam_open_bytes(W.header_text(HDR) + text)
            b = c.sam_read(with_raw=True)
        assert bytes(b["raw"]) == raw
        assert b["hash"].tolist() == [O.record_hash(r) for r in recs]


def test_resident_bam(bam1):
    texts = []
    for split in (0, 131072):
        with _lib.Context(split_size=split) as c:
            c.open_bytes(bam1["data"])
            before = c.read(with_raw=False)["hash"].copy()
            n, ms = c.sam_write_resident()
            texts.append(bytes(c.sam_write_fetch(n)))
            assert ms > 0
            assert np.array_equal(c.read(with_raw=False)["hash"], before)   # reads as before
    assert texts[0] == texts[1] == bam1["text"]


def test_resident_sam_context(bam1):
    full = W.header_text(bam1["hdr"]) + bam1["text"]
    with _lib.Context(split_size=100000) as c:
        c.sam_open_bytes(full)
        n, _ = c.sam_write_resident()
        assert bytes(c.sam_write_fetch(n)) == bam1["text"]
        assert c.sam_run().n_records == 4917


def test_resident_needs_a_whole_record_file(bam1, golden):
    data, split = bam1["data"], 131072
    s = P.shard_plan(len(data), 1, split_size=split)[0]
    with _lib.Context(split_size=split) as c:
        with pytest.raises(_lib.DqError) as e:
            c.sam_write_resident()                      # nothing open
        assert e.value.code == _lib.DQ_EINVAL
        c.open_shard(data[s.lo:], s.lo, len(data), s.p0, s.p1, bam1["hdr"])
        with pytest.raises(_lib.DqError) as e:
            c.sam_write_resident()
        assert e.value.code == _lib.DQ_EINVAL
    with _lib.Context() as c:
        c.text_open_path(os.path.join(golden, "HiSeq.10000.vcf.bgz"))
        with pytest.raises(_lib.DqError) as e:
            c.sam_write_resident()
        assert e.value.code == _lib.DQ_EINVAL


def test_device_round_trip(bam1):
    with _lib.Context() as c:
        text = c.sam_write(bam1["hdr"], bam1["raw"], bam1["off"])
    with _lib.Context() as c:
        c.sam_open_bytes(W.header_text(bam1["hdr"]) + text)
        b = c.sam_read(with_raw=True)
    assert bytes(b["raw"]) == bam1["raw"]
    assert np.array_equal(b["hash"], bam1["hash"])


@pytest.mark.parametrize("split", [0, 131072])
def test_storage_write_sam(tmp_path, golden, bam1, split):
    src = os.path.join(golden, "1.bam")
    st = HtsjdkReadsRddStorage.makeDefault().splitSize(split)
    rdd = st.read(src)
    assert rdd.getReads().getNumPartitions() == (5 if split else 1)
    out = str(tmp_path / "o.sam")
    st.write(rdd, out, str(tmp_path / "parts"))
    assert open(out, "rb").read() == W.header_text(bam1["hdr"]) + bam1["text"]
    assert not os.path.exists(tmp_path / "parts")
    back = st.read(out)
    assert np.array_equal(back.getReads().hashes(), rdd.getReads().hashes())
    with pytest.raises(ValueError):
        st.write(rdd, out, bai=True)
    with pytest.raises(ValueError):
        st.write(rdd, out, sbi=True)
    bam = str(tmp_path / "o.bam")
    st.write(rdd, bam)
    assert B.inflate_all(open(bam, "rb").read()) == B.inflate_all(bam1["data"])
