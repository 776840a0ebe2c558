"""SAM text path on the GPU: dq_sam_* against the plain-Python oracle
tests/samutil.py -- record bytes from sam_line_to_bam_record, partition membership from
plain_text_partitions (Hadoop's rule for an uncompressed split), hashes and digests from
oracle.record_hash / stream_digest -- and against the BAM path reading the same reads."""
import os
import re
import struct

import numpy as np
import pytest

from disq_amd import _lib
from disq_amd.storage import (HtsjdkReadsRddStorage, HtsjdkReadsTraversalParameters, Interval)
from oracle import oracle as O
import bamutil as B
import floatcases as F
import samcases as K
import samutil as S
from floatref import exact_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAM_LONG = int(re.search(r"SAM_LONG = (\d+);", open(os.path.join(ROOT, "disq_amd", "csrc", "dq_sam.hip")).read()).group(1))

FIELDS = ("block_size", "ref_id", "pos", "l_read_name", "mapq", "bin", "n_cigar", "flag", "l_seq",
          "next_ref_id", "next_pos", "tlen")


def oracle_parts(text, splits, memo=None):
    """Per split the [(line offset, record bytes)] of its lines that do not start with '@'.  memo:
    a dict that keeps every line's record for the next call on the same text."""
    names = S.sam_header_to_bam(text)[1]
    memo = {} if memo is None else memo

    def rec(o, v):
        if o not in memo:
            memo[o] = S.sam_line_to_bam_record(v, names)
        return memo[o]
    return [[(o, rec(o, v)) for o, v in part if not v.startswith(b"@")]
            for part in S.plain_text_partitions(text, splits)]


def records_of(b):
    raw, ro, bs = b["raw"], b["raw_offset"], b["block_size"]
    return [bytes(raw[int(ro[i]):int(ro[i]) + 4 + int(bs[i])]) for i in range(len(bs))]


def assert_sam_parity(text, split=0, nio=False, memo=None):
    splits = O.path_splits(len(text), split, nio)
    want = oracle_parts(text, splits, memo)
    with _lib.Context(split_size=split, use_nio=nio) as c:
        c.sam_open_bytes(text)
        _, hdr = c.header()
        st = c.sam_run()
        b = c.sam_read(with_raw=True)
        cnt, dig = c.partition_digests()
    assert hdr == S.sam_header_to_bam(text)[0]
    po = b["part_offset"]
    assert len(po) - 1 == len(want) == st.n_partitions == len(cnt)
    recs = records_of(b)
    for i, part in enumerate(want):
        lo, hi = int(po[i]), int(po[i + 1])
        assert hi - lo == len(part) == int(cnt[i]), (split, i)
        assert recs[lo:hi] == [r for _, r in part], (split, i)
        assert b["voffset"][lo:hi].tolist() == [o for o, _ in part], (split, i)
        d = O.stream_digest([O.record_hash(r) for _, r in part])
        assert int(b["part_digest"][i]) == d == int(dig[i]), (split, i)
    n = sum(len(p) for p in want)
    assert st.n_records == n == len(recs)
    assert st.compressed_bytes == st.decompressed_bytes == len(text) and st.n_blocks == 0
    nat = sum(1 for _, v in S.text_lines(text) if v.startswith(b"@"))
    if not text.startswith(b"\xef\xbb\xbf"):
        assert st.n_filtered == nat
    if n:
        assert b["hash"].tolist() == [O.record_hash(r) for r in recs]
        head = np.frombuffer(b"".join(r[:36] for r in recs), _lib.LEAN_HEAD)
        for k in FIELDS:
            assert np.array_equal(b[k], head[k]), k
    return b, st


def sam_error(text, split=0):
    with _lib.Context(split_size=split) as c:
        c.sam_open_bytes(text)
        with pytest.raises(_lib.DqError) as e:
            c.sam_run()
    assert e.value.code == _lib.DQ_EFORMAT
    return str(e.value)


@pytest.fixture(scope="module")
def bam1(golden):
    data = open(os.path.join(golden, "1.bam"), "rb").read()
    return data, S.bam_to_sam_text(B.inflate_all(data))


def test_test_sam(golden):
    """The smallest case (2 records, 6 lines): header, records, fields, line offsets, hashes."""
    text = open(os.path.join(golden, "test.sam"), "rb").read()
    b, st = assert_sam_parity(text)
    assert st.n_records == 2 and st.n_filtered == 4
    assert b["voffset"].tolist() == [text.index(b"read_28833"), text.index(b"read_28701")]
    assert b["pos"].tolist() == [28832, 28833] and b["flag"].tolist() == [99, 147]


@pytest.mark.parametrize("split", [0, 100000, 65536, 4096])
def test_1bam_as_sam(bam1, split):
    data, text = bam1
    b, st = assert_sam_parity(text, split)
    assert st.n_records == 4917
    if split == 4096:  # lines longer than a split: splits in which no line starts
        sizes = np.diff(b["part_offset"])
        assert (sizes == 0).any() and len(sizes) == len(O.path_splits(len(text), split))
    # the BAM path gives every record the same hash
    with _lib.Context(split_size=split) as c:
        c.open_bytes(data)
        bb = c.read(with_raw=True)
    assert np.array_equal(bb["hash"], b["hash"]) and np.array_equal(bb["raw"], b["raw"])


def _lines24():
    return [K.line(qname=b"r%d" % i, pos=100 + i, seq=b"ACGT" * (1 + i % 5), qual=b"*",
                   cigar=b"%dM" % (4 * (1 + i % 5)), tags=(b"XI:i:%d" % (i * 1000),))
            for i in range(24)]


@pytest.mark.parametrize("nl", ["lf", "crlf", "cr", "mixed"])
@pytest.mark.parametrize("variant", ["plain", "bom", "nofinal", "co"])
def test_terminators(nl, variant):
    seps = {"lf": [b"\n"], "crlf": [b"\r\n"], "cr": [b"\r"], "mixed": [b"\n", b"\r\n", b"\r", b"\r\n"]}[nl]
    lines = _lines24()
    head = [l for l in K.HEADER.split(b"\n") if l]
    if variant == "bom":  # the header rule sees no '@' line behind a BOM: unmapped reads only
        head = []
        lines = [K.line(qname=b"r%d" % i, rname=b"*", pos=0, cigar=b"*", flag=4) for i in range(24)]
    if variant == "co":
        lines[11:11] = [b"@CO\tin the middle"]
    allv = head + lines
    text = b"".join(l + seps[i % len(seps)] for i, l in enumerate(allv))
    if variant == "bom":
        text = b"\xef\xbb\xbf" + text
    if variant == "nofinal":
        text = text[:-len(seps[(len(allv) - 1) % len(seps)])]
    for split in (0, 97):
        b, st = assert_sam_parity(text, split, nio=split > 0)
        assert st.n_records == 24


def test_split_boundaries_at_a_line_start():
    lines = _lines24()
    text = K.HEADER + b"".join(l + (b"\r\n" if i % 2 else b"\n") for i, l in enumerate(lines))
    offs = [o for o, v in S.text_lines(text) if not v.startswith(b"@")]
    s = offs[8]
    assert text[s - 2:s] == b"\r\n"
    # useNio splits are [i * ss, (i + 1) * ss): a boundary at s - 1 (between the CR and its LF),
    # at s and at s + 1
    for ss in (s - 1, s, s + 1):
        assert any(e == ss for _, e in O.path_splits(len(text), ss, True))
        assert_sam_parity(text, ss, nio=True)


def test_long_lines():
    """Lines over the wave threshold between short ones; every tag type on one record."""
    rng = np.random.default_rng(7)
    seq = bytes(rng.choice(np.frombuffer(b"ACGTNacgtn.=MRSVWYHKDB", np.uint8), 5000))
    qual = bytes(rng.integers(33, 127, 5000, dtype=np.uint8))
    tags = (b"NM:i:3", b"XA:A:q", b"XZ:Z:some text", b"XH:H:0AFF", b"XF:f:2.5", b"Xc:B:c,-1,2",
            b"XC:B:C,1,255", b"Xs:B:s,-300,300", b"XS:B:S,0,65535", b"Xi:B:i,-70000,70000",
            b"XI:B:I,0,4294967295", b"Xf:B:f,1.5,7.038531e-26", b"Xn:i:-40000", b"XN:i:3000000000")
    short = _lines24()
    lines = short[:3] + [K.line(qname=b"long1", cigar=b"5000M", seq=seq, qual=qual, tags=tags)] + \
        short[3:5] + [K.line(qname=b"long2", cigar=b"2500M2500S", seq=seq[::-1], qual=b"*", tags=tags[:3]),
                      K.line(qname=b"long3", cigar=b"*", seq=seq[:4999], qual=qual[:4999])] + short[5:]
    text = K.HEADER + b"".join(l + b"\n" for l in lines)
    assert max(len(l) for l in lines) > 10000
    b, st = assert_sam_parity(text)
    assert st.n_records == len(lines) and b["l_seq"].max() == 5000
    assert_sam_parity(text, 4096)
    # errors in a long line's SEQ / QUAL bytes rank before its tags
    bad = K.line(qname=b"long4", cigar=b"5000M", seq=seq[:2500] + b"J" + seq[2501:], qual=qual,
                 tags=(b"XX:i:x",))
    assert "SAM line 8: SEQ" in sam_error(K.HEADER + b"".join(l + b"\n" for l in short[:3] + [bad]))
    bad = K.line(qname=b"long5", cigar=b"5000M", seq=seq, qual=qual[:4000] + b" " + qual[4001:],
                 tags=(b"XX:i:x",))
    assert "SAM line 5: QUAL" in sam_error(K.HEADER + bad + b"\n")
    bad = K.line(qname=b"long6", cigar=b"5000M", seq=seq, qual=qual, tags=(b"XX:i:x",))
    assert "SAM line 5: tag XX" in sam_error(K.HEADER + bad + b"\n")


def test_one_line_per_rule_and_float_fixups():
    hard = b"1.00000017881393421514957253748434595763683319091796875"  # past 19 digits: the host's
    lines = K.good_lines() + [
        K.BASE + b"\tXF:f:1.234567890123456789012345",
        K.BASE + b"\tXF:f:" + hard + b"\tXB:B:f,1.5," + hard + b",-2.5e3,0.1000000000000000055511151231,7"]
    text = K.HEADER + b"".join(l + b"\n" for l in lines)
    b, st = assert_sam_parity(text)
    assert st.n_records == len(lines)
    assert records_of(b)[-1].endswith(struct.pack("<f", 7.0))


def test_errors(bam1):
    cases = K.bad_lines()
    for l, what in cases[::4]:
        assert sam_error(K.HEADER + K.BASE + b"\n" + l + b"\n").endswith("SAM line 6: " + what)
    # two malformed lines: the earlier one is reported
    lines = _lines24()
    lines[9] = K.line(mapq=256)
    lines[4] = K.line(cigar=b"0M")
    assert sam_error(K.HEADER + b"".join(l + b"\n" for l in lines)).endswith("SAM line 9: CIGAR")
    # one malformed line inside 1.bam's text, in a later tile and partition
    _, text = bam1
    tl = S.text_lines(text)
    k = 3000
    o, v = tl[k]
    f = v.split(b"\t")
    f[4] = b"300"
    broken = text[:o] + b"\t".join(f) + text[o + len(v):]
    for split in (0, 65536):
        assert sam_error(broken, split).endswith("SAM line %d: MAPQ" % k)


def test_mode_separation(golden, bam1):
    data, _ = bam1
    text = open(os.path.join(golden, "test.sam"), "rb").read()
    with _lib.Context() as c:
        c.sam_open_bytes(text)
        for call in (c.read, c.run_resident, c.text_run, c.plan):
            with pytest.raises(_lib.DqError) as e:
                call()
            assert e.value.code == _lib.DQ_EINVAL
        assert c.sam_run().n_records == 2  # the context still reads SAM
        c.open_bytes(data)
        for call in (c.sam_read, c.sam_run):
            with pytest.raises(_lib.DqError) as e:
                call()
            assert e.value.code == _lib.DQ_EINVAL
        assert len(c.read(with_raw=False)["pos"]) == 4917  # and the BAM path works afterwards
        c.text_open_bytes(open(os.path.join(golden, "test.vcf.bgz"), "rb").read())
        with pytest.raises(_lib.DqError) as e:
            c.sam_run()
        assert e.value.code == _lib.DQ_EINVAL


@pytest.mark.parametrize("text", [b"", K.HEADER, b"@HD\tVN:1.5"],
                         ids=["empty", "header", "header_unterminated"])
def test_empty_and_header_only(text):
    b, st = assert_sam_parity(text)
    assert st.n_partitions == 1 and st.n_records == 0 and len(b["part_offset"]) == 2


def test_storage(tmp_path, golden, bam1):
    data, text = bam1
    (tmp_path / "x.sam").write_bytes(text)
    st = HtsjdkReadsRddStorage.makeDefault().splitSize(100000)
    rdd = st.read(str(tmp_path / "x.sam"))
    ref = st.read(os.path.join(golden, "1.bam"))

    def recs(r):
        return [p.record_bytes(i) for p in r.getReads().partitions for i in range(len(p))]
    want = recs(ref)
    assert recs(rdd) == want and len(want) == 4917
    assert rdd.getHeader().raw == ref.getHeader().raw
    assert rdd.getReads().getNumPartitions() == len(O.path_splits(len(text), 100000))
    st.write(rdd, str(tmp_path / "y.bam"))
    assert recs(st.read(str(tmp_path / "y.bam"))) == want
    # a directory of .sam parts
    d = tmp_path / "parts"
    d.mkdir()
    lines = S.text_lines(text)
    hdr = b"".join(v + b"\n" for _, v in lines if v.startswith(b"@"))
    body = [v + b"\n" for _, v in lines if not v.startswith(b"@")]
    (d / "part-00000.sam").write_bytes(hdr + b"".join(body[:2000]))
    (d / "part-00001.sam").write_bytes(hdr + b"".join(body[2000:]))
    (d / "_SUCCESS").write_bytes(b"")
    assert recs(st.read(str(d))) == want
    with pytest.raises(ValueError, match="Cannot find format extension"):
        st.read(str(tmp_path / "x.cram"))
    with pytest.raises(ValueError):
        st.read(str(tmp_path / "x.sam"),
                HtsjdkReadsTraversalParameters([Interval("chr21", 1, 1000)], False))


def test_export_modes_and_arena(golden):
    text = open(os.path.join(golden, "test.sam"), "rb").read()
    with _lib.Context() as c:
        c.sam_open_bytes(text)
        full = c.sam_read(with_raw=True)
        recs = records_of(full)
        fields = c.sam_read(with_raw=False)
        assert fields["raw"] is None and np.array_equal(fields["hash"], full["hash"])
        lean = c.sam_read(with_raw="lean")
        assert np.array_equal(lean["raw"], full["raw"]) and len(lean["block_size"]) == 0
        assert np.array_equal(lean["voffset"], full["voffset"])
        off, f = _lib.parse_lean(lean["raw"], 2)
        assert np.array_equal(off, full["raw_offset"]) and np.array_equal(f["pos"], full["pos"])
        del lean, fields
        c.set_export_arena(1 << 20)
        a = c.sam_read(with_raw=True)
        assert not a["raw"].flags.writeable and records_of(a) == recs
        assert np.array_equal(a["part_digest"], full["part_digest"])
        with pytest.raises(_lib.DqError):
            c.sam_read(with_raw=True)  # the arena still holds `a`
        del a
        assert records_of(c.sam_read(with_raw="lean") | {"raw_offset": full["raw_offset"],
                                                          "block_size": full["block_size"]}) == recs


# ---- float texts at the CPU tests' scale: the device's own conversion, and the host's fix-ups
@pytest.fixture(scope="module")
def float_texts():
    """(decided, hard, exact): the texts of floatcases.sam_float_texts() the SAM rule accepts, with
    at most 19 significant digits (sam_parse_float takes them all in) and with more (it leaves
    them to the host, whatever their value), and every text's exact binary32 bytes."""
    texts = [t.encode() for t in F.sam_float_texts()]
    texts = [t for t in texts if S.FLOAT_RE.match(t)]
    decided = [t for t in texts if F.sig_digits(t.decode()) <= 19]
    hard = [t for t in texts if F.sig_digits(t.decode()) > 19]
    assert len(decided) > 65000 and len(hard) > 1500
    assert set(t.encode() for t in F.short_ties()) <= set(decided)
    return decided, hard, {t: exact_bytes(t) for t in set(texts)}


def array_line(texts, qname=b"q"):
    return K.line(qname=qname, flag=4, rname=b"*", pos=0, mapq=0, cigar=b"*", seq=b"*", qual=b"*",
                  tags=(b"XB:B:f," + b",".join(texts),))


def array_lines(texts, per_line, max_len=None, min_len=None):
    """[(line, its texts)]: B:f arrays of per_line texts each.  max_len: a line is closed early
    where one more text would take it past max_len bytes.  min_len: a last line that is not longer
    than min_len gives its texts to the line before it."""
    groups, cur = [], []
    for t in texts:
        if len(cur) == per_line or (max_len and cur and len(array_line(cur + [t], b"a%d" % len(groups))) > max_len):
            groups.append(cur)
            cur = []
        cur.append(t)
    if cur:
        if min_len and groups and len(array_line(cur)) <= min_len:
            groups[-1] += cur
        else:
            groups.append(cur)
    return [(array_line(g, b"a%d" % i), g) for i, g in enumerate(groups)]


def assert_float_parity(lines, exact, splits):
    """assert_sam_parity of HEADER + the (line, float texts) pairs at every split; the expected
    records' float bytes -- the last 4 per text of each record -- are the exact reference's, so
    the oracle's strtof is pinned to it."""
    text = K.HEADER + b"".join(l + b"\n" for l, _ in lines)
    memo = {}
    for split in splits:
        b, st = assert_sam_parity(text, split, memo=memo)
        assert st.n_records == len(lines)
    for (o, v), (l, ts) in zip([x for x in S.text_lines(text) if not x[1].startswith(b"@")], lines):
        assert v == l
        if ts:
            assert memo[o][-4 * len(ts):] == b"".join(exact[t] for t in ts), l[:60]
    return b, text


def test_float_texts_thread_path(float_texts):
    """Every text the device decides itself, in lines of up to SAM_LONG bytes: a thread per line."""
    decided, _, exact = float_texts
    lines = array_lines(decided, 100, max_len=SAM_LONG)
    singles = decided[::len(decided) // 2000][:2000]
    assert len(singles) == 2000
    lines += [(K.BASE + b"\tXF:f:" + t, [t]) for t in singles]
    assert max(len(l) for l, _ in lines) <= SAM_LONG
    assert sum(len(ts) == 100 for _, ts in lines) > len(decided) // 200     # most arrays are full
    b, _ = assert_float_parity(lines, exact, (0, 65536))
    assert len(b["part_offset"]) - 1 > 10


def test_float_texts_wave_path(float_texts):
    """The same texts in lines past SAM_LONG -- a wave per line, lane 0 walks the tags -- between
    short lines."""
    decided, _, exact = float_texts
    long_lines = array_lines(decided, 1000, min_len=SAM_LONG)
    assert min(len(l) for l, _ in long_lines) > SAM_LONG and len(long_lines) >= len(decided) // 1000
    short = [(l, []) for l in _lines24()]
    lines = []
    for i, ll in enumerate(long_lines):
        lines += [short[i % 24], ll, (K.BASE + b"\tXF:f:" + decided[i * 997], [decided[i * 997]])]
    assert_float_parity(lines, exact, (0, 65536))


def _fixup_lines(decided, hard):
    """Long lines of a hundred undecided texts each, a decided one after every undecided one, and
    short lines of (up to) ten undecided texts, in turn."""
    lines, i, k = [], 0, 0
    while i < len(hard):
        ts = []
        for t in hard[i:i + 100]:
            ts += [t, decided[k % len(decided)]]
            k += 7
        while len(array_line(ts)) <= SAM_LONG:      # the last, shorter group
            ts.append(decided[k % len(decided)])
            k += 7
        lines.append((array_line(ts, b"long%d" % len(lines)), ts))
        i += 100
        ts = []
        for t in hard[i:i + 10]:
            if ts and len(array_line(ts + [t])) > SAM_LONG:
                break
            ts.append(t)
        if ts:
            lines.append((array_line(ts, b"short%d" % len(lines)), ts))
            i += len(ts)
    return lines


def test_float_fixups_at_scale(float_texts):
    """Some 1,600 texts the host converts, in both encode kernels' fix-up lists: each value lands
    in its own 4-byte slot before the hash pass (assert_sam_parity compares the record bytes and
    the hash of every record), in partitions of 4096 bytes, some of which start inside a long line."""
    decided, hard, exact = float_texts
    lines = _fixup_lines(decided, hard)
    kinds = [len(l) > SAM_LONG for l, _ in lines]
    assert kinds[:-1] == [i % 2 == 0 for i in range(len(lines) - 1)] and sum(kinds) >= 15
    hs = set(hard)
    n_long = sum(sum(t in hs for t in ts) for (l, ts), k in zip(lines, kinds) if k)
    n_short = sum(len(ts) for (l, ts), k in zip(lines, kinds) if not k)
    assert n_long > 1000 and n_short > 100 and n_long + n_short == len(hard)
    b, text = assert_float_parity(lines, exact, (0, 4096))
    assert (np.diff(b["part_offset"]) == 0).any()           # splits in which no line starts
    # an error behind undecided texts, in a long line that follows lines with undecided texts: the
    # size pass reports it, and nothing of the fix-up counts gets in its way
    ts = lines[2][1]
    bad = array_line(ts[:9] + [b"1."] + ts[9:], b"bad")
    assert len(bad) > SAM_LONG and all(t in hs for t in ts[:9:2])
    broken = K.HEADER + b"".join(l + b"\n" for l, _ in lines[:6]) + bad + b"\n" + lines[6][0] + b"\n"
    assert sam_error(broken).endswith("SAM line %d: tag XB" % (K.HEADER.count(b"\n") + 6))
