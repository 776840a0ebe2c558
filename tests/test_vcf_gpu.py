"""VCF site decode on the GPU: dq_vcf_* against the plain-Python
oracle tests/vcfutil.py applied to the oracle's text partitions (oracle/oracle.py) -- every column
of every variant, the three export modes, the thread / wave threshold and the ballot edges of the
TAB search, every error class, interval traversal, QUAL texts the host converts."""
import gzip
import os
import re
import struct

import numpy as np
import pytest

from disq_amd import _lib
from oracle import oracle as O
import floatcases as F
import textutil as T
import vcfcases as K
import vcfutil as V
from floatref import BINARY64, exact_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VCF_LONG = int(re.search(r"VCF_LONG = (\d+);", open(os.path.join(ROOT, "disq_amd", "csrc", "dq_vcf.hip")).read()).group(1))

COLS = ("contig", "pos", "end", "flags", "n_alt", "n_filter", "n_info", "n_sample_cols")
SAME_AS_TEXT = ("line_offset", "line_len", "hash", "part_offset", "part_digest")


def oracle_fields(u, parts, G, contigs):
    return [V.vcf_decode_line(bytes(u[a:a + l]), G, contigs)
            for vs, vl in parts for a, l in zip(vs.tolist(), vl.tolist())]


def assert_columns(b, want):
    assert len(b["pos"]) == len(want)
    for c in COLS:
        assert np.array_equal(b[c], np.array([f[c] for f in want], b[c].dtype)), c
    assert np.array_equal(b["col_end"].reshape(-1), np.array([x for f in want for x in f["col_end"]], np.int32))
    wq = np.array([f["qual"] if f["qual"] is not None else 0.0 for f in want], np.float64)
    assert np.array_equal(b["qual"].view(np.uint64), wq.view(np.uint64))   # bit for bit
    assert b["n_qual_host"] == sum(f["qual_host"] for f in want)


def assert_vcf_parity(data, split, intervals=None, tbi=None):
    ot = O.OracleText(data)
    u = ot.inflated()
    G, contigs = V.vcf_header(bytes(u))
    if intervals is None:
        parts = ot.read_partitions(split, True)
    else:
        parts = [p for _, p in ot.read_partitions_intervals(split, intervals, tbi)]
    want = oracle_fields(u, parts, G, contigs)
    with _lib.Context(split_size=split, verify_crc=True) as c:
        c.text_open_bytes(data)
        if intervals is not None:
            c.text_set_index(tbi)
            c.text_set_intervals(intervals)
        tb = c.text_read(True)
        out = {m: c.vcf_read(m) for m in (_lib.VCF_EXPORT_FIELDS, _lib.VCF_EXPORT_SITES, _lib.VCF_EXPORT_LINES)}
        tb2 = c.text_read(True)
    assert all(np.array_equal(tb[k], tb2[k]) for k in tb)      # the text calls read as before
    assert len(tb["part_offset"]) - 1 == len(parts)
    assert [int(x) for x in np.diff(tb["part_offset"])] == [len(vs) for vs, _ in parts]
    for m, b in out.items():
        for k in SAME_AS_TEXT:
            assert np.array_equal(b[k], tb[k]), (m, k)
        assert b["contigs"] == contigs
        assert_columns(b, want)
    f, s, l = (out[m] for m in (0, 1, 2))
    assert f["n_bytes"] == 0 and len(f["data"]) == 0
    assert s["n_bytes"] == int(s["col_end"][:, 7].sum()) == len(s["data"])
    assert np.array_equal(np.diff(s["data_offset"]), s["col_end"][:, 7])
    site = np.concatenate([u[a:a + e] for a, e in zip(s["line_offset"].tolist(), s["col_end"][:, 7].tolist())]) \
        if len(want) else np.zeros(0, np.uint8)
    assert np.array_equal(s["data"], site)
    assert np.array_equal(l["data"], tb["data"]) and np.array_equal(l["data_offset"], tb["data_offset"])
    return s, want


# ---- 1. fixtures
def test_test_vcf(golden):
    d = open(os.path.join(golden, "test.vcf.bgz"), "rb").read()
    b, want = assert_vcf_parity(d, 0)
    assert len(want) == 5 and b["n_qual_host"] == 0
    assert [int(x) for x in b["n_info"]] == [5, 3, 5, 3, 3] and set(b["n_sample_cols"].tolist()) == {3}


@pytest.mark.parametrize("split", [64 * 1024, 128 * 1024])
def test_hiseq(golden, split):
    d = open(os.path.join(golden, "HiSeq.10000.vcf.bgz"), "rb").read()
    b, want = assert_vcf_parity(d, split)
    assert len(want) == 9965 and b["n_qual_host"] == 0
    assert int(((b["flags"] & _lib.VCF_PASS) != 0).sum()) == 6623
    assert int(((b["flags"] & _lib.VCF_HAS_ID) == 0).sum()) == 3348


# ---- 2. thread / wave threshold and ballot edges
def _pad_to(prefix, length):
    """prefix + sample columns up to exactly `length` bytes."""
    out, rem = [prefix], length - len(prefix)
    assert rem >= 0
    while rem > 0:
        c = min(rem, 37)
        out.append(b"\t" + b"0" * (c - 1))
        rem -= c
    return b"".join(out)


def edge_lines(G):
    site7 = b"chr1\t100\trs5\tA\tT\t50\tPASS\t"
    lines = []
    if G:
        for n in (2047, 2048, 2049):                       # a thread up to 2048 bytes, a wave past them
            lines.append(_pad_to(K.line(rest=b"\tGT"), n))
        for t in (63, 64, 65, 127, 128):                   # the 8th TAB at the edge of a ballot window
            lines.append(site7 + b"DP=" + b"1" * (t - len(site7) - 3) + b"\tGT\t0/1" + b"\t1/1" * 600)
            assert lines[-1].index(b"\tGT") == t
        lines.append(site7 + b"DP=5;X=" + b"a" * 3000 + b";END=777" + b"\tGT\t0/1")   # 8th TAB past 2048
        lines.append(site7 + b"END=9;X=" + b"a" * 2040 + b"\tGT" + b"\t0/1" * 200)
        lines += K.good_lines()
    else:
        for n in (2047, 2048, 2049):
            lines.append(site7 + b"DP=" + b"7" * (n - len(site7) - 3))
        for t in (63, 64, 65):
            lines.append(site7 + b"DP=" + b"1" * (t - len(site7) - 3))
        lines.append(site7 + b"DP=5;X=" + b"a" * 3000 + b";END=777")
        lines += K.sites_good_lines()
    k = 0
    while len(lines) < 64:
        lines.append(K.line(pos=b"%d" % (1000 + k), rest=b"\tGT\t0/1\t1/1" if G else b""))
        k += 1
    return lines


@pytest.mark.parametrize("G", [True, False])
def test_thread_wave_and_ballot_edges(G):
    lines = edge_lines(G)
    text = (K.HEADER if G else K.SITES_HEADER) + b"".join(l + b"\n" for l in lines)
    data = T.bgzf_text(text, block_u=3000, cuts=T.corner_cuts(text))
    for split in (0, len(data) // 3):                       # one partition, and three or more
        b, want = assert_vcf_parity(data, split)
        assert len(want) == len(lines) and (len(b["part_offset"]) - 1 >= 3) == bool(split)
        lens = set(b["line_len"].tolist())
        assert {2047, 2048, 2049} <= lens
        if G:
            assert {63, 64, 65, 127, 128} <= set(b["col_end"][:, 7].tolist())
            assert int(b["col_end"][:, 7].max()) > 2048 and int(b["n_sample_cols"].max()) == 601


# ---- 3. errors
def _error_of(c, data):
    c.text_open_bytes(data)
    with pytest.raises(_lib.DqError) as e:
        c.vcf_read(_lib.VCF_EXPORT_SITES)
    assert e.value.code == _lib.DQ_EFORMAT
    return str(e.value)


def _file(lines, header=K.HEADER):
    return T.bgzf_text(header + b"".join(l + b"\n" for l in lines))


NH = K.HEADER.count(b"\n")   # '#' lines before the first data line


def test_every_error_class_as_the_last_line():
    good = [K.line(pos=b"%d" % (10 + i)) for i in range(39)]
    with _lib.Context() as c:
        for bad, what in K.bad_lines() + K.ORDER:
            msg = _error_of(c, _file(good + [bad]))
            assert msg.endswith(f"VCF line {NH + 39}: {what}"), (bad, msg)
            assert len(c.text_read(True)["line_len"]) == 40     # the text calls still work
        for bad, what in K.sites_bad_lines():
            sites = [K.line(pos=b"%d" % (10 + i), rest=b"") for i in range(39)]
            msg = _error_of(c, _file(sites + [bad], K.SITES_HEADER))
            assert msg.endswith(f"VCF line {K.SITES_HEADER.count(bytes([10])) + 39}: {what}"), (bad, msg)


def test_first_offender_wins():
    good = [K.line(pos=b"%d" % (10 + i)) for i in range(38)]
    with _lib.Context() as c:
        # the later class (INFO) earlier in the file than the earlier class (CHROM)
        lines = good[:5] + [K.line(info=b"")] + good[5:30] + [K.line(chrom=b"")] + good[30:]
        assert _error_of(c, _file(lines)).endswith(f"VCF line {NH + 5}: INFO")
        # at the first data line
        assert _error_of(c, _file([K.line(pos=b"x")] + good)).endswith(f"VCF line {NH}: POS")
        # long lines go through the wave kernel
        long_bad = K.line(info=b"DP=1; X=2") + b"\t0/1" * 700
        assert len(long_bad) > 2048
        assert _error_of(c, _file(good[:7] + [long_bad] + good[7:])).endswith(f"VCF line {NH + 7}: INFO")
        assert _error_of(c, _file(good + [b"x" * 3000])).endswith(f"VCF line {NH + 38}: fields")
        long_ref = K.line(ref=b"AC!T") + b"\t0/1" * 700
        assert _error_of(c, _file(good[:3] + [long_ref, K.line(chrom=b"")] + good[3:])).endswith(
            f"VCF line {NH + 3}: REF")
        # no #CHROM line
        msg = _error_of(c, T.bgzf_text(b"##fileformat=VCFv4.2\n" + K.line() + b"\n"))
        assert "VCF header: no #CHROM line" in msg
        assert len(c.text_read(True)["line_len"]) == 1


def make_vcf(n, seed):
    """textutil.make_vcf with the lines whose ALT repeats their REF (T and T: htsjdk's "Duplicate
    allele") given another ALT."""
    out = []
    for l in T.make_vcf(n, seed=seed).split(b"\n")[:-1]:
        f = l.split(b"\t")
        if not l.startswith(b"#") and f[3] == f[4]:
            f[4] = b"G"
        out.append(b"\t".join(f))
    return b"\n".join(out) + b"\n"


def _tabix_upto(contigs, end_off):
    """A decompressed tabix index whose only bin holds one chunk over file offsets [0, end_off)."""
    names = b"".join(c.encode() + b"\x00" for c in contigs)
    d = b"TBI\x01" + struct.pack("<iiiiiiii", len(contigs), 2, 1, 2, 0, ord("#"), 0, len(names)) + names
    for _ in contigs:
        d += struct.pack("<i", 1) + struct.pack("<Ii", 0, 1) + struct.pack("<QQ", 0, end_off << 16)
        d += struct.pack("<i", 0)
    return d


def test_errors_follow_the_kept_splits():
    lines = make_vcf(6000, seed=11).split(b"\n")[:-1]
    bad = b"chrX\t999999999\t.\tA\tT\t50\tPASS\tDP=1; X"      # a valid CHROM and POS outside every interval
    split, ivs = 15000, [("chr1", 1, 5000)]

    def run(ls):
        data = T.bgzf_text(b"\n".join(ls) + b"\n", block_u=8000)
        assert len(data) > 2 * split
        with _lib.Context(split_size=split) as c:
            c.text_open_bytes(data)
            c.text_set_index(_tabix_upto(["chr1", "chr2", "chrX"], 10000))
            c.text_set_intervals(ivs)
            st = c.text_run()
            assert st.n_partitions == 1                      # the index prunes every split but the first
            return c.vcf_read(_lib.VCF_EXPORT_FIELDS)

    # in a split the tabix pruning drops: no error
    b = run(lines + [bad])
    assert len(b["pos"]) > 0 and all(0 < p <= 5000 for p in b["pos"].tolist())
    # in the kept split, outside every interval: Disq decodes before it filters
    with pytest.raises(_lib.DqError, match="VCF line 40: INFO"):
        run(lines[:40] + [bad] + lines[40:])


# ---- 4. intervals
@pytest.mark.parametrize("intervals", [
    [("chr1", 2700000, 2800000)],
    [("chr1", 1, 100000)],
    [("chr1", 2700000, 2800000), ("chr1", 4000000, 4100000), ("chr1", 4050000, 4060000)],
    [("chr2", 1, 1000000)],
    [("chr1", 1, 300000000)],
])
def test_hiseq_intervals(golden, intervals):
    d = open(os.path.join(golden, "HiSeq.10000.vcf.bgz"), "rb").read()
    tbi = open(os.path.join(golden, "HiSeq.10000.vcf.bgz.tbi"), "rb").read()
    b, want = assert_vcf_parity(d, 128 * 1024, intervals, tbi)
    txt = gzip.decompress(d)
    exp = [l for l in T.split_lines(txt) if not l.startswith(b"#") and O.vcf_overlaps(l, intervals)]
    assert len(want) == len(exp)
    for ci, p, e in zip(b["contig"].tolist(), b["pos"].tolist(), b["end"].tolist()):
        name = b["contigs"][ci].decode()
        assert any(c == name and p <= hi and e >= lo for c, lo, hi in intervals)


def test_synthetic_intervals_with_info_end():
    text = make_vcf(6000, seed=4)
    data = T.bgzf_text(text, block_u=8000)
    tbi = T.whole_file_tabix(["chr1", "chr2", "chrX"], len(data))
    rng = np.random.default_rng(9)
    ivs = [(("chr1", "chr2", "chrX", "chr7")[int(rng.integers(0, 4))], int(a), int(a) + int(rng.integers(0, 3000)))
           for a in rng.integers(1, 400000, size=40)]
    for split in (0, 30000):
        b, want = assert_vcf_parity(data, split, ivs, tbi)
        ends = (b["flags"] & _lib.VCF_INFO_END) != 0
        assert 0 < int(ends.sum()) < len(want)
        assert np.array_equal(ends, (b["flags"] & _lib.VCF_SYMBOLIC) != 0)
        assert np.all(b["end"][ends] >= b["pos"][ends] + 50) and np.all(b["contig"] == -1)


# ---- 5. QUAL off the fast path
def test_qual_texts_the_host_converts():
    texts = [b"1e-30", b"1e400", b"123456789012345678", b".5"]
    lines = [K.line(pos=b"%d" % (5 + i), qual=q) for i, q in enumerate(texts)] + [K.line(qual=b"12.5")]
    b, want = assert_vcf_parity(_file(lines), 0)
    assert b["n_qual_host"] == len(texts)
    for q, t in zip(b["qual"].tolist(), texts):
        assert struct.pack("<d", q) == struct.pack("<d", float(t))
    assert b["qual"][4] == 12.5


# ---- 6. QUAL texts at the CPU test's scale: the device's f64 multiply / divide, the host's list
def assert_quals_exact(want, texts):
    """The oracle's float() pinned to the exact reference: variant i's QUAL is texts[i]'s binary64."""
    assert len(want) == len(texts)
    for f, t in zip(want, texts):
        assert struct.unpack("<Q", struct.pack("<d", f["qual"]))[0] == exact_bits(t, BINARY64), t


def test_qual_texts_bit_for_bit():
    texts = [t.encode() for t in F.qual_texts()[:21000] + F.qual_edge_texts() + F.QUAL_EXTRA]
    assert len(texts) == 21000 + 1200 + len(F.QUAL_EXTRA)
    lines = [K.line(pos=b"%d" % (i + 1), qual=t) for i, t in enumerate(texts)]
    data = T.bgzf_text(K.HEADER + b"".join(l + b"\n" for l in lines))
    for split in (0, 70000):
        b, want = assert_vcf_parity(data, split)
        assert (len(b["part_offset"]) - 1 > 2) == bool(split)
        host = sum(f["qual_host"] for f in want)
        assert len(want) - host > len(lines) // 2            # the device's own path is what is under test
        assert host > 1000 and b["n_qual_host"] == host
    assert_quals_exact(want, texts)
    # the edge of the exact path: 15 digits times 10^+-22 on the device, times 10^+-23 on the host
    assert [f["qual_host"] for f in want[21000:22200]] == [i // 200 >= 4 for i in range(1200)]


def _long_line_file():
    """(text, QUAL texts, which lines are long): chr1 lines at POS 1000, 1010, ...; every other one
    carries 600 genotype columns, which takes it past VCF_LONG; QUAL texts the device decides and
    texts it leaves to the host in both kinds of line."""
    edge = F.qual_edge_texts()
    pool = edge[0:40] + edge[800:840] + edge[400:440] + edge[1000:1040] + F.QUAL_EXTRA
    texts, lines, is_long = [], [], []
    for i in range(320):
        t = pool[(i // 2 + (len(pool) // 2) * (i % 2)) % len(pool)].encode()    # both kinds see the whole pool
        rest = K.GT + (b"\t0|1:35:4" * 598 if i % 2 else b"")
        texts.append(t)
        lines.append(K.line(pos=b"%d" % (1000 + 10 * i), qual=t, rest=rest))
        is_long.append(bool(i % 2))
    assert all((len(l) > VCF_LONG) == k for l, k in zip(lines, is_long))
    for k in (False, True):
        fast = [V.qual_fast_path(t) for t, kk in zip(texts, is_long) if kk == k]
        assert sum(fast) > 40 and len(fast) - sum(fast) > 40
    return K.HEADER + b"".join(l + b"\n" for l in lines), texts, is_long


def test_qual_in_long_lines():
    text, texts, is_long = _long_line_file()
    data = T.bgzf_text(text, block_u=8000)
    for split in (0, 4000):
        b, want = assert_vcf_parity(data, split)                 # all three export modes
        assert b["n_qual_host"] == sum(not V.qual_fast_path(t) for t in texts) > 80
        assert (len(b["part_offset"]) - 1 > 2) == bool(split)
        assert int(b["n_sample_cols"].max()) == 600 and (b["line_len"] > VCF_LONG).tolist() == is_long
    assert_quals_exact(want, texts)
    # intervals: every line is validated (and its undecided QUAL counted), the kept ones are decoded
    tbi = T.whole_file_tabix(["chr1", "chr2", "chrM"], len(data))
    ivs = [("chr1", 1200, 1495), ("chr1", 2000, 2001), ("chr1", 3005, 3990), ("chr2", 1, 5000)]
    keep = [any(lo <= 1000 + 10 * i <= hi for c, lo, hi in ivs if c == "chr1") for i in range(len(texts))]
    all_host = sum(not V.qual_fast_path(t) for t in texts)
    for split in (0, 4000):
        b, want = assert_vcf_parity(data, split, ivs, tbi)
        assert b["pos"].tolist() == [1000 + 10 * i for i, k in enumerate(keep) if k]
        host = sum(not V.qual_fast_path(t) for t, k in zip(texts, keep) if k)
        assert 0 < host < all_host and b["n_qual_host"] == host
        kept_long = [l for l, k in zip(is_long, keep) if k]
        assert (b["line_len"] > VCF_LONG).tolist() == kept_long and 20 < sum(kept_long) < len(kept_long)
    assert_quals_exact(want, [t for t, k in zip(texts, keep) if k])


# ---- 7. edges
def test_header_only_file():
    text = b"".join(b"##meta=%d\n" % i for i in range(2000)) + K.HEADER
    data = T.bgzf_text(text, block_u=3000)
    for split in (0, 2000):
        with _lib.Context(split_size=split) as c:
            c.text_open_bytes(data)
            tb = c.text_read(True)
            b = c.vcf_read(_lib.VCF_EXPORT_SITES)
            st = c.vcf_run()
        assert len(b["pos"]) == 0 and b["n_bytes"] == 0 and st.n_records == 0
        assert np.array_equal(b["part_offset"], tb["part_offset"]) and len(b["part_offset"]) >= 2
        assert np.array_equal(b["part_digest"], tb["part_digest"])
        assert b["contigs"] == [b"chr1", b"chr2", b"chrM"]


def test_other_contexts_and_modes_are_refused(golden):
    import samcases
    with _lib.Context() as c:
        with pytest.raises(_lib.DqError) as e:     # no open file
            c.vcf_read()
        assert e.value.code == _lib.DQ_EINVAL
        c.open_bytes(open(os.path.join(golden, "1.bam"), "rb").read())
        for call in (c.vcf_read, c.vcf_run):
            with pytest.raises(_lib.DqError) as e:
                call()
            assert e.value.code == _lib.DQ_EINVAL
        c.sam_open_bytes(samcases.HEADER + samcases.good_lines()[0] + b"\n")
        for call in (c.vcf_read, c.vcf_run):
            with pytest.raises(_lib.DqError) as e:
                call()
            assert e.value.code == _lib.DQ_EINVAL
        c.text_open_bytes(open(os.path.join(golden, "test.vcf.bgz"), "rb").read())
        with pytest.raises(_lib.DqError) as e:
            c.vcf_read(3)
        assert e.value.code == _lib.DQ_EINVAL
        assert len(c.vcf_read(_lib.VCF_EXPORT_LINES)["pos"]) == 5


def test_vcf_run_stats(golden):
    d = open(os.path.join(golden, "HiSeq.10000.vcf.bgz"), "rb").read()
    with _lib.Context(split_size=128 * 1024) as c:
        c.text_open_bytes(d)
        t = c.text_run(True)
        v = c.vcf_run()
        b = c.vcf_read(_lib.VCF_EXPORT_FIELDS)      # the columns of the run, no second decode needed
    assert (v.n_records, v.n_partitions, v.digest) == (t.n_records, t.n_partitions, t.digest) == (9965, 4, t.digest)
    assert v.ms_records > 0 and v.ms_total > v.ms_records and len(b["pos"]) == 9965


def test_storage_decode(golden, tmp_path):
    """read(decode=True): VariantSite rows equal to test.vcf's fields written out by hand."""
    import shutil
    from disq_amd.storage import HtsjdkVariantsRddStorage, VariantSite
    p = str(tmp_path / "test.vcf.bgz")
    shutil.copy(os.path.join(golden, "test.vcf.bgz"), p)
    st = HtsjdkVariantsRddStorage.makeDefault()
    v = st.read(p, decode=True).getVariants()
    info = [l.split(b"\t")[7] for l in st.read(p).getVariants().collect()]   # the default: lines, as before
    want = [VariantSite(b"20", pos, end, vid, ref, alts, qual, filters, inf)
            for (pos, end, vid, ref, alts, qual, filters, _, _, _), inf in zip(K.TEST_VCF, info)]
    assert v.getNumPartitions() == 1 and v.collect() == want
    assert want[1].filters == {b"q10"} and want[3].alts == [] and want[0].info == b"NS=3;DP=14;AF=0.5;DB;H2"
