"""The VCF site rules of tests/vcfutil.py (the oracle of the GPU VCF decode)
pinned on the CPU: the reference's test.vcf decodes to fields written out here by hand, every line
of HiSeq.10000.vcf.bgz decodes with the counts measured on that fixture, and every bad line of
tests/vcfcases.py names its error class, the earlier check first."""
import gzip
import os

import pytest

import vcfcases as K
import vcfutil as V

TEST_VCF = K.TEST_VCF


def test_test_vcf_by_hand(golden):
    text = open(os.path.join(golden, "test.vcf"), "rb").read()
    G, contigs = V.vcf_header(text)
    assert G and contigs == [b"20"]
    got = V.decode_text(text)
    assert len(got) == 5 and all(e is None for _, _, e in got)
    for (_, f, _), w in zip(got, TEST_VCF):
        pos, end, vid, ref, alts, qual, filters, flags, n_info, col_end = w
        assert (f["contig"], f["chrom"], f["pos"], f["end"], f["id"], f["ref"], f["alts"]) == \
            (0, b"20", pos, end, vid, ref, alts)
        assert (f["qual"], f["filters"], f["flags"], f["n_info"], f["col_end"]) == \
            (qual, filters, flags, n_info, col_end)
        assert f["n_alt"] == len(alts) and f["n_filter"] == len(filters) and f["n_sample_cols"] == 3
        assert not f["qual_host"]
    assert [f["n_info"] for _, f, _ in got] == [5, 3, 5, 3, 3]
    assert [f["n_alt"] for _, f, _ in got] == [1, 1, 2, 0, 2]


def test_hiseq_counts(golden):
    text = gzip.decompress(open(os.path.join(golden, "HiSeq.10000.vcf.bgz"), "rb").read())
    G, contigs = V.vcf_header(text)
    assert G and contigs == [b"chr1"]   # the trailing TAB after NA12878 adds no sample
    got = V.decode_text(text)
    assert len(got) == 9965 and all(e is None for _, _, e in got)
    fs = [f for _, f, _ in got]
    assert sum(bool(f["flags"] & V.PASS) for f in fs) == 6623
    assert sum(not f["flags"] & V.HAS_ID for f in fs) == 3348
    assert {f["n_alt"] for f in fs} == {1}
    assert {len(f["ref"]) for f in fs} == {1}
    assert {f["n_info"] for f in fs} == {11, 12, 13}
    assert all(f["contig"] == 0 for f in fs if f["chrom"] == b"chr1")
    assert all(f["flags"] & V.HAS_QUAL and not f["qual_host"] for f in fs)
    assert {f["n_sample_cols"] for f in fs} == {1}


def test_good_lines():
    text = K.HEADER + b"".join(l + b"\n" for l in K.good_lines())
    G, contigs = V.vcf_header(text)
    assert G and contigs == [b"chr1", b"chr2", b"chrM"]
    got = V.decode_text(text)
    assert [e for _, _, e in got] == [None] * len(K.good_lines())
    fs = [f for _, f, _ in got]
    assert [f["contig"] for f in fs[:4]] == [0, 1, 2, -1]
    assert fs[1]["flags"] & V.REF_LOWER and fs[1]["flags"] & V.SYMBOLIC and fs[1]["n_alt"] == 3
    assert fs[2]["flags"] & V.UNFILTERED and fs[2]["filters"] is None and fs[2]["n_info"] == 0
    assert (fs[4]["end"], fs[5]["end"], fs[6]["end"]) == (77, -4, -2147483647)
    assert fs[7]["end"] == 12 and fs[7]["flags"] & V.INFO_END
    assert sum(f["qual_host"] for f in fs) == 5
    sites = K.SITES_HEADER + b"".join(l + b"\n" for l in K.sites_good_lines())
    assert V.vcf_header(sites) == (False, [b"chr1"])
    got = V.decode_text(sites)
    assert [e for _, _, e in got] == [None] * 3
    assert all(not f["flags"] & V.HAS_GENOTYPES and f["n_sample_cols"] == 0 for _, f, _ in got)
    assert got[1][1]["end"] == 500 and got[2][1]["contig"] == -1


@pytest.mark.parametrize("case", range(len(K.bad_lines())))
def test_bad_line_names_its_class(case):
    l, what = K.bad_lines()[case]
    with pytest.raises(V.VcfError) as e:
        V.vcf_decode_line(l, True, [b"chr1", b"chr2", b"chrM"])
    assert e.value.what == what


def test_error_classes_and_order():
    seen = {}
    for _, w in K.bad_lines():
        seen[w] = seen.get(w, 0) + 1
    assert set(seen) == {"fields", "CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO"}
    assert min(seen.values()) >= 2
    for l, what in K.ORDER:
        with pytest.raises(V.VcfError) as e:
            V.vcf_decode_line(l, True, [b"chr1"])
        assert e.value.what == what, l
    for l, what in K.sites_bad_lines():
        with pytest.raises(V.VcfError) as e:
            V.vcf_decode_line(l, False, [b"chr1"])
        assert e.value.what == what, l


def test_header_without_chrom_line():
    with pytest.raises(V.VcfError, match="header"):
        V.vcf_header(b"##fileformat=VCFv4.2\n" + K.line() + b"\n")
    assert V.vcf_header(b"##fileformat=VCFv4.2\n") == (False, [])   # no data lines: accepted
    assert V.vcf_header(b"") == (False, [])


def test_qual_fast_path_predicate():
    fast = [b"0", b"50", b"12.50", b"5.", b"1e3", b"1E-5", b"123456789012345", b"-0", b"0e999",
            b"1e22", b"1e-22", b"100000000000000000000", b"0.000001", b"123456789012345e7"]
    host = [b".5", b"1e-30", b"1e400", b"123456789012345678", b"0.1234567890123456", b"1e23",
            b"1e-23", b"1234567890123456", b"123456789012345e23"]
    assert all(V.qual_fast_path(t) for t in fast)
    assert not any(V.qual_fast_path(t) for t in host)
