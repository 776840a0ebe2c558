"""The genotype oracle tests/vcfgtutil.py pinned: the cells of
tests/golden/test.vcf written out by hand, counts over HiSeq.10000.vcf.bgz, the table of bad lines,
Java's rounding."""
import gzip
import os
import re

import pytest

import textutil as T
import vcfcases as K
import vcfgtcases as GK
import vcfgtutil as G
import vcfutil as V

ALL = G.HAS_GT | G.HAS_GQ | G.HAS_DP
PH = G.PHASED

# (alleles, phased, GQ, DP) of the 15 cells of test.vcf, line by line
TEST_VCF_CELLS = [
    [((0, 0), True, 48, 1), ((1, 0), True, 48, 8), ((1, 1), False, 43, 5)],
    [((0, 0), True, 49, 3), ((0, 1), True, 3, 5), ((0, 0), False, 41, 3)],     # 0/0:41:3: HQ missing
    [((1, 2), True, 21, 6), ((2, 1), True, 2, 0), ((2, 2), False, 35, 4)],     # the two-ALT line
    [((0, 0), True, 54, 7), ((0, 0), True, 48, 4), ((0, 0), False, 61, 2)],
    [((0, 1), False, 35, 4), ((0, 2), False, 17, 2), ((1, 1), False, 40, 3)],
]


def test_test_vcf_by_hand(golden):
    text = open(os.path.join(golden, "test.vcf"), "rb").read()
    names, rows = G.decode_text(text)
    assert names == [b"NA00001", b"NA00002", b"NA00003"]
    assert len(rows) == 5 and all(e is None for _, _, e in rows)
    for (k, cells, _), want in zip(rows, TEST_VCF_CELLS):
        line = T.split_lines(text)[k]
        assert len(cells) == 3
        for c, (al, ph, gq, dp) in zip(cells, want):
            assert tuple(c["alleles"]) == al and c["gq"] == gq and c["dp"] == dp
            assert c["flags"] == ALL | (PH if ph else 0) and not c["gq_host"]
        # cell_off: the cell's first byte
        cols = line.split(b"\t")
        for s, c in enumerate(cells):
            assert line[c["cell_off"]:].split(b"\t")[0] == cols[9 + s]
            assert line[c["cell_off"] - 1:c["cell_off"]] == b"\t"
    # "1|0:48:8:51,51" and "0/0:41:3" and "2/2:35:4", as the issue spells them
    assert (rows[0][1][1]["alleles"], rows[0][1][1]["gq"], rows[0][1][1]["dp"]) == ([1, 0], 48, 8)
    assert (rows[1][1][2]["gq"], rows[1][1][2]["dp"]) == (41, 3)
    assert rows[2][1][2]["alleles"] == [2, 2]


def test_hiseq_counts(golden):
    text = gzip.decompress(open(os.path.join(golden, "HiSeq.10000.vcf.bgz"), "rb").read())
    names, rows = G.decode_text(text)
    assert names == [b"NA12878"]                       # the #CHROM line's trailing TAB: S = 1
    assert all(e is None and len(c) == 1 for _, c, e in rows)
    cells = [c[0] for _, c, _ in rows]
    assert len(cells) == 9965
    assert sum(c["alleles"] == [0, 1] for c in cells) == 7128 and sum(c["alleles"] == [1, 1] for c in cells) == 2837
    assert not any(c["flags"] & G.PHASED for c in cells)
    gq_texts = []
    for l in T.split_lines(text):
        if not l.startswith(b"#"):
            f = l.split(b"\t")
            keys = f[8].split(b":")
            gq_texts.append(f[9].split(b":")[keys.index(b"GQ")])
    assert sum(b"." in t for t in gq_texts) == 1794
    assert sum(t.endswith(b".5") or re.fullmatch(rb"[0-9]+\.50*", t) is not None for t in gq_texts) == 11
    assert all(G.GQ_DEVICE_RE.match(t) for t in gq_texts) and not any(c["gq_host"] for c in cells)
    assert sum(c["gq"] for c in cells) == 907868 and sum(c["dp"] for c in cells) == 611423


def _decode(line, header=K.HEADER):
    names, rows = G.decode_text(header + line + b"\n")
    assert len(rows) == 1
    return names, rows[0]


@pytest.mark.parametrize("line,what,sample", GK.BAD + GK.ORDER)
def test_bad_lines(line, what, sample):
    V.vcf_decode_line(line, True, [b"chr1", b"chr2", b"chrM"])      # the site decode accepts it
    names, (k, cells, e) = _decode(line)
    assert len(names) == 2 and cells is None
    assert (e.what, e.sample) == (what, sample)
    mid = "" if sample is None else f"sample {sample}: "
    assert e.message(k) == f"VCF line {k}: {mid}{what}"


def test_at_least_two_bad_lines_per_class():
    for what in ("samples", "FORMAT", "cell", "GT", "GQ", "DP"):
        assert sum(w == what for _, w, _ in GK.BAD) >= 2, what


def test_good_lines():
    rows = [_decode(l)[1] for l in GK.GOOD]
    assert all(e is None for _, _, e in rows)
    c = [cells for _, cells, _ in rows]
    assert c[0][1] == {"flags": ALL | PH | G.FILTERED, "alleles": [1, 1], "gq": 13, "dp": 7, "gq_host": False,
                       "cell_off": c[0][1]["cell_off"]}
    assert c[0][0]["flags"] == ALL                                     # FT PASS does not filter
    assert (c[1][0]["gq"], c[1][0]["dp"], c[1][1]["flags"], c[1][1]["alleles"]) == (41, 3, G.HAS_GT, [-1, -1])
    assert c[2][0]["flags"] == G.HAS_GQ | G.HAS_DP and c[2][1]["flags"] == 0 and c[2][1]["gq"] == -1
    assert [x["alleles"] for x in c[3]] == [[], []] and all(x["flags"] == G.HAS_GT for x in c[3])
    assert [x["alleles"] for x in c[4]] == [[-1], [0]]
    assert [x["alleles"] for x in c[5]] == [[0, 1], [0, 1, 0]] and c[5][0]["flags"] == G.HAS_GT
    assert [x["alleles"] for x in c[6]] == [[1, 0], [1, 1]]
    assert [(x["gq"], bool(x["flags"] & G.HAS_GQ)) for x in c[7]] == [(-1, False), (-1, True)]
    assert [x["gq"] for x in c[8]] == [1, 0] and [x["gq"] for x in c[9]] == [-2, -3]
    assert [x["gq"] for x in c[10]] == [1000000000, -999999999] and [x["gq"] for x in c[11]] == [7, 3]
    assert [x["dp"] for x in c[12]] == [-7, 0]
    assert [bool(x["flags"] & G.FILTERED) for x in c[13]] == [False, True]
    assert (c[14][0]["dp"], c[14][1]["dp"]) == (3, -1) and [x["gq"] for x in c[15]] == [9, 8]
    assert not any(x["gq_host"] for cells in c[:16] for x in cells)
    # the host's texts: 1e1, .5, 12.5000000, 1234567890, 0.4999...9 (its binary64 is 0.5), 1e400
    host = [x for cells in c[16:] for x in cells]
    assert all(x["gq_host"] and x["flags"] & G.HAS_GQ for x in host)
    assert [x["gq"] for x in host] == [10, 1, 13, 1234567890, 1, -1, 0, 1]


def test_java_round():
    r = G.java_round_to_int
    assert [r(x) for x in (0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.49999999999999994, -0.0)] == [1, 0, 2, -1, 3, -2, 0, 0]
    assert r(float("inf")) == -1 and r(float("-inf")) == 0 and r(float("nan")) == 0
    assert r(2147483648.0) == -2147483648 and r(4294967297.0) == 1 and r(1e19) == -1 and r(-1e19) == 0
    assert r(4503599627370497.0) == 1                               # 2^52 + 1: already an integer


def test_sample_names():
    assert G.sample_names(K.SITES_HEADER) == []
    assert G.sample_names(K.HEADER) == [b"S1", b"S2"]
    h = K.SITES_HEADER.rstrip(b"\n")
    assert G.sample_names(h + b"\tFORMAT\tA\t\tB\t\t\n") == [b"A", b"", b"B"]
    assert G.sample_names(h + b"\tFORMAT\t\tB\n") == []             # the tenth column is empty: no sample
    assert G.sample_names(GK.header(130))[129] == b"S129"
