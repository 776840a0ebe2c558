"""Tabix index build (row f6, DESIGN.md "Building the .tbi"): dq_text_write_tbi,
TabixIndexer.createIndex and HtsjdkVariantsRddStorage.write(..., tabix=True).

Pinning: htsjdk is not vendored, so TabixIndexCreator / BinningIndexBuilder are restated in
tests/tbiutil.py (plain Python, zlib only).  The restatement is pinned by the reference's own
fixture, HiSeq.10000.vcf.bgz.tbi (made by htslib: the same bins, chunks and linear index, plus a
pseudo-bin 37450 and a trailing count that htsjdk does not write), and by the oracle's interval
traversal, which must select the same splits and lines through either index.  The GPU index must
equal the restatement byte for byte."""
import functools
import gzip
import os
import re
import shutil
import struct

import numpy as np
import pytest

from oracle import oracle as O
import bamutil as B
import tbiutil as TU
import textutil as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SPLIT = 128 * 1024
HISEQ_INTERVALS = [
    ([("chr1", 2700000, 2800000)], 1),
    ([("chr1", 1, 100000)], None),
    ([("chr1", 2700000, 2800000), ("chr1", 4000000, 4100000), ("chr1", 4050000, 4060000)], None),
    ([("chr2", 1, 1000000)], 0),
    ([("chr1", 1, 300000000)], 4),
]


def golden_bytes(name):
    with open(os.path.join(GOLDEN, name), "rb") as fh:
        return fh.read()


def level(b):
    return 5 if b >= 4681 else 4 if b >= 585 else 3 if b >= 73 else 2 if b >= 9 else 1 if b >= 1 else 0


def vcf_line(chrom, pos, ref=b"A", info=b"DP=1", alt=b"T"):
    return b"\t".join([chrom, b"%d" % pos, b".", ref, alt, b"50", b"PASS", info])


HEAD = [b"##fileformat=VCFv4.2", b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]


def levels_text():
    """Records whose [POS - 1, end) crosses a 16 kb, 128 kb, 1 Mb, 8 Mb and 64 Mb boundary: one bin
    on every level, the last end exactly 2^29."""
    rows = [(100, 200), (16000, 17000), (130000, 140000), (1000000, 1100000), (8000000, 9000000),
            (60000000, 70000000), (1 << 29, 1 << 29)]
    return b"\n".join(HEAD + [vcf_line(b"chr1", p, info=b"SVTYPE=DEL;END=%d" % e, alt=b"<DEL>")
                              for p, e in rows]) + b"\n"


def wide_text():
    """40 lines of 3000 bytes of sample columns."""
    rng = np.random.default_rng(5)
    out = HEAD[:1] + [HEAD[1] + b"\tFORMAT" + b"".join(b"\tS%03d" % i for i in range(748))]
    for i in range(40):
        gt = b"\t".join((b"0/0", b"0/1", b"1/1")[int(x)] for x in rng.integers(0, 3, 748))
        out.append(vcf_line(b"chr1" if i < 25 else b"chr2", 1000 + 37 * i) + b"\tGT\t" + gt)
    return b"\n".join(out) + b"\n"


@functools.lru_cache(maxsize=None)
def inputs():
    text = T.make_vcf(600, seed=4)
    ls = text.split(b"\n")[:-1]
    gaps = b"\n".join(ls[:40] + [b"", b"#a comment between records"] + ls[40:300] + [b"", b""] + ls[300:]) + b"\n"
    d700 = T.bgzf_text(text, block_u=700)
    assert d700.endswith(B.EOF_BLOCK)
    return {
        "hiseq": golden_bytes("HiSeq.10000.vcf.bgz"),
        "test": golden_bytes("test.vcf.bgz"),
        "syn300": T.bgzf_text(text, block_u=300),
        "syn700": d700,
        "syn8000": T.bgzf_text(text, block_u=8000),
        "crlf": T.bgzf_text(text.replace(b"\n", b"\r\n"), block_u=700),
        "gaps": T.bgzf_text(gaps, block_u=700),
        "no_last_terminator": T.bgzf_text(text[:-1], block_u=700),
        "no_eof_block": d700[:-len(B.EOF_BLOCK)],
        "header_only": T.bgzf_text(b"\n".join(HEAD) + b"\n"),
        "wide": T.bgzf_text(wide_text(), block_u=1000),
        "levels": T.bgzf_text(levels_text(), block_u=120),
        "one_line": T.bgzf_text(b"\n".join(HEAD + [vcf_line(b"chr1", 1000)]) + b"\n"),
        "eof_only": B.EOF_BLOCK,
        "two_eof_blocks": d700 + B.EOF_BLOCK,
    }


@functools.lru_cache(maxsize=None)
def restated(name):
    return TU.build_tbi(inputs()[name])


@functools.lru_cache(maxsize=None)
def error_inputs():
    """name -> (file, the offending line's index among all lines)."""
    ls = T.make_vcf(60, seed=1).split(b"\n")[:-1]   # 2 header lines, 20 lines per contig

    def f(k):
        return ls[k].split(b"\t")

    def with_line(k, fields):
        return T.bgzf_text(b"\n".join(ls[:k] + [b"\t".join(fields)] + ls[k + 1:]) + b"\n", block_u=500)
    down = f(12)
    down[1] = b"%d" % (int(f(11)[1]) - 1)
    letters = f(30)
    letters[1] = b"12x"
    far = f(50)
    far[7] = b"END=%d" % ((1 << 29) + 1)
    back = T.bgzf_text(b"\n".join(ls + [vcf_line(b"chr1", 900000)]) + b"\n", block_u=500)
    return {"pos_down": (with_line(12, down), 12), "contig_back": (back, 62),
            "pos_not_numeric": (with_line(30, letters), 30), "end_too_far": (with_line(50, far), 50)}


def strip_htslib(p):
    """The parts of a parsed index that htsjdk writes too."""
    return (p["format"], p["names"], [(r["bins"], r["linear"]) for r in p["refs"]])


def seeded_intervals(n=8, seed=9):
    rng = np.random.default_rng(seed)
    ivs = [(("chr1", "chr2", "chrX")[int(rng.integers(0, 3))], int(a), int(a) + int(rng.integers(0, 3000)))
           for a in rng.integers(1, 45000, size=n)]
    return ivs + [("chr7", 1, 100000)]


def data_lines(data):
    return [l for l in T.split_lines(gzip.decompress(data)) if l and not l.startswith(b"#")]


# ------------------------------------------------------------------ CPU: the restatement is pinned
def test_restatement_equals_fixture():
    fx = TU.parse_tbi(golden_bytes("HiSeq.10000.vcf.bgz.tbi"))
    mine = TU.parse_tbi(restated("hiseq"))
    assert len(TU.records(inputs()["hiseq"])) == 9965
    assert mine["names"] == [b"chr1"] and len(mine["refs"][0]["bins"]) == 298
    assert len(mine["refs"][0]["linear"]) == 320
    assert restated("hiseq")[:36 + 5] == gzip.decompress(golden_bytes("HiSeq.10000.vcf.bgz.tbi"))[:36 + 5]
    assert strip_htslib(mine) == strip_htslib(fx)
    # what htslib adds: the pseudo-bin (the contig's span, its line count) and a zero trailing count;
    # the span's end is the EOF block's address, the final pointer
    assert fx["refs"][0]["pseudo"] == [(9223, 509222 << 16), (9965, 0)] and fx["n_no_coor"] == 0
    assert mine["refs"][0]["pseudo"] is None and mine["n_no_coor"] is None
    eof_at = len(inputs()["hiseq"]) - len(B.EOF_BLOCK)
    assert eof_at == 509222
    assert max(e for ch in mine["refs"][0]["bins"].values() for _, e in ch) == eof_at << 16


@pytest.mark.parametrize("intervals,counts", [
    ([("chr1", 2700000, 2800000)], [243]),
    ([("chr1", 1, 100000)], None),
    ([("chr1", 1, 300000000)], [2577, 2586, 2631, 2171]),
])
def test_oracle_traversal_same_through_either_index(intervals, counts):
    ot = O.OracleText(inputs()["hiseq"])
    a = ot.read_partitions_intervals(SPLIT, intervals, golden_bytes("HiSeq.10000.vcf.bgz.tbi"))
    b = ot.read_partitions_intervals(SPLIT, intervals, restated("hiseq"))
    assert [k for k, _ in a] == [k for k, _ in b]
    for (_, (vs, vl)), (_, (ws, wl)) in zip(a, b):
        assert np.array_equal(vs, ws) and np.array_equal(vl, wl)
    if counts is None:
        assert sum(len(p[0]) for _, p in a) == 189
    else:
        assert [len(p[0]) for _, p in a] == counts


def test_rules_the_fixture_does_not_reach():
    """The fixture has only level-5 bins and one chunk per bin.  The synthetic file has three
    contigs and bins with several chunks, on two levels (its records stay below 50 kb, so only the
    16 kb and 128 kb levels occur); the `levels` file puts one bin on each of the six levels."""
    p = TU.parse_tbi(restated("syn700"))
    assert p["names"] == [b"chr1", b"chr2", b"chrX"]
    for r in p["refs"]:
        assert len(r["bins"]) == 4 and 6 <= sum(len(c) for c in r["bins"].values()) <= 7
        assert len(r["linear"]) == 3
        assert len({level(b) for b in r["bins"]}) >= 2
    assert any(len(c) > 1 for r in p["refs"] for c in r["bins"].values())
    q = TU.parse_tbi(restated("levels"))
    assert {level(b) for b in q["refs"][0]["bins"]} == {0, 1, 2, 3, 4, 5}
    assert len({level(b) for b in q["refs"][0]["bins"]}) >= 3
    assert len(q["refs"][0]["linear"]) == 1 << 15
    # the traversal through the index selects what brute force selects
    data = inputs()["syn700"]
    ot = O.OracleText(data)
    lines = data_lines(data)
    for iv in seeded_intervals():
        got = [l for _, part in ot.read_partitions_intervals(6000, [iv], restated("syn700"))
               for l in ot.lines(part)]
        assert got == [l for l in lines if O.vcf_overlaps(l, [iv])], iv
    assert any(O.vcf_overlaps(l, seeded_intervals()[:-1]) for l in lines)


def test_restatement_smallest_inputs():
    """One data line; no decompressed byte at all; two empty blocks behind the last line, where the
    final pointer is the first of them."""
    p = TU.parse_tbi(restated("one_line"))
    assert len(TU.records(inputs()["one_line"])) == 1 and p["names"] == [b"chr1"]
    assert len(p["refs"][0]["bins"]) == 1 and [len(c) for c in p["refs"][0]["bins"].values()] == [1]
    assert gzip.decompress(inputs()["eof_only"]) == b"" and len(inputs()["eof_only"]) == 28
    assert restated("eof_only") == restated("header_only") and len(restated("eof_only")) == 36
    two, one = inputs()["two_eof_blocks"], inputs()["syn700"]
    assert two.endswith(2 * B.EOF_BLOCK) and not one.endswith(2 * B.EOF_BLOCK)
    first_eof = len(one) - len(B.EOF_BLOCK)
    assert TU.records(two)[-1][2] == first_eof << 16 == TU.records(one)[-1][2]
    assert restated("two_eof_blocks") == restated("syn700")


@pytest.mark.parametrize("name", ["pos_down", "contig_back", "pos_not_numeric", "end_too_far"])
def test_restatement_errors(name):
    data, k = error_inputs()[name]
    with pytest.raises(ValueError, match=rf"line {k}\b"):
        TU.build_tbi(data)


def test_restatement_line_rules():
    """Blank and '#' lines between records move no pointer but their own: a record's chunk ends
    after its own terminator.  A BOM belongs to line 0; CR LF and a missing last terminator."""
    u = b"\xef\xbb\xbf#h\r\n" + vcf_line(b"c", 5) + b"\r\n\r\n#x\r\n" + vcf_line(b"c", 9)
    data = T.bgzf_text(u, block_u=1 << 16)
    recs = TU.records(data)
    first = len(b"\xef\xbb\xbf#h\r\n")
    n = len(vcf_line(b"c", 5))
    assert [(k, vs, ve) for k, vs, ve, *_ in recs] == [
        (1, first, first + n + 2), (4, first + n + 2 + 2 + 4, (len(data) - len(B.EOF_BLOCK)) << 16)]
    assert TU.lines(b"\xef\xbb\xbfa\nb")[0][:2] == [0, 3]


# ------------------------------------------------------------------ GPU
gpu = pytest.mark.gpu


def text_lines(c):
    b = c.text_read(True)
    return {k: b[k].copy() for k in ("line_offset", "line_len", "data", "part_offset", "hash")}


@gpu
@pytest.mark.parametrize("name", ["hiseq", "test", "syn300", "syn700", "syn8000", "crlf", "gaps",
                                  "no_last_terminator", "no_eof_block", "header_only", "wide",
                                  "levels", "one_line", "eof_only"])
def test_gpu_tbi_equals_restatement(name):
    from disq_amd import _lib
    data, want = inputs()[name], restated(name)
    if name == "header_only":
        assert struct.unpack_from("<i", want, 4)[0] == 0 and len(want) == 36
    if name == "test":
        assert TU.parse_tbi(want)["names"] == [b"20"] and len(TU.records(data)) == 5
    if name == "wide":
        assert min(len(l) for l in data_lines(data)) >= 3000
    with _lib.Context(split_size=0, verify_crc=True) as c:
        c.text_open_bytes(data)
        got = c.text_write_tbi()
        assert c.tbi_ms >= 0
        assert got == want
        assert c.text_write_tbi() == want
        after = text_lines(c)
    with _lib.Context(split_size=0, verify_crc=True) as c:
        c.text_open_bytes(data)
        fresh = text_lines(c)
        assert c.text_write_tbi() == want   # and after a read
    for k in fresh:
        assert np.array_equal(after[k], fresh[k]), k
    with _lib.Context(split_size=30000, use_nio=True) as c:
        c.text_open_bytes(data)
        c.text_set_index(T.whole_file_tabix(["chr1"], len(data)))
        c.text_set_intervals([("chr1", 1, 2)])
        assert c.text_write_tbi() == want


@gpu
def test_gpu_tbi_two_trailing_empty_blocks():
    """The final pointer with two empty blocks behind the last line (what the input reaches:
    test_restatement_smallest_inputs).  The index only: the text run itself takes no empty block
    before the stream's last one, so the reads of test_gpu_tbi_equals_restatement do not apply."""
    from disq_amd import _lib
    with _lib.Context(split_size=0, verify_crc=True) as c:
        c.text_open_bytes(inputs()["two_eof_blocks"])
        assert c.text_write_tbi() == restated("two_eof_blocks")
        assert c.text_write_tbi() == restated("two_eof_blocks")


@gpu
def test_gpu_tbi_fixture_structure():
    from disq_amd import _lib
    with _lib.Context() as c:
        c.text_open_bytes(inputs()["hiseq"])
        got = TU.parse_tbi(c.text_write_tbi())
    assert strip_htslib(got) == strip_htslib(TU.parse_tbi(golden_bytes("HiSeq.10000.vcf.bgz.tbi")))


def assert_interval_parity(data, split, intervals, tbi):
    """tests/test_text_gpu.py's helper, the GPU side reading through the index it built itself and
    the oracle through `tbi`."""
    from disq_amd import _lib
    ot = O.OracleText(data)
    want = ot.read_partitions_intervals(split, intervals, tbi)
    with _lib.Context(split_size=split, verify_crc=True) as c:
        c.text_open_bytes(data)
        c.text_set_index(c.text_write_tbi())
        c.text_set_intervals(intervals)
        st = c.text_run()
        b = c.text_read()
    po = b["part_offset"]
    assert len(po) - 1 == len(want) == st.n_partitions
    for i, (_, (vs, vl)) in enumerate(want):
        lo, hi = int(po[i]), int(po[i + 1])
        assert np.array_equal(b["line_offset"][lo:hi], vs), i
        assert np.array_equal(b["line_len"][lo:hi], vl), i
    return b, want


@gpu
def test_gpu_tbi_end_to_end():
    d = inputs()["hiseq"]
    lines = data_lines(d)
    for intervals, nparts in HISEQ_INTERVALS:
        b, want = assert_interval_parity(d, SPLIT, intervals, golden_bytes("HiSeq.10000.vcf.bgz.tbi"))
        if nparts is not None:
            assert len(want) == nparts
        assert len(b["line_len"]) == len([l for l in lines if O.vcf_overlaps(l, intervals)])
    d = inputs()["syn700"]
    lines = data_lines(d)
    ivs = seeded_intervals()
    for intervals in [ivs, ivs[:1], ivs[-1:]]:
        b, want = assert_interval_parity(d, 6000, intervals, restated("syn700"))
        assert len(b["line_len"]) == len([l for l in lines if O.vcf_overlaps(l, intervals)])


@gpu
def test_gpu_tbi_errors():
    from disq_amd import _lib
    for name, (data, k) in error_inputs().items():
        with pytest.raises(ValueError) as want:
            TU.build_tbi(data)
        with _lib.Context() as c:
            c.text_open_bytes(data)
            with pytest.raises(_lib.DqError) as e:
                c.text_write_tbi()
            assert e.value.code == _lib.DQ_EFORMAT, name
            m, w = re.search(r"line (\d+)", str(e.value)), re.search(r"line (\d+)", str(want.value))
            assert m and w and int(m.group(1)) == int(w.group(1)) == k, (name, str(e.value))
            assert ("not sorted" in str(e.value)) == ("not sorted" in str(want.value)), name
            assert len(c.text_read(True)["line_len"]) == len(data_lines(data))   # still reads
    with _lib.Context() as c:
        with pytest.raises(_lib.DqError) as e:
            c.text_write_tbi()
        assert e.value.code == _lib.DQ_EINVAL
        c.open_bytes(golden_bytes("1.bam"))   # a BAM is no text file
        with pytest.raises(_lib.DqError) as e:
            c.text_write_tbi()
        assert e.value.code == _lib.DQ_EINVAL


@gpu
def test_gpu_tbi_storage(tmp_path):
    from disq_amd.storage import HtsjdkVariantsRddStorage, Interval, TabixIndexer
    src = os.path.join(GOLDEN, "HiSeq.10000.vcf.bgz")
    st = HtsjdkVariantsRddStorage.makeDefault().splitSize(SPLIT)
    rdd = st.read(src)
    v = rdd.getVariants()
    assert v.getNumPartitions() == 4 and v.count() == 9965
    out = str(tmp_path / "out.vcf.bgz")
    assert st.write(rdd, out, tabix=True) == out
    assert sorted(os.listdir(tmp_path)) == ["out.vcf.bgz", "out.vcf.bgz.tbi"]
    written = open(out, "rb").read()
    text = b"".join(l + b"\n" for l in rdd.getHeader() + v.collect())
    assert gzip.decompress(written) == text
    assert written.endswith(B.EOF_BLOCK)
    assert T.split_lines(text) == T.split_lines(gzip.decompress(golden_bytes("HiSeq.10000.vcf.bgz")))
    # the sidecar is a BGZF file of the index of the written file, and the reader takes it
    tbi = open(out + ".tbi", "rb").read()
    assert tbi.endswith(B.EOF_BLOCK) and B.inflate_all(tbi) == TU.build_tbi(written)
    got = st.read(out, [Interval("chr1", 2700000, 2800000)]).getVariants()
    assert got.count() == 243
    # createIndex on a copy without the sidecar reproduces it
    cp = str(tmp_path / "copy.vcf.bgz")
    shutil.copy(out, cp)
    assert TabixIndexer.createIndex(cp) == cp + ".tbi"
    assert open(cp + ".tbi", "rb").read() == tbi
    other = str(tmp_path / "elsewhere.tbi")
    assert TabixIndexer.createIndex(cp, other) == other and open(other, "rb").read() == tbi
    # the defaults write one file with the same bytes; the parts directory is gone afterwards
    d2 = tmp_path / "plain"
    d2.mkdir()
    out2 = str(d2 / "out.vcf.bgz")
    st.write(rdd, out2, str(tmp_path / "parts"))
    assert os.listdir(d2) == ["out.vcf.bgz"] and open(out2, "rb").read() == written
    assert not os.path.exists(tmp_path / "parts")
    # an uncompressed path takes the plain text; no index without compression, no other extension
    x = str(d2 / "x.vcf")
    st.write(rdd, x)
    assert open(x, "rb").read() == text
    with pytest.raises(ValueError):
        st.write(rdd, str(d2 / "y.vcf"), tabix=True)
    with pytest.raises(ValueError):
        st.write(rdd, str(d2 / "x.txt"))
    assert sorted(os.listdir(d2)) == ["out.vcf.bgz", "x.vcf"]
