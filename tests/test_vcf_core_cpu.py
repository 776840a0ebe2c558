"""The per-line VCF rules of disq_amd/csrc/dq_vcf_core.h -- the functions the VCF kernels call -- run
on the CPU through tools/vcf_core_check.cpp and compared with the oracle tests/vcfutil.py: fields
column by column, error classes by name, QUAL values bit for bit (an undecided text is allowed, a
wrong value is not)."""
import gzip
import os
import struct
import subprocess

import pytest

import floatcases as F
import vcfcases as K
import vcfutil as V
from floatref import BINARY64, exact_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.run(["g++", "-g", "-std=c++17", "-pthread", *flags, "-I", os.path.join(ROOT, "disq_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tools", "vcf_core_check.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("vcfcore"), "vcf_core_check", ["-O1"])


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def run_lines(tool, tmp_path, text):
    """((G, n contigs), [(line index, row or None, error class or None)]); row = the S line's ints."""
    src, dst = tmp_path / "in.vcf", tmp_path / "out.txt"
    src.write_bytes(text)
    subprocess.run([tool, "lines", str(src), str(dst)], check=True)
    rows = dst.read_text().split("\n")[:-1]
    h = rows[0].split()
    out = []
    for r in rows[1:]:
        f = r.split()
        if f[1] == "E":
            out.append((int(f[0]), None, f[2]))
        else:
            out.append((int(f[0]), [int(f[2]), int(f[3]), int(f[4]), int(f[5]), int(f[6], 16), int(f[7])] +
                        [int(x) for x in f[8:]], None))
    return (int(h[1]), int(h[2])), out


def oracle_rows(text):
    G, contigs = V.vcf_header(text)
    out = []
    for k, f, e in V.decode_text(text):
        if e is not None:
            out.append((k, None, e))
            continue
        q = bits(f["qual"]) if f["qual"] is not None else 0
        out.append((k, [f["contig"], f["pos"], f["end"], f["flags"], q, int(f["qual_host"])] + f["col_end"] +
                    [f["n_alt"], f["n_filter"], f["n_info"], f["n_sample_cols"]], None))
    return (int(G), len(contigs)), out


def assert_same(tool, tmp_path, text):
    got, want = run_lines(tool, tmp_path, text), oracle_rows(text)
    assert got[0] == want[0]
    assert len(got[1]) == len(want[1])
    for g, w in zip(got[1], want[1]):
        assert g == w
    return got[1]


def test_fixtures(tool, tmp_path, golden):
    rows = assert_same(tool, tmp_path, open(os.path.join(golden, "test.vcf"), "rb").read())
    assert len(rows) == 5 and all(e is None for _, _, e in rows)
    text = gzip.decompress(open(os.path.join(golden, "HiSeq.10000.vcf.bgz"), "rb").read())
    rows = assert_same(tool, tmp_path, text)
    assert len(rows) == 9965 and all(e is None and r[5] == 0 for _, r, e in rows)


def test_every_case_of_the_table(tool, tmp_path):
    good = K.good_lines()
    rows = assert_same(tool, tmp_path, K.HEADER + b"".join(l + b"\n" for l in good))
    assert [e for _, _, e in rows] == [None] * len(good)
    bad = K.bad_lines() + K.ORDER
    # CR LF terminators (an empty line between CR and LF would be a line of its own: none is)
    rows = assert_same(tool, tmp_path, K.HEADER + b"".join(l + b"\r\n" for l, _ in bad))
    assert [e for _, _, e in rows] == [w for _, w in bad]
    rows = assert_same(tool, tmp_path, K.SITES_HEADER + b"".join(l + b"\n" for l in K.sites_good_lines()) +
                       b"".join(l + b"\n" for l, _ in K.sites_bad_lines()))
    assert [e for _, _, e in rows] == [None] * 3 + [w for _, w in K.sites_bad_lines()]
    # a last line without a terminator, and a BOM before the header
    assert_same(tool, tmp_path, b"\xef\xbb\xbf" + K.HEADER + good[1] + b"\n" + good[2])


def test_header_without_chrom_line(tool, tmp_path):
    src, dst = tmp_path / "in.vcf", tmp_path / "out.txt"
    src.write_bytes(b"##fileformat=VCFv4.2\n" + K.line() + b"\n")
    assert subprocess.run([tool, "lines", str(src), str(dst)]).returncode == 3
    assert dst.read_text() == "H nochrom\n"


def test_quals_bit_for_bit(tool, tmp_path):
    """Against the exact reference tests/floatref.py."""
    texts = F.qual_texts()
    edge = F.qual_edge_texts()
    assert len(texts) == 60000 + len(edge) and texts[60000:] == edge and len(edge) == 1200
    extra, bad = F.QUAL_EXTRA, F.QUAL_BAD
    texts = texts + extra + bad
    src, dst = tmp_path / "q.txt", tmp_path / "q.out"
    src.write_bytes(b"".join(t.encode() + b"\n" for t in texts))
    subprocess.run([tool, "quals", str(src), str(dst)], check=True)
    got = dst.read_text().split("\n")[:-1]
    assert len(got) == len(texts)
    decided = 0
    for i, (t, g) in enumerate(zip(texts, got)):
        ok = V.QUAL_RE.match(t.encode()) is not None
        assert (g == "BAD") == (not ok), (t, g)
        if not ok:
            continue
        assert (g == "UNDECIDED") == (not V.qual_fast_path(t.encode())), (t, g)
        if g != "UNDECIDED":                       # never a wrong value
            assert g == "OK %016x" % exact_bits(t.encode(), BINARY64), (t, g)
            decided += 1
        if i < 60000 and i % 3 == 0 and F.sig_digits(t) <= 15:
            assert g != "UNDECIDED", t           # no %.2f text of up to 15 digits goes to the host
    assert all(g == "BAD" for g in got[-len(bad):])
    assert decided > 30000
    # the 15-digit mantissas: decided at the decimal exponents +-21 and +-22, the host's at +-23
    assert [g != "UNDECIDED" for g in got[60000:61200]] == [i // 200 < 4 for i in range(1200)]


def test_runs_clean_under_the_sanitizers(tmp_path, golden):
    """The same program as a stand-alone binary under AddressSanitizer and UBSan, over the fixtures
    and the table: every line sits in a heap buffer of exactly its length."""
    exe = _build(tmp_path, "vcf_core_check_san", ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    texts = [open(os.path.join(golden, "test.vcf"), "rb").read(),
             gzip.decompress(open(os.path.join(golden, "HiSeq.10000.vcf.bgz"), "rb").read()),
             K.HEADER + b"".join(l + b"\n" for l in K.good_lines()) +
             b"".join(l + b"\n" for l, _ in K.bad_lines() + K.ORDER),
             K.SITES_HEADER + b"".join(l + b"\n" for l, _ in K.sites_bad_lines())]
    for text in texts:
        got, want = run_lines(exe, tmp_path, text), oracle_rows(text)
        assert got == want
    src, dst = tmp_path / "q.txt", tmp_path / "q.out"
    src.write_bytes(b"".join(t.encode() + b"\n" for t in F.qual_texts()[:3000] + ["", ".", "1e", "1e400", ".5"]))
    subprocess.run([exe, "quals", str(src), str(dst)], check=True)
    out = subprocess.run([exe, "bench", str(tmp_path / "in.vcf"), "4", "1"], check=True, capture_output=True).stdout
    assert out.startswith(b"{") and out.rstrip().endswith(b"}")
