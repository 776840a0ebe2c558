"""The per-cell genotype rules of disq_amd/csrc/dq_vcf_gt_core.h -- the functions the genotype
kernels call -- run on the CPU through tools/vcf_gt_check.cpp and compared with the oracle
tests/vcfgtutil.py, cell for cell and error for error: both fixtures, the table of bad lines and the
synthetic lines of the GPU parity cases."""
import gzip
import os
import re
import subprocess

import pytest

import vcfcases as K
import vcfgtcases as GK
import vcfgtutil as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the synthetic files of tests/test_vcf_gt_gpu.py: (S, largest ploidy)
_GT = open(os.path.join(ROOT, "disq_amd", "csrc", "dq_vcf_gt.hip")).read()
SYNTH = GK.synth_cases(int(re.search(r"GT_WAVE_S = (\d+);", _GT).group(1)),
                       int(re.search(r"GT_OFFS = (\d+);", _GT).group(1)))


def _build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.run(["g++", "-g", "-std=c++17", "-pthread", *flags, "-I", os.path.join(ROOT, "disq_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tools", "vcf_gt_check.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("vcfgt"), "vcf_gt_check", ["-O1"])


def run_lines(tool, tmp_path, text):
    """(names, [(line index, cells or None, (class, sample) or None)]); a cell = (flags, ploidy, gq,
    host, dp, cell_off, alleles)."""
    src, dst = tmp_path / "in.vcf", tmp_path / "out.txt"
    src.write_bytes(text)
    subprocess.run([tool, "lines", str(src), str(dst)], check=True)
    rows = dst.read_bytes().split(b"\n")[:-1]
    S = int(rows[0].split()[1])
    names = [r[2:] for r in rows[1:1 + S]]
    out = []
    for r in rows[1 + S:]:
        f = r.split(b" ")
        if f[1] == b"E":
            out.append((int(f[0]), None, (f[2].decode(), None if f[3] == b"-1" else int(f[3]))))
            continue
        assert f[1] == b"G"
        P, cells = int(f[2]), []
        for c in f[3:]:
            v = c.split(b",")
            al = [int(x) for x in v[6].split(b"/")]
            assert len(al) == P
            cells.append(tuple(int(x) for x in v[:6]) + (al,))
        out.append((int(f[0]), cells, None))
    return names, out


def oracle_rows(text):
    names, rows = G.decode_text(text)
    out = []
    for k, cells, e in rows:
        if e is not None:
            out.append((k, None, (e.what, e.sample)))
            continue
        P = max([1] + [len(c["alleles"]) for c in cells])
        out.append((k, [(c["flags"], len(c["alleles"]), c["gq"], int(c["gq_host"]), c["dp"], c["cell_off"],
                         c["alleles"] + [-2] * (P - len(c["alleles"]))) for c in cells], None))
    return names, out


def assert_same(tool, tmp_path, text):
    got, want = run_lines(tool, tmp_path, text), oracle_rows(text)
    assert got[0] == want[0]
    assert len(got[1]) == len(want[1])
    for g, w in zip(got[1], want[1]):
        assert g == w
    return got[1]


def table_text():
    return K.HEADER + b"".join(l + b"\n" for l in GK.GOOD) + b"".join(l + b"\r\n" for l, _, _ in GK.BAD + GK.ORDER)


def test_fixtures(tool, tmp_path, golden):
    rows = assert_same(tool, tmp_path, open(os.path.join(golden, "test.vcf"), "rb").read())
    assert len(rows) == 5 and all(e is None and len(c) == 3 for _, c, e in rows)
    text = gzip.decompress(open(os.path.join(golden, "HiSeq.10000.vcf.bgz"), "rb").read())
    rows = assert_same(tool, tmp_path, text)
    assert len(rows) == 9965 and all(e is None and c[0][3] == 0 for _, c, e in rows)
    assert sum(c[0][2] for _, c, _ in rows) == 907868 and sum(c[0][4] for _, c, _ in rows) == 611423


def test_every_case_of_the_table(tool, tmp_path):
    rows = assert_same(tool, tmp_path, table_text())
    assert [e for _, _, e in rows] == [None] * len(GK.GOOD) + [(w, s) for _, w, s in GK.BAD + GK.ORDER]
    assert sum(c[3] for _, cells, e in rows if e is None for c in cells) == 8      # the host's GQ texts
    # a sites-only file: no cells; a last line without a terminator
    rows = assert_same(tool, tmp_path, K.SITES_HEADER + b"\n".join(K.sites_good_lines()))
    assert [c for _, c, _ in rows] == [[]] * 3


@pytest.mark.parametrize("S,maxp", SYNTH)
def test_synthetic_lines(tool, tmp_path, S, maxp):
    rows = assert_same(tool, tmp_path, GK.synth_file(S, maxp))
    assert len(rows) == 12 and all(e is None and len(c) == S for _, c, e in rows)
    assert max(c[1] for _, cells, _ in rows for c in cells) == maxp


def test_runs_clean_under_the_sanitizers(tmp_path, golden):
    """The same program as a stand-alone binary under AddressSanitizer and UBSan, over the fixtures,
    the table and the synthetic lines: every line sits in a heap buffer of exactly its length."""
    exe = _build(tmp_path, "vcf_gt_check_san", ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    texts = [open(os.path.join(golden, "test.vcf"), "rb").read(),
             gzip.decompress(open(os.path.join(golden, "HiSeq.10000.vcf.bgz"), "rb").read()),
             table_text()] + [GK.synth_file(S, p) for S, p in SYNTH]
    for text in texts:
        assert run_lines(exe, tmp_path, text) == oracle_rows(text)
    out = subprocess.run([exe, "bench", str(tmp_path / "in.vcf"), "4", "1", str(tmp_path / "m.bin")],
                         check=True, capture_output=True).stdout
    assert out.startswith(b"{") and out.rstrip().endswith(b"}")
