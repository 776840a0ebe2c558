"""The per-line SAM rules of disq_amd/csrc/dq_sam_core.h -- the functions the SAM kernels call -- run
on the CPU through tools/sam_core_check.cpp and compared with the oracle tests/samutil.py: records
byte for byte, error classes by name, floats bit for bit (an undecided float is allowed, a wrong
one is not)."""
import os
import struct
import subprocess
import sys

import pytest

import bamutil as B
import floatcases as F
import samcases as K
import samutil as S
from floatref import exact_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("samcore") / "sam_core_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-I", os.path.join(ROOT, "disq_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tools", "sam_core_check.cpp")], check=True)
    return exe


def run_records(tool, tmp_path, text):
    """(header bytes, [(line index, record bytes or None, error class or None)])."""
    src, dst = tmp_path / "in.sam", tmp_path / "out.bin"
    src.write_bytes(text)
    subprocess.run([tool, "records", str(src), str(dst)], check=True)
    d = dst.read_bytes()
    n = struct.unpack_from("<I", d, 0)[0]
    hdr, p, out = d[4:4 + n], 4 + n, []
    while p < len(d):
        k, kind, n = struct.unpack_from("<III", d, p)
        body = d[p + 12:p + 12 + n]
        out.append((k, body, None) if kind == 0 else (k, None, body.decode("latin-1")))
        p += 12 + n
    return hdr, out


def oracle(text):
    """The same per line that does not start with '@': the record or SamError.what."""
    names = S.sam_header_to_bam(text)[1]
    out = []
    for k, (_, v) in enumerate(S.text_lines(text)):
        if v.startswith(b"@"):
            continue
        try:
            out.append((k, S.sam_line_to_bam_record(v, names), None))
        except S.SamError as e:
            out.append((k, None, e.what))
    return out


def test_1bam_and_test_sam_records(tool, tmp_path, golden):
    u = B.inflate_all(open(os.path.join(golden, "1.bam"), "rb").read())
    text = S.bam_to_sam_text(u)
    hdr, got = run_records(tool, tmp_path, text)
    assert hdr == S.sam_header_to_bam(text)[0] == u[:B.header_len(u)]
    want = S.sam_records(text)
    assert len(want) == 4917
    assert [(k, r) for k, r, _ in got] == [(k, r) for k, _, r in want]
    text = open(os.path.join(golden, "test.sam"), "rb").read()
    hdr, got = run_records(tool, tmp_path, text)
    assert hdr == S.sam_header_to_bam(text)[0]
    assert [(k, r) for k, r, _ in got] == [(k, r) for k, _, r in S.sam_records(text)] and len(got) == 2


def test_one_line_per_rule(tool, tmp_path):
    lines = K.good_lines()
    text = K.HEADER + b"".join(l + b"\n" for l in lines)
    hdr, got = run_records(tool, tmp_path, text)
    assert hdr == S.sam_header_to_bam(text)[0]
    want = oracle(text)
    assert all(e is None for _, _, e in want) and len(want) == len(lines)
    for (k, r, e), (k2, r2, _) in zip(got, want):
        assert (k, e) == (k2, None) and r == r2, lines[k - 5]
    assert len(got) == len(want)
    # what the cases are there for
    first = got[0][1]
    assert struct.unpack_from("<H", first, 14)[0] == 4680 and struct.unpack_from("<H", first, 18)[0] == 4
    assert max(struct.unpack_from("<H", r, 16)[0] for _, r, _ in got) == 300
    assert max(r[12] for _, r, _ in got) == 255


def test_one_line_per_error_class(tool, tmp_path):
    cases = K.bad_lines()
    text = K.HEADER + b"".join(l + b"\n" for l, _ in cases)
    _, got = run_records(tool, tmp_path, text)
    want = oracle(text)
    assert [w for _, _, w in want] == [w for _, w in cases]  # the oracle agrees with the table
    assert [(k, e) for k, _, e in got] == [(k, e) for k, _, e in want]
    seen = {w.split()[0] for _, w in cases}
    assert seen == {"fields", "QNAME", "FLAG", "RNAME", "POS", "MAPQ", "CIGAR", "RNEXT", "PNEXT",
                    "TLEN", "SEQ", "QUAL", "tag"}


def test_floats_bit_for_bit(tool, tmp_path):
    """Against the exact reference tests/floatref.py: libc's strtof is what the library's own
    fix-up path calls."""
    texts, bad = F.sam_float_texts(), F.SAM_BAD
    ties = set(F.short_ties())
    assert texts[-len(bad):] == bad and len(ties) > 3000
    src, dst = tmp_path / "f.txt", tmp_path / "f.out"
    src.write_bytes(b"".join(t.encode() + b"\n" for t in texts))
    subprocess.run([tool, "floats", str(src), str(dst)], check=True)
    got = dst.read_text().split("\n")[:-1]
    assert len(got) == len(texts)
    short = undecided_short = 0
    for t, g in zip(texts, got):
        ok = S.FLOAT_RE.match(t.encode()) is not None
        assert (g == "BAD") == (not ok), (t, g)
        if not ok:
            continue
        if F.sig_digits(t) <= 17:
            short += 1
            undecided_short += g == "UNDECIDED"
        if t in ties:                              # the tie rule decides every one of them itself
            assert g != "UNDECIDED", t
        if g != "UNDECIDED":
            assert g == "OK %08x" % exact_bits(t.encode()), (t, g)
    assert all(g == "BAD" for g in got[-len(bad):])
    assert got[texts.index("7.038531e-26")] == "OK 15ae43fd"
    assert short > 60000 and undecided_short <= short // 100, (undecided_short, short)


def test_power_table_is_the_generators():
    """dq_sam_pow5.h is what tools/gen_sam_pow5.py computes with exact integers."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_sam_pow5.py")],
                         check=True, capture_output=True).stdout
    assert out == open(os.path.join(ROOT, "disq_amd", "csrc", "dq_sam_pow5.h"), "rb").read()
