"""The per-record rules of disq_amd/csrc/dq_samw_core.h -- the functions the SAM writer's kernels
call -- run on the CPU through tools/sam_write_check.cpp and compared with the oracle
tests/samwriteutil.py byte for byte: lines, error classes by name, Float.toString texts."""
import os
import struct
import subprocess

import pytest

import bamutil as B
import samcases as K
import samutil as S
import samwriteutil as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("samw") / "sam_write_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-I", os.path.join(ROOT, "disq_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tools", "sam_write_check.cpp")], check=True)
    return exe


def run_lines(tool, tmp_path, recs, refs):
    """[line bytes (LF included) or "what"] per record."""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    d = struct.pack("<I", len(refs)) + b"".join(struct.pack("<I", len(n)) + n for n in refs)
    d += struct.pack("<I", len(recs)) + b"".join(struct.pack("<I", len(r)) + r for r in recs)
    src.write_bytes(d)
    subprocess.run([tool, "lines", str(src), str(dst)], check=True)
    d, p, out = dst.read_bytes(), 0, []
    while p < len(d):
        kind, n = struct.unpack_from("<II", d, p)
        body = d[p + 8:p + 8 + n]
        out.append(body if kind == 0 else body.decode("latin-1"))
        p += 8 + n
    assert len(out) == len(recs)
    return out


def oracle(recs, refs):
    out = []
    for r in recs:
        try:
            out.append(W.record_to_sam_line(r, refs) + b"\n")
        except W.SamWriteError as e:
            out.append(e.what)
    return out


def sam_text_records(text):
    names = S.sam_header_to_bam(text)[1]
    return [r for _, _, r in S.sam_records(text, names)], [n.encode() for n in names]


def test_golden_sam(tool, tmp_path):
    recs, refs = sam_text_records(open(os.path.join(GOLDEN, "test.sam"), "rb").read())
    assert run_lines(tool, tmp_path, recs, refs) == oracle(recs, refs)


def test_1bam(tool, tmp_path):
    u = B.inflate_all(open(os.path.join(GOLDEN, "1.bam"), "rb").read())
    text = S.bam_to_sam_text(u)
    recs, refs = sam_text_records(text)
    got = run_lines(tool, tmp_path, recs, refs)
    assert len(got) == 4917 and got == oracle(recs, refs)
    assert b"".join(got) == b"".join(l + b"\n" for _, l in S.text_lines(text) if not l.startswith(b"@"))


def test_rule_lines(tool, tmp_path):
    recs, refs = sam_text_records(K.HEADER + b"".join(l + b"\n" for l in K.good_lines()))
    assert len(recs) == 76
    assert run_lines(tool, tmp_path, recs, refs) == oracle(recs, refs)


def test_trim_cases(tool, tmp_path):
    recs = W.trim_cases()
    got = run_lines(tool, tmp_path, recs, W.REFS)
    assert got == oracle(recs, W.REFS)
    assert got[0].endswith(b"\tXZ:Z:abc\n") and got[1].endswith(b"\tXA:A:\n") and got[2].startswith(b"name\t")


def test_error_classes_and_order(tool, tmp_path):
    cases = W.error_cases()
    recs = [r for r, _ in cases]
    got = run_lines(tool, tmp_path, recs, W.REFS)
    assert got == [w for _, w in cases] == oracle(recs, W.REFS)
    # a record that does not fill its slot in the chain, or overruns it
    r = W.make_record()
    assert run_lines(tool, tmp_path, [r + b"\0", r[:-1]], W.REFS) == ["fields", "fields"]


def test_floats(tool, tmp_path):
    bits = W.float_set(200000)
    src, dst = tmp_path / "f.txt", tmp_path / "o.txt"
    src.write_text("".join("%08x\n" % b for b in bits))
    subprocess.run([tool, "floats", str(src), str(dst)], check=True)
    got = dst.read_bytes().split(b"\n")[:-1]
    assert len(got) == len(bits)
    bad = [(hex(b), g) for b, g in zip(bits, got) if g != W.float_text(b)]
    assert not bad, bad[:10]
    want = dict(W.FLOAT_PAIRS)
    assert all(g == want[b] for b, g in zip(bits[:len(want)], got))


def test_float_arrays_in_records(tool, tmp_path):
    edges = W.binade_edges()
    tags = b"XBBf" + struct.pack("<i", len(edges)) + struct.pack("<%dI" % len(edges), *edges)
    recs = [W.make_record(tags=tags)] + [W.make_record(tags=b"XFf" + struct.pack("<I", b)) for b in edges[:200]]
    assert run_lines(tool, tmp_path, recs, W.REFS) == oracle(recs, W.REFS)
