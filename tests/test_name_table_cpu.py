"""The name table of disq_amd/csrc/dq_text_core.h -- what resolves @SQ names, ##contig IDs and INFO
keys in the kernels -- run on the CPU through tools/name_table_check.cpp: the empty table, the empty
name, equal names, prefixes, the collision scan behind a forged hash array and 1,000 names against a
dict; then the same program under AddressSanitizer and UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "disq_amd", "csrc")
MANY = [b"ctg%d_%x" % (i, i * 2654435761 % 4093) for i in range(1000)]


def _build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.run(["g++", "-g", "-std=c++17", *flags, "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tools", "name_table_check.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("nametable"), "name_table_check", ["-O1"])


def lookup(tool, tmp_path, names, queries):
    for f, rows in (("names", names), ("queries", queries)):
        (tmp_path / f).write_bytes(b"%d\n" % len(rows) + b"".join(r + b"\n" for r in rows))
    out = subprocess.run([tool, "lookup", str(tmp_path / "names"), str(tmp_path / "queries")], check=True,
                         stdout=subprocess.PIPE).stdout
    return [int(x) for x in out.split()]


def forged(tool, a, b):
    out = subprocess.run([tool, "forged", a, b], check=True, stdout=subprocess.PIPE).stdout
    return [int(x) for x in out.split()]


def first_index(names):
    d = {}
    for i, n in enumerate(names):
        d.setdefault(n, i)
    return d


def check_all(tool, tmp_path):
    assert lookup(tool, tmp_path, [], [b"", b"chr1"]) == [-1, -1]
    # a zero-length name: found when listed, -1 when not
    assert lookup(tool, tmp_path, [b"chr1", b"", b"chr2"], [b"", b"chr2"]) == [1, 2]
    assert lookup(tool, tmp_path, [b"chr1", b"chr2"], [b""]) == [-1]
    # equal names resolve to the first
    assert lookup(tool, tmp_path, [b"chr1", b"chr2", b"chr1"], [b"chr1", b"chr2"]) == [0, 1]
    # a proper prefix or an extension of a listed name is no match
    assert lookup(tool, tmp_path, [b"chr10", b"chrX"], [b"chr1", b"chr", b"chr100", b"chrXY", b"chr10"]) == \
        [-1, -1, -1, -1, 0]
    # both hash entries forged to the second name's hash: the byte compare walks past the first entry
    assert forged(tool, "chr1", "chr2") == [1, -1]
    assert forged(tool, "scaffold_12", "x") == [1, -1]
    assert len(set(MANY)) == len(MANY)
    want = first_index(MANY)
    queries = MANY + [n + b"_" for n in MANY[:50]] + [n[:-1] for n in MANY[:50]]
    assert lookup(tool, tmp_path, MANY, queries) == [want.get(q, -1) for q in queries]


def test_name_table(tool, tmp_path):
    check_all(tool, tmp_path)


def test_runs_clean_under_the_sanitizers(tmp_path):
    exe = _build(tmp_path, "name_table_check_san", ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    check_all(exe, tmp_path)
