"""The aux tag rules of disq_amd/csrc/dq_tags_core.h -- the functions the tag kernels call -- run on
the CPU through tools/tags_check.cpp and compared with the oracle tests/tagutil.py, cell for cell and
error for error: the tables of good and bad aux regions, the records of both BAM fixtures and the
synthetic records of the GPU cases; then the same program under AddressSanitizer and UBSan."""
import gzip
import io
import os
import re
import struct
import subprocess

import pytest

import tagcases as C
import tagutil as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "disq_amd", "csrc")
_TAGS = open(os.path.join(CSRC, "dq_tags.hip")).read()
TAG_SLOT = int(re.search(r"TAG_SLOT = (\d+);", _TAGS).group(1))
FIXTURE_KEYS = [(b"NM", U.INT), (b"AS", U.INT), (b"RG", U.STRING), (b"MD", U.ANY), (b"XS", U.ANY), (b"MC", U.STRING),
                (b"OQ", U.STRING), (b"XT", U.ANY), (b"X0", U.INT), (b"SM", U.INT)]


def edge_lens():
    return [0, 4, 60, TAG_SLOT - 1, TAG_SLOT, TAG_SLOT + 1, 77, 3 * TAG_SLOT, 90]


def _build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.run(["g++", "-g", "-std=c++17", "-pthread", *flags, "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tools", "tags_check.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("tags"), "tags_check", ["-O1"])


def key_arg(keys):
    return b",".join(vid + b":%d" % ty for vid, ty in U.norm_keys(keys))


def run_records(tool, tmp_path, recs, keys):
    """[(row, cells or None, error text or None)]; a cell = (flags, vtype, subtype, val_off, val_len, val)."""
    src, dst = tmp_path / "in.bin", tmp_path / "out.txt"
    src.write_bytes(b"".join(recs))
    subprocess.run([tool, "records", str(src), key_arg(keys), str(dst)], check=True)
    out, nk = [], 0
    for r in dst.read_bytes().split(b"\n")[:-1]:
        f = r.split(b" ")
        if f[0] == b"K":
            nk += 1
        elif f[1] == b"E":
            out.append((int(f[0]), None, b" ".join(f[2:]).decode("latin-1")))
        else:
            assert f[1] == b"C" and len(f) == 2 + nk
            out.append((int(f[0]), [tuple(int(x) for x in c.split(b",")) for c in f[2:]], None))
    return out


def oracle_rows(recs, keys):
    out = []
    for k, r in enumerate(recs):
        try:
            c = U.decode_record(r, keys)
            out.append((k, [(x["flags"], x["vtype"], x["subtype"], x["val_off"], x["val_len"], x["val"]) for x in c],
                        None))
        except U.TagError as e:
            out.append((k, None, e.what))
    return out


def assert_same(tool, tmp_path, recs, keys):
    got, want = run_records(tool, tmp_path, recs, keys), oracle_rows(recs, keys)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
    return got


def bam_records(path):
    """Every record of a BAM file (the BGZF members are gzip members)."""
    u = gzip.GzipFile(fileobj=io.BytesIO(open(path, "rb").read())).read()
    p = 8 + struct.unpack_from("<i", u, 4)[0]
    n_ref = struct.unpack_from("<i", u, p)[0]
    p += 4
    for _ in range(n_ref):
        p += 8 + struct.unpack_from("<i", u, p)[0]
    return U.split_records(u[p:])


def cases(golden):
    return [(bam_records(os.path.join(golden, "1.bam")), FIXTURE_KEYS),
            (bam_records(os.path.join(golden, "hiseq_part-r-00000.bam")), FIXTURE_KEYS),
            (C.table_records(), C.KEYS), (C.table_records(), C.KEYS1), (C.table_records(), C.KEYS64),
            (C.synth_records(300, edge_lens()), C.KEYS), (C.synth_records(40, edge_lens(), seed=3), C.KEYS64)]


def test_fixtures(tool, tmp_path, golden):
    (r1, k1), (r2, k2) = cases(golden)[:2]
    rows = assert_same(tool, tmp_path, r1, k1)
    assert len(rows) > 100 and all(e is None for _, _, e in rows)
    rows = assert_same(tool, tmp_path, r2, k2)
    assert len(rows) >= 837 and all(e is None for _, _, e in rows)
    assert any(c[0][0] for _, c, _ in rows)    # some record carries NM


def test_every_case_of_the_table(tool, tmp_path, golden):
    rows = assert_same(tool, tmp_path, C.table_records(), C.KEYS)
    want = [None] * len(C.GOOD) + [w for _, w in C.BAD + C.MISMATCH]
    assert [e for _, _, e in rows][:len(want)] == want
    assert [e for _, _, e in rows][-3:] == ["fields"] * 3
    for recs, keys in cases(golden)[3:5]:
        assert_same(tool, tmp_path, recs, keys)


def test_refused_key_lists(tool, tmp_path):
    src, dst = tmp_path / "in.bin", tmp_path / "out.txt"
    src.write_bytes(C.rec_of(C.NM))
    for arg in (b"NM,NM", b"NM,,AS", b"N", b"NMX", b"1M", b"N_", b"NM:7", b"NM:-1",
                b",".join(b"K%c" % c for c in b"0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZabc")):
        subprocess.run([tool, "records", str(src), arg, str(dst)], check=True)
        assert dst.read_bytes().startswith(b"K bad "), arg


def test_a_broken_chain_is_fields(tool, tmp_path):
    recs = [C.rec_of(C.NM), C.rec_of(C.AS, 1)]
    raw = b"".join(recs)
    rows = run_records(tool, tmp_path, [raw[:-1]], C.KEYS1)
    assert [(k, e) for k, _, e in rows] == [(0, None), (1, "fields")]


def test_synthetic_records(tool, tmp_path):
    recs = C.synth_records(300, edge_lens())
    rows = assert_same(tool, tmp_path, recs, C.KEYS)
    assert all(e is None for _, _, e in rows)
    lens = {U.aux_region(r)[1] - U.aux_region(r)[0] for r in recs}
    assert {0, TAG_SLOT - 1, TAG_SLOT, TAG_SLOT + 1, 3 * TAG_SLOT} <= lens


def test_bench_mode(tool, tmp_path):
    recs = C.synth_records(500, edge_lens())
    (tmp_path / "in.bin").write_bytes(b"".join(recs))
    out = [subprocess.run([tool, "bench", str(tmp_path / "in.bin"), key_arg(C.KEYS), str(t), "2"], check=True,
                          capture_output=True).stdout for t in (1, 3)]
    import json
    a, b = (json.loads(o) for o in out)
    assert a["records"] == 500 and a["bad_records"] == 0 and a["checksum"] == b["checksum"]
    assert a["aux_bytes"] == sum(U.aux_region(r)[1] - U.aux_region(r)[0] for r in recs)


def test_runs_clean_under_the_sanitizers(tmp_path, golden):
    """The same program as a stand-alone binary under AddressSanitizer and UBSan over the same
    inputs: every record and every aux region sits in a heap buffer of exactly its length."""
    exe = _build(tmp_path, "tags_check_san", ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    for recs, keys in cases(golden):
        assert run_records(exe, tmp_path, recs, keys) == oracle_rows(recs, keys)
    out = subprocess.run([exe, "bench", str(tmp_path / "in.bin"), key_arg(C.KEYS), "4", "1"], check=True,
                         capture_output=True).stdout
    assert out.startswith(b"{") and out.rstrip().endswith(b"}")
