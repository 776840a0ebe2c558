"""The INFO rules of disq_amd/csrc/dq_vcf_info_core.h -- the functions the INFO kernels call -- run
on the CPU through tools/vcf_info_check.cpp and compared with the oracle tests/vcfinfoutil.py, cell
for cell and error for error: both fixtures, the tables of good and bad columns and the synthetic
lines of the GPU parity cases; then the same program under AddressSanitizer and UBSan."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import vcfinfocases as C
import vcfinfoutil as U
from test_vcf_info_rules import HISEQ_KEYS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "disq_amd", "csrc")
_INFO = open(os.path.join(CSRC, "dq_vcf_info.hip")).read()
INFO_WAVE = int(re.search(r"INFO_WAVE = (\d+);", _INFO).group(1))
INFO_WSLOT = int(re.search(r"INFO_WSLOT = (\d+);", _INFO).group(1))
VCF_LONG = int(re.search(r"VCF_LONG = (\d+);", open(os.path.join(CSRC, "dq_vcf.hip")).read()).group(1))
TEST_KEYS = [b"NS", b"DP", b"AF", b"AA", b"DB", b"H2"]
OVERRIDES = [(b"AF", U.STRING), (b"NOHDR", U.INTEGER), (b"DB", U.INTEGER), b"DP", (b"MQ", U.FLOAT), (b"AA", U.FLAG)]


def synth_texts():
    return [C.synth_file(w, INFO_WAVE, VCF_LONG, INFO_WSLOT, so) for w, so in C.SYNTH]


def _build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.run(["g++", "-g", "-std=c++17", "-pthread", *flags, "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tools", "vcf_info_check.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("vcfinfo"), "vcf_info_check", ["-O1"])


def key_arg(keys):
    return b",".join(k if isinstance(k, bytes) else k[0] + b":%d" % k[1] for k in keys)


def run_lines(tool, tmp_path, text, keys):
    """([(id, type, header Flag)], [(line index, cells or None, failing key or None)]); a cell =
    (flags, n_values, val_off, val_len, host, values)."""
    src, dst = tmp_path / "in.vcf", tmp_path / "out.txt"
    src.write_bytes(text)
    subprocess.run([tool, "lines", str(src), key_arg(keys), str(dst)], check=True)
    rows = dst.read_bytes().split(b"\n")[:-1]
    rk, out = [], []
    for r in rows:
        f = r.split(b" ")
        if f[0] == b"K":
            rk.append((f[2], int(f[3]), f[4] == b"1"))
        elif f[1] == b"E":
            out.append((int(f[0]), None, int(f[2])))
        else:
            assert f[1] == b"C" and len(f) == 2 + len(rk)
            cells = []
            for q, c in enumerate(f[2:]):
                v = c.split(b",")
                vals = [] if v[5] == b"-" else [int(x, 16 if rk[q][1] == U.FLOAT else 10) for x in v[5].split(b"/")]
                cells.append(tuple(int(x) for x in v[:5]) + (vals,))
            out.append((int(f[0]), cells, None))
    return rk, out


def oracle_rows(text, keys):
    rk, rows = U.decode_text(text, keys)
    return rk, [(k, None if c is None else [(x["flags"], x["n_values"], x["val_off"], x["val_len"], x["host"],
                                             [v & 0xffffffffffffffff if rk[q][1] == U.FLOAT else v
                                              for v in x["values"]]) for q, x in enumerate(c)], e)
                for k, c, e in rows]


def assert_same(tool, tmp_path, text, keys):
    got, want = run_lines(tool, tmp_path, text, keys), oracle_rows(text, keys)
    assert got[0] == want[0] and len(got[1]) == len(want[1])
    for g, w in zip(got[1], want[1]):
        assert g == w
    return got[1]


def table_text():
    return C.good_text() + b"".join(C.iline(i) + b"\r\n" for i, _ in C.BAD + C.ORDER)


def cases(golden):
    return [(open(os.path.join(golden, "test.vcf"), "rb").read(), TEST_KEYS),
            (gzip.decompress(open(os.path.join(golden, "HiSeq.10000.vcf.bgz"), "rb").read()), HISEQ_KEYS),
            (table_text(), C.KEYS), (table_text(), OVERRIDES), (table_text(), [b"AF"]),
            (C.good_text(C.SITES_HEADER).replace(C.K.GT, b""), C.KEYS[::-1] + [b"K%d" % i for i in range(52)])] + \
        [(t, C.KEYS) for t in synth_texts()]


def test_fixtures(tool, tmp_path, golden):
    (t1, k1), (t2, k2) = cases(golden)[:2]
    rows = assert_same(tool, tmp_path, t1, k1)
    assert len(rows) == 5 and rows[2][1][2][5] == [0x3fd54fdf3b645a1d, 0x3fe55810624dd2f2]      # 0.333, 0.667
    rows = assert_same(tool, tmp_path, t2, k2)
    assert len(rows) == 9965 and all(e is None for _, _, e in rows)
    assert sum(c[4][5][0] for _, c, _ in rows) == 897363                                          # DP


def test_every_case_of_the_table(tool, tmp_path, golden):
    rows = assert_same(tool, tmp_path, table_text(), C.KEYS)
    assert [e for _, _, e in rows] == [None] * len(C.GOOD) + [C.KEYS.index(k) for _, k in C.BAD + C.ORDER]
    assert sum(c[4] for _, cells, e in rows if e is None for c in cells) == 4      # the host's Float texts
    for text, keys in cases(golden)[3:6]:
        assert_same(tool, tmp_path, text, keys)


def test_refused_key_lists(tool, tmp_path):
    src, dst = tmp_path / "in.vcf", tmp_path / "out.txt"
    src.write_bytes(C.good_text())
    for arg in (b"DP,DP", b"DP,,AF", b"A=B", b"A B", b"DP:7", b",".join(b"K%d" % i for i in range(65))):
        subprocess.run([tool, "lines", str(src), arg, str(dst)], check=True)
        assert dst.read_bytes().startswith(b"K bad ")


def test_synthetic_lines(tool, tmp_path):
    for (w, so), text in zip(C.SYNTH, synth_texts()):
        rows = assert_same(tool, tmp_path, text, C.KEYS)
        assert all(e is None for _, _, e in rows)
        lens = [len(l.split(b"\t")[7]) for l in text.split(b"\n") if l and not l.startswith(b"#")]
        assert {INFO_WAVE, INFO_WAVE + 1, INFO_WSLOT, INFO_WSLOT + 1} <= set(lens) and min(lens) < 100
        assert max(c[1] for _, cells, _ in rows for c in cells) == max(w, 2)


def test_bench_mode_matches_the_oracle(tool, tmp_path):
    text = synth_texts()[2]
    (tmp_path / "in.vcf").write_bytes(text)
    out = subprocess.run([tool, "bench", str(tmp_path / "in.vcf"), key_arg(C.KEYS), "3", "2", str(tmp_path / "m.bin")],
                         check=True, capture_output=True).stdout
    assert out.startswith(b"{") and out.rstrip().endswith(b"}")
    rk, rows = U.decode_text(text, C.KEYS)
    want, nhost = U.want_arrays([c for _, c, _ in rows], rk)
    got = read_bench_bin(str(tmp_path / "m.bin"))
    assert got["n_float_host"] == nhost
    for k, w in want.items():
        assert np.array_equal(got[k], w), k


def read_bench_bin(path):
    b = open(path, "rb").read()
    n, K, ni, nf, nhost = np.frombuffer(b, np.int64, 5)
    at = [40]

    def take(dt, count, shape=None):
        a = np.frombuffer(b, dt, count, at[0])
        at[0] += a.nbytes
        return a.reshape(shape) if shape else a
    g = {"key_type": take(np.int32, K), "key_width": take(np.int32, K), "key_base": take(np.int64, K),
         "flags": take(np.uint8, K * n, (K, n)), "n_values": take(np.int32, K * n, (K, n)),
         "val_off": take(np.int32, K * n, (K, n)), "val_len": take(np.int32, K * n, (K, n)),
         "ival": take(np.int32, ni), "fval": take(np.uint64, nf)}
    assert at[0] == len(b)
    g["n_float_host"] = int(nhost)
    return g


def test_runs_clean_under_the_sanitizers(tmp_path, golden):
    """The same program as a stand-alone binary under AddressSanitizer and UBSan over the same
    inputs: every INFO column sits in a heap buffer of exactly its length, every value row has
    exactly its size."""
    exe = _build(tmp_path, "vcf_info_check_san", ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    for text, keys in cases(golden):
        assert run_lines(exe, tmp_path, text, keys) == oracle_rows(text, keys)
    out = subprocess.run([exe, "bench", str(tmp_path / "in.vcf"), key_arg(C.KEYS), "4", "1", str(tmp_path / "m.bin")],
                         check=True, capture_output=True).stdout
    assert out.startswith(b"{") and out.rstrip().endswith(b"}")
