"""The serial DEFLATE block-header decoder of disq_amd/csrc/dq_hdr_core.h -- what one lane of the
inflate kernels' header pre-pass runs -- on the CPU through tools/hdr_core_check.cpp: the code
lengths, the end position and the status of every header against tests/deflate_reader.py (zlib
streams) and against the tokens the header was written from (tests/hdrcases.py); then the same
program under AddressSanitizer and UBSan."""
import os
import random
import struct
import subprocess
import zlib

import pytest

import deflate_reader as R
import deflate_writer as W
import hdrcases as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "disq_amd", "csrc")


def _build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.run(["g++", "-g", "-std=c++17", *flags, "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tools", "hdr_core_check.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("hdrcore"), "hdr_core_check", ["-O1"])


def run(tool, tmp_path, cases):
    """cases: (bytes, header bit position, end bit position) -> (kind, status, nlen, ndist, bfinal,
    end, the 320 lengths) per case."""
    f = tmp_path / "cases.bin"
    f.write_bytes(b"".join(struct.pack("<III", len(b), pos, end) + b for b, pos, end in cases))
    out = subprocess.run([tool, str(f)], check=True, stdout=subprocess.PIPE).stdout.decode().split("\n")
    res = []
    for line in out[:len(cases)]:
        p = line.split()
        res.append(tuple(int(x) for x in p[:6]) + ([int(ch, 16) for ch in p[6]],))
    assert len(res) == len(cases)
    return res


def zlib_bodies():
    rng = random.Random(5)
    rnd = bytes(rng.randrange(256) for _ in range(20000))
    few = bytes(rng.choice(b"ACGTN#!I5") for _ in range(30000))
    rep = (b"the quick brown fox " * 40 + bytes(range(256))) * 12
    bam = b"".join(struct.pack("<iiiBBHHHiiii", 100 + i % 7, i % 3, 1000 * i, 9, 30, 4681, 1, 99, 36, 0,
                               1000 * i + 200, 300) + b"read%05d\0" % i + bytes([i & 255] * 40)
                   for i in range(400))
    for data in (rnd, few, rep, bam):
        for level in range(1, 10):
            c = zlib.compressobj(level, zlib.DEFLATED, -15)
            yield c.compress(data) + c.flush()


def check_all(tool, tmp_path):
    # ---- zlib streams, levels 1-9: every block's header against the reader
    cases, want = [], []
    kinds = set()
    for body in zlib_bodies():
        for blk in R.read(body):
            cases.append((body, blk.start, 8 * len(body)))
            kinds.add(blk.btype)
            if blk.btype == 2:
                want.append((H.DYN, 0, blk.hlit, blk.hdist, int(blk.final), blk.data,
                             H.lens320(blk.ll_lens, blk.d_lens)))
            else:
                want.append((H.NONE, 0))
    assert 2 in kinds and len(kinds) > 1, kinds
    got = run(tool, tmp_path, cases)
    for g, w in zip(got, want):
        if w[0] == H.DYN:
            assert g == w
        else:
            assert g[:2] == w and g[6] == [0] * 320
    # ---- directed headers: at every start bit 0-7 and every 16-byte misalignment
    hc = H.header_cases()
    cases, want = [], []
    for k, (name, (hlit, hdist, toks, cl, hclen, kind, status)) in enumerate(hc.items()):
        for start in range(8):
            for mis in (range(16) if name in ("hlit257_hdist1", "longest_legal") else ((k + start) % 16,)):
                w = W.BitWriter()
                w.bits(0x5a5a5a5a5a5a5a5a5a5a5a5a5a5a5a5a5a5a >> 3, 8 * mis + start)  # what precedes
                H.header(w, hlit, hdist, toks, cl=cl, hclen=hclen, final=bool(start & 1))
                end = w.n
                w.bits(0x2aaaaaaaaaaaaaaa, 62)  # what follows the header
                b = w.bytes()
                cases.append((b, 8 * mis + start, 8 * len(b)))
                if kind == H.DYN:
                    want.append((name, (kind, 0, hlit, hdist, start & 1, end,
                                        H.lens320(H.expand(toks)[:hlit], H.expand(toks)[hlit:]))))
                else:
                    want.append((name, (kind, status)))
    got = run(tool, tmp_path, cases)
    for g, (name, w) in zip(got, want):
        assert (g if w[0] == H.DYN else g[:2]) == w, name
    # ---- a header cut by the member's end: ST_OVERREAD wherever the end falls inside it; no room
    #      for BFINAL + BTYPE is the kernels' own check (not a dynamic header)
    hlit, hdist, toks, cl, hclen, _, _ = hc["hlit286_hdist30"]
    w = W.BitWriter()
    w.bits(5, 3)
    H.header(w, hlit, hdist, toks, cl=cl, hclen=hclen)
    end = w.n
    w.bits(0xffffffffffffffff, 64)
    b = w.bytes()
    cuts = [3, 5, 6, 19, 20, 60, 77, 100, end // 2, end - 9, end - 1, end, end + 1]
    got = run(tool, tmp_path, [(b, 3, c) for c in cuts])
    for c, g in zip(cuts, got):
        if c < 6:
            assert g[:2] == (H.NONE, 0), c
        elif c < end:
            assert g[:2] == (H.ERR, H.OVERREAD), c
        else:
            assert g[:2] == (H.DYN, 0) and g[5] == end, c
    # ---- the longest read: nothing but 7 + 7-bit symbols after a valid code-length code (runs of 18:
    #      the run passes the tables at once) and a header at the very end of the data
    cl = [0] * 19
    for s, n in ((0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (8, 7), (18, 7)):
        cl[s] = n
    w = W.BitWriter()
    H.header(w, 286, 30, [(18, 127)] * 316, cl=cl, hclen=19)
    b = w.bytes()
    w = W.BitWriter()
    H.header(w, 257, 1, hc["hlit257_hdist1"][2])
    b2 = w.bytes()
    got = run(tool, tmp_path, [(b, 0, 8 * len(b)), (b2[:8], 0, 64), (b"", 0, 0), (b"\x05", 0, 8),
                               (b"\x05" + bytes(3), 0, 32)])
    assert got[0][:2] == (H.ERR, H.BAD_TABLE)
    assert got[1][:2] == (H.ERR, H.OVERREAD)
    # (a header word whose 4 code-length code lengths would end at bit 29 of 8: cut off)
    assert got[2][:2] == (H.NONE, 0) and got[3][:2] == (H.ERR, H.OVERREAD)
    assert got[4][:2] == (H.ERR, H.BAD_TABLE)  # all of it there: no code-length code has a length


def test_hdr_core(tool, tmp_path):
    check_all(tool, tmp_path)


def test_runs_clean_under_the_sanitizers(tmp_path):
    exe = _build(tmp_path, "hdr_core_check_san", ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    check_all(exe, tmp_path)
