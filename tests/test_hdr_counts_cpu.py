"""The numbers of codes of each length that the serial header decoder (disq_amd/csrc/dq_hdr_core.h)
hands its sink while it decodes a dynamic DEFLATE header -- what the header pre-pass stores in its
records, so that the inflate kernels' table builds need not count the lengths again -- on the CPU
through tools/hdr_core_check.cpp (`counts`), against the ll_lens and d_lens tests/deflate_reader.py
reads from the same bits: zlib streams, the directed headers of tests/hdrcases.py and the extreme
ones below; then the same program under AddressSanitizer and UBSan."""
import os
import struct
import subprocess

import pytest

import deflate_reader as R
import deflate_writer as W
import hdrcases as H
from test_hdr_core_cpu import zlib_bodies

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "disq_amd", "csrc")


def _build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.run(["g++", "-g", "-std=c++17", *flags, "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tools", "hdr_core_check.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("hdrcounts"), "hdr_core_check", ["-O1"])


def run(tool, tmp_path, cases):
    """cases: (bytes, header bit position, end bit position) -> per case (kind, status, the 320
    lengths, the 15 litlen counts, the 15 distance counts)."""
    f = tmp_path / "cases.bin"
    f.write_bytes(b"".join(struct.pack("<III", len(b), pos, end) + b for b, pos, end in cases))
    out = subprocess.run([tool, str(f), "counts"], check=True, stdout=subprocess.PIPE).stdout.decode().split("\n")
    res = []
    for line in out[:len(cases)]:
        p = line.split()
        c = [int(x) for x in p[7:]]
        assert len(c) == 30
        res.append((int(p[0]), int(p[1]), [int(ch, 16) for ch in p[6]], c[:15], c[15:]))
    assert len(res) == len(cases)
    return res


def counts(lens):
    return [sum(1 for x in lens if x == ln) for ln in range(1, 16)]


def reader_lens(b, pos):
    """ll_lens, d_lens of the dynamic header at bit `pos`, by the reader (DeflateError if it
    rejects the header)."""
    r = R._Bits(b)
    r.get(pos)
    blk = R.Block()
    blk.final, blk.btype = bool(r.get(1)), r.get(2)
    assert blk.btype == 2
    R._dynamic_header(r, blk)
    return blk.ll_lens, blk.d_lens


def extreme_cases():
    """name -> (hlit, hdist, tokens, cl or None, expected kind): the headers the counts are most
    likely to go wrong on, beside hdrcases.header_cases()."""
    c = {}
    ll257, ll286, d30 = H.flat_ll(257), H.flat_ll(286), H.flat_ll(30)

    def add(name, ll, dl, toks=None, kind=H.DYN, hlit=None, hdist=None):
        seq = list(ll) + list(dl)
        toks = H.rle(seq) if toks is None else toks
        if kind == H.DYN:
            assert H.expand(toks) == seq, name
        c[name] = (len(ll) if hlit is None else hlit, len(dl) if hdist is None else hdist, toks, None, kind)

    add("hlit257_hdist1_zero_distance", ll257, [0])
    add("hlit286_hdist30", ll286, d30)                       # 286 and 30 codes: the largest counts
    add("all_286_of_one_length", [9] * 286, [5] * 30)        # one field holds 286 / 30
    add("one_distance_code_of_length_1", ll257, [1])         # the incomplete code zlib allows
    add("one_distance_code_at_the_end", ll257, [0] * 29 + [1])
    add("all_lengths_15", [15] * 257, [15] * 2)              # (incomplete codes: the tables' business)
    add("all_lengths_15_max", [15] * 286, [15] * 30)
    # runs that cross from the litlen into the distance alphabet: a 16 (three on each side, and
    # five + one), a 17 and an 18 (zeros: nothing is counted), a 16 right after them
    add("rep16_3_3", ll257[:253] + [7] * 4, [7] * 3 + [4, 4],
        H.rle(ll257[:253]) + [(7, None), (16, 3), (4, None), (4, None)])
    add("rep16_5_1", ll257[:251] + [6] * 6, [6, 3],
        H.rle(ll257[:251]) + [(6, None), (16, 3), (3, None)])
    add("rep16_1_5", ll257[:255] + [6] * 2, [6] * 5 + [2],
        H.rle(ll257[:255]) + [(6, None), (16, 3), (2, None)])
    add("rep17_crosses", ll257 + [0] * 2, [0] * 3 + [2, 2],
        H.rle(ll257) + [(17, 2), (2, None), (2, None)])
    add("rep18_crosses", ll257 + [0] * 6, [0] * 14 + [1, 1],
        H.rle(ll257) + [(18, 9), (1, None), (1, None)])
    add("rep16_of_a_length_before_zeros", ll257, [5, 0, 0, 0, 5, 5, 5, 5],
        H.rle(ll257) + [(5, None), (17, 0), (5, None), (16, 0)])
    # a run that ends exactly at HLIT + HDIST, and the same tokens with HDIST one smaller
    t = H.rle(ll257) + [(3, None), (16, 3)]
    add("run_ends_exactly", ll257, [3] * 7, t)
    add("run_one_past", ll257, [3] * 6, t, kind=H.ERR)
    add("zero_run_one_past", ll257, [0] * 11, H.rle(ll257) + [(18, 1)], kind=H.ERR)
    # a repeat with nothing before it; no end-of-block code
    add("rep16_first", ll257, [0], [(16, 0)] + H.rle(ll257[3:] + [0]), kind=H.ERR)
    noeob = list(ll257)
    noeob[256] = 0
    add("no_eob", noeob, [1, 1], kind=H.ERR)
    add("no_eob_inside_a_run", [8] * 250 + [0] * 7 + [8] * 20, [1, 1], kind=H.ERR)
    return c


def check_all(tool, tmp_path):
    # ---- zlib streams, levels 1-9: every dynamic block
    cases, want = [], []
    for body in zlib_bodies():
        for blk in R.read(body):
            if blk.btype == 2:
                cases.append((body, blk.start, 8 * len(body)))
                want.append((blk.ll_lens, blk.d_lens))
    assert len(cases) >= 10
    for g, (ll, dl) in zip(run(tool, tmp_path, cases), want):
        assert g[0] == H.DYN and g[2] == H.lens320(ll, dl)
        assert (g[3], g[4]) == (counts(ll), counts(dl))
    # ---- the directed headers and the extreme ones, at start bits 0-7 and shifting misalignments
    hc = [(n, c[:5], c[5]) for n, c in H.header_cases().items()] + \
         [(n, c[:4] + (None,), c[4]) for n, c in extreme_cases().items()]
    cases, want = [], []
    for k, (name, (hlit, hdist, toks, cl, hclen), kind) in enumerate(hc):
        for start in range(8):
            w = W.BitWriter()
            w.bits(0x5a5a5a5a5a5a5a5a5a5a5a5a5a5a5a5a5a5a >> 3, 8 * ((k + start) % 16) + start)
            pos = w.n
            H.header(w, hlit, hdist, toks, cl=cl, hclen=hclen)
            w.bits(0x2aaaaaaaaaaaaaaa, 62)
            b = w.bytes()
            cases.append((b, pos, 8 * len(b)))
            if kind == H.DYN:
                ll, dl = reader_lens(b, pos)
                assert (ll, dl) == (H.expand(toks)[:hlit], H.expand(toks)[hlit:]), name
                want.append((name, ll, dl))
            else:
                if not (hlit > 286 or hdist > 30):
                    with pytest.raises(R.DeflateError):
                        reader_lens(b, pos)
                want.append((name, None, None))
    seen = set()
    for g, (name, ll, dl) in zip(run(tool, tmp_path, cases), want):
        if ll is None:
            assert g[:2] == (H.ERR, H.BAD_TABLE), name
            continue
        assert g[0] == H.DYN and g[2] == H.lens320(ll, dl), name
        assert (g[3], g[4]) == (counts(ll), counts(dl)), name
        seen.add((max(g[3]), max(g[4])))
    assert (286, 30) in seen and (257, 0) not in seen and any(d == 0 for _, d in seen)


def test_extreme_cases_are_what_they_say():
    c = extreme_cases()
    assert c["one_distance_code_of_length_1"][:2] == (257, 1)
    assert c["hlit286_hdist30"][:2] == (286, 30)
    for name in ("rep16_3_3", "rep16_5_1", "rep16_1_5", "rep17_crosses", "rep18_crosses"):
        hlit, _, toks, _, _ = c[name]
        n, crossing = 0, 0
        for t in toks:
            k = R.header_run(t)
            crossing += t[0] >= 16 and n < hlit < n + k
            n += k
        assert crossing == 1, name
    assert R.header_run(c["run_ends_exactly"][2][-1]) == 6


def test_counts(tool, tmp_path):
    check_all(tool, tmp_path)


def test_counts_under_the_sanitizers(tmp_path):
    exe = _build(tmp_path, "hdr_core_check_san", ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    check_all(exe, tmp_path)
