"""The header pre-pass's records carry the numbers of codes of each length, and the tail kernel
builds its tables from them instead of counting the lengths again (dq_inflate3.hip, round 10; the
block kernel reads the same records' lengths and counts them itself).
Hand-built BGZF members (tests/deflate_writer.py, tests/hdrcases.py) whose dynamic headers put the
counts at their extremes -- HLIT / HDIST at 257 / 1 and 286 / 30, one distance code of length 1,
codes down to 15 bits, repeat runs that cross from the litlen into the distance alphabet, a run that
ends exactly at HLIT + HDIST -- as first blocks and as deferred tails, beside members whose first
block is stored or fixed (the in-kernel path); member counts around the pre-pass's wave width; a
sparse selection; the rejected and the cut headers.  Expected bytes come from zlib, CRCs are
verified, and tools/gpu_checked_tests.sh runs the file under the bounds-checked library too."""
import zlib

import numpy as np
import pytest

import bamutil as B
import deflate_writer as W
import hdrcases as H
from test_header_prepass import BAD_TABLE_MSG, OVERREAD_MSG, _error_of, _gpu_inflate, cut_members, payload

LL257, LL258, LL286, D30 = H.flat_ll(257), H.flat_ll(258), H.flat_ll(286), H.flat_ll(30)
# 257 codes of 10 / 11 bits (a quarter of the code space) and three length symbols of 2 bits
LL_X16 = [x + 2 for x in LL257] + [2, 2, 2]
# 'a'..'o' with 2, 2, 3, 4 .. 15 bits, the end-of-block code with 15 and the length symbol 257 with
# 2: a complete code that uses every length from 2 to 15
LL_DEEP = [0] * 97 + [2, 2] + list(range(3, 16)) + [0] * (256 - 112) + [15, 2]
assert sum(2.0 ** -x for x in LL_DEEP if x) == 1.0


def lit_and_runs(data, n, d):
    """Tokens for codes without most length / distance symbols: every byte of `data` as a literal,
    followed by a match of length n at distance d (which repeats what was just written)."""
    toks = []
    for k, b in enumerate(data):
        toks.append(b)
        if k >= d - 1:
            toks.append((n[k % len(n)], d))
    return toks


def extreme_block(D, name, data=None, hist=b"", final=True):
    """Append to Deflater D one dynamic block with the header `name`; -> the bytes it produces.
    `data` (default: some text) is what the block should hold where its code can hold anything."""
    text = payload(len(name), 300) if data is None else data
    deep = bytes(97 + (7 * k * k + k) % 15 for k in range(200))
    kw = dict(final=final)
    if name == "hlit257_hdist1":          # literals only, no distance code at all
        toks = list(text)
        H.block(D, toks, LL257, [0], hlit=257, hdist=1, **kw)
    elif name == "hlit286_hdist30":       # every symbol has a code: any tokens
        u = hist + text
        toks = W.lz77(u, len(hist))
        H.block(D, toks, LL286, D30, **kw)
    elif name == "one_distance_code":     # one distance code of length 1 (zlib allows the incomplete code)
        toks = lit_and_runs(text[:120], [3], 1)
        H.block(D, toks, LL258, [1], **kw)
    elif name == "rep16_crosses":         # a 16 whose run covers litlen 258, 259 and all four distances
        toks = lit_and_runs(text[:120], [3, 4, 5], 3)
        ht = H.rle(LL_X16[:257]) + [(2, None), (16, 3)]
        assert H.expand(ht) == LL_X16 + [2] * 4
        H.block(D, toks, LL_X16, [2] * 4, htoks=ht, **kw)
    elif name == "rep17_crosses":         # a 17: two zero litlen lengths and three zero distance lengths
        toks = list(text)
        ht = H.rle(LL257) + [(17, 2), (1, None), (1, None)]
        H.block(D, toks, LL257 + [0, 0], [0, 0, 0, 1, 1], htoks=ht, hlit=259, hdist=5, **kw)
    elif name == "rep18_crosses":         # an 18: six zero litlen lengths and fourteen zero distance lengths
        toks = list(text)
        ht = H.rle(LL257) + [(18, 9), (1, None), (1, None)]
        H.block(D, toks, LL257 + [0] * 6, [0] * 14 + [1, 1], htoks=ht, hlit=263, hdist=16, **kw)
    elif name == "run_ends_exactly":      # the last run ends at HLIT + HDIST
        toks = list(text)
        dl = [2, 3, 3, 3, 3, 3, 3]
        ht = H.rle(LL257) + [(2, None), (3, None), (16, 2)]
        assert H.expand(ht) == LL257 + dl
        H.block(D, toks, LL257, dl, htoks=ht, **kw)
    elif name == "codes_of_15_bits":      # every length from 2 to 15: the deepest canonical code
        toks = lit_and_runs(deep, [3], 1)
        H.block(D, toks, LL_DEEP, [1], **kw)
    else:
        raise KeyError(name)
    return W.expand(toks, hist)


EXTREME = ["hlit257_hdist1", "hlit286_hdist30", "one_distance_code", "rep16_crosses", "rep17_crosses",
           "rep18_crosses", "run_ends_exactly", "codes_of_15_bits"]


def member(i):
    """Member i, its kind by i mod 12: the eight extreme headers as first blocks; a stored and a
    fixed first block (then an extreme dynamic one: decoded in the block kernel); an ordinary
    dynamic block; a final extreme one on other data."""
    k = i % 12
    D = W.Deflater()
    if k < 8:
        data = extreme_block(D, EXTREME[k], payload(i, 60 + 23 * (i % 9)))
    elif k == 8:
        head = payload(i, 25)
        D.stored(head)
        data = head + extreme_block(D, "hlit286_hdist30", payload(i, 200), hist=head)
    elif k == 9:
        head = payload(i, 80)
        D.fixed(W.lz77(head))
        data = head + extreme_block(D, "rep16_crosses", payload(i, 90))
    elif k == 10:
        data = payload(i, 400)
        D.dynamic(W.lz77(data), final=True)
    else:
        data = extreme_block(D, "hlit286_hdist30", payload(i, 500))
    body = D.finish()
    assert zlib.decompress(body, -15) == data, (i, k)
    return W.member(body, data), data


def _file(n, first=0):
    ms = [member(first + i) for i in range(n)]
    return b"".join(m for m, _ in ms) + B.EOF_BLOCK, b"".join(d for _, d in ms)


def tail_member(text, name, first="dynamic"):
    """7,000 bytes in a first block (ordinary dynamic header, or the 286 / 30 one), then a small
    last block with the extreme header `name`: the block kernel defers it to the tail kernel, whose
    header the tail pre-pass decodes."""
    D = W.Deflater()
    head = text[:7000]
    t0 = W.lz77(head)
    if first == "dynamic":
        H.block(D, t0, *W.Deflater().dynamic_lengths(t0))
    else:
        H.block(D, t0, LL286, D30)
    data = head + extreme_block(D, name, text[7000:7600], hist=head)
    body = D.finish()
    assert zlib.decompress(body, -15) == data, name
    return W.member(body, data), data


def bad_member(name):
    """A member whose first header is rejected; zlib rejects it too."""
    w = W.BitWriter()
    if name == "all_lengths_15":          # 257 + 2 codes of 15 bits: incomplete, the table build's error
        H.header(w, 257, 2, H.rle([15] * 259), final=True)
    elif name == "all_lengths_15_max":
        H.header(w, 286, 30, H.rle([15] * 316), final=True)
    elif name == "run_one_past":          # run_ends_exactly's tokens with HDIST one smaller
        H.header(w, 257, 6, H.rle(LL257) + [(2, None), (3, None), (16, 2)], final=True)
    else:                                 # hdrcases: rep16_first, missing_eob, zero_run_past
        hlit, hdist, toks, cl, hclen, kind, _ = H.header_cases()[name]
        assert kind == H.ERR
        H.header(w, hlit, hdist, toks, cl=cl, hclen=hclen, final=True)
    body = w.bytes() + bytes(40)
    with pytest.raises(zlib.error):
        zlib.decompress(body, -15)
    return W.member(body, b"0123456789")


BAD = ["all_lengths_15", "all_lengths_15_max", "run_one_past", "rep16_first", "missing_eob", "zero_run_past"]


@pytest.fixture(scope="module")
def text():
    return b"".join(payload(i, 900) for i in range(9))


def test_fixtures(text):
    """Every member inflates with zlib (member / tail_member assert it), zlib rejects the bad ones,
    and the headers are what their names say (tests/deflate_reader.py)."""
    import deflate_reader as R
    seen, blocks = {}, []
    for i in range(12):
        m, _ = member(i)
        for blk in R.read(m[18:-8]):
            if blk.btype == 2:
                seen[(blk.hlit, blk.hdist)] = blk
                blocks.append(blk)
    assert (257, 1) in seen and (286, 30) in seen
    assert max(seen[(286, 30)].ll_lens) == 9 and sum(1 for x in seen[(286, 30)].d_lens if x) == 30
    assert seen[(258, 1)].d_lens == [1]
    assert any(sorted(set(b.ll_lens) - {0}) == list(range(2, 16)) for b in blocks)
    for key, tok, left in (((260, 4), 16, 2), ((259, 5), 17, 2), ((263, 16), 18, 6)):
        blk, n = seen[key], 0
        for t in blk.header:
            k = R.header_run(t)
            if n < blk.hlit < n + k:
                assert t[0] == tok and blk.hlit - n == left, key
                break
            n += k
        else:
            raise AssertionError(key)
    for name in EXTREME:
        for first in ("dynamic", "flat"):
            m, _ = tail_member(text, name, first)
            blks = R.read(m[18:-8])
            assert len(blks) == 2 and blks[1].end - blks[1].start <= 32768
    for name in BAD:
        bad_member(name)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_gpu_member_counts(n):
    f, want = _file(n, first=n % 12)
    got = _gpu_inflate(f)
    assert np.array_equal(got, np.frombuffer(want, np.uint8))


@pytest.mark.gpu
def test_gpu_extreme_tails(text):
    """Deferred tails whose own header is each extreme one (after an ordinary first block and after
    a 286 / 30 one), between members whose first block is stored or fixed."""
    ms = []
    for k, name in enumerate(EXTREME):
        ms += [tail_member(text, name, "dynamic"), member(8 + k % 2), tail_member(text, name, "flat")]
    got = _gpu_inflate(b"".join(m for m, _ in ms) + B.EOF_BLOCK)
    assert np.array_equal(got, np.frombuffer(b"".join(d for _, d in ms), np.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("name", BAD)
def test_gpu_rejected_headers(name):
    """A rejected header among good members: the read fails at that block with the table error,
    whether the header decoder (runs, missing codes) or the table build (the incomplete codes of 15
    bits) finds it."""
    from disq_amd import _lib
    k = 2 + 5 * BAD.index(name)
    before = _file(k)[0][:-len(B.EOF_BLOCK)]
    after = _file(66 - k, first=k)[0]
    with pytest.raises(_lib.DqError, match="%s in BGZF block at %d$" % (BAD_TABLE_MSG, len(before))):
        _gpu_inflate(before + bad_member(name) + after)


@pytest.mark.gpu
def test_gpu_rejected_tail_header(text):
    """A deferred tail whose header decodes but whose codes are incomplete: the tail kernel's table
    build rejects it from the record's counts."""
    from disq_amd import _lib
    good = tail_member(text, "rep16_crosses")[0]
    D = W.Deflater()
    t0 = W.lz77(text[:7000])
    H.block(D, t0, *W.Deflater().dynamic_lengths(t0))
    H.header(D.w, 257, 2, H.rle([15] * 259), final=True)
    D.w.bits(0, 300)
    bad = W.member(D.finish(), text[:7100])
    with pytest.raises(_lib.DqError, match="%s in BGZF block at %d$" % (BAD_TABLE_MSG, len(good))):
        _gpu_inflate(good + bad + good + B.EOF_BLOCK)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(cut_members()))
def test_gpu_cut_headers(name):
    """The five headers cut by the member's end keep the code of profiles/r9e_cut_header_codes.txt
    (this build's column): ST_OVERREAD at block 0."""
    ok = _file(5)[0]
    assert _error_of(cut_members()[name] + ok).endswith("%s in BGZF block at 0" % OVERREAD_MSG)


# ---------------------------------------------------------------------------- a sparse selection
def sparse_bam(bam1):
    """A BAM of 2,400 short records on reference 0 in hand-built members of 500-900 bytes, by member
    index mod 6: a 286 / 30 header, an ordinary one, a stored first block, a fixed first block, a
    deferred tail with the 286 / 30 header, a deferred tail with the one-distance-code header."""
    u = B.inflate_all(bam1)
    stream = u[:B.header_len(u)] + b"".join(
        B.make_record(0, 1000 + 2000 * i, b"q%d" % i, 50 + 10 * (i % 7)) for i in range(2400))
    out, p, k = [], 0, 0
    while p < len(stream):
        n = min(len(stream) - p, 500 + 80 * (k % 6))
        data = stream[p:p + n]
        D, kind = W.Deflater(), k % 6
        if kind == 0:
            H.block(D, W.lz77(data), LL286, D30, final=True)
        elif kind == 1:
            D.dynamic(W.lz77(data), final=True)
        elif kind == 2:
            D.stored(data[:30])
            H.block(D, W.lz77(data, 30), LL286, D30, final=True)
        elif kind == 3:
            D.fixed(W.lz77(data), final=True)
        elif kind == 4:
            H.block(D, W.lz77(data, 0, n - 150), LL286, D30)
            H.block(D, W.lz77(data, n - 150), LL286, D30, final=True)
        else:
            t0 = W.lz77(data, 0, n - 150)
            H.block(D, t0, *D.dynamic_lengths(t0))
            H.block(D, list(data[n - 150:]), LL258, [1], final=True)
        body = D.finish()
        assert zlib.decompress(body, -15) == data
        out.append(W.member(body, data))
        p += n
        k += 1
    return b"".join(out) + B.EOF_BLOCK, k


@pytest.mark.gpu
def test_gpu_sparse_selection(golden):
    """Two far-apart intervals through the .bai span run: record i of the pre-pass (and tails[i])
    belongs to block sel[i] != i, and neighbouring records hold different headers and counts."""
    import os
    from disq_amd import _lib
    from oracle import oracle as O
    data, nmem = sparse_bam(open(os.path.join(golden, "1.bam"), "rb").read())
    recs = O.OracleBam(data).read_all()
    ivs = [(0, 2000 * 700, 2000 * 730), (0, 2000 * 1900, 2000 * 1930)]
    q = O.optimize_intervals(ivs)
    want = recs[[bool(O.overlaps(r, q)) for r in recs]]
    assert 50 < len(want) < 70
    with _lib.Context(split_size=0, verify_crc=True, device=0) as c:
        c.open_bytes(data)
        c.set_index(c.write_bai())
        b = c.read(with_raw=False, traversal=(ivs, False))
        assert np.array_equal(b["voffset"], want["voffset"])
        assert np.array_equal(b["hash"], want["hash"])
        st = c.run_resident((ivs, False))
        assert st.n_blocks == nmem + 1 and 0 < st.blocks_inflated < nmem // 4


# ---------------------------------------------------------------------------- the paths are reached
_PHASES = """
import sys
sys.path[:0] = [%r, %r]
import test_header_prepass_counts as T
text = b"".join(T.payload(i, 900) for i in range(9))
ms = [T.tail_member(text, name)[0] for name in T.EXTREME[:3]] + [T.member(8)[0]]
T._gpu_inflate(b"".join(ms) + T.B.EOF_BLOCK)
"""


@pytest.mark.gpu
def test_gpu_tails_are_deferred_and_predecoded():
    """The tail members do reach the tail kernel, and both pre-pass launches ran (the library's
    phase report, DQ_TIMING, read once per process: one child process, which is what this test is
    about)."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", _PHASES % (os.path.dirname(here), here)],
                       env=dict(os.environ, DQ_TIMING="1"), stderr=subprocess.PIPE, check=True)
    assert b"tail kernel: 3 tails" in r.stderr, r.stderr[-2000:]
    assert b"header pre-pass (first blocks): 1 waves" in r.stderr, r.stderr[-2000:]
    assert b"header pre-pass (tails): 1 waves" in r.stderr, r.stderr[-2000:]
