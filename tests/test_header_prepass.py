"""The inflate kernels' header pre-pass (dq_inflate3.hip, inflate_header_kernel): one lane per BGZF
block decodes the dynamic header of the block's first deflate block (and of a deferred tail's first)
before the kernel that inflates it.  Small hand-built members (tests/deflate_writer.py,
tests/hdrcases.py), expected bytes from zlib: block counts around the wave width with very
different header lengths in one wave, stored and fixed first blocks (the in-kernel path), later
dynamic blocks (the in-kernel path), deferred tails (good, fixed-code, with a bad header), every
rejected header of hdrcases.header_cases() between good blocks, and one context run on files of
different block counts (the record buffer grows and is reused)."""
import zlib

import numpy as np
import pytest

import bamutil as B
import deflate_reader as R
import deflate_writer as W
import hdrcases as H

BAD_TABLE_MSG, OVERREAD_MSG = "invalid Huffman code lengths", "deflate data overrun"  # dq_api.hip


def payload(i, n):
    rng = np.random.default_rng(1000 + i)
    words = [b"chr%d\t" % (i % 23), b"ACGT" * (1 + i % 5), b"PASS;", bytes([65 + i % 26]) * 7, b"\n"]
    out = b"".join(words[k] for k in rng.integers(0, len(words), n // 3 + 1))
    return (out + bytes(rng.integers(0, 256, 16, dtype=np.uint8)))[:n]


def good_member(i):
    """Member i, its kind by i mod 5: a dynamic first block with a run-length coded header (short),
    one with every length sent literally (some 1,500 bits), a stored first block, a fixed first
    block, a one-symbol payload (nearly all lengths zero: the shortest header)."""
    k = i % 5
    data = payload(i, 40 + 37 * (i % 11)) if k != 4 else b"z" * (3 + i % 9)
    toks = W.lz77(data)
    D = W.Deflater()
    if k in (0, 4):
        ll, dl = D.dynamic_lengths(toks) if k == 0 else ([0] * 122 + [1] + [0] * 133 + [1], [1, 1])
        if k == 4:
            toks = list(data)  # literals only: this litlen code has no length symbols
        H.block(D, toks, ll, dl, final=True)
    elif k == 1:
        D.dynamic(toks, final=True)
    elif k == 2:
        D.stored(data[:20])
        H.block(D, W.lz77(data, 20), *W.Deflater().dynamic_lengths(W.lz77(data, 20)), final=True)
    else:
        D.fixed(toks, final=True)
    body = D.finish()
    assert zlib.decompress(body, -15) == data
    return W.member(body, data), data


def bad_member(name):
    """A member whose first deflate block has the rejected header `name`, then zero bytes."""
    hlit, hdist, toks, cl, hclen, kind, status = H.header_cases()[name]
    assert kind == H.ERR
    w = W.BitWriter()
    H.header(w, hlit, hdist, toks, cl=cl, hclen=hclen, final=True)
    body = w.bytes() + bytes(40)
    with pytest.raises(zlib.error):
        zlib.decompress(body, -15)
    return W.member(body, b"0123456789")


BAD = [n for n, c in H.header_cases().items() if c[5] == H.ERR]


def _gpu_inflate(bgzf_bytes, ctx=None):
    from disq_amd import _lib
    if ctx is not None:
        ctx.text_open_bytes(bgzf_bytes)
        ctx.text_run(drop_header_lines=False)
        return ctx.inflated().copy()
    with _lib.Context(split_size=0, verify_crc=True, device=0) as c:
        return _gpu_inflate(bgzf_bytes, c)


def _file(n, first=0):
    ms = [good_member(first + i) for i in range(n)]
    return b"".join(m for m, _ in ms) + B.EOF_BLOCK, b"".join(d for _, d in ms)


def test_fixtures():
    """The good members inflate with zlib (good_member asserts it), zlib rejects the bad ones, and
    the header lengths in one wave differ widely."""
    bits = []
    for i in range(10):
        m, _ = good_member(i)
        blk = R.read(m[18:-8])[0]
        if blk.btype == 2:
            bits.append(blk.data - blk.start)
    assert min(bits) < 150 and max(bits) > 5 * min(bits), bits
    for name in BAD:
        bad_member(name)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_gpu_block_counts(n):
    f, want = _file(n)
    got = _gpu_inflate(f)
    assert np.array_equal(got, np.frombuffer(want, np.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("name", BAD)
def test_gpu_rejected_headers(name):
    """A rejected header at a lane inside a wave of good blocks: the read fails with the header's
    error at that block (so every block before it inflated)."""
    from disq_amd import _lib
    k = 3 + 7 * BAD.index(name) % 60
    before, _ = _file(k)
    before = before[:-len(B.EOF_BLOCK)]
    after, _ = _file(70 - k, first=k)
    with pytest.raises(_lib.DqError, match="%s in BGZF block at %d$" % (BAD_TABLE_MSG, len(before))):
        _gpu_inflate(before + bad_member(name) + after)


@pytest.mark.gpu
def test_gpu_several_rejected_in_one_wave():
    """Rejected headers at several lanes of one wave: the first one is reported."""
    from disq_amd import _lib
    parts = [good_member(i)[0] if i % 4 else bad_member(BAD[i // 4 % len(BAD)]) for i in range(1, 64)]
    pos = len(b"".join(parts[:3]))
    with pytest.raises(_lib.DqError, match="%s in BGZF block at %d$" % (BAD_TABLE_MSG, pos)):
        _gpu_inflate(b"".join(parts) + B.EOF_BLOCK)


def cut_members():
    """name -> a member whose dynamic header (hdrcases' hlit286_hdist30, 307 bits, the code-length
    code's lengths end at bit 17 + 3 HCLEN) is cut off by the member's end after `cut` bytes: inside
    the code-length code's lengths (3, 6), inside the length symbols (12, 30) and in the last
    symbol (38).  The gzip trailer and the next member follow."""
    hlit, hdist, toks, cl, hclen, _, _ = H.header_cases()["hlit286_hdist30"]
    w = W.BitWriter()
    H.header(w, hlit, hdist, toks, cl=cl, hclen=hclen, final=True)
    body = w.bytes()
    assert len(body) == 39
    return {"cut%d" % cut: W.member(body[:cut], b"0123456789") for cut in (3, 6, 12, 30, 38)}


def _error_of(bgzf_bytes):
    from disq_amd import _lib
    try:
        _gpu_inflate(bgzf_bytes)
    except _lib.DqError as e:
        return str(e)
    return "no error"


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(cut_members()))
def test_gpu_header_cut_by_the_member_end(name):
    """A header that runs past the member's deflate data is ST_OVERREAD: the decoder checks the end
    before the code-length code's lengths and before every length symbol, and every symbol that
    starts before the end is the header's own.  (The parent checks the end every 1024 bits, after
    it has judged the code-length code: its codes for these members, ST_OVERREAD or ST_BAD_TABLE by
    what follows the member, are in profiles/r9e_cut_header_codes.txt.)"""
    ok, _ = _file(5)
    assert _error_of(cut_members()[name] + ok).endswith("%s in BGZF block at 0" % OVERREAD_MSG)


def _multi(u, cuts, kinds, bad_tail=None):
    """A member of deflate blocks u[cuts[i]:cuts[i + 1]] of the given kinds (dynamic / fixed)."""
    D = W.Deflater()
    for i, kind in enumerate(kinds):
        toks = W.lz77(u, cuts[i], cuts[i + 1])
        final = i == len(kinds) - 1
        if kind == "fixed":
            D.fixed(toks, final)
        elif kind == "bad":
            hlit, hdist, ht, cl, hclen, _, _ = H.header_cases()[bad_tail]
            H.header(D.w, hlit, hdist, ht, cl=cl, hclen=hclen, final=True)
            D.w.bits(0, 300)
        else:
            ll, dl = W.Deflater().dynamic_lengths(toks)
            H.block(D, toks, ll, dl, final=final)
    data = u[:cuts[-1]]
    return W.member(D.finish(), data), data


@pytest.fixture(scope="module")
def text():
    return b"".join(payload(i, 900) for i in range(24))


@pytest.mark.gpu
def test_gpu_later_dynamic_blocks_and_tails(text):
    """Three dynamic blocks of 6,000 bytes each (none deferred: the later headers are decoded in
    the block kernel); a dynamic and a fixed-code tail of 1,000 bytes (deferred: the tail pre-pass
    decodes the first, the tail kernel's own path the second)."""
    ms = [_multi(text, [0, 6000, 12000, 18000], ["dynamic"] * 3),
          _multi(text, [0, 7000, 8000], ["dynamic", "dynamic"]),
          _multi(text, [0, 7000, 8000], ["dynamic", "fixed"]),
          _multi(text, [0, 7000, 7500, 8000], ["dynamic", "dynamic", "dynamic"])]
    for m, d in ms:
        assert zlib.decompress(m[18:-8], -15) == d
    got = _gpu_inflate(b"".join(m for m, _ in ms) + B.EOF_BLOCK)
    assert np.array_equal(got, np.frombuffer(b"".join(d for _, d in ms), np.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rep16_first", "cl_incomplete", "missing_eob", "hlit288_hdist1"])
def test_gpu_bad_tail_header(text, name):
    from disq_amd import _lib
    good = _multi(text, [0, 7000, 8000], ["dynamic", "dynamic"])[0]
    bad = _multi(text, [0, 7000, 8000], ["dynamic", "bad"], bad_tail=name)[0]
    with pytest.raises(_lib.DqError, match="%s in BGZF block at %d$" % (BAD_TABLE_MSG, len(good))):
        _gpu_inflate(good + bad + good + B.EOF_BLOCK)


@pytest.mark.gpu
def test_gpu_one_context_files_of_different_sizes():
    """130 blocks, then 3, then 200 on one context: the record buffer is reused and grown."""
    from disq_amd import _lib
    with _lib.Context(split_size=0, verify_crc=True, device=0) as c:
        for n, first in ((130, 0), (3, 7), (200, 2)):
            f, want = _file(n, first)
            assert np.array_equal(_gpu_inflate(f, c), np.frombuffer(want, np.uint8)), n


# ---------------------------------------------------------------------------- a sparse selection
def sparse_bam(bam1):
    """A BAM of 2,400 short records on reference 0 in some 630 hand-built members of 500-900 bytes
    whose neighbours differ: by member index mod 6 a run-length coded dynamic header, a literal
    one, a stored first block, a fixed first block, a dynamic deferred tail, a fixed deferred tail."""
    u = B.inflate_all(bam1)
    stream = u[:B.header_len(u)] + b"".join(
        B.make_record(0, 1000 + 2000 * i, b"q%d" % i, 50 + 10 * (i % 7)) for i in range(2400))
    out, p, k = [], 0, 0
    while p < len(stream):
        n = min(len(stream) - p, 500 + 80 * (k % 6))
        data = stream[p:p + n]
        D, kind = W.Deflater(), k % 6
        if kind == 0:
            H.block(D, W.lz77(data), *D.dynamic_lengths(W.lz77(data)), final=True)
        elif kind == 1:
            D.dynamic(W.lz77(data), final=True)
        elif kind == 2:
            D.stored(data[:30])
            t = W.lz77(data, 30)
            H.block(D, t, *D.dynamic_lengths(t), final=True)
        elif kind == 3:
            D.fixed(W.lz77(data), final=True)
        else:
            t0, t1 = W.lz77(data, 0, n - 150), W.lz77(data, n - 150)
            H.block(D, t0, *D.dynamic_lengths(t0))
            if kind == 4:
                H.block(D, t1, *D.dynamic_lengths(t1), final=True)
            else:
                D.fixed(t1, final=True)
        body = D.finish()
        assert zlib.decompress(body, -15) == data
        out.append(W.member(body, data))
        p += n
        k += 1
    return b"".join(out) + B.EOF_BLOCK, k


@pytest.mark.gpu
def test_gpu_sparse_selection(golden):
    """Two far-apart intervals through the .bai span run (the records lie 2 kb apart, eight to a
    16 kb index window, five to a member): the blocks of two windows are inflated,
    so record i of the pre-pass (and tails[i]) belongs to block sel[i] != i, and neighbouring
    records hold different headers.  The records read equal the oracle's (zlib), CRCs verified."""
    import os
    from disq_amd import _lib
    from oracle import oracle as O
    data, nmem = sparse_bam(open(os.path.join(golden, "1.bam"), "rb").read())
    recs = O.OracleBam(data).read_all()
    ivs = [(0, 2000 * 700, 2000 * 730), (0, 2000 * 1900, 2000 * 1930)]  # 30 records each, 2 kb apart
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


# ---------------------------------------------------------------------------- deferral is reached
_TAIL_COUNT = """
import sys
sys.path[:0] = [%r, %r]
import test_header_prepass as T
text = b"".join(T.payload(i, 900) for i in range(24))
ms = [T._multi(text, [0, 7000, 8000], ["dynamic", k])[0] for k in ("dynamic", "fixed", "dynamic")]
ms.append(T._multi(text, [0, 6000, 12000, 18000], ["dynamic"] * 3)[0])
T._gpu_inflate(b"".join(ms) + T.B.EOF_BLOCK)
"""


@pytest.mark.gpu
def test_gpu_tails_are_deferred():
    """The members the tail tests use do reach the tail kernel (and so the tail pre-pass): the
    library's phase report (DQ_TIMING, read once per process: a child process) counts 3 tails of 4
    blocks.  This is what the test is about: one child process."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", _TAIL_COUNT % (os.path.dirname(here), here)],
                       env=dict(os.environ, DQ_TIMING="1"), stderr=subprocess.PIPE, check=True)
    assert b"tail kernel: 3 tails" in r.stderr, r.stderr[-2000:]


if __name__ == "__main__":  # the cut-header members' errors under the library DQ_GPU_LIB names
    ok = _file(5)[0]
    for name, m in sorted(cut_members().items()):
        print(name, _error_of(m + ok))
