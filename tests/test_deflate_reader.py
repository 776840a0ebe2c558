"""tests/deflate_reader.py against zlib and tests/deflate_writer.py (no GPU): the token lists it
reads expand to what zlib inflates, the bit length it re-derives is the body's, what the writer
wrote is what it reads back, and it raises on invalid streams."""
import zlib

import numpy as np
import pytest

import bamutil as B
import deflate_reader as R
import deflate_writer as W
from disq_amd import synth
from test_inflate_codes import litlen_long_prefixes, skewed_stream


@pytest.fixture(scope="module")
def streams():
    wgs = B.inflate_all(synth.generate(900, seed=41, nthreads=2).bam)
    return {"wgs": wgs[:2 * B.BLOCK_U], "skewed": skewed_stream(n=600)[:2 * B.BLOCK_U]}


def raw(data, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(data) + c.flush()


def check_body(body, history=b""):
    blocks = R.read(body, len(history))
    toks = [t for b in blocks for t in b.tokens]
    z = zlib.decompressobj(-15, zdict=history) if history else zlib.decompressobj(-15)
    assert W.expand(toks, history) == z.decompress(body)
    assert blocks[-1].final and not any(b.final for b in blocks[:-1])
    assert blocks[0].start == 0
    for a, b in zip(blocks, blocks[1:]):
        assert a.end == b.start
    pad = 8 * len(body) - blocks[-1].end
    assert 0 <= pad < 8 and blocks[-1].end == 8 * len(body) - pad
    return blocks


@pytest.mark.parametrize("level,strategy", [(0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY),
                                            (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY),
                                            (6, zlib.Z_FIXED)])
@pytest.mark.parametrize("name", ["wgs", "skewed"])
def test_reads_zlib_bodies(streams, name, level, strategy):
    u = streams[name]
    assert len(u) > B.BLOCK_U
    blocks = check_body(raw(u, level, strategy))
    want = 0 if level == 0 else 1 if strategy == zlib.Z_FIXED else 2
    assert {b.btype for b in blocks} == {want}
    for b in blocks:
        if b.btype == 2:
            assert len(b.ll_lens) == b.hlit and len(b.d_lens) == b.hdist
            assert sum(R.header_run(t) for t in b.header) == b.hlit + b.hdist
            assert len(b.cl_lens) == 19 and not any(b.cl_lens[s] for s in W.CL_ORDER[b.hclen:])


def test_agrees_with_the_inflate_tests_header_parser(streams):
    """test_inflate_codes.litlen_long_prefixes (its own small parser) counts the same prefixes from
    this reader's code lengths."""
    body = raw(streams["skewed"][:B.BLOCK_U], 6)
    b = R.read(body)[0]
    codes = W.canonical(b.ll_lens)
    mine = len({codes[i] >> (ln - 10) for i, ln in enumerate(b.ll_lens) if ln > 10})
    assert mine == litlen_long_prefixes(body) > 0


def test_reads_back_what_the_writer_wrote(streams):
    u = streams["wgs"]
    pieces = {"s": u[:700], "f": u[700:3000], "d": u[3000:9000]}
    for order in ("sfd", "dfs", "fsd", "ddf"):
        D = W.Deflater()
        want, data = [], b""
        for i, k in enumerate(order):
            final = i == len(order) - 1
            piece = pieces[k]
            toks = W.lz77(data + piece, len(data))  # (matches may reach into the earlier blocks)
            if k == "s":
                D.stored(piece, final)
                want.append((0, list(piece), None))
            elif k == "f":
                D.fixed(toks, final)
                want.append((1, toks, None))
            else:
                ll = D.dynamic_lengths(toks)
                D.dynamic(toks, final, lens=ll)
                want.append((2, toks, ll))
            data += piece
        body = D.finish()
        blocks = check_body(body)
        assert [x.start for x in blocks] == D.starts
        assert len(blocks) == len(want)
        for x, (bt, toks, ll) in zip(blocks, want):
            assert x.btype == bt and x.tokens == toks
            if ll is not None:
                assert x.ll_lens == ll[0][:x.hlit] and not any(ll[0][x.hlit:])
                assert x.d_lens == ll[1][:x.hdist] and not any(ll[1][x.hdist:])
        assert W.expand([t for x in blocks for t in x.tokens]) == data


def test_members_splits_bgzf():
    d1, d2 = b"hello hello hello", bytes(range(200))
    z = W.member(raw(d1, 6), d1) + W.member(raw(d2, 0), d2)
    got = R.members(z + B.EOF_BLOCK)
    assert [(zlib.decompress(b, -15), c, n) for b, c, n in got] == [
        (d1, zlib.crc32(d1), len(d1)), (d2, zlib.crc32(d2), len(d2)), (b"", 0, 0)]
    with pytest.raises(R.DeflateError):
        R.members(z[:-1])
    with pytest.raises(R.DeflateError):
        R.members(b"\x00" + z)


def _bad_bodies():
    rng = np.random.default_rng(5)
    lit = [int(x) for x in rng.integers(0, 256, 40)]
    out = {}
    D = W.Deflater()
    D.fixed(lit, final=True, extra=(286,))
    out["symbol 286"] = D.finish()
    D = W.Deflater()
    D.fixed(lit + [(5, 41)], final=True)
    out["distance before the start"] = D.finish()
    D = W.Deflater()
    D.fixed(lit, final=False)
    out["no final block"] = D.finish()
    D = W.Deflater()
    D.fixed(lit, final=True)
    out["bytes after the final block"] = D.finish() + b"\x00"
    D = W.Deflater()
    D.stored(bytes(lit), final=True)
    s = bytearray(D.finish())
    s[3] ^= 1
    out["LEN / NLEN"] = bytes(s)
    out["reserved type"] = b"\x07\x00"
    # dynamic blocks with a broken literal/length code: over-subscribed, incomplete
    for name, fix in (("over-subscribed", lambda ll: ll.__setitem__(0, ll[0] - 1)),
                      ("incomplete", lambda ll: ll.__setitem__(0, ll[0] + 1))):
        D = W.Deflater()
        ll, dl = D.dynamic_lengths(lit)
        ll = list(ll)
        fix(ll)
        w = W.Deflater()
        try:
            w.dynamic(lit, final=True, lens=(ll, dl))
            out[name] = w.finish()
        except Exception:  # (the writer's own canonical() may refuse: then no fixture)
            pass
    return out


@pytest.mark.parametrize("name", sorted(_bad_bodies()))
def test_raises_on_invalid(name):
    body = _bad_bodies()[name]
    with pytest.raises(R.DeflateError):
        R.read(body)
    # zlib refuses the same body (or, for a missing final block, never reaches the end)
    z = zlib.decompressobj(-15)
    try:
        z.decompress(body)
        assert not z.eof or z.unused_data
    except zlib.error:
        pass
