"""Directed tests of K2's match resolve with the first hop by groups of eight bytes (DQ_RES_OCT,
DESIGN.md section 3, round 12).

With DQ_RES_OCT a thread of the first four waves takes the bytes 8t .. 8t + 7 of a 2048-byte batch
as two half-groups in sequence: the second half inherits the owner live at its byte 0 (and that
owner's descriptor, carry rule and length cut at the resolved size) from the first half's
registers, unless a match starts at its byte 0, and the eight next pointers leave as one 16-byte
store.  The members here are at most three batches long and put match starts at each offset of an
aligned group of eight, the three-start groups, a start at the second half's byte 0 behind a live
match, overlapping runs across the half and the group boundary, carries that end 1-8 bytes into a
batch, sizes of every residue mod 8 next to a batch boundary, and deferred tails that cut the
resolved prefix at each offset of a group; they are read at all 16 output alignments, in sequence
and as a sparse selection through the index.  Every member is one BAM record (44 literal bytes:
the fixed fields, the name "a" and one base; then the pattern as opaque aux bytes), so that the same
members serve the plain read path and the interval traversal.  The CPU test checks the members
against zlib and checks that each holds the pattern it is named for; the GPU tests compare the
decompressed stream with zlib's, CRCs verified."""
import struct
import zlib

import numpy as np
import pytest

import bamutil as B
import deflate_writer as W
import reccases
from test_resolve_groups import Toks, matches

BATCH = 2048           # dq_inflate3.hip: the resolve batch
MAXLEN = 3 * BATCH + 8
HDR = 44               # a record's fixed fields, name "a\0", CIGAR 1M, base and quality: literals
SPACING = 40000        # reference positions of consecutive members' records: > two index windows


def rec_pos(k):
    return SPACING * k + 100


def rec_head(n, k):
    """The first HDR bytes of member k's record of n bytes: a one-base read named "a" mapped at
    rec_pos(k), the smallest record the split guesser accepts (reccases.MIN_FILLER)."""
    h = reccases.record(0, rec_pos(k), b"a\x00", [(1, 0)], 1, mapq=60)
    assert len(h) == HDR
    return struct.pack("<i", n - 4) + h[4:]


def oct_bits(toks):
    """group index -> start bits of the eight bytes of the group (bit i: a match starts at 8g + i)."""
    ob = {}
    for s, _, _ in matches(toks):
        ob[s >> 3] = ob.get(s >> 3, 0) | 1 << (s & 7)
    return ob


def rand_toks(n, seed):
    """n output bytes: HDR literals, then short literal runs and matches of random length and of
    distances up to 64 (half of them at most 8)."""
    rng = np.random.default_rng(seed)
    k = Toks(seed + 500).lit(HDR + 3)
    while k.n < n:
        left = n - k.n
        if left < 3 or rng.random() < 0.35:
            k.lit(min(left, int(rng.integers(1, 6))))
            continue
        r = rng.random()
        ln = 258 if r < 0.03 else int(rng.integers(3, 12)) if r < 0.8 else int(rng.integers(12, 120))
        d = int(rng.integers(1, 9)) if rng.random() < 0.5 else int(rng.integers(1, min(k.n, 64) + 1))
        k.m(min(ln, left), d)
    assert k.n == n
    return k.t


# ---------------------------------------------------------------- the token lists

LENS = (3, 4, 5, 8, 9, 258)


def start_tokens():
    """A lone match of each length from each offset of an aligned group (so it ends at each offset
    too, the half boundary among them), literals on both sides."""
    k = Toks(21).lit(HDR + 300)
    for ln in LENS:
        for off in range(8):
            k.to(((k.n + 12) & ~7) + off).m(ln, 300 - ln % 7).lit(5)
    k.lit((1 - k.n) % 16)  # length 1 mod 16: 16 copies in a row start at 16 alignments
    return k.t


PATTERNS = ((0, 3, 6), (0, 3, 7), (0, 4, 7), (1, 4, 7))
LEADS = ("literal", "match", "overlap")


def pattern_tokens():
    """The groups of three starts, behind a literal, behind a match that ends where the first one
    starts and behind an overlapping match from two groups before; then a start at byte 0 of the
    second half behind a match that is live at byte 3: one from before the group, one that starts
    in the first half."""
    k = Toks(22).lit(HDR + 100)
    placed, live = [], []
    for i, pat in enumerate(PATTERNS):
        for lead in LEADS:
            g = (k.n + 32) & ~7
            if lead == "literal":
                k.to(g + pat[0])
            elif lead == "match":
                k.to(g - 6).m(6 + pat[0], 50)
            else:
                k.to(g - 20).m(20 + pat[0], 9)
            for a, b in zip(pat, pat[1:]):
                k.m(b - a, 60 + a)
            k.m((3, 4, 9)[i % 3], 71).lit(3)
            placed.append((g, pat, lead))
    g = (k.n + 32) & ~7
    k.to(g - 5).m(9, 33).m(6, 44).lit(2)  # bytes 0-3 belong to a match from before the group
    live.append(g)
    g = (k.n + 32) & ~7
    k.to(g + 1).m(3, 35).m(4, 46).lit(2)  # bytes 1-3 to a match that starts in the first half
    live.append(g)
    g = (k.n + 56) & ~7
    k.to(g - 40).m(44, 3).m(258, 2).lit(2)  # the same with overlapping matches on both sides
    live.append(g)
    k.lit((1 - k.n) % 16)
    return k.t, placed, live


OV_D = (1, 2, 3, 4, 5, 6, 7)


def overlap_tokens():
    """Overlapping matches (length > distance) of every distance 1-7 from every offset of a group,
    long enough to cross the half boundary (from the first half) and the group's end; one of 258
    bytes per distance."""
    k = Toks(23).lit(HDR + 11)
    placed = []
    for D in OV_D:
        for s in range(8):
            g = (k.n + 16) & ~7
            ln = 258 if s == D else 9 + D + s % 3
            k.to(g + s).m(ln, D).lit(1 + s % 2)
            placed.append((D, s, ln))
    k.lit((1 - k.n) % 16)
    return k.t, placed


CARRY_R = ((1, 5), (2, 6), (3, 7), (4, 8), (5, 1), (6, 2), (7, 3), (8, 4))


def carry_tokens(r1, r2):
    """A match that straddles the first batch boundary and ends r1 bytes into the batch, one that
    straddles the second and ends r2 bytes into it (overlapping, distance 5); a new match right
    behind the first and literals behind the second."""
    k = Toks(30 + r1).lit(HDR + 700)
    k.to(BATCH - 10).m(10 + r1, 650).m(3 + r1 % 4, 123)
    k.to(2 * BATCH - 9).m(9 + r2, 5).lit(20)
    return k.t


def no_carry_tokens():
    """A match that ends at the first batch boundary and literals behind it, and literals on both
    sides of the second: the first groups of these batches have no start and no carry."""
    k = Toks(40).lit(HDR + 400)
    k.to(BATCH - 30).m(30, 333).lit(40)
    k.to(2 * BATCH - 50).m(4, 8).lit(120).m(7, 2).lit(5)
    return k.t


SIZES = tuple(range(BATCH - 3, BATCH + 5)) + tuple(range(2 * BATCH - 3, 2 * BATCH + 5))
CUT0 = 5000  # a multiple of 8: the deferred tails cut the prefix at CUT0 + 0 .. 7
TAIL = [(9, 4), 70, 71, (30, 2000), 72]


def token_lists():
    """name -> (tokens, tail tokens or None, what the CPU test checks), in the members' order."""
    out = {}
    out["start"] = (start_tokens(), None, None)
    t, placed, live = pattern_tokens()
    out["pattern"] = (t, None, (placed, live))
    t, placed = overlap_tokens()
    out["overlap"] = (t, None, placed)
    for r1, r2 in CARRY_R:
        out["carry%d" % r1] = (carry_tokens(r1, r2), None, (r1, r2))
    out["no_carry"] = (no_carry_tokens(), None, None)
    for n in SIZES:
        out["size%d" % n] = (rand_toks(n, n), None, None)
    out["literals"] = (Toks(41).lit(MAXLEN, 7).t, None, None)  # no match at all, the largest size
    out["run258"] = (Toks(42).lit(HDR + 258).t + [(258, 258)] * 20 + [9], None, None)
    out["run1"] = (Toks(43).lit(HDR + 1).t + [(258, 1)] * 22 + [9, 9], None, None)
    for r in range(8):
        # a first deflate block of CUT0 + r bytes that ends in a match, and a small tail that
        # starts with a match into it: the block kernel resolves a prefix that cuts a group
        out["cut%d" % r] = (rand_toks(CUT0 + r - 6, 60 + r) + [(6, 5)], TAIL, r)
    return out


def build(toks, tail, k):
    """(member, data, tokens) of member k: its first HDR literals become the record's fixed fields."""
    n = W.token_bytes(toks) + (W.token_bytes(tail) if tail else 0)
    assert n <= MAXLEN and not any(isinstance(t, tuple) for t in toks[:HDR])
    toks = list(rec_head(n, k)) + toks[HDR:]
    D = W.Deflater()
    data = W.expand(toks)
    if tail is None:
        D.dynamic(toks, final=True)
    else:
        D.dynamic(toks, final=False)
        D.fixed(tail, final=True)
        data += W.expand(tail, data)
        toks = toks + tail
    assert len(data) == n
    return W.member(D.finish(), data), data, toks


@pytest.fixture(scope="module")
def fx():
    return {name: build(t, tail, k) + (want,) for k, (name, (t, tail, want)) in enumerate(token_lists().items())}


def test_fixtures_hold_their_patterns(fx):
    legal = {b for b in range(256) if not b & (b >> 1 | b >> 2)}  # starts are >= 3 bytes apart
    assert max(bin(b).count("1") for b in legal) == 3
    assert {b for b in legal if bin(b).count("1") == 3} == {sum(1 << i for i in p) for p in PATTERNS}
    for name, (m, d, toks, _) in fx.items():
        assert zlib.decompress(m[18:-8], -15) == d, name
        assert W.token_bytes(toks) == len(d) <= MAXLEN and struct.unpack_from("<i", d)[0] == len(d) - 4
        assert set(oct_bits(toks).values()) <= legal, name
    # a lone match of every length from every offset, so ending at every offset
    _, d, toks, _ = fx["start"]
    ms = matches(toks)
    ends, starts = {s + ln for s, ln, _ in ms}, {s for s, _, _ in ms}
    iso = {(s & 7, ln) for s, ln, _ in ms if s not in ends and s + ln not in starts}
    assert iso == {(o, ln) for o in range(8) for ln in LENS}
    assert {((s + ln) & 7, ln) for s, ln, _ in ms} == iso and len(d) % 16 == 1
    # the three-start groups behind each lead; the second half's own start behind a live match
    _, d, toks, (placed, live) = fx["pattern"]
    ob, ms = oct_bits(toks), matches(toks)
    covered = {x for s, ln, _ in ms for x in range(s, s + ln)}
    assert {(pat, lead) for _, pat, lead in placed} == {(p, l) for p in PATTERNS for l in LEADS}
    for g, pat, lead in placed:
        assert g % 8 == 0 and ob[g >> 3] == sum(1 << b for b in pat)
        assert (g + pat[0] - 1 in covered) == (lead != "literal")
    for g in live:
        assert ob[g >> 3] >> 4 & 1 and g + 3 in covered and g + 4 in {s for s, _, _ in ms}
    assert [ob[g >> 3] & 15 for g in live] == [0, 2, 0] and len(d) % 16 == 1
    # overlaps: every distance from every offset, across the half boundary and the group's end
    _, d, toks, placed = fx["overlap"]
    at = {s: (ln, dist) for s, ln, dist in matches(toks)}
    assert {(D, s) for D, s, _ in placed} == {(D, s) for D in OV_D for s in range(8)}
    for D, s, ln in placed:
        assert any(x & 7 == s and at[x] == (ln, D) for x in at) and ln > D and s + ln > 8
    assert sum(ln == 258 for _, _, ln in placed) == len(OV_D) and len(d) % 16 == 1
    # carries that end 1 .. 8 bytes into the second and the third batch
    for r1, r2 in CARRY_R:
        at = {s: ln for s, ln, _ in matches(fx["carry%d" % r1][2])}
        assert at[BATCH - 10] == 10 + r1 and BATCH + r1 in at and at[2 * BATCH - 9] == 9 + r2
        assert not any(2 * BATCH + r2 <= s < 2 * BATCH + r2 + 20 for s in at)
    assert {r for r, _ in CARRY_R} == {r for _, r in CARRY_R} == set(range(1, 9))
    ms = matches(fx["no_carry"][2])
    for edge in (BATCH, 2 * BATCH):
        assert not any(s < edge + 8 and s + ln > edge for s, ln, _ in ms)
    assert any(s + ln == BATCH for s, ln, _ in ms)
    # sizes of every residue mod 8 on both sides of two batch boundaries; the odd members
    assert {n % 8 for n in SIZES if n < 2 * BATCH - 8} == {n % 8 for n in SIZES if n > BATCH + 8} == set(range(8))
    for n in SIZES:
        assert len(fx["size%d" % n][1]) == n
    assert not matches(fx["literals"][2]) and len(fx["literals"][1]) == MAXLEN
    assert {(ln, dist) for _, ln, dist in matches(fx["run258"][2])} == {(258, 258)}
    assert {(ln, dist) for _, ln, dist in matches(fx["run1"][2])} == {(258, 1)}
    # deferred tails that cut the prefix at each offset of a group
    for r in range(8):
        _, d, toks, _ = fx["cut%d" % r]
        ms, cut = matches(toks), CUT0 + r
        assert cut & 7 == r and any(s + ln == cut for s, ln, _ in ms) and any(s == cut for s, _, _ in ms)
        assert len(d) - cut <= 4096  # small enough for the tail kernel to take (TOUT)


def _gpu_inflate(bgzf_bytes):
    from disq_amd import _lib
    with _lib.Context(split_size=0, verify_crc=True, device=0) as c:
        c.text_open_bytes(bgzf_bytes)
        c.text_run(drop_header_lines=False)
        return c.inflated()


def _check(parts):
    got = _gpu_inflate(b"".join(m for m, _ in parts) + B.EOF_BLOCK)
    want = np.frombuffer(b"".join(d for _, d in parts), np.uint8)
    assert len(got) == len(want)
    bad = np.flatnonzero(np.asarray(got) != want)
    assert bad.size == 0, "first differing byte %d of %d" % (bad[0], len(want))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["start", "pattern", "overlap"])
def test_gpu_groups_at_every_alignment(fx, name):
    m, d = fx[name][:2]
    assert len(d) % 16 == 1
    _check([(m * 16, d * 16)])  # copy i starts at output alignment i


@pytest.mark.gpu
def test_gpu_carries(fx):
    parts = []
    for i, (r1, _) in enumerate(CARRY_R):  # an odd size between them: other alignments
        parts += [fx["carry%d" % r1][:2], fx["size%d" % SIZES[2 * i]][:2]]
    _check(parts + [fx["no_carry"][:2]] * 3)


@pytest.mark.gpu
def test_gpu_sizes_and_runs(fx):
    names = ["size%d" % n for n in SIZES] + ["literals", "run258", "run1"]
    _check([fx[n][:2] for n in names] + [fx[n][:2] for n in reversed(names)])


@pytest.mark.gpu
def test_gpu_deferred_tails_cut_a_group(fx):
    names = ["cut%d" % r for r in range(8)]
    _check([fx[n][:2] for n in names] + [fx["size%d" % SIZES[1]][:2]] + [fx[n][:2] for n in reversed(names)])


FILL = 24  # filler members behind each member: more than the 16-block gap that the span run bridges


def sparse_file(fx):
    """The members, each followed by FILL members of one small record in later 16 kb index windows."""
    out = [B.bgzf_member(reccases.header([("chr1", SPACING * (len(fx) + 1))]), 6)]
    for k, (m, _, _, _) in enumerate(fx.values()):
        out.append(m)
        out += [B.bgzf_member(reccases.filler(60, 0, rec_pos(k) + 17000 + 100 * j), 6) for j in range(FILL)]
    return b"".join(out) + B.EOF_BLOCK, 1 + len(fx) * (1 + FILL)


@pytest.fixture(scope="module")
def sparse(fx):
    from oracle import oracle as O
    data, nmem = sparse_file(fx)
    recs = O.OracleBam(data).read_all()
    assert len(recs) == nmem - 1
    return data, nmem, recs


@pytest.mark.gpu
@pytest.mark.parametrize("phase", [0, 1, 2])
def test_gpu_sparse_selection(fx, sparse, phase):
    """Every third member's record through the index (one record per member, SPACING apart, FILL
    small members between two of them, so that no two selected members share a window of the
    span run): block i of the launch is member sel[i] != i and the output offsets are those of
    the selection.  A window is the member and the few blocks inflated past it, so well under a
    quarter of the file's blocks is inflated.  The records read equal the oracle's (zlib), CRCs
    verified; the three phases cover every member."""
    from disq_amd import _lib
    from oracle import oracle as O
    data, nmem, recs = sparse
    ivs = [(0, rec_pos(k) - 50, rec_pos(k) + 50) for k in range(phase, len(fx), 3)]
    q = O.optimize_intervals(ivs)
    want = recs[[bool(O.overlaps(r, q)) for r in recs]]
    assert len(want) == len(ivs) and set(want["block_size"]) <= {len(d) - 4 for _, d, _, _ in fx.values()}
    with _lib.Context(split_size=0, verify_crc=True, device=0) as c:
        c.open_bytes(data)
        c.set_index(c.write_bai())
        b = c.read(with_raw=False, traversal=(ivs, False))
        assert np.array_equal(b["voffset"], want["voffset"])
        assert np.array_equal(b["hash"], want["hash"])
        st = c.run_resident((ivs, False))
        assert st.n_blocks == nmem + 1 and len(ivs) <= st.blocks_inflated < nmem // 4
