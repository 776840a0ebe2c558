"""Directed tests of K2's match resolve, whose first hop works by groups of four bytes (DESIGN.md
section 3, round 7).

inflate_block_kernel resolves a block's matches in batches of 2048 output bytes.  In the first
hop thread t takes the four bytes 4t .. 4t + 3 of a batch, finds their (at most two) owning
matches with one search of the match-start bitmap and publishes the four next pointers as one
64-bit word; then every thread adopts the pointers of the bytes it copies (one byte per 512-byte
step in the product build, the same four bytes with -DDQ_RES_G=4), follows chains inside the
byte's 512-byte step by pointer jumping and copies step by step.  A match that straddles a batch
start is the carry.  These members put match starts at every offset of a group, overlapping runs
across the step and batch boundaries, carries that end 1-4 bytes into a batch, chains of matches
inside one step, and sizes that cut a group; the patterns are read at several output alignments
(the group pattern at all 16).  The members are token lists written bit by bit
(tests/deflate_writer.py); the CPU test checks them against zlib and checks that each one really
holds the pattern it is named for, the GPU tests compare the decompressed stream with zlib's."""
import zlib

import numpy as np
import pytest

import bamutil as B
import deflate_writer as W

STEP, BATCH = 512, 2048  # dq_inflate3.hip: the ordered step and the resolve batch (NB * G * WG)


class Toks:
    """A token list under construction: literals are pseudo-random bytes, n is the output size."""

    def __init__(self, seed):
        self.t, self.n, self.rng = [], 0, np.random.default_rng(seed)

    def lit(self, k=1, alphabet=256):
        self.t += [int(b) for b in self.rng.integers(0, alphabet, k)]
        self.n += k
        return self

    def to(self, pos):
        assert pos >= self.n, (pos, self.n)
        return self.lit(pos - self.n)

    def m(self, ln, d):
        assert 3 <= ln <= 258 and 1 <= d <= min(self.n, 32768), (ln, d, self.n)
        self.t.append((ln, d))
        self.n += ln
        return self


def rand_tokens(n, seed, far=True):
    """n output bytes of short literal runs and matches of random length and distance (no search:
    any distance into the output so far is a valid match)."""
    rng = np.random.default_rng(seed)
    k = Toks(seed + 1000)
    k.lit(min(n, 3))
    while k.n < n:
        left = n - k.n
        if left < 3 or rng.random() < 0.35:
            k.lit(min(left, int(rng.integers(1, 6))))
            continue
        r = rng.random()
        ln = 258 if r < 0.03 else int(rng.integers(3, 12)) if r < 0.8 else int(rng.integers(12, 120))
        hi = min(k.n, 32768 if far else 64)
        d = int(rng.integers(1, min(hi, 9) + 1)) if rng.random() < 0.3 else int(rng.integers(1, hi + 1))
        k.m(min(ln, left), d)
    assert k.n == n
    return k.t


def mk(toks, tail=None):
    """(member, data, tokens): one final dynamic block, or a dynamic block and a fixed tail."""
    D = W.Deflater()
    data = W.expand(toks)
    if tail is None:
        D.dynamic(toks, final=True)
    else:
        D.dynamic(toks, final=False)
        D.fixed(tail, final=True)
        data += W.expand(tail, data)
        toks = toks + tail
    return W.member(D.finish(), data), data, toks


def matches(toks):
    """[(start, length, distance)] of a token list."""
    out, n = [], 0
    for t in toks:
        if isinstance(t, tuple):
            out.append((n, t[0], t[1]))
            n += t[0]
        else:
            n += 1
    return out


def nibbles(toks):
    """group index -> start bits of the four bytes of the group (bit i: a match starts at 4g + i)."""
    nb = {}
    for s, _, _ in matches(toks):
        nb[s >> 2] = nb.get(s >> 2, 0) | 1 << (s & 3)
    return nb


def step_depths(toks):
    """Per byte, the number of hops its copy chain makes inside its own 512-byte step."""
    n = W.token_bytes(toks)
    src = np.arange(n)
    for s, ln, d in matches(toks):
        for x in range(s, s + ln):
            src[x] = x - d
    dep = np.zeros(n, np.int32)
    for x in range(n):
        if src[x] != x:
            dep[x] = 1 + (dep[src[x]] if src[x] >= (x & ~(STEP - 1)) else 0)
    return dep


# ---------------------------------------------------------------- the members

PH_LENS = (3, 4, 5, 8, 258)


def group_phase_tokens():
    k = Toks(11).lit(301)
    for ln in PH_LENS:
        for off in range(4):
            k.to(((k.n + 8) & ~3) + off).m(ln, 300 - ln % 7).lit(5)  # literals on both sides
    runs = []
    for ph in range(4):  # back-to-back 3-byte matches from every phase: starts at every offset,
        k.to(((k.n + 8) & ~3) + ph)  # 0 and 3 of one group among them (start bits 9)
        runs.append(k.n)
        for _ in range(9):
            k.m(3, 200 + ph)
        k.lit(2)
    squeezed = []
    for e in range(4):  # a match ending at offset e, one literal, the next match
        k.to(((k.n + 12) & ~3) - 5 + e + 1).m(5, 77)
        squeezed.append(k.n)
        k.lit(1).m(4, 91)
    k.lit(3)
    k.lit((1 - k.n) % 16)  # length 1 mod 16: 16 copies in a row start at 16 alignments
    return k.t, runs, squeezed


OV_D = (1, 2, 3, 4, 5, 7)
OV_J = (1, 2, 3, 4, 257)


def overlap_tokens():
    """Runs of distance D (overlapping: length > D) that cross a step boundary and a batch
    boundary, starting j bytes before it."""
    k = Toks(12).lit(9)
    placed = []
    b = 1
    for D in OV_D:
        for j in OV_J:
            for edge in (BATCH * b - 3 * STEP, BATCH * b):  # a step boundary, then a batch boundary
                ln = 258 if j == 257 else (258, 37, 9, 130)[(D + j) % 4]
                k.to(edge - j).m(ln, D)
                placed.append((D, j, edge, ln))
            b += 1
    k.lit(7)
    return k.t, placed


def carry_tokens():
    k = Toks(13).lit(700)
    want = {}
    for r in (1, 2, 3, 4):  # a carry ending r bytes into the batch, a new start right behind it
        e = BATCH * r
        k.to(e - 10).m(10 + r, 650).m(3 + r, 123)
        want["end%d" % r] = e
    e = BATCH * 5  # a carried match whose source lies in the previous step: near and far
    k.to(e - 5).m(40, 8)
    want["src_near"] = e
    e = BATCH * 6
    k.to(e - 2).m(30, 600)
    want["src_far"] = e
    e = BATCH * 7  # the first groups of the batch owned by the carry alone
    k.to(e - 100).m(200, 1000)
    want["own"] = e
    e = BATCH * 8  # the same with an overlapping carry of distance 3
    k.to(e - 100).m(258, 3).lit(1).m(3, 1)
    want["own_ov"] = e
    k.lit(6)
    return k.t, want


def chain_tokens():
    """Chains of matches inside one 512-byte step: each copy's source is the copy before it."""
    k = Toks(14).lit(STEP)
    want = []
    for depth, ln, seed_in_step in ((1, 6, True), (2, 5, True), (3, 4, True), (100, 4, True),
                                    (120, 3, True), (90, 5, False), (3, 3, False)):
        s = (k.n + STEP) & ~(STEP - 1)
        k.to(s if seed_in_step else s - ln)
        k.lit(ln)  # the seed: literals at the step's start, or right before the step
        for _ in range(depth):
            k.m(ln, ln)
        assert k.n <= s + STEP
        want.append((s, depth))  # (a first copy from before the step is one hop too)
        k.lit(2)
    # chains through non-adjacent matches: a copy of a copy of a copy, 40 bytes apart
    s = (k.n + STEP) & ~(STEP - 1)
    k.to(s + 3).lit(7)
    for _ in range(3):
        k.lit(33).m(7, 40)
    want.append((s, 3))
    k.lit(5)
    return k.t, want


SIZES = (1, 2, 3, 4, 5, 7, 2047, 2048, 2049, 65535, 65536)


def size_members():
    out = {}
    tiny = {1: [65], 2: [65, 66], 3: [65, 66, 67], 4: [65, (3, 1)], 5: [65, (4, 1)],
            7: [65, 66, (5, 2)]}
    for n in SIZES:
        out["size%d" % n] = mk(tiny[n] if n in tiny else rand_tokens(n, n))
    # no match at all in a full block: "no start yet" holds up to the last byte (65535); four
    # literal values, so that the member stays below BGZF's 64 KiB
    out["literals65536"] = mk(Toks(15).lit(65536, 4).t)
    # the first match of a full block in its last group
    out["late_match"] = mk(Toks(16).lit(65532, 4).m(4, 9).t)
    # a first deflate block of 1, 2, 3 mod 4 bytes ending in a match, and a small tail that starts
    # with a match into it: the block kernel resolves a prefix that cuts a group
    for r in (1, 2, 3):
        pre = rand_tokens(5000 + r - 6, 40 + r, far=False) + [(6, 5)]
        out["cut%d" % r] = mk(pre, tail=[(9, 4), 70, 71, (30, 2000), 72])
    return out


@pytest.fixture(scope="module")
def fx():
    f = {}
    t, runs, sq = group_phase_tokens()
    f["phase"] = mk(t) + ((runs, sq),)
    t, placed = overlap_tokens()
    f["overlap"] = mk(t) + (placed,)
    t, want = carry_tokens()
    f["carry"] = mk(t) + (want,)
    t, want = chain_tokens()
    f["chain"] = mk(t) + (want,)
    for name, m in size_members().items():
        f[name] = m + (None,)
    return f


def shifted(member, data, n=16):
    """n copies of a member whose length is 1 mod 16: copy i starts at output alignment i."""
    assert len(data) % 16 == 1
    return member * n, data * n


def test_fixtures_hold_their_patterns(fx):
    for name, (m, d, toks, _) in fx.items():
        assert zlib.decompress(m[18:-8], -15) == d, name
        assert W.token_bytes(toks) == len(d) and len(d) <= 65536
        # every group's start bits are one of 0, 1, 2, 4, 8, 9 (a match is >= 3 bytes)
        assert set(nibbles(toks).values()) <= {1, 2, 4, 8, 9}, name
    # group phase: every (offset in the group, length), literals on both sides
    m, d, toks, (runs, sq) = fx["phase"]
    ms = matches(toks)
    ends = {s + ln for s, ln, _ in ms}
    starts = {s for s, _, _ in ms}
    iso = {(s & 3, ln) for s, ln, _ in ms if s not in ends and s + ln not in starts}
    assert iso >= {(o, ln) for o in range(4) for ln in PH_LENS}
    nb = nibbles(toks)
    assert set(nb.values()) == {1, 2, 4, 8, 9}
    for ph, r in enumerate(runs):  # a back-to-back run from each phase holds start bits 9
        assert r & 3 == ph and all(r + 3 * i in starts for i in range(9))
        assert any(nb.get(g) == 9 for g in range(r >> 2, (r + 27) >> 2))
    for e, p in enumerate(sq):  # ... match | literal at p | match ...
        assert p in ends and p not in starts and p + 1 in starts and (p - 1) & 3 == e
    assert {p >> 2 == (p + 1) >> 2 and (p - 1) >> 2 == p >> 2 for p in sq} == {True, False}
    assert len(d) % 16 == 1
    # overlaps: every distance from every j before a step and a batch boundary, across it
    m, d, toks, placed = fx["overlap"]
    ms = {s: (ln, dist) for s, ln, dist in matches(toks)}
    seen = set()
    for D, j, edge, ln in placed:
        assert ms[edge - j] == (ln, D) and ln > D and edge - j + ln > edge
        assert edge % STEP == 0 and (edge % BATCH == 0 or edge % BATCH == STEP)
        seen.add((D, j, edge % BATCH == 0))
    assert seen == {(D, j, e) for D in OV_D for j in OV_J for e in (True, False)}
    assert {(edge - j) & 3 for _, j, edge, _ in placed} == {0, 1, 2, 3}
    assert max(ln for _, _, _, ln in placed) == 258
    # carries
    m, d, toks, want = fx["carry"]
    ms = matches(toks)
    at = {s: (ln, dist) for s, ln, dist in ms}
    for r in (1, 2, 3, 4):
        e = want["end%d" % r]
        assert e % BATCH == 0 and at[e - 10][0] == 10 + r and e + r in at
    e = want["src_near"]
    assert at[e - 5] == (40, 8) and (e - 5 - 8) // STEP == e // STEP - 1
    e = want["src_far"]
    assert at[e - 2] == (30, 600) and (e - 2 - 600) // STEP < e // STEP - 1
    for key in ("own", "own_ov"):
        e = want[key]
        s = max(s for s in at if s < e)
        assert s + at[s][0] >= e + 8 and not any(e <= x < e + 8 for x in at)
    # chains: the depths inside a step
    m, d, toks, want = fx["chain"]
    dep = step_depths(toks)
    got = {s: int(dep[s:s + STEP].max()) for s, _ in want}
    assert [got[s] for s, _ in want] == [w for _, w in want]
    assert {1, 2, 3} <= set(got.values()) and max(got.values()) >= 100
    # sizes
    for n in SIZES:
        assert len(fx["size%d" % n][1]) == n
    assert not matches(fx["literals65536"][2]) and len(fx["literals65536"][1]) == 65536
    assert [s for s, _, _ in matches(fx["late_match"][2])] == [65532]
    for r in (1, 2, 3):
        m, d, toks, _ = fx["cut%d" % r]
        ms = matches(toks)
        cut = 5000 + r
        assert cut & 3 == r and any(s + ln == cut for s, ln, _ in ms) and any(s == cut for s, _, _ in ms)
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
def test_gpu_group_phase_at_every_alignment(fx):
    m, d = fx["phase"][:2]
    _check([shifted(m, d)])


@pytest.mark.gpu
def test_gpu_overlaps_across_steps_and_batches(fx):
    m, d = fx["overlap"][:2]
    one = fx["size1"][:2]
    _check([(m, d), one, (m, d), fx["size5"][:2], (m, d)])  # alignments 0, 8 + 2, 7 + ...


@pytest.mark.gpu
def test_gpu_carries(fx):
    m, d = fx["carry"][:2]
    parts = []
    for i in range(4):  # the member's length is 6 mod 16 plus these: four alignments
        parts += [(m, d), fx["size%d" % (1, 2, 3, 7)[i]][:2]]
    _check(parts)


@pytest.mark.gpu
def test_gpu_chains_inside_a_step(fx):
    m, d = fx["chain"][:2]
    _check([(m, d), fx["size3"][:2], (m, d), fx["size2"][:2], (m, d)])


@pytest.mark.gpu
def test_gpu_sizes(fx):
    names = ["size%d" % n for n in SIZES] + ["literals65536", "late_match", "cut1", "cut2", "cut3"]
    _check([fx[n][:2] for n in names] + [fx[n][:2] for n in reversed(names)])
