"""Directed tests of the jump rounds of K2's match resolve and of their pending-state bookkeeping
(DESIGN.md section 3, round 8).

inflate_block_kernel resolves a block's matches in batches of 2048 output bytes: four chunks of
512 bytes, each one ordered step.  After the first hop a byte is pending when its source lies in
its own step; pending bytes follow their chains by pointer jumping through the batch's next
pointers.  Wave w owns bytes 64 w .. 64 w + 63 of each chunk, its four slices, one entry per lane
and slice; an entry's state is the offset of the pointer it reads next, its own when it is
final.  A wave runs a round while any of its entries is pending, and the final ones take the
round idempotently; the -DDQ_RES_SLICE=1 build keeps one bit per slice and a round reads and
updates only the slices with a pending byte.  These members put the
pending bytes where that bookkeeping can go wrong: a single live slice in each chunk and in the
first and last wave, slices of one wave that finish in different rounds (one round against six,
and a chain that only the loop after the steps ends), a chain that reads the pointers of a slice
whose wave went quiet after the first hop, batches with nothing pending and with everything
pending, the first batch (adopted outside the batch loop), last batches cut by the block's size,
a prefix in front of a deferred tail block, and every output alignment of the four-byte words.
The members are token lists written bit by bit (tests/deflate_writer.py); the CPU test checks them
against zlib and checks that each one holds the pattern it is named for, the GPU tests compare
the decompressed stream with zlib's."""
import zlib

import numpy as np
import pytest

import deflate_writer as W
from test_resolve_groups import BATCH, STEP, Toks, _check, matches, mk

SLICE = 64  # a wave's bytes of one chunk
NW = STEP // SLICE
FAR = 600  # a distance that reaches before any byte's step


def instep_depths(toks):
    """Per byte, the number of hops its copy chain makes to sources inside its own 512-byte step:
    0 for a literal and for a copy from before the step (final after the first hop), else one
    more than its source's."""
    n = W.token_bytes(toks)
    src = np.arange(n)
    for s, ln, d in matches(toks):
        for x in range(s, s + ln):
            src[x] = x - d
    dep = np.zeros(n, np.int32)
    for x in range(n):
        if src[x] != x and src[x] >= (x & ~(STEP - 1)):
            dep[x] = 1 + dep[src[x]]
    return dep, src


def live_slices(dep):
    """{(batch, chunk, wave): deepest in-step chain} of the slices that hold a pending byte."""
    out = {}
    for x in np.flatnonzero(dep):
        key = (int(x) // BATCH, int(x) % BATCH // STEP, int(x) % STEP // SLICE)
        out[key] = max(out.get(key, 0), int(dep[x]))
    return out


def rounds_of(depth):
    """Jump rounds a chain of that in-step depth inside one slice takes: the lanes of a wave read
    together, so a round doubles what a pointer skips, and one more round sees the end."""
    return 0 if depth == 0 else int(np.ceil(np.log2(depth))) + 1


def quiet(k, end):
    """Fill up to `end` with literals and copies from before their step: nothing pending."""
    while k.n < end:
        left = end - k.n
        if left >= 8 and k.n >= FAR + 40 and k.rng.random() < 0.5:
            k.m(int(k.rng.integers(3, min(left, 40) + 1)), FAR + int(k.rng.integers(0, 40)))
        else:
            k.lit(min(left, int(k.rng.integers(1, 9))))
    return k


def chain(k, end, ln=3):
    """`ln` literals, then copies of the `ln` bytes before them up to `end` exactly."""
    k.lit(ln)
    while k.n < end:
        left = end - k.n
        k.m(left if left < 2 * ln else ln, ln)
    return k


def one_slice_tokens(batch, chunk, wave, seed, size=None):
    """Exactly one live slice: a chain of 3-byte copies fills bytes 0 .. 62 of the slice."""
    s = batch * BATCH + chunk * STEP + wave * SLICE
    k = Toks(seed)
    quiet(k, s)
    chain(k, s + SLICE - 1)
    quiet(k, (batch + 1) * BATCH + 40 if size is None else size)
    return k.t


def two_speed_tokens(wave, deep):
    """In batch 1, wave `wave`'s slice of chunk 0 holds copies of literals of its step (one
    round); chunk 2 holds a chain of 3-byte copies: in that slice alone (20 deep, six rounds), or
    from the start of its step (`deep`: more than 100 deep, more rounds than the steps hold)."""
    b0 = BATCH
    k = Toks(30 + wave + 10 * deep)
    s0 = b0 + wave * SLICE
    quiet(k, s0)
    k.lit(8).m(8, 8).lit(4).m(5, 20)  # copies of literals: in-step depth 1
    if deep:
        quiet(k, b0 + 2 * STEP)
        chain(k, b0 + 3 * STEP - 2)
    else:
        quiet(k, b0 + 2 * STEP + wave * SLICE)
        chain(k, b0 + 2 * STEP + wave * SLICE + SLICE - 1)
    quiet(k, 2 * BATCH + 9)
    return k.t


def cross_slice_tokens():
    """Chunk 1 of batch 1: slice 1 is final after the first hop (literals and a copy from before
    the step), slice 5 copies 40 of its bytes (distance 256), and slice 6 copies from slice 5."""
    c = BATCH + STEP
    k = quiet(Toks(41), c + SLICE)
    k.lit(20).m(30, FAR).lit(14)  # slice 1: bytes 64 .. 127 of the chunk
    quiet(k, c + 5 * SLICE + 10)
    k.m(40, 4 * SLICE)  # from bytes 74 .. 113: literals and the far copy
    quiet(k, c + 6 * SLICE + 5)
    k.m(30, SLICE - 10)  # from the copy in slice 5: two in-step hops
    quiet(k, 2 * BATCH + 3)
    return k.t


def all_pending_tokens(steps=9):
    """Every step: 16 literals, then copies from inside the step only, distances 1 .. 15, with
    overlapping runs of distance 1, 2, 3 and 7."""
    k = Toks(42)
    for s in range(steps):
        end = (s + 1) * STEP
        k.lit(16)
        for d in (1, 2, 3, 7):
            k.m(20 + 3 * d, d)
        while k.n < end:
            left = end - k.n
            ln = int(k.rng.integers(3, 30))
            ln = left if left - ln < 3 else ln
            k.m(ln, int(k.rng.integers(1, 16)))
    return k.t


def far_only_tokens():
    """Literals, then nothing but copies from at least 512 bytes back: never pending."""
    k = Toks(43).lit(700)
    while k.n < 3 * BATCH + 100:
        k.m(int(k.rng.integers(3, 259)), int(k.rng.integers(STEP, k.n + 1)))
    return k.t


LAST = (1, 63, 65, 511, 513)  # bytes in the last batch


def last_batch_tokens(r):
    """2048 + r bytes whose last copy chain runs to the last byte: the pending bytes lie in the
    last slices the size leaves (r = 1 and 513 end one byte into a step: that byte copies from
    before its step, the pending bytes end in the slice before it)."""
    end = BATCH + r
    k = quiet(Toks(50 + r), end - min(r + 30, 62) if r in (1, 65, 513) else end - (r - 1) % SLICE - 1)
    chain(k, end)
    return k.t


def tail_prefix():
    """(prefix tokens, tail tokens): the first deflate block ends inside a batch with a chain up
    to its last byte, a small fixed block follows (the block kernel defers it: rsize < isize)."""
    end = 2 * BATCH + STEP + 2 * SLICE + 60
    k = quiet(Toks(60), end - 59)
    chain(k, end)
    return k.t, [(9, 4), 70, 71, (30, 2000), 72]


ONE = [(c, w) for c in range(4) for w in (0, NW - 1)]
TINY = {1: [65], 2: [65, 66], 3: [65, 66, 67]}


@pytest.fixture(scope="module")
def fx():
    f = {}
    for c, w in ONE:
        f["one_c%dw%d" % (c, w)] = mk(one_slice_tokens(1, c, w, 100 + 8 * c + w))
        f["first_c%dw%d" % (c, w)] = mk(one_slice_tokens(0, c, w, 200 + 8 * c + w))
    for w in (0, 3, NW - 1):
        f["speed_w%d" % w] = mk(two_speed_tokens(w, False))
    f["speed_deep"] = mk(two_speed_tokens(2, True))
    f["cross"] = mk(cross_slice_tokens())
    f["literals"] = mk(Toks(44).lit(2 * BATCH + 77).t)
    f["far_only"] = mk(far_only_tokens())
    f["all_pending"] = mk(all_pending_tokens())
    for r in LAST:
        f["last%d" % r] = mk(last_batch_tokens(r))
    pre, tail = tail_prefix()
    f["tail"] = mk(pre, tail=tail) + (len(W.expand(pre)),)
    for n, t in TINY.items():
        f["tiny%d" % n] = mk(t)
    return f


def aligned(fx, names):
    """The members `names` at each output alignment 0 .. 3 in turn; [(name or None, offset)] too."""
    parts, at, off = [], [], 0
    for a in range(4):
        for n in names:
            pad = (a - off) % 4
            if pad:
                parts.append(fx["tiny%d" % pad][:2])
                off += pad
            at.append((n, off))
            parts.append(fx[n][:2])
            off += len(fx[n][1])
    return parts, at


ALIGNED = ["one_c%dw%d" % cw for cw in ONE] + ["speed_w0", "speed_w3", "speed_w7", "speed_deep"]


def test_fixtures_hold_their_patterns(fx):
    info = {}
    for name, f in fx.items():
        m, d, toks = f[:3]
        assert zlib.decompress(m[18:-8], -15) == d, name
        assert W.token_bytes(toks) == len(d) and len(d) <= 65536 and len(m) <= 65536, name
        dep, src = instep_depths(toks)
        info[name] = (dep, src, live_slices(dep))
    # one live slice, in batch 1 and in the first batch: nothing else pending in the member
    for b, key in ((1, "one"), (0, "first")):
        for c, w in ONE:
            dep, _, live = info["%s_c%dw%d" % (key, c, w)]
            assert list(live) == [(b, c, w)] and live[b, c, w] == 20
            assert len(dep) > (b + 1) * BATCH  # a batch follows: the rounds run in the pipeline
    # two speeds in one wave: chunk 0 ends after one round, chunk 2 after six / only in the loop
    # behind the steps (a batch's steps hold four rounds)
    for w in (0, 3, NW - 1):
        live = info["speed_w%d" % w][2]
        assert live == {(1, 0, w): 1, (1, 2, w): 20}
        assert rounds_of(live[1, 0, w]) == 1 and rounds_of(live[1, 2, w]) == 6
    live = info["speed_deep"][2]
    assert live[1, 0, 2] == 1 and {k[:2] for k in live} == {(1, 0), (1, 2)}
    assert [live[1, 2, w] for w in range(NW)] == sorted(live[1, 2, w] for w in range(NW))
    assert live[1, 2, NW - 1] >= 100 and rounds_of(live[1, 2, 2]) > 4
    # a chain into a slice that was final after the first hop
    dep, src, live = info["cross"]
    assert live == {(1, 1, 5): 1, (1, 1, 6): 2}
    c = BATCH + STEP
    into = {int(src[x]) for x in range(c + 5 * SLICE, c + 6 * SLICE) if dep[x]}
    assert into and all(c + SLICE <= s < c + 2 * SLICE for s in into)
    assert {int(src[s]) == s for s in into} == {True, False}  # literals and far copies there
    assert all(src[s] == s or src[s] < c for s in into)
    # nothing pending / everything pending
    assert not matches(fx["literals"][2]) and not info["literals"][2]
    ms = matches(fx["far_only"][2])
    assert len(ms) > 20 and min(d for _, _, d in ms) >= STEP and not info["far_only"][2]
    dep, _, live = info["all_pending"]
    assert len(dep) > 2 * BATCH and all(dep[x] > 0 for x in range(len(dep)) if x % STEP >= 16)
    assert set(live) == {(x // BATCH, x % BATCH // STEP, x % STEP // SLICE) for x in range(len(dep))}
    ms = matches(fx["all_pending"][2])
    assert {d for _, _, d in ms} == set(range(1, 16))
    assert {d for _, ln, d in ms if ln > d} >= {1, 2, 3, 7}
    # last batches: the chain ends with the member
    for r in LAST:
        dep, src, live = info["last%d" % r]
        n = len(dep)
        assert n == BATCH + r and src[n - 1] != n - 1
        last = {k for k in live if k[0] == 1}
        if r in (1, 513):  # one byte into a step: it copies from before the step
            assert dep[n - 1] == 0 and dep[n - 2] > 0 and ((r - 1) // STEP, 0) not in {k[1:] for k in last}
        else:
            assert dep[n - 1] > 0 and (1, (r - 1) // STEP, (r - 1) % STEP // SLICE) in last
        assert (r == 1) == (not last)
    # the prefix of a deferred tail: pending bytes up to its last byte, a small tail behind it
    m, d, toks, cut = fx["tail"]
    dep, src, _ = info["tail"]
    live = live_slices(dep[:cut])
    assert cut % BATCH and dep[cut - 1] > 0 and max(live) == (cut // BATCH, cut % BATCH // STEP, cut % STEP // SLICE)
    assert 0 < len(d) - cut <= 4096 and any(s == cut for s, _, _ in matches(toks))
    # every alignment of every member of the first two cases
    _, at = aligned(fx, ALIGNED)
    assert {(n, o % 4) for n, o in at} == {(n, a) for n in ALIGNED for a in range(4)}


@pytest.mark.gpu
def test_gpu_one_live_slice(fx):
    _check([fx["one_c%dw%d" % cw][:2] for cw in ONE])


@pytest.mark.gpu
def test_gpu_slices_finish_in_different_rounds(fx):
    _check([fx[n][:2] for n in ("speed_w0", "speed_w3", "speed_w7", "speed_deep")])


@pytest.mark.gpu
def test_gpu_chain_into_a_quiet_slice(fx):
    _check([fx["cross"][:2], fx["tiny1"][:2], fx["cross"][:2]])


@pytest.mark.gpu
def test_gpu_nothing_and_everything_pending(fx):
    _check([fx[n][:2] for n in ("literals", "far_only", "all_pending", "far_only", "literals")])


@pytest.mark.gpu
def test_gpu_first_batch(fx):
    _check([fx["first_c%dw%d" % cw][:2] for cw in ONE])


@pytest.mark.gpu
def test_gpu_last_partial_batch(fx):
    _check([fx["last%d" % r][:2] for r in LAST] + [fx["last%d" % r][:2] for r in reversed(LAST)])


@pytest.mark.gpu
def test_gpu_prefix_of_a_deferred_tail(fx):
    _check([fx["tail"][:2], fx["tiny3"][:2], fx["tail"][:2]])


@pytest.mark.gpu
def test_gpu_output_alignments(fx):
    _check(aligned(fx, ALIGNED)[0])
