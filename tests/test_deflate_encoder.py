"""The BGZF encoder's output (dq_bgzf_compress, dq_deflate.hip) read token by token.

tests/test_deflate_gpu.py proves with zlib that the written members are valid; it cannot say which
branch of the encoder wrote them.  Here every member is read back with tests/deflate_reader.py (a
plain RFC 1951 reader: block type, header fields, run-length tokens, code lengths, matches), and
each test asserts from those that the case it is about was emitted: a code that needed the length
limiter (15 bits for the literal/length and distance codes, 7 for the code-length code), every
shape of the dynamic header's run-length coder, the one- and no-symbol distance alphabets, matches
at the ends of the match finder's reach (distance 32768, length 258, the chunk boundary at 32640,
the 13600 bytes a chunk sees before its start), and the dynamic / fixed / stored choice.

The fixtures are built so that their parse is known: either no 3-byte string repeats (a parse of
literals only, whose histogram is the byte histogram) or the only repeats are the planted copies.
Their shapes are checked on the CPU (the tests without the gpu mark), with a restatement in Python
of the kernel's code-length construction (kernel_lengths, kernel_header below: the
Moffat-Katajainen pass, the cap and Kraft fix-up, the run-length coder of bgzf_huff_kernel) where
the shape depends on it.  The GPU tests never trust that restatement for a verdict about the
fixture: they take the histograms from the emitted tokens and fail with "fixture does not reach
..." if the emitted block is not the case (they do not skip).

What is asserted of every emitted member (check_member): one final deflate block that expands to
the input; zero padding bits; BSIZE in range; no match across offset 32640 of a block, none whose
source lies more than 13600 bytes before 32640 when it starts after it, none beyond 32768; for a
dynamic block complete codes (Kraft sum exactly 1) within 15 / 7 bits whose lengths never give a
more frequent symbol a longer code, cost the Huffman optimum whenever that optimum needs no
limiting, a header that is the shortest listing (HLIT, HDIST, HCLEN minimal, the run-length tokens
the greedy ones of RFC 1951's symbols 16 / 17 / 18) and the block-type rule
`header + dynamic < 3 + fixed`, `ceil(bits / 8) <= min(65510, n + 5)`; for a fixed block the same
size rule and that a dynamic coding of the same tokens (tests/deflate_writer.py's) would not have
been shorter by more than the two encoders' header sizes differ."""
import functools
import heapq
import zlib

import numpy as np
import pytest

import bamutil as B
import deflate_reader as R
import deflate_writer as W

BLK = B.BLOCK_U            # 65280
CH = BLK // 2              # 32640: the parse kernel's chunk
XW = 13600                 # bytes a chunk sees before its start
MAX_DEFLATE = 65536 - 26


# ---------------------------------------------------------------------------------------------
# plain references

def huffman_depth(freqs):
    """The depth of a Huffman code of the nonzero frequencies: of the optimal code of least depth
    (ties merge leaves before subtrees and shallow subtrees before deep ones), so a result above a
    limit means that no optimal code fits the limit."""
    h = [(f, 0, i) for i, f in enumerate(freqs) if f > 0]
    if len(h) < 2:
        return 1
    heapq.heapify(h)
    k = len(freqs)
    while len(h) > 1:
        a = heapq.heappop(h)
        b = heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], max(a[1], b[1]) + 1, k))
        k += 1
    return h[0][1]


def huffman_cost(freqs):
    """Sum of frequency x code length of an optimal prefix code (two or more used symbols)."""
    h = [f for f in freqs if f > 0]
    heapq.heapify(h)
    cost = 0
    while len(h) > 1:
        s = heapq.heappop(h) + heapq.heappop(h)
        cost += s
        heapq.heappush(h, s)
    return cost


def kraft(lens):
    """Kraft sum in units of 2^-15."""
    return sum(1 << (15 - x) for x in lens if x)


def monotone(freqs, lens):
    """No used symbol has a longer code than a less frequent one."""
    used = sorted((f, x) for f, x in zip(freqs, lens) if f > 0)
    return all(a[1] >= b[1] for a, b in zip(used, used[1:]) if a[0] < b[0])


# ---------------------------------------------------------------------------------------------
# the kernel's code construction, restated (dq_deflate.hip build_lengths and the t == 64 block of
# bgzf_huff_kernel): used to shape fixtures on the CPU and to bound the fixed / dynamic choice

def kernel_lengths(f, maxlen):
    m = len(f)
    srt = sorted((s for s in range(m) if f[s] > 0), key=lambda s: (f[s], s))
    ln = [0] * m
    n = len(srt)
    if n < 2:
        a = srt[0] if n == 1 else 0
        ln[a] = ln[1 if a == 0 else 0] = 1
        return ln
    w = [f[s] for s in srt]
    w[0] += w[1]
    root, leaf = 0, 2
    for nxt in range(1, n - 1):
        if leaf >= n or w[root] < w[leaf]:
            w[nxt] = w[root]
            w[root] = nxt
            root += 1
        else:
            w[nxt] = w[leaf]
            leaf += 1
        if leaf >= n or (root < nxt and w[root] < w[leaf]):
            w[nxt] += w[root]
            w[root] = nxt
            root += 1
        else:
            w[nxt] += w[leaf]
            leaf += 1
    w[n - 2] = 0
    for nxt in range(n - 3, -1, -1):
        w[nxt] = w[w[nxt]] + 1
    avbl, usedn, dpth, root, nxt = 1, 0, 0, n - 2, n - 1
    while avbl > 0:
        while root >= 0 and w[root] == dpth:
            usedn += 1
            root -= 1
        while avbl > usedn:
            w[nxt] = dpth
            nxt -= 1
            avbl -= 1
        avbl, dpth, usedn = 2 * usedn, dpth + 1, 0
    cnt = [0] * (maxlen + 1)
    for x in w:
        cnt[min(x, maxlen)] += 1
    total = sum(cnt[x] << (maxlen - x) for x in range(1, maxlen + 1))
    while total != 1 << maxlen:
        cnt[maxlen] -= 1
        for x in range(maxlen - 1, 0, -1):
            if cnt[x]:
                cnt[x] -= 1
                cnt[x + 1] += 2
                break
        total -= 1
    j = n
    for x in range(1, maxlen + 1):
        for _ in range(cnt[x]):
            j -= 1
            ln[srt[j]] = x
    return ln


def rle_tokens(seq):
    """The greedy run-length tokens of a code-length sequence: zero runs as 18 (11..138) while 11
    or more are left, then one 17 (3..10), then zeros; other runs as the length, 16 (3..6) while 3
    or more are left, then the length itself."""
    out, i = [], 0
    while i < len(seq):
        v, run = seq[i], 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        r = run
        if v == 0:
            while r >= 11:
                k = min(r, 138)
                out.append((18, k - 11))
                r -= k
            if r >= 3:
                out.append((17, r - 3))
                r = 0
        else:
            out.append((v, None))
            r -= 1
            while r >= 3:
                k = min(r, 6)
                out.append((16, k - 3))
                r -= k
        out += [(v, None)] * r
        i += run
    return out


XBITS = {16: 2, 17: 3, 18: 7}


def kernel_header(ll, d):
    """(hlit, hdist, hclen, code-length-code lengths, tokens, header bits) the kernel writes for
    the 286 literal/length and 30 distance code lengths."""
    hlit, hdist = 286, 30
    while hlit > 257 and ll[hlit - 1] == 0:
        hlit -= 1
    while hdist > 1 and d[hdist - 1] == 0:
        hdist -= 1
    toks = rle_tokens(list(ll[:hlit]) + list(d[:hdist]))
    cf = [0] * 19
    for s, _ in toks:
        cf[s] += 1
    cl = kernel_lengths(cf, 7)
    hclen = 19
    while hclen > 4 and cl[W.CL_ORDER[hclen - 1]] == 0:
        hclen -= 1
    bits = 17 + 3 * hclen + sum(cl[s] + XBITS.get(s, 0) for s, _ in toks)
    return hlit, hdist, hclen, cl, toks, bits


def histograms(tokens):
    lf, df = [0] * 286, [0] * 30
    for t in tokens:
        if isinstance(t, tuple):
            lf[257 + W.len_sym(t[0])[0]] += 1
            df[W.dist_sym(t[1])[0]] += 1
        else:
            lf[t] += 1
    lf[256] += 1
    return lf, df


def body_bits(tokens, ll, d):
    """Bits of the tokens and the end-of-block code under the code lengths ll / d."""
    n = ll[256]
    for t in tokens:
        if isinstance(t, tuple):
            s, nb, _ = W.len_sym(t[0])
            n += ll[257 + s] + nb
            s, nb, _ = W.dist_sym(t[1])
            n += d[s] + nb
        else:
            n += ll[t]
    return n


def literal_parse(data):
    """The histograms of a parse that is literals only."""
    return histograms(list(data))


# ---------------------------------------------------------------------------------------------
# fixtures

def repeated_grams(data, k):
    """Positions whose k bytes occurred before."""
    seen, out = set(), []
    for i in range(len(data) - k + 1):
        g = bytes(data[i:i + k])
        if g in seen:
            out.append(i)
        seen.add(g)
    return out


def _no_repeats(a, k, rng):
    """Swap bytes of the array (its histogram stays) until no k bytes repeat."""
    a = bytearray(a)
    for _ in range(200):
        rep = repeated_grams(a, k)
        if not rep:
            return bytes(a)
        for i in rep:
            j = int(rng.integers(0, len(a)))
            a[i], a[j] = a[j], a[i]
    raise AssertionError("repeats remain")


FIB = [1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181]


def skewed_tail(seed, ntail=16, nflat=200):
    """65280 bytes: `ntail` byte values with counts 1, 2, 3, 5, 8, ... and `nflat` values sharing
    the rest evenly (which values: a random choice among the 256, so the code-length sequence has
    zero runs and few repeat runs), shuffled, then bytes swapped until no 4 bytes repeat: the
    encoder's 4-byte match key finds nothing, the parse is literals only, its literal/length code
    needs more than 15 bits and (seed 3) the code-length code of its header more than 7."""
    rng = np.random.default_rng(seed)
    vals = [int(x) for x in rng.permutation(256)]
    tail = FIB[:ntail]
    rest = BLK - sum(tail)
    counts = dict(zip(vals[:ntail], tail))
    for i, v in enumerate(vals[ntail:ntail + nflat]):
        counts[v] = rest // nflat + (i < rest % nflat)
    a = np.concatenate([np.full(c, v, np.uint8) for v, c in sorted(counts.items())])
    assert len(a) == BLK
    return _no_repeats(rng.permutation(a).tobytes(), 4, rng)


def unique_grams(n, k, rng, values=64, p=None):
    """n random bytes over `values` byte values (with probabilities p) in which no k bytes repeat."""
    seen, out = set(), bytearray()
    draws = rng.choice(values, size=4 * n + 64, p=p)
    i = 0
    while len(out) < n:
        out.append(int(draws[i]))
        i += 1
        if len(out) >= k:
            g = bytes(out[-k:])
            if g in seen:
                out.pop()
                continue
            seen.add(g)
    return out


# distances of skewed_distances are multiples of 9 (8 copied bytes and a separator): the nearest 18
# distance symbols such a distance can have, and the least number of 9-byte items that reaches each
SD_SYMS = [6] + list(range(8, 25))
SD_COUNTS = [1] + FIB[:17]  # 1, 1, 2, 3, 5, ..., 2584: 6764 copies


def skewed_distances(seed=11):
    """One block of 9-byte items, each 8 bytes and a separator byte: an item is a new random string
    or a copy of the nearest earlier occurrence of one.  The strings rotate in a queue, so a copy's
    distance is 9 x the queue's length; the queue grows from phase to phase through the lengths
    that reach the distance symbols SD_SYMS, and phase i makes SD_COUNTS[i] copies: 6764 copies
    (54 KB) whose distance histogram is Fibonacci-like over 18 symbols -- a Huffman depth of 17.
    Each separator differs from the byte after every earlier occurrence of the string before it and
    from every separator that preceded the string after it, so no match can be longer than 8 and
    none can start on a separator.  Returns (data, planted distance histogram)."""
    rng = np.random.default_rng(seed)
    plan = []          # string ids in item order
    queue, nstr = [], 0
    hist = [0] * 30
    for sym, cnt in zip(SD_SYMS, SD_COUNTS):
        k = -(-W.DBASE[sym] // 9)
        assert W.dist_sym(9 * k)[0] == sym
        while len(queue) < k:
            plan.append(nstr)
            queue.append(nstr)
            nstr += 1
        for _ in range(cnt):
            s = queue.pop(0)
            plan.append(s)
            queue.append(s)
            hist[sym] += 1
    fill = BLK - 9 * len(plan)
    assert fill >= 0
    body = unique_grams(8 * nstr + fill, 3, rng, values=256)
    strings = [bytes(body[8 * i:8 * i + 8]) for i in range(nstr)]
    out = bytearray(body[8 * nstr:])          # the filler first: it moves no distance
    after = [set() for _ in range(nstr)]      # separators that followed string s
    before = [set() for _ in range(nstr)]     # separators that preceded string s
    for i, s in enumerate(plan):
        out += strings[s]
        nxt = plan[i + 1] if i + 1 < len(plan) else None
        bad = after[s] | (before[nxt] if nxt is not None else set())
        r = next(int(x) for x in rng.permutation(256) if int(x) not in bad)
        out.append(r)
        after[s].add(r)
        if nxt is not None:
            before[nxt].add(r)
    assert len(out) == BLK
    return bytes(out), hist


def literal_only(counts, rng):
    """Bytes with the histogram `counts` ({value: count}) in which no 3 bytes repeat: no match of
    DEFLATE's minimum length exists, so every parse is literals only."""
    left = dict(counts)
    n = sum(left.values())
    for _ in range(50):
        out, seen, rem = bytearray(), set(), dict(left)
        vals = sorted(rem)
        ok = True
        while len(out) < n:
            w = np.array([rem[v] for v in vals], float)
            for _try in range(64):
                v = vals[int(rng.choice(len(vals), p=w / w.sum()))]
                g = bytes(out[-2:]) + bytes([v])
                if len(out) < 2 or g not in seen:
                    break
            else:
                ok = False
                break
            if len(out) >= 2:
                seen.add(g)
            out.append(v)
            rem[v] -= 1
            if rem[v] == 0:
                del rem[v]
                vals = sorted(rem)
        if ok:
            return bytes(out)
    raise AssertionError("no sequence without a repeated 3 bytes")


def two_values(k, n=2048, seed=0):
    """Random bytes over {0, k}: the literal/length lengths have a run of k - 1 zeros between the
    two literals and 255 - k before the end-of-block code."""
    rng = np.random.default_rng(1000 * seed + k)
    return bytes(np.where(rng.integers(0, 2, n) == 1, k, 0).astype(np.uint8))


def equal_run(m, rng, first=64, f=32):
    """2016 literal-only bytes over 63 byte values, each `f` times: with the end-of-block code 64
    symbols, 6 bits each.  The values are 1, `m` consecutive ones from `first`, and others two
    apart (a zero between them): the consecutive ones are a run of m equal lengths."""
    vals = [1] + list(range(first, first + m))
    v = 3
    while len(vals) < 63:
        if not first - 2 < v < first + m + 1:
            vals.append(v)
        v += 2
    assert len(set(vals)) == 63 and max(vals) < 256
    return literal_only({v: f for v in vals}, rng)


def alternating(rng):
    """Literal-only bytes over all 256 values whose code lengths alternate: even values 8 times as
    frequent as odd ones, so no two neighbouring literals share a length and the header needs a
    token for each of them."""
    return literal_only({v: (16 if v % 2 == 0 else 2) for v in range(256)}, rng)


def runs_of_periods(reps=8, periods=(1, 2, 3, 4)):
    """For each period p, `reps` stretches of p distinct bytes repeated to p + 258 bytes, each
    stretch over another set of p of the values 0..15 (so no 4 bytes of one occur in another): the
    parse is p literals and one (258, p) match each, the length symbol 285 and the distance
    symbols 0..3 are the only ones used, and equally often; 16 literal values keep the dynamic
    header short enough to beat the fixed code."""
    import itertools
    out = bytearray()
    sets = {p: itertools.combinations(range(16), p) for p in periods}
    for r in range(reps):
        for p in periods:
            pat = bytes(next(sets[p]))
            out += (pat * (258 // p + 2))[:p + 258]
    return bytes(out)


def alphabet_gaps():
    """{name: bytes}: the header run-length coder's cases, one small block each."""
    rng = np.random.default_rng(17)
    out = {}
    for k in range(2, 256):
        out["0,%d" % k] = two_values(k)
    out["255 only"] = bytes([255]) * 3000
    out["0 only"] = bytes(3000)
    for m in (4, 7, 8, 9, 10, 11):
        out["run %d" % m] = equal_run(m, rng)
    out["seam"] = runs_of_periods()
    out["alternating"] = alternating(rng)
    return out


@functools.lru_cache(maxsize=None)
def _background(seed, n):
    return bytes(unique_grams(n, 4, np.random.default_rng(seed)))


def background(seed, n=BLK):
    """n bytes over 64 values (6 bits a byte: the block is not stored) in which no 4 bytes repeat:
    the match finder's 4-byte key finds nothing but what is planted."""
    return bytearray(_background(seed, n))


def plant(buf, d, l, at):
    """Copy l bytes at distance d to offset `at` of the bytearray, and make the bytes before and
    after the copy differ from those around its source, so the match is exactly (l, d)."""
    assert at - d >= 0 and at + l < len(buf)
    if at - d - 1 >= 0 and buf[at - 1] == buf[at - d - 1]:
        buf[at - 1] ^= 1
    for i in range(l):
        buf[at + i] = buf[at + i - d]
    if buf[at + l] == buf[at + l - d]:
        buf[at + l] ^= 1
    return buf


def planted(d, l, at, seed=0):
    return bytes(plant(background(100 + seed), d, l, at))


FAR = 51808  # CH - XW + 32768: the first offset of a block whose chunk holds a source 32768 back

# name: (d, l, at)
PLANTS = {
    "d1": (1, 40, FAR + 100), "d2": (2, 40, FAR + 100), "d3": (3, 40, FAR + 100),
    "d4": (4, 40, FAR + 100),
    "d32767": (32767, 40, FAR), "d32768": (32768, 40, FAR), "d32769": (32769, 40, FAR + 1),
    "d32768 late": (32768, 40, BLK - 41),
    "l3": (700, 3, 60000), "l4": (700, 4, 60000), "l257": (700, 257, 60000),
    "l258": (700, 258, 60000), "l259": (700, 259, 60000), "l600": (700, 600, 60000),
    "cross": (5000, 200, CH - 100), "cross 1": (5000, 200, CH - 1), "cross 3": (5000, 200, CH - 3),
    "cross 199": (5000, 200, CH - 199),
    "reach 13599": (XW - 1, 100, CH), "reach 13600": (XW, 100, CH), "reach 13601": (XW + 1, 100, CH),
}


def full_alphabets(seed=2):
    """One block with a planted copy for each of the 29 length symbols and 30 distance symbols
    (copy i has a length of length symbol i -- 4 for symbol 0 -- and a distance of distance
    symbol i; the 30th copy a distance of symbol 29)."""
    buf = background(300 + seed)
    rng = np.random.default_rng(seed)
    # (a stretch of two byte values, clear of every copy's source: its dense matches are cut short
    # where the parse's segments merge, which is where matches of length 3 come from -- a 3-byte
    # copy of its own is below the match finder's 4-byte key)
    buf[2000:10000] = np.where(rng.integers(0, 2, 8000) == 1, 200, 201).astype(np.uint8).tobytes()
    plants, at = [], 33000
    for i in range(30):
        ls = min(i, 28)
        l = W.LBASE[ls] + (int(rng.integers(0, 1 << W.LEXT[ls])) if W.LEXT[ls] else 0)
        l = max(l, 4)  # (a 3-byte copy is below the match finder's key; symbol 257 is not planted)
        hi = W.DBASE[i + 1] - 1 if i < 29 else 32768
        d = int(rng.integers(W.DBASE[i], hi + 1))
        d = min(d, at - (CH - XW))
        assert W.dist_sym(d)[0] == i
        plant(buf, d, l, at)
        plants.append((l, d, at))
        at += l + 300 + 40 * i
    assert at < BLK
    return bytes(buf), plants


def header_worst_case(seed=3):
    """One block whose dynamic header needs a token for every one of its 286 + 30 code lengths, the
    316 that exactly fill the kernel's token area: neighbouring symbols' lengths differ, or are
    equal for at most three in a row (two zeros), too few for a repeat token.
    Literals: all 256 values, the even ones 8 times as frequent as the odd ones, no 4 bytes
    repeating.  Planted copies: the length symbols 258..285 and the distance symbols 0..29, eight (or
    nine) copies of each even symbol and one of each odd symbol; the length symbol 257 stays
    unused (length 0 between the end-of-block code and 258).  Returns (data, [(l, d, at)])."""
    rng = np.random.default_rng(seed)
    w = np.where(np.arange(256) % 2 == 0, 8.0, 1.0)
    buf = bytearray(unique_grams(BLK, 4, rng, values=256, p=w / w.sum()))
    dsyms = [i for i in range(30) for _ in range(8 if i % 2 == 0 else 1)]
    lsyms = [j for j in range(1, 29) for _ in range(8 if j % 2 == 0 else 1)]
    lsyms += list(range(2, 29, 3))[:len(dsyms) - len(lsyms)]
    assert len(lsyms) == len(dsyms) == 135
    lsyms = [lsyms[int(i)] for i in rng.permutation(len(lsyms))]
    plants, at = [], 1000
    for ds, ls in zip(dsyms, lsyms):  # (ascending distance symbols: the far ones late in the block)
        l = max(4, W.LBASE[ls] + (int(rng.integers(0, 1 << W.LEXT[ls])) if W.LEXT[ls] else 0))
        assert W.len_sym(l)[0] == ls
        if at < CH + 8 and at + l + 8 > CH:  # (no copy across the chunk boundary)
            at = CH + 8
        hi = min(W.DBASE[ds + 1] - 1 if ds < 29 else 32768, at - (CH - XW) if at >= CH else at - 8)
        # (a source clear of the earlier copies, its first 36 bytes clear of their sources too: the
        # search at the copy's start has one candidate, at distance d)
        d = next(d for d in (int(x) for x in rng.permutation(np.arange(W.DBASE[ds], hi + 1)))
                 if d <= l or all((at - d + l + 4 <= a or a + m + 4 <= at - d) and
                                  (at - d + 36 <= a - e or a - e + m + 4 <= at - d)
                                  for m, e, a in plants))
        plant(buf, d, l, at)
        plants.append((l, d, at))
        at += l + 270  # (a gap that can hold any copy's source)
    assert at < BLK
    return bytes(buf), plants


def planned_tokens(data, plants):
    """The parse that takes exactly the planted copies and literals elsewhere."""
    toks, p = [], 0
    for l, d, at in sorted(plants, key=lambda x: x[2]):
        toks += list(data[p:at]) + [(l, d)]
        p = at + l
    return toks + list(data[p:])


def structured():
    """{name: bytes} of highly compressible blocks: none may be stored."""
    rng = np.random.default_rng(23)
    out = {"one byte": b"\x5a" * (2 * BLK)}
    for p in (2, 5, 31, 32, 33, 1021):
        pat = rng.integers(0, 256, p, dtype=np.uint8).tobytes()
        out["period %d" % p] = (pat * (2 * BLK // p + 1))[:2 * BLK]
    out["run then noise"] = b"\x00" * 50000 + rng.integers(0, 256, 15280, dtype=np.uint8).tobytes()
    lit = bytes(unique_grams(600, 3, rng, values=256))
    rep = rng.integers(0, 256, 258, dtype=np.uint8).tobytes()
    out["600 literals between matches"] = ((rep + lit) * 77)[:BLK]
    out["two symbols"] = bytes(np.where(rng.integers(0, 2, BLK) == 1, 65, 67).astype(np.uint8))
    return out


def tiny_inputs():
    """1..64 bytes below 144 (8-bit fixed codes): fixed costs n + 2 bytes, stored n + 5, and a
    dynamic header alone is longer than the 10 bits a shorter code could save per few bytes."""
    rng = np.random.default_rng(29)
    return [rng.integers(0, 144, n, dtype=np.uint8).tobytes() for n in range(1, 65)]


# ---------------------------------------------------------------------------------------------
# fixture shapes (no GPU)

def zlib5(data):
    z = zlib.compressobj(5, zlib.DEFLATED, -15)
    return len(z.compress(data) + z.flush())


@pytest.mark.parametrize("ntail,nflat", [(16, 200), (18, 100)])
def test_skewed_tail_shape(ntail, nflat):
    data = skewed_tail(3, ntail, nflat)
    assert len(data) == BLK
    lf, df = literal_parse(data)
    counts = sorted(c for c in lf[:256] if c)
    for c in FIB[:ntail]:
        counts.remove(c)
    assert len(counts) == nflat and counts[-1] - counts[0] <= 1
    depth = huffman_depth(lf)
    rep4 = len(repeated_grams(data, 4))
    z = zlib5(data)
    print("depth", depth, "repeated 4-grams", rep4, "zlib level 5", z)
    assert depth >= 17
    assert rep4 <= 16
    assert z < BLK + 5
    # what the kernel's construction makes of a literal-only parse: both limiters at work
    ll = kernel_lengths(lf, 15)
    assert max(ll) == 15 and kraft(ll) == 1 << 15 and monotone(lf, ll)
    hlit, hdist, hclen, cl, toks, bits = kernel_header(ll, kernel_lengths(df, 15))
    cf = [0] * 19
    for s, _ in toks:
        cf[s] += 1
    print("code-length code: histogram", cf, "depth", huffman_depth(cf), "lengths", cl)
    assert huffman_depth(cf) >= 8 and max(cl) == 7 and kraft(cl) == 1 << 15


def test_skewed_distances_shape():
    data, hist = skewed_distances()
    assert len(data) == BLK
    assert sorted(c for c in hist if c) == sorted(SD_COUNTS) and sum(hist) == 6764
    assert huffman_depth(hist) >= 17
    d = kernel_lengths(hist, 15)
    assert max(d) == 15 and kraft(d) == 1 << 15
    # every copy's nearest earlier occurrence is where it was planned, and nothing else repeats:
    # the 4 bytes at an item's start occur before it exactly when it is a copy
    last, copies, dh = {}, 0, [0] * 30
    off = BLK % 9
    for p in range(len(data) - 3):
        g = data[p:p + 4]
        if g in last:
            assert (p - off) % 9 <= 4, p  # repeats only inside items (their 8 bytes)
            if (p - off) % 9 == 0:
                copies += 1
                dh[W.dist_sym(p - last[g])[0]] += 1
        last[g] = p
    assert copies == 6764 and dh == hist
    assert zlib5(data) < BLK // 2


def test_alphabet_gaps_shape():
    fx = alphabet_gaps()
    assert all(len(v) <= 4200 for k, v in fx.items() if k != "seam") and len(fx["seam"]) < 9000
    for k in range(2, 256):
        assert set(fx["0,%d" % k]) == {0, k}
    seen = set()
    for m in (4, 7, 8, 9, 10, 11):
        data = fx["run %d" % m]
        assert not repeated_grams(data, 3)
        lf, df = literal_parse(data)
        ll = kernel_lengths(lf, 15)
        assert ll[64:64 + m] == [6] * m and ll[63] == ll[64 + m] == 0
        toks = kernel_header(ll, kernel_lengths(df, 15))[4]
        seen |= {t for t in toks if t[0] == 16}
    assert {(16, 0), (16, 3)} <= seen  # repeats of 3 and of 6
    data = fx["alternating"]
    assert not repeated_grams(data, 3)
    lf, df = literal_parse(data)
    ll = kernel_lengths(lf, 15)
    assert all(a != b for a, b in zip(ll[:257], ll[1:257]))
    toks = kernel_header(ll, kernel_lengths(df, 15))[4]
    assert len(toks) >= 257 + 2
    # the seam: the planned parse (p literals, one (258, p) match per stretch)
    toks = []
    data = fx["seam"]
    p = 0
    for r in range(8):
        for per in (1, 2, 3, 4):
            toks += list(data[p:p + per]) + [(258, per)]
            p += per + 258
    assert W.expand(toks) == data
    lf, df = histograms(toks)
    ll, d = kernel_lengths(lf, 15), kernel_lengths(df, 15)
    assert d[:4] == [2, 2, 2, 2] and ll[285] == 2 and ll[284] == 0
    hdr = kernel_header(ll, d)
    assert hdr[4][-2:] == [(2, None), (16, 1)]  # the repeat covers the four distance lengths
    assert hdr[5] + body_bits(toks, ll, d) < 3 + body_bits(toks, W.FIXED_LL, W.FIXED_D)


def test_planted_shape():
    for name, (d, l, at) in PLANTS.items():
        data = planted(d, l, at)
        assert len(data) == BLK
        assert data[at:at + l] == bytes(W.expand([(l, d)], data[:at])), name
        assert data[at + l] != data[at + l - d] and data[at - 1] != data[at - 1 - d], name
        rep = repeated_grams(data, 4)
        # the only repeated 4 bytes are the copy's (and, for l < 4, none)
        assert all(at <= p <= at + l - 4 for p in rep), (name, rep[:5])
        assert len(rep) == max(0, l - 3), name
        assert zlib5(data) < BLK


def test_full_alphabets_shape():
    data, plants = full_alphabets()
    assert len(data) == BLK
    assert {W.len_sym(l)[0] for l, d, at in plants} == set(range(1, 29))
    assert {W.dist_sym(d)[0] for l, d, at in plants} == set(range(30))
    assert zlib5(data) < BLK
    for l, d, at in plants:
        assert data[at:at + l] == W.expand([(l, d)], data[:at]) and at - d >= CH - XW
    # nothing repeats but the copies and the two-value stretch
    inside = [(at, at + l) for l, d, at in plants] + [(2000, 10000)]
    assert all(any(a <= p < b for a, b in inside) for p in repeated_grams(data, 4))


def test_header_worst_case_shape():
    data, plants = header_worst_case()
    toks = planned_tokens(data, plants)
    assert W.expand(toks) == data
    inside = [(at, at + l) for l, d, at in plants]
    assert all(any(a <= p < b for a, b in inside) for p in repeated_grams(data, 4))
    for l, d, at in plants:  # the search at a copy's start has one candidate
        assert d <= l or data.count(data[at:at + 4], 0, at + 3) == 1, (l, d, at)
    lf, df = histograms(toks)
    assert all(df) and all(lf[258:286]) and not lf[257]
    ll, d = kernel_lengths(lf, 15), kernel_lengths(df, 15)
    hdr = kernel_header(ll, d)
    assert len(hdr[4]) == 316 and all(s < 16 for s, _ in hdr[4])  # no run worth a repeat token
    assert hdr[5] + body_bits(toks, ll, d) < 3 + body_bits(toks, W.FIXED_LL, W.FIXED_D)
    assert zlib5(data) < BLK


def test_structured_shape():
    for name, data in structured().items():
        for a in range(0, len(data), BLK):
            blk = data[a:a + BLK]
            assert zlib5(blk) < len(blk) // 2, name


def test_tiny_shape():
    t = tiny_inputs()
    assert [len(x) for x in t] == list(range(1, 65)) and max(max(x) for x in t) < 144


# ---------------------------------------------------------------------------------------------
# the encoder's output (GPU)

class Encoder:
    """dq_bgzf_compress on one context; outputs kept by input, so the read-back test inflates
    what the other tests inspected."""

    def __init__(self):
        from disq_amd import _lib
        self.c = _lib.Context()
        self.done = {}

    def __call__(self, data):
        if data not in self.done:
            self.done[data] = self.c.bgzf_compress(data)
        return self.done[data]

    def close(self):
        self.c.close()


@pytest.fixture(scope="module")
def enc():
    e = Encoder()
    yield e
    e.close()


def positions(tokens):
    """(offset, token) of every token."""
    out, p = [], 0
    for t in tokens:
        out.append((p, t))
        p += t[0] if isinstance(t, tuple) else 1
    return out


def check_dynamic(blk, n):
    lf, df = histograms(blk.tokens)
    ll, d = blk.ll_lens + [0] * (286 - blk.hlit), blk.d_lens + [0] * (30 - blk.hdist)
    cf = [0] * 19
    for s, _ in blk.header:
        cf[s] += 1
    # complete codes within the limits, shortest codes to the most frequent symbols
    for name, f, x, lim in (("literal/length", lf, ll, 15), ("distance", df, d, 15),
                            ("code-length", cf, blk.cl_lens, 7)):
        assert max(x) <= lim, (name, x)
        assert kraft(x) == 1 << 15, (name, "Kraft sum", kraft(x) / 32768.0)
        assert monotone(f, x), (name, f, x)
        used = [s for s in range(len(f)) if f[s]]
        assert all(x[s] for s in used), (name, "a used symbol without a code")
        if len(used) >= 2:
            assert all(f[s] for s in range(len(f)) if x[s]), (name, "a code for an unused symbol")
            if huffman_depth(f) <= lim:  # no limiting needed: the optimum
                assert sum(f[s] * x[s] for s in used) == huffman_cost(f), name
        else:
            assert sorted(v for v in x if v) == [1, 1], (name, x)
    # the header lists no more than it must, in the greedy run-length tokens
    assert blk.hlit == 257 or blk.ll_lens[-1], blk.hlit
    assert blk.hdist == 1 or blk.d_lens[-1], blk.hdist
    assert blk.hclen == 4 or blk.cl_lens[W.CL_ORDER[blk.hclen - 1]], blk.hclen
    assert blk.header[0][0] != 16
    assert blk.header == rle_tokens(blk.ll_lens + blk.d_lens)
    assert len(blk.header) <= 316
    # dynamic was the shorter coding, and it fits
    hdr, dyn = blk.data - blk.start, blk.end - blk.data
    assert dyn == body_bits(blk.tokens, ll, d)
    assert hdr == 17 + 3 * blk.hclen + sum(blk.cl_lens[s] + XBITS.get(s, 0) for s, _ in blk.header)
    assert hdr + dyn < 3 + body_bits(blk.tokens, W.FIXED_LL, W.FIXED_D), "fixed would be shorter"
    assert (hdr + dyn + 7) // 8 <= min(MAX_DEFLATE, n + 5)


def reference_dynamic(tokens):
    """(header bits, all bits) of tests/deflate_writer.py's dynamic coding of the tokens with
    Huffman lengths of their own histograms."""
    lf, df = histograms(tokens)
    D = W.Deflater()
    D.dynamic(tokens, final=True, lens=(W.limited_lengths(lf, 15), W.limited_lengths(df, 15)))
    b = R.read(D.finish())[0]
    assert b.tokens == tokens
    return b.data - b.start, b.end - b.start


def fixed_undercut(blk):
    """For a fixed block: (bits by which the reference writer's dynamic coding of the same tokens
    is shorter, bits by which the kernel's dynamic header is longer than the reference's).  The
    kernel codes fixed when header + body >= 3 + fixed; both encoders' bodies cost the Huffman
    optimum (no limiting at these depths), so the first number can exceed the second only if the
    kernel chose fixed against its own rule."""
    lf, df = histograms(blk.tokens)
    assert huffman_depth(lf) <= 15 and huffman_depth(df) <= 15
    ref_hdr, ref_all = reference_dynamic(blk.tokens)
    mine = kernel_header(kernel_lengths(lf, 15), kernel_lengths(df, 15))[5]
    return (blk.end - blk.start) - ref_all, mine - ref_hdr


def check_member(data, member):
    """Everything that holds for any member the encoder writes; returns its deflate block."""
    body, crc, isize = member
    n = len(data)
    assert isize == n and crc == zlib.crc32(data) & 0xffffffff
    assert zlib.decompress(body, -15) == data
    assert 18 + len(body) + 8 <= 65536
    blocks = R.read(body)
    assert len(blocks) == 1 and blocks[0].final and blocks[0].start == 0
    blk = blocks[0]
    assert W.expand(blk.tokens) == data
    assert len(body) == (blk.end + 7) // 8
    pad = 8 * len(body) - blk.end
    assert pad == 0 or body[-1] >> (8 - pad) == 0, "padding bits"
    for p, t in positions(blk.tokens):
        if isinstance(t, tuple):
            assert 3 <= t[0] <= 258 and 1 <= t[1] <= 32768, (p, t)
            assert not p < CH < p + t[0], ("a match across the chunk boundary", p, t)
            assert p < CH or p - t[1] >= CH - XW, ("a source before the chunk's reach", p, t)
    if blk.btype == 2:
        check_dynamic(blk, n)
    elif blk.btype == 1:
        assert (blk.end + 7) // 8 <= min(MAX_DEFLATE, n + 5)
        under, allowed = fixed_undercut(blk)
        assert under <= allowed, ("dynamic would be shorter", under, allowed)
    else:
        assert len(body) == n + 5
    return blk


def encode(enc, data):
    """The deflate blocks of the members the encoder writes for `data`, all checked."""
    ms = R.members(enc(data))
    parts = [data[a:a + BLK] for a in range(0, len(data), BLK)]
    assert len(ms) == len(parts)
    return [check_member(p, m) for p, m in zip(parts, ms)]


def limiter_reached(name, freqs, lens, lim):
    depth = huffman_depth(freqs)
    print(name, "plain Huffman depth", depth, "emitted maximum", max(lens))
    assert depth > lim, "fixture does not reach the limiter: %s depth %d" % (name, depth)
    assert max(lens) == lim, (name, max(lens))
    assert kraft(lens) == 1 << 15 and monotone(freqs, lens), name


@pytest.mark.gpu
@pytest.mark.parametrize("ntail,nflat", [(16, 200), (18, 100)])
def test_gpu_limits_litlen_and_code_length_codes(enc, ntail, nflat):
    """skewed_tail: the emitted literal/length code is capped at 15 bits and the code-length code
    at 7, both complete and monotone, for histograms (tallied from the emitted block) whose
    Huffman codes are deeper."""
    blk, = encode(enc, skewed_tail(3, ntail, nflat))
    assert blk.btype == 2, "fixture does not reach the limiter: block type %d" % blk.btype
    lf, df = histograms(blk.tokens)
    limiter_reached("literal/length", lf, blk.ll_lens, 15)
    cf = [0] * 19
    for s, _ in blk.header:
        cf[s] += 1
    limiter_reached("code-length", cf, blk.cl_lens, 7)


@pytest.mark.gpu
def test_gpu_limits_distance_code(enc):
    """skewed_distances: the planted copies are found at their distances (the emitted distance
    histogram is the planted one, but for a copy cut at the chunk boundary), and the distance code
    is capped at 15 bits."""
    data, hist = skewed_distances()
    blk, = encode(enc, data)
    assert blk.btype == 2, "fixture does not reach the limiter: block type %d" % blk.btype
    lf, df = histograms(blk.tokens)
    print("planted", hist, "emitted", df)
    limiter_reached("distance", df, blk.d_lens, 15)
    assert sum(abs(a - b) for a, b in zip(df, hist)) <= 2


@pytest.mark.gpu
def test_gpu_header_run_length_coder(enc):
    """alphabet_gaps: every block dynamic, its header checked by check_dynamic; across the sweep
    every shape of run the coder can emit occurs."""
    pairs, zeros_after_138, seam = set(), [], []
    longest = 0
    for name, data in alphabet_gaps().items():
        blk, = encode(enc, data)
        assert blk.btype == 2, (name, blk.btype)
        pairs |= {t for t in blk.header if t[0] >= 16}
        i = 0
        for a, b in zip(blk.header, blk.header[1:] + [None]):
            if a == (18, 127) and b == (0, None):
                zeros_after_138.append(name)
            if a[0] == 16 and i <= blk.hlit < i + R.header_run(a):
                seam.append(name)
            i += R.header_run(a)
        longest = max(longest, len(blk.header))
        if name == "alternating":
            assert len(blk.header) >= 259, len(blk.header)
        if name.startswith("run "):
            m = int(name[4:])
            assert blk.ll_lens[64:64 + m] == [blk.ll_lens[64]] * m and not blk.ll_lens[63]
    print("header tokens at most", longest, "seam", seam, "zeros after 18/138", zeros_after_138)
    assert {(17, c - 3) for c in range(3, 11)} <= pairs
    assert {(18, 0), (18, 127)} <= pairs and any(s == 18 and 0 < x < 127 for s, x in pairs)
    assert {(16, 0), (16, 3)} <= pairs
    assert zeros_after_138
    assert "seam" in seam


@pytest.mark.gpu
def test_gpu_header_worst_case(enc):
    """header_worst_case: 316 header tokens, one per code length, the most the kernel's token area
    holds; the planted copies are the block's only matches."""
    data, plants = header_worst_case()
    blk, = encode(enc, data)
    assert blk.btype == 2
    got = [(t[0], t[1], p) for p, t in positions(blk.tokens) if isinstance(t, tuple)]
    print("header tokens", len(blk.header), "matches", len(got), "planted", len(plants))
    assert len(blk.header) == 316, "fixture does not reach the worst case: %d" % len(blk.header)
    assert blk.hlit == 286 and blk.hdist == 30 and all(s < 16 for s, _ in blk.header)
    assert got == plants


@pytest.mark.gpu
def test_gpu_degenerate_distance_alphabets(enc):
    """No match at all: distance lengths [1, 1] (two codes, none used).  Matches at distance 1
    only: two 1-bit codes, the second unused.  zlib (check_member) and this library inflate both."""
    from test_tail_handoff import _gpu_inflate
    lit = alphabet_gaps()["run 7"]
    run = alphabet_gaps()["0 only"]
    a, = encode(enc, lit)
    assert a.btype == 2 and not any(isinstance(t, tuple) for t in a.tokens)
    assert a.d_lens == [1, 1] and a.hdist == 2
    b, = encode(enc, run)
    assert b.btype == 2 and {t[1] for t in b.tokens if isinstance(t, tuple)} == {1}
    assert b.d_lens == [1, 1] and histograms(b.tokens)[1][1] == 0
    got = _gpu_inflate(enc(lit) + enc(run) + B.EOF_BLOCK)
    assert got.tobytes() == lit + run


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PLANTS))
def test_gpu_match_extremes(enc, name):
    """One planted copy in bytes where nothing else repeats: found exactly where the match finder
    can reach it, cut at length 258 and at the chunk boundary, and not found beyond distance 32768
    or 13600 bytes before the second chunk."""
    d, l, at = PLANTS[name]
    data = planted(d, l, at)
    blk, = encode(enc, data)
    assert blk.btype == 2
    pos = dict(positions(blk.tokens))
    inside = {p: t for p, t in pos.items() if isinstance(t, tuple) and at - 3 <= p < at + l}
    print(name, "tokens at the plant", sorted(inside.items()))
    if d > 32768:
        assert not inside
    elif name == "reach 13601":
        assert pos[at] == data[at] and (l, d) not in inside.values()
    elif l < 4:
        # (a 3-byte copy whose 4th byte differs is not under the match finder's 4-byte key)
        assert all(t[0] == 3 for t in inside.values())
    else:
        # the copy in pieces: cut at the chunk boundary and every 258 bytes; a piece under 4
        # bytes at a chunk's end is literals
        p, want = at, {}
        while p < at + l:
            end = min(at + l, CH if p < CH else BLK, p + 258)
            if end - p >= 4:
                want[p] = (end - p, d)
            p = end
        for p, t in want.items():
            assert pos.get(p) == t, (p, t, pos.get(p))
        if l >= 258:
            assert any(t[0] == 258 for t in inside.values())


@pytest.mark.gpu
def test_gpu_full_alphabets(enc):
    data, plants = full_alphabets()
    blk, = encode(enc, data)
    assert blk.btype == 2
    pos = positions(blk.tokens)
    got = {(t[0], t[1], p) for p, t in pos if isinstance(t, tuple)}
    missing = [t for t in plants if t not in got]
    assert not missing, missing
    lf, df = histograms(blk.tokens)
    assert all(df), df
    assert all(lf[257:286]), lf[257:286]
    assert blk.hlit == 286 and blk.hdist == 30


@pytest.mark.gpu
def test_gpu_tiny_inputs_are_fixed(enc):
    """Inputs of 1..64 bytes come out as fixed blocks, and a dynamic coding of the same tokens
    (the reference writer's) is never shorter than the fixed one by more than the kernel's header
    is longer than the reference's (check_member asserts it for each; printed here).  Measured on
    an MI355X: the reference's dynamic coding is 240 to 314 bits LONGER than the fixed block for
    every one of the 64 inputs (it never undercuts; its header lists every length without
    run-length tokens), the kernel's header would be 63 to 231 bits shorter than the reference's,
    and the assertion `undercut <= header difference` holds with at least 83 bits to spare."""
    worst = []
    for data in tiny_inputs():
        blk, = encode(enc, data)
        assert blk.btype == 1, (len(data), blk.btype)
        worst.append(fixed_undercut(blk))
    print("fixed - reference dynamic bits", min(u for u, a in worst), "..", max(u for u, a in worst),
          "kernel header - reference header", min(a for u, a in worst), "..",
          max(a for u, a in worst), "allowed - undercut (min)", min(a - u for u, a in worst))


@pytest.mark.gpu
def test_gpu_structured_blocks_are_never_stored(enc):
    kinds = {}
    for name, data in structured().items():
        blocks = encode(enc, data)
        assert all(b.btype != 0 for b in blocks), (name, [b.btype for b in blocks])
        kinds[name] = [b.btype for b in blocks]
        for b, a in zip(blocks, range(0, len(data), BLK)):
            n = len(data[a:a + BLK])
            assert (b.end + 7) // 8 < n // 2, (name, b.end // 8)
    print(kinds)


@pytest.mark.gpu
def test_gpu_reads_back_its_own_output(enc):
    """The encoder's 15-bit literal/length and distance codes, 7-bit code-length codes, full
    alphabets, two-code distance alphabets and distance 32768, through this library's inflate."""
    from test_tail_handoff import _gpu_inflate
    fx = [skewed_tail(3), skewed_tail(3, 18, 100), skewed_distances()[0], full_alphabets()[0],
          alphabet_gaps()["run 7"], alphabet_gaps()["0 only"], alphabet_gaps()["seam"],
          alphabet_gaps()["alternating"], alphabet_gaps()["0,140"]]
    fx += [planted(*PLANTS[k]) for k in ("d32768", "d32767", "d32768 late", "l258", "cross")]
    fx.append(header_worst_case()[0])
    z = b"".join(enc(x) for x in fx)
    got = _gpu_inflate(z + B.EOF_BLOCK)
    want = b"".join(fx)
    assert len(got) == len(want) and got.tobytes() == want
