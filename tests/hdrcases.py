"""Test helper: dynamic DEFLATE block headers written token by token, for the serial header decoder
(disq_amd/csrc/dq_hdr_core.h) and the header pre-pass of the inflate kernels.

deflate_writer.Deflater.dynamic() sends every code length as a literal length symbol; the cases here
need chosen HLIT / HDIST / HCLEN values, repeat symbols (16, 17, 18) with chosen runs, and headers
RFC 1951 forbids.  header() writes exactly the fields it is given; rle() and expand() convert
between a length sequence and header tokens ((symbol, extra value), extra None for 0..15, the
format of deflate_reader.Block.header).  Test infrastructure only."""
import deflate_writer as W

NONE, DYN, ERR = 0, 1, 2           # dq_hdr_core.h: HDR_NONE, HDR_DYN, HDR_ERR
BAD_TABLE, OVERREAD = 4, 8         # dq_internal.h: ST_BAD_TABLE, ST_OVERREAD


def expand(toks):
    """The code lengths the header tokens stand for (a 16 before any length repeats None)."""
    out = []
    for s, x in toks:
        if s < 16:
            out.append(s)
        elif s == 16:
            out += [out[-1] if out else None] * (3 + x)
        else:
            out += [0] * ((3 if s == 17 else 11) + x)
    return out


def rle(seq):
    """Greedy header tokens of a length sequence: 18 / 17 for zero runs, 16 for repeats."""
    toks, i = [], 0
    while i < len(seq):
        v, n = seq[i], 1
        while i + n < len(seq) and seq[i + n] == v:
            n += 1
        if v == 0 and n >= 3:
            k = min(n, 138)
            toks.append((18, k - 11) if k >= 11 else (17, k - 3))
            i += k
        elif v != 0 and n >= 4:
            toks.append((v, None))
            k = min(n - 1, 6)
            toks.append((16, k - 3))
            i += 1 + k
        else:
            toks.append((v, None))
            i += 1
    return toks


def cl_for(toks, force=()):
    """Complete code-length-code lengths (<= 7 bits) for the symbols the tokens use (and `force`)."""
    f = [0] * 19
    for s, _ in toks:
        f[s] += 1
    for s in force:
        f[s] += 1
    return W.limited_lengths(f, 7)


def header(w, hlit, hdist, toks, cl=None, hclen=None, final=False):
    """Write a dynamic block header into BitWriter `w`: the fields as given (HLIT 257..288,
    HDIST 1..32, HCLEN 4..19; nothing is checked), the code-length code `cl` (19 lengths by symbol,
    default: a complete code for the tokens) and the tokens."""
    cl = cl_for(toks) if cl is None else cl
    if hclen is None:
        hclen = max(4, max(i for i, s in enumerate(W.CL_ORDER) if cl[s]) + 1)
    w.bits(int(final), 1)
    w.bits(2, 2)
    w.bits(hlit - 257, 5)
    w.bits(hdist - 1, 5)
    w.bits(hclen - 4, 4)
    for s in W.CL_ORDER[:hclen]:
        w.bits(cl[s], 3)
    codes = W.canonical(cl)
    for s, x in toks:
        w.code(codes[s], cl[s])
        if s >= 16:
            w.bits(x, {16: 2, 17: 3, 18: 7}[s])


def block(D, toks, ll, dl, htoks=None, cl=None, hclen=None, hlit=None, hdist=None, final=False):
    """Append a dynamic block to Deflater `D`: this module's header (tokens default to rle() of the
    lengths), then the data tokens and the end-of-block code under (ll, dl)."""
    hlit = max(257, max(i for i, x in enumerate(ll) if x) + 1) if hlit is None else hlit
    hdist = max(1, max((i for i, x in enumerate(dl) if x), default=0) + 1) if hdist is None else hdist
    ll = list(ll) + [0] * (288 - len(ll))
    dl = list(dl) + [0] * (32 - len(dl))
    if htoks is None:
        htoks = rle(ll[:hlit] + dl[:hdist])
    D.starts.append(D.w.n)
    header(D.w, hlit, hdist, htoks, cl=cl, hclen=hclen, final=final)
    D._symbols(toks, W.canonical(ll[:288]), ll[:288], W.canonical(dl[:30]), dl[:30])


def lens320(ll, dl):
    """The decoder's length layout: litlen at [0, 288), distance at [288, 320)."""
    return list(ll) + [0] * (288 - len(ll)) + list(dl) + [0] * (32 - len(dl))


def flat_ll(n):
    """A complete litlen code over symbols 0 .. n - 1 (n <= 286, a power-of-two split: 2^k - n
    symbols of k - 1 bits first, the rest of k bits)."""
    k = (n - 1).bit_length()
    short = (1 << k) - n
    return [k - 1] * short + [k] * (n - short)


def header_cases():
    """name -> (hlit, hdist, tokens, cl or None, hclen or None, expected kind, expected status).
    For DYN cases the expected lengths are expand(tokens) split at hlit."""
    c = {}
    ll257 = flat_ll(257)            # 255 x 8 bits, 2 x 9 bits
    ll286 = flat_ll(286)
    d1, d30 = [0], flat_ll(30)
    d2 = [1, 1]

    def good(name, ll, dl, toks=None, cl=None, hclen=None):
        seq = list(ll) + list(dl)
        toks = rle(seq) if toks is None else toks
        assert expand(toks) == seq, name
        c[name] = (len(ll), len(dl), toks, cl, hclen, DYN, 0)

    def bad(name, hlit, hdist, toks, cl=None, hclen=None, status=BAD_TABLE):
        c[name] = (hlit, hdist, toks, cl, hclen, ERR, status)

    good("hlit257_hdist1", ll257, d1)
    good("hlit286_hdist30", ll286, d30)
    good("hlit257_hdist30", ll257, d30)
    good("hlit286_hdist1", ll286, d1)
    # HCLEN 19: the last code-length symbol in transmission order (15) has a code
    ll15 = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15] + [0] * 241 + [15]
    t = rle(ll15 + d2)
    good("hclen19", ll15, d2, t)
    assert cl_for(t)[15] > 0
    # HCLEN 4 can only name the symbols 16, 17, 18 and 0: every length is 0, so no EOB code
    bad("hclen4_no_eob", 257, 1, [(18, 127), (18, 109)], cl=[1] + [0] * 17 + [1], hclen=4)
    # a 16 whose run crosses from the litlen into the distance alphabet
    llx = flat_ll(256) + [8]        # 256 x 8 bits + the EOB at 8 bits: over-subscribed litlen code,
    # which is the table builder's business, not the header's
    dlx = [8, 8, 8, 5, 5]
    seq = llx + dlx
    t = rle(seq[:254]) + [(8, None), (16, 2), (5, None), (5, None)]
    assert expand(t) == seq
    good("rep16_crosses_alphabets", llx, dlx, t)
    # 17 and 18 at their minimum and maximum runs (3, 10, 11, 138), an 18 crossing the alphabets
    llz = [8] * 4 + [0] * 3 + [8] + [0] * 10 + [8] + [0] * 11 + [8] + [0] * 138 + [8] * 87 + [9]
    assert len(llz) == 257
    t = [(8, None)] * 4 + [(17, 0), (8, None), (17, 7), (8, None), (18, 0), (8, None), (18, 127)] + \
        [(8, None)] * 87 + [(9, None)]
    good("zero_runs_min_max", llz, [0] * 12 + [3], t + [(18, 1), (3, None)])
    # a run ending exactly at HLIT + HDIST, and the same run one longer
    t = rle(ll257) + [(4, None), (16, 3)]
    good("run_ends_exactly", ll257, [4] * 7, t)
    bad("run_one_past", 257, 6, t)
    bad("zero_run_past", 257, 1, rle(ll257[:250]) + [(18, 0)])
    bad("rep16_first", 257, 1, [(16, 0)] + rle(ll257[3:] + d1))
    # code-length codes: over-subscribed (four 1-bit codes), incomplete (a hole), a single code
    t = rle(ll257 + d1)
    over = [0] * 19
    over[0] = over[8] = over[9] = over[16] = 1
    bad("cl_oversubscribed", 257, 1, t, cl=over)
    hole = [0] * 19
    hole[0], hole[8], hole[9], hole[16] = 1, 2, 3, 4  # the pattern 1111 has no code
    bad("cl_incomplete", 257, 1, t, cl=hole)
    one = [0] * 19
    one[8] = 1
    bad("cl_single_code", 257, 1, [(8, None)] * 258, cl=one)
    bad("cl_all_zero", 257, 1, [], cl=[0] * 19, hclen=19)
    # no end-of-block code
    noeob = list(ll257)
    noeob[256] = 0
    bad("missing_eob", 257, 1, rle(noeob + d1), cl=cl_for(rle(ll257 + d1)))
    # counts past the alphabets
    for hlit, hdist in ((287, 1), (288, 1), (257, 31), (257, 32)):
        bad("hlit%d_hdist%d" % (hlit, hdist), hlit, hdist, rle([8] * hlit + [5] * hdist))
    # the longest legal header: 316 length symbols of 7-bit codes, HCLEN 19
    cl7 = [0] * 19
    for s, n in ((0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (8, 7), (9, 7)):
        cl7[s] = n
    cl7[15] = 0
    lll = ([8, 9] * 143)[:286]
    dll = ([9, 8] * 15)[:30]
    good("longest_legal", lll, dll, [(x, None) for x in lll + dll], cl=cl7, hclen=19)
    return c
