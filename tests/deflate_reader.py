"""Test helper: a plain-Python raw-DEFLATE reader (RFC 1951), the mirror of deflate_writer.py.

zlib says whether a stream is valid and what it inflates to; it does not say which block type an
encoder chose, which code lengths it sent, how it run-length coded them or which matches it made.
read() returns all of that for every deflate block of a body, with the tokens in deflate_writer's
format (a literal byte, or a (length, distance) pair), so a test of an ENCODER can assert that the
case it is about was really emitted.  The reader tolerates nothing: it raises DeflateError on
anything RFC 1951 forbids (and on what zlib rejects: over-subscribed codes, incomplete codes other
than a single one-bit code, a missing end-of-block code, a repeat with nothing before it).  Test
infrastructure only; tests/test_deflate_reader.py checks it against zlib and deflate_writer."""
import struct

import deflate_writer as W


class DeflateError(ValueError):
    pass


class Block:
    """One deflate block.  start / data / end: bit offsets of its header (BFINAL), of its first
    symbol (for a stored block: of its first byte) and of the bit after its end-of-block code.
    Dynamic blocks: hlit, hdist, hclen (the counts, not the header fields), cl_lens (the 19
    code-length-code lengths by symbol), header (the run-length tokens, (symbol, extra value) with
    extra None for 0..15), ll_lens and d_lens (hlit and hdist long).  Fixed blocks carry the fixed
    tables in ll_lens / d_lens."""
    __slots__ = ("btype", "final", "start", "data", "end", "hlit", "hdist", "hclen", "cl_lens",
                 "header", "ll_lens", "d_lens", "tokens")

    def __init__(self):
        for k in self.__slots__:
            setattr(self, k, None)


class _Bits:
    def __init__(self, b):
        self.b, self.p, self.acc, self.n, self.nb = bytes(b), 0, 0, 0, 8 * len(b)

    @property
    def pos(self):
        return 8 * self.p - self.n

    def need(self, k):
        while self.n < k:
            chunk = self.b[self.p:self.p + 8]
            if not chunk:
                raise DeflateError("the stream ends inside a block")
            self.acc |= int.from_bytes(chunk, "little") << self.n
            self.n += 8 * len(chunk)
            self.p += len(chunk)

    def get(self, k):
        self.need(k)
        v = self.acc & ((1 << k) - 1)
        self.acc >>= k
        self.n -= k
        return v

    def peek(self, k):  # up to k bits (zero filled past the end; sym() checks the length)
        if self.n < k and self.p < len(self.b):
            chunk = self.b[self.p:self.p + 8]
            self.acc |= int.from_bytes(chunk, "little") << self.n
            self.n += 8 * len(chunk)
            self.p += len(chunk)
        return self.acc & ((1 << k) - 1)

    def skip(self, k):
        if k > self.n:
            raise DeflateError("the stream ends inside a block")
        self.acc >>= k
        self.n -= k

    def align(self):
        self.skip(self.n & 7)


class _Code:
    """A canonical prefix code: a flat table over max-length bit-reversed prefixes."""

    def __init__(self, lens, what):
        used = [ln for ln in lens if ln]
        if not used:
            raise DeflateError("%s code has no codes" % what)
        self.max = max(used)
        kraft = sum(1 << (self.max - ln) for ln in used)
        if kraft > 1 << self.max:
            raise DeflateError("%s code is over-subscribed" % what)
        if kraft < 1 << self.max and not (len(used) == 1 and used[0] == 1):
            raise DeflateError("%s code is incomplete" % what)
        self.tab = [None] * (1 << self.max)
        codes = W.canonical(list(lens))
        for s, ln in enumerate(lens):
            if ln:
                r = int(format(codes[s], "0%db" % ln)[::-1], 2)
                n = 1 << (self.max - ln)
                self.tab[r::1 << ln] = [(s, ln)] * n

    def sym(self, r):
        e = self.tab[r.peek(self.max)]
        if e is None:
            raise DeflateError("a bit pattern without a code")
        r.skip(e[1])
        return e[0]


def _dynamic_header(r, blk):
    blk.hlit, blk.hdist, blk.hclen = r.get(5) + 257, r.get(5) + 1, r.get(4) + 4
    if blk.hlit > 286 or blk.hdist > 30:
        raise DeflateError("too many literal/length or distance codes")
    cl = [0] * 19
    for i in range(blk.hclen):
        cl[W.CL_ORDER[i]] = r.get(3)
    blk.cl_lens = cl
    cc = _Code(cl, "code-length")
    if len([x for x in cl if x]) < 2:
        raise DeflateError("code-length code is incomplete")
    lens, blk.header = [], []
    total = blk.hlit + blk.hdist
    while len(lens) < total:
        s = cc.sym(r)
        if s < 16:
            blk.header.append((s, None))
            lens.append(s)
            continue
        if s == 16:
            if not lens:
                raise DeflateError("a repeat with no length before it")
            x = r.get(2)
            run = [lens[-1]] * (3 + x)
        elif s == 17:
            x = r.get(3)
            run = [0] * (3 + x)
        else:
            x = r.get(7)
            run = [0] * (11 + x)
        blk.header.append((s, x))
        lens += run
        if len(lens) > total:
            raise DeflateError("a run of code lengths passes the end of the tables")
    blk.ll_lens, blk.d_lens = lens[:blk.hlit], lens[blk.hlit:]
    if blk.ll_lens[256] == 0:
        raise DeflateError("no end-of-block code")


def header_run(tok):
    """The number of code lengths a header token stands for."""
    s, x = tok
    return 1 if s < 16 else (3 + x if s < 18 else 11 + x)


def read(body, history=0):
    """The deflate blocks of a raw-DEFLATE body (up to and including the final one; at most 7
    padding bits may follow).  history: bytes of output before the body that distances may reach."""
    r = _Bits(body)
    out, produced = [], history
    fixed = None
    while True:
        blk = Block()
        blk.start = r.pos
        blk.final = bool(r.get(1))
        blk.btype = r.get(2)
        if blk.btype == 3:
            raise DeflateError("reserved block type")
        if blk.btype == 0:
            r.align()
            n, nn = r.get(16), r.get(16)
            if n ^ nn != 0xffff:
                raise DeflateError("stored block: LEN and NLEN disagree")
            blk.data = r.pos
            if r.pos + 8 * n > r.nb:
                raise DeflateError("the stream ends inside a stored block")
            a = blk.data // 8
            blk.tokens = list(r.b[a:a + n])
            # (the bit buffer is byte aligned here: restart it after the bytes)
            r.p, r.acc, r.n = a + n, 0, 0
            blk.end = r.pos
            produced += n
        else:
            if blk.btype == 2:
                _dynamic_header(r, blk)
                llc = _Code(blk.ll_lens, "literal/length")
                dc = _Code(blk.d_lens, "distance") if any(blk.d_lens) else None
            else:
                if fixed is None:
                    fixed = (_Code(W.FIXED_LL, "literal/length"),
                             _Code(W.FIXED_D + [5, 5], "distance"))
                llc, dc = fixed
                blk.ll_lens, blk.d_lens = list(W.FIXED_LL), list(W.FIXED_D)
            blk.data = r.pos
            toks = []
            while True:
                s = llc.sym(r)
                if s < 256:
                    toks.append(s)
                    produced += 1
                elif s == 256:
                    break
                else:
                    if s > 285:
                        raise DeflateError("invalid length symbol %d" % s)
                    n = W.LBASE[s - 257] + r.get(W.LEXT[s - 257])
                    if dc is None:
                        raise DeflateError("a match in a block without distance codes")
                    ds = dc.sym(r)
                    if ds > 29:
                        raise DeflateError("invalid distance symbol %d" % ds)
                    d = W.DBASE[ds] + r.get(W.DEXT[ds])
                    if d > produced:
                        raise DeflateError("distance %d reaches before the start" % d)
                    toks.append((n, d))
                    produced += n
            blk.tokens = toks
            blk.end = r.pos
        out.append(blk)
        if blk.final:
            break
    if r.nb - r.pos > 7:
        raise DeflateError("%d bits after the final block" % (r.nb - r.pos))
    return out


def members(bgzf):
    """The members of a BGZF stream as (raw-DEFLATE body, CRC32, ISIZE); raises on a member that
    is not htsjdk's layout ('BC' extra field, BSIZE) or runs past the end."""
    out, p = [], 0
    while p < len(bgzf):
        h = bgzf[p:p + 18]
        if len(h) < 18 or h[:4] != b"\x1f\x8b\x08\x04" or h[10:12] != b"\x06\x00" or h[12:14] != b"BC":
            raise DeflateError("not a BGZF member header at %d" % p)
        cs = struct.unpack_from("<H", h, 16)[0] + 1
        if cs < 26 or p + cs > len(bgzf):
            raise DeflateError("BSIZE of the member at %d" % p)
        crc, isize = struct.unpack_from("<II", bgzf, p + cs - 8)
        out.append((bytes(bgzf[p + 18:p + cs - 8]), crc, isize))
        p += cs
    return out
