"""Fixtures and expected values for the BGZF block chain by windows (dq_chain_core.h):

- a Python restatement of the serial chain walk (start at the chain start, hop by BSIZE + 1 while
  htsjdk's BlockGunzipper would take the header: chain_serial) and of
  BgzfBlockGuesser.guessNextBGZFPos (guess_next), both held against the oracle on tests/golden/
  by tests/test_chain_core_cpu.py before anything else is held against them;
- builders of files whose members lie where the windowed walk can go wrong: at a window's edges,
  fake members in stored payload as a window's first guesser hit, dense runs of tiny members,
  headers the guesser takes and htsjdk does not, cut members, trailing garbage.

Stored (level-0) members keep their payload verbatim and cost a fixed 31 bytes each, so the
compressed position of every payload byte is known: byte j of the stream lies at
j + 31 * (its member's index) + 23.
"""
import struct
import zlib

MAGIC = b"\x1f\x8b\x08\x04"
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
W_SMALL = 65536  # the window of the chainw variant build (-DDQ_CHAIN_W=65536)


# ---------------------------------------------------------------- restatements
def htsjdk_block(d, p):
    """BlockGunzipper.unzipBlock's header checks at p: the member's length, or 0."""
    L = len(d)
    if p + 18 > L or d[p:p + 4] != MAGIC or d[p + 10] | d[p + 11] << 8 != 6:
        return 0
    c = (d[p + 16] | d[p + 17] << 8) + 1
    return c if c >= 26 and p + c <= L else 0


def chain_serial(d, start=0):
    """[(pos, csize, usize)] of the walk from `start`."""
    out, p = [], start
    while p < len(d):
        c = htsjdk_block(d, p)
        if not c:
            break
        out.append((p, c, struct.unpack_from("<i", d, p + c - 4)[0]))
        p += c
    return out


def guess_next(d, p, end):
    """BgzfBlockGuesser.guessNextBGZFPos(p, end) (BgzfBlockGuesser.java:76-149): (pos, cSize, uSize)
    or None.  The byte-stepping scan of :79-92 lands on the next magic at or after p and gives up
    at the first position it steps to at or past `end`."""
    L = len(d)
    while True:
        q = d.find(MAGIC, p)
        if q < 0 or (q != p and q >= end):
            return None
        p0 = q
        if q + 12 > L:
            return None
        xlen = d[q + 10] | d[q + 11] << 8
        p = q + 12
        sub_end = p + xlen
        hit = None
        while p < sub_end:
            if p + 4 > L:
                return None
            if d[p:p + 4] != b"BC\x02\x00":
                p += 4 + (d[p + 2] | d[p + 3] << 8)
                continue
            if p + 6 > L:
                return None
            bsize = d[p + 4] | d[p + 5] << 8
            p += 6
            while p < sub_end:
                if p + 4 > L:
                    return None
                p += 4 + (d[p + 2] | d[p + 3] << 8)
            if p != sub_end:
                break  # cancelled
            p += bsize - xlen - 19 + 4
            if p < 0 or p + 4 > L:
                return None
            hit = (p0, p + 4 - p0, struct.unpack_from("<i", d, p)[0])
            break
        if hit:
            return hit
        p = p0 + 4


def first_guess(d):
    """A shard's chain start: the first position from byte 0 that the guesser returns, else len."""
    g = guess_next(d, 0, 1 << 62)
    return g[0] if g else len(d)


# ---------------------------------------------------------------- builders
def stored_member(data, extra=b""):
    """One stored deflate block of `data` as a BGZF member; `extra`: further gzip subfields after BC
    (XLEN grows: the guesser walks them, htsjdk wants XLEN == 6)."""
    assert len(data) <= 65535
    body = bytes([1]) + struct.pack("<HH", len(data), len(data) ^ 0xffff) + data
    xlen = 6 + len(extra)
    total = 12 + xlen + len(body) + 8
    hdr = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", xlen) + b"BC\x02\x00"
    return hdr + struct.pack("<H", total - 1) + extra + body + struct.pack("<II", zlib.crc32(data), len(data))


def deflated_member(data, level=6):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = co.compress(data) + co.flush()
    hdr = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00"
    return hdr + struct.pack("<H", 18 + len(body) + 8 - 1) + body + struct.pack("<II", zlib.crc32(data), len(data))


def stored_file(stream, sizes, rest=30000, eof=True):
    """`stream` in stored members of the given compressed sizes (31 + payload each), then members
    of `rest` payload bytes, then the EOF block."""
    out, at = [], 0
    for s in sizes:
        n = s - 31
        assert 0 <= n <= 65535 and at + n <= len(stream), (s, at, len(stream))
        out.append(stored_member(stream[at:at + n]))
        at += n
    while at < len(stream):
        out.append(stored_member(stream[at:at + rest]))
        at += rest
    return b"".join(out) + (EOF_BLOCK if eof else b"")


def text_stream(nbytes, seed=1):
    """Lines of digits, exactly nbytes long, LF terminated."""
    out, k = bytearray(), seed
    while len(out) < nbytes:
        k = (k * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        out += b"%d\t%d\tline\n" % (k % 1000003, len(out))
    out = out[:nbytes]
    if nbytes:
        out[-1:] = b"\n"
    return bytes(out)


def sized_text_file(total):
    """A stored-member text file of exactly `total` bytes, EOF block included."""
    body = total - 28
    n_full = body // (31 + 30000)
    last = body - n_full * (31 + 30000)
    if 0 < last < 32:  # the last member needs a payload: take the bytes from the one before
        n_full -= 1
        last += 31 + 30000
    sizes = [31 + 30000] * n_full
    if last > 65535 + 31:
        sizes += [31 + 20000, last - 31 - 20000]
    elif last:
        sizes += [last]
    stream = text_stream(sum(s - 31 for s in sizes))
    f = stored_file(stream, sizes)
    assert len(f) == total, (len(f), total)
    return f, stream


def edge_text_file(boundary, nwin=4, rest=30000):
    """A member boundary exactly at `boundary`, the members behind it of `rest` payload bytes."""
    first = []
    left = boundary
    while left > 65536:
        first.append(31 + 30000)
        left -= 31 + 30000
    if left < 31 + 1:
        first[-1] -= 40
        left += 40
    first.append(left)
    stream = text_stream(sum(s - 31 for s in first) + nwin * W_SMALL)
    f = stored_file(stream, first, rest)
    assert any(b[0] == boundary for b in chain_serial(f))
    return f, stream


def fake_at_window_text(fakes, windows=(2,), nwin=5):
    """A stored-member text file in which `fakes[i]` (a complete BGZF member, as payload bytes
    inside a line) starts exactly at window windows[i]'s first byte, so it is that window's first
    guesser hit.  Returns (file, stream)."""
    rest = 30000
    stream = bytearray(text_stream(nwin * W_SMALL))
    for fake, w in zip(fakes, windows):
        assert b"\n" not in fake and b"\r" not in fake
        target = w * W_SMALL
        # payload byte j of member k lies at j + 31 k + 23: find j with that position == target
        for k in range(len(stream) // rest + 1):
            j = target - 31 * k - 23
            if k * rest <= j and j + len(fake) <= min((k + 1) * rest, len(stream)):
                break
        else:
            raise AssertionError("no member holds the fake at the window start")
        stream[j:j + len(fake)] = fake
    stream = bytes(stream)
    f = stored_file(stream, [], rest)
    for fake, w in zip(fakes, windows):
        assert f[w * W_SMALL:w * W_SMALL + len(fake)] == fake
        assert guess_next(f, w * W_SMALL, 1 << 62)[0] == w * W_SMALL  # the window's first hit
        assert w * W_SMALL not in [b[0] for b in chain_serial(f)]    # and off the chain
    return f, stream


def lines_of(stream):
    """The text path's lines of a stream read in one split: values without terminators."""
    parts = stream.split(b"\n")
    return parts[:-1] if stream.endswith(b"\n") else parts
