"""Tables of good and bad aux regions for the tag decode tests (dq_tags), each
wrapped into a record by reccases.record(aux=...), the key lists they are decoded with, and the
synthetic records of the GPU cases.  The expected cells and errors come from tests/tagutil.py."""
import random
import struct

import reccases as R
import tagutil as U


def tag(vid, ty, payload=b""):
    return vid + ty + payload


def z(vid, text):
    return tag(vid, b"Z", text + b"\x00")


def barr(vid, sub, count, payload=None):
    if payload is None:
        payload = bytes((1 + i) & 0xff for i in range(U.ELEM_SIZE[sub] * count))
    return tag(vid, b"B", sub + struct.pack("<i", count) + payload)


NM = tag(b"NM", b"C", b"\x03")
AS = tag(b"AS", b"s", struct.pack("<h", -77))
XS = tag(b"XS", b"i", struct.pack("<i", -123456))
RG = z(b"RG", b"grp1")
MD = z(b"MD", b"10A5^AC6")
FL = tag(b"XF", b"f", struct.pack("<f", -1.5))
CH = tag(b"XA", b"A", b"Q")
HX = tag(b"XH", b"H", b"1aE3\x00")

# the keys most tables are read with: one of every class, two that never occur
KEYS = [(b"NM", U.INT), (b"AS", U.INT), (b"XS", U.INT), (b"RG", U.STRING), (b"MD", U.ANY), (b"XF", U.FLOAT),
        (b"XA", U.CHAR), (b"XH", U.ANY), (b"XB", U.ANY), (b"XI", U.INT), (b"zz", U.ANY), (b"Z9", U.INT),
        (b"XZ", U.STRING)]
KEYS1 = [(b"NM", U.INT)]
KEYS64 = KEYS + [(b"K%c" % c, U.ANY) for c in b"0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNO"]
assert len(KEYS) == 13 and len(KEYS64) == 64

GOOD = [
    b"",                                                              # empty aux
    NM,
    NM + AS + XS + RG + MD + FL + CH + HX,                           # every class
    tag(b"XI", b"c", b"\x80") + tag(b"NM", b"s", b"\x00\x80"),      # c / s negative
    tag(b"XI", b"C", b"\xff") + tag(b"NM", b"S", b"\xff\xff"),
    tag(b"XI", b"I", struct.pack("<I", 0x80000000)),
    tag(b"XI", b"I", struct.pack("<I", 0xffffffff)),
    tag(b"XI", b"i", struct.pack("<i", -2 ** 31)),
    z(b"XZ", b""),                                                    # empty Z
    tag(b"XH", b"H", b"\x00"),                                        # empty H
    tag(b"XH", b"H", b"abcdef\x00"),                                  # H lower-case
    z(b"XZ", b"x" * 7), z(b"XZ", b"x" * 8), z(b"XZ", b"x" * 9), z(b"XZ", b"y" * 300),  # the word scan's edges
    RG + z(b"XZ", b"tail") + NM,                                      # the key last
    NM + RG,                                                          # the key first
    RG + MD,                                                          # the key absent
    NM + NM,                                                          # repeated
    NM + RG + tag(b"NM", b"i", struct.pack("<i", 9)) + NM,           # repeated, another type behind
    z(b"RG", b"a") + z(b"RG", b"b"),
    tag(b"Xq", b"A", b"!") + tag(b"xq", b"A", b"?"),                 # ids differ in case only
] + [barr(b"XB", s, c) for s in (b"c", b"C", b"s", b"S", b"i", b"I", b"f") for c in (0, 1)] + [
    barr(b"XB", b"S", 300) + NM,                                     # a long array in front of a key
    barr(b"XB", b"c", 3, b"\x00\x00\x00") + AS,                      # NULs inside an array
]

# (aux, the error tagutil must name) -- every check of the walk
BAD = [
    (b"N", "tag "), (b"NM", "tag "),                                 # fewer than three bytes
    (NM + b"A", "tag "), (NM + b"AS", "tag "),
    (b"NMC", "tag NM"),                                               # no payload byte
    (b"ASs\x01", "tag AS"), (b"XSi\x01\x02\x03", "tag XS"), (b"XFf\x01\x02\x03", "tag XF"),
    (b"XAA", "tag XA"),
    (b"RGZabc", "tag RG"), (b"RGZ", "tag RG"),                      # no NUL
    (b"XHH1a", "tag XH"),                                             # no NUL
    (b"XHH1\x00", "tag XH"), (b"XHH1ag0\x00", "tag XH"),            # odd, not hex
    (b"XBBc\x01\x00\x00", "tag XB"),                                  # head cut
    (b"XBBx\x00\x00\x00\x00", "tag XB"),                              # unknown element type
    (b"XBBc\xff\xff\xff\xff", "tag XB"),                              # negative count
    (b"XBBi\x02\x00\x00\x00" + b"\x00" * 7, "tag XB"),               # elements cut
    (b"XBBS\x00\x00\x00\x40", "tag XB"),                              # count * size far past the record
    (b"XQq\x00", "tag XQ"), (b"XQ\x00\x00", "tag XQ"),              # unknown type byte
    (NM + RG + b"ASs\x01", "tag AS"),                                 # behind good tags
]

# a key's first occurrence stored outside the class asked for, one per class
MISMATCH = [
    (tag(b"NM", b"f", b"\x00" * 4), "tag NM type"), (z(b"NM", b"3"), "tag NM type"),
    (tag(b"XF", b"i", b"\x00" * 4), "tag XF type"),
    (tag(b"XA", b"C", b"A"), "tag XA type"),
    (tag(b"RG", b"H", b"ab\x00"), "tag RG type"), (tag(b"XZ", b"A", b"r"), "tag XZ type"),
    (barr(b"XI", b"i", 1), "tag XI type"),
    (RG + tag(b"NM", b"A", b"3") + b"ASs\x01", "tag NM type"),       # in front of a bad tag: it wins
    (RG + b"XQ?" + tag(b"NM", b"A", b"3"), "tag XQ"),                # behind one: never seen
]
# not a mismatch: only the first occurrence is held to the class
GOOD.append(NM + tag(b"NM", b"f", b"\x00" * 4))


def truncations():
    """Every good multi-tag region cut at each byte of its last tag's head and payload: (aux, what)
    with what = None where the cut region is itself well formed."""
    out = []
    for aux in (NM + AS, NM + XS, RG + FL, NM + CH, NM + RG, NM + HX, NM + barr(b"XB", b"s", 2), NM + MD):
        first = len(NM) if aux.startswith(NM) else len(RG)
        for cut in range(first + 1, len(aux)):
            out.append(aux[:cut])
    return out


def rec_of(aux, i=0, l_seq=10):
    """A mapped record around an aux region."""
    return R.record(0, 100 + i, b"r%d\x00" % i, [(l_seq, 0)], l_seq, mapq=30, aux=aux)


def fields_records():
    """Records whose layout does not fit: (record bytes, 'fields')."""
    good = bytearray(rec_of(NM))
    a = bytearray(good)
    struct.pack_into("<i", a, 20, 4000)           # l_seq runs past the record
    b = bytearray(good)
    struct.pack_into("<H", b, 16, 60000)          # n_cigar does
    c = bytearray(good)
    struct.pack_into("<i", c, 20, -1)             # negative l_seq
    return [bytes(a), bytes(b), bytes(c)]


def all_auxes():
    return GOOD + [a for a, _ in BAD + MISMATCH] + truncations()


def table_records():
    return [rec_of(a, i) for i, a in enumerate(all_auxes())] + fields_records()


# ------------------------------------------------------------------ synthetic records (GPU cases)
def synth_aux(r, target):
    """A well-formed aux region of exactly `target` bytes (0, or >= 4) that holds the usual keys
    where they fit."""
    if target == 0:
        return b""
    assert target >= 4
    parts, left = [], target
    for t in r.sample([NM, AS, XS, RG, MD, FL, CH, HX], 8):
        if left - len(t) >= 4 or left == len(t):
            parts.append(t)
            left -= len(t)
    if left:
        parts.insert(r.randrange(len(parts) + 1), z(b"XZ", bytes(r.choice(b"ACGT") for _ in range(left - 4))))
    aux = b"".join(parts)
    assert len(aux) == target
    return aux


def synth_records(n, lens, seed=0, l_seq=None):
    """n records whose aux lengths cycle through `lens`."""
    r = random.Random(seed)
    return [rec_of(synth_aux(r, lens[i % len(lens)]), i, l_seq if l_seq is not None else r.choice((1, 36, 101)))
            for i in range(n)]
