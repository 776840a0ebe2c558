"""tests/floatref.py, the exact decimal -> IEEE reference of the float tests, against the three
converters the other oracles use: libc strtof (samutil.pack_float), Python's float() and the SAM
writer's Float.toString oracle (samwriteutil.float_text).  And the shape of the shared inputs."""
import struct

import pytest

import floatcases as F
import samutil as S
import samwriteutil as W
import vcfutil as V
from floatref import BINARY32, BINARY64, exact_bits, exact_bytes


def test_hand_checked_values():
    f, d = (lambda t: exact_bits(t, BINARY32)), (lambda t: exact_bits(t, BINARY64))
    assert f(b"0") == 0 and f(b"-0.0") == 0x80000000 and f(b"-0e5") == 0x80000000
    assert f(b"1") == 0x3f800000 and f(b".5") == 0x3f000000 and f(b"5.") == 0x40a00000
    assert f(b"7.038531e-26") == 0x15ae43fd
    assert f(b"3.4028235e38") == 0x7f7fffff
    assert f(b"340282356779733661637539395458142568447") == 0x7f7fffff       # just under max + half an ulp
    assert f(b"340282356779733661637539395458142568448") == 0x7f800000       # the tie: to even = infinity
    assert f(b"-1e39") == 0xff800000
    assert f(b"1e-45") == 1 and f(b"7e-46") == 0 and f(b"-7e-46") == 0x80000000
    half_min = b"%de-150" % 5 ** 150                                          # 2^-150 exactly: to even
    assert f(half_min) == 0 and f(half_min.replace(b"e", b".0001e")) == 1 and f(b"-" + half_min) == 0x80000000
    three_halves = b"%de-150" % (3 * 5 ** 150)                                # 1.5 * 2^-149: up to even
    assert f(three_halves) == 2 and f(b"%de-150" % (3 * 5 ** 150 - 1)) == 1
    assert f(b"1.17549435e-38") == 0x00800000 and f(b"1.1754942e-38") == 0x007fffff
    assert f(b"16777217") == 0x4b800000 and f(b"16777219") == 0x4b800002     # ties to even, both ways
    assert f(b"16777217.0000001") == 0x4b800001
    assert d(b"1") == 0x3ff0000000000000 and d(b"-2.5E0") == 0xc004000000000000
    assert d(b"9007199254740993") == 0x4340000000000000 and d(b"9007199254740995") == 0x4340000000000002
    assert d(b"4.9e-324") == 1 and d(b"2.4e-324") == 0 and d(b"1.7976931348623157e308") == 0x7fefffffffffffff
    assert d(b"1.7976931348623159e308") == 0x7ff0000000000000
    assert exact_bytes(b"1.5") == struct.pack("<f", 1.5) and exact_bytes(b"1.5", BINARY64) == struct.pack("<d", 1.5)
    # far exponents are clamped before a power is formed
    assert f(b"1e99999999999999999999") == 0x7f800000 and d(b"-1e99999999999999999999") == 0xfff0000000000000
    assert f(b"1e-99999999999999999999") == 0 and d(b"0e99999999999999999999") == 0
    assert d(b"0." + b"0" * 5000 + b"1e5000") == 0x3fb999999999999a           # 0.1
    # more digits than any rounding boundary has: the tail only says which side
    assert f(b"1" + b"0" * 5000 + b"e-5000") == 0x3f800000
    assert f(b"16777217." + b"0" * 2000) == 0x4b800000 and f(b"16777217." + b"0" * 2000 + b"1") == 0x4b800001
    for bad in(b"", b"+", b".", b"e5", b"1e", b"nan", b"inf", b"0x1p3", b" 1", b"1 ", b"1.5.2", b"+.e1"):
        with pytest.raises(ValueError):
            exact_bits(bad)


def test_short_ties_are_ties():
    """Every kept tie is exactly half way between two binary32 values: its two neighbours round to
    adjacent floats, and the tie itself to the even one of them."""
    texts, n = F.short_ties(), F.short_tie_count()
    ties, near = texts[:n], F.short_tie_neighbours()
    assert n >= 1000 and len(texts) == n + 2 * len(near) >= 3000
    assert all(F.sig_digits(t) <= 19 for t in texts) and len(set(ties)) == n
    assert all(exact_bits(t.encode()) & 1 == 0 for t in ties)      # a tie goes to the even neighbour
    up = down = 0
    for t, above, below in near:
        hi, lo, mid = (exact_bits(x.encode()) for x in (above, below, t))
        assert hi == lo + 1 and mid in (lo, hi), (t, above, below)
        up += mid == hi
        down += mid == lo
    assert up > 100 and down > 100, (up, down)                     # both directions occur


def test_exact_bits_is_strtof_on_the_sam_texts():
    texts = F.sam_float_texts()
    assert texts[-len(F.SAM_BAD):] == F.SAM_BAD
    n = 0
    for t in texts:
        t = t.encode()
        if S.FLOAT_RE.match(t):
            assert exact_bytes(t) == S.pack_float(t), t
            n += 1
        else:
            with pytest.raises(ValueError):
                S.pack_float(t)
    assert n > 62000 + 3000


def test_exact_bits_is_float_on_the_qual_texts():
    texts = F.qual_texts() + F.QUAL_EXTRA
    assert len(texts) == F.N_QUAL_RANDOM + 1200 + len(F.QUAL_EXTRA)
    for t in texts:
        assert V.QUAL_RE.match(t.encode()), t
        assert exact_bytes(t.encode(), BINARY64) == struct.pack("<d", float(t)), t
    # the edge family: the exponents +-21 and +-22 stay on the device, +-23 go to the host
    edge = F.qual_edge_texts()
    fast = [V.qual_fast_path(t.encode()) for t in edge]
    assert fast == [i // 200 < 4 for i in range(1200)]


def test_the_writers_text_reads_back_to_its_bits():
    """Float.toString as samwriteutil works it out, read by the exact reference: the same bits, for
    every finite value of the writer's tests.  Ties the writer's oracle to the reader's."""
    edges = W.binade_edges()
    vals = W.float_set(20000) + edges + [0x80000000 | b for b in edges]
    n = 0
    for b in vals:
        if (b >> 23) & 0xff == 0xff:
            continue
        assert exact_bits(W.float_text(b)) == b, hex(b)
        n += 1
    assert n > 22000
