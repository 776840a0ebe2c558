"""Pins the SAM writer's oracle (tests/samwriteutil.py) without the library:
real SAM lines are reproduced from the records the SAM reader's oracle makes of them, the lines
that reading normalises come out in their canonical text, and Float.toString is checked against
hand-written pairs and against numpy's shortest digits."""
import os
import struct

import numpy as np
import pytest

import bamutil as B
import samcases as K
import samutil as S
import samwriteutil as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def roundtrip(text):
    """(line, the oracle's text of the record samutil makes of it) per non-'@' line."""
    names = S.sam_header_to_bam(text)[1]
    out = []
    for _, v in S.text_lines(text):
        if not v.startswith(b"@"):
            out.append((v, W.record_to_sam_line(S.sam_line_to_bam_record(v, names), names)))
    return out


def test_golden_sam_lines_reproduced():
    rt = roundtrip(open(os.path.join(GOLDEN, "test.sam"), "rb").read())
    assert len(rt) == 2
    assert all(a == b for a, b in rt)


def test_1bam_lines_reproduced():
    text = S.bam_to_sam_text(B.inflate_all(open(os.path.join(GOLDEN, "1.bam"), "rb").read()))
    rt = roundtrip(text)
    assert len(rt) == 4917 and max(len(a) for a, _ in rt) == 411
    assert all(a == b for a, b in rt)


# the canonical text of the 13 rule lines that reading normalises (hand-written)
B_ = K.BASE
CANON = {
    17: B_ + b"\tXX:i:7", 18: B_ + b"\tXX:i:0", 19: B_ + b"\tXX:i:12",
    27: B_ + b"\tXF:f:-0.001", 28: B_ + b"\tXF:f:7.038531E-26", 29: B_ + b"\tXF:f:0.5",
    30: B_ + b"\tXF:f:Infinity",
    51: B_ + b"\tXB:B:f,1.5,-0.0,3.0E10,7.038531E-26,0.0,0.25,1.0",
    54: b"r1\t0\tchr1\t100\t30\t17M\t*\t0\t0\tACGTNN=MRSVWYHKDB\t" + b"!" * 17,
    55: b"r1\t0\tchr1\t100\t30\t18M\t*\t0\t0\tACGTNNN=MRSVWYHKDB\t" + b"~" * 18,
    61: b"r1\t0\t*\t100\t30\t4M\t*\t0\t0\tACGT\tIIII",
    69: b"r1\t0\tchr1\t100\t30\t4M\t*\t0\t2147483647\tACGT\tIIII",
    70: b"r1\t0\tchr1\t100\t30\t4M\t*\t0\t0\tACGT\tIIII",
}


def test_rule_lines_roundtrip_or_canonical():
    lines = K.good_lines()
    assert len(lines) == 76
    rt = roundtrip(K.HEADER + b"".join(l + b"\n" for l in lines))
    same = 0
    for i, (a, b) in enumerate(rt):
        if i in CANON:
            assert a != CANON[i] and b == CANON[i], i
        else:
            assert a == b, i
            same += 1
    assert same == 63


def test_trim_and_errors():
    t = [W.record_to_sam_line(r, W.REFS) for r in W.trim_cases()]
    base = b"r1\t0\tchr1\t100\t30\t4M\t*\t0\t0\tACGT\tIIII"
    assert t[0] == base + b"\tXZ:Z:abc" and t[1] == base + b"\tXA:A:"
    assert t[2] == b"name" + base[2:] and t[3] == base[3:]
    assert t[5] == base + b"\tXZ:Z:a  \tXY:Z:b" and t[7] == b"a b \t" + base[3:]
    for rec, what in W.error_cases():
        with pytest.raises(W.SamWriteError) as e:
            W.record_to_sam_line(rec, W.REFS)
        assert e.value.what == what
    text, err = W.records_to_sam_text([W.make_record(), W.make_record(qual=b"((^("),
                                       W.make_record(ref=9)], W.REFS)
    assert text is None and err == "record 1: QUAL"


def test_float_pairs():
    for bits, text in W.FLOAT_PAIRS:
        assert W.float_text(bits) == text, hex(bits)


def test_float_min_normal_is_the_shortest_text():
    """0x00800000 prints as 1.1754944E-38 under the JDK 19+ contract: eight digits read back to the
    same bits.  JDK 8 printed 1.17549435E-38, one digit longer, which reads back too."""
    assert W.float_text(0x00800000) == b"1.1754944E-38"
    for t in (b"1.1754944E-38", b"1.17549435E-38"):
        assert S.pack_float(t.replace(b"E", b"e")) == struct.pack("<I", 0x00800000)
    assert S.pack_float(b"1.175494e-38") != struct.pack("<I", 0x00800000)


def numpy_digits(bits):
    s = np.format_float_scientific(np.array([bits & 0x7fffffff], dtype=np.uint32).view(np.float32)[0],
                                   unique=True, trim="-")
    mant, ex = s.split("e")
    return mant.replace(".", "").rstrip("0") or "0", int(ex)


def test_floats_against_numpy():
    """Digits and exponent equal numpy's shortest repr, except where Float.toString's two-digit
    clause applies: numpy prints one digit there, and the two-digit decimal nearest the value is
    not that digit followed by 0 (small subnormals only)."""
    differ = []
    for bits in W.random_finite(100000, 11) + W.binade_edges() + list(range(1, 1200)):
        bits &= 0x7fffffff
        if not bits:
            continue
        c, n, e = W.float_decimal(bits)
        d = str(c).rstrip("0")
        got = (d, e + len(str(c)) - 1)
        if got != numpy_digits(bits):
            differ.append(bits)
    # e.g. the subnormal range's first two values: 1.4E-45 and 2.8E-45 against numpy's 1e-45, 3e-45
    differ = sorted(set(differ))
    assert differ[:2] == [1, 2] and max(differ) < 1024
    assert all(len(numpy_digits(b)[0]) == 1 and W.float_decimal(b)[1] == 2 for b in differ)


def test_oracle_floats_read_back():
    """Whatever the oracle prints reads back to the same bits (libc strtof), at the binade edges,
    where the rounding interval is lopsided."""
    for bits in W.binade_edges():
        c, n, e = W.float_decimal(bits)
        assert S.pack_float(b"%de%d" % (c, e)) == struct.pack("<I", bits)
