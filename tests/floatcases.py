"""Test helper: the decimal texts of the float tests, shared by the CPU tests of dq_sam_core.h and
dq_vcf_core.h, the reference's own test and the GPU tests of the SAM reader and the VCF decode.
Every list is seeded and built once; callers get a copy."""
import decimal
import fractions
import functools
import random
import struct

import numpy as np

# texts the SAM float rule refuses (tests/samutil.py FLOAT_RE); the last of sam_float_texts()
SAM_BAD = ["", "+", ".", "5.", "1.e5", "e5", "1e", "1e+", "nan", "inf", "0x1p3", "1 ", " 1", "1f", "--1",
           "1.5.2", "1e5.0", "1,5", "+.e1"]

# QUAL texts by hand (every one matches tests/vcfutil.py QUAL_RE), and texts the QUAL rule refuses
QUAL_EXTRA = ["0", "-0", "-0.0", "5.", "1e22", "1e23", "1e-22", "1e-23", "9007199254740993", "123456789012345e7",
              "0.000000000000000000000001", "100000000000000000000", "1e400", "1e-400", "4.9e-324", ".5",
              "+.5e+1", "0e999", "1e-30", "123456789012345678", "000000000000000000001.50",
              "8.98846567431158e307", "2.2250738585072011e-308", "1.7976931348623157e308"]
QUAL_BAD = ["", "+", ".", "e5", "1e", "1e+", "nan", "NaN", "inf", "Infinity", "0x1p3", "1 ", " 1", "1f", "1d", "--1",
            "1.5.2", "1e5.0", "1,5", "+.e1", "1e5f"]


def sig_digits(t):
    """Significant digits of a decimal text: its mantissa's digits without leading zeros."""
    return len(t.lstrip("+-").lower().split("e")[0].replace(".", "").lstrip("0"))


# ------------------------------------------------------------------ binary32 texts
@functools.lru_cache(maxsize=None)
def _sam_base_texts():
    rng = random.Random(20240607)
    pats = []
    while len(pats) < 20000:
        b = rng.getrandbits(32)
        if (b >> 23) & 0xff != 0xff:
            pats.append(b)
    texts = []
    f32 = np.array(pats, np.uint32).view(np.float32)
    for x in f32:
        texts.append(repr(float(x)))                # shortest repr of the binary32 as a double
        texts.append("%.9g" % float(x))
        texts.append(np.format_float_scientific(x, unique=True, trim="-"))  # shortest for binary32 itself
    # exact decimal midpoints between a float and its successor
    ctx = decimal.Context(prec=400)
    for b in pats[:2000]:
        b &= 0x7fffffff
        if b >= 0x7f7fffff:
            continue
        lo, hi = (fractions.Fraction(float(np.array([v], np.uint32).view(np.float32)[0]))
                  for v in (b, b + 1))
        mid = (lo + hi) / 2
        texts.append(format(ctx.divide(decimal.Decimal(mid.numerator), decimal.Decimal(mid.denominator)), "f"))
    texts += ["7.038531e-26", "0", "-0.0", "1e-46", "1e39", ".5", "+1e+0", "-1e39", "1e-45", "7e-46",
              "0." + "0" * 30 + "123", "0" * 30 + "1.5", "1.234567890123456789012345",
              "3.4028235e38", "3.4028236e38", "1.17549435e-38", "1e99999999999999999999",
              "1e-99999999999999999999", "0e99999", "123456789012345678901234567890",
              "16777217", "16777219", "9007199791611905", "1.00000017881393432617187500",
              "1.00000017881393421514957253748434595763683319091796875"]
    return tuple(texts)


def _decimal_text(digits, q):
    """The integer `digits` (a string without leading zeros) times 10^q as a plain decimal, or with
    an eN suffix where q > 0."""
    if q > 0:
        return digits + "e%d" % q
    if q == 0:
        return digits
    if len(digits) > -q:
        return digits[:q] + "." + digits[q:]
    return "0." + "0" * (-q - len(digits)) + digits


@functools.lru_cache(maxsize=None)
def _short_ties():
    rng = random.Random(20250311)
    ties, near, parity = [], [], set()
    for e in range(-10, 90):
        for _ in range(40):
            m = rng.getrandbits(23) | 1 << 23          # a 24-bit significand: m * 2^(e-23) is a binary32
            v = 2 * m + 1                              # the midpoint to its successor = v * 2^(e-24)
            k = e - 24
            n, q = (v << k, 0) if k >= 0 else (v * 5 ** -k, k)
            full = str(n)
            d = full.rstrip("0")                       # an integer's trailing zeros go into the eN suffix
            if len(d) > 19:
                continue
            ties.append(_decimal_text(d, q + len(full) - len(d)))
            parity.add(m & 1)
            if len(full) < 19:
                # one more digit: just above (digits + "1") and just below (a final 5 becomes 49).
                # For an integer tie these are a tenth above and below it, zeros written out: a
                # digit appended to the integer's own text would multiply it by ten.
                near.append((ties[-1], _decimal_text(full + "1", q - 1), _decimal_text(str(10 * n - 1), q - 1)))
    assert len(ties) >= 1000 and parity == {0, 1}, (len(ties), parity)
    return tuple(ties), tuple(near)


def short_tie_neighbours():
    """[(tie, the text just above it, the text just below it)] where those still have 19 digits."""
    return list(_short_ties()[1])


def short_ties():
    """Exact midpoints between two neighbouring binary32 values that have at most 19 significant
    digits -- what dq_sam_core.h must decide itself, by its tie rule -- then, for every tie that
    leaves room for one more digit, a text just above and one just below it."""
    ties, near = _short_ties()
    return list(ties) + [t for _, a, b in near for t in (a, b)]


def short_tie_count():
    """How many of short_ties() are the ties themselves (they come first)."""
    return len(_short_ties()[0])


def sam_float_texts():
    """Random binary32 values in three notations, exact midpoints of 2,000 of them (far past 19
    digits), hand-written edges, short_ties(), and SAM_BAD last."""
    return list(_sam_base_texts()) + short_ties() + SAM_BAD


# ------------------------------------------------------------------ binary64 (QUAL) texts
@functools.lru_cache(maxsize=None)
def _qual_random_texts():
    rng = random.Random(20241019)
    texts = []
    while len(texts) < 60000:
        x = struct.unpack("<d", struct.pack("<Q", rng.getrandbits(64)))[0]
        if x != x or x in (float("inf"), float("-inf")):
            continue
        y = rng.uniform(-1e6, 1e6) if len(texts) % 2 else x   # QUAL-like magnitudes and any double
        texts += ["%.2f" % y if abs(y) < 1e30 else "%.2f" % rng.uniform(0, 1e5), "%.6g" % y, "%.17g" % y]
    return tuple(texts)


N_QUAL_RANDOM = 60000


@functools.lru_cache(maxsize=None)
def _qual_edge_texts():
    """15-digit mantissas at the decimal exponents where the device's exact path ends: as the
    15-digit integer times 10^x, x = +-21 and +-22 stay on the device, +-23 go to the host; each
    also with the point behind its first digit (the same value: 14 more in the exponent)."""
    rng = random.Random(20250312)
    texts = []
    for x in (-22, -21, 21, 22, 23, -23):
        for i in range(100):
            d = str(rng.randrange(10 ** 14, 10 ** 15))
            sign = "-" if i % 10 == 9 else ""
            texts.append("%s%se%d" % (sign, d, x))
            texts.append("%s%s.%sE%+d" % (sign, d[0], d[1:], x + 14))
    return tuple(texts)


def qual_edge_texts():
    return list(_qual_edge_texts())


def qual_texts():
    """N_QUAL_RANDOM texts of random doubles and QUAL-like magnitudes (%.2f, %.6g, %.17g in turn),
    then qual_edge_texts()."""
    return list(_qual_random_texts()) + qual_edge_texts()
