"""Test helper: decimal text -> the correctly rounded IEEE binary32 / binary64 bit pattern, worked
out with Python integers alone (no libc call, no float()): the reference of the float tests that
is independent of strtof / strtod, which the library's own fix-up path calls.  Round to nearest,
ties to even; subnormals, overflow to infinity, underflow to a signed zero."""
import re

BINARY32 = "binary32"
BINARY64 = "binary64"

# (precision p in bits with the hidden one, minimum normal exponent, bytes)
_FMT = {BINARY32: (24, -126, 4), BINARY64: (53, -1022, 8)}

# the union of what the SAM float rule and the VCF QUAL rule accept: an optional sign, digits with
# at most one point and at least one digit, an optional exponent
_TEXT = re.compile(rb"([-+]?)([0-9]*)(?:\.([0-9]*))?(?:[eE]([-+]?[0-9]+))?\Z")

# A decimal magnitude past these needs no power: 10^400 is above every finite binary64 and 10^-400
# is below half the smallest subnormal (2^-1075 > 10^-324).
_E10_MAX = 400
_DIGITS_MAX = 1000


def exact_bits(text: bytes, fmt=BINARY32) -> int:
    """The bit pattern of the binary32 / binary64 nearest to the decimal `text` (ties to even)."""
    p, emin, size = _FMT[fmt]
    m = _TEXT.match(text)
    if not m or not (m.group(2) or m.group(3)):
        raise ValueError(text)
    sign = 1 << (8 * size - 1) if m.group(1) == b"-" else 0
    ip, fp = m.group(2), m.group(3) or b""
    digits = (ip + fp).lstrip(b"0")
    if not digits:
        return sign
    inf = ((1 << (8 * size - p)) - 1) << (p - 1)           # exponent field all ones, fraction 0
    q = int(m.group(4) or 0) - len(fp)                     # value = digits * 10^q
    if len(digits) > _DIGITS_MAX:
        # a rounding boundary of either format has fewer than _DIGITS_MAX significant digits (a
        # binary64 midpoint has at most 768), so which side of every boundary the value lies on
        # shows in that many digits and one more that says whether anything non-zero follows
        q += len(digits) - _DIGITS_MAX
        digits = digits[:_DIGITS_MAX] + (b"1" if digits[_DIGITS_MAX:].strip(b"0") else b"0")
        q -= 1
    w = int(digits)
    # 10^(mag - 1) <= value < 10^mag: clamped before any power is formed
    mag = q + len(str(w))
    if mag > _E10_MAX:
        return sign | inf
    if mag < -_E10_MAX:
        return sign
    num, den = (w * 10 ** q, 1) if q >= 0 else (w, 10 ** -q)
    # e = floor(log2(value))
    e = num.bit_length() - den.bit_length()
    if (num << -e if e < 0 else num) < (den << e if e > 0 else den):
        e -= 1
    E = max(e, emin)                                       # the exponent the value is rounded at
    s = E - (p - 1)                                        # one ulp = 2^s
    if s >= 0:
        den <<= s
    else:
        num <<= -s
    n, r = divmod(num, den)                                # value / ulp = n + r / den
    if 2 * r > den or (2 * r == den and n & 1):
        n += 1
    # n < 2^(p-1): subnormal (E = emin, field 0); else the hidden bit carries into the field, and
    # so does n == 2^p after rounding up
    bits = n + ((E - emin) << (p - 1))
    return sign | min(bits, inf)


def exact_bytes(text: bytes, fmt=BINARY32) -> bytes:
    """exact_bits as the little-endian bytes a record or a column holds."""
    return exact_bits(text, fmt).to_bytes(_FMT[fmt][2], "little")
