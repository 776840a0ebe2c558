"""Test helper: BAM records -> SAM lines in plain Python, the oracle of the SAM writer
(DESIGN.md section 14): htsjdk 2.16 SAMTextWriter.getSAMString + TextTagCodec, then Java's
String.trim, as SamSink.save maps every read (D/impl/formats/sam/SamSink.java:37).  It shares no
code with the library.  Floats are Java's Float.toString (the JDK 19+ contract) worked out with
fractions.Fraction; samutil is used for nothing here, its own converter is careless about floats,
trim and malformed records."""
import functools
import struct
from fractions import Fraction

SEQ_CODE = b"=ACMGRSVTWYHKDBN"
CIGAR_CODE = b"MIDNSHP=X"
_WS = bytes(range(0x21))  # what String.trim removes at both ends
_INT = {ord("c"): "<b", ord("C"): "<B", ord("s"): "<h", ord("S"): "<H", ord("i"): "<i", ord("I"): "<I"}


class SamWriteError(ValueError):
    """what = "fields", a column name or "tag XX" (the reader's vocabulary)."""

    def __init__(self, what):
        super().__init__(what)
        self.what = what


# ------------------------------------------------------------------ Float.toString
def float_decimal(bits: int):
    """Digits and exponent of a finite non-zero binary32 (sign ignored): (c, n, e) with the value
    printed as the n-digit integer c times 10^e.  R = the decimals that read back to the same bits
    under round to nearest, ties to even; n = the fewest digits any member of R has, but 2 where
    that is 1 (Float.toString's own clause: it always renders two digits, and picks them as the
    nearest two-digit decimal, which is why the smallest subnormal prints as 1.4E-45 and not
    1.0E-45); of R's n-digit members the nearest to the value, on a tie the even one."""
    exp, frac = (bits >> 23) & 0xff, bits & 0x7fffff
    assert exp != 0xff and (exp or frac)
    m, e2 = (frac, -149) if exp == 0 else (frac | 1 << 23, exp - 150)
    v = Fraction(m) * Fraction(2) ** e2
    half = Fraction(2) ** (e2 - 1)
    lo = v - (half / 2 if (frac == 0 and exp > 1) else half)   # the binade's first value: lopsided
    hi = v + half
    closed = m % 2 == 0

    def inside(x):
        return lo <= x <= hi if closed else lo < x < hi

    E = 0                                                      # 10^E <= v < 10^(E+1)
    while Fraction(10) ** E > v:
        E -= 1
    while Fraction(10) ** (E + 1) <= v:
        E += 1

    def members(n):
        scale = Fraction(10) ** (E - n + 1)
        c = (v / scale).__floor__()
        return [(k, E - n + 1) for k in (c, c + 1) if k > 0 and inside(k * scale)]

    for n in range(1, 10):
        T = members(n)
        if T:
            break
    else:
        raise AssertionError("nine digits always suffice for a binary32")
    if n == 1:
        n = 2
        T = members(2)
    best = min(T, key=lambda t: (abs(t[0] * Fraction(10) ** t[1] - v), t[0] % 2))
    return best[0], n, best[1]


@functools.lru_cache(maxsize=None)
def float_text(bits: int) -> bytes:
    """Float.toString of the binary32 with these bits (worked out once per value)."""
    bits &= 0xffffffff
    exp, frac = (bits >> 23) & 0xff, bits & 0x7fffff
    sign = b"-" if bits >> 31 else b""
    if exp == 0xff:
        return b"NaN" if frac else sign + b"Infinity"
    if not exp and not frac:
        return sign + b"0.0"
    c, _, e = float_decimal(bits)
    s = str(c)
    e10 = e + len(s) - 1                  # exponent of the first digit
    d = s.rstrip("0")                     # at least one digit follows the point below
    if -3 <= e10 <= 6:                    # 1e-3 <= |x| < 1e7: plain notation
        if e10 < 0:
            t = "0." + "0" * (-e10 - 1) + d
        else:
            ip = d[:e10 + 1].ljust(e10 + 1, "0")
            t = ip + "." + (d[e10 + 1:] or "0")
    else:
        t = d[0] + "." + (d[1:] or "0") + "E" + str(e10)
    return sign + t.encode()


# ------------------------------------------------------------------ one record -> one line
def record_to_sam_line(rec: bytes, ref_names) -> bytes:
    """rec = block_size word + block_size bytes.  The trimmed line without its LF.  Checks run in
    this order and the first failure is raised: fields (the layout), QNAME, RNAME, CIGAR, RNEXT,
    QUAL, then the tags as stored."""
    if len(rec) < 36:
        raise SamWriteError("fields")
    (bs, ref_id, pos, l_rn, mapq, _bin, n_cig, flag, l_seq, nref, npos, tlen) = \
        struct.unpack_from("<iiiBBHHHiiii", rec, 0)
    if bs != len(rec) - 4 or l_seq < 0 or 32 + l_rn + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs:
        raise SamWriteError("fields")
    if l_rn < 2:
        raise SamWriteError("QNAME")
    n_ref = len(ref_names)
    if not -1 <= ref_id < n_ref:
        raise SamWriteError("RNAME")
    p = 36
    qname = rec[p:p + l_rn - 1]
    p += l_rn
    cig = b""
    for w in struct.unpack_from("<%dI" % n_cig, rec, p):
        if w & 15 > 8:
            raise SamWriteError("CIGAR")
        cig += b"%d%c" % (w >> 4, CIGAR_CODE[w & 15])
    p += 4 * n_cig
    if not -1 <= nref < n_ref:
        raise SamWriteError("RNEXT")
    sb = rec[p:p + (l_seq + 1) // 2]
    seq = bytes(SEQ_CODE[(sb[i >> 1] >> (0 if i & 1 else 4)) & 15] for i in range(l_seq))
    p += (l_seq + 1) // 2
    q = rec[p:p + l_seq]
    p += l_seq
    if l_seq == 0 or all(x == 0xff for x in q):
        qual = b"*"
    else:
        if any(x > 93 for x in q):
            raise SamWriteError("QUAL")
        qual = bytes(x + 33 for x in q)

    def name(r):
        n = ref_names[r]
        return n if isinstance(n, bytes) else n.encode("latin-1")

    i32 = lambda x: ((x + 2 ** 31) & 0xffffffff) - 2 ** 31
    out = [qname, b"%d" % flag, b"*" if ref_id < 0 else name(ref_id), b"%d" % i32(pos + 1),
           b"%d" % mapq, cig or b"*",
           b"*" if nref < 0 else (b"=" if nref == ref_id else name(nref)),
           b"%d" % i32(npos + 1), b"%d" % tlen, seq or b"*", qual]
    end = len(rec)
    while p < end:
        if end - p < 3:
            raise SamWriteError("tag ")
        tag, ty = rec[p:p + 2], rec[p + 2]
        err = SamWriteError("tag " + tag.decode("latin-1"))
        p += 3

        def need(n):
            if n < 0 or p + n > end:
                raise err

        if ty == ord("A"):
            need(1)
            out.append(tag + b":A:" + rec[p:p + 1])
            p += 1
        elif ty in _INT:
            n = struct.calcsize(_INT[ty])
            need(n)
            out.append(tag + b":i:%d" % struct.unpack_from(_INT[ty], rec, p)[0])
            p += n
        elif ty == ord("f"):
            need(4)
            out.append(tag + b":f:" + float_text(struct.unpack_from("<I", rec, p)[0]))
            p += 4
        elif ty in b"ZH":
            z = rec.find(b"\0", p)
            if z < 0:
                raise err
            val = rec[p:z]
            if ty == ord("H"):
                if len(val) % 2 or any(c not in b"0123456789abcdefABCDEF" for c in val):
                    raise err
                val = val.upper()
            out.append(tag + b":" + bytes([ty]) + b":" + val)
            p = z + 1
        elif ty == ord("B"):
            need(5)
            sub, cnt = rec[p], struct.unpack_from("<i", rec, p + 1)[0]
            p += 5
            if sub == ord("f"):
                size = 4
            elif sub in _INT:
                size = struct.calcsize(_INT[sub])
            else:
                raise err
            if cnt < 0:
                raise err
            need(size * cnt)
            if sub == ord("f"):
                vals = [float_text(x) for x in struct.unpack_from("<%dI" % cnt, rec, p)]
            else:
                vals = [b"%d" % x for x in struct.unpack_from("<%d%s" % (cnt, _INT[sub][1]), rec, p)]
            p += size * cnt
            out.append(tag + b":B:" + bytes([sub]) + b"".join(b"," + x for x in vals))
        else:
            raise err
    return b"\t".join(out).lstrip(_WS).rstrip(_WS)


def split_records(raw: bytes):
    """The records of a back-to-back run (block_size chain)."""
    out, p = [], 0
    while p < len(raw):
        bs = struct.unpack_from("<i", raw, p)[0]
        out.append(raw[p:p + 4 + bs])
        p += 4 + bs
    return out


def records_to_sam_text(recs, ref_names):
    """(text, None) with every line followed by LF, or (None, "record <k>: <what>") for the first
    record in input order that fails."""
    out = []
    for k, r in enumerate(recs):
        try:
            out.append(record_to_sam_line(r, ref_names) + b"\n")
        except SamWriteError as e:
            return None, "record %d: %s" % (k, e.what)
    return b"".join(out), None


def header_ref_names(header: bytes):
    """The reference names of a BAM header (magic, l_text, text, n_ref, references), as bytes."""
    l_text = struct.unpack_from("<i", header, 4)[0]
    p = 8 + l_text
    n = struct.unpack_from("<i", header, p)[0]
    p += 4
    names = []
    for _ in range(n):
        ln = struct.unpack_from("<i", header, p)[0]
        names.append(header[p + 4:p + 4 + ln - 1])
        p += 8 + ln
    return names


def header_text(header: bytes) -> bytes:
    """SamSink's header file: the text inside the BAM header, ending in one LF (empty stays empty)."""
    l_text = struct.unpack_from("<i", header, 4)[0]
    t = header[8:8 + l_text].rstrip(b"\0")
    return t if (not t or t.endswith(b"\n")) else t + b"\n"


# ------------------------------------------------------------------ shared test inputs
FLOAT_PAIRS = [
    (0x3f800000, b"1.0"), (0x3dcccccd, b"0.1"), (0x3a83126f, b"0.001"), (0x38d1b717, b"1.0E-4"),
    (0x4b189680, b"1.0E7"), (0x4b18967f, b"9999999.0"), (0x15ae43fd, b"7.038531E-26"),
    (0x00000001, b"1.4E-45"), (0x00800000, b"1.1754944E-38"), (0x7f7fffff, b"3.4028235E38"),
    (0x7f800000, b"Infinity"), (0xffc00000, b"NaN"), (0x80000000, b"-0.0"),
    (0xff800000, b"-Infinity"), (0x00000000, b"0.0"), (0x7fc00001, b"NaN"),
    (0x42c80000, b"100.0"), (0xc2c80000, b"-100.0"), (0x3fc00000, b"1.5"), (0x40490fdb, b"3.1415927"),
    (0x00000002, b"2.8E-45"), (0x00000007, b"9.8E-45"), (0x00000008, b"1.1E-44"),
    (0x501502f9, b"1.0E10"), (0x49742400, b"1000000.0"), (0x3a83126e, b"9.999999E-4"),
    (0x7e967699, b"1.0E38"), (0x4cbebc20, b"1.0E8"), (0x3e800000, b"0.25"), (0x461c4000, b"10000.0"),
]


def binade_edges():
    """The first two and last two mantissas of every binade (subnormals: of the subnormal range),
    both signs left to the caller: where the rounding interval is lopsided."""
    out = []
    for e in range(0, 255):
        for f in (0, 1, 0x7ffffe, 0x7fffff):
            b = e << 23 | f
            if b:
                out.append(b)
    return out


def random_finite(n, seed):
    import numpy as np
    r = np.random.default_rng(seed).integers(0, 2 ** 32, size=n + n // 64 + 16, dtype=np.uint64)
    r = r[(r >> 23) & 0xff != 0xff][:n]
    assert len(r) == n
    return [int(x) for x in r]


def float_set(n_random, seed=7):
    """The float inputs of the CPU and GPU tests: the hand-written ones, the binade edges, small
    integers and halves (exact values, trailing zeros, rounding ties), small subnormals, randoms."""
    s = [b for b, _ in FLOAT_PAIRS] + binade_edges()
    s += [struct.unpack("<I", struct.pack("<f", x / 2))[0] for x in range(1, 600)]
    s += [struct.unpack("<I", struct.pack("<f", float(10 ** k)))[0] for k in range(0, 39)]
    s += [struct.unpack("<I", struct.pack("<f", 10.0 ** -k))[0] for k in range(1, 46)]
    s += list(range(1, 1200)) + [0x80000000 | x for x in range(1, 40)]
    s += random_finite(n_random, seed)
    return s


# ------------------------------------------------------------------ hand-built records
REFS = [b"chr1", b"chr2", b"HLA-A*01:01"]


def bam_header(refs=REFS, text=b"@HD\tVN:1.5\tSO:unsorted\n"):
    h = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for n in refs:
        h += struct.pack("<i", len(n) + 1) + n + b"\0" + struct.pack("<i", 1000000)
    return h


def make_record(qname=b"r1", flag=0, ref=0, pos=99, mapq=30, cigar=(4 << 4,), nref=-1, npos=-1,
                tlen=0, seq=b"\x12\x48", l_seq=4, qual=b"((((", tags=b"", l_rn=None, n_cig=None,
                bs=None):
    """A record from its parts; l_rn, n_cig and bs override the counts the parts give."""
    body = struct.pack("<iiBBHHHiiii", ref, pos, len(qname) + 1 if l_rn is None else l_rn, mapq, 4680,
                       len(cigar) if n_cig is None else n_cig, flag, l_seq, nref, npos, tlen)
    body += qname + b"\0" + struct.pack("<%dI" % len(cigar), *cigar) + seq + qual + tags
    return struct.pack("<i", len(body) if bs is None else bs) + body


def trim_cases():
    """Records whose line String.trim changes, and two it must leave alone."""
    return [make_record(tags=b"XZZabc  \0"), make_record(tags=b"XAA "),
            make_record(qname=b"\x1fname"), make_record(qname=b"  "),
            make_record(tags=b"XZZ  \0"), make_record(tags=b"XZZa  \0XYZb\0"),
            make_record(tags=b"XAA XBAb"), make_record(qname=b" a b "),
            make_record(tags=b"NMC\x05XZZ\t\0")]


def error_cases():
    """(record, what): one malformed record per error class, then records with two faults, where
    the first failing check in column order is reported."""
    i = struct.pack
    return [
        (make_record(l_seq=-1), "fields"), (make_record(l_seq=100), "fields"),
        (i("<i", 8) + b"\0" * 8, "fields"), (make_record(n_cig=50), "fields"),
        (make_record(qname=b"", l_rn=1, seq=b"\0\x12\x48"), "QNAME"),
        (make_record(qname=b"", l_rn=0, seq=b"\0\x12\x48"), "QNAME"),
        (make_record(ref=3), "RNAME"), (make_record(ref=-2), "RNAME"),
        (make_record(cigar=(4 << 4 | 9,)), "CIGAR"), (make_record(cigar=(1 << 4, 3 << 4 | 15)), "CIGAR"),
        (make_record(nref=3), "RNEXT"), (make_record(nref=-2), "RNEXT"),
        (make_record(qual=b"((^("), "QUAL"), (make_record(qual=b"(\xff(("), "QUAL"),
        (make_record(qual=b"\xff\xff\xff\xfe"), "QUAL"),
        (make_record(tags=b"XQq\x01"), "tag XQ"), (make_record(tags=b"XBBx" + i("<i", 0)), "tag XB"),
        (make_record(tags=b"XBBc" + i("<i", -1)), "tag XB"), (make_record(tags=b"XIi\x01\x02"), "tag XI"),
        (make_record(tags=b"XBBs" + i("<i", 3) + b"\1\0\2\0\3"), "tag XB"),
        (make_record(tags=b"XBBi" + i("<i", 0x40000000) + b"\0" * 8), "tag XB"),
        (make_record(tags=b"XZZabc"), "tag XZ"), (make_record(tags=b"XHH0A"), "tag XH"),
        (make_record(tags=b"XHH0AB\0"), "tag XH"), (make_record(tags=b"XHH0G\0"), "tag XH"),
        (make_record(tags=b"XAA"), "tag XA"), (make_record(tags=b"XFf\0\0\0"), "tag XF"),
        (make_record(tags=b"XBBc\x01\0\0"), "tag XB"),
        (make_record(tags=b"NMC\x01X"), "tag "), (make_record(tags=b"NMC\x01XY"), "tag "),
        # the order of checks
        (make_record(ref=3, cigar=(4 << 4 | 9,)), "RNAME"), (make_record(cigar=(4 << 4 | 9,), nref=7), "CIGAR"),
        (make_record(qual=b"((^(", tags=b"XQq\x01"), "QUAL"), (make_record(l_seq=-1, qname=b"", l_rn=1), "fields"),
        (make_record(nref=9, qual=b"\x60(((",), "RNEXT"), (make_record(tags=b"XAAaXQq\x01XZZabc"), "tag XQ"),
    ]
