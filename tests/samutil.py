"""Test helper: SAM text <-> BAM records in plain Python -- htsjdk 2.16 SAMLineParser.parseLine +
BAMRecordCodec.encode + BinaryTagCodec as SamSource.getReads runs them
(D/impl/formats/sam/SamSource.java:36-77), restated in DESIGN.md "SAM text rules" -- and Hadoop's
rule for the lines of an uncompressed split.  It shares no code with the library: it is the
oracle a device SAM reader has to reproduce byte for byte.  Floats go through libc strtof (the
correctly rounded conversion that Float.parseFloat makes)."""
import ctypes
import re
import struct

SEQ_CODE = "=ACMGRSVTWYHKDBN"
CIGAR_CODE = "MIDNSHP=X"
FLOAT_RE = re.compile(rb"[-+]?[0-9]*\.?[0-9]+([eE][-+]?[0-9]+)?\Z")
COLUMNS = ("QNAME", "FLAG", "RNAME", "POS", "MAPQ", "CIGAR", "RNEXT", "PNEXT", "TLEN", "SEQ", "QUAL")

_libc = ctypes.CDLL(None)
_libc.strtof.restype = ctypes.c_float
_libc.strtof.argtypes = [ctypes.c_char_p, ctypes.c_void_p]


class SamError(ValueError):
    """what = a column name, "fields" or "tag XX"."""

    def __init__(self, what):
        super().__init__(what)
        self.what = what


def pack_float(text: bytes) -> bytes:
    if not FLOAT_RE.match(text):
        raise ValueError(text)
    return struct.pack("<f", _libc.strtof(text, None))


def reg2bin(beg, end):
    end -= 1
    for sh, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> sh == end >> sh:
            return base + (beg >> sh)
    return 0


def _i32(v):
    v &= 0xffffffff
    return v - (1 << 32) if v >= 1 << 31 else v


# ------------------------------------------------------------------ BAM record -> SAM line
def _fmt_float(raw4):
    import numpy as np
    return repr(float(np.frombuffer(raw4, "<f4")[0])).encode()


def bam_record_to_sam_line(rec: bytes, ref_names) -> bytes:
    """`rec` = block_size word + record; the line has no terminator."""
    (bs, ref_id, pos, l_rn, mapq, _bin, n_cig, flag, l_seq, nref, npos, tlen) = \
        struct.unpack_from("<iiiBBHHHiiii", rec, 0)
    assert 4 + bs == len(rec)
    p = 36
    name = rec[p:p + l_rn - 1]
    p += l_rn
    cig = b"".join(b"%d%c" % (op >> 4, ord(CIGAR_CODE[op & 15]))
                   for op in struct.unpack_from(f"<{n_cig}I", rec, p)) or b"*"
    p += 4 * n_cig
    sb = rec[p:p + (l_seq + 1) // 2]
    seq = "".join(SEQ_CODE[b >> 4] + SEQ_CODE[b & 15] for b in sb)[:l_seq].encode() or b"*"
    p += (l_seq + 1) // 2
    q = rec[p:p + l_seq]
    qual = b"*" if (l_seq == 0 or all(x == 0xff for x in q)) else bytes(x + 33 for x in q)
    p += l_seq
    rname = b"*" if ref_id < 0 else ref_names[ref_id].encode()
    rnext = b"*" if nref < 0 else (b"=" if nref == ref_id else ref_names[nref].encode())
    out = [name, b"%d" % flag, rname, b"%d" % (pos + 1), b"%d" % mapq, cig, rnext,
           b"%d" % (npos + 1), b"%d" % tlen, seq, qual]
    ints = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}
    while p < len(rec):
        tag, ty = rec[p:p + 2], chr(rec[p + 2])
        p += 3
        if ty == "A":
            out.append(tag + b":A:" + rec[p:p + 1])
            p += 1
        elif ty in ints:
            n = struct.calcsize(ints[ty])
            out.append(tag + b":i:%d" % struct.unpack_from(ints[ty], rec, p)[0])
            p += n
        elif ty == "f":
            out.append(tag + b":f:" + _fmt_float(rec[p:p + 4]))
            p += 4
        elif ty in "ZH":
            e = rec.index(b"\0", p)
            out.append(tag + b":" + ty.encode() + b":" + rec[p:e])
            p = e + 1
        elif ty == "B":
            sub = chr(rec[p])
            cnt = struct.unpack_from("<i", rec, p + 1)[0]
            p += 5
            if sub == "f":
                vals = [_fmt_float(rec[p + 4 * k:p + 4 * k + 4]) for k in range(cnt)]
                p += 4 * cnt
            else:
                n = struct.calcsize(ints[sub])
                vals = [b"%d" % v for v in struct.unpack_from("<%d%s" % (cnt, ints[sub][1]), rec, p)]
                p += n * cnt
            out.append(tag + b":B:" + sub.encode() + b"".join(b"," + v for v in vals))
        else:
            raise ValueError(f"tag type {ty!r}")
    return b"\t".join(out)


# ------------------------------------------------------------------ SAM line -> BAM record
def _dec(text, col, lo, hi, signed=False):
    pat = rb"[-+]?[0-9]+\Z" if signed else rb"[0-9]+\Z"
    if not re.match(pat, text):
        raise SamError(col)
    v = int(text)
    if not lo <= v <= hi:
        raise SamError(col)
    return v


def _ref(name, ref_names, col):
    try:
        return ref_names.index(name.decode("latin-1"))
    except ValueError:
        raise SamError(col)


_B_RANGE = {"c": (-128, 127), "C": (0, 255), "s": (-32768, 32767), "S": (0, 65535),
            "i": (-2 ** 31, 2 ** 31 - 1), "I": (0, 2 ** 32 - 1)}
_B_FMT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}


def _tag(field: bytes) -> bytes:
    what = "tag " + field[:2].decode("latin-1")
    if len(field) < 5 or field[2:3] != b":" or field[4:5] != b":":
        raise SamError(what)
    tag, ty, val = field[:2], chr(field[3]), field[5:]
    if ty == "A":
        if len(val) != 1 or not 33 <= val[0] <= 126:
            raise SamError(what)
        return tag + b"A" + val
    if ty == "i":
        if not re.match(rb"[-+]?[0-9]+\Z", val):
            raise SamError(what)
        v = int(val)
        if not -2 ** 31 <= v < 2 ** 32:
            raise SamError(what)
        if v > 2147483647:
            t = "I"
        elif v > 65535:
            t = "i"
        elif v > 32767:
            t = "S"
        elif v > 255:
            t = "s"
        elif v > 127:
            t = "C"
        elif v >= -128:
            t = "c"
        elif v >= -32768:
            t = "s"
        else:
            t = "i"
        return tag + t.encode() + struct.pack(_B_FMT[t], v)
    if ty == "Z":
        return tag + b"Z" + val + b"\0"
    if ty == "H":
        if len(val) % 2 or not re.match(rb"[0-9A-F]*\Z", val):
            raise SamError(what)
        return tag + b"H" + val + b"\0"
    if ty == "f":
        if not FLOAT_RE.match(val):
            raise SamError(what)
        return tag + b"f" + pack_float(val)
    if ty == "B":
        sub = chr(val[0]) if val else ""
        if sub not in "cCsSiIf" or not sub or (len(val) > 1 and val[1:2] != b","):
            raise SamError(what)
        items = val[2:].split(b",") if len(val) > 1 else []
        out = tag + b"B" + sub.encode() + struct.pack("<i", len(items))
        for it in items:
            if sub == "f":
                if not FLOAT_RE.match(it):
                    raise SamError(what)
                out += pack_float(it)
            else:
                if not re.match(rb"[-+]?[0-9]+\Z", it):
                    raise SamError(what)
                v = int(it)
                if not _B_RANGE[sub][0] <= v <= _B_RANGE[sub][1]:
                    raise SamError(what)
                out += struct.pack(_B_FMT[sub], v)
        return out
    raise SamError(what)


def sam_line_to_bam_record(line: bytes, ref_names) -> bytes:
    """The record's bytes (block_size word included); SamError names the offending column/tag."""
    f = line.split(b"\t")
    if len(f) < 11:
        raise SamError("fields")
    if not 1 <= len(f[0]) <= 254:
        raise SamError("QNAME")
    flag = _dec(f[1], "FLAG", 0, 65535)
    ref = -1 if f[2] == b"*" else _ref(f[2], ref_names, "RNAME")
    pos = _dec(f[3], "POS", 0, 2 ** 31 - 1)
    mapq = _dec(f[4], "MAPQ", 0, 255)
    if f[6] == b"=":
        nref = ref
    elif f[6] == b"*":
        nref = -1
    else:
        nref = _ref(f[6], ref_names, "RNEXT")
    pnext = _dec(f[7], "PNEXT", 0, 2 ** 31 - 1)
    tlen = _dec(f[8], "TLEN", -2 ** 31, 2 ** 31 - 1, signed=True)
    seq_star, qual_star = f[9] == b"*", f[10] == b"*"
    l_seq = 0 if seq_star else len(f[9])
    if not seq_star and l_seq < 1:
        raise SamError("SEQ")
    if not qual_star and len(f[10]) != l_seq:
        raise SamError("QUAL")
    ops, reflen = [], 0
    if f[5] != b"*":
        if not re.match(rb"([0-9]+[^0-9])+\Z", f[5]):
            raise SamError("CIGAR")
        for n, op in re.findall(rb"([0-9]+)([^0-9])", f[5]):
            k = CIGAR_CODE.find(op.decode("latin-1"))
            if k < 0 or len(n) > 10 or not 1 <= int(n) <= 2 ** 28 - 1:
                raise SamError("CIGAR")
            ops.append(int(n) << 4 | k)
            if op in b"MDN=X":
                reflen += int(n)
        if len(ops) > 65535:
            raise SamError("CIGAR")
    seq = bytearray((l_seq + 1) // 2)
    if not seq_star:
        for i, c in enumerate(f[9]):
            ch = "N" if c == ord(".") else chr(c).upper()
            k = SEQ_CODE.find(ch) if c < 128 else -1
            if k < 0:
                raise SamError("SEQ")
            seq[i >> 1] |= k << (0 if i & 1 else 4)
    if qual_star:
        qual = b"\xff" * l_seq
    else:
        if any(c < 33 for c in f[10]):
            raise SamError("QUAL")
        qual = bytes((c - 33) & 0xff for c in f[10])
    tags = b"".join(_tag(t) for t in f[11:])
    beg = _i32(pos - 1)
    end = 0 if flag & 4 else _i32(beg + reflen)
    if end <= 0:
        end = _i32(beg + 1)
    body = struct.pack("<iiBBHHHiiii", ref, beg, len(f[0]) + 1, mapq, reg2bin(beg, end) & 0xffff,
                       len(ops), flag, l_seq, nref, _i32(pnext - 1), tlen)
    body += f[0] + b"\0" + struct.pack(f"<{len(ops)}I", *ops) + bytes(seq) + qual + tags
    return struct.pack("<i", len(body)) + body


# ------------------------------------------------------------------ headers and whole files
def sam_header_to_bam(text: bytes):
    """The leading '@' lines as a BAM header, and the @SQ names."""
    lines, p = [], 0
    while p < len(text) and text[p:p + 1] == b"@":
        m = re.compile(rb"\r\n|\n|\r").search(text, p)
        e, nx = (m.start(), m.end()) if m else (len(text), len(text))
        lines.append(text[p:e])
        p = nx
    names, lens = [], []
    for l in lines:
        if l.startswith(b"@SQ\t"):
            kv = dict(x.split(b":", 1) for x in l.split(b"\t")[1:] if b":" in x)
            names.append(kv[b"SN"].decode())
            lens.append(int(kv[b"LN"]))
    t = b"".join(l + b"\n" for l in lines)
    h = b"BAM\x01" + struct.pack("<i", len(t)) + t + struct.pack("<i", len(names))
    for n, ln in zip(names, lens):
        h += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", ln)
    return h, names


def text_lines(data: bytes):
    """(offset of the first byte, value) of every line: LF, CR LF or a lone CR end a line, a last
    line without a terminator counts."""
    out, a, i, n = [], 0, 0, len(data)
    while i < n:
        c = data[i]
        if c == 10:
            out.append((a, data[a:i])); i += 1; a = i
        elif c == 13:
            out.append((a, data[a:i])); i += 2 if i + 1 < n and data[i + 1] == 10 else 1; a = i
        else:
            i += 1
    if a < n:
        out.append((a, data[a:]))
    return out


def plain_text_partitions(data: bytes, splits):
    """Hadoop 2.7 LineRecordReader over the uncompressed splits [(start, end)]: per split the list
    of (line offset, value).  A line whose first byte is at s belongs to the split with
    start < s <= end, offset 0 to the first split; a UTF-8 BOM at offset 0 is dropped from the
    first value (a line of only the BOM and no terminator is no record)."""
    lines = text_lines(data)
    if lines and data.startswith(b"\xef\xbb\xbf"):
        off, v = lines[0]
        if len(v) == 3 and len(data) == 3:
            lines = []
        else:
            lines[0] = (off, v[3:])
    import bisect
    offs = [o for o, _ in lines]  # ascending
    parts = []
    for i, (s, e) in enumerate(splits):
        lo = 0 if i == 0 else bisect.bisect_right(offs, s)   # first line start > s (or offset 0)
        hi = bisect.bisect_right(offs, e)                    # first line start > e
        parts.append(lines[lo:max(lo, hi)])
    return parts


def sam_records(text: bytes, ref_names=None):
    """[(line index, line offset, record bytes)] of every line that does not start with '@'."""
    if ref_names is None:
        ref_names = sam_header_to_bam(text)[1]
    out = []
    for k, (o, v) in enumerate(text_lines(text)):
        if v.startswith(b"@"):
            continue
        out.append((k, o, sam_line_to_bam_record(v, ref_names)))
    return out


def bam_to_sam_text(bam_inflated: bytes, newline=b"\n") -> bytes:
    """A whole inflated BAM stream as SAM text: the header text, then a line per record."""
    l_text = struct.unpack_from("<i", bam_inflated, 4)[0]
    text = bam_inflated[8:8 + l_text].rstrip(b"\0")
    p = 8 + l_text
    n_ref = struct.unpack_from("<i", bam_inflated, p)[0]
    p += 4
    names = []
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", bam_inflated, p)[0]
        names.append(bam_inflated[p + 4:p + 4 + ln - 1].decode())
        p += 8 + ln
    out = [text if (not text or text.endswith(b"\n")) else text + b"\n"]
    while p < len(bam_inflated):
        bs = struct.unpack_from("<i", bam_inflated, p)[0]
        out.append(bam_record_to_sam_line(bam_inflated[p:p + 4 + bs], names) + newline)
        p += 4 + bs
    return b"".join(out)
