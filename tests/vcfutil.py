"""The VCF site decode in plain Python, written from DESIGN.md section 15 (htsjdk 2.16
AbstractVCFCodec.parseVCFLine restated), not from disq_amd/csrc/dq_vcf_core.h: the oracle of the
dq_vcf_* tests.  vcf_header(text) -> (G, contigs); vcf_decode_line(value, G, contigs) -> the fields
of one data line, or raises VcfError(what) with the class of the first failing check."""
import re

from textutil import split_lines

HAS_ID, HAS_QUAL, UNFILTERED, PASS, INFO_END, HAS_GENOTYPES, SYMBOLIC, REF_LOWER = (
    1, 2, 4, 8, 16, 32, 64, 128)

INT_RE = re.compile(rb"[-+]?[0-9]+\Z")
QUAL_RE = re.compile(rb"[-+]?([0-9]+\.?[0-9]*|\.[0-9]+)([eE][-+]?[0-9]+)?\Z")
BASES = frozenset(b"ACGTNacgtn")


class VcfError(Exception):
    def __init__(self, what):
        super().__init__(what)
        self.what = what


def vcf_header(text):
    """(G, contigs) of the leading '#' lines: G = the #CHROM line has a non-empty tenth column,
    contigs = the IDs of the ##contig=<...> lines in order.  Raises VcfError("header") when data
    lines follow a header without a #CHROM line."""
    if text[:3] == b"\xef\xbb\xbf":
        text = text[3:]
    G, chrom, contigs, data = False, False, [], False
    for line in split_lines(text):
        if not line.startswith(b"#"):
            data = True
            break
        if line.startswith(b"#CHROM") and not chrom:
            chrom = True
            cols = line.split(b"\t")
            G = len(cols) >= 10 and len(cols[9]) > 0
        elif line.startswith(b"##contig=<"):
            end = line.rfind(b">")
            body = line[10:end] if end >= 10 else line[10:]
            for piece in body.split(b","):
                if piece.startswith(b"ID="):
                    contigs.append(piece[3:])
                    break
    if data and not chrom:
        raise VcfError("header")
    return G, contigs


def parse_int(t):
    """Java Integer.valueOf, or None."""
    if not INT_RE.match(t):
        return None
    v = int(t)
    return v if -2 ** 31 <= v < 2 ** 31 else None


def qual_fast_path(t):
    """The QUAL text is converted on the device: an integer digit, at most 15 significant digits
    (zeros may follow) and a decimal exponent of that 15-digit integer in -22..22, or a zero."""
    m = re.match(rb"[-+]?([0-9]*)\.?([0-9]*)(?:[eE]([-+]?[0-9]+))?\Z", t)
    ip, fp, ex = m.group(1), m.group(2), int(m.group(3) or 0)
    if not ip:
        return False
    d = (ip + fp).lstrip(b"0")
    if not d:
        return True
    kept, rest = d[:15], d[15:]
    if rest.strip(b"0"):
        return False
    return -22 <= ex - len(fp) + len(rest) <= 22


def _wrap32(v):
    return (v + 2 ** 31) % 2 ** 32 - 2 ** 31


def vcf_decode_line(value, G, contigs):
    cols = value.split(b"\t")
    # fields
    if G:
        if len(cols) < 9:
            raise VcfError("fields")
    elif len(cols) != 8:
        raise VcfError("fields")
    chrom, pos_t, vid, ref, alt, qual_t, filt, info = cols[:8]
    flags = HAS_GENOTYPES if G else 0
    col_end, x = [], -1
    for c in cols[:8]:
        x += 1 + len(c)
        col_end.append(x)
    # CHROM
    if not chrom:
        raise VcfError("CHROM")
    contig = contigs.index(chrom) if chrom in contigs else -1
    # POS
    pos = parse_int(pos_t)
    if pos is None:
        raise VcfError("POS")
    # ID
    if not vid:
        raise VcfError("ID")
    if vid != b".":
        flags |= HAS_ID
    # REF
    if not ref or any(c not in BASES for c in ref):
        raise VcfError("REF")
    if ref != ref.upper():
        flags |= REF_LOWER
    # ALT
    alts = []
    if alt != b".":
        seen = [ref.upper()]
        for piece in alt.split(b","):
            if not piece:
                raise VcfError("ALT")
            symbolic = (piece.startswith(b"<") and piece.endswith(b">")) or b"[" in piece or b"]" in piece
            if not (symbolic or piece == b"*" or all(c in BASES for c in piece)):
                raise VcfError("ALT")
            if piece.upper() in seen:
                raise VcfError("ALT")
            seen.append(piece.upper())
            if symbolic:
                flags |= SYMBOLIC
            alts.append(piece)
    # QUAL
    qual, qual_host = None, False
    if qual_t != b".":
        if not QUAL_RE.match(qual_t):
            raise VcfError("QUAL")
        qual = float(qual_t)
        qual_host = not qual_fast_path(qual_t)
        flags |= HAS_QUAL
    # FILTER
    if not filt or filt == b"0":
        raise VcfError("FILTER")
    filters = []
    if filt == b".":
        flags |= UNFILTERED
        filters = None
    elif filt == b"PASS":
        flags |= PASS
    else:
        filters = filt.split(b";")
        if b"PASS" in filters:
            raise VcfError("FILTER")
    # INFO
    if not info or b" " in info:
        raise VcfError("INFO")
    end = pos + len(ref) - 1
    n_info = 0
    if info != b".":
        pieces = info.split(b";")
        n_info = len(pieces)
        for p in pieces:
            key, eq, val = p.partition(b"=")
            if key == b"END":
                e = parse_int(val) if eq else None
                if e is None:
                    raise VcfError("INFO")
                end = e
                flags |= INFO_END
                break
    return {"contig": contig, "pos": pos, "end": _wrap32(end), "flags": flags, "qual": qual,
            "qual_host": qual_host, "col_end": col_end, "n_alt": len(alts),
            "n_filter": len(filters) if filters else 0, "n_info": n_info,
            "n_sample_cols": max(0, len(cols) - 9) if G else 0,
            # what a consumer builds from the columns and the site bytes
            "chrom": chrom, "id": None if vid == b"." else vid, "ref": ref, "alts": alts,
            "filters": None if filters is None else set(filters), "info": info}


def decode_text(text):
    """[(line index, fields or None, error class or None)] of every line that does not start with
    '#', in file order."""
    G, contigs = vcf_header(text)
    if text[:3] == b"\xef\xbb\xbf":
        text = text[3:]
    out = []
    for k, v in enumerate(split_lines(text)):
        if v.startswith(b"#"):
            continue
        try:
            out.append((k, vcf_decode_line(v, G, contigs), None))
        except VcfError as e:
            out.append((k, None, e.what))
    return out
