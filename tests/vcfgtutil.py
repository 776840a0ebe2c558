"""The VCF genotype decode in plain Python, written from DESIGN.md section 16 (htsjdk 2.16
AbstractVCFCodec.createGenotypeMap / parseGenotypeAlleles restated), not from
disq_amd/csrc/dq_vcf_gt_core.h: the oracle of the dq_vcf_genotypes tests.
sample_names(text) -> the header's sample names; gt_decode_line(value, S) -> the cells of one data
line that the site decode (vcfutil.py) accepted, or raises GtError(what, sample) with the class of
the first failing check."""
import math
import re
from fractions import Fraction

from textutil import split_lines
import vcfutil as V

HAS_GT, PHASED, HAS_GQ, HAS_DP, FILTERED = 1, 2, 4, 8, 16

GQ_DEVICE_RE = re.compile(rb"[-+]?[0-9]{1,9}(\.[0-9]{0,6})?\Z")
MAX_PLOIDY, MAX_ALLELE = 255, 32767


class GtError(Exception):
    def __init__(self, what, sample=None):
        super().__init__(what)
        self.what, self.sample = what, sample

    def message(self, k):
        """dq_last_error's text for line k."""
        mid = "" if self.sample is None else f"sample {self.sample}: "
        return f"VCF line {k}: {mid}{self.what}"


def sample_names(text):
    """The columns of the first #CHROM line behind the ninth, trailing empty ones dropped (Java
    String.split); [] when the tenth column is empty or missing (vcfutil's G)."""
    if text[:3] == b"\xef\xbb\xbf":
        text = text[3:]
    for line in split_lines(text):
        if not line.startswith(b"#"):
            break
        if line.startswith(b"#CHROM"):
            cols = line.split(b"\t")
            if not (len(cols) >= 10 and cols[9]):
                return []
            names = cols[9:]
            while names and not names[-1]:
                names.pop()
            return names
    return []


def java_round_to_int(x):
    """Java (int) Math.round(double): nearest integer, ties toward +infinity, clamped to int64, the
    low 32 bits."""
    if x != x:
        return 0
    if math.isinf(x):
        r = 2 ** 63 - 1 if x > 0 else -2 ** 63
    else:
        r = math.floor(Fraction(x) + Fraction(1, 2))
        r = max(-2 ** 63, min(2 ** 63 - 1, r))
    return (r + 2 ** 31) % 2 ** 32 - 2 ** 31


def parse_format(fmt):
    """The keys of column 9, or GtError("FORMAT")."""
    if not fmt:
        raise GtError("FORMAT")
    keys = fmt.split(b":")
    if b"GT" in keys[1:]:
        raise GtError("FORMAT")
    for k in (b"GT", b"GQ", b"DP", b"FT"):
        if keys.count(k) > 1:
            raise GtError("FORMAT")
    return keys


def decode_cell(cell, keys, n_alt, s=None):
    vals = cell.split(b":")
    if len(vals) > len(keys):
        raise GtError("cell", s)

    def value(key):
        i = keys.index(key) if key in keys else -1
        return vals[i] if 0 <= i < len(vals) else None

    flags, alleles = 0, []
    if keys[0] == b"GT":
        flags |= HAS_GT
        gt = vals[0]
        if b"|" in gt:
            flags |= PHASED
        for tok in re.split(rb"[/|\\]", gt):
            if not tok:
                continue
            if tok == b".":
                alleles.append(-1)
                continue
            v = V.parse_int(tok)
            if v is None or not 0 <= v <= min(n_alt, MAX_ALLELE):
                raise GtError("GT", s)
            alleles.append(v)
        if len(alleles) > MAX_PLOIDY:
            raise GtError("GT", s)
    gq, gq_host = -1, False
    t = value(b"GQ")
    if t is not None and t not in (b".", b"-1"):
        if not V.QUAL_RE.match(t):
            raise GtError("GQ", s)
        gq = java_round_to_int(float(t))
        gq_host = not GQ_DEVICE_RE.match(t)
        flags |= HAS_GQ
    dp = -1
    t = value(b"DP")
    if t is not None and t != b".":
        dp = V.parse_int(t)
        if dp is None:
            raise GtError("DP", s)
        flags |= HAS_DP
    t = value(b"FT")
    if t is not None and t not in (b".", b"PASS"):
        flags |= FILTERED
    return {"flags": flags, "alleles": alleles, "gq": gq, "dp": dp, "gq_host": gq_host}


def gt_decode_line(value, S):
    """The S cells of a data line the site decode accepted (left to right; cell_off = the offset of
    the cell's first byte in the line), or GtError."""
    cols = value.split(b"\t")
    if len(cols) - 9 != S:
        raise GtError("samples")
    keys = parse_format(cols[8])
    n_alt = 0 if cols[4] == b"." else cols[4].count(b",") + 1
    off = sum(len(c) + 1 for c in cols[:9])
    cells = []
    for s, cell in enumerate(cols[9:]):
        c = decode_cell(cell, keys, n_alt, s)
        c["cell_off"] = off
        off += len(cell) + 1
        cells.append(c)
    return cells


def decode_text(text):
    """(sample names, [(line index, cells or None, GtError or None)]) of every line that does not
    start with '#', in file order; the site decode must accept the lines."""
    names = sample_names(text)
    if text[:3] == b"\xef\xbb\xbf":
        text = text[3:]
    out = []
    for k, v in enumerate(split_lines(text)):
        if v.startswith(b"#"):
            continue
        if not names:
            out.append((k, [], None))
            continue
        try:
            out.append((k, gt_decode_line(v, len(names)), None))
        except GtError as e:
            out.append((k, None, e))
    return names, out
