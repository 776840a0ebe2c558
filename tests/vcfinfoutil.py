"""The VCF INFO decode in plain Python, written from DESIGN.md section 17 (htsjdk 2.16
AbstractVCFCodec.parseInfo restated for a list of requested keys), not from
disq_amd/csrc/dq_vcf_info_core.h: the oracle of the dq_vcf_info tests.
info_header(text) -> {id: type}; resolve_keys(keys, header) -> [(id, type, header says Flag)];
info_decode_line(value, rkeys) -> one cell per key, or raises InfoError(q) with the lowest failing
key index; want_arrays(rows, rkeys) -> the arrays of dq_info_batch."""
import struct

import numpy as np

from textutil import split_lines
from vcfutil import QUAL_RE, parse_int, qual_fast_path

AUTO, FLAG, INTEGER, FLOAT, STRING = 0, 1, 2, 3, 4
PRESENT, HAS_VALUE, REPEATED = 1, 2, 4
I_MISSING = -2 ** 31
F_MISSING_BITS = 0x7ff8000000000001        # a quiet NaN with payload 1
F_NAN_BITS = 0x7ff8000000000000            # Java's Double.NaN
TYPES = {b"Flag": FLAG, b"Integer": INTEGER, b"Float": FLOAT, b"String": STRING, b"Character": STRING}
MAX_KEYS = 64


class InfoError(Exception):
    def __init__(self, q):
        super().__init__(q)
        self.q = q


def info_header(text):
    """{id: type} of the ##INFO=<...> lines: the first ','-pieces starting with ID= and Type=
    between '<' and the last '>' (quoted commas are not honoured); a repeated ID keeps its first
    line; an unknown Type is STRING."""
    if text[:3] == b"\xef\xbb\xbf":
        text = text[3:]
    out = {}
    for line in split_lines(text):
        if not line.startswith(b"#"):
            break
        if not line.startswith(b"##INFO=<"):
            continue
        end = line.rfind(b">")
        body = line[8:end] if end >= 8 else line[8:]
        vid = ty = None
        for piece in body.split(b","):
            if vid is None and piece.startswith(b"ID="):
                vid = piece[3:]
            if ty is None and piece.startswith(b"Type="):
                ty = piece[5:]
        if vid is not None and vid not in out:
            out[vid] = TYPES.get(ty, STRING)
    return out


def resolve_keys(keys, header):
    """keys: ids or (id, type) pairs.  [(id, conversion type, the header types it as Flag)];
    ValueError for a list dq_vcf_info refuses."""
    if not 1 <= len(keys) <= MAX_KEYS:
        raise ValueError("count")
    out = []
    for k in keys:
        vid, ty = (k, AUTO) if isinstance(k, (bytes, str)) else k
        vid = vid.encode() if isinstance(vid, str) else vid
        if not vid or any(c in vid for c in b";=,\t ") or vid in [o[0] for o in out]:
            raise ValueError("id")
        if ty not in (AUTO, FLAG, INTEGER, FLOAT, STRING):
            raise ValueError("type")
        ht = header.get(vid, 0)
        out.append((vid, ty if ty != AUTO else (ht or STRING), ht == FLAG))
    return out


def float_element(t):
    """(bits, left to the host's strtod) of one Float element, or None when it is refused."""
    if t == b".":
        return F_MISSING_BITS, False
    if t == b"NaN":
        return F_NAN_BITS, False
    if t in (b"Infinity", b"+Infinity", b"-Infinity"):
        return struct.unpack("<Q", struct.pack("<d", float(t.decode())))[0], False
    if not QUAL_RE.match(t):
        return None
    return struct.unpack("<Q", struct.pack("<d", float(t)))[0], not qual_fast_path(t)


def decode_value(text, ty):
    """(n_values, values, host count) of a value text that is neither empty nor '.', or None."""
    pieces = text.split(b",")
    if ty == INTEGER:
        vals = [I_MISSING if p == b"." else parse_int(p) for p in pieces]
        return None if None in vals else (len(pieces), vals, 0)
    if ty == FLOAT:
        el = [float_element(p) for p in pieces]
        return None if None in el else (len(pieces), [b for b, _ in el], sum(h for _, h in el))
    return len(pieces), [], 0


def blank():
    return {"flags": 0, "n_values": 0, "val_off": -1, "val_len": 0, "values": [], "host": 0}


def info_decode_line(value, rkeys):
    """The cells of a data line the site decode accepted, one per requested key."""
    cols = value.split(b"\t")
    info = cols[7]
    at = sum(len(c) + 1 for c in cols[:7])
    ids = [k[0] for k in rkeys]
    cells = [blank() for _ in rkeys]
    seen, bad = set(), []
    if info != b".":
        for piece in info.split(b";"):
            key, eq, val = piece.partition(b"=")
            if key in ids:
                q = ids.index(key)
                _, ty, hflag = rkeys[q]
                c = cells[q]
                if q in seen:
                    c["flags"] |= REPEATED          # the first piece is the decoded one
                elif not eq:
                    c["flags"] = PRESENT
                elif hflag and val == b"0":
                    pass                             # htsjdk leaves "DB=0" out of the map
                else:
                    c["flags"], c["val_off"], c["val_len"] = PRESENT, at + len(key) + 1, len(val)
                    if val not in (b"", b"."):
                        d = decode_value(val, ty)
                        if d is None:
                            bad.append(q)
                            cells[q] = blank()
                        else:
                            c["flags"] |= HAS_VALUE
                            c["n_values"], c["values"], c["host"] = d
                seen.add(q)
            at += len(piece) + 1
    if bad:
        raise InfoError(min(bad))
    return cells


def decode_text(text, keys):
    """(resolved keys, [(line index, cells or None, failing key index or None)]) of every line
    that does not start with '#', in file order; the site decode must accept the lines."""
    rkeys = resolve_keys(keys, info_header(text))
    if text[:3] == b"\xef\xbb\xbf":
        text = text[3:]
    out = []
    for k, v in enumerate(split_lines(text)):
        if v.startswith(b"#"):
            continue
        try:
            out.append((k, info_decode_line(v, rkeys), None))
        except InfoError as e:
            out.append((k, None, e.q))
    return rkeys, out


def want_arrays(rows, rkeys):
    """The oracle's cells of the variants (rows[k][q]) as the arrays of dq_info_batch; fval as its
    bits."""
    n, K = len(rows), len(rkeys)
    w = {"flags": np.zeros((K, n), np.uint8), "n_values": np.zeros((K, n), np.int32),
         "val_off": np.full((K, n), -1, np.int32), "val_len": np.zeros((K, n), np.int32)}
    width = [max([1] + [r[q]["n_values"] for r in rows]) for q in range(K)]
    base, ni, nf = [], 0, 0
    for q, (_, ty, _) in enumerate(rkeys):
        if ty == INTEGER:
            base.append(ni)
            ni += n * width[q]
        elif ty == FLOAT:
            base.append(nf)
            nf += n * width[q]
        else:
            base.append(-1)
    ival, fval = np.full(ni, I_MISSING, np.int32), np.full(nf, F_MISSING_BITS, np.uint64)
    for k, r in enumerate(rows):
        for q, c in enumerate(r):
            for f in w:
                w[f][q, k] = c[f]
            dst = ival if rkeys[q][1] == INTEGER else fval
            for j, v in enumerate(c["values"]):
                dst[base[q] + k * width[q] + j] = v
    w.update(ival=ival, fval=fval, key_type=np.array([k[1] for k in rkeys], np.int32),
             key_width=np.array(width, np.int32), key_base=np.array(base, np.int64))
    return w, sum(c["host"] for r in rows for c in r)
