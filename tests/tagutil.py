"""Test oracle of the BAM aux tag decode (dq_tags), in plain Python from SAMv1
section 4.2.4: one record's bytes and the requested keys in, the cells or the exact error out.
Nothing here shares code with disq_amd/csrc/dq_tags_core.h."""
import re
import struct

import numpy as np

ANY, INT, FLOAT, CHAR, STRING = 0, 1, 2, 3, 4
PRESENT, REPEATED = 1, 4
INT_TYPES = {b"c": "<b", b"C": "<B", b"s": "<h", b"S": "<H", b"i": "<i", b"I": "<I"}
ELEM_SIZE = {b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}
HEX = set(b"0123456789abcdefABCDEF")
ID_RE = re.compile(rb"[A-Za-z][A-Za-z0-9]\Z")


class TagError(Exception):
    """what: 'fields', 'tag XX' (XX missing when fewer than three bytes are left), 'tag XX type'."""

    def __init__(self, what):
        super().__init__(what)
        self.what = what


def norm_keys(keys):
    """[(id bytes, class)] of ids (str or bytes) or (id, class) pairs."""
    out = []
    for k in keys:
        vid, ty = (k, ANY) if isinstance(k, (str, bytes)) else k
        out.append((vid.encode() if isinstance(vid, str) else bytes(vid), int(ty)))
    return out


def keys_refused(keys):
    """Why dq_tags answers DQ_EINVAL to this key list, or None."""
    ks = norm_keys(keys)
    if not 1 <= len(ks) <= 64:
        return "count"
    seen = set()
    for vid, ty in ks:
        if not ID_RE.match(vid):
            return "id"
        if ty not in (ANY, INT, FLOAT, CHAR, STRING):
            return "type"
        if vid in seen:
            return "twice"
        seen.add(vid)
    return None


def aux_region(rec):
    """(start, end) of the aux bytes of a record (block_size word included), or TagError('fields')."""
    if len(rec) < 36:
        raise TagError("fields")
    bs = struct.unpack_from("<i", rec, 0)[0]
    if bs < 32 or 4 + bs > len(rec):
        raise TagError("fields")
    l_rn = rec[12]
    n_cig = struct.unpack_from("<H", rec, 16)[0]
    l_seq = struct.unpack_from("<i", rec, 20)[0]
    if l_seq < 0:
        raise TagError("fields")
    start = 36 + l_rn + 4 * n_cig + (l_seq + 1) // 2 + l_seq
    if start > 4 + bs:
        raise TagError("fields")
    return start, 4 + bs


def iter_tags(rec):
    """(id, type byte, subtype byte or b'', payload offset, payload length) of every tag of the
    record in stored order; TagError at the first tag that is not well formed, after the tags in
    front of it."""
    p, end = aux_region(rec)
    while p < end:
        if end - p < 3:
            raise TagError("tag ")
        vid, ty = rec[p:p + 2], rec[p + 2:p + 3]
        bad = TagError("tag " + vid.decode("latin-1"))
        p += 3
        if ty in (b"Z", b"H"):
            z = rec.find(b"\x00", p, end)
            if z < 0:
                raise bad
            if ty == b"H" and ((z - p) % 2 or not set(rec[p:z]) <= HEX):
                raise bad
            yield vid, ty, b"", p, z - p
            p = z + 1
        elif ty == b"B":
            if end - p < 5:
                raise bad
            sub = rec[p:p + 1]
            cnt = struct.unpack_from("<i", rec, p + 1)[0]
            p += 5
            if sub not in ELEM_SIZE or cnt < 0 or ELEM_SIZE[sub] * cnt > end - p:
                raise bad
            yield vid, ty, sub, p, ELEM_SIZE[sub] * cnt
            p += ELEM_SIZE[sub] * cnt
        else:
            n = 1 if ty == b"A" else 4 if ty == b"f" else ELEM_SIZE[ty] if ty in INT_TYPES else 0
            if n == 0 or end - p < n:
                raise bad
            yield vid, ty, b"", p, n
            p += n


def walk(rec):
    return list(iter_tags(rec))


def class_ok(want, ty):
    return (want == ANY or (want == INT and ty in INT_TYPES) or (want == FLOAT and ty == b"f") or
            (want == CHAR and ty == b"A") or (want == STRING and ty == b"Z"))


def value_of(want, ty, rec, at):
    """The 32 bits of a cell's value."""
    if want == INT:
        return struct.unpack_from(INT_TYPES[ty], rec, at)[0] & 0xffffffff
    if want == FLOAT:
        return struct.unpack_from("<I", rec, at)[0]
    if want == CHAR:
        return rec[at]
    return 0


BLANK = {"flags": 0, "vtype": 0, "subtype": 0, "val_off": -1, "val_len": 0, "val": 0}


def decode_record(rec, keys):
    """The cells of one record, one dict per key; TagError(first failing check in stored order): a
    class mismatch in front of a bad tag wins, one behind it is never seen."""
    ks = norm_keys(keys)
    index = {vid: q for q, (vid, _) in enumerate(ks)}
    cells = [dict(BLANK) for _ in ks]
    for vid, ty, sub, at, n in iter_tags(rec):
        q = index.get(vid)
        if q is None:
            continue
        c = cells[q]
        if c["flags"] & PRESENT:
            c["flags"] |= REPEATED
            continue
        if not class_ok(ks[q][1], ty):
            raise TagError("tag " + vid.decode("latin-1") + " type")
        c.update(flags=PRESENT, vtype=ty[0], subtype=sub[0] if sub else 0, val_off=at, val_len=n,
                 val=value_of(ks[q][1], ty, rec, at))
    return cells


def decode_records(recs, keys):
    """([cells or None per record], (row, what) of the lowest failing row or None)."""
    out, first = [], None
    for k, r in enumerate(recs):
        try:
            out.append(decode_record(r, keys))
        except TagError as e:
            out.append(None)
            if first is None:
                first = (k, e.what)
    return out, first


def want_arrays(rows, keys):
    """The arrays of Context.tags for rows of cells (no failing row): flags, vtype, subtype,
    val_off, val_len shaped (K, n), key_type, key_base, val."""
    ks = norm_keys(keys)
    K, n = len(ks), len(rows)
    g = {"flags": np.zeros((K, n), np.uint8), "vtype": np.zeros((K, n), np.uint8),
         "subtype": np.zeros((K, n), np.uint8), "val_off": np.full((K, n), -1, np.int32),
         "val_len": np.zeros((K, n), np.int32), "key_type": np.array([t for _, t in ks], np.int32)}
    base, nval = [], 0
    for _, t in ks:
        has = t in (INT, FLOAT, CHAR)
        base.append(nval if has else -1)
        nval += n if has else 0
    g["key_base"] = np.array(base, np.int64)
    val = np.zeros(nval, np.uint32)
    for k, cells in enumerate(rows):
        for q, c in enumerate(cells):
            for f in ("flags", "vtype", "subtype", "val_off", "val_len"):
                g[f][q, k] = c[f]
            if base[q] >= 0:
                val[base[q] + k] = c["val"]
    g["val"] = val
    return g


def split_records(raw):
    """The records of back-to-back raw bytes (block_size chain)."""
    out, p = [], 0
    while p < len(raw):
        bs = struct.unpack_from("<i", raw, p)[0]
        out.append(bytes(raw[p:p + 4 + bs]))
        p += 4 + bs
    return out
