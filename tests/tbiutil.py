"""Test helper: the tabix index rules of DESIGN.md "Building the .tbi" (htsjdk TabixIndexCreator /
BinningIndexBuilder / TabixIndex.write as restated there) in plain Python and zlib, and a parser
of the tabix layout.  The restatement walks the inflated stream itself and shares no code with
the library: dq_text_write_tbi must reproduce its bytes."""
import bisect
import re
import struct
import zlib

PSEUDO_BIN = 37450
MAX_END = 1 << 29
VCF_FORMAT = (2, 1, 2, 0, ord("#"), 0)   # flags, sequence / begin / end column, meta, skip
_SIGNED = re.compile(rb"[+-]?[0-9]+\Z")


def reg2bin(beg: int, end: int) -> int:
    """SAMv1 section 5.3: the smallest bin that holds [beg, end) (0-based, end exclusive)."""
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def _blocks(data: bytes):
    """(file position, inflated offset) of every non-empty BGZF block, the position of the first
    block after the last non-empty one (None: the file ends there), the inflated stream."""
    pos, uoff, out, p, u, after = [], [], [], 0, 0, None
    while p < len(data):
        cs = struct.unpack_from("<H", data, p + 16)[0] + 1
        d = zlib.decompress(data[p + 18:p + cs - 8], -15)
        if d:
            pos.append(p)
            uoff.append(u)
            out.append(d)
            u += len(d)
            after = None
        elif after is None:
            after = p
        p += cs
    return pos, uoff, after, b"".join(out)


def lines(u: bytes):
    """(first byte, value start, value end, byte after the terminator) of every line: LF, CR LF or
    a lone CR end a line, a last line without a terminator counts, a BOM on line 0 is not part of
    its value."""
    out, a, i, n = [], 0, 0, len(u)
    while i < n:
        c = u[i]
        if c == 10:
            out.append([a, a, i, i + 1])
        elif c == 13:
            out.append([a, a, i, i + 2 if i + 1 < n and u[i + 1] == 10 else i + 1])
        else:
            i += 1
            continue
        a = i = out[-1][3]
    if a < n:
        out.append([a, a, n, n])
    if out and u[:3] == b"\xef\xbb\xbf" and out[0][2] >= 3:
        out[0][1] = 3
    return out


def vcf_fields(value: bytes, k: int):
    """(CHROM, POS, end) of a data line; ValueError naming line k."""
    f = value.split(b"\t")
    if len(f) < 4 or not f[0] or not f[1].isdigit():
        raise ValueError(f"line {k} is not a VCF record")
    pos = int(f[1])
    end = pos + len(f[3]) - 1
    if len(f) >= 8:
        for kv in f[7].split(b";"):
            if kv.startswith(b"END="):    # the first END key decides, numeric or not
                if _SIGNED.match(kv[4:]):
                    end = int(kv[4:])
                break
    end = max(end, pos)
    if pos < 1 or end > MAX_END:
        raise ValueError(f"line {k}: POS below 1 or end beyond 2^29, the tabix limit")
    return f[0], pos, end


def records(data: bytes):
    """Per data line in file order: (line index, vs, ve, CHROM, POS, end)."""
    bpos, uoff, after, u = _blocks(data)
    fin = (after if after is not None else len(data)) << 16

    def voffset(x):
        if x >= len(u):
            return fin
        j = bisect.bisect_right(uoff, x) - 1
        return bpos[j] << 16 | (x - uoff[j])

    out = []
    for k, (a0, a, z, nx) in enumerate(lines(u)):
        v = u[a:z]
        if not v or v[:1] == b"#":
            continue
        out.append((k, voffset(a0), voffset(nx)) + vcf_fields(v, k))
    return out


def build_tbi(data: bytes) -> bytes:
    names, refs, prev_pos = [], [], 0
    for k, vs, ve, chrom, pos, end in records(data):
        if names and names[-1] == chrom:
            if pos < prev_pos:
                raise ValueError(f"not sorted: line {k}")
        else:
            if chrom in names:
                raise ValueError(f"not sorted: line {k}")
            names.append(chrom)
            refs.append(dict(bins={}, linear={}))
        prev_pos = pos
        r = refs[-1]
        chunks = r["bins"].setdefault(reg2bin(pos - 1, end), [])
        if chunks and (chunks[-1][1] >> 16 == vs >> 16 or (chunks[-1][1] >> 16) + 1 == vs >> 16):
            chunks[-1][1] = ve
        else:
            chunks.append([vs, ve])
        for w in range((pos - 1) >> 14, ((end - 1) >> 14) + 1):
            r["linear"][w] = min(r["linear"].get(w, vs), vs)
    nm = b"".join(n + b"\x00" for n in names)
    o = [b"TBI\x01", struct.pack("<8i", len(names), *VCF_FORMAT, len(nm)), nm]
    for r in refs:
        o.append(struct.pack("<i", len(r["bins"])))
        for b in sorted(r["bins"]):
            o.append(struct.pack("<Ii", b, len(r["bins"][b])))
            o += [struct.pack("<QQ", a, e) for a, e in r["bins"][b]]
        n_intv = max(r["linear"]) + 1 if r["linear"] else 0
        o.append(struct.pack("<i", n_intv))
        last = 0
        for w in range(n_intv):   # an untouched window takes the previous entry
            last = r["linear"].get(w, last)
            o.append(struct.pack("<Q", last))
    return b"".join(o)


def parse_tbi(tbi: bytes):
    """dict(format=(the six format words), names=[bytes], refs=[{bins: {bin: [(beg, end)]},
    pseudo: the chunks of bin 37450 or None, linear: [offsets]}], n_no_coor=int or None) of a
    tabix index, BGZF-compressed or not; htslib's pseudo-bin and trailing count are kept apart."""
    if tbi[:2] == b"\x1f\x8b":
        import gzip
        tbi = gzip.decompress(tbi)
    assert tbi[:4] == b"TBI\x01"
    w = struct.unpack_from("<8i", tbi, 4)
    n_ref, l_nm = w[0], w[7]
    names = tbi[36:36 + l_nm].split(b"\x00")[:-1] if l_nm else []
    assert len(names) == n_ref and sum(len(n) + 1 for n in names) == l_nm
    p, refs = 36 + l_nm, []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", tbi, p)[0]
        p += 4
        bins, pseudo = {}, None
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", tbi, p)
            p += 8
            ch = [struct.unpack_from("<QQ", tbi, p + 16 * k) for k in range(n_chunk)]
            p += 16 * n_chunk
            if b == PSEUDO_BIN:
                assert pseudo is None
                pseudo = ch
            else:
                assert b not in bins
                bins[b] = ch
        n_intv = struct.unpack_from("<i", tbi, p)[0]
        p += 4
        linear = list(struct.unpack_from(f"<{n_intv}Q", tbi, p))
        p += 8 * n_intv
        refs.append(dict(bins=bins, pseudo=pseudo, linear=linear))
    n_no_coor = None
    if p + 8 == len(tbi):
        n_no_coor = struct.unpack_from("<Q", tbi, p)[0]
        p += 8
    assert p == len(tbi)
    return dict(format=w[1:7], names=names, refs=refs, n_no_coor=n_no_coor)
