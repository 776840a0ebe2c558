"""Test helper: the .bai index rules of DESIGN.md "Building the .bai" (htsjdk BAMIndexer /
BinningIndexBuilder as restated there; SAMv1 sections 5.2 and 5.3) in plain Python and zlib, and a
parser of the .bai layout.  The restatement walks the inflated stream itself and shares no code
with the library: dq_write_bai must reproduce its bytes."""
import bisect
import struct
import zlib

PSEUDO_BIN = 37450
MAX_END = 1 << 29


def reg2bin(beg: int, end: int) -> int:
    """SAMv1 section 5.3: the smallest bin that holds [beg, end) (0-based, end exclusive)."""
    end -= 1
    if beg >> 14 == end >> 14:
        return 4681 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return 585 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return 73 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return 9 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return 1 + (beg >> 26)
    return 0


def _blocks(bam: bytes):
    """(file position, inflated offset) of every BGZF block, the inflated stream."""
    pos, uoff, out, p, u = [], [], [], 0, 0
    while p < len(bam):
        cs = struct.unpack_from("<H", bam, p + 16)[0] + 1
        d = zlib.decompress(bam[p + 18:p + cs - 8], -15)
        pos.append(p)
        uoff.append(u)
        out.append(d)
        u += len(d)
        p += cs
    return pos, uoff, b"".join(out)


def records(bam: bytes):
    """n_ref and, per record in file order, (vs, ve, ref_id, pos, flag, ref_len of the CIGAR)."""
    pos, uoff, u = _blocks(bam)
    assert u[:4] == b"BAM\x01"
    p = 8 + struct.unpack_from("<i", u, 4)[0]
    n_ref = struct.unpack_from("<i", u, p)[0]
    p += 4
    for _ in range(n_ref):
        p += 8 + struct.unpack_from("<i", u, p)[0]

    def voffset(x):
        j = bisect.bisect_right(uoff, x) - 1
        return pos[j] << 16 | (x - uoff[j])

    starts, fields = [], []
    while p < len(u):
        bs, ref_id, rpos = struct.unpack_from("<iii", u, p)
        l_read_name = u[p + 12]
        n_cigar, flag = struct.unpack_from("<HH", u, p + 16)
        rl = 0
        if 32 + l_read_name + 4 * n_cigar <= bs:
            for op in struct.unpack_from(f"<{n_cigar}I", u, p + 36 + l_read_name):
                if op & 0xf in (0, 2, 3, 7, 8):   # M D N = X consume the reference
                    rl += op >> 4
        starts.append(p)
        fields.append((ref_id, rpos, flag, rl))
        p += 4 + bs
    # the pointer after the last record, as BlockCompressedInputStream.getFilePointer gives it:
    # a consumed block points to the next block's start, or to the file's end
    fin = len(bam) << 16
    if starts:
        e = p
        j = bisect.bisect_right(uoff, e - 1) - 1
        nxt = uoff[j + 1] if j + 1 < len(uoff) else len(u)
        if e < nxt:
            fin = pos[j] << 16 | (e - uoff[j])
        elif j + 1 < len(pos):
            fin = pos[j + 1] << 16
    vs = [voffset(x) for x in starts]
    out = [(vs[i], vs[i + 1] if i + 1 < len(vs) else fin) + fields[i] for i in range(len(vs))]
    return n_ref, out


def build_bai(bam: bytes) -> bytes:
    n_ref, recs = records(bam)
    refs = [dict(bins={}, linear={}, first=None, last=None, mapped=0, unmapped=0)
            for _ in range(n_ref)]
    n_no_coor, prev, seen_unplaced = 0, None, False
    for i, (vs, ve, ref_id, pos, flag, rl) in enumerate(recs):
        if ref_id < 0 or pos < 0:
            n_no_coor += 1
            seen_unplaced = True
            continue
        if seen_unplaced or (prev is not None and (ref_id, pos) < prev):
            raise ValueError(f"not coordinate sorted: record {i} is out of order")
        prev = (ref_id, pos)
        if ref_id >= n_ref:
            raise ValueError(f"record {i}: reference index beyond the header's references")
        beg = pos
        end = beg + rl if not flag & 4 and rl > 0 else beg + 1
        if end > MAX_END:
            raise ValueError(f"record {i}: alignment end beyond 2^29, the .bai limit")
        r = refs[ref_id]
        chunks = r["bins"].setdefault(reg2bin(beg, end), [])
        if chunks and (chunks[-1][1] >> 16 == vs >> 16 or (chunks[-1][1] >> 16) + 1 == vs >> 16):
            chunks[-1][1] = ve
        else:
            chunks.append([vs, ve])
        for w in range(beg >> 14, ((end - 1) >> 14) + 1):
            r["linear"][w] = min(r["linear"].get(w, vs), vs)
        if r["first"] is None:
            r["first"] = vs
        r["last"] = ve
        if flag & 4:
            r["unmapped"] += 1
        else:
            r["mapped"] += 1
    o = [b"BAI\x01", struct.pack("<i", n_ref)]
    for r in refs:
        any_rec = r["first"] is not None
        o.append(struct.pack("<i", len(r["bins"]) + (1 if any_rec else 0)))
        for b in sorted(r["bins"]):
            o.append(struct.pack("<Ii", b, len(r["bins"][b])))
            o += [struct.pack("<QQ", a, e) for a, e in r["bins"][b]]
        if any_rec:
            o.append(struct.pack("<IiQQQQ", PSEUDO_BIN, 2, r["first"], r["last"], r["mapped"],
                                 r["unmapped"]))
        n_intv = max(r["linear"]) + 1 if r["linear"] else 0
        o.append(struct.pack("<i", n_intv))
        last = 0
        for w in range(n_intv):   # an untouched window takes the previous entry
            last = r["linear"].get(w, last)
            o.append(struct.pack("<Q", last))
    o.append(struct.pack("<Q", n_no_coor))
    return b"".join(o)


def parse_bai(bai: bytes):
    """([{bins: {bin: [(beg, end)]}, meta: ((vs, ve), (n_mapped, n_unmapped)) or None,
    linear: [offsets]} per reference], n_no_coor)."""
    assert bai[:4] == b"BAI\x01"
    n_ref = struct.unpack_from("<i", bai, 4)[0]
    p, refs = 8, []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", bai, p)[0]
        p += 4
        bins, meta = {}, None
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", bai, p)
            p += 8
            ch = [struct.unpack_from("<QQ", bai, p + 16 * k) for k in range(n_chunk)]
            p += 16 * n_chunk
            if b == PSEUDO_BIN:
                assert n_chunk == 2 and meta is None
                meta = (ch[0], ch[1])
            else:
                assert b not in bins and meta is None   # ascending, the pseudo-bin last
                assert not bins or b > max(bins)
                bins[b] = ch
        n_intv = struct.unpack_from("<i", bai, p)[0]
        p += 4
        linear = list(struct.unpack_from(f"<{n_intv}Q", bai, p))
        p += 8 * n_intv
        refs.append(dict(bins=bins, meta=meta, linear=linear))
    n_no_coor = struct.unpack_from("<Q", bai, p)[0]
    assert p + 8 == len(bai)
    return refs, n_no_coor
