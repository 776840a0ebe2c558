"""Test helper: BAM headers, records and record layouts built to the byte with `struct` alone, the
kernel thresholds the edge fixtures aim at read from the source text, and the record guesser's
start check restated in plain Python.

No library or oracle code builds these bytes: tests/test_record_edges.py and
tests/test_coord_edges.py place records at chosen offsets of the decompressed stream (a 64 KiB
record-chain segment edge, a BGZF block edge, a staging or hashing threshold) and hand the file to
the library and to the oracle alike."""
import os
import re
import struct
from collections import namedtuple

import baiutil

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "disq_amd", "csrc")
REF_OPS = (0, 2, 3, 7, 8)  # M D N = X consume the reference


# ------------------------------------------------------------------ thresholds from the source
def _src(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def _find(text, pattern, what):
    m = re.search(pattern, text)
    if m is None:
        raise LookupError(f"{what}: /{pattern}/ not found in the source; the kernel changed, "
                          "re-derive the edge fixtures of tests/reccases.py")
    return m


def _product(expr):
    v = 1
    for f in expr.split("*"):
        v *= int(f.strip())
    return v


Consts = namedtuple("Consts", "SEG SEG_OFF_CAP REC_WAVE REC_LANES REC_GROUP REC_STAGE LONG_N "
                              "LONG_PIECE SPEC_N")


def constants():
    """The constants the fixtures are built around, each found by a regex in the source text (a
    missing one raises LookupError), and the two expressions the fixtures restate (the staging rule
    of decode_group_core and the segment start of the chain kernels) checked to be there still."""
    k, h, a = _src("dq_kernels.hip"), _src("dq_internal.h"), _src("dq_api.hip")
    seg = _product(_find(a, r"int64_t SEG = ([0-9* ]+);", "SEG").group(1))
    _find(a, r"if \(SEG <= 65536\) \{", "recorded starts only for 64 KiB segments")
    cap = int(_find(h, r"constexpr int SEG_OFF_CAP = (\d+);", "SEG_OFF_CAP").group(1))
    wave = int(_find(k, r"constexpr int REC_WAVE = (\d+);", "REC_WAVE").group(1))
    lanes = int(_find(k, r"#define DQ_REC_LANES (\d+)", "DQ_REC_LANES").group(1))
    _find(k, r"constexpr int REC_GROUP = REC_WAVE / REC_LANES;", "REC_GROUP")
    stage = int(_find(k, r"constexpr int REC_STAGE = REC_GROUP \* (\d+);", "REC_STAGE").group(1))
    long_n = int(_find(k, r"constexpr int64_t LONG_N = (\d+);", "LONG_N").group(1))
    piece = int(_find(k, r"constexpr int64_t LONG_PIECE = (\d+);", "LONG_PIECE").group(1))
    spec_n = int(_find(k, r"hit = check_record_start<(\d+)>\(", "speculation depth").group(1))
    # the rules the fixtures restate
    _find(k, r"const int64_t base = first & ~\(int64_t\)15;", "staging base")
    _find(k, r"bool staged = len >= 0 && len \+ 32 <= REC_STAGE && end <= ulen;", "staging rule")
    _find(k, r"lng = n > LONG_N;", "long-record rule")
    _find(k, r"const int64_t sb = start_lin \+ s \* seg_bytes;", "segment start")
    group = wave // lanes
    return Consts(seg, cap, wave, lanes, group, group * stage, long_n, piece, spec_n)


def staged_len(first, end):
    """decode_group_core's quantity: a group whose first record starts at `first` and whose bytes
    end at `end` is staged iff staged_len(first, end) <= REC_STAGE."""
    return end - (first & ~15) + 32


# ------------------------------------------------------------------ header and records
def header(refs, text=b""):
    """A BAM header (SAMv1 section 4.2) from (name, length) pairs."""
    o = [b"BAM\x01", struct.pack("<i", len(text)), text, struct.pack("<i", len(refs))]
    for name, length in refs:
        nm = name.encode() + b"\x00"
        o.append(struct.pack("<i", len(nm)) + nm + struct.pack("<i", length))
    return b"".join(o)


def ref_len_of(cigar):
    return sum(n for n, op in cigar if op in REF_OPS)


def record(ref, pos, name_bytes, cigar=(), l_seq=0, flag=0, mapq=0, bin=None, next_ref=-1,
           next_pos=-1, tlen=0, aux=b"", qual=None, seq=None):
    """One BAM record, block_size word included; every field is explicit.  `name_bytes` is written
    verbatim with l_read_name = its length (the caller supplies the NUL, or leaves it out);
    `cigar` is [(length, op code 0..15)]; bin=None computes reg2bin as tests/baiutil.py does
    (reference length of the CIGAR for a mapped record, one base otherwise)."""
    assert len(name_bytes) <= 255 and len(cigar) <= 65535
    if bin is None:
        rl = ref_len_of(cigar)
        end = pos + rl if not flag & 4 and rl > 0 else pos + 1
        bin = baiutil.reg2bin(pos, end) & 0xffff
    if seq is None:
        seq = b"\x11" * ((l_seq + 1) // 2)
    if qual is None:
        qual = b"\x1e" * l_seq
    assert len(seq) == (l_seq + 1) // 2 and len(qual) == l_seq
    cg = struct.pack(f"<{len(cigar)}I", *[(n << 4) | op for n, op in cigar])
    body = struct.pack("<iiBBHHHiiii", ref, pos, len(name_bytes), mapq, bin, len(cigar), flag,
                       l_seq, next_ref, next_pos, tlen) + name_bytes + cg + seq + qual + aux
    return struct.pack("<i", len(body)) + body


MIN_FILLER = 44  # a one-base read named "a": the smallest record the guesser accepts


def filler(total, ref=0, pos=0, flag=0):
    """A mapped record (<l_seq>M) of exactly `total` bytes, any total >= 44: the name takes 1 to 3
    letters so that every size is reached (l_seq + ceil(l_seq / 2) skips every third)."""
    if total < MIN_FILLER:
        raise ValueError(f"no record of {total} bytes: the smallest is {MIN_FILLER}")
    for ln in (2, 3, 4):
        body = total - 36 - ln - 4  # seq + qual bytes
        l_seq = (2 * body + 1) // 3
        if l_seq >= 1 and l_seq + (l_seq + 1) // 2 == body:
            r = record(ref, pos, b"abc"[:ln - 1] + b"\x00", [(l_seq, 0)], l_seq, flag=flag, mapq=60)
            assert len(r) == total
            return r
    raise AssertionError(total)


def filler_size(l_seq):
    return 36 + 2 + 4 + (l_seq + 1) // 2 + l_seq


At = namedtuple("At", "offset rec fill_l_seq", defaults=(100,))
Layout = namedtuple("Layout", "stream offsets records index")


def layout(hdr, items):
    """The decompressed stream of `hdr` followed by `items`: each a record's bytes (placed next),
    or At(X, record[, fill_l_seq]): the record must start at absolute stream offset X, and the gap
    before it is filled with filler records of fill_l_seq bases, the last one sized to end at X.
    Returns Layout(stream, offset of every record, every record's bytes, index[i] = the record
    number of items[i]).  Raises ValueError when a gap cannot be filled exactly."""
    out, offsets, records, index = [hdr], [], [], []
    p = len(hdr)

    def put(r):
        nonlocal p
        offsets.append(p)
        records.append(r)
        out.append(r)
        p += len(r)

    for it in items:
        if isinstance(it, At):
            gap = it.offset - p
            if gap < 0 or 0 < gap < MIN_FILLER:
                raise ValueError(f"cannot fill {gap} bytes before offset {it.offset}")
            d = filler_size(it.fill_l_seq)
            while gap >= d + MIN_FILLER:
                put(filler(d))
                gap -= d
            if gap:
                put(filler(gap))
            it = it.rec
        index.append(len(records))
        put(it)
    return Layout(b"".join(out), offsets, records, index)


def header_info(hdr):
    """(n_ref, [reference lengths]) of a header's bytes."""
    p = 8 + struct.unpack_from("<i", hdr, 4)[0]
    n_ref = struct.unpack_from("<i", hdr, p)[0]
    p += 4
    lens = []
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", hdr, p)[0]
        lens.append(struct.unpack_from("<i", hdr, p + 4 + ln)[0])
        p += 8 + ln
    assert p == len(hdr)
    return n_ref, lens


# ------------------------------------------------------------------ the guesser, restated
def _i32(x):
    x &= 0xffffffff
    return x - (1 << 32) if x >> 31 else x


_EOF = object()


def _check_internal(u, n_ref, ref_len, v):
    """checkRecordStartInternal at stream offset v by the rules of oracle/disq_oracle.c
    check_internal: the next start, None (no start) or _EOF (a read past the stream's end)."""
    if v + 36 > len(u):
        return _EOF
    remaining, rid, pos = struct.unpack_from("<iii", u, v)
    if rid < -1 or rid >= n_ref or pos < -1:
        return None
    if rid >= 0 and pos > ref_len[rid]:
        return None
    nid, npos = struct.unpack_from("<ii", u, v + 24)
    if nid < -1 or nid >= n_ref or npos < -1:
        return None
    if nid >= 0 and npos > ref_len[nid]:
        return None
    name_len = u[v + 12]
    if name_len < 2:
        return None
    n_cig, flags = struct.unpack_from("<HH", u, v + 16)
    l_seq = struct.unpack_from("<i", u, v + 20)[0]
    half = _i32(l_seq + 1)
    half = -((-half) // 2) if half < 0 else half // 2  # Java int division truncates
    seq_len = _i32(l_seq + half)
    if not flags & 4 and (seq_len == 0 or n_cig == 0):
        return None
    p = v + 36
    if p + name_len > len(u):
        return _EOF
    if u[p + name_len - 1] != 0:
        return None
    for c in u[p:p + name_len - 1]:
        if not (0x21 <= c <= 0x3f or 0x41 <= c <= 0x7e):
            return None
    p += name_len
    for _ in range(n_cig):
        if p + 4 > len(u):
            return _EOF
        op = struct.unpack_from("<i", u, p)[0]
        if op == -1:
            return _EOF
        if op & 0xf > 8:
            return None
        p += 4
    zero_min = _i32(_i32(_i32(32 + name_len) + 4 * n_cig) + seq_len)
    if remaining < zero_min:
        return None
    skip = _i32(4 + remaining)
    if skip > 0:
        if v + skip > len(u):
            return _EOF
        return v + skip
    return v


def spec_check(stream, hinfo, x, n=3):
    """checkRecordStart at stream offset x with n chained records (Disq: 10; the record chain's
    speculation: Consts.SPEC_N): True when n records chain, or at least one does and the next read
    runs past the end of the stream."""
    n_ref, ref_len = hinfo
    v = x
    for k in range(n):
        r = _check_internal(stream, n_ref, ref_len, v)
        if r is _EOF:
            return k > 0
        if r is None:
            return False
        v = r
    return True
