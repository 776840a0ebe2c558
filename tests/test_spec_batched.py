"""The record chain's speculation (seg_spec_split_kernel: candidates found on the staged windows
first, then one chained check for the wave's four sub-segments) on records placed to the byte
(tests/reccases.py).

Every file is a chain of 64 KiB segments from the header's end.  A segment's case is where its
first record starts (an offset from the segment start, which the header length makes the start of a
512-byte window, or leaves 9 bytes into one) and which decoys lie before it: bytes inside the
preceding record's qualities that pass the header prefilter and fail the chained check.

  starts   window offsets 0, 15, 16, 495, 496, 511, 512, 513; the second and the third window; a
           segment in which no record starts (one record longer than 64 KiB)
  decoys   one before the true start; 17 in a row, 32 bytes apart (more than the 16 lanes of a
           sub-segment hold, and into the second window); in all four sub-segments of one wave
           (segments 4 to 7) at different offsets; one 8 bytes before the true start, in the
           same 16-position step (two candidates in one sub-segment's share of the ballot)
  counts   1, 3, 4, 5 and 9 segments; a last segment cut by the end of the data

The CPU tests prove from the laid-out bytes that each case is reached and that the speculated
start of every segment is the chain's, so the GPU run must report no broken link; the GPU tests
hold record count, record starts and per-record hashes to the oracle.  Under the bounds-checked
library the same runs compare every segment's start with seg_spec_kernel<64>'s."""
import bisect
import functools
import struct
from collections import namedtuple

import pytest

from oracle import oracle as O

import bamutil as B
import reccases as R

K = R.constants()
REFS = [("chr1", 100_000_000)]
HDR_ALIGNED = R.header(REFS, text=b"@CO\tab\n")  # 32 bytes: segments start on a window's first byte
HDR_PLAIN = R.header(REFS)                       # 25 bytes: segments start 9 bytes into a window
# three references and a length of 64: a header that straddles a record start can pass (below)
HDR_THREE = R.header([("chr1", 100_000_000), ("chr2", 100_000_000), ("chr3", 100_000_000)],
                     text=b"@CO\tpadpadpa\n")
WIN = 512

# decoys: pass the prefilter, fail the chained check
DECOY_NAME = R.record(0, 7, b"a b\x00", [(10, 0)], 10)  # a space in the name: the first record fails
DECOY_NEXT = R.filler(60)                               # a whole record; qualities follow: the second fails
# 32 bytes that read as a record header at every 32nd byte of their repetition: the next copy's
# block size is this one's tlen, its reference id this one's 2-byte name (a NUL where a letter must be)
DENSE = struct.pack("<iiiIIiii", 40, 0, 0, 2, 1, 1, -1, -1)
# a header 8 bytes before a record start: these two words (block size, reference 0), then the
# record's own block size as the position, its reference id 2 as the name length, its position 1 as
# one CIGAR op, its op count 1 as the mate's reference and a NUL from its mate position 0
STRADDLE = struct.pack("<ii", 0x7fffffff, 0)
STRADDLED = R.record(2, 1, b"t\x00", [(10, 0)], 10, next_pos=0, bin=4681)

# first: the first start's offset in the segment (None: no start); after: records behind it;
# rec: the record that starts there (None: a filler)
Case = namedtuple("Case", "first decoys after rec", defaults=((), 3, None))


def spanning(x0, x1, patches):
    """A record over stream bytes [x0, x1) whose qualities hold `patches` (offset, bytes)."""
    total = x1 - x0
    for ln in (2, 3, 4):
        body = total - 36 - ln - 4
        l_seq = (2 * body + 1) // 3
        if l_seq >= 1 and l_seq + (l_seq + 1) // 2 == body:
            q0 = x0 + 36 + ln + 4 + (l_seq + 1) // 2
            qual = bytearray(b"\x1e" * l_seq)
            for at, bs in patches:
                assert q0 <= at and at + len(bs) <= x1, (x0, x1, at)
                qual[at - q0:at - q0 + len(bs)] = bs
            r = R.record(0, 5, b"spn"[:ln - 1] + b"\x00", [(l_seq, 0)], l_seq, mapq=60, qual=bytes(qual))
            assert len(r) == total
            return r
    raise AssertionError(total)


@functools.lru_cache(maxsize=None)
def build(name):
    """(bam, layout, header, [(segment, true first start or None, decoy offsets)])."""
    hdr, cases, tail = FILES[name]
    h = len(hdr)
    edge = lambda s: h + s * K.SEG  # noqa: E731
    items, want, lead_seg = [R.filler(198)] * 12, [], None
    for s, c in enumerate(cases, 1):
        dec = [(edge(s) + o, bs) for o, bs in c.decoys]
        if c.first is None:  # the spanning record of the next case starts before this segment
            assert not dec
            lead_seg = lead_seg or s
            want.append((s, None, ()))
            continue
        a = lead_seg or s
        lead = c.first // 2 + 120 + (K.SEG * (s - a)) // 2  # the qualities begin before segment s
        items.append(R.At(edge(a) - lead, spanning(edge(a) - lead, edge(s) + c.first, dec)))
        items += ([c.rec] if c.rec else []) + [R.filler(198)] * c.after
        want.append((s, edge(s) + c.first, tuple(o for o, _ in dec)))
        lead_seg = None
    items += tail
    lay = R.layout(hdr, items)
    return B.bgzf(lay.stream, 1), lay, hdr, want


FILES = {
    "seg1": (HDR_ALIGNED, [], [R.filler(198)] * 8),
    "seg3": (HDR_PLAIN, [Case(WIN - 9 - 1), Case(WIN - 9)], []),  # a window's last and first position
    "seg4": (HDR_ALIGNED, [Case(200, ((50, DECOY_NAME),)), Case(700), Case(2 * WIN + 6)], []),
    "seg5": (HDR_ALIGNED, [Case(511), Case(512), Case(None), Case(513)], [R.filler(198)] * 40),
    "seg9": (HDR_ALIGNED,
             [Case(0), Case(15), Case(16),
              Case(495, ((5, DECOY_NAME),)), Case(496, ((100, DECOY_NEXT),)),
              Case(700, ((20, DENSE * 18),)),  # the last copy's name is not one: 17 candidates
              Case(1100, ((300, DECOY_NAME), (600, DECOY_NEXT))),
              Case(511, (), 2)],  # the last segment: two records, then the data ends
             []),
    # a decoy and the true start in one step (positions 32 and 40 of the segment)
    "step": (HDR_THREE, [Case(40, ((32, STRADDLE),), 3, STRADDLED)], []),
}
NSEG = {"seg1": 1, "seg3": 3, "seg4": 4, "seg5": 5, "seg9": 9, "step": 2}


def prefilter(u, hinfo, v):
    """spec_prefilter's header conditions at stream offset v (all of the header staged)."""
    n_ref, ref_len = hinfo
    if v + 36 > len(u):
        return False
    rem, rid, pos = struct.unpack_from("<iii", u, v)
    nid, npos = struct.unpack_from("<ii", u, v + 24)
    for i, p in ((rid, pos), (nid, npos)):
        if i < -1 or i >= n_ref or p < -1 or (i >= 0 and p > ref_len[i]):
            return False
    name_len = u[v + 12]
    n_cig, flags = struct.unpack_from("<HH", u, v + 16)
    l_seq = struct.unpack_from("<i", u, v + 20)[0]
    half = R._i32(l_seq + 1)
    half = -((-half) // 2) if half < 0 else half // 2
    seq_len = R._i32(l_seq + half)
    if name_len < 2 or (not flags & 4 and (seq_len == 0 or n_cig == 0)):
        return False
    if v + 36 + name_len > len(u) or u[v + 36 + name_len - 1] != 0:
        return False
    return rem >= R._i32(R._i32(R._i32(32 + name_len) + 4 * n_cig) + seq_len)


@pytest.mark.parametrize("name", sorted(FILES))
def test_layout_reaches_the_cases(name):
    bam, lay, hdr, want = build(name)
    h, hinfo, end = len(hdr), R.header_info(hdr), len(lay.stream)
    assert len(lay.stream) < 1 << 20
    assert (end - h + K.SEG - 1) // K.SEG == NSEG[name] and len(want) == NSEG[name] - 1
    assert (h % 16 == 0) == (hdr is not HDR_PLAIN)
    # the first ten records are short: the chain's segments are 64 KiB
    assert 16 * (lay.offsets[10] - lay.offsets[0]) // 10 <= K.SEG
    for s, first, decoys in want:
        sb, se = h + s * K.SEG, min(end, h + (s + 1) * K.SEG)
        i = bisect.bisect_left(lay.offsets, sb)
        true = lay.offsets[i] if i < len(lay.offsets) and lay.offsets[i] < se else None
        assert true == first, s
        # what the kernel must find: the first position at which SPEC_N records chain
        stop = se if first is None else first + 1
        hits = [x for x in range(sb, stop) if prefilter(lay.stream, hinfo, x)]
        spec = next((x for x in hits if R.spec_check(lay.stream, hinfo, x, K.SPEC_N)), None)
        assert spec == first, s
        assert set(decoys) <= set(hits) and len(hits) >= len(decoys) + (first is not None), s
    # the oracle reads exactly the laid-out records
    recs = O.OracleBam(bam).read_all()
    assert len(recs) == len(lay.records)
    assert recs["hash"].tolist() == [O.record_hash(r) for r in lay.records]


def test_the_cases_are_the_ones_asked_for():
    firsts = {c.first for hdr, cases, _ in FILES.values() if hdr is HDR_ALIGNED for c in cases}
    assert {0, 15, 16, 495, 496, 511, 512, 513} <= firsts
    assert any(WIN <= f < 2 * WIN for f in firsts - {None}) and any(2 * WIN <= f < 3 * WIN for f in firsts - {None})
    assert None in firsts
    # the dense decoys: 17 candidates in a row, the last ones in the segment's second window
    bam, lay, hdr, want = build("seg9")
    s, first, decoys = want[5]
    at = len(hdr) + s * K.SEG + 20
    hinfo = R.header_info(hdr)
    dense = [x for x in range(at, at + 32 * 18) if prefilter(lay.stream, hinfo, x)]
    assert dense == [at + 32 * i for i in range(17)] and dense[-1] - (at - 20) >= WIN
    assert not any(R.spec_check(lay.stream, hinfo, x, 1) for x in dense)
    # one decoy fails at its own record, the other at the record after it
    for s, o, n in ((4, 5, False), (5, 100, True)):
        x = len(hdr) + s * K.SEG + o
        assert R.spec_check(lay.stream, hinfo, x, 1) == n and not R.spec_check(lay.stream, hinfo, x, 2)
    # segments 4 to 7 are one wave's four sub-segments, their decoys at different offsets
    assert [want[s - 1][2][0] - (len(hdr) + s * K.SEG) for s in (4, 5, 6, 7)] == [5, 100, 20, 300]
    # the last segment is cut by the end of the data: the chained check runs off the stream
    last = want[-1][1]
    assert len(lay.stream) - last == 2 * 198 and len(lay.stream) < len(hdr) + 9 * K.SEG
    assert R.spec_check(lay.stream, hinfo, last, K.SPEC_N) and not prefilter(lay.stream, hinfo, last + 2 * 198)


def test_two_candidates_in_one_step():
    bam, lay, hdr, want = build("step")
    hinfo, sb = R.header_info(hdr), len(hdr) + K.SEG
    (s, first, decoys), = want
    hits = [x for x in range(sb, first + 1) if prefilter(lay.stream, hinfo, x)]
    assert hits == [sb + 32, sb + 40] and first == sb + 40 and sb % 16 == 0
    assert (hits[0] - sb) // 16 == (hits[1] - sb) // 16  # one step of a sub-segment's 16 lanes
    assert not R.spec_check(lay.stream, hinfo, hits[0], 1) and R.spec_check(lay.stream, hinfo, first, K.SPEC_N)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(FILES))
def test_gpu_speculated_starts(tmp_path, name):
    from test_record_edges import child_segs, parity
    bam, lay, hdr, want = build(name)
    b = parity(bam, 0)  # record count, starts, fields and hashes against the oracle
    assert len(b["voffset"]) == len(lay.records)
    # every speculated start was the chain's: no link broke, nothing was repaired
    assert child_segs(tmp_path, bam) == (NSEG[name], 0, len(lay.records))
    parity(bam, max(200, len(bam) // 3 + 1))  # and with splits that start inside the file
