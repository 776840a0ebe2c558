"""The record chain (seg_*), the record decode and the record hashes on records placed to the byte
(tests/reccases.py): every fixture aims at one edge of those kernels, a CPU test proves from the
laid-out offsets that the edge is reached (and that the oracle reads exactly the records laid
out), and a GPU test holds the library to the oracle on it, bit for bit.

  A  records starting 0..37 bytes before a 64 KiB chain-segment edge; segments holding exactly
     SEG_OFF_CAP and SEG_OFF_CAP + 1 record starts
  B  the first record of a segment is valid BAM that the guesser rejects (speculation misses)
  C  complete small records inside a long record's qualities, right after a segment edge
     (speculation takes a fake): the link check must find it and the repair re-walk the segment
  D  BGZF block edges at and inside every record's fixed part; 300 blocks inside one 64 KiB page
  E  the staging threshold, the long-record thresholds, every (n mod 8, p mod 4), 1 / 32 / 33 records
  F  field extremes

The constants come from the source text (reccases.constants): a kernel change that moves one
breaks the CPU tests here instead of leaving fixtures that no longer reach their edge."""
import bisect
import functools
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

from disq_amd import _lib
from oracle import oracle as O

import baiutil
import bamutil as B
import reccases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = R.constants()
HDR = R.header([("chr1", 100_000_000)])
HINFO = R.header_info(HDR)
H = len(HDR)
TINY = R.filler(44)
FIELDS = ("block_size", "ref_id", "pos", "l_seq", "next_ref_id", "next_pos", "tlen", "flag", "bin",
          "n_cigar", "mapq", "l_read_name")


def edge(s):
    """Start of chain segment s: the chain starts at the first record (split 0: the header's end)."""
    return H + s * K.SEG


def nseg_of(lay):
    return (len(lay.stream) - H + K.SEG - 1) // K.SEG


def test_constants_are_the_ones_the_fixtures_were_laid_out_for():
    """The layouts below are computed from K, so other values would still aim at the edges; the
    shapes themselves (44-byte records filling a segment, an 8000-base record spanning an edge)
    assume these magnitudes."""
    assert K.SEG == 65536 and K.SEG_OFF_CAP == 512 and K.SPEC_N == 3
    assert (K.REC_GROUP, K.REC_STAGE, K.LONG_N, K.LONG_PIECE) == (32, 12288, 2048, 32768)
    assert K.SEG_OFF_CAP * len(TINY) < K.SEG  # SEG_OFF_CAP + 1 minimal records fit in a segment


def test_a_missing_constant_fails_loudly():
    with pytest.raises(LookupError, match="NO_SUCH"):
        R._find("constexpr int OTHER = 1;", r"constexpr int NO_SUCH = (\d+);", "NO_SUCH")


# ------------------------------------------------------------------ shared proofs
def block_table(bam):
    pos, uoff, u = baiutil._blocks(bam)
    return pos, uoff, u


def voffset_of(bam):
    """x -> the htsjdk start pointer of stream offset x (a block's end is the next block's 0)."""
    pos, uoff, _ = block_table(bam)

    def f(x):
        j = bisect.bisect_right(uoff, x) - 1
        return pos[j] << 16 | (x - uoff[j])
    return f


def assert_oracle_reads_layout(bam, lay):
    """The oracle's sequential reader returns exactly the laid-out records: start pointers, every
    fixed field as the bytes hold it, and the hash of each record's bytes."""
    assert B.inflate_all(bam) == lay.stream
    recs = O.OracleBam(bam).read_all()
    assert len(recs) == len(lay.records)
    v = voffset_of(bam)
    # Disq's split 0 starts at the first record (its 10-record guesser accepts it), so the
    # record chain and its segments start at the header's end
    assert O.OracleBam(bam).plan(0)[0][2][0] == v(H)
    assert recs["voffset"].tolist() == [v(x) for x in lay.offsets]
    head = np.frombuffer(b"".join(r[:36] for r in lay.records), _lib.LEAN_HEAD)
    for f in FIELDS:
        assert np.array_equal(recs[f], head[f]), f
    assert recs["block_size"].tolist() == [len(r) - 4 for r in lay.records]
    assert recs["hash"].tolist() == [O.record_hash(r) for r in lay.records]
    return recs


def first_true_starts(lay):
    """Per chain segment: the first record start inside it, or None."""
    end, out = len(lay.stream), []
    for s in range(nseg_of(lay)):
        i = bisect.bisect_left(lay.offsets, edge(s))
        ok = i < len(lay.offsets) and lay.offsets[i] < min(end, edge(s + 1))
        out.append(lay.offsets[i] if ok else None)
    return out


def speculated_starts(lay):
    """Per chain segment what seg_spec finds: the first position of the segment at which SPEC_N
    records chain (segment 0: the chain's start)."""
    end, out = len(lay.stream), [H]
    for s in range(1, nseg_of(lay)):
        hit = None
        for x in range(edge(s), min(end, edge(s + 1))):
            if R.spec_check(lay.stream, HINFO, x, K.SPEC_N):
                hit = x
                break
        out.append(hit)
    return out


def wrong_speculations(lay):
    """The segments whose speculated start is not the chain's: seg_link reports a broken link
    iff there is one."""
    return [s for s, (a, b) in enumerate(zip(speculated_starts(lay), first_true_starts(lay)))
            if a != b]


CHILD = """
import sys
from disq_amd import _lib
with _lib.Context(split_size=0) as c:
    c.open_bytes(open(sys.argv[1], "rb").read())
    print(len(c.read(with_raw=False)["voffset"]))
"""


def child_segs(tmp_path, bam):
    """(segments, broken link flag, records) of a split-0 read in a fresh process with DQ_DEBUG
    set (the library reads the variable once per process)."""
    p = tmp_path / "f.bam"
    p.write_bytes(bam)
    r = subprocess.run([sys.executable, "-c", CHILD, str(p)], env=dict(os.environ, DQ_DEBUG="1"),
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    m = re.findall(r"\[dq\] segs (\d+) (\d+) ", r.stderr)
    assert len(m) == 1, r.stderr
    return int(m[0][0]), int(m[0][1]), int(r.stdout.strip())


def parity(bam, split=0, **kw):
    from test_gpu_parity import assert_parity
    return assert_parity(bam, split, raw_check=None, **kw)


def some_split(bam, parts):
    return max(200, len(bam) // parts + 1)


# ------------------------------------------------------------------ A: segment edges
EDGE_D = (0, 1, 2, 3, 4, 35, 36, 37)


@functools.lru_cache(maxsize=None)
def family_a():
    items, marks = [], {}
    for s in range(1, 17):  # every d at two segment edges
        d = EDGE_D[(s - 1) % 8]
        marks[s] = (len(items), d)
        items.append(R.At(edge(s) - d, R.record(0, s, b"edge%02d\x00" % s, [(20, 0)], 20, mapq=s)))
    items.append(R.At(edge(17) - 44, TINY))  # one more record that ends exactly on an edge
    marks["ends"] = len(items) - 1
    # segment 18: SEG_OFF_CAP starts (its last record runs 10 bytes into segment 19);
    # segment 19: SEG_OFF_CAP + 1 starts (its last record runs 5 bytes into segment 20)
    items.append(R.At(edge(18), TINY))
    items += [TINY] * (K.SEG_OFF_CAP - 2)
    items.append(R.filler(edge(19) + 10 - (edge(18) + (K.SEG_OFF_CAP - 1) * 44)))
    items += [TINY] * K.SEG_OFF_CAP
    items.append(R.filler(edge(20) + 5 - (edge(19) + 10 + K.SEG_OFF_CAP * 44)))
    items += [R.filler(198)] * 5
    lay = R.layout(HDR, items)
    return B.bgzf(lay.stream, 1), lay, marks


def test_a_layout_reaches_the_segment_edges():
    bam, lay, marks = family_a()
    assert len(bam) < 4 << 20
    seen = {}
    for s in range(1, 17):
        i, d = marks[s]
        x = lay.offsets[lay.index[i]]
        assert x == edge(s) - d  # SEG: a record d bytes before edge s
        seen.setdefault(d, []).append(s)
    assert sorted(seen) == sorted(EDGE_D) and all(len(v) == 2 for v in seen.values())
    # d = 1..3: the block_size word straddles the edge; d = 35: the 36-byte fixed part does
    assert all(len(lay.records[lay.index[marks[s][0]]]) >= 44 for s in range(1, 17))
    i = lay.index[marks["ends"]]
    assert lay.offsets[i] + len(lay.records[i]) == edge(17) == lay.offsets[i + 1]
    starts = [sum(edge(s) <= x < edge(s + 1) for x in lay.offsets) for s in (18, 19)]
    assert starts == [K.SEG_OFF_CAP, K.SEG_OFF_CAP + 1]  # SEG_OFF_CAP: recorded / walked twice
    assert lay.offsets[1 + bisect.bisect_left(lay.offsets, edge(18)) + K.SEG_OFF_CAP - 1] == edge(19) + 10
    # the first ten records are short: the chain's segments stay 64 KiB
    assert 16 * (lay.offsets[10] - lay.offsets[0]) // 10 <= K.SEG
    assert_oracle_reads_layout(bam, lay)
    assert wrong_speculations(lay) == []  # every speculated start is the chain's: no repair


@pytest.mark.gpu
def test_a_gpu_segment_edges(tmp_path):
    bam, lay, _ = family_a()
    for split in (0, some_split(bam, 7)):
        parity(bam, split)
    assert child_segs(tmp_path, bam) == (nseg_of(lay), 0, len(lay.records))


# ------------------------------------------------------------------ B: speculation misses a record
ODD = {
    "n_cigar_0": lambda: R.record(0, 7, b"odd\x00", [], 10),
    "l_read_name_1": lambda: R.record(0, 7, b"\x00", [(10, 0)], 10),
    "space_in_name": lambda: R.record(0, 7, b"a b\x00", [(10, 0)], 10),
    "cigar_op_9": lambda: R.record(0, 7, b"odd\x00", [(4, 0), (2, 9), (4, 0)], 10),
}


@functools.lru_cache(maxsize=None)
def family_b(variant):
    lay = R.layout(HDR, [R.At(edge(1) + 5, ODD[variant]()), R.At(edge(3) + 100, R.filler(198))]
                   + [R.filler(198)] * 3)
    return B.bgzf(lay.stream, 1), lay


@pytest.mark.parametrize("variant", sorted(ODD))
def test_b_layout_is_a_false_negative(variant):
    bam, lay = family_b(variant)
    i = lay.index[0]
    x, nxt = lay.offsets[i], lay.offsets[i + 1]
    assert lay.offsets[i - 1] < edge(1) < x == edge(1) + 5  # SEG: the first record of segment 1
    assert not R.spec_check(lay.stream, HINFO, x, K.SPEC_N)
    assert not R.spec_check(lay.stream, HINFO, x, 1)  # this record itself is rejected
    assert R.spec_check(lay.stream, HINFO, nxt, K.SPEC_N)
    assert speculated_starts(lay)[1] == nxt
    assert wrong_speculations(lay) == [1]
    assert_oracle_reads_layout(bam, lay)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", sorted(ODD))
def test_b_gpu_false_negative(variant):
    bam, _ = family_b(variant)
    for split in (0, some_split(bam, 3)):
        parity(bam, split)


@pytest.mark.gpu
def test_b_gpu_repair_path_observed(tmp_path):
    bam, lay = family_b("cigar_op_9")
    assert child_segs(tmp_path, bam) == (nseg_of(lay), 1, len(lay.records))


# ------------------------------------------------------------------ C: speculation takes a fake
FAKE = R.filler(105)
BIG_L = 8000


@functools.lru_cache(maxsize=None)
def family_c(k, sorted_pos=False):
    """An 8000-base record starting 4344 bytes before segment edge 1; its qualities hold k
    complete 105-byte records from edge + 7 on; it ends 7700 bytes after the edge.  sorted_pos:
    every record's position is its number, so that the file can be indexed."""
    x = edge(1) - 4344
    q0 = edge(1) + 7 - (x + 36 + 4 + 4 + BIG_L // 2)
    qual = b"\x1e" * q0 + FAKE * k
    qual += b"\x1e" * (BIG_L - len(qual))
    items = [R.At(x, R.record(0, 0, b"big\x00", [(BIG_L, 0)], BIG_L, mapq=60, qual=qual)),
             R.At(edge(4) + 100, R.filler(198))]
    lay = R.layout(HDR, items)
    if sorted_pos:
        recs = [r[:8] + struct.pack("<i", i) + r[12:] for i, r in enumerate(lay.records)]
        lay = R.Layout(HDR + b"".join(recs), lay.offsets, recs, lay.index)
    return B.bgzf(lay.stream, 0), lay


@pytest.mark.parametrize("k", [4, 12])
def test_c_layout_is_a_false_positive(k):
    bam, lay = family_c(k)
    i = lay.index[0]
    x, nxt = lay.offsets[i], lay.offsets[i + 1]
    assert x == edge(1) - 4344 and nxt == edge(1) + 7700  # SEG: the record spans edge 1
    fake0 = edge(1) + 7
    assert lay.stream[fake0:fake0 + 105 * k] == FAKE * k
    assert R.spec_check(lay.stream, HINFO, fake0, K.SPEC_N)  # SPEC_N records chain at the fake
    spec = speculated_starts(lay)
    assert spec[1] == fake0 and first_true_starts(lay)[1] == nxt
    assert wrong_speculations(lay) == [1]
    ob, v = O.OracleBam(bam), voffset_of(bam)
    fired = [d for d in range(1500) if ob.check_record_start(v(edge(1) + d))]
    # Disq's 10-record check: never with 4 fakes; with 12, at the three from which 10 chain
    assert fired == ([] if k == 4 else [7, 112, 217])
    assert fired == [d for d in range(1500) if R.spec_check(lay.stream, HINFO, edge(1) + d, 10)]
    assert_oracle_reads_layout(bam, lay)


def far_split(bam, lay):
    """A split size whose only inner split start lies well after the fakes' block."""
    pos, uoff, _ = block_table(bam)
    fake_block_end = pos[bisect.bisect_right(uoff, edge(1) + 7)]
    split = fake_block_end + 20000
    assert split < len(bam) < 2 * split
    return split


@pytest.mark.gpu
@pytest.mark.parametrize("k", [4, 12])
def test_c_gpu_false_positive(k):
    bam, lay = family_c(k)
    for split in (0,) + ((30000, 47000) if k == 4 else (far_split(bam, lay),)):
        parity(bam, split)


@pytest.mark.gpu
def test_c_gpu_repair_path_observed(tmp_path):
    bam, lay = family_c(4)
    assert child_segs(tmp_path, bam) == (nseg_of(lay), 1, len(lay.records))


def c_intervals(lay):
    big = lay.index[0]
    # around the long record's start; a stretch only the long record covers; past every record
    return [(0, big - 20, big + 30), (0, len(lay.records) + 500, len(lay.records) + 900),
            (0, 20000, 30000)]


def test_c_indexed_layout_keeps_the_fake_and_one_window():
    bam, lay = family_c(4, True)
    assert wrong_speculations(lay) == [1]
    assert_oracle_reads_layout(bam, lay)
    bai = baiutil.build_bai(bam)
    refs, _ = baiutil.parse_bai(bai)
    # every record is in the first 16 KiB window and in one bin: the span of an interval starts
    # at the first record, so the windowed chain's segments are the whole-file chain's
    assert len(lay.records) + BIG_L < 1 << 14 and list(refs[0]["bins"]) == [4681]
    q = O.optimize_intervals(c_intervals(lay))
    spans = O.bai_span(bai, q, 0, (1 << 64) - 1)
    assert [a for a, _ in spans] == [voffset_of(bam)(H)]
    ob = O.OracleBam(bam)
    sel = ob.read_partitions(0, traversal=(c_intervals(lay), False), bai=bai)[0]
    big = lay.index[0]
    assert 0 < len(sel) < len(lay.records) and ob.read_all()["voffset"][big] in sel["voffset"]


@pytest.mark.gpu
@pytest.mark.parametrize("full_traversal", [False, True], ids=["span_run", "full_traversal"])
def test_c_gpu_interval_run_over_the_fake(full_traversal):
    """dq_run_resident with intervals.  Without full_traversal it is the .bai span run: the span
    starts at the file's first record (test_c_indexed_layout_keeps_the_fake_and_one_window), so
    the windowed chain (wseg_*) cuts the same segments, speculates the fake at segment 1 and has
    to repair it (wseg_fix_kernel).  With full_traversal the filter runs over the whole-file
    chain's records.  Both keep what the oracle's traversal through the index spans keeps."""
    bam, lay = family_c(4, True)
    bai, ivs = baiutil.build_bai(bam), c_intervals(lay)
    want = O.OracleBam(bam).read_partitions(0, traversal=(ivs, False), bai=bai, spans=True)
    assert len(want) == 1 and len(want[0]) > 0
    with _lib.Context(split_size=0, verify_crc=True, full_traversal=full_traversal) as c:
        c.open_bytes(bam)
        c.set_index(bai)
        st = c.run_resident((ivs, False))
        cnt, dig = c.partition_digests()
        assert st.n_filtered == len(want[0])
        if not full_traversal:  # the kept records themselves, by count and ordered digest
            assert 0 < st.blocks_inflated <= st.n_blocks
            assert cnt.tolist() == [len(want[0])]
            assert dig.tolist() == [O.stream_digest(want[0]["hash"])]
        assert c.run_resident((ivs, False)).n_filtered == len(want[0])  # and again


@pytest.mark.gpu
def test_c_gpu_filtered_read_over_the_fake():
    """dq_read with a traversal: the whole-file chain (repaired at the fake) and the filter."""
    bam, lay = family_c(4, True)
    parity(bam, 0, traversal=(c_intervals(lay), False), bai=baiutil.build_bai(bam))


# ------------------------------------------------------------------ D: BGZF block edges
CUT_D = (0, 1, 3, 4, 35, 36)


@functools.lru_cache(maxsize=None)
def d_layout(n=60):
    return R.layout(HDR, [R.filler(44 + (37 * i) % 400, pos=100 * i) for i in range(n)])


@functools.lru_cache(maxsize=None)
def family_d(d):
    lay = d_layout()
    return B.bgzf(lay.stream, 6, cuts=[x + d for x in lay.offsets]), lay


@functools.lru_cache(maxsize=None)
def family_d_tiny_blocks():
    """300 blocks of 150 to 200 bytes from the stream's start, all inside the first 64 KiB page."""
    lay = d_layout(330)
    cuts, c = [], 0
    for i in range(300):
        c += 150 + (7 * i) % 51
        cuts.append(c)
    return B.bgzf(lay.stream, 6, cuts=cuts), lay


@pytest.mark.parametrize("d", CUT_D)
def test_d_layout_cuts_every_record(d):
    bam, lay = family_d(d)
    pos, uoff, _ = block_table(bam)
    assert all(x + d in uoff for x in lay.offsets)
    # no empty block but the EOF block
    assert all(b > a for a, b in zip(uoff, uoff[1:])) and uoff[-1] == len(lay.stream)
    recs = assert_oracle_reads_layout(bam, lay)
    if d == 0:  # a record at a block's start reads (that block, 0), not (the block before, its size)
        assert all(int(v) & 0xffff == 0 for v in recs["voffset"])
        assert sorted(int(v) >> 16 for v in recs["voffset"]) == pos[1:len(recs) + 1]
    else:
        assert all(int(v) & 0xffff for v in recs["voffset"][1:])


def test_d_layout_tiny_blocks_share_a_page():
    bam, lay = family_d_tiny_blocks()
    pos, uoff, _ = block_table(bam)
    sizes = [b - a for a, b in zip(uoff[:300], uoff[1:301])]
    assert len(sizes) == 300 and min(sizes) >= 150 and max(sizes) <= 200
    assert uoff[300] < 1 << 16 < len(lay.stream)  # one page of the block page table, and a second
    # a record in the page's last blocks is hundreds of blocks after the page's first block
    assert sum(uoff[250] <= x < uoff[300] for x in lay.offsets) > 10
    assert_oracle_reads_layout(bam, lay)


@pytest.mark.gpu
@pytest.mark.parametrize("d", CUT_D)
def test_d_gpu_block_edges(d):
    bam, _ = family_d(d)
    for split in (0, some_split(bam, 5)):
        parity(bam, split)


@pytest.mark.gpu
def test_d_gpu_tiny_blocks():
    bam, _ = family_d_tiny_blocks()
    for split in (0, some_split(bam, 4)):
        parity(bam, split)


# ------------------------------------------------------------------ E: decode thresholds
def residue_walk(a0):
    """32 values of n mod 8 such that records of those sizes laid end to end from a start with
    p mod 4 == a0 meet every pair (n mod 8, p mod 4) once: an Euler circuit of the graph on
    Z4 with the edges a -> a + r (r = 0..7)."""
    left = {a: list(range(8)) for a in range(4)}
    stack, out = [(a0, None)], []
    while stack:
        a = stack[-1][0]
        if left[a]:
            r = left[a].pop()
            stack.append(((a + r) % 4, r))
        else:
            out.append(stack.pop()[1])
    return out[-2::-1]


def staged_group(p, target):
    """32 record sizes from stream offset p whose group has staged_len == target."""
    total = target - 32 + (p & ~15) - p
    return [380] * 31 + [total - 31 * 380]


def lay_of_sizes(sizes):
    return R.layout(HDR, [R.filler(n, pos=i) for i, n in enumerate(sizes)])


LONG_SHAPES = [k * K.LONG_PIECE + d for k in (1, 2) for d in (-1, 0, 1)]


@functools.lru_cache(maxsize=None)
def family_e_main():
    sizes = [198] * 32                                            # group 0: short records
    p = lambda: H + sum(sizes)  # noqa: E731
    sizes += staged_group(p(), K.REC_STAGE)                       # 1: the largest staged group
    sizes += staged_group(p(), K.REC_STAGE + 1)                   # 2: the smallest unstaged one
    sizes += [104 + r for r in residue_walk(p() % 4)]             # 3: residues, staged
    sizes += [400 + r for r in residue_walk(p() % 4)]             # 4: residues, unstaged
    sizes += [400] * 15 + [K.LONG_N, K.LONG_N + 1] + [400] * 15   # 5: lanes / pieces
    sizes += [400] * 13 + LONG_SHAPES + [400] * 13                # 6: one and two pieces
    sizes += [198] * 5                                            # 7: a partial last group
    lay = lay_of_sizes(sizes)
    return B.bgzf(lay.stream, 1), lay


def group_len(lay, g):
    """staged_len of group g (its bytes end where the next group starts, or the stream)."""
    a = lay.offsets[K.REC_GROUP * g]
    i = K.REC_GROUP * (g + 1)
    return R.staged_len(a, lay.offsets[i] if i < len(lay.offsets) else len(lay.stream))


def pairs(lay, g):
    return {(len(lay.records[i]) % 8, lay.offsets[i] % 4)
            for i in range(K.REC_GROUP * g, K.REC_GROUP * (g + 1))}


def test_e_layout_reaches_the_decode_thresholds():
    bam, lay = family_e_main()
    n = [len(r) for r in lay.records]
    assert len(n) == 7 * K.REC_GROUP + 5
    assert 16 * (lay.offsets[10] - lay.offsets[0]) // 10 <= K.SEG
    assert group_len(lay, 1) == K.REC_STAGE          # REC_STAGE: staged
    assert group_len(lay, 2) == K.REC_STAGE + 1      # REC_STAGE + 1: read from the stream
    every = {(r, a) for r in range(8) for a in range(4)}
    assert pairs(lay, 3) == every and group_len(lay, 3) <= K.REC_STAGE
    assert pairs(lay, 4) == every and group_len(lay, 4) > K.REC_STAGE
    assert group_len(lay, 5) > K.REC_STAGE           # unstaged, so LONG_N decides
    g5 = n[5 * K.REC_GROUP:6 * K.REC_GROUP]
    assert K.LONG_N in g5 and K.LONG_N + 1 in g5 and max(g5) == K.LONG_N + 1
    g6 = n[6 * K.REC_GROUP:7 * K.REC_GROUP]
    assert [x for x in g6 if x > K.LONG_N] == LONG_SHAPES  # LONG_PIECE k - 1, k, k + 1; k = 1, 2
    assert max(n[:5 * K.REC_GROUP]) <= K.LONG_N
    assert_oracle_reads_layout(bam, lay)


TAILS = {f"n{n}": [198] * 32 + [400] * 31 + [n] for n in [K.LONG_N, K.LONG_N + 1] + LONG_SHAPES}
TAILS["staged"] = lambda: [198] * 32 + staged_group(H + 198 * 32, K.REC_STAGE)
TAILS["unstaged"] = lambda: [198] * 32 + staged_group(H + 198 * 32, K.REC_STAGE + 1)
TAILS["residues_staged"] = lambda: [198] * 32 + [104 + r for r in residue_walk((H + 198 * 32) % 4)]
TAILS["residues_unstaged"] = lambda: [198] * 32 + [400 + r for r in residue_walk((H + 198 * 32) % 4)]
COUNTS = {f"count{n}": [198] * n for n in (1, 32, 33)}


@functools.lru_cache(maxsize=None)
def family_e_small(name):
    sizes = {**TAILS, **COUNTS}[name]
    lay = lay_of_sizes(sizes() if callable(sizes) else sizes)
    return B.bgzf(lay.stream, 1), lay


@pytest.mark.parametrize("name", sorted(TAILS))
def test_e_layout_tail_shapes_end_the_file(name):
    """Each shape once as the file's last record (the last group finds its end from the last
    record's block size, not from the next group's start)."""
    bam, lay = family_e_small(name)
    assert len(lay.records) == 2 * K.REC_GROUP
    assert lay.offsets[-1] + len(lay.records[-1]) == len(lay.stream)
    if name.startswith("n"):
        assert len(lay.records[-1]) == int(name[1:]) and group_len(lay, 1) > K.REC_STAGE
    elif name == "staged":
        assert group_len(lay, 1) == K.REC_STAGE
    elif name == "unstaged":
        assert group_len(lay, 1) == K.REC_STAGE + 1
    else:
        assert len(pairs(lay, 1)) == 32
        assert (group_len(lay, 1) <= K.REC_STAGE) == (name == "residues_staged")
    assert_oracle_reads_layout(bam, lay)


@pytest.mark.parametrize("n", [1, 32, 33])
def test_e_layout_record_counts(n):
    bam, lay = family_e_small(f"count{n}")
    assert len(lay.records) == n  # REC_GROUP - 31, REC_GROUP, REC_GROUP + 1
    assert_oracle_reads_layout(bam, lay)


@pytest.mark.gpu
def test_e_gpu_decode_thresholds():
    bam, _ = family_e_main()
    for split in (0, some_split(bam, 3)):
        parity(bam, split)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(TAILS) + sorted(COUNTS))
def test_e_gpu_tails_and_counts(name):
    parity(family_e_small(name)[0], 0)


# ------------------------------------------------------------------ F: field extremes
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
EXTREMES = {
    "flag_fffb": dict(ref=0, pos=100, name_bytes=b"f\x00", cigar=[(10, 0)], l_seq=10, flag=0xfffb),
    "bin_ffff": dict(ref=0, pos=101, name_bytes=b"b\x00", cigar=[(10, 0)], l_seq=10, bin=0xffff),
    "mapq_255": dict(ref=0, pos=102, name_bytes=b"m\x00", cigar=[(10, 0)], l_seq=10, mapq=255),
    "l_read_name_255": dict(ref=0, pos=103, name_bytes=b"n" * 254 + b"\x00", cigar=[(10, 0)], l_seq=10),
    "n_cigar_65535": dict(ref=0, pos=104, name_bytes=b"c\x00", cigar=[(1, 0)] * 65535, l_seq=65535),
    "l_seq_0_unmapped": dict(ref=-1, pos=-1, name_bytes=b"z\x00", l_seq=0, flag=4),
    "tlen_min": dict(ref=-1, pos=-1, name_bytes=b"t\x00", l_seq=5, flag=4, tlen=I32_MIN),
    "next_pos_max": dict(ref=-1, pos=-1, name_bytes=b"p\x00", l_seq=5, flag=4, next_pos=I32_MAX),
    "pos_max_no_ref": dict(ref=-1, pos=I32_MAX, name_bytes=b"q\x00", l_seq=5, flag=4),
}


@functools.lru_cache(maxsize=None)
def family_f():
    lay = R.layout(HDR, [R.filler(198)] * 12 + [R.record(**kw) for kw in EXTREMES.values()]
                   + [R.filler(198)] * 3)
    return B.bgzf(lay.stream, 1), lay


def test_f_layout_holds_the_extremes():
    bam, lay = family_f()
    assert len(bam) < 4 << 20
    recs = assert_oracle_reads_layout(bam, lay)[12:12 + len(EXTREMES)]
    e = dict(zip(EXTREMES, recs))
    assert e["flag_fffb"]["flag"] == 0xfffb and not e["flag_fffb"]["flag"] & 4
    assert e["bin_ffff"]["bin"] == 0xffff and e["mapq_255"]["mapq"] == 255
    assert e["l_read_name_255"]["l_read_name"] == 255
    assert e["n_cigar_65535"]["n_cigar"] == 65535
    assert e["n_cigar_65535"]["block_size"] == 32 + 2 + 4 * 65535 + 32768 + 65535  # the CIGAR is there
    assert e["l_seq_0_unmapped"]["l_seq"] == 0 and e["l_seq_0_unmapped"]["flag"] == 4
    assert e["tlen_min"]["tlen"] == I32_MIN and e["next_pos_max"]["next_pos"] == I32_MAX
    assert e["pos_max_no_ref"]["pos"] == I32_MAX and e["pos_max_no_ref"]["ref_id"] == -1


@pytest.mark.gpu
def test_f_gpu_field_extremes():
    bam, lay = family_f()
    parity(bam, 0)
    ref = O.OracleBam(bam).read_all()
    with _lib.Context(split_size=0, verify_crc=True) as c:
        c.open_bytes(bam)
        lean = c.read(with_raw="lean")
    n = len(lean["voffset"])
    assert n == len(lay.records) and np.array_equal(lean["voffset"], ref["voffset"])
    off, f = _lib.parse_lean(lean["raw"], n)
    assert bytes(lean["raw"]) == lay.stream[H:] and off.tolist() == [x - H for x in lay.offsets]
    for k in FIELDS:
        assert np.array_equal(f[k], ref[k]), k


# ------------------------------------------------------------------ the restated guesser
def test_spec_check_equals_the_oracle_guesser_everywhere():
    """reccases.spec_check with Disq's 10 records against OracleBam.check_record_start at every
    position of a small file that holds the odd records of family B, fakes inside qualities,
    unmapped records and the stream's end (where a chain that runs out of data still counts)."""
    fakes = R.filler(60) * 12
    items = [R.filler(100 + 7 * i, pos=i) for i in range(12)] + [f() for f in ODD.values()]
    items += [R.record(0, 50, b"q\x00", [(900, 0)], 900, qual=b"\x07" * 11 + fakes + b"\x07" * 169)]
    items += [R.record(**EXTREMES[k]) for k in EXTREMES if k != "n_cigar_65535"]
    items += [R.filler(44 + 3 * i, pos=60 + i) for i in range(11)]
    lay = R.layout(HDR, items)
    bam = B.bgzf(lay.stream, 6, cuts=range(997, len(lay.stream), 997))
    ob, v = O.OracleBam(bam), voffset_of(bam)
    want = [x for x in range(len(lay.stream)) if ob.check_record_start(v(x))]
    got = [x for x in range(len(lay.stream)) if R.spec_check(lay.stream, HINFO, x, 10)]
    assert got == want
    assert set(lay.offsets[:3]) <= set(got) and len(got) > 12  # starts, fakes and the tail
    assert not set(got) & {lay.offsets[12 + i] for i in range(len(ODD))}
    assert any(x not in lay.offsets for x in got)  # the fakes fire too


def test_make_record_bytes_are_the_hand_packed_ones():
    """bamutil.make_record builds its record through reccases.record: the bytes are those of the
    layout it packed by hand before (one M op, bin 4680, one base and one quality value)."""
    def packed(ref_id, pos, name, l_seq, flag=0, mapq=60, base=0x11, qual=30, next_ref_id=-1,
               next_pos=-1, tlen=0):
        rn = name + b"\x00"
        body = struct.pack("<iiBBHHHiiii", ref_id, pos, len(rn), mapq, 4680, 1, flag, l_seq,
                           next_ref_id, next_pos, tlen) + rn + struct.pack("<I", l_seq << 4) \
            + bytes([base]) * ((l_seq + 1) // 2) + bytes([qual]) * l_seq
        return struct.pack("<i", len(body)) + body
    for args, kw in (((0, 100, b"a", 1), {}), ((3, 7, b"read/1", 151), dict(flag=99, mapq=0)),
                     ((-1, -1, b"u", 50), dict(flag=4, base=0x48, qual=2)),
                     ((0, 5, b"m", 10), dict(next_ref_id=2, next_pos=900, tlen=-350)),
                     ((1, 2, b"long", 20001), {})):
        assert B.make_record(*args, **kw) == packed(*args, **kw)
    assert B.make_record(0, 100, b"a", 1) == R.record(0, 100, b"a\x00", [(1, 0)], 1, mapq=60, bin=4680)


# ------------------------------------------------------------------ Disq's first record
@functools.lru_cache(maxsize=None)
def rejected_lead():
    """Four plain records, one the guesser rejects, twenty plain ones."""
    lay = R.layout(HDR, [R.filler(198, pos=i) for i in range(4)] + [ODD["cigar_op_9"]()]
                   + [R.filler(198, pos=10 + i) for i in range(20)])
    return B.bgzf(lay.stream, 6), lay


def test_disq_drops_leading_records_before_a_rejected_one():
    """A split's first record comes from the 10-record guesser even at file offset 0
    (BamSource.getFirstReadInPartition): with a record the guesser rejects among the first ten,
    Disq's only partition starts after it.  (Why every other file here leads with plain records.)"""
    bam, lay = rejected_lead()
    ob, v = O.OracleBam(bam), voffset_of(bam)
    assert len(ob.read_all()) == 25
    assert ob.plan(0)[0][2][0] == v(lay.offsets[5])
    parts = ob.read_partitions(0)
    assert len(parts) == 1 and parts[0]["voffset"].tolist() == [v(x) for x in lay.offsets[5:]]


@pytest.mark.gpu
def test_gpu_drops_the_same_leading_records():
    bam, lay = rejected_lead()
    b = parity(bam, 0)
    assert len(b["voffset"]) == 20
