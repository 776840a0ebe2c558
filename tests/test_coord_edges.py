"""The interval filter (interval_filter_kernel) and the .bai keys (bai_keys_kernel) on records whose
coordinates sit on the edges of those kernels' rules: every CIGAR op code, reference length 0,
placed-unmapped records, records that begin or end on a bin edge of every level or at 2^29, and
intervals one base before and after each record's start and end.

The expected selection is a brute force in this file (the rule in dq_kernels.hip's kernel-4
comment, on the alignment ends computed from the CIGARs that were laid out), first held against
the oracle's overlap test on the CPU; the expected index bytes are tests/baiutil.py's."""
import functools

import numpy as np
import pytest

from disq_amd import _lib
from oracle import oracle as O

import baiutil
import bamutil as B
import reccases as R

I32_MAX = (1 << 31) - 1
REFS = [("big", I32_MAX), ("r1", 1000), ("r2", 1 << 29)]
HDR = R.header(REFS)
LEVEL_EDGES = [1 << 14, 1 << 17, 1 << 20, 1 << 23, 1 << 26]
# the sixteen op-code records start 20 bases before a 16 KiB bin edge: with a reference length of
# 22 they cross it (another bin, another linear window), with 15 they do not, so the index bytes
# depend on each op code's rule as the interval filter's result does
OP_POS = [((k + 2) << 14) - 20 for k in range(16)]
# Disq's split planner takes a file's first record from its 10-record guesser, which rejects CIGAR
# op codes above 8 and references beyond the header's: twelve plain records lead every file here,
# so that the odd records are not among the ten after the first and the chunk starts at the first
LEAD = 12


def _rec(ref, pos, cigar, flag=0, name=b"r", tag=None):
    l_seq = max(1, sum(n for n, op in cigar))
    return dict(ref=ref, pos=pos, cigar=cigar, flag=flag, tag=tag,
                bytes=R.record(ref, pos, name + b"\x00", cigar, l_seq, flag=flag, mapq=30))


@functools.lru_cache(maxsize=None)
def coord_file():
    """(bam, layout, the records as dicts of what was laid out), coordinate sorted."""
    recs = [_rec(0, 10 * i, [(5, 0)]) for i in range(LEAD)]
    recs += [_rec(0, OP_POS[k], [(10, 0), (7, k), (5, 0)], tag=f"op{k}") for k in range(16)]  # 10M 7<op> 5M
    recs.append(_rec(0, 3000, [(20, 4)], tag="soft"))         # soft clip only: reference length 0
    recs.append(_rec(0, 3200, [(30, 0)], flag=4, tag="unmapped_cigar"))  # placed unmapped, with a CIGAR
    recs.append(_rec(0, 3300, [], flag=4, tag="unmapped"))    # placed unmapped, without
    for e in LEVEL_EDGES:
        recs += [_rec(0, p, [(n, 0)], tag=f"edge{e}_{j}") for j, (p, n) in enumerate(
            ((e - 10, 10), (e - 10, 11), (e - 1, 1), (e - 1, 2), (e, 1)))]
    recs.append(_rec(0, (1 << 29) - 50, [(50, 0)], tag="ends_2^29"))  # ends exactly at 2^29
    recs.append(_rec(2, (1 << 29) - 1, [(1, 0)], tag="r2_last"))      # the last base of r2
    recs.sort(key=lambda r: (r["ref"], r["pos"]))             # (stable: equal positions keep their order)
    recs.append(_rec(0, -1, [], flag=4))                      # pos -1 on reference 0: no coordinate
    recs += [_rec(-1, -1, [], flag=4, name=b"u%d" % i) for i in range(3)]
    lay = R.layout(HDR, [r["bytes"] for r in recs])
    return B.bgzf(lay.stream, 6), lay, recs


def alignment(recs):
    """(ref, alignmentStart, alignmentEnd) as kernel 4 defines them: end = pos + the M/D/N/=/X
    lengths for a mapped read, the start for an unmapped read with a position, 0 otherwise."""
    ref = np.array([r["ref"] for r in recs], np.int64)
    start = np.array([r["pos"] + 1 for r in recs], np.int64)
    rl = np.array([R.ref_len_of(r["cigar"]) for r in recs], np.int64)
    mapped = np.array([not r["flag"] & 4 for r in recs])
    return ref, start, np.where(mapped, start + rl - 1, start)


def brute(recs, q):
    """The records an optimized interval list q keeps: a record matches iff an interval on its
    reference has start <= alignmentEnd and end >= alignmentStart (end <= 0: the contig's end)."""
    ref, start, end = alignment(recs)
    keep = np.zeros(len(recs), bool)
    for r, s, e in q:
        keep |= (ref == r) & (s <= end) & ((e if e > 0 else I32_MAX) >= start)
    return keep


def idx(tag):
    """The record number of a tagged record."""
    return [r["tag"] for r in coord_file()[2]].index(tag)


def placed(recs):
    return [i for i, r in enumerate(recs) if r["ref"] >= 0 and r["pos"] >= 0]


@functools.lru_cache(maxsize=None)
def queries():
    """name -> interval list (as a caller gives it: unsorted, unmerged)."""
    _, _, recs = coord_file()
    ref, start, end = alignment(recs)
    kinds = {"before_start": [], "at_start": [], "at_end": [], "after_end": []}
    for i in placed(recs):
        r, s, e = int(ref[i]), int(start[i]), int(end[i])
        for name, x in (("before_start", s - 1), ("at_start", s), ("at_end", e), ("after_end", e + 1)):
            if 1 <= x <= REFS[r][1]:
                kinds[name].append((r, x, x))
    q = dict(kinds)
    q["all_edges"] = [iv for k in kinds.values() for iv in k][::-1]  # about 200, unsorted
    for r in range(3):
        q[f"whole_ref{r}"] = [(r, 1, 0)]
    for i in placed(recs):  # from one base after every record's end to the contig's end
        if 1 <= int(end[i]) + 1 <= REFS[int(ref[i])][1]:
            q[f"after_end_to_contig_end_{i:02d}"] = [(int(ref[i]), int(end[i]) + 1, 0)]
    # abutting and overlapping pairs that optimizeIntervals merges (the first pair only matches
    # the soft-clip-only record, start 3001 and end 3000, once merged), a reference without
    # records, an interval given twice
    q["merged"] = [(0, 3001, 3002), (0, 2999, 3000), (0, 40000, 40010), (0, 40005, 49200), (1, 1, 1000),
                   (0, 1 << 14, 1 << 14), (0, 1 << 14, 1 << 14), (0, (1 << 14) + 1, (1 << 14) + 5)]
    return q


def expected(name):
    bam, lay, recs = coord_file()
    return brute(recs, O.optimize_intervals(queries()[name]))


def test_coord_file_is_what_was_laid_out():
    bam, lay, recs = coord_file()
    got = O.OracleBam(bam).read_all()
    assert got["pos"].tolist() == [r["pos"] for r in recs]
    assert got["ref_id"].tolist() == [r["ref"] for r in recs]
    assert got["hash"].tolist() == [O.record_hash(r["bytes"]) for r in recs]
    assert O.OracleBam(bam).plan(0)[0][2][0] == got["voffset"][0] == len(HDR)  # Disq reads them all
    ref, start, end = alignment(recs)
    for k in range(16):  # an interval one base wide tells reference length 22 from 15
        i = idx(f"op{k}")
        assert end[i] - start[i] + 1 == (22 if k in R.REF_OPS else 15)
        assert bool(brute(recs, [(0, OP_POS[k] + 16, OP_POS[k] + 16)])[i]) == (k in R.REF_OPS)
        # and reference length 22 crosses a 16 KiB bin edge where 15 does not
        assert (baiutil.reg2bin(OP_POS[k], int(end[i])) < 4681) == (k in R.REF_OPS)
    assert [(r["ref"], r["pos"]) for r in recs[:len(placed(recs))]] == sorted(
        (r["ref"], r["pos"]) for r in recs[:len(placed(recs))])
    assert end[idx("soft")] == start[idx("soft")] - 1  # reference length 0
    assert all(end[idx(t)] == start[idx(t)] for t in ("unmapped", "unmapped_cigar"))
    on_edge = {int(e) for e in end[placed(recs)]} | {int(s) - 1 for s in start[placed(recs)]}
    assert all(e in on_edge for e in LEVEL_EDGES + [1 << 29])  # records end / begin on each edge
    assert int(end[len(placed(recs)) - 1]) == 1 << 29 and recs[len(placed(recs)) - 1]["ref"] == 2
    assert len(recs) - len(placed(recs)) == 4
    tails = [n for n in queries() if n.startswith("after_end_to_contig_end_")]
    assert len(tails) == len(placed(recs)) - 1  # every placed record but the last base of r2
    assert 180 <= len(queries()["all_edges"]) <= 260


def test_optimize_merges_the_pairs():
    assert O.optimize_intervals(queries()["merged"]) == [
        (0, 2999, 3002), (0, 1 << 14, (1 << 14) + 5), (0, 40000, 49200), (1, 1, 1000)]
    _, _, recs = coord_file()
    soft = idx("soft")
    assert expected("merged")[soft]  # the soft-clip-only record, by the merged interval only
    assert not brute(recs, [(0, 2999, 3000)])[soft] and not brute(recs, [(0, 3001, 3002)])[soft]
    assert expected("merged")[idx("op1")] and expected("merged").sum() > 5


@pytest.mark.parametrize("name", sorted(queries()))
def test_brute_force_equals_the_oracle(name):
    """The two references agree before the GPU is asked: the oracle's overlap test record by
    record, and its traversal through the index (the .bai spans of the intervals)."""
    bam, lay, recs = coord_file()
    ivs = queries()[name]
    ob = O.OracleBam(bam)
    allr = ob.read_all()
    q = O.optimize_intervals(ivs)
    want = expected(name)
    assert [O.overlaps(r, q) for r in allr] == want.tolist()
    bai = baiutil.build_bai(bam)
    for spans in (False, True):
        got = ob.read_partitions(0, traversal=(ivs, False), bai=bai, spans=spans)
        assert np.array_equal(np.concatenate(got)["voffset"], allr["voffset"][want]), spans
    on_ref0 = want[placed(recs)]
    if name == "whole_ref0":  # the soft-clip-only record and the placed unmapped ones too
        assert on_ref0[:-1].all() and not on_ref0[-1] and want.sum() == len(on_ref0) - 1
    if name in ("at_start", "at_end"):  # every record but the one of reference length 0
        assert [i for i in placed(recs) if not want[i]] == [idx("soft")]
    if name == "whole_ref1":
        assert not want.any()


@pytest.mark.gpu
@pytest.mark.parametrize("full_traversal", [True, False], ids=["full_traversal", "span_run"])
def test_gpu_interval_filter(full_traversal):
    """read(traversal=...) filters the whole-file pipeline's records in both cases;
    run_resident(...) is the filter over the whole resident stream with full_traversal and the
    .bai span run without it, where the partition's count and ordered digest say which records
    the span run kept."""
    bam, lay, recs = coord_file()
    allr = O.OracleBam(bam).read_all()
    with _lib.Context(split_size=0, verify_crc=True, full_traversal=full_traversal) as c:
        c.open_bytes(bam)
        c.set_index(baiutil.build_bai(bam))
        for name, ivs in sorted(queries().items()):
            want = expected(name)
            got = c.read(with_raw=False, traversal=(ivs, False))["voffset"]
            assert np.array_equal(got, allr["voffset"][want]), name
            assert c.run_resident((ivs, False)).n_filtered == int(want.sum()), name
            if not full_traversal:
                cnt, dig = c.partition_digests()
                assert cnt.tolist() == [int(want.sum())], name
                assert dig.tolist() == [O.stream_digest(allr["hash"][want])], name


@pytest.mark.gpu
def test_gpu_interval_filter_chunk_from_disk(tmp_path):
    bam, lay, recs = coord_file()
    path = str(tmp_path / "coord.bam")
    with open(path, "wb") as fh:
        fh.write(bam)
    ob = O.OracleBam(bam)
    voff = ob.read_all()["voffset"]
    chunk = ob.plan(0)[0][2]
    with _lib.Context(split_size=0, verify_crc=True) as c:
        c.set_index(baiutil.build_bai(bam))
        for name in ("all_edges", "merged", "after_end"):
            got = c.decode_chunk(path, *chunk, with_raw=False, traversal=(queries()[name], False))
            assert np.array_equal(got["voffset"], voff[expected(name)]), name


# ------------------------------------------------------------------ .bai keys
@pytest.mark.gpu
def test_gpu_bai_equals_restatement_on_the_edges():
    bam, lay, recs = coord_file()
    with _lib.Context(split_size=0) as c:
        c.open_bytes(bam)
        assert c.write_bai() == baiutil.build_bai(bam)


@pytest.mark.gpu
def test_gpu_bai_records_at_block_starts():
    from test_record_edges import family_d
    bam, lay = family_d(0)
    with _lib.Context(split_size=0) as c:
        c.open_bytes(bam)
        assert c.write_bai() == baiutil.build_bai(bam)


def test_restated_bai_of_the_edges():
    """What the restatement says about this file: every record on a level edge in the bin the
    SAM specification gives it, the record that ends at 2^29 in the last 16 KiB window."""
    bam, lay, recs = coord_file()
    refs, n_no_coor = baiutil.parse_bai(baiutil.build_bai(bam))
    assert n_no_coor == 4 and not refs[1]["bins"] and refs[1]["meta"] is None
    assert len(refs[0]["linear"]) == len(refs[2]["linear"]) == 1 << 15
    first = {1 << 14: 4681, 1 << 17: 585, 1 << 20: 73, 1 << 23: 9, 1 << 26: 1}
    for e, lvl0 in first.items():
        # up to the edge and from it on: two neighbouring 16 KiB bins; across it: one level up
        assert baiutil.reg2bin(e - 10, e) == baiutil.reg2bin(e - 1, e) == 4681 + (e >> 14) - 1
        assert baiutil.reg2bin(e, e + 1) == 4681 + (e >> 14)
        crossing = baiutil.reg2bin(e - 1, e + 1)
        assert crossing == baiutil.reg2bin(e - 10, e + 1) < lvl0
        assert {crossing, 4681 + (e >> 14) - 1, 4681 + (e >> 14)} <= set(refs[0]["bins"])
    assert refs[0]["meta"][1] == (LEAD + 16 + 1 + 25 + 1, 2)


_LEAD = [(0, i, 5) for i in range(LEAD)]
ERRORS = {
    "end_beyond_2^29": (_LEAD + [(0, 100, 50), (0, (1 << 29) - 49, 50)],
                        f"record {LEAD + 1}: alignment end beyond 2^29, the .bai limit"),
    "reference_3_of_3": (_LEAD + [(0, 100, 50), (2, 200, 50), (3, 300, 50)],
                         f"record {LEAD + 2}: reference index beyond the header's references"),
    "unsorted_before_out_of_range": (
        _LEAD + [(0, 100, 50), (0, 200, 50), (0, 150, 50), (0, (1 << 29) + 10, 50)],
        f"not coordinate sorted: record {LEAD + 2} is out of order"),
}


@functools.lru_cache(maxsize=None)
def error_file(name):
    lay = R.layout(HDR, [R.record(r, p, b"e%d\x00" % i, [(n, 0)], n, mapq=30)
                         for i, (r, p, n) in enumerate(ERRORS[name][0])])
    return B.bgzf(lay.stream, 6)


@pytest.mark.parametrize("name", sorted(ERRORS))
def test_restated_bai_errors(name):
    bam = error_file(name)
    ob = O.OracleBam(bam)
    assert len(ob.read_all()) == len(ERRORS[name][0])
    assert ob.plan(0)[0][2][0] == len(HDR)  # Disq's chunk starts at the first record
    with pytest.raises(ValueError) as e:
        baiutil.build_bai(bam)
    assert str(e.value) == ERRORS[name][1]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ERRORS))
def test_gpu_bai_coordinate_errors(name):
    """The status words the host reports (BAI_ST_END, BAI_ST_REF, and the earlier offender of
    two): DQ_EFORMAT with the restatement's message, and the context still reads the file."""
    bam = error_file(name)
    with pytest.raises(ValueError) as want:
        baiutil.build_bai(bam)
    ref = O.OracleBam(bam).read_all()
    with _lib.Context(split_size=0) as c:
        c.open_bytes(bam)
        with pytest.raises(_lib.DqError) as e:
            c.write_bai()
        assert e.value.code == _lib.DQ_EFORMAT
        assert str(e.value).endswith(str(want.value))
        b = c.read(with_raw=False)
        assert np.array_equal(b["voffset"], ref["voffset"]) and np.array_equal(b["hash"], ref["hash"])
        with pytest.raises(_lib.DqError):
            c.write_bai()
        assert len(c.read(with_raw=False)["voffset"]) == len(ref)
