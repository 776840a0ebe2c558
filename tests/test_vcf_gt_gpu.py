"""VCF genotype decode on the GPU: dq_vcf_genotypes against the
plain-Python oracle tests/vcfgtutil.py applied to the oracle's text partitions (oracle/oracle.py),
cell for cell -- both fixtures, synthetic files around the thread / wave threshold and the ballot
window edges, every error class with its exact message, interval traversal, GQ texts the host
converts, sites-only files, other contexts, the storage layer."""
import os
import re

import numpy as np
import pytest

from disq_amd import _lib
from oracle import oracle as O
import textutil as T
import vcfcases as K
import vcfgtcases as GK
import vcfgtutil as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "disq_amd", "csrc")
VCF_LONG = int(re.search(r"VCF_LONG = (\d+);", open(os.path.join(CSRC, "dq_vcf.hip")).read()).group(1))
_GT = open(os.path.join(CSRC, "dq_vcf_gt.hip")).read()
GT_WAVE_S = int(re.search(r"GT_WAVE_S = (\d+);", _GT).group(1))     # the path threshold
GT_OFFS = int(re.search(r"GT_OFFS = (\d+);", _GT).group(1))         # a wave's offset list
GT_WSLOT = int(re.search(r"GT_WSLOT = (\d+);", _GT).group(1))       # a wave's LDS slot


def want_arrays(rows, S):
    """The oracle's cells of the variants as the arrays of dq_genotype_batch."""
    n = len(rows)
    P = max([1] + [len(c["alleles"]) for r in rows for c in r]) if S else 0
    w = {"flags": np.zeros((n, S), np.uint8), "ploidy": np.zeros((n, S), np.uint8),
         "allele": np.full((n, S, P), -2, np.int16), "gq": np.zeros((n, S), np.int32),
         "dp": np.zeros((n, S), np.int32), "cell_off": np.zeros((n, S), np.int32)}
    for k, r in enumerate(rows):
        for s, c in enumerate(r):
            w["flags"][k, s], w["ploidy"][k, s] = c["flags"], len(c["alleles"])
            w["allele"][k, s, :len(c["alleles"])] = c["alleles"]
            w["gq"][k, s], w["dp"][k, s], w["cell_off"][k, s] = c["gq"], c["dp"], c["cell_off"]
    return w, P, sum(c["gq_host"] for r in rows for c in r)


def assert_gt_parity(data, split, intervals=None, tbi=None):
    ot = O.OracleText(data)
    u = ot.inflated()
    names = G.sample_names(bytes(u))
    S = len(names)
    if intervals is None:
        parts = ot.read_partitions(split, True)
    else:
        parts = [p for _, p in ot.read_partitions_intervals(split, intervals, tbi)]
    rows = [G.gt_decode_line(bytes(u[a:a + l]), S) if S else []
            for vs, vl in parts for a, l in zip(vs.tolist(), vl.tolist())]
    want, P, nhost = want_arrays(rows, S)
    with _lib.Context(split_size=split, verify_crc=True) as c:
        c.text_open_bytes(data)
        if intervals is not None:
            c.text_set_index(tbi)
            c.text_set_intervals(intervals)
        g = c.vcf_genotypes()                       # runs the site decode itself
        v = c.vcf_read(_lib.VCF_EXPORT_FIELDS)
        st = c.vcf_genotypes_run()
        g2 = c.vcf_genotypes()
    assert g["samples"] == names and g["n_samples"] == S and g["max_ploidy"] == P
    assert g["n_gq_host"] == nhost
    for k, w in want.items():
        assert g[k].shape == w.shape and g[k].dtype == w.dtype, k
        assert np.array_equal(g[k], w), k
        assert np.array_equal(g2[k], w), k
    # the rows are dq_vcf_read's variants: the same count and partitions, and every cell starts
    # behind a TAB of the line at line_offset
    assert len(v["pos"]) == len(rows) and np.array_equal(g["part_offset"], v["part_offset"])
    assert [int(x) for x in np.diff(g["part_offset"])] == [len(vs) for vs, _ in parts]
    if S and len(rows):
        at = v["line_offset"][:, None] + g["cell_off"]
        assert np.all(u[at - 1] == 9) and np.all(g["cell_off"] < v["line_len"][:, None] + 1)
        assert np.all(v["n_sample_cols"] == S)
    assert st.ms_records > 0 or not len(rows)
    return g, v, rows


# ---- 1. fixtures
@pytest.mark.parametrize("split", [0, 500])          # one BGZF block: two partitions, the second empty
def test_test_vcf(golden, split):
    d = open(os.path.join(golden, "test.vcf.bgz"), "rb").read()
    g, v, rows = assert_gt_parity(d, split)
    assert g["flags"].shape == (5, 3) and g["max_ploidy"] == 2 and g["n_gq_host"] == 0
    assert (len(g["part_offset"]) - 1 == 2) == bool(split)
    assert g["allele"][0, 1].tolist() == [1, 0] and g["flags"][0, 1] == 15 and g["gq"][0, 1] == 48 and g["dp"][0, 1] == 8
    assert (g["gq"][1, 2], g["dp"][1, 2], g["allele"][2, 2].tolist()) == (41, 3, [2, 2])


@pytest.mark.parametrize("split", [0, 64 * 1024])
def test_hiseq(golden, split):
    d = open(os.path.join(golden, "HiSeq.10000.vcf.bgz"), "rb").read()
    g, v, rows = assert_gt_parity(d, split)
    assert g["flags"].shape == (9965, 1) and (len(g["part_offset"]) - 1 > 2) == bool(split)
    assert int(g["gq"].sum()) == 907868 and int(g["dp"].sum()) == 611423 and g["n_gq_host"] == 0
    assert int((g["allele"][:, 0] == [0, 1]).all(axis=1).sum()) == 7128


@pytest.mark.parametrize("intervals", [
    [("chr1", 2700000, 2800000)],
    [("chr1", 2700000, 2800000), ("chr1", 4000000, 4100000), ("chr1", 4050000, 4060000)],
    [("chr2", 1, 1000000)],
])
def test_hiseq_intervals(golden, intervals):
    d = open(os.path.join(golden, "HiSeq.10000.vcf.bgz"), "rb").read()
    tbi = open(os.path.join(golden, "HiSeq.10000.vcf.bgz.tbi"), "rb").read()
    g, v, rows = assert_gt_parity(d, 128 * 1024, intervals, tbi)
    assert (len(rows) > 0) == (intervals[0][0] == "chr1") and len(rows) < 9965


# ---- 2. synthetic files: the sample counts around the path threshold, the ballot width and the
# wave's offset list; ploidies 1, 2 and 3; lines either side of VCF_LONG and of the wave's LDS slot
SYNTH = GK.synth_cases(GT_WAVE_S, GT_OFFS)


@pytest.mark.parametrize("S,maxp", SYNTH)
def test_synthetic_files(S, maxp):
    text = GK.synth_file(S, maxp)
    lines = T.split_lines(text)[-12:]
    lens = [len(l) for l in lines]
    assert min(lens) <= VCF_LONG < max(lens) or S > 300
    data = T.bgzf_text(text, block_u=3000, cuts=T.corner_cuts(text))
    for split in (0, max(200, len(data) // 3)):
        g, v, rows = assert_gt_parity(data, split)
        assert g["flags"].shape == (12, S) and g["max_ploidy"] == maxp
        assert (len(g["part_offset"]) - 1 >= 2) == bool(split)
    # -2 fills past each cell's ploidy, and only there
    filled = np.arange(maxp)[None, None, :] >= g["ploidy"][:, :, None]
    assert np.array_equal(g["allele"] == -2, filled) and int(g["ploidy"].max()) == maxp
    if S > GT_OFFS:   # the list is flushed mid-line; a short line's tail fits the slot, a rich one's does not
        tails = [len(l) - l.index(b"\tGT:") for l in lines]
        assert min(tails) <= GT_WSLOT < max(tails)


def test_max_ploidy_spans_one_two_three():
    assert {p for _, p in SYNTH} == {1, 2, 3}
    assert {GT_WAVE_S - 1, GT_WAVE_S} <= {S for S, _ in SYNTH} and GT_WAVE_S > 2


def test_good_table():
    text = K.HEADER + b"".join(l + b"\n" for l in GK.GOOD)
    g, v, rows = assert_gt_parity(T.bgzf_text(text), 0)
    assert g["max_ploidy"] == 3 and g["n_gq_host"] == 8


# ---- 3. errors
NH = K.HEADER.count(b"\n")   # '#' lines before the first data line


def _file(lines, header=K.HEADER):
    return T.bgzf_text(header + b"".join(l + b"\n" for l in lines))


def _error_of(c, data):
    c.text_open_bytes(data)
    with pytest.raises(_lib.DqError) as e:
        c.vcf_genotypes()
    assert e.value.code == _lib.DQ_EFORMAT
    n = len(c.vcf_read(_lib.VCF_EXPORT_FIELDS)["pos"])      # dq_vcf_read still succeeds
    assert n == len(c.text_read(True)["line_len"])
    with pytest.raises(_lib.DqError):
        c.vcf_genotypes_run()
    return str(e.value)


def _msg(k, what, sample):
    return f"VCF line {k}: " + ("" if sample is None else f"sample {sample}: ") + what


def test_every_error_class():
    good = [GK.gline(b"GT:GQ", [b"0/1:5", b"1/1:7"], pos=b"%d" % (10 + i)) for i in range(20)]
    with _lib.Context() as c:
        for bad, what, sample in GK.BAD + GK.ORDER:
            msg = _error_of(c, _file(good + [bad]))
            assert msg.endswith(_msg(NH + 20, what, sample)), (bad, msg)


def test_every_error_class_in_the_wave_kernel():
    S = 70
    assert S >= GT_WAVE_S
    ok = [b"0/1:5:3"] * S

    def line(fmt=b"GT:GQ:DP", edit=None, cells=None):
        cs = list(cells if cells is not None else ok)
        for s, cell in (edit or {}).items():
            cs[s] = cell
        return GK.gline(fmt, cs)
    cases = [(line(cells=ok[:-1]), "samples", None), (line(cells=ok + [b"0/1"]), "samples", None),
             (line(fmt=b"GQ:GT:DP"), "FORMAT", None), (line(fmt=b"GT:GQ:GQ"), "FORMAT", None),
             (GK.gline(b"", ok), "FORMAT", None),
             (line(edit={69: b"0/1:5:3:9"}), "cell", 69),
             (line(edit={64: b"0/2:5:3"}), "GT", 64), (line(edit={3: b"0/x"}), "GT", 3),
             (line(edit={63: b"0/1:zz"}), "GQ", 63), (line(edit={65: b"0/1:5:3.0"}), "DP", 65),
             # two bad cells: the lower sample, whatever its class and lane
             (line(edit={66: b"0/x", 2: b"0/1:5:y"}), "DP", 2),
             (line(edit={1: b"0/1:q", 65: b"0/1:5:3:9"}), "GQ", 1)]
    good = [line() for _ in range(9)]
    with _lib.Context() as c:
        for bad, what, sample in cases:
            msg = _error_of(c, _file(good + [bad], GK.header(S)))
            assert msg.endswith(_msg(NH + 9, what, sample)), (what, sample, msg)


def test_first_offender_wins():
    good = [GK.gline(b"GT:GQ", [b"0/1:5", b"1/1:7"], pos=b"%d" % (10 + i)) for i in range(300)]
    bad_dp, bad_fmt, bad_gt = GK.BAD[24][0], GK.BAD[4][0], GK.BAD[14][0]
    with _lib.Context() as c:
        # two bad lines: the lower one, though its class comes later in the order
        assert _error_of(c, _file(good[:7] + [bad_dp] + good[7:280] + [bad_fmt] + good[280:])).endswith(
            _msg(NH + 7, "DP", 0))
        assert _error_of(c, _file([bad_gt] + good + [bad_dp])).endswith(_msg(NH, "GT", 1))
        # two bad cells in one line: the lower sample
        two = GK.gline(b"GT:GQ:DP", [b"0/1:5:y", b"0/x"])
        assert _error_of(c, _file(good + [two])).endswith(_msg(NH + 300, "DP", 0))
        # the site decode's errors come first, unchanged
        c.text_open_bytes(_file(good[:3] + [bad_gt, K.line(pos=b"x")]))
        with pytest.raises(_lib.DqError, match=f"VCF line {NH + 4}: POS"):
            c.vcf_genotypes()


def test_bad_line_outside_every_interval_is_not_reported():
    text = GK.synth_text(3, 2, seed=5, n=400)
    lines = T.split_lines(text)
    nh = len(lines) - 400
    bad = GK.gline(b"GT:GQ", [b"0/1:5", b"0/x", b"0/1"], pos=b"90000")
    data = T.bgzf_text(b"\n".join(lines + [bad]) + b"\n", block_u=8000)
    tbi = T.whole_file_tabix(["chr1", "chr2", "chrM"], len(data))
    g, v, rows = assert_gt_parity(data, 0, [("chr1", 150, 250)], tbi)      # POS 100 .. 499 and 90000
    assert v["pos"].tolist() == list(range(150, 251))
    with _lib.Context() as c:                                              # inside an interval it is
        c.text_open_bytes(data)
        c.text_set_index(tbi)
        c.text_set_intervals([("chr1", 150, 250), ("chr1", 89999, 90001)])
        with pytest.raises(_lib.DqError) as e:
            c.vcf_genotypes()
        assert str(e.value).endswith(_msg(nh + 400, "GT", 1))
        assert len(c.vcf_read(_lib.VCF_EXPORT_FIELDS)["pos"]) == 102


# ---- 4. GQ texts the host converts
@pytest.mark.parametrize("S", [2, 66])
def test_gq_texts_the_host_converts(S):
    texts = [b"1e1", b".5", b"12.5000000", b"1234567890", b"0.49999999999999999999", b"1e400"]
    gqs = [10, 1, 13, 1234567890, 1, -1]
    lines = [GK.gline(b"GT:GQ", [b"0/1:7"] * (S - 1) + [b"1/1:" + t], pos=b"%d" % (5 + i)) for i, t in enumerate(texts)]
    lines.append(GK.gline(b"GT:GQ", [b"0/1:12.5"] * S))
    g, v, rows = assert_gt_parity(_file(lines, GK.header(S)), 0)
    assert g["n_gq_host"] == len(texts)
    assert g["gq"][:6, S - 1].tolist() == gqs and np.all(g["flags"][:6, S - 1] & _lib.GT_HAS_GQ)
    assert np.all(g["gq"][6] == 13) and np.all(g["gq"][:6, :S - 1] == 7)


# ---- 5. edges
def test_sites_only_file():
    text = K.SITES_HEADER + b"".join(l + b"\n" for l in K.sites_good_lines())
    g, v, rows = assert_gt_parity(T.bgzf_text(text), 0)
    assert g["n_samples"] == 0 and g["samples"] == [] and g["max_ploidy"] == 0
    assert all(g[k].size == 0 for k in ("flags", "ploidy", "allele", "gq", "dp", "cell_off"))
    assert len(v["pos"]) == 3 and g["part_offset"].tolist() == [0, 3]


def test_header_only_file():
    g, v, rows = assert_gt_parity(T.bgzf_text(K.HEADER), 0)
    assert g["n_samples"] == 2 and g["max_ploidy"] == 1 and g["allele"].shape == (0, 2, 1)


def test_other_contexts_are_refused(golden):
    import samcases
    with _lib.Context() as c:
        for call in (c.vcf_genotypes, c.vcf_genotypes_run):     # no open file
            with pytest.raises(_lib.DqError) as e:
                call()
            assert e.value.code == _lib.DQ_EINVAL
        c.open_bytes(open(os.path.join(golden, "1.bam"), "rb").read())
        for call in (c.vcf_genotypes, c.vcf_genotypes_run):
            with pytest.raises(_lib.DqError) as e:
                call()
            assert e.value.code == _lib.DQ_EINVAL
        c.sam_open_bytes(samcases.HEADER + samcases.good_lines()[0] + b"\n")
        for call in (c.vcf_genotypes, c.vcf_genotypes_run):
            with pytest.raises(_lib.DqError) as e:
                call()
            assert e.value.code == _lib.DQ_EINVAL
        c.text_open_bytes(open(os.path.join(golden, "test.vcf.bgz"), "rb").read())
        assert c.vcf_genotypes()["flags"].shape == (5, 3)


def test_run_stats(golden):
    d = open(os.path.join(golden, "HiSeq.10000.vcf.bgz"), "rb").read()
    with _lib.Context(split_size=128 * 1024) as c:
        c.text_open_bytes(d)
        v = c.vcf_run()
        g = c.vcf_genotypes_run()
        b = c.vcf_genotypes()                  # the matrix of the run, no second decode needed
    assert (g.n_records, g.n_partitions, g.digest) == (v.n_records, v.n_partitions, v.digest)
    assert g.ms_records > v.ms_records > 0 and g.ms_total > v.ms_total and b["flags"].shape == (9965, 1)


def test_storage_genotypes(golden, tmp_path):
    import shutil
    from disq_amd.storage import HtsjdkVariantsRddStorage
    p = str(tmp_path / "test.vcf.bgz")
    shutil.copy(os.path.join(golden, "test.vcf.bgz"), p)
    st = HtsjdkVariantsRddStorage.makeDefault()
    with pytest.raises(ValueError):
        st.read(p, genotypes=True)
    plain = st.read(p, decode=True)
    assert plain.getGenotypes() is None and plain.getSampleNames() is None
    rdd = st.read(p, decode=True, genotypes=True)
    assert rdd.getSampleNames() == [b"NA00001", b"NA00002", b"NA00003"]
    parts = rdd.getGenotypes()
    assert len(parts) == rdd.getVariants().getNumPartitions() == 1 and len(parts[0]) == 5
    assert rdd.getVariants().collect() == plain.getVariants().collect()
    gp = parts[0]
    assert gp.allele.shape == (5, 3, 2) and gp.allele[2].tolist() == [[1, 2], [2, 1], [2, 2]]
    assert gp.gq[4].tolist() == [35, 17, 40] and gp.dp[0].tolist() == [1, 8, 5]
    assert (gp.flags[:, :2] & _lib.GT_PHASED).astype(bool).tolist() == [[True, True]] * 4 + [[False, False]]
