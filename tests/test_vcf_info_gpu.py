"""VCF INFO decode on the GPU: dq_vcf_info against the plain-Python
oracle tests/vcfinfoutil.py applied to the oracle's text partitions (oracle/oracle.py), cell for cell
and array for array -- both fixtures, key lists of 1, 13 and 64, type overrides, synthetic files
around the thread / wave threshold and the ballot window edges, every error of the table in both
kernels with its exact message, interval traversal, Float texts the host converts, other contexts,
the storage layer."""
import os

import numpy as np
import pytest

from disq_amd import _lib
from oracle import oracle as O
import textutil as T
import vcfcases as K
import vcfinfocases as C
import vcfinfoutil as U
from test_vcf_info_core_cpu import INFO_WAVE, INFO_WSLOT, VCF_LONG, TEST_KEYS, synth_texts
from test_vcf_info_rules import HISEQ_KEYS

pytestmark = pytest.mark.gpu


def assert_info_parity(data, split, keys, intervals=None, tbi=None):
    ot = O.OracleText(data)
    u = ot.inflated()
    rkeys = U.resolve_keys(keys, U.info_header(bytes(u)))
    if intervals is None:
        parts = ot.read_partitions(split, True)
    else:
        parts = [p for _, p in ot.read_partitions_intervals(split, intervals, tbi)]
    rows = [U.info_decode_line(bytes(u[a:a + l]), rkeys)
            for vs, vl in parts for a, l in zip(vs.tolist(), vl.tolist())]
    want, nhost = U.want_arrays(rows, rkeys)
    with _lib.Context(split_size=split, verify_crc=True) as c:
        c.text_open_bytes(data)
        if intervals is not None:
            c.text_set_index(tbi)
            c.text_set_intervals(intervals)
        g = c.vcf_info(keys)                        # runs the site decode itself
        v = c.vcf_read(_lib.VCF_EXPORT_FIELDS)
        st = c.vcf_info_run(keys)
        g2 = c.vcf_info(keys)
    n = len(rows)
    assert g["keys"] == [k[0] for k in rkeys] and g["n_float_host"] == nhost
    for k, w in want.items():
        for got in (g[k], g2[k]):
            got = got.view(np.uint64) if k == "fval" else got
            assert got.shape == w.shape and got.dtype == w.dtype, k
            assert np.array_equal(got, w), k
    # the rows are dq_vcf_read's variants: the same count and partitions; every value text starts
    # behind an '=' inside the line's INFO column
    assert len(v["pos"]) == n and np.array_equal(g["part_offset"], v["part_offset"])
    assert [int(x) for x in np.diff(g["part_offset"])] == [len(vs) for vs, _ in parts]
    has = g["val_off"] >= 0
    if has.any():
        at = (v["line_offset"][None, :] + g["val_off"])[has]
        assert np.all(u[at - 1] == ord("="))
        assert np.all((g["val_off"] + g["val_len"])[has] <= np.broadcast_to(v["col_end"][:, 7][None, :], has.shape)[has])
    for q, (_, ty, _) in enumerate(rkeys):      # the per-key views
        W = int(g["key_width"][q])
        if ty in (U.INTEGER, U.FLOAT):
            assert g["values"][q].shape == ((n,) if W == 1 else (n, W))
        else:
            assert g["values"][q] is None
    assert st.ms_records > 0 or not n
    return g, v, rows


# ---- 1. fixtures
@pytest.mark.parametrize("split", [0, 500])          # one BGZF block: two partitions, the second empty
def test_test_vcf(golden, split):
    d = open(os.path.join(golden, "test.vcf.bgz"), "rb").read()
    g, v, rows = assert_info_parity(d, split, TEST_KEYS)
    assert g["flags"].shape == (6, 5) and g["key_width"].tolist() == [1, 1, 2, 1, 1, 1]
    assert (len(g["part_offset"]) - 1 == 2) == bool(split)
    assert g["values"][0].tolist() == [3, 3, 2, 3, 3] and g["values"][1][0] == 14
    assert g["values"][2][2].tolist() == [0.333, 0.667] and g["values"][2][0][0] == 0.5
    assert g["flags"][4].tolist() == [1, 0, 1, 0, 0] and g["flags"][3].tolist() == [0, 0, 3, 3, 3]


@pytest.mark.parametrize("split", [0, 64 * 1024])
@pytest.mark.parametrize("nkeys", [1, 13, 64])
def test_hiseq(golden, split, nkeys):
    d = open(os.path.join(golden, "HiSeq.10000.vcf.bgz"), "rb").read()
    keys = [b"DP"] if nkeys == 1 else HISEQ_KEYS + [b"K%d" % i for i in range(nkeys - 13)]
    g, v, rows = assert_info_parity(d, split, keys)
    assert g["flags"].shape == (nkeys, 9965) and (len(g["part_offset"]) - 1 > 2) == bool(split)
    assert int(g["values"][keys.index(b"DP")].sum()) == 897363 and g["n_float_host"] == 0
    if nkeys > 1:
        assert int((g["flags"][3] & 1).sum()) == 6617 and int((g["flags"][10] & 1).sum()) == 8348
    if nkeys == 64:     # keys no line holds: all zeros, width 1
        assert not g["flags"][13:].any() and not g["n_values"][13:].any() and np.all(g["val_off"][13:] == -1)
        assert g["key_width"].tolist() == [1] * 64 and g["key_type"][13:].tolist() == [U.STRING] * 51


def test_hiseq_keys_out_of_file_order_and_overrides(golden):
    d = open(os.path.join(golden, "HiSeq.10000.vcf.bgz"), "rb").read()
    keys = [(b"AF", U.STRING), b"SB", (b"NONE", U.INTEGER), b"DB", (b"AC", U.FLOAT), b"AN", (b"QD", U.FLAG)]
    g, v, rows = assert_info_parity(d, 0, keys)
    assert g["key_type"].tolist() == [4, 3, 2, 1, 3, 2, 1] and g["key_base"].tolist() == [-1, 0, 0, -1, 9965, 9965, -1]
    assert g["values"][0] is None and np.all(g["values"][2] == _lib.INFO_I_MISSING)
    assert float(g["values"][4].sum()) == 12802.0 and int(g["values"][5].sum()) == 19930


@pytest.mark.parametrize("intervals", [
    [("chr1", 2700000, 2800000)],
    [("chr1", 2700000, 2800000), ("chr1", 4000000, 4100000), ("chr1", 4050000, 4060000)],
    [("chr2", 1, 1000000)],
])
def test_hiseq_intervals(golden, intervals):
    d = open(os.path.join(golden, "HiSeq.10000.vcf.bgz"), "rb").read()
    tbi = open(os.path.join(golden, "HiSeq.10000.vcf.bgz.tbi"), "rb").read()
    g, v, rows = assert_info_parity(d, 128 * 1024, HISEQ_KEYS, intervals, tbi)
    assert (len(rows) > 0) == (intervals[0][0] == "chr1") and len(rows) < 9965


def test_test_vcf_intervals(golden):
    d = open(os.path.join(golden, "test.vcf.bgz"), "rb").read()
    tbi = T.whole_file_tabix(["20"], len(d))
    g, v, rows = assert_info_parity(d, 0, TEST_KEYS, [("20", 17000, 1200000)], tbi)
    assert v["pos"].tolist() == [17330, 1110696] and g["key_width"].tolist() == [1, 1, 2, 1, 1, 1]


# ---- 2. synthetic files: value counts of 1, 2 and 5; INFO columns either side of INFO_WAVE and of
# the wave's LDS slot; lines either side of VCF_LONG; ';', '=' and ',' on bytes 63 and 64 of a ballot
# window and a key across two windows; with samples and without; a block whose span does not stage
@pytest.mark.parametrize("case", range(len(C.SYNTH)))
def test_synthetic_files(case):
    (w, sites_only), text = C.SYNTH[case], synth_texts()[case]
    lines = [l for l in T.split_lines(text) if not l.startswith(b"#")]
    lens = [len(l.split(b"\t")[7]) for l in lines]
    assert {INFO_WAVE, INFO_WAVE + 1, INFO_WSLOT, INFO_WSLOT + 1} <= set(lens) and min(lens) < 100
    if not sites_only:     # a long line with a short INFO column; a line that alone outgrows the stage
        assert any(len(l) > VCF_LONG and n <= INFO_WAVE for l, n in zip(lines, lens)) and max(map(len, lines)) > 40960
    data = T.bgzf_text(text, block_u=3000, cuts=T.corner_cuts(text))
    for split in (0, max(200, len(data) // 3)):
        g, v, rows = assert_info_parity(data, split, C.KEYS)
        assert g["flags"].shape == (len(C.KEYS), len(lines)) and (len(g["part_offset"]) - 1 >= 2) == bool(split)
    assert int(g["key_width"].max()) == max(w, 2) and g["key_width"][C.KEYS.index(b"AF")] == w
    assert (g["flags"] & _lib.INFO_REPEATED).any()
    # the missing values fill the rows past each cell's count, and nothing else of an Integer block
    q = C.KEYS.index(b"AC")
    vals = g["values"][q].reshape(len(lines), -1)
    filled = np.arange(vals.shape[1])[None, :] >= g["n_values"][q][:, None]
    assert np.all(vals[filled] == _lib.INFO_I_MISSING)
    # explicit types: AF as String, keys without a header line as Integer and Float
    g, v, rows = assert_info_parity(data, 0, [(b"AF", U.STRING), (b"ZZ", U.INTEGER), (b"DB", U.INTEGER), b"DP",
                                              (b"LATE", U.FLOAT), (b"XX", U.INTEGER), (b"SOMATIC", U.FLOAT)])
    assert g["key_type"].tolist() == [4, 2, 2, 2, 3, 2, 3] and g["key_width"][1] == 2


def test_good_table():
    for header, strip in ((C.HEADER, b""), (C.SITES_HEADER, K.GT)):
        text = C.good_text(header).replace(strip, b"") if strip else C.good_text(header)
        g, v, rows = assert_info_parity(T.bgzf_text(text), 0, C.KEYS)
        assert g["n_float_host"] == 4 and g["key_width"].tolist() == [1, 5, 1, 1, 3, 1, 5, 1, 2, 1, 1, 1]
    assert_info_parity(T.bgzf_text(text), 0, C.KEYS[::-1] + [b"K%d" % i for i in range(52)])
    # the same columns in the wave kernel: a tail nobody asked for behind each
    long_text = C.HEADER + b"".join(C.iline(i + (b";" if i != b"." else b"X;") + b"CSQ=" + b"x|" * INFO_WAVE, pos=b"%d" % (10 + n)) + b"\n"
                                    for n, i in enumerate(C.GOOD))
    g, v, rows = assert_info_parity(T.bgzf_text(long_text), 0, C.KEYS)
    assert g["n_float_host"] == 4 and g["key_width"].tolist() == [1, 5, 1, 1, 3, 1, 5, 1, 2, 1, 1, 1]


# ---- 3. errors
NH = C.HEADER.count(b"\n")   # '#' lines before the first data line
TAIL = b";CSQ=" + b"x|" * INFO_WAVE


def _file(lines, header=C.HEADER):
    return T.bgzf_text(header + b"".join(l + b"\n" for l in lines))


def _error_of(c, data, keys=C.KEYS):
    c.text_open_bytes(data)
    with pytest.raises(_lib.DqError) as e:
        c.vcf_info(keys)
    assert e.value.code == _lib.DQ_EFORMAT
    n = len(c.vcf_read(_lib.VCF_EXPORT_FIELDS)["pos"])      # dq_vcf_read still succeeds
    assert n == len(c.text_read(True)["line_len"])
    with pytest.raises(_lib.DqError):
        c.vcf_info_run(keys)
    return str(e.value)


def _msg(k, key):
    return f"VCF line {k}: INFO {key.decode()}"


def test_every_error_in_the_thread_kernel():
    good = [C.iline(b"DP=5;AF=0.5", pos=b"%d" % (10 + i)) for i in range(20)]
    with _lib.Context() as c:
        for bad, key in C.BAD + C.ORDER:
            msg = _error_of(c, _file(good + [C.iline(bad)]))
            assert msg.endswith(_msg(NH + 20, key)), (bad, msg)


def test_every_error_in_the_wave_kernel():
    good = [C.iline(b"DP=5;AF=0.5" + TAIL, pos=b"%d" % (10 + i)) for i in range(9)]
    with _lib.Context() as c:
        for n, (bad, key) in enumerate(C.BAD + C.ORDER):
            info = bad + TAIL if n % 2 else TAIL[1:] + b";" + bad        # in front of the tail and behind it
            msg = _error_of(c, _file(good + [C.iline(info)]))
            assert msg.endswith(_msg(NH + 9, key)), (bad, msg)


def test_first_offender_wins():
    good = [C.iline(b"DP=5;AF=0.5", pos=b"%d" % (10 + i)) for i in range(300)]
    bad_af, bad_dp, bad_mq = C.iline(b"AF=1,,2"), C.iline(b"DP=x"), C.iline(b"DP=1;MQ=--1" + TAIL)
    with _lib.Context() as c:
        # two bad lines: the lower one, whatever its key's index and its kernel
        assert _error_of(c, _file(good[:7] + [bad_af] + good[7:280] + [bad_dp] + good[280:])).endswith(_msg(NH + 7, b"AF"))
        assert _error_of(c, _file(good[:7] + [bad_mq] + good[7:280] + [bad_dp] + good[280:])).endswith(_msg(NH + 7, b"MQ"))
        assert _error_of(c, _file([bad_dp] + good + [bad_mq])).endswith(_msg(NH, b"DP"))
        # two bad keys in one line: the lowest index in keys, wherever the pieces stand
        for tail in (b"", TAIL):
            two = C.iline(b"MQ=x;AF=y;AC=z" + tail)
            assert _error_of(c, _file(good + [two])).endswith(_msg(NH + 300, b"AF"))
            assert _error_of(c, _file(good + [two]), [b"AC", b"MQ", b"AF"]).endswith(_msg(NH + 300, b"AC"))
        # keys that were not asked for are not validated
        c.text_open_bytes(_file(good + [bad_dp]))
        assert c.vcf_info([b"AF"])["flags"].shape == (1, 301)
        # the site decode's errors come first, unchanged
        c.text_open_bytes(_file(good[:3] + [bad_dp, K.line(pos=b"x")]))
        with pytest.raises(_lib.DqError, match=f"VCF line {NH + 4}: POS"):
            c.vcf_info(C.KEYS)


def test_bad_value_outside_every_interval_is_not_reported():
    lines = [C.iline(b"DP=%d;AF=0.5,0.25" % i, pos=b"%d" % (100 + i)) for i in range(400)]
    bad = C.iline(b"DP=x", pos=b"90000")
    data = T.bgzf_text(C.HEADER + b"\n".join(lines + [bad]) + b"\n", block_u=8000)
    tbi = T.whole_file_tabix(["chr1", "chr2", "chrM"], len(data))
    g, v, rows = assert_info_parity(data, 0, C.KEYS, [("chr1", 150, 250)], tbi)      # POS 100 .. 499 and 90000
    assert v["pos"].tolist() == list(range(150, 251)) and g["values"][0].tolist() == list(range(50, 151))
    with _lib.Context() as c:                                                        # inside an interval it is
        c.text_open_bytes(data)
        c.text_set_index(tbi)
        c.text_set_intervals([("chr1", 150, 250), ("chr1", 89999, 90001)])
        with pytest.raises(_lib.DqError) as e:
            c.vcf_info(C.KEYS)
        assert str(e.value).endswith(_msg(NH + 400, b"DP"))
        assert len(c.vcf_read(_lib.VCF_EXPORT_FIELDS)["pos"]) == 102


# ---- 4. Float texts the host converts
@pytest.mark.parametrize("tail", [b"", TAIL])
def test_float_texts_the_host_converts(tail):
    texts = [b"1e-30", b"12345678901234567", b".5", b"0.1234567890123456", b"1e400", b"-.25"]
    lines = [C.iline(b"DP=1;AF=0.5," + t + b";MQ=" + t + tail, pos=b"%d" % (5 + i)) for i, t in enumerate(texts)]
    lines.append(C.iline(b"AF=0.25;MQ=12.5" + tail))
    g, v, rows = assert_info_parity(_file(lines), 0, C.KEYS)
    assert g["n_float_host"] == 2 * len(texts)
    assert g["values"][1][:6, 1].tolist() == [float(t) for t in texts] == g["values"][5][:6].tolist()
    assert g["values"][5][6] == 12.5 and g["values"][1][6].view(np.uint64).tolist() == [0x3fd0000000000000, _lib.INFO_F_MISSING_BITS]


# ---- 5. edges
def test_dot_column_and_header_only_file():
    g, v, rows = assert_info_parity(_file([C.iline(b".")] * 3), 0, C.KEYS)
    assert not g["flags"].any() and g["key_width"].tolist() == [1] * len(C.KEYS) and len(g["ival"]) == 3 * 3
    g, v, rows = assert_info_parity(T.bgzf_text(C.HEADER), 0, C.KEYS)
    assert g["flags"].shape == (len(C.KEYS), 0) and g["key_width"].tolist() == [1] * len(C.KEYS)
    assert len(g["ival"]) == len(g["fval"]) == 0 and g["values"][0].shape == (0,)


def test_other_contexts_and_bad_key_lists_are_refused(golden):
    import samcases

    def refused(c, keys=(b"DP",)):
        for call in (c.vcf_info, c.vcf_info_run):
            with pytest.raises(_lib.DqError) as e:
                call(list(keys))
            assert e.value.code == _lib.DQ_EINVAL
    with _lib.Context() as c:
        refused(c)                                                   # no open file
        c.open_bytes(open(os.path.join(golden, "1.bam"), "rb").read())
        refused(c)
        c.sam_open_bytes(samcases.HEADER + samcases.good_lines()[0] + b"\n")
        refused(c)
        c.text_open_bytes(open(os.path.join(golden, "test.vcf.bgz"), "rb").read())
        for keys in ([], [b"K%d" % i for i in range(65)], [b""], [b"A;B"], [b"A=B"], [b"A,B"], [b"A\tB"], [b"A B"],
                     [b"DP", b"AF", b"DP"], [(b"DP", 5)], [(b"DP", -1)]):
            refused(c, keys)
        assert c.vcf_info([b"DP"])["values"][0].tolist() == [14, 11, 10, 13, 9]


def test_read_and_genotypes_are_unchanged_after_info(golden):
    d = open(os.path.join(golden, "test.vcf.bgz"), "rb").read()
    with _lib.Context() as c:
        c.text_open_bytes(d)
        v0, g0 = c.vcf_read(_lib.VCF_EXPORT_SITES), c.vcf_genotypes()
    with _lib.Context() as c:
        c.text_open_bytes(d)
        i1 = c.vcf_info(TEST_KEYS)
        v1, g1 = c.vcf_read(_lib.VCF_EXPORT_SITES), c.vcf_genotypes()
        i2 = c.vcf_info([b"AF"])                                     # another key list on the same context
        t = c.text_read(True)
    for a, b in ((v0, v1), (g0, g1)):
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k], k
    assert np.array_equal(i2["values"][0], i1["values"][2], equal_nan=True) and len(t["line_len"]) == 5


def test_run_stats(golden):
    d = open(os.path.join(golden, "HiSeq.10000.vcf.bgz"), "rb").read()
    with _lib.Context(split_size=128 * 1024) as c:
        c.text_open_bytes(d)
        v = c.vcf_run()
        g = c.vcf_info_run(HISEQ_KEYS)
        b = c.vcf_info(HISEQ_KEYS)                  # the columns of the run, no second decode needed
    assert (g.n_records, g.n_partitions, g.digest) == (v.n_records, v.n_partitions, v.digest)
    assert g.ms_records > v.ms_records > 0 and g.ms_total > v.ms_total and b["flags"].shape == (13, 9965)


def test_storage_info(golden, tmp_path):
    import shutil
    from disq_amd.storage import HtsjdkVariantsRddStorage
    p = str(tmp_path / "test.vcf.bgz")
    shutil.copy(os.path.join(golden, "test.vcf.bgz"), p)
    st = HtsjdkVariantsRddStorage.makeDefault()
    with pytest.raises(ValueError):
        st.read(p, info=["DP"])
    plain = st.read(p, decode=True)
    assert plain.getInfo() is None
    rdd = st.read(p, decode=True, info=["DP", "AF", ("DB", _lib.INFO_AUTO)])
    parts = rdd.getInfo()
    assert len(parts) == rdd.getVariants().getNumPartitions() == 1 and len(parts[0]) == 5
    assert rdd.getVariants().collect() == plain.getVariants().collect()
    ip = parts[0]
    assert ip.keys == [b"DP", b"AF", b"DB"] and ip.values[0].tolist() == [14, 11, 10, 13, 9] and ip.values[2] is None
    fl, af = ip.get("AF")
    assert af.shape == (5, 2) and af[2].tolist() == [0.333, 0.667] and fl.tolist() == [3, 3, 3, 0, 0]
    assert ip.get(b"DB")[0].tolist() == [1, 0, 1, 0, 0]
