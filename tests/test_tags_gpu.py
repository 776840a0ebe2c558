"""GPU parity of the aux tag decode (dq_tags): the columns of Context.tags
against the oracle tests/tagutil.py applied to the record bytes of the oracle's partitions
(oracle/oracle.py, as tests/test_gpu_parity.py obtains them), array for array; the error of every
bad aux region of tests/tagcases.py with its exact message, in both walk paths; hand-placed streams
around the block size and the slot size of dq_tags.hip."""
import bisect
import functools
import os
import re

import numpy as np
import pytest

from disq_amd import _lib
from disq_amd.storage import HtsjdkReadsRddStorage, HtsjdkReadsTraversalParameters, Interval
from oracle import oracle as O

import baiutil
import bamutil as B
import reccases as R
import samutil as S
import tagcases as C
import tagutil as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TAGS = open(os.path.join(ROOT, "disq_amd", "csrc", "dq_tags.hip")).read()
TAG_SLOT = int(re.search(r"TAG_SLOT = (\d+);", _TAGS).group(1))
HDR = R.header([("chr1", 100_000_000)])
FIXTURE_KEYS = [(b"NM", U.INT), (b"AS", U.INT), (b"RG", U.STRING), (b"MD", U.ANY), (b"XS", U.ANY), (b"MC", U.STRING),
                (b"OQ", U.STRING), (b"XT", U.ANY), (b"X0", U.INT), (b"SM", U.INT)]
ARRAYS = ("flags", "vtype", "subtype", "val_off", "val_len", "key_type", "key_base", "val")


def record_bytes_of(bam):
    """voffset, block_size -> the record's bytes in the decompressed stream."""
    pos, uoff, u = baiutil._blocks(bam)

    def f(v, bs):
        j = bisect.bisect_left(pos, int(v) >> 16)
        assert pos[j] == int(v) >> 16
        a = uoff[j] + (int(v) & 0xffff)
        return bytes(u[a:a + 4 + int(bs)])
    return f


def oracle_rows(bam, split=0, traversal=None, bai=None):
    """(the records' bytes of every oracle partition in order, the partitions' bounds)."""
    parts = O.OracleBam(bam).read_partitions(split, traversal=traversal, bai=bai)
    rb = record_bytes_of(bam)
    recs, bounds = [], [0]
    for p in parts:
        recs += [rb(v, bs) for v, bs in zip(p["voffset"], p["block_size"])]
        bounds.append(len(recs))
    return recs, bounds


def assert_columns(g, recs, keys, bounds=None):
    rows, first = U.decode_records(recs, keys)
    assert first is None, first
    want = U.want_arrays(rows, keys)
    for k in ARRAYS:
        assert np.array_equal(g[k], want[k]), k
    if bounds is not None:
        assert g["part_offset"].tolist() == bounds
    for q, (vid, ty) in enumerate(U.norm_keys(keys)):
        v = g["values"][q]
        if ty in (U.ANY, U.STRING):
            assert v is None
        else:
            at = int(want["key_base"][q])
            assert v.view(np.uint8 if ty == U.CHAR else np.uint32).astype(np.uint32).tolist() == \
                want["val"][at:at + len(recs)].tolist()
            assert v.dtype == {U.FLOAT: np.float32, U.CHAR: np.uint8}.get(ty, v.dtype)


def gpu_tags(bam, keys, split=0, traversal=None, bai=None):
    with _lib.Context(split_size=split) as c:
        c.open_bytes(bam)
        if bai is not None:
            c.set_index(bai)
        return c.tags(keys, traversal=traversal)


# ------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def bam1(golden):
    return open(os.path.join(golden, "1.bam"), "rb").read()


@pytest.mark.parametrize("split", [0, 14146])
def test_1bam(bam1, split, stage):
    recs, bounds = oracle_rows(bam1, split)
    if split:
        assert len(recs) > len(oracle_rows(bam1, 0)[0])    # records duplicated across a split boundary
    g = gpu_tags(bam1, FIXTURE_KEYS, split)
    assert_columns(g, recs, FIXTURE_KEYS, bounds)
    assert g["flags"].any()


def test_hiseq_part(golden):
    d = open(os.path.join(golden, "hiseq_part-r-00000.bam"), "rb").read()
    recs, bounds = oracle_rows(d, 40000)
    assert_columns(gpu_tags(d, FIXTURE_KEYS, 40000), recs, FIXTURE_KEYS, bounds)


def test_test_sam(golden):
    text = open(os.path.join(golden, "test.sam"), "rb").read()
    names = S.sam_header_to_bam(text)[1]
    recs = [S.sam_line_to_bam_record(v, names) for _, v in S.text_lines(text) if not v.startswith(b"@")]
    keys = FIXTURE_KEYS + [(b"XX", U.ANY)]
    with _lib.Context() as c:
        c.sam_open_bytes(text)
        g = c.tags(keys)
        b = c.sam_read(with_raw=True)
        with pytest.raises(_lib.DqError) as e:
            c.tags(keys, traversal=(None, True))
        assert e.value.code == _lib.DQ_EINVAL
    assert_columns(g, recs, keys, b["part_offset"].tolist())
    assert len(recs) == 2


@pytest.fixture(scope="module")
def anysam():
    from disq_amd import synth
    return synth.generate(1000, shape=synth.ANYSAM, bai=True)


@pytest.mark.parametrize("ivs,unplaced", [([("chr21", 5000, 9999), ("chr21", 20000, 22999)], False),
                                          ([("chr21", 5000, 9999), ("chr21", 20000, 22999)], True),
                                          (None, True)])
def test_interval_traversal(anysam, ivs, unplaced):
    ob = O.OracleBam(anysam.bam)
    conv = None if ivs is None else [(ob.ref_index(c), s, e) for c, s, e in ivs]
    tr = (conv, unplaced)
    recs, bounds = oracle_rows(anysam.bam, 8000, traversal=tr, bai=anysam.bai)
    keys = [(b"NM", U.INT), (b"RG", U.STRING), (b"AS", U.ANY), (b"MD", U.STRING)]
    with _lib.Context(split_size=8000) as c:
        c.open_bytes(anysam.bam)
        c.set_index(anysam.bai)
        g = c.tags(keys, traversal=tr)
        b = c.read(with_raw=False, traversal=tr)
    assert len(recs) > 0 and len(b["voffset"]) == len(recs)
    assert g["part_offset"].tolist() == b["part_offset"].tolist()
    assert_columns(g, recs, keys, bounds)


# ------------------------------------------------------------------ hand-placed streams
@pytest.fixture(params=[None, "0"], ids=["slot", "memory"])
def stage(request, monkeypatch):
    """The two walk paths (dq_tags.hip reads DQ_TAGS_STAGE at every launch): a copy of the aux
    region in the thread's LDS slot where it fits, and every record walked in memory."""
    if request.param is None:
        monkeypatch.delenv("DQ_TAGS_STAGE", raising=False)
    else:
        monkeypatch.setenv("DQ_TAGS_STAGE", request.param)
    return request.param


def bam_of(recs, level=1):
    lay = R.layout(HDR, recs)
    return B.bgzf(lay.stream, level), lay


def lead(n=12):
    """Plain records in front, so that Disq's ten-record start check sees good ones."""
    return [C.rec_of(C.NM + C.RG, 1000 + i) for i in range(n)]


@functools.lru_cache(maxsize=None)
def table_bam():
    recs = lead() + [C.rec_of(a, i) for i, a in enumerate(C.GOOD)]
    return recs, bam_of(recs)[0]


@pytest.mark.parametrize("keys", [C.KEYS1, C.KEYS, C.KEYS64], ids=["1", "13", "64"])
def test_good_table(keys, stage):
    recs, bam = table_bam()
    assert_columns(gpu_tags(bam, keys), recs, keys, [0, len(recs)])


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_record_counts(n, stage):
    recs = C.synth_records(n, [60, 0, 90, 33], seed=n)
    bam, _ = bam_of(recs)
    assert_columns(gpu_tags(bam, C.KEYS), recs, C.KEYS, [0, n])


def test_no_records_and_an_empty_partition():
    g = gpu_tags(B.bgzf(HDR, 1), C.KEYS)
    assert g["flags"].shape == (len(C.KEYS), 0) and len(g["val"]) == 0
    recs = C.synth_records(300, [60], seed=5, l_seq=101)
    bam, _ = bam_of(recs)
    with _lib.Context(split_size=3000) as c:     # several splits start inside one BGZF block: empty partitions
        c.open_bytes(bam)
        b = c.read(with_raw=False)
        g = c.tags(C.KEYS)
    rows, bounds = oracle_rows(bam, 3000)
    assert g["part_offset"].tolist() == b["part_offset"].tolist() == bounds
    assert_columns(g, rows, C.KEYS)


def test_aux_lengths_around_the_constants(stage):
    """Aux regions of TAG_SLOT - 1, TAG_SLOT and TAG_SLOT + 1 bytes, one far larger than a slot
    between short ones, and a Z around the word scan's step at every alignment."""
    lens = [40, TAG_SLOT - 1, TAG_SLOT, TAG_SLOT + 1, 50, 70000, 60, 2 * TAG_SLOT, 0, 4]
    recs = lead() + C.synth_records(3 * len(lens), lens, seed=9)
    recs += [C.rec_of(C.z(b"XZ", b"w" * k) + C.NM, k, l_seq=1 + k % 3) for k in range(0, 40)]
    bam, _ = bam_of(recs)
    assert_columns(gpu_tags(bam, C.KEYS), recs, C.KEYS, [0, len(recs)])


# ------------------------------------------------------------------ errors
def error_of(bam, keys, **kw):
    with pytest.raises(_lib.DqError) as e:
        gpu_tags(bam, keys, **kw)
    return e.value.code, str(e.value)


@functools.lru_cache(maxsize=None)
def bad_bams():
    """One file per bad aux region: good records, the bad one, good ones, then a second bad record
    (the lowest row must win)."""
    out = []
    cases = C.BAD + C.MISMATCH + [(a, None) for a in C.truncations()]
    for i, (aux, what) in enumerate(cases):
        recs = lead() + C.synth_records(3 + i % 5, [60, 0], seed=i) + [C.rec_of(aux, i)] + lead(3) + \
            [C.rec_of(b"XQ?", 7)]
        out.append((recs, bam_of(recs)[0]))
    return out


def test_every_error_of_the_table(stage):
    seen = set()
    with _lib.Context() as c:
        for recs, bam in bad_bams():
            rows, first = U.decode_records(recs, C.KEYS)
            assert first is not None
            c.open_bytes(bam)
            with pytest.raises(_lib.DqError) as e:
                c.tags(C.KEYS)
            msg = str(e.value)
            assert e.value.code == _lib.DQ_EFORMAT and msg.endswith(f"record {first[0]}: {first[1]}"), (msg, first)
            seen.add(first[1])
    assert {w for _, w in C.BAD + C.MISMATCH} <= seen


def test_fields_error_and_the_lowest_row(stage):
    recs = lead() + [C.fields_records()[0]] + lead(2) + [C.rec_of(b"NMC")]
    code, msg = error_of(bam_of(recs)[0], C.KEYS1)
    assert code == _lib.DQ_EFORMAT and msg.endswith("record 12: fields")
    recs = lead() + [C.rec_of(b"NMC")] + [C.fields_records()[0]]
    code, msg = error_of(bam_of(recs)[0], C.KEYS1)
    assert msg.endswith("record 12: tag NM")


def test_einval_cases(bam1, golden):
    with _lib.Context() as c:
        for call in (lambda: c.tags(["NM"]), lambda: c.tags_run(["NM"])):
            with pytest.raises(_lib.DqError) as e:
                call()
            assert e.value.code == _lib.DQ_EINVAL      # no open file
        c.open_bytes(bam1)
        for keys in ([], C.KEYS64 + [b"QQ"], [b"N"], [b"NMX"], [b"1M"], [b"N-"], [b"NM", b"NM"], [(b"NM", 5)],
                     [(b"NM", -1)]):
            assert U.keys_refused(keys) is not None
            with pytest.raises(_lib.DqError) as e:
                c.tags(keys)
            assert e.value.code == _lib.DQ_EINVAL, keys
        assert c.tags(["NM"])["flags"].shape[1] == len(c.read(with_raw=False)["voffset"])
    vcf = open(os.path.join(golden, "test.vcf"), "rb").read()
    with _lib.Context() as c:
        c.text_open_bytes(B.bgzf(vcf, 1))
        with pytest.raises(_lib.DqError) as e:
            c.tags(["NM"])
        assert e.value.code == _lib.DQ_EINVAL


# ------------------------------------------------------------------ the context afterwards
def test_repeatable_and_the_context_reads_as_before(bam1):
    with _lib.Context(split_size=40000) as c:
        c.open_bytes(bam1)
        b0 = c.read(with_raw=True)
        n0, _ = c.sam_write_resident()
        t0 = bytes(c.sam_write_fetch(n0))
        g1 = c.tags(FIXTURE_KEYS)
        st = c.tags_run(FIXTURE_KEYS)
        g2 = c.tags(FIXTURE_KEYS)
        b1 = c.read(with_raw=True)
        n1, _ = c.sam_write_resident()
        t1 = bytes(c.sam_write_fetch(n1))
        g3 = c.tags(FIXTURE_KEYS)
    for k in ARRAYS + ("part_offset",):
        assert np.array_equal(g1[k], g2[k]) and np.array_equal(g1[k], g3[k]), k
    assert st.n_records > 0 and st.ms_records > 0
    for k in ("voffset", "hash", "raw_offset", "raw", "part_offset", "part_digest"):
        assert np.array_equal(b0[k], b1[k]), k
    assert t0 == t1 and len(t0) > 0
    # the spans point at the same bytes in the raw export
    raw, ro = b1["raw"], b1["raw_offset"]
    q = [k for k, _ in FIXTURE_KEYS].index(b"RG")
    rows = np.nonzero(g1["flags"][q])[0]
    assert len(rows) > 0
    for k in rows[:200]:
        a = int(ro[k]) + int(g1["val_off"][q, k])
        ln = int(g1["val_len"][q, k])
        assert bytes(raw[a - 3:a]) == b"RGZ" and raw[a + ln] == 0 and 0 not in raw[a:a + ln]
    q = [k for k, _ in FIXTURE_KEYS].index(b"NM")
    for k in np.nonzero(g1["flags"][q])[0][:200]:
        a = int(ro[k]) + int(g1["val_off"][q, k])
        ln = int(g1["val_len"][q, k])
        assert bytes(raw[a - 3:a - 1]) == b"NM" and raw[a - 1] == g1["vtype"][q, k]
        assert int.from_bytes(bytes(raw[a:a + ln]), "little", signed=chr(raw[a - 1]).islower()) == \
            int(g1["values"][q][k])


def test_storage_layer(tmp_path, golden, bam1):
    p = tmp_path / "a.bam"
    p.write_bytes(bam1)
    st = HtsjdkReadsRddStorage.makeDefault().splitSize(40000)
    rdd = st.read(str(p), tags=[("NM", U.INT), ("RG", U.STRING)]).getReads()
    recs, bounds = oracle_rows(bam1, 40000)
    parts = rdd.partitions
    assert len(parts) == len(bounds) - 1
    nm = rdd.tag("NM")
    assert len(nm) == len(parts)
    rows, _ = U.decode_records(recs, [(b"NM", U.INT), (b"RG", U.STRING)])
    for i, t in enumerate(nm):
        lo, hi = bounds[i], bounds[i + 1]
        assert t["flags"].tolist() == [r[0]["flags"] for r in rows[lo:hi]]
        assert [int(v) for v in t["values"]] == [r[0]["val"] for r in rows[lo:hi]]
    rg = rdd.tag("RG")
    assert rg[0]["values"] is None and rg[0]["val_off"].tolist() == [r[1]["val_off"] for r in rows[:bounds[1]]]
    with pytest.raises(KeyError):
        rdd.tag("AS")
    sam = os.path.join(golden, "test.sam")
    rdd = HtsjdkReadsRddStorage.makeDefault().read(sam, tags=["NM"]).getReads()
    assert sum(len(t["flags"]) for t in rdd.tag("NM")) == 2 and rdd.count() == 2
