"""The INFO oracle tests/vcfinfoutil.py pinned by hand: the five variants of
test.vcf, counts and sums over HiSeq.10000.vcf.bgz, the Flag quirks, key matching, missing
elements, Java's spellings of NaN and the infinities, the refused values, repeated keys."""
import gzip
import os
import struct

import numpy as np
import pytest

import vcfinfocases as C
import vcfinfoutil as U
from textutil import split_lines

HISEQ_KEYS = [b"AC", b"AF", b"AN", b"DB", b"DP", b"Dels", b"HRun", b"HaplotypeScore", b"MQ", b"MQ0", b"OQ", b"QD", b"SB"]


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def cells_of(info, keys=C.KEYS, header=C.HEADER):
    return U.info_decode_line(C.iline(info), U.resolve_keys(keys, U.info_header(header)))


def cell(info, key, **kw):
    keys = kw.pop("keys", C.KEYS)
    return cells_of(info, keys, **kw)[[k if isinstance(k, bytes) else k[0] for k in keys].index(key)]


def test_header_types():
    assert U.info_header(C.HEADER) == C.HEADER_TYPES
    rk = U.resolve_keys([b"DP", (b"AF", U.STRING), (b"DB", U.INTEGER), b"NOHDR", (b"NOHDR2", U.INTEGER)], C.HEADER_TYPES)
    assert rk == [(b"DP", U.INTEGER, False), (b"AF", U.STRING, False), (b"DB", U.INTEGER, True),
                  (b"NOHDR", U.STRING, False), (b"NOHDR2", U.INTEGER, False)]
    for bad in ([], [b"K%d" % i for i in range(65)], [b""], [b"A;B"], [b"A=B"], [b"A,B"], [b"A\tB"], [b"A B"],
                [b"DP", b"DP"], [(b"DP", 5)], [(b"DP", -1)]):
        with pytest.raises(ValueError):
            U.resolve_keys(bad, C.HEADER_TYPES)
    assert len(U.resolve_keys([b"K%d" % i for i in range(64)], {})) == 64


def test_test_vcf(golden):
    text = open(os.path.join(golden, "test.vcf"), "rb").read()
    hdr = U.info_header(text)
    assert hdr == {b"NS": U.INTEGER, b"DP": U.INTEGER, b"AF": U.FLOAT, b"AA": U.STRING, b"DB": U.FLAG, b"H2": U.FLAG}
    keys = [b"NS", b"DP", b"AF", b"AA", b"DB", b"H2"]
    rk, rows = U.decode_text(text, keys)
    assert len(rows) == 5 and all(e is None for _, _, e in rows)
    lines = [l for l in split_lines(text) if not l.startswith(b"#")]
    c = rows[0][1]
    assert [x["values"] for x in c[:3]] == [[3], [14], [bits(0.5)]]
    assert c[4]["flags"] == c[5]["flags"] == U.PRESENT and c[4]["val_off"] == -1 and c[3]["flags"] == 0
    c = rows[2][1]
    assert c[2]["values"] == [bits(0.333), bits(0.667)] and c[2]["n_values"] == 2
    assert c[3]["flags"] == 3 and lines[2][c[3]["val_off"]:c[3]["val_off"] + c[3]["val_len"]] == b"T"
    w, nhost = U.want_arrays([r for _, r, _ in rows], rk)
    assert w["key_width"].tolist() == [1, 1, 2, 1, 1, 1] and nhost == 0
    assert w["key_base"].tolist() == [0, 5, 0, -1, -1, -1] and len(w["ival"]) == 10 and len(w["fval"]) == 10
    assert w["fval"][2 * 2 + 1] == bits(0.667) and w["fval"][1] == U.F_MISSING_BITS


def test_hiseq_counts(golden):
    text = gzip.decompress(open(os.path.join(golden, "HiSeq.10000.vcf.bgz"), "rb").read())
    hdr = U.info_header(text)
    assert sorted(hdr) == sorted(HISEQ_KEYS) and len(hdr) == 13
    rk, rows = U.decode_text(text, HISEQ_KEYS)
    assert len(rows) == 9965 and all(e is None for _, _, e in rows)
    w, nhost = U.want_arrays([r for _, r, _ in rows], rk)
    present = {k: int((w["flags"][q] & U.PRESENT).sum()) for q, k in enumerate(HISEQ_KEYS)}
    assert present.pop(b"DB") == 6617 and present.pop(b"OQ") == 8348 and set(present.values()) == {9965}
    assert not (w["flags"] & U.REPEATED).any() and w["key_width"].tolist() == [1] * 13
    sums = {}
    for q, k in enumerate(HISEQ_KEYS):
        if rk[q][1] == U.INTEGER:
            v = w["ival"][w["key_base"][q]:][:9965].astype(np.int64)
            sums[k] = int(v[v != U.I_MISSING].sum())
    assert sums == {b"DP": 897363, b"AN": 19930, b"AC": 12802, b"HRun": 8245, b"MQ0": 70645}
    nfloat = sum(r[q]["n_values"] for _, r, _ in rows for q in range(13) if rk[q][1] == U.FLOAT)
    assert nfloat == 68138 and nhost == 0
    lens = [len(l.split(b"\t")[7]) for l in split_lines(text) if not l.startswith(b"#")]
    assert (min(lens), max(lens)) == (90, 115)


def test_flag_quirks():
    assert cell(b"DB=0", b"DB") == U.blank()                          # a Flag line and "0": not in the map
    assert cell(b"NOHDR=0", b"NOHDR")["flags"] == 3 and cell(b"DP=0", b"DP")["values"] == [0]
    assert cell(b"DB=0", b"DB", keys=[(b"DB", U.INTEGER)]) == U.blank()   # the header's type decides, not the override
    assert cell(b"DB=1", b"DB")["flags"] == 3 and cell(b"DB=00", b"DB")["flags"] == 3
    c = cell(b"DP", b"DP")                                            # no '=' under an Integer line
    assert (c["flags"], c["n_values"], c["val_off"], c["values"]) == (U.PRESENT, 0, -1, [])
    for info in (b"DP=", b"DP=."):
        c = cell(info, b"DP")
        assert (c["flags"], c["n_values"], c["values"]) == (U.PRESENT, 0, [])
        assert c["val_off"] == len(C.iline(b"")) - len(C.K.GT) + 3 and c["val_len"] == len(info) - 3
    assert cells_of(b"X=") == [U.blank()] * len(C.KEYS) == cells_of(b".")


def test_key_matching():
    assert cell(b"DP4=1,2,3,4;DPX;XDP=2", b"DP") == U.blank() and cell(b"DP4=1,2;DP=7", b"DP")["values"] == [7]
    assert cell(b"ENDX=5;XEND=4", b"END") == U.blank() and cell(b"ENDX=5;END=7", b"END")["flags"] == 3
    assert cell(b"dp=5", b"DP") == U.blank() and cell(b"=5;DP=3;", b"DP")["values"] == [3]


def test_values():
    assert cell(b"AF=0.1,.", b"AF")["values"] == [bits(0.1), U.F_MISSING_BITS]
    assert cell(b"AC=1,.,3", b"AC")["values"] == [1, U.I_MISSING, 3]
    v = cell(b"AF=NaN,-Infinity,Infinity,+Infinity", b"AF")["values"]
    assert v == [U.F_NAN_BITS, bits(float("-inf")), bits(float("inf")), bits(float("inf"))] and U.F_NAN_BITS != U.F_MISSING_BITS
    c = cell(b"MQ=1e-30;AF=12345678901234567,.5,0.25", b"AF")
    assert c["host"] == 2 and c["values"] == [bits(12345678901234567.0), bits(0.5), bits(0.25)]
    assert cell(b"MQ=1e-30", b"MQ")["host"] == 1
    s = cell(b"AA=a,b,", b"AA")
    assert (s["n_values"], s["values"], s["val_len"]) == (3, [], 4)
    assert cell(b"AF=0.5", b"AF", keys=[(b"AF", U.STRING)])["values"] == []
    assert cell(b"NOHDR=12", b"NOHDR", keys=[(b"NOHDR", U.INTEGER)])["values"] == [12]


@pytest.mark.parametrize("info,key", [(b"AF=nan", b"AF"), (b"DP=1,,2", b"DP"), (b"DP=1,", b"DP"), (b"DP=1.5", b"DP")] + C.BAD + C.ORDER)
def test_refused(info, key):
    with pytest.raises(U.InfoError) as e:
        cells_of(info)
    assert C.KEYS[e.value.q] == key


def test_good_table_and_repeats():
    rk, rows = U.decode_text(C.good_text(), C.KEYS)
    assert all(e is None for _, _, e in rows) and len(rows) == len(C.GOOD)
    c = cell(b"DP=5;DP=bad;DP=7", b"DP")                # the first wins, a bad later duplicate is no error
    assert c["flags"] == 7 and c["values"] == [5]
    assert cell(b"AF=1;X=2;AF=1,,2", b"AF")["flags"] == 7
    assert cell(b"DB=0;DB", b"DB")["flags"] == U.REPEATED and cell(b"H2;H2=0", b"H2")["flags"] == 5
    with pytest.raises(U.InfoError):
        cells_of(b"DP=bad;DP=5")
