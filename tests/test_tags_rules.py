"""The tag oracle tests/tagutil.py itself, pinned on hand-written records with literal expected
values (SAMv1 section 4.2.4), and the tables of tests/tagcases.py checked against what they claim."""
import struct

import pytest

import reccases as R
import tagcases as C
import tagutil as U


def rec(aux):
    # 36 + 3 name bytes + 1 cigar word + 2 seq bytes + 3 quals = 48: the aux region starts there
    return R.record(0, 7, b"ab\x00", [(3, 0)], 3, aux=aux)


def test_aux_region_of_a_hand_written_record():
    r = rec(b"NMC\x05")
    assert len(r) == 52 and U.aux_region(r) == (48, 52)
    assert U.aux_region(rec(b"")) == (48, 48)


def test_literal_cells():
    aux = (b"NMC\x05" + b"ASs\xb3\xff" + b"XSi\xc0\x1d\xfe\xff" + b"RGZgrp1\x00" + b"XFf\x00\x00\xc0\xbf" +
           b"XAAQ" + b"XHH1aE3\x00" + b"XBBS\x02\x00\x00\x00\x01\x00\x02\x00" + b"XII\x00\x00\x00\x80")
    keys = [("NM", U.INT), ("AS", U.INT), ("XS", U.INT), ("RG", U.STRING), ("XF", U.FLOAT), ("XA", U.CHAR),
            ("XH", U.ANY), ("XB", U.ANY), ("XI", U.INT), ("ZZ", U.INT)]
    c = U.decode_record(rec(aux), keys)
    assert c[0] == dict(flags=1, vtype=ord("C"), subtype=0, val_off=51, val_len=1, val=5)
    assert c[1] == dict(flags=1, vtype=ord("s"), subtype=0, val_off=55, val_len=2, val=0xffffffb3)     # -77
    assert c[2] == dict(flags=1, vtype=ord("i"), subtype=0, val_off=60, val_len=4, val=0xfffe1dc0)     # -123456
    assert c[3] == dict(flags=1, vtype=ord("Z"), subtype=0, val_off=67, val_len=4, val=0)
    assert c[4] == dict(flags=1, vtype=ord("f"), subtype=0, val_off=75, val_len=4, val=0xbfc00000)     # -1.5
    assert c[5] == dict(flags=1, vtype=ord("A"), subtype=0, val_off=82, val_len=1, val=ord("Q"))
    assert c[6] == dict(flags=1, vtype=ord("H"), subtype=0, val_off=86, val_len=4, val=0)
    assert c[7] == dict(flags=1, vtype=ord("B"), subtype=ord("S"), val_off=99, val_len=4, val=0)
    assert c[8] == dict(flags=1, vtype=ord("I"), subtype=0, val_off=106, val_len=4, val=0x80000000)
    assert c[9] == dict(flags=0, vtype=0, subtype=0, val_off=-1, val_len=0, val=0)


def test_first_occurrence_wins_and_the_cell_says_so():
    c = U.decode_record(rec(b"NMC\x05" + b"NMC\x09" + b"NMZx\x00"), [("NM", U.INT)])
    assert c[0] == dict(flags=5, vtype=ord("C"), subtype=0, val_off=51, val_len=1, val=5)


@pytest.mark.parametrize("aux,what", [
    (b"NM", "tag "), (b"NMC", "tag NM"), (b"RGZabc", "tag RG"), (b"XHHabc\x00", "tag XH"),
    (b"XHHag\x00", "tag XH"), (b"XBBq\x00\x00\x00\x00", "tag XB"), (b"XBBi\x01\x00\x00\x00abc", "tag XB"),
    (b"XQ?\x00", "tag XQ"), (b"NMZ5\x00", "tag NM type"), (b"RGA5", "tag RG type"),
    (b"NMC\x01" + b"RGA5" + b"XQ?", "tag RG type"), (b"NMC\x01" + b"XQ?" + b"RGA5", "tag XQ"),
])
def test_literal_errors(aux, what):
    with pytest.raises(U.TagError) as e:
        U.decode_record(rec(aux), [("NM", U.INT), ("RG", U.STRING)])
    assert e.value.what == what


def test_fields():
    for r in C.fields_records():
        with pytest.raises(U.TagError) as e:
            U.decode_record(r, ["NM"])
        assert e.value.what == "fields"
    short = bytearray(rec(b""))
    struct.pack_into("<i", short, 0, 31)
    with pytest.raises(U.TagError):
        U.aux_region(bytes(short))


def test_the_tables_are_what_they_claim():
    for aux in C.GOOD:
        assert U.decode_record(C.rec_of(aux), C.KEYS) is not None
    for aux, what in C.BAD + C.MISMATCH:
        with pytest.raises(U.TagError) as e:
            U.decode_record(C.rec_of(aux), C.KEYS)
        assert e.value.what == what, aux
    cut = C.truncations()
    bad = 0
    for aux in cut:
        try:
            U.decode_record(C.rec_of(aux), C.KEYS)
        except U.TagError:
            bad += 1
    assert len(cut) > 40 and bad >= len(cut) - 8    # a cut Z that ends in an earlier NUL is well formed
    types = {t[1] for aux in C.GOOD for t in U.walk(C.rec_of(aux))}
    assert types == {b"A", b"c", b"C", b"s", b"S", b"i", b"I", b"f", b"Z", b"H", b"B"}
    subs = {(t[2], t[4] // U.ELEM_SIZE[t[2]]) for aux in C.GOOD for t in U.walk(C.rec_of(aux)) if t[1] == b"B"}
    assert {(s, c) for s in (b"c", b"C", b"s", b"S", b"i", b"I", b"f") for c in (0, 1)} <= subs


def test_key_lists():
    assert U.keys_refused(C.KEYS) is None and U.keys_refused(C.KEYS1) is None and U.keys_refused(C.KEYS64) is None
    assert U.keys_refused([]) == "count" and U.keys_refused(C.KEYS64 + [b"QQ"]) == "count"
    for bad in (b"N", b"NMX", b"1M", b"N_", b""):
        assert U.keys_refused([bad]) == "id"
    assert U.keys_refused([b"NM", b"NM"]) == "twice"
    assert U.keys_refused([(b"NM", 5)]) == "type" and U.keys_refused([(b"NM", -1)]) == "type"


def test_synthetic_aux_lengths():
    import random
    r = random.Random(1)
    for n in [0, 4, 5, 17, 127, 128, 129, 500]:
        aux = C.synth_aux(r, n)
        assert len(aux) == n and U.decode_record(C.rec_of(aux), C.KEYS) is not None
