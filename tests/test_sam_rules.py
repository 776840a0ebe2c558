"""The SAM <-> BAM restatement of tests/samutil.py (the oracle of the GPU SAM reader), pinned on
the CPU: the golden BAM survives BAM -> SAM -> BAM byte for byte, the reference's test.sam encodes
to the fields written out here by hand, and floats are converted correctly rounded."""
import os
import struct

import pytest

import bamutil as B
import samutil as S


def test_1bam_round_trips_byte_exactly(golden):
    u = B.inflate_all(open(os.path.join(golden, "1.bam"), "rb").read())
    hdr = u[:B.header_len(u)]
    names = [n for n, _ in _refs(hdr)]
    spans = B.record_spans(u)
    assert len(spans) == 4917
    same = 0
    for p, n in spans:
        rec = u[p:p + n]
        same += S.sam_line_to_bam_record(S.bam_record_to_sam_line(rec, names), names) == rec
    assert same == 4917
    # the whole file as text: the header comes back too
    text = S.bam_to_sam_text(u)
    h, names2 = S.sam_header_to_bam(text)
    assert names2 == names and h == hdr
    assert [r for _, _, r in S.sam_records(text)] == [u[p:p + n] for p, n in spans]


def _refs(hdr):
    p = 8 + struct.unpack_from("<i", hdr, 4)[0]
    n = struct.unpack_from("<i", hdr, p)[0]
    p += 4
    out = []
    for _ in range(n):
        ln = struct.unpack_from("<i", hdr, p)[0]
        out.append((hdr[p + 4:p + 4 + ln - 1].decode(), struct.unpack_from("<i", hdr, p + 4 + ln)[0]))
        p += 8 + ln
    return out


def test_test_sam_fields(golden):
    text = open(os.path.join(golden, "test.sam"), "rb").read()
    h, names = S.sam_header_to_bam(text)
    assert names == ["chr21"] and _refs(h) == [("chr21", 62435964)]
    assert h[8:8 + struct.unpack_from("<i", h, 4)[0]] == text[:text.index(b"read_28833")]
    recs = S.sam_records(text)
    assert [k for k, _, _ in recs] == [4, 5]
    assert [o for _, o, _ in recs] == [text.index(b"read_28833"), text.index(b"read_28701")]
    r0, r1 = recs[0][2], recs[1][2]
    f0 = struct.unpack_from("<iiiBBHHHiiii", r0, 0)
    # block_size, refID, pos, l_read_name, mapq, bin, n_cigar, flag, l_seq, next_refID, next_pos, tlen
    assert f0 == (len(r0) - 4, 0, 28832, 22, 20, 4682, 3, 99, 35, 0, 28992, 195)
    assert r0[36:58] == b"read_28833_29006_6945\0"
    assert struct.unpack_from("<3I", r0, 58) == (10 << 4 | 0, 1 << 4 | 2, 25 << 4 | 0)
    tags0 = r0[58 + 12 + 18 + 35:]
    assert tags0 == (b"H0c\x00" + b"H1c\x00" + b"MFC\x82" + b"RGZL1\0" + b"Nmc\x01")
    f1 = struct.unpack_from("<iiiBBHHHiiii", r1, 0)
    assert f1 == (len(r1) - 4, 0, 28833, 22, 30, 4682, 1, 147, 35, 0, 28700, -168)
    assert struct.unpack_from("<I", r1, 58) == (35 << 4,)
    assert r1[58 + 4 + 18 + 35:] == b"H0c\x01" + b"H1c\x00" + b"MFc\x12" + b"RGZL2\0" + b"Nmc\x00"
    # the first bases and qualities: AGCT -> 1 4 2 8, '<' -> 27
    assert r0[70:72] == bytes([0x14, 0x28]) and r0[88] == ord("<") - 33


def test_float_is_correctly_rounded():
    # decimal -> double -> float gives 0x15ae43fe here; strtof gives the nearest float
    assert S.pack_float(b"7.038531e-26").hex() == "fd43ae15"
    assert S.pack_float(b"0.0123") == struct.pack("<f", 0.0123)
    with pytest.raises(ValueError):
        S.pack_float(b"5.")


def test_integer_tag_types_and_bin():
    names = ["chr1"]
    line = b"q\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*"
    rec = S.sam_line_to_bam_record(line, names)
    assert struct.unpack_from("<H", rec, 14)[0] == 4680  # pos == -1
    want = {-2147483648: b"i", -32769: b"i", -32768: b"s", -129: b"s", -128: b"c", 127: b"c",
            128: b"C", 255: b"C", 256: b"s", 32767: b"s", 32768: b"S", 65535: b"S", 65536: b"i",
            2147483647: b"i", 2147483648: b"I", 4294967295: b"I"}
    for v, t in want.items():
        rec = S.sam_line_to_bam_record(line + b"\tXX:i:%d" % v, names)
        assert rec[-(1 + {b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4}[t]):][:1] == t, v
    with pytest.raises(S.SamError, match="tag XX"):
        S.sam_line_to_bam_record(line + b"\tXX:i:4294967296", names)


def test_plain_text_partitions_rule():
    data = b"a\r\nbb\rc\n\nlast"
    lines = S.text_lines(data)
    assert lines == [(0, b"a"), (3, b"bb"), (6, b"c"), (8, b""), (9, b"last")]
    parts = S.plain_text_partitions(data, [(0, 2), (2, 3), (3, 8), (8, 13)])
    assert parts == [[(0, b"a")], [(3, b"bb")], [(6, b"c"), (8, b"")], [(9, b"last")]]
    assert S.plain_text_partitions(b"\xef\xbb\xbfx\n", [(0, 5)]) == [[(0, b"x")]]
