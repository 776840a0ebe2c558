"""Test helper: SAM lines that exercise one rule of DESIGN.md section 13 each, shared by the CPU
test of dq_sam_core.h and the GPU tests of the SAM reader.  The oracle is samutil throughout."""
HEADER = b"@HD\tVN:1.5\tSO:unsorted\n@SQ\tSN:chr1\tLN:248956422\n@SQ\tSN:chr2\tLN:242193529\n" \
         b"@SQ\tSN:HLA-A*01:01\tLN:3503\n@RG\tID:L1\n"
BASE = b"q\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*"


def line(qname=b"r1", flag=0, rname=b"chr1", pos=100, mapq=30, cigar=b"4M", rnext=b"*", pnext=0,
         tlen=0, seq=b"ACGT", qual=b"IIII", tags=()):
    f = [qname, b"%d" % flag if isinstance(flag, int) else flag, rname,
         b"%d" % pos if isinstance(pos, int) else pos, b"%d" % mapq if isinstance(mapq, int) else mapq,
         cigar, rnext, b"%d" % pnext if isinstance(pnext, int) else pnext,
         b"%d" % tlen if isinstance(tlen, int) else tlen, seq, qual]
    return b"\t".join(f + list(tags))


INT_BOUNDS = (-2147483648, -32769, -32768, -129, -128, 127, 128, 255, 256, 32767, 32768, 65535,
              65536, 2147483647, 2147483648, 4294967295)


def good_lines():
    """One line per encoding rule; every one is a valid record."""
    out = [BASE]                                                   # POS 0 -> bin 4680, flag 0x4
    out += [BASE + b"\tXX:i:%d" % v for v in INT_BOUNDS]
    out += [BASE + b"\tXX:i:+7", BASE + b"\tXX:i:-0", BASE + b"\tXX:i:000000000000000000000012"]
    out += [BASE + b"\tXA:A:!", BASE + b"\tXA:A:~", BASE + b"\tXZ:Z:hello world", BASE + b"\tXZ:Z:",
            BASE + b"\tXH:H:", BASE + b"\tXH:H:0AF9", BASE + b"\tXF:f:3.25", BASE + b"\tXF:f:-1e-3",
            BASE + b"\tXF:f:7.038531e-26", BASE + b"\tXF:f:.5", BASE + b"\tXF:f:1e39"]
    vals = {"c": (-128, 127, 0, 5, -7, 100, -100), "C": (0, 255, 1, 2, 3, 4, 5),
            "s": (-32768, 32767, 0, 1, -1, 300, -300), "S": (0, 65535, 1, 2, 3, 4, 5),
            "i": (-2147483648, 2147483647, 0, 1, -1, 70000, -70000),
            "I": (0, 4294967295, 1, 2, 3, 4, 5)}
    for sub, v in vals.items():
        for n in (0, 1, 7):
            out.append(BASE + b"\tXB:B:" + sub.encode() + b"".join(b",%d" % x for x in v[:n]))
    fv = (b"1.5", b"-0.0", b"3e10", b"7.038531e-26", b"1e-46", b".25", b"+1e+0")
    for n in (0, 1, 7):
        out.append(BASE + b"\tXB:B:f" + b"".join(b"," + x for x in fv[:n]))
    out += [line(seq=b"*", qual=b"*", cigar=b"*"), line(seq=b"ACGTN", qual=b"*", cigar=b"5M"),
            line(seq=b"acgtn.=MRSVWYHKDB", qual=b"!" * 17, cigar=b"17M"),   # odd l_seq
            line(seq=b"acgtnN.=mrsvwyhkdb", qual=b"~" * 18, cigar=b"18M"),  # even l_seq
            line(seq=b"A", qual=b"*", cigar=b"1M"), line(seq=b"A", qual=b"5", cigar=b"1M"),
            line(rnext=b"="), line(rnext=b"*"), line(rnext=b"chr2", pnext=77, tlen=-5),
            line(rname=b"*", rnext=b"="), line(rname=b"HLA-A*01:01", rnext=b"chr1"),
            line(flag=4, pos=0), line(flag=0, pos=0, cigar=b"*"), line(flag=65535, mapq=255),
            line(pos=2147483647, cigar=b"*"), line(pos=2147483647, cigar=b"268435455M", pnext=2147483647),
            line(tlen=-2147483648), line(tlen=b"+2147483647"), line(pos=b"000100"),
            line(cigar=b"1M2I3D4N5S6H7P8=9X", seq=b"A" * 33, qual=b"*"),
            line(pos=16384, cigar=b"100000M", seq=b"*", qual=b"*"),         # a higher bin level
            line(cigar=b"".join(b"1M1I" for _ in range(150)), seq=b"C" * 300, qual=b"#" * 300),
            line(qname=b"n" * 254),
            line(tags=(b"NM:i:1", b"MD:Z:4", b"XA:A:x", b"XF:f:0.5", b"XB:B:s,1,2", b"XH:H:AB"))]
    return out


def bad_lines():
    """(line, the SamError.what it must give), one per error class."""
    return [
        (b"a\tb", "fields"), (b"", "fields"), (b"\t".join([b"x"] * 10), "fields"),
        (line(qname=b"n" * 255), "QNAME"), (line(qname=b""), "QNAME"),
        (line(flag=65536), "FLAG"), (line(flag=b"-1"), "FLAG"), (line(flag=b"0x10"), "FLAG"),
        (line(flag=b""), "FLAG"),
        (line(rname=b"chrX"), "RNAME"), (line(rname=b""), "RNAME"), (line(rname=b"chr"), "RNAME"),
        (line(pos=b"2147483648"), "POS"), (line(pos=b"-1"), "POS"), (line(pos=b"1.0"), "POS"),
        (line(mapq=256), "MAPQ"),
        (line(cigar=b"0M"), "CIGAR"), (line(cigar=b"4"), "CIGAR"), (line(cigar=b"M"), "CIGAR"),
        (line(cigar=b"4Z"), "CIGAR"), (line(cigar=b"268435456M"), "CIGAR"), (line(cigar=b""), "CIGAR"),
        (line(cigar=b"00000000004M"), "CIGAR"),
        (line(rnext=b"nope"), "RNEXT"),
        (line(pnext=b"x"), "PNEXT"), (line(pnext=b"2147483648"), "PNEXT"),
        (line(tlen=b"2147483648"), "TLEN"), (line(tlen=b"-2147483649"), "TLEN"),
        (line(tlen=b"--1"), "TLEN"),
        (line(seq=b"", qual=b"*"), "SEQ"), (line(seq=b"ACGJ"), "SEQ"), (line(seq=b"AC\xc4T"), "SEQ"),
        (line(seq=b"ACGT", qual=b"III"), "QUAL"), (line(seq=b"ACGT", qual=b"II I"), "QUAL"),
        (line(seq=b"*", qual=b"II"), "QUAL"),
        (BASE + b"\tXX:i:4294967296", "tag XX"), (BASE + b"\tXX:i:-2147483649", "tag XX"),
        (BASE + b"\tXX:i:", "tag XX"), (BASE + b"\tXX:i:1.5", "tag XX"),
        (BASE + b"\tXB:B:c,128", "tag XB"), (BASE + b"\tXB:B:C,-1", "tag XB"),
        (BASE + b"\tXB:B:c,", "tag XB"), (BASE + b"\tXB:B:", "tag XB"), (BASE + b"\tXB:B:q,1", "tag XB"),
        (BASE + b"\tXB:B:c1", "tag XB"), (BASE + b"\tXB:B:f,1.", "tag XB"),
        (BASE + b"\tXB:B:S,65536", "tag XB"),
        (BASE + b"\tXA:A:", "tag XA"), (BASE + b"\tXA:A:ab", "tag XA"), (BASE + b"\tXA:A: ", "tag XA"),
        (BASE + b"\tXH:H:ABC", "tag XH"), (BASE + b"\tXH:H:ab", "tag XH"),
        (BASE + b"\tXF:f:5.", "tag XF"), (BASE + b"\tXF:f:nan", "tag XF"), (BASE + b"\tXF:f:", "tag XF"),
        (BASE + b"\tXF:f:1e", "tag XF"), (BASE + b"\tXF:f:0x1p3", "tag XF"),
        (BASE + b"\tXQ:q:1", "tag XQ"), (BASE + b"\tXX", "tag XX"), (BASE + b"\tX", "tag X"),
        (BASE + b"\t", "tag "), (BASE + b"\tXX:i:1\t", "tag "), (BASE + b"\tXXi:i:1", "tag XX"),
        # the order of checks: the first failing one is reported
        (line(flag=b"x", rname=b"nope"), "FLAG"), (line(seq=b"ACGJ", cigar=b"0M"), "CIGAR"),
        (line(seq=b"ACGJ", qual=b"II I"), "SEQ"), (line(qual=b"II I", tags=(b"XX:i:x",)), "QUAL"),
        (line(seq=b"ACGT", qual=b"III", cigar=b"0M"), "QUAL"),
    ]
