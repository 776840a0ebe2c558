"""INFO columns for the INFO-decode tests: good columns that take every
rule's branches, bad ones with the id the error names, ORDER cases where two keys of a line fail
(the lowest index in KEYS is named, wherever its piece stands), and the synthetic files of the GPU
cases: value counts of 1, 2 and 5, INFO columns either side of the wave threshold and of the wave's
LDS slot, lines either side of the site decode's long-line threshold, ';', '=' and ',' on bytes 63
and 64 of a ballot window, a key split across two windows, a line that keeps its block from
staging."""
import random

import vcfcases as K

INFO_LINES = (b"##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Depth, all reads\">\n"
              b"##INFO=<ID=AF,Number=A,Type=Float,Description=\"Allele Frequency\">\n"
              b"##INFO=<ID=DB,Number=0,Type=Flag,Description=\"dbSNP membership, build 129\">\n"
              b"##INFO=<ID=H2,Number=0,Type=Flag,Description=\"HapMap2 membership\">\n"
              b"##INFO=<ID=AA,Number=1,Type=String,Description=\"Ancestral Allele\">\n"
              b"##INFO=<ID=MQ,Number=1,Type=Float,Description=\"RMS Mapping Quality\">\n"
              b"##INFO=<ID=AC,Number=A,Type=Integer,Description=\"Allele count\">\n"
              b"##INFO=<ID=CH,Number=1,Type=Character,Description=\"A character\">\n"
              b"##INFO=<ID=ZZ,Number=1,Type=Weird,Description=\"An unknown type: String\">\n"
              b"##INFO=<ID=DP,Number=1,Type=Float,Description=\"A repeated ID: the first line holds\">\n"
              b"##INFO=<Number=1,Type=Integer,Description=\"no ID\">\n"
              b"##INFO=<ID=LATE,Description=\"quoted commas are not honoured,Type=Integer,so this is one\",Type=Float>\n")
_H = K.HEADER.split(b"#CHROM")
HEADER = _H[0].replace(b"##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Depth, all reads\">\n", b"") \
    + INFO_LINES + b"#CHROM" + _H[1]
SITES_HEADER = K.SITES_HEADER.split(b"#CHROM")[0] + INFO_LINES + b"#CHROM" + K.SITES_HEADER.split(b"#CHROM")[1]
HEADER_TYPES = {b"DP": 2, b"AF": 3, b"DB": 1, b"H2": 1, b"AA": 4, b"MQ": 3, b"AC": 2, b"CH": 4, b"ZZ": 4,
                b"LATE": 2}

# NOHDR has no ##INFO line (String); END is the key the site decode reads as well
KEYS = [b"DP", b"AF", b"DB", b"H2", b"AA", b"MQ", b"AC", b"CH", b"ZZ", b"NOHDR", b"END", b"LATE"]


def iline(info, **kw):
    return K.line(info=info, **kw)


GOOD = [
    b"DP=14;AF=0.5;DB;H2;AA=T",
    b".",
    b"DP=.;AF=.;AA=.;DB=.",
    b"DP=;AF=;X=;AA=",
    b"DB=0;H2=0;NOHDR=0;DP=0",            # "DB=0" under a Flag line: absent; "0" elsewhere is a value
    b"DB=1;H2=00",
    b"DP;AF;AA",                          # no '=' under a typed line: present, no value
    b"DP4=1,2,3,4;DP=7;DPX;XDP=9",        # DP does not match DP4
    b"ENDX=5;END=7;EN=3",
    b"AF=0.1,.;AC=1,.,3",
    b"AF=NaN,-Infinity,Infinity,+Infinity,.",
    b"MQ=1e-30;AF=12345678901234567,.5",  # the host's Float texts
    b"DP=5;DP=bad;DP=7",                  # the first wins, the later ones only set the flag
    b"AF=1;X=2;AF=1,,2",
    b"DB=0;DB",
    b"H2;H2=0",
    b"AA=a,b,;CH=x;ZZ=1,2;NOHDR=q=r",
    b"DP=+7;AC=-2147483648,2147483647,-0,+0",
    b"DP=1;;AF=2",
    b"=5;DP=3",
    b"DP=3;",
    b"AF=1e400,-0,0e999,5.,100000000000000000000;MQ=0.000001",
    b"LATE=12;LATE",
    b"AC=1,2,3,4,5;AF=.,.,.",
    b"dp=1;Dp=2;dP=x",
]

BAD = [
    (b"DP=1.5", b"DP"), (b"DP=1,,2", b"DP"), (b"DP=1,", b"DP"), (b"DP=,1", b"DP"), (b"DP=,", b"DP"),
    (b"DP=2147483648", b"DP"), (b"DP=x", b"DP"), (b"DP=1e3", b"DP"), (b"DP=..", b"DP"),
    (b"AF=nan", b"AF"), (b"AF=inf", b"AF"), (b"AF=Infinit", b"AF"), (b"AF=1,,2", b"AF"), (b"AF=1,", b"AF"),
    (b"AF=NaN,", b"AF"), (b"AF=1e", b"AF"), (b"AF=0x1p3", b"AF"), (b"AF=1.5f", b"AF"), (b"AF=-NaN", b"AF"),
    (b"AC=1;MQ=--1", b"MQ"), (b"AC=1,.x", b"AC"), (b"DB;LATE=1.5", b"LATE"), (b"X=1;MQ=Infinity1;Y", b"MQ"),
]

ORDER = [
    (b"AF=bad;DP=bad", b"DP"),
    (b"MQ=x;AC=y;AF=z", b"AF"),
    (b"LATE=x;AC=1,", b"AC"),
]


def good_text(header=None):
    return (header or HEADER) + b"".join(iline(i, pos=b"%d" % (10 + n)) + b"\n" for n, i in enumerate(GOOD))


# ---- synthetic files
_VALS = {b"DP": lambda r, w: b"%d" % r.randrange(0, 500),
         b"AC": lambda r, w: b",".join(r.choice([b".", b"%d" % r.randrange(-9, 99)]) for _ in range(r.randint(1, w))),
         b"AF": lambda r, w: b",".join(r.choice([b".", b"0.%03d" % r.randrange(1000), b"1", b"1e-%d" % r.randrange(40),
                                                 b".25", b"NaN"]) for _ in range(r.randint(1, w))),
         b"MQ": lambda r, w: b"%d.%02d" % (r.randrange(70), r.randrange(100)),
         b"AA": lambda r, w: r.choice([b"T", b"acg", b".", b""]),
         b"CH": lambda r, w: b"x", b"ZZ": lambda r, w: b"1,2", b"NOHDR": lambda r, w: b"q",
         b"LATE": lambda r, w: b"%d" % r.randrange(9)}


def synth_info(r, w, target):
    """An INFO column of about `target` bytes: requested keys in random order, some left out, some
    repeated, Flags with and without values, keys nobody asked for between them (the filler that
    brings it to its length is an annotation piece, pipes and commas inside)."""
    pieces = []
    for key in r.sample(sorted(_VALS), r.randint(3, len(_VALS))):
        pieces.append(key + b"=" + _VALS[key](r, w))
    pieces += r.sample([b"DB", b"H2", b"DB=0", b"H2=1", b"XX=1,2", b"DP4=1,2,3,4", b"DPX", b"SOMATIC"], 3)
    r.shuffle(pieces)
    if r.random() < 0.5:                                              # a repeat, never validated
        pieces.append(r.choice(pieces).split(b"=")[0] + r.choice([b"=bad,,", b"", b"=1"]))
    have = len(b";".join(pieces))
    if target > have + 6:
        fill = b"".join(r.choice([b"A|", b"missense_variant|", b"ENST00000|", b"c.1A>T,", b"||", b"x=y|"])
                        for _ in range(target))[:target - have - 5]
        pieces.insert(r.randrange(len(pieces) + 1), b"CSQ=" + fill.rstrip(b","))
    return b";".join(pieces)


def edge_infos(tail):
    """';', '=' and ',' on bytes 63 and 64 of the INFO column (a ballot window's last byte and the
    next one's first), a key split across two windows, a key that ends the column at a window's
    edge; `tail` bytes of filler behind them."""
    out = []
    t = (b";CSQ=" + b"x|" * (tail // 2)) if tail else b""
    for at in (63, 64):
        out.append(b"PAD=" + b"x" * (at - 4) + b";DP=5;AF=0.5" + t)                 # ';' at `at`
        out.append(b"PAD=" + b"x" * (at - 7) + b";DP=5;AC=1,2" + t)                 # '=' at `at`
        out.append(b"PAD=" + b"x" * (at - 9) + b";AC=1,2;DP=7" + t)                 # ',' at `at`
        out.append(b"PAD=" + b"x" * (at - 7) + b";NOHDR=q;DB" + t)                  # a key across the edge
        out.append(b"PAD=" + b"x" * (at - 6) + b";H2" + (t and t + b";H2"))         # ends (or repeats) at the edge
    for o in out:
        assert len(o) >= 64
    return out


def synth_file(w, info_wave, vcf_long, wslot, sites_only=False, seed=0):
    """Lines of value counts up to w: INFO columns well below, just below, just above the wave
    threshold and past the wave's LDS slot; with samples, a line past vcf_long whose INFO is short,
    and a line long enough that its block's span does not stage."""
    r = random.Random(seed * 1000 + w)
    infos = [synth_info(r, w, t) for t in (0, 90, info_wave - 40, info_wave + 60, info_wave + 300, wslot + 500, 120)]
    infos += edge_infos(0)[:5] + edge_infos(info_wave)
    for n in (info_wave, info_wave + 1, wslot, wslot + 1):                        # exactly at the thresholds
        infos.append((b"DP=5;CSQ=" + b"x|" * n)[:n - 5] + b";AF=1")
    wide = b"AC=" + b",".join(b"%d" % i for i in range(w)) + b";AF=" + b",".join([b"0.5"] * w)
    infos += [wide, wide + b";CSQ=" + b"x|" * (info_wave // 2)]                   # exactly w values, both walks
    lines = []
    for n, info in enumerate(infos):
        rest = b"" if sites_only else K.GT
        if not sites_only and n == 1:
            rest = b"\tGT:X\t0/1:" + b"a" * (vcf_long + 50) + b"\t1/1:b"
        if not sites_only and n == 6:
            rest = b"\tGT:X\t0/1:" + b"a" * 42000 + b"\t1/1:b"
        lines.append(iline(info, pos=b"%d" % (100 + n), rest=rest))
    return (SITES_HEADER if sites_only else HEADER) + b"".join(l + b"\n" for l in lines)


SYNTH = [(1, False), (2, False), (5, False), (2, True)]
