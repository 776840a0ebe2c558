"""VCF data lines for the genotype-decode tests: bad lines, at least two per
error class, with the class (and sample) the first failing check names; ORDER holds lines that fail
two checks; synth_text() makes small files of a given sample count whose cells are drawn from a
pool that takes every rule's branches."""
import random

import vcfcases as K


def header(S):
    names = b"".join(b"\tS%d" % i for i in range(S))
    return K.HEADER[:K.HEADER.index(b"#CHROM")] + b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT" + names + b"\n"


def gline(fmt, cells, **kw):
    return K.line(rest=b"\t" + fmt + b"".join(b"\t" + c for c in cells), **kw)


# (line, class, sample or None) of a file with K.HEADER: two samples, one ALT unless given
BAD = [
    (gline(b"GT", [b"0/1"]), "samples", None),                         # one column too few
    (gline(b"GT", [b"0/1", b"0/1", b"1/1"]), "samples", None),         # one too many
    (gline(b"GT", []), "samples", None),
    (gline(b"GT", [b"0/1", b"0/1", b""]), "samples", None),            # a trailing TAB is a column
    (gline(b"GQ:GT", [b"5:0/1", b"5:0/1"]), "FORMAT", None),           # GT second
    (gline(b"GT:DP:DP", [b"0/1:1:1", b"0/1:1:1"]), "FORMAT", None),    # a repeated key
    (gline(b"", [b"0/1", b"0/1"]), "FORMAT", None),                    # an empty FORMAT column
    (gline(b"GT:GQ:AD:GQ", [b"0/1", b"0/1"]), "FORMAT", None),
    (gline(b"GT:FT:FT", [b"0/1", b"0/1"]), "FORMAT", None),
    (gline(b"AD:DP:GT", [b"1", b"1"]), "FORMAT", None),
    (gline(b"GT", [b"0/1:5", b"0/1"]), "cell", 0),
    (gline(b"GT:GQ", [b"0/1:5", b"0/1:5:3"]), "cell", 1),
    (gline(b"GT:GQ", [b"0/1", b"0/1::"]), "cell", 1),
    (gline(b"GT", [b"2/0", b"0/1"]), "GT", 0),                          # an index above n_alt
    (gline(b"GT", [b"0/1", b"0/x"]), "GT", 1),                          # a non-number
    (gline(b"GT", [b"0/1", b"0/-1"]), "GT", 1),
    (gline(b"GT", [b"0/1.0", b"0/1"]), "GT", 0),
    (gline(b"GT", [b"0/1", b"0/ 1"]), "GT", 1),
    (gline(b"GT", [b"0/1", b"/".join([b"0"] * 256)]), "GT", 1),         # more than 255 tokens
    (gline(b"GT", [b"3|0", b"0/1"], alt=b"G,T"), "GT", 0),
    (gline(b"GT:GQ", [b"0/1:abc", b"0/1:5"]), "GQ", 0),
    (gline(b"GT:GQ", [b"0/1:5", b"0/1:"]), "GQ", 1),
    (gline(b"GT:GQ", [b"0/1:5", b"0/1:1e"]), "GQ", 1),
    (gline(b"GQ", [b"NaN", b"5"]), "GQ", 0),
    (gline(b"GT:DP", [b"0/1:3.0", b"0/1:3"]), "DP", 0),                 # htsjdk fails on 3.0 too
    (gline(b"GT:DP", [b"0/1:3", b"0/1:"]), "DP", 1),
    (gline(b"DP", [b"3", b"x"]), "DP", 1),
    (gline(b"GT:GQ:DP", [b"0/1:5:2147483648", b"0/1"]), "DP", 0),
]

# two failing checks: the earlier one in the order samples, FORMAT, then per cell left to right
# cell, GT, GQ, DP
ORDER = [
    (gline(b"GQ:GT", [b"0/1"]), "samples", None),                      # samples before FORMAT
    (gline(b"GT:GT", [b"0/x", b"0/1"]), "FORMAT", None),               # FORMAT before the cells
    (gline(b"GT:GQ", [b"0/x:1:2", b"0/1"]), "cell", 0),                # cell before GT
    (gline(b"GT:GQ:DP", [b"0/x:abc:y", b"0/1"]), "GT", 0),             # GT before GQ before DP
    (gline(b"GT:DP:GQ", [b"0/1:y:abc", b"0/1"]), "GQ", 0),             # GQ before DP whatever the key order
    (gline(b"GT:GQ:DP", [b"0/1:5:y", b"0/x"]), "DP", 0),               # the lower sample
    (gline(b"GT:GQ:DP", [b"0/1:5:1", b"0/1:abc:y"]), "GQ", 1),
]

# good lines of a file with K.HEADER that take the remaining branches
GOOD = [
    gline(b"GT:GQ:DP:FT:AD", [b"0/1:35:4:PASS:1,2", b"1|1:12.5:7:q10:3,4"]),
    gline(b"GT:GQ:DP:HQ", [b"0/0:41:3", b"./."]),                       # trailing values dropped
    gline(b"GQ:DP", [b"5:6", b".:."]),                                  # no GT key: flags without HAS_GT
    gline(b"GT", [b"", b"/"]),                                          # ploidy 0
    gline(b"GT", [b".", b"0"]),                                         # ploidy 1
    gline(b"GT", [b"0\\1", b"0|1|0"]),                                  # '\\' separates; ploidy 3
    gline(b"GT", [b"+1/-0", b"01/001"]),                                # Integer.valueOf texts
    gline(b"GT:GQ", [b"0/1:-1", b"0/1:-1.0"]),                          # -1 is missing, -1.0 is a value
    gline(b"GT:GQ", [b"0/1:0.5", b"0/1:-0.5"]),                         # ties toward +infinity
    gline(b"GT:GQ", [b"0/1:-2.5", b"0/1:-2.500001"]),
    gline(b"GT:GQ", [b"0/1:999999999.999999", b"0/1:-999999999.5"]),
    gline(b"GT:GQ", [b"0/1:7.", b"0/1:+3.49"]),
    gline(b"GT:DP", [b"0/1:-7", b"0/1:+0"]),                            # a negative DP is a value
    gline(b"GT:FT", [b"0/1:.", b"0/1:"]),                               # an empty FT filters
    gline(b"GT::DP", [b"0/1:x:3", b"0/1"]),                             # an empty key takes a value
    gline(b"GT:XX:GQ", [b"2/1::9", b"1/2:a:8"], alt=b"G,T"),
    # GQ texts the host converts
    gline(b"GT:GQ", [b"0/1:1e1", b"0/1:.5"]),
    gline(b"GT:GQ", [b"0/1:12.5000000", b"0/1:1234567890"]),
    gline(b"GT:GQ", [b"0/1:0.49999999999999999999", b"0/1:1e400"]),
    gline(b"GT:GQ", [b"0/1:-1e400", b"0/1:4294967296.5"]),
]

# cells under FORMAT GT:GQ:DP:FT:AD of a line with ALT T,G, by ploidy
GTS = {0: [b"", b"/", b"|"], 1: [b"0", b".", b"2"], 2: [b"0/1", b"./.", b"1|2", b"0\\1", b"2/2", b".|1"],
       3: [b"0/1/2", b"0|1|.", b"2/2/2"]}
TAILS = [b"", b":35", b":35:4", b":35:4:PASS", b":35:4:PASS:1,2", b":.:.:.", b":-1:-7:q10", b":12.5:3",
         b":48", b":0.5:0:.:5", b":99.499999:120:lowGQ;lowDP:10,20,30", b":7.:+3"]
FMT = b"GT:GQ:DP:FT:AD"


def synth_lines(S, max_ploidy, seed, n=12, long_at=(), short_at=()):
    """n lines of S cells each, ploidies up to max_ploidy (line 0 holds one of exactly it); INFO is
    padded by 0..64 bytes; a line in long_at gets 2100 bytes more INFO (past VCF_LONG whatever S),
    a line in short_at only bare GT values (the shortest cells)."""
    rng = random.Random(seed)
    lines = []
    for i in range(n):
        cells = []
        for s in range(S):
            p = max_ploidy if (i == 0 and s == S - 1) else rng.randint(0, max_ploidy)
            gt = rng.choice(GTS[p])
            cells.append(gt if i in short_at else gt + rng.choice(TAILS))
        pad = (seed * 7 + i * 11) % 65 + (2100 if i in long_at else 0)
        lines.append(gline(FMT, cells, pos=b"%d" % (100 + i), alt=b"T,G", info=b"DP=5;X=" + b"a" * pad))
    return lines


def synth_cases(wave_s, offs):
    """(S, largest ploidy) of the synthetic files: the sample counts around the path threshold
    wave_s, the ballot width and the wave's offset list of offs entries; ploidies 1, 2 and 3."""
    ss = sorted({1, 2, wave_s - 1, wave_s, 63, 64, 65, 130, offs + 24})
    return [(S, 1 + i % 3) for i, S in enumerate(ss)]


def synth_file(S, max_ploidy):
    """The file of a synth_cases entry: lines 3 and 9 past VCF_LONG, lines 5 and 6 of bare GT values."""
    return synth_text(S, max_ploidy, seed=S, long_at=(3, 9), short_at=(5, 6))


def synth_text(S, max_ploidy, seed, **kw):
    return header(S) + b"".join(l + b"\n" for l in synth_lines(S, max_ploidy, seed, **kw))
