"""VCF data lines for the site-decode tests: good lines that take every rule's
branches, and bad lines, at least two per error class, with the class the first failing check
names.  ORDER holds lines that fail two checks: the earlier check in the order fields, CHROM, POS,
ID, REF, ALT, QUAL, FILTER, INFO names the error."""

HEADER = (b"##fileformat=VCFv4.2\n"
          b"##contig=<ID=chr1,length=1000000>\n"
          b"##contig=<ID=chr2,length=500000,assembly=b37>\n"
          b"##contig=<length=7,ID=chrM>\n"
          b"##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Depth, all reads\">\n"
          b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\tS2\n")
SITES_HEADER = (b"##fileformat=VCFv4.2\n"
                b"##contig=<ID=chr1>\n"
                b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")

GT = b"\tGT\t0/1\t1/1"


def line(chrom=b"chr1", pos=b"100", vid=b".", ref=b"A", alt=b"T", qual=b"50", filt=b"PASS",
         info=b"DP=5", rest=GT):
    return b"\t".join([chrom, pos, vid, ref, alt, qual, filt, info]) + rest


def good_lines():
    """Lines of a file with HEADER; each is accepted."""
    return [
        line(),
        line(chrom=b"chr2", pos=b"+7", vid=b"rs1;rs2", ref=b"acgtn", alt=b"A,<DEL>,*", qual=b"."),
        line(chrom=b"chrM", pos=b"-3", ref=b"N", alt=b".", filt=b".", info=b"."),
        line(chrom=b"unknown", pos=b"0000012", alt=b"G]chr2:5]", qual=b"1e3", filt=b"q10;s50"),
        line(pos=b"2147483647", ref=b"ACGT", alt=b"[chr1:9[N", qual=b"12.50", info=b"SVTYPE=BND;END=77;X"),
        line(pos=b"-2147483648", alt=b"<INS:ME>", qual=b"5.", info=b"END=-4"),
        line(pos=b"2147483647", ref=b"ACG"),                            # end wraps as a Java int does
        line(alt=b"a", ref=b"G", qual=b"0.000001", info=b"ENDX=5;XEND=7;AEND;END=+12;END=bad"),
        line(alt=b"T,c,G", qual=b"-0", filt=b"LowQual", info=b"A=1;B;C=x,y;END=2147483647"),
        line(qual=b"123456789012345", rest=b"\tGT"),                    # 15 digits, nine columns
        line(qual=b"1E-5", rest=GT + b"\t"),                             # a trailing TAB: one more column
        line(qual=b"4.94e+2", filt=b"PASSED;pass", info=b"END=5"),
        line(qual=b"100000000000000000000"),                             # zeros past the 15th digit
        line(qual=b"0e999", alt=b"<>"),
        # QUAL texts the host converts
        line(qual=b"1e-30"), line(qual=b"1e400"), line(qual=b"123456789012345678"), line(qual=b".5"),
        line(qual=b"0.1234567890123456"),
    ]


def bad_lines():
    """(line, class) of a file with HEADER."""
    return [
        (b"", "fields"),
        (b"chr1\t100\t.\tA\tT\t50\tPASS\tDP=5", "fields"),              # eight columns under a sample header
        (b"chr1\t100\t.\tA\tT\t50\tPASS", "fields"),
        (b"chr1 100 . A T 50 PASS DP=5 GT 0/1", "fields"),
        (line(chrom=b""), "CHROM"),
        (b"\t\t\t\t\t\t\t\t", "CHROM"),
        (line(pos=b""), "POS"),
        (line(pos=b"12a"), "POS"),
        (line(pos=b"2147483648"), "POS"),
        (line(pos=b"-2147483649"), "POS"),
        (line(pos=b"+"), "POS"),
        (line(pos=b"1.0"), "POS"),
        (line(pos=b" 5"), "POS"),
        (line(vid=b""), "ID"),
        (line(vid=b"", ref=b"X"), "ID"),
        (line(ref=b""), "REF"),
        (line(ref=b"AXG"), "REF"),
        (line(ref=b"."), "REF"),
        (line(ref=b"A*"), "REF"),
        (line(alt=b""), "ALT"),
        (line(alt=b"T,"), "ALT"),
        (line(alt=b",T"), "ALT"),
        (line(alt=b"T,,G"), "ALT"),
        (line(alt=b"T,."), "ALT"),
        (line(alt=b"TX"), "ALT"),
        (line(alt=b"<DEL"), "ALT"),
        (line(alt=b"**"), "ALT"),
        (line(alt=b"a"), "ALT"),                                         # equals REF without case
        (line(alt=b"T,G,t"), "ALT"),                                     # "Duplicate allele"
        (line(alt=b"<DEL>,<del>"), "ALT"),
        (line(qual=b""), "QUAL"),
        (line(qual=b"abc"), "QUAL"),
        (line(qual=b"NaN"), "QUAL"),
        (line(qual=b"Infinity"), "QUAL"),
        (line(qual=b"0x1p3"), "QUAL"),
        (line(qual=b"1.5f"), "QUAL"),
        (line(qual=b"1d"), "QUAL"),
        (line(qual=b"1e"), "QUAL"),
        (line(qual=b"1e+"), "QUAL"),
        (line(qual=b".e1"), "QUAL"),
        (line(qual=b"+"), "QUAL"),
        (line(qual=b"1 "), "QUAL"),
        (line(qual=b"1.2.3"), "QUAL"),
        (line(filt=b""), "FILTER"),
        (line(filt=b"0"), "FILTER"),
        (line(filt=b"q10;PASS"), "FILTER"),
        (line(filt=b"PASS;q10"), "FILTER"),
        (line(info=b""), "INFO"),
        (line(info=b"DP=5; AF=1"), "INFO"),
        (line(info=b"END=abc"), "INFO"),
        (line(info=b"DP=1;END=;X"), "INFO"),
        (line(info=b"END"), "INFO"),
        (line(info=b"END=2147483648"), "INFO"),
        (line(info=b"A;END=1.5;END=7"), "INFO"),
    ]


ORDER = [
    (b"\t100\t.\tA\tT\t50\tPASS", "fields"),                             # fields before CHROM
    (line(chrom=b"", pos=b"x"), "CHROM"),
    (line(pos=b"x", vid=b""), "POS"),
    (line(vid=b"", ref=b""), "ID"),
    (line(ref=b"X", alt=b""), "REF"),
    (line(alt=b"X!", qual=b"bad"), "ALT"),
    (line(qual=b"bad", filt=b"0"), "QUAL"),
    (line(filt=b"", info=b""), "FILTER"),
    (line(chrom=b"", info=b"END=x"), "CHROM"),
]


def sites_good_lines():
    """Lines of a file with SITES_HEADER (no sample): exactly eight columns."""
    return [line(rest=b""), line(rest=b"", alt=b"<DEL>", info=b"END=500", filt=b"."),
            line(rest=b"", chrom=b"chrZ", qual=b".", vid=b"rs9")]


def sites_bad_lines():
    return [(line(), "fields"), (line(rest=b"\t"), "fields"), (b"chr1\t100\t.\tA\tT\t50\tPASS", "fields"),
            (line(rest=b"", info=b""), "INFO")]


# The five variants of tests/golden/test.vcf, written out by hand: (pos, end, id, ref, alts, qual,
# filters, flags, n_info, col_end); CHROM is 20 (contig 0), three sample columns.  Flags: HAS_ID 1,
# HAS_QUAL 2, PASS 8, HAS_GENOTYPES 32.
TEST_VCF = [
    (14370, 14370, b"rs6054257", b"G", [b"A"], 29.0, set(), 1 | 2 | 8 | 32, 5,
     [2, 8, 18, 20, 22, 25, 30, 54]),
    (17330, 17330, None, b"T", [b"A"], 3.0, {b"q10"}, 2 | 32, 3,
     [2, 8, 10, 12, 14, 16, 20, 40]),
    (1110696, 1110696, b"rs6040355", b"A", [b"G", b"T"], 67.0, set(), 1 | 2 | 8 | 32, 5,
     [2, 10, 20, 22, 26, 29, 34, 68]),
    (1230237, 1230237, None, b"T", [], 47.0, set(), 2 | 8 | 32, 3,
     [2, 10, 12, 14, 16, 19, 24, 40]),
    (1234567, 1234569, b"microsat1", b"GTC", [b"G", b"GTCT"], 50.0, set(), 1 | 2 | 8 | 32, 3,
     [2, 10, 20, 24, 31, 34, 39, 54]),
]
