"""Host-side mirror of Disq's reads API over the MI355X path.

Mirrors, with the same names, argument meaning and error behaviour:
  HtsjdkReadsRddStorage      D/HtsjdkReadsRddStorage.java:17-131 (read side)
  HtsjdkReadsRdd             D/HtsjdkReadsRdd.java:16-38
  HtsjdkReadsTraversalParameters  D/HtsjdkReadsTraversalParameters.java:13-30
  getReads (AbstractBinarySamSource.java:42-136) with BamSource's planning/iteration
  (BamSource.java:61-182) executed by libdisq_gpu.so.

There is no Spark here: the "RDD" is the ordered list of partitions Spark would hold, each a
structure-of-arrays batch of records (plus each record's raw 4 + block_size bytes).
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import _lib


class ValidationStringency:
    STRICT = 0
    LENIENT = 1
    SILENT = 2
    DEFAULT_STRINGENCY = STRICT


@dataclass(frozen=True)
class Interval:
    """htsjdk.samtools.util.Interval (1-based, closed)."""
    contig: str
    start: int
    end: int

    def getContig(self):
        return self.contig

    def getStart(self):
        return self.start

    def getEnd(self):
        return self.end


class HtsjdkReadsTraversalParameters:
    def __init__(self, intervalsForTraversal: Optional[Sequence[Interval]],
                 traverseUnplacedUnmapped: bool):
        self._intervals = None if intervalsForTraversal is None else list(intervalsForTraversal)
        self._unplaced = bool(traverseUnplacedUnmapped)

    def getIntervalsForTraversal(self):
        return self._intervals

    def getTraverseUnplacedUnmapped(self):
        return self._unplaced


@dataclass
class SAMFileHeader:
    text: str
    sequences: List[tuple]  # (name, length)
    raw: bytes = b""        # the BAM header as stored (BAMFileWriter.writeHeader's bytes)

    def getSequenceDictionary(self):
        return self.sequences

    def getSequenceIndex(self, name):
        for i, (n, _) in enumerate(self.sequences):
            if n == name:
                return i
        return -1


@dataclass
class ReadsPartition:
    """Records of one Spark partition, as structure-of-arrays."""
    fields: dict
    raw: Optional[np.ndarray]
    digest: int
    path: str = ""
    tags: Optional[dict] = None  # read(tags=...): per requested id the partition's tag columns

    def __len__(self):
        return len(self.fields["voffset"])

    def record_bytes(self, i):
        o = int(self.fields["raw_offset"][i])
        n = 4 + int(self.fields["block_size"][i])
        return bytes(self.raw[o:o + n])


@dataclass
class ReadsRDD:
    partitions: List[ReadsPartition] = field(default_factory=list)

    def count(self):
        return sum(len(p) for p in self.partitions)

    def getNumPartitions(self):
        return len(self.partitions)

    def field(self, name):
        arrs = [p.fields[name] for p in self.partitions]
        return np.concatenate(arrs) if arrs else np.zeros(0)

    def hashes(self):
        return self.field("hash").astype(np.uint64)

    def tag(self, name):
        """The columns of one of the tags asked of read(tags=[...]), per partition: a list of dicts
        with flags, vtype, subtype, val_off, val_len (one entry per read; val_off counts from the
        read's block_size word, so it indexes record_bytes(i)) and values (Context.tags' typed
        view of the key, None for an ANY or STRING key).  KeyError for a tag that was not asked
        for."""
        name = name.decode() if isinstance(name, bytes) else name
        out = []
        for p in self.partitions:
            if p.tags is None or name not in p.tags:
                raise KeyError(name)
            out.append(p.tags[name])
        return out


class HtsjdkReadsRdd:
    def __init__(self, header: SAMFileHeader, reads: ReadsRDD):
        self._header = header
        self._reads = reads

    def getHeader(self):
        return self._header

    def getReads(self):
        return self._reads


def _parse_header(raw: bytes) -> SAMFileHeader:
    import struct
    l_text = struct.unpack_from("<i", raw, 4)[0]
    text = raw[8:8 + l_text].decode(errors="replace")
    p = 8 + l_text
    n_ref = struct.unpack_from("<i", raw, p)[0]
    p += 4
    seqs = []
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", raw, p)[0]
        name = raw[p + 4:p + 4 + ln - 1].decode()
        length = struct.unpack_from("<i", raw, p + 4 + ln)[0]
        seqs.append((name, length))
        p += 8 + ln
    return SAMFileHeader(text, seqs, bytes(raw[:p]))


def _is_hidden(name):  # HiddenFileFilter (D/impl/file/HiddenFileFilter.java)
    return name.startswith("_") or name.startswith(".")


class HtsjdkReadsRddStorage:
    """Builder + read() of Disq's reads entry point, backed by libdisq_gpu.so."""

    def __init__(self, device: int = 0):
        self._split_size = 0
        self._stringency = ValidationStringency.DEFAULT_STRINGENCY
        self._use_nio = False
        self._reference = None
        self._device = device
        self._verify_crc = False
        self._use_sbi = False

    @staticmethod
    def makeDefault(device: int = 0) -> "HtsjdkReadsRddStorage":
        return HtsjdkReadsRddStorage(device)

    def splitSize(self, splitSize: int):
        self._split_size = int(splitSize)
        return self

    def validationStringency(self, s: int):
        self._stringency = s
        return self

    def useNio(self, useNio: bool):
        self._use_nio = bool(useNio)
        return self

    def referenceSourcePath(self, p):
        self._reference = p
        return self

    def verifyCrc(self, v: bool):
        """Extension: check every BGZF block's CRC32 (htsjdk's default does not)."""
        self._verify_crc = bool(v)
        return self

    def useSplittingIndex(self, v: bool):
        """Extension: plan partitions from path.sbi (SBIIndex.getChunk) when it exists.  Disq
        itself loads the .sbi and discards the result (BamSource.java:69-87), so the default
        (False) only validates it and plans by record guessing."""
        self._use_sbi = bool(v)
        return self

    def _files(self, path):
        if os.path.isdir(path):
            names = sorted(n for n in os.listdir(path) if not _is_hidden(n))
            return [os.path.join(path, n) for n in names]
        return [path]

    def read(self, path: str, traversalParameters: Optional[HtsjdkReadsTraversalParameters] = None,
             tags: Optional[Sequence] = None) -> HtsjdkReadsRdd:
        """tags (extension): aux tag ids, or (id, _lib.TAG_* class) pairs, decoded on the device
        next to the reads (Context.tags) and handed out per partition by ReadsRDD.tag(id)."""
        files = self._files(path)
        if not files:
            raise ValueError(f"No files found in {path}")
        first = files[0]
        sam = first.endswith(".sam")  # SamFormat.fromPath: the first file's extension decides
        if not sam and not first.endswith(".bam"):
            raise ValueError(f"Cannot find format extension for {path}")
        tp = traversalParameters
        if sam and tp is not None:
            raise ValueError("Traversal parameters are not supported for SAM text input")
        if tp is not None and tp.getIntervalsForTraversal() is None and \
                not tp.getTraverseUnplacedUnmapped():
            # AbstractBinarySamSource.java:50-54
            raise ValueError("Traversing mapped reads only is not supported.")
        header = None
        parts: List[ReadsPartition] = []
        for f in files:
            with _lib.Context(split_size=self._split_size, use_nio=self._use_nio,
                              verify_crc=self._verify_crc, device=self._device,
                              stringency=self._stringency) as ctx:
                if sam:
                    ctx.sam_open_path(f)
                else:
                    ctx.open_path(f)
                sbi = f + ".sbi"  # SBIIndex.FILE_EXTENSION, BamSource.java:69-72
                if not sam and os.path.exists(sbi):
                    with open(sbi, "rb") as fh:
                        ctx.set_splitting_index(fh.read(), self._use_sbi)
                _, hraw = ctx.header()
                h = _parse_header(hraw)
                if header is None:
                    header = h
                trav = None
                if tp is not None:
                    bai = self._find_index(f)
                    if bai is None:
                        raise ValueError(f"Intervals set but no index file found for {f}")
                    with open(bai, "rb") as fh:
                        ctx.set_index(fh.read())
                    ivs = tp.getIntervalsForTraversal()
                    conv = None
                    if ivs is not None:
                        conv = []
                        for iv in ivs:  # BoundedTraversalUtil.convertSimpleIntervalToQueryInterval
                            if iv is None:
                                raise ValueError("interval may not be null")
                            idx = h.getSequenceIndex(iv.getContig())
                            if idx == -1:
                                raise ValueError(f"Contig {iv.getContig()} not present in reads "
                                                 "sequence dictionary")
                            conv.append((idx, iv.getStart(), iv.getEnd()))
                    trav = (conv, tp.getTraverseUnplacedUnmapped())
                b = ctx.sam_read(with_raw=True) if sam else ctx.read(with_raw=True, traversal=trav)
                po = b["part_offset"]
                g = ctx.tags(list(tags), traversal=trav) if tags else None
                if g is not None and g["part_offset"].tolist() != po.tolist():
                    raise RuntimeError("the tag columns' partitions differ from the reads'")
                for p in range(len(po) - 1):
                    lo, hi = int(po[p]), int(po[p + 1])
                    ptags = None
                    if g is not None:
                        ptags = {}
                        for q, vid in enumerate(g["keys"]):
                            t = {k: g[k][q, lo:hi] for k in ("flags", "vtype", "subtype", "val_off", "val_len")}
                            t["values"] = None if g["values"][q] is None else g["values"][q][lo:hi]
                            ptags[vid.decode()] = t
                    fields = {k: b[k][lo:hi] for k, _ in _lib.FIELDS}
                    raw = None
                    if b["raw"] is not None and hi > lo:
                        r0 = int(fields["raw_offset"][0])
                        r1 = int(fields["raw_offset"][-1]) + 4 + int(fields["block_size"][-1])
                        raw = b["raw"][r0:r1]
                        fields["raw_offset"] = fields["raw_offset"] - r0
                    parts.append(ReadsPartition(fields, raw, int(b["part_digest"][p]), f, ptags))
        return HtsjdkReadsRdd(header, ReadsRDD(parts))

    def write(self, rdd: HtsjdkReadsRdd, path: str, tempPartsDirectory: Optional[str] = None, *,
              bai: bool = False, sbi: bool = False, sbiGranularity: int = 4096):
        """BamSink.save (D/impl/formats/bam/BamSink.java:32-69) with GPU BGZF compression: each
        partition's records as a headerless BGZF part (HeaderlessBamOutputFormat, no terminator),
        the header as its own BGZF blocks, the 28-byte EOF block, then the parts merged in
        partition order (Merger.mergeParts) into `path`; the temporary parts directory is deleted
        after the merge (BamSink.java:67-68).  The header bytes are the ones the file was read
        with (header.raw), not re-encoded from a SAMFileHeader as BAMFileWriter.writeHeader does:
        for a header read by this package they are the same BAM header.

        bai / sbi: after the merge the written file is opened on the device and indexed into
        `path + ".bai"` (dq_write_bai; the reads must be coordinate sorted) and / or
        `path + ".sbi"` (dq_write_sbi at sbiGranularity).  They stand in for the BaiWriteOption /
        SbiWriteOption of later Disq versions; with the defaults nothing but `path` is written."""
        header = rdd.getHeader()
        if not header.raw:
            raise ValueError("header has no BAM encoding")
        if path.endswith(".sam"):  # SamFormat.formatWriteOptionFromPath
            if bai or sbi:
                raise ValueError(f"{path}: a .bai / .sbi index needs a BAM path, not SAM text")
            return self._write_sam(rdd, path, tempPartsDirectory)
        eof = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
        with _lib.Context(device=self._device) as ctx:
            pieces = [ctx.bgzf_compress(header.raw)]
            for p in rdd.getReads().partitions:
                raw = b"" if p.raw is None else p.raw.tobytes()
                pieces.append(ctx.bgzf_compress(raw))
        pieces.append(eof)
        if tempPartsDirectory:
            os.makedirs(tempPartsDirectory, exist_ok=True)
            names = ["header"] + [f"part-r-{i:05d}" for i in range(len(pieces) - 2)] + ["terminator"]
            for n, d in zip(names, pieces):
                with open(os.path.join(tempPartsDirectory, n), "wb") as fh:
                    fh.write(d)
        with open(path, "wb") as fh:
            for d in pieces:
                fh.write(d)
        if tempPartsDirectory:  # fileSystemWrapper.delete(tempPartsDirectory)
            import shutil
            shutil.rmtree(tempPartsDirectory, ignore_errors=True)
        if bai or sbi:
            with _lib.Context(device=self._device) as ctx:
                ctx.open_path(path)
                if bai:
                    with open(path + ".bai", "wb") as fh:
                        fh.write(ctx.write_bai())
                if sbi:
                    with open(path + ".sbi", "wb") as fh:
                        fh.write(ctx.write_sbi(sbiGranularity))
        return path

    def _write_sam(self, rdd: HtsjdkReadsRdd, path: str, tempPartsDirectory: Optional[str]):
        """SamSink.save (D/impl/formats/sam/SamSink.java:31-49): every read as
        SAMRecord.getSAMString, trimmed, one per line (dq_sam_write formats each partition on the
        GPU; an empty partition gives an empty part), the header as its own file, then the parts
        merged in partition order (Merger.mergeParts) into `path`; the temporary parts directory
        is deleted after the merge.  The header file is the text inside header.raw, ending in one
        newline, not re-encoded from a SAMFileHeader (the caveat of the BAM writer above)."""
        import struct
        header = rdd.getHeader()
        l_text = struct.unpack_from("<i", header.raw, 4)[0]
        text = bytes(header.raw[8:8 + l_text]).rstrip(b"\0")
        if text and not text.endswith(b"\n"):
            text += b"\n"
        pieces = [text]
        with _lib.Context(device=self._device) as ctx:
            for p in rdd.getReads().partitions:
                if p.raw is None or len(p) == 0:
                    pieces.append(b"")
                else:
                    pieces.append(ctx.sam_write(header.raw, p.raw, p.fields["raw_offset"]))
        if tempPartsDirectory:
            os.makedirs(tempPartsDirectory, exist_ok=True)
            names = ["header"] + [f"part-r-{i:05d}" for i in range(len(pieces) - 1)]
            for n, d in zip(names, pieces):
                with open(os.path.join(tempPartsDirectory, n), "wb") as fh:
                    fh.write(d)
        with open(path, "wb") as fh:
            for d in pieces:
                fh.write(d)
        if tempPartsDirectory:  # fileSystemWrapper.delete(tempPartsDirectory)
            import shutil
            shutil.rmtree(tempPartsDirectory, ignore_errors=True)
        return path

    @staticmethod
    def _find_index(path):
        # AbstractSamSource.findIndex (D/impl/formats/sam/AbstractSamSource.java:92-108)
        cand = [path + ".bai"]
        if path.endswith(".bam"):
            cand.append(path[: -len(".bam")] + ".bai")
        for c in cand:
            if os.path.exists(c):
                return c
        return None


class VariantsPartition(list):
    """The variant lines of one Spark partition (bytes, terminators excluded)."""


class VariantSite:
    """One decoded variant (read(decode=True)): the site fields htsjdk's VCFCodec.decode computes
    eagerly, built from dq_vcf_read's columns and the variant's site bytes.  contig is the CHROM
    text, start and end are 1-based and closed, id is None for ".", alts is a list of bytes, qual
    the QUAL text's value or None, filters None (unfiltered), an empty set (PASS) or the set of
    filter names, info the INFO column's bytes."""
    __slots__ = ("contig", "start", "end", "id", "ref", "alts", "qual", "filters", "info")

    def __init__(self, contig, start, end, id, ref, alts, qual, filters, info):
        self.contig, self.start, self.end, self.id, self.ref = contig, start, end, id, ref
        self.alts, self.qual, self.filters, self.info = alts, qual, filters, info

    def _key(self):
        return tuple(getattr(self, k) for k in self.__slots__)

    def __eq__(self, other):
        return isinstance(other, VariantSite) and self._key() == other._key()

    def __repr__(self):
        return "VariantSite(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in self.__slots__) + ")"


def variant_sites(b):
    """The VariantSite rows of a SITES (or LINES) batch of Context.vcf_read, per partition."""
    d, do, ce, fl = b["data"], b["data_offset"], b["col_end"], b["flags"]
    rows = []
    for k in range(len(fl)):
        e = [int(x) for x in ce[k]]
        site = bytes(d[do[k]:do[k] + e[7]])
        col = [site[(e[c - 1] + 1 if c else 0):e[c]] for c in range(8)]
        f = int(fl[k])
        filters = None if f & _lib.VCF_UNFILTERED else set() if f & _lib.VCF_PASS else set(col[6].split(b";"))
        rows.append(VariantSite(col[0], int(b["pos"][k]), int(b["end"][k]),
                                col[2] if f & _lib.VCF_HAS_ID else None, col[3],
                                col[4].split(b",") if int(b["n_alt"][k]) else [],
                                float(b["qual"][k]) if f & _lib.VCF_HAS_QUAL else None, filters, col[7]))
    po = b["part_offset"]
    return [VariantsPartition(rows[po[p]:po[p + 1]]) for p in range(len(po) - 1)]


class GenotypesPartition:
    """One partition's rows of the genotype matrix (Context.vcf_genotypes): flags, ploidy, gq, dp and
    cell_off shaped (rows, S), allele shaped (rows, S, P); row k belongs to the partition's variant
    k."""
    __slots__ = ("flags", "ploidy", "allele", "gq", "dp", "cell_off")

    def __init__(self, g, lo, hi):
        for k in self.__slots__:
            setattr(self, k, g[k][lo:hi])

    def __len__(self):
        return len(self.flags)


class InfoPartition:
    """One partition's rows of the INFO columns (Context.vcf_info): keys (the ids), flags, n_values,
    val_off and val_len shaped (K, rows), and values: per key its rows of the Integer or Float
    column shaped (rows,) or (rows, W), None for a Flag or String key; row k belongs to the
    partition's variant k."""
    __slots__ = ("keys", "flags", "n_values", "val_off", "val_len", "values")

    def __init__(self, g, lo, hi):
        self.keys = list(g["keys"])
        for k in ("flags", "n_values", "val_off", "val_len"):
            setattr(self, k, g[k][:, lo:hi])
        self.values = [None if v is None else v[lo:hi] for v in g["values"]]

    def __len__(self):
        return self.flags.shape[1]

    def get(self, key):
        """(flags, values) of one key by its id."""
        q = self.keys.index(key.encode() if isinstance(key, str) else key)
        return self.flags[q], self.values[q]


class VariantsRDD:
    def __init__(self, partitions):
        self.partitions = partitions

    def count(self):
        return sum(len(p) for p in self.partitions)

    def getNumPartitions(self):
        return len(self.partitions)

    def collect(self):
        return [l for p in self.partitions for l in p]


class HtsjdkVariantsRdd:
    def __init__(self, header_lines, variants: VariantsRDD, genotypes=None, info=None):
        self._header = header_lines
        self._variants = variants
        self._genotypes = genotypes
        self._info = info

    def getInfo(self):
        """One InfoPartition per partition (read(info=[...])), else None."""
        g = self._info
        if g is None:
            return None
        po = g["part_offset"]
        return [InfoPartition(g, int(po[p]), int(po[p + 1])) for p in range(len(po) - 1)]

    def getSampleNames(self):
        """The #CHROM line's sample names (read(genotypes=True)), else None."""
        return None if self._genotypes is None else list(self._genotypes["samples"])

    def getGenotypes(self):
        """One GenotypesPartition per partition (read(genotypes=True)), else None."""
        g = self._genotypes
        if g is None:
            return None
        po = g["part_offset"]
        return [GenotypesPartition(g, int(po[p]), int(po[p + 1])) for p in range(len(po) - 1)]

    def getHeader(self):
        """The '#' lines of the file (VCFHeader source text)."""
        return self._header

    def getVariants(self):
        """The data lines per partition, as VcfSource hands them to VCFCodec.decode."""
        return self._variants


class HtsjdkVariantsRddStorage:
    """Builder + read() of Disq's variants entry point (D/HtsjdkVariantsRddStorage.java:25-83,
    VcfSource.getVariants D/impl/formats/vcf/VcfSource.java:88-113) for BGZF-compressed VCF on the
    GPU text path.  Lines are returned undecoded by default; read(decode=True) decodes them on the
    device (dq_vcf_read) into VariantSite rows."""

    def __init__(self, device: int = 0):
        self._split_size = 0
        self._device = device

    @staticmethod
    def makeDefault(device: int = 0) -> "HtsjdkVariantsRddStorage":
        return HtsjdkVariantsRddStorage(device)

    def splitSize(self, splitSize: int):
        self._split_size = int(splitSize)
        return self

    def read(self, path: str, intervals: Optional[Sequence[Interval]] = None,
             decode: bool = False, genotypes: bool = False, info=None) -> HtsjdkVariantsRdd:
        """decode: each partition holds VariantSite rows (the device's VCFCodec.decode, SITES
        export: only the first eight columns' bytes cross to the host) instead of line bytes.
        genotypes (with decode): the sample columns decoded on the device as well
        (dq_vcf_genotypes); the rdd then answers getSampleNames() and getGenotypes().
        info (with decode): INFO keys, names or (name, type) pairs, decoded on the device into
        typed columns (dq_vcf_info); the rdd then answers getInfo()."""
        if genotypes and not decode:
            raise ValueError("genotypes=True needs decode=True")
        if info is not None and not decode:
            raise ValueError("info=[...] needs decode=True")
        if not (path.endswith(".gz") or path.endswith(".bgz")):
            raise ValueError(f"{path}: the GPU text path reads BGZF-compressed VCF (.vcf.gz/.vcf.bgz)")
        with _lib.Context(split_size=self._split_size, device=self._device) as ctx:
            ctx.text_open_path(path)
            if intervals is not None:
                tbi = path + ".tbi"  # TabixUtils.STANDARD_INDEX_EXTENSION (VcfSource.java:147)
                if not os.path.exists(tbi):
                    raise ValueError(f"Intervals set but no index file found for {path} at {tbi}")
                with open(tbi, "rb") as fh:
                    ctx.text_set_index(fh.read())
                ctx.text_set_intervals([(iv.getContig(), iv.getStart(), iv.getEnd())
                                        for iv in intervals])
            b = ctx.vcf_read(_lib.VCF_EXPORT_SITES) if decode else ctx.text_read(True)
            g = ctx.vcf_genotypes() if genotypes else None
            i = ctx.vcf_info(list(info)) if info is not None else None
        if decode:
            return HtsjdkVariantsRdd(vcf_header_lines(path), VariantsRDD(variant_sites(b)), g, i)
        d, do, ln, po = b["data"], b["data_offset"], b["line_len"], b["part_offset"]
        parts = [VariantsPartition(bytes(d[do[k]:do[k] + ln[k]]) for k in range(po[p], po[p + 1]))
                 for p in range(len(po) - 1)]
        return HtsjdkVariantsRdd(vcf_header_lines(path), VariantsRDD(parts))

    def write(self, rdd: HtsjdkVariantsRdd, path: str, tempPartsDirectory: Optional[str] = None, *,
              tabix: bool = False):
        """VcfSink.save (D/impl/formats/vcf/VcfSink.java:27-68) with GPU BGZF compression: the
        header lines as read (getHeader(), each followed by a newline) as their own BGZF blocks,
        each partition's lines with a newline after each (as TextOutputFormat writes them) as a
        BGZF part without the EOF terminator, the 28-byte EOF block, then the parts merged in partition order
        (Merger.mergeParts) into `path`; the temporary parts directory is deleted after the merge.
        The output is compressed when `path` ends in .bgz or .gz and a plain concatenation for
        .vcf; any other extension raises ValueError (VcfSink's format lookup).

        tabix: after the merge the written file is opened on the device and indexed into
        `path + ".tbi"` (dq_text_write_tbi; the variants must be sorted).  It stands in for the
        TabixIndexWriteOption of later Disq versions and needs a compressed path; with the
        default nothing but `path` is written."""
        compressed = path.endswith(".bgz") or path.endswith(".gz")
        if not compressed and not path.endswith(".vcf"):
            raise ValueError(f"Cannot find format extension for {path}")
        if tabix and not compressed:
            raise ValueError(f"{path}: a tabix index needs a BGZF-compressed VCF (.vcf.gz/.vcf.bgz)")
        texts = [b"".join(bytes(h) + b"\n" for h in rdd.getHeader())]
        for p in rdd.getVariants().partitions:
            texts.append(b"".join(bytes(l) + b"\n" for l in p))
        if compressed:
            eof = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
            with _lib.Context(device=self._device) as ctx:
                pieces = [ctx.bgzf_compress(t) for t in texts] + [eof]
            names = ["header"] + [f"part-r-{i:05d}" for i in range(len(texts) - 1)] + ["terminator"]
        else:
            pieces = texts
            names = ["header"] + [f"part-r-{i:05d}" for i in range(len(texts) - 1)]
        if tempPartsDirectory:
            os.makedirs(tempPartsDirectory, exist_ok=True)
            for n, d in zip(names, pieces):
                with open(os.path.join(tempPartsDirectory, n), "wb") as fh:
                    fh.write(d)
        with open(path, "wb") as fh:
            for d in pieces:
                fh.write(d)
        if tempPartsDirectory:  # fileSystemWrapper.delete(tempPartsDirectory)
            import shutil
            shutil.rmtree(tempPartsDirectory, ignore_errors=True)
        if tabix:
            TabixIndexer.createIndex(path, device=self._device)
        return path


def vcf_header_lines(path: str):
    """The leading '#' lines of a BGZF VCF, read from a prefix of the file: BGZF members are
    inflated from the start (on the driver, as VcfSource.getVCFCodec reads the header through
    htsjdk, D/impl/formats/vcf/VcfSource.java:60-86) only until the first line that does not start
    with '#' (or the end of the file: no byte cap, however many contig/sample lines there are).  Terminators as Hadoop's LineReader: LF, CR LF, lone CR; a UTF-8 BOM on the first
    line is dropped (LineRecordReader.skipUtfByteOrderMark)."""
    import struct
    import zlib
    lines, buf, first, read = [], b"", True, 0
    with open(path, "rb") as fh:
        while True:
            hdr = fh.read(12)
            if len(hdr) < 12:
                break
            if hdr[:4] != b"\x1f\x8b\x08\x04":
                raise ValueError(f"{path}: not a BGZF member at {read}")
            xlen = struct.unpack_from("<H", hdr, 10)[0]
            extra = fh.read(xlen)
            bsize, k = None, 0
            while k + 4 <= len(extra):  # the BC subfield holds BSIZE
                si1, si2, slen = extra[k], extra[k + 1], struct.unpack_from("<H", extra, k + 2)[0]
                if si1 == 66 and si2 == 67 and slen == 2:
                    bsize = struct.unpack_from("<H", extra, k + 4)[0] + 1
                k += 4 + slen
            if bsize is None:
                raise ValueError(f"{path}: BGZF member without a BC subfield at {read}")
            body = fh.read(bsize - 12 - xlen)
            read += bsize
            buf += zlib.decompress(body[:-8], -15)
            if first and buf.startswith(b"\xef\xbb\xbf"):
                buf = buf[3:]
            first = False if buf else first
            # complete lines (a CR at the very end may be the first half of a CR LF)
            pos = 0
            while True:
                i = min([x for x in (buf.find(b"\n", pos), buf.find(b"\r", pos)) if x >= 0],
                        default=-1)
                if i < 0 or (buf[i:i + 1] == b"\r" and i + 1 == len(buf)):
                    break
                line = buf[pos:i]
                if not line.startswith(b"#"):
                    return lines
                lines.append(line)
                pos = i + (2 if buf[i:i + 2] == b"\r\n" else 1)
            buf = buf[pos:]
            if buf and not buf.startswith(b"#"):
                return lines
    if buf.startswith(b"#"):  # a header line that runs to the end of the file
        lines.append(buf.rstrip(b"\r"))
    return lines


class BAMSBIIndexer:
    """htsjdk BAMSBIIndexer (M/htsjdk/samtools/BAMSBIIndexer.java:20-66) on the GPU read path."""

    @staticmethod
    def createIndex(bamFile: str, granularity: int = 4096, device: int = 0) -> str:
        with _lib.Context(device=device) as ctx:
            ctx.open_path(bamFile)
            data = ctx.write_sbi(granularity)
        out = bamFile + ".sbi"
        with open(out, "wb") as fh:
            fh.write(data)
        return out


class BAMIndexer:
    """htsjdk BAMIndexer.createIndex on the GPU read path (dq_write_bai): the .bai of a
    coordinate-sorted BAM, built from the resident records."""

    @staticmethod
    def createIndex(bamFile: str, output: Optional[str] = None, device: int = 0) -> str:
        if output is None:  # the sibling AbstractSamSource.findIndex looks for (_find_index)
            output = (bamFile[: -len(".bam")] if bamFile.endswith(".bam") else bamFile) + ".bai"
        with _lib.Context(device=device) as ctx:
            ctx.open_path(bamFile)
            data = ctx.write_bai()
        with open(output, "wb") as fh:
            fh.write(data)
        return output


class TabixIndexer:
    """htsjdk TabixIndexCreator on the GPU text path (dq_text_write_tbi): the .tbi of a sorted
    BGZF-compressed VCF, built from the resident lines and written, as htsjdk writes it, as a BGZF
    file (the index bytes in BGZF blocks, then the EOF block)."""

    @staticmethod
    def createIndex(vcfFile: str, output: Optional[str] = None, device: int = 0) -> str:
        if output is None:
            output = vcfFile + ".tbi"  # TabixUtils.STANDARD_INDEX_EXTENSION
        with _lib.Context(device=device) as ctx:
            ctx.text_open_path(vcfFile)
            data = ctx.text_write_tbi()
            packed = ctx.bgzf_compress(data)
        with open(output, "wb") as fh:
            fh.write(packed)
            fh.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
        return output
