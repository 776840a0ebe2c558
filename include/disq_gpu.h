/*
 * disq_gpu.h -- C ABI of libdisq_gpu.so, the MI355X (gfx950) BAM read path for Disq.
 *
 * Drop-in boundary.  A JNI / Panama shim implements the three
 * template methods of D/impl/formats/sam/AbstractBinarySamSource.java:138-150 on top of these
 * calls; callers of HtsjdkReadsRddStorage.read() (D/HtsjdkReadsRddStorage.java:83-131) are
 * unchanged.  No HIP or torch types cross this boundary: plain pointers and sizes only.
 *
 *   reference interface                                         replaced by
 *   ---------------------------------------------------------   -------------------------------
 *   BamSource.getPathChunks (D/impl/formats/bam/BamSource.java:61-104)
 *     = PathSplitSource.getPathSplits (D/impl/file/PathSplitSource.java:26-64)
 *     + BgzfBlockSource/BgzfBlockGuesser (D/impl/formats/bgzf/BgzfBlockSource.java:34-84,
 *       BgzfBlockGuesser.java:76-149)
 *     + getFirstReadInPartition/BamRecordGuesser (BamSource.java:110-153,
 *       D/impl/formats/bam/BamRecordGuesser.java:34-194)                    dq_plan
 *   BamSource.getIterator(SamReader, SAMFileSpan) (BamSource.java:172-175), one Spark task
 *                                                      dq_decode_chunk (dq_decode on a resident file)
 *   BamSource.createIndexIterator + queryUnmapped tail
 *     (BamSource.java:177-182; AbstractBinarySamSource.java:86-134)
 *                                    dq_decode_chunk_filtered (dq_decode_filtered on a resident file)
 *   AbstractBinarySamSource.getReads, whole RDD (AbstractBinarySamSource.java:42-136)  dq_read
 *   AbstractSamSource.getFileHeader (D/impl/formats/sam/AbstractSamSource.java:32-49)
 *                                                                           dq_read_header
 *   htsjdk BAMIndexer.createIndex / BinningIndexBuilder (the .bai that
 *     AbstractBinarySamSource.java:87-91 requires for an interval traversal)    dq_write_bai
 *   SamSource.getReads, whole RDD of a SAM text file
 *     (D/impl/formats/sam/SamSource.java:36-77)                             dq_sam_read
 *   SamSink.save's part file: SAMRecord.getSAMString, String.trim, a LF per read
 *     (D/impl/formats/sam/SamSink.java:37)                                  dq_sam_write
 *   VCFCodec.decode of every data line, the step of VcfSource.getVariants between the '#'
 *     filter and the overlap filter (D/impl/formats/vcf/VcfSource.java:113)    dq_vcf_read
 *   AbstractVCFCodec.createGenotypeMap, what VariantContext.getGenotypes() runs on the text
 *     LazyGenotypesContext kept, over the variants VcfSource.getVariants hands out  dq_vcf_genotypes
 *   AbstractVCFCodec.parseInfo for the keys a consumer asks of VariantContext.getAttribute /
 *     getAttributeAsInt / getAttributeAsDouble / hasAttribute, over the same variants  dq_vcf_info
 *
 * Error mapping (Java side): DQ_EIO -> IOException; DQ_EFORMAT -> htsjdk SAMFormatException;
 * DQ_EINVAL -> IllegalArgumentException; DQ_EDEVICE / DQ_ENOMEM -> RuntimeException.
 * Threading: a dq_ctx is used by one thread at a time (one per Spark task thread); each ctx owns
 * its own HIP stream.  Every call is synchronous with respect to its results.
 */
#ifndef DISQ_GPU_H
#define DISQ_GPU_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version: 2 = dq_batch with the trailing arena_hold pointer (round 5) and the export modes
 * below (round 6).  A JNI / FFM binding compares dq_abi_version() with the value it was built
 * against before it maps dq_batch. */
#define DQ_ABI_VERSION 2

#define DQ_OK 0
#define DQ_EIO (-1)
#define DQ_EFORMAT (-2)
#define DQ_EINVAL (-3)
#define DQ_EDEVICE (-4)
#define DQ_ENOMEM (-5)

/* ValidationStringency (htsjdk); recorded, see DESIGN.md "STRICT validation". */
#define DQ_STRINGENCY_STRICT 0
#define DQ_STRINGENCY_LENIENT 1
#define DQ_STRINGENCY_SILENT 2

typedef struct dq_ctx dq_ctx;

/* HtsjdkReadsRddStorage builder state (D/HtsjdkReadsRddStorage.java:19-73) + device knobs. */
typedef struct dq_opts {
  int32_t device;            /* HIP device ordinal */
  int32_t split_size;        /* splitSize(int); 0 = Hadoop default (one split per block) */
  int32_t use_nio;           /* useNio(boolean): NIO ceil(len/splitSize) splits */
  int32_t verify_crc;        /* check each BGZF block's CRC32 (stricter than htsjdk default) */
  int32_t stringency;        /* validationStringency (recorded) */
  int32_t full_traversal;    /* 1: interval runs inflate and filter the whole file; 0 (default):
                                only the .bai spans of the intervals (dq_run_resident) */
  int64_t hadoop_block_size; /* fs.local.block.size; 0 = 32 MiB */
  int32_t compat;            /* DQ_COMPAT_DISQ_EXACT (default) or DQ_COMPAT_DEDUPE */
  int32_t reserved;
} dq_opts;

/* dq_opts.compat.  DISQ_EXACT reproduces Disq's chunk ends, (splitEnd << 16) | 0xffff
 * (BamSource.java:136-143): when a BGZF block starts exactly at a split end, the records starting
 * in it are read by that partition and again by the next one (BgzfBlockSource includes a block at
 * pos == splitEnd in both splits).  DEDUPE ends guessed chunks at splitEnd << 16 instead, so each
 * record belongs to exactly one partition (the one whose split holds its start block); .sbi chunks
 * are unaffected (they never overlap). */
#define DQ_COMPAT_DISQ_EXACT 0
#define DQ_COMPAT_DEDUPE 1

/* One Spark partition of the BAM read plan: a PathChunk (D/impl/file/PathChunk.java). */
typedef struct dq_chunk {
  int64_t split_start;  /* PathSplit [start, end) */
  int64_t split_end;
  uint64_t vstart;      /* Chunk virtual start (first record found by the guesser) */
  uint64_t vend;        /* Chunk virtual end = (split_end << 16) | 0xffff */
  int32_t has_chunk;    /* 0: getFirstReadInPartition returned null (empty partition) */
  int32_t reserved;
} dq_chunk;

/* Records as structure-of-arrays (fixed BAM fields, SAMv1 §4.2), host memory owned by the
 * library.  raw holds each record's 4 + block_size bytes (what htsjdk's
 * SAMRecordFactory.createBAMRecord needs as restOfData) at raw_offset[i].
 *
 * Export modes (the `with_raw` argument of the decode calls):
 *   DQ_EXPORT_FIELDS  every SoA field, hash and raw_offset; raw = NULL
 *   DQ_EXPORT_RAW     the same plus the raw bytes
 *   DQ_EXPORT_LEAN    voffset and raw only (every other pointer NULL, partition digests kept): the
 *                     fields are the first 36 bytes of each record's raw bytes (block_size, refID,
 *                     pos, bin_mq_nl, flag_nc, l_seq, next_refID, next_pos, tlen: what htsjdk's
 *                     BAMRecordCodec.decode reads, H/BAMFileReader2.java:929-931), and record i+1
 *                     starts 4 + block_size bytes after record i.  52 fewer bytes per record
 *                     cross PCIe.
 * dq_batch_free may release pinned memory (an arena batch) after dq_ctx_destroy: a JNI consumer
 * must free its batches before the HIP runtime shuts down (not from a JVM shutdown hook that can
 * run after it). */
#define DQ_EXPORT_FIELDS 0
#define DQ_EXPORT_RAW 1
#define DQ_EXPORT_LEAN 2
typedef struct dq_batch {
  int64_t n_records;
  uint64_t* voffset;     /* htsjdk start file pointer of the record */
  int32_t* block_size;
  int32_t* ref_id;
  int32_t* pos;          /* 0-based as stored; SAMRecord alignmentStart = pos + 1 */
  int32_t* l_seq;
  int32_t* next_ref_id;
  int32_t* next_pos;
  int32_t* tlen;
  uint16_t* flag;
  uint16_t* bin;
  uint16_t* n_cigar;
  uint8_t* mapq;
  uint8_t* l_read_name;
  uint64_t* hash;        /* per-record raw-byte hash */
  int64_t* raw_offset;
  uint8_t* raw;          /* may be NULL when the caller asked for fields only */
  int64_t raw_len;
  int64_t n_partitions;
  int64_t* part_offset;  /* n_partitions + 1 entries: partition p = [part_offset[p], [p+1]) */
  uint64_t* part_digest; /* ordered digest of each partition's record hashes */
  int32_t in_arena;      /* 1: the arrays live in the context's export arena (dq_set_export_arena) */
  int32_t reserved;
  void* arena_hold;      /* library-internal: the arena's ownership record (NULL off the arena) */
} dq_batch;

/* Interval traversal (HtsjdkReadsTraversalParameters, D/HtsjdkReadsTraversalParameters.java):
 * intervals already converted to (reference index, 1-based start, 1-based end) as in
 * BoundedTraversalUtil.convertSimpleIntervalToQueryInterval (BoundedTraversalUtil.java:36-53).
 * intervals == NULL means getIntervalsForTraversal() == null. */
typedef struct dq_traversal {
  const int32_t* ref;
  const int32_t* start;
  const int32_t* end;
  int64_t n;
  int32_t has_intervals;            /* 0: null interval list */
  int32_t traverse_unplaced_unmapped;
} dq_traversal;

typedef struct dq_header_info {
  int32_t n_ref;
  int32_t reserved;
  uint64_t first_record_voffset;
  int64_t header_bytes;   /* l_text etc. total, uncompressed */
} dq_header_info;

/* Timings / counters of the last pipeline run on the device (for benchmarks). */
typedef struct dq_stats {
  int64_t compressed_bytes;
  int64_t decompressed_bytes;
  int64_t n_blocks;
  int64_t n_records;        /* records emitted over all partitions (duplicates included) */
  int64_t n_partitions;
  double ms_total;          /* device time of the whole pipeline (HIP events) */
  double ms_scan;           /* kernel 1: BGZF scan + chain */
  double ms_inflate;        /* kernel 2: the inflate kernel alone */
  double ms_records;        /* kernel 3: record starts + SoA decode + hash */
  double ms_filter;         /* kernel 4: interval filter */
  double ms_plan;           /* split planning (guesser) */
  uint64_t digest;          /* digest over partition digests, in partition order */
  double ms_crc;            /* CRC32 verification kernel */
  int64_t deflate_bytes;    /* compressed DEFLATE payload bytes (sum of BSIZE + 1 - 26) */
  int64_t n_filtered;       /* records kernel 4 kept (dq_run_resident with intervals), else -1 */
  int64_t h2d_bytes;        /* compressed bytes the last open/decode copied host -> device */
  int64_t owned_bytes;      /* decompressed bytes of the blocks starting inside the splits (the
                               whole stream for a whole file; the shards of a file sum to it) */
  int64_t blocks_inflated;  /* BGZF blocks the last run inflated (fewer than n_blocks in a
                               .bai span run) */
  double ms_span;           /* .bai span run: device time of the sparse inflate + chains + filter */
} dq_stats;

int dq_ctx_create(dq_ctx** out, const dq_opts* opts);
void dq_ctx_destroy(dq_ctx* ctx);
const char* dq_last_error(const dq_ctx* ctx);
const char* dq_version(void);
int32_t dq_abi_version(void); /* DQ_ABI_VERSION of the library */

/* Open a BAM from host memory (copied to HBM) or from a path.  The resident file is used by
 * every call below until the next open. */
int dq_open_memory(dq_ctx* ctx, const uint8_t* bam, int64_t len);
int dq_open_path(dq_ctx* ctx, const char* path);

/* Byte-range shard of one file (multi-GPU): `bytes` are the file's bytes
 * [base, base + len) -- from the start of split p0 through the end of split p1 - 1, plus a halo
 * long enough to hold the last partition's straddling record (the end of the halo may cut a
 * BGZF block).  `file_len` is the whole file's length (split arithmetic) and the shard owns Disq
 * partitions [p0, p1).  `header` is the decompressed BAM header (dq_read_header of the file's
 * first bytes), which the record guesser needs.  Every later call reports file coordinates
 * (split offsets and virtual offsets), exactly as for the whole file.  A halo that is too short
 * fails with DQ_EFORMAT "shard halo too small" (retry with more bytes). */
int dq_open_shard(dq_ctx* ctx, const uint8_t* bytes, int64_t len, int64_t base, int64_t file_len,
                  int64_t p0, int64_t p1, const uint8_t* header, int64_t header_len);

/* The same with the shard's bytes already in device memory (multi-GPU: a rank's own byte range
 * stays resident in HBM and the halo arrives from the next rank over RCCL/xGMI).  dev_bytes is a
 * caller-owned device pointer on this context's device with at least len + 4096 readable bytes,
 * the last 4096 zero; it must stay valid and unchanged until the next open. */
int dq_open_shard_device(dq_ctx* ctx, const void* dev_bytes, int64_t len, int64_t base,
                         int64_t file_len, int64_t p0, int64_t p1, const uint8_t* header,
                         int64_t header_len);

/* The same, reading the shard's bytes [base, base + len) from `path` itself (pinned staging,
 * parallel reads from the page cache overlapped with the copies to the device): the streaming
 * (out-of-core) reader's windows and multi-GPU ranks that read a shared file. */
int dq_open_shard_path(dq_ctx* ctx, const char* path, int64_t base, int64_t len, int64_t p0,
                       int64_t p1, const uint8_t* header, int64_t header_len);

/* Whole-node mode in one process (the benchmark entry of SURVEY.md section 8(b)): the file's
 * partitions in contiguous groups, one per device of `devices` (by the even byte range holding
 * each split's first byte, as disq_amd.parallel.shard_plan), each group decoded on its own
 * context and host thread from the file alone (dq_open_shard_path with a halo grown x4 while too
 * short + dq_run_resident; records stay in HBM and are freed).  `ctx` supplies the options and
 * reads the header once.  digest folds every partition's digest in partition order: it equals
 * dq_stats.digest of a one-device run of the whole file. */
typedef struct dq_multi_result {
  int32_t n_devices;
  int32_t reserved;
  int64_t n_partitions;
  int64_t n_records;
  int64_t compressed_bytes;    /* file length */
  int64_t decompressed_bytes;  /* sum of the shards' owned bytes (= the file's stream) */
  uint64_t digest;
  double ms_wall;              /* header read + all shards (open, upload, pipeline), host clock */
  double ms_shard_wall_max;    /* slowest shard, host clock */
  double ms_device_max;        /* slowest shard's device pipeline (HIP events) */
} dq_multi_result;
int dq_decode_file_multi(dq_ctx* ctx, const char* path, const int32_t* devices, int32_t n_devices,
                         dq_multi_result* out);

/* The decompressed BAM header (AbstractSamSource.getFileHeader, D/impl/formats/sam/
 * AbstractSamSource.java:32-49) from the first `len` bytes of a file: enough BGZF blocks to hold
 * it (the last one may be cut).  Writes up to cap bytes to out; *out_len = header length.  Used
 * by the multi-GPU path: one rank reads it and broadcasts it to the others' dq_open_shard. */
int dq_header_from_prefix(dq_ctx* ctx, const uint8_t* bytes, int64_t len, uint8_t* out,
                          int64_t cap, int64_t* out_len);

/* .bai bytes for interval traversal (AbstractSamSource.findIndex: path.bai or .bam->.bai). */
int dq_set_index(dq_ctx* ctx, const uint8_t* bai, int64_t len);

int dq_read_header(dq_ctx* ctx, dq_header_info* info, uint8_t* header_bytes, int64_t cap);

/* .sbi splitting index bytes (htsjdk SBIIndex.load, M/htsjdk/samtools/SBIIndex.java:117-165:
 * magic "SBI\1", ascending virtual offsets).  Disq's getPathChunks loads it and then discards the
 * result (D/impl/formats/bam/BamSource.java:69-87), so with use_for_planning = 0 (Disq-exact,
 * the default) it is validated and ignored.  With use_for_planning = 1 dq_plan gives each split
 * the chunk SBIIndex.getChunk(splitStart, splitEnd) returns (SBIIndex.java:244-264: from the
 * first indexed record at or after the split start to the first at or after the split end) and
 * no record guessing runs.  NULL clears it. */
int dq_set_splitting_index(dq_ctx* ctx, const uint8_t* sbi, int64_t len, int32_t use_for_planning);

/* BAMSBIIndexer.createIndex (M/htsjdk/samtools/BAMSBIIndexer.java:45-66) + SBIIndexWriter
 * (SBIIndexWriter.java:84-151) for the open (whole) file: every granularity-th record's virtual
 * offset from the first record, then the final pointer; zero MD5 and UUID.  *out is
 * library-allocated (dq_free); granularity <= 0 means htsjdk's default 4096. */
int dq_write_sbi(dq_ctx* ctx, int64_t granularity, uint8_t** out, int64_t* out_len);

/* BAMIndexer.createIndex for the open (whole) file: the .bai file's bytes (SAMv1 §5.2; the rules
 * are in DESIGN.md "Building the .bai").  A file that is not coordinate sorted, a reference index
 * beyond the header's or an alignment end beyond 2^29 gives DQ_EFORMAT; a shard gives DQ_EINVAL.
 * *out is library-allocated (dq_free); *ms (may be NULL) = device time of the index build
 * alone, after the record pipeline. */
int dq_write_bai(dq_ctx* ctx, uint8_t** out, int64_t* out_len, double* ms);

/* getPathChunks: all splits of the open file, in Disq partition order.  *chunks is
 * library-allocated; free with dq_free. */
int dq_plan(dq_ctx* ctx, dq_chunk** chunks, int64_t* n);

/* getIterator(span): the records of one chunk (start pointer < vend), in file order. */
int dq_decode(dq_ctx* ctx, uint64_t vstart, uint64_t vend, int32_t with_raw, dq_batch** out);

/* BamSource.getIterator(SamReader, SAMFileSpan) as a Spark task runs it (BamSource.java:172-175),
 * with no resident file: reads from `path` only the compressed bytes of the chunk's blocks
 * [vstart >> 16, first block past vend >> 16] plus what the last record needs (the window grows
 * until that record is whole), inflates them and walks the records from the exact start pointer
 * while start < vend.  The file's header is read once per context and path.  Afterwards the
 * context holds no open file (dq_plan / dq_read need an open again).  stats.h2d_bytes
 * (dq_get_stats) reports the compressed bytes copied to the device. */
int dq_decode_chunk(dq_ctx* ctx, const char* path, uint64_t vstart, uint64_t vend, int32_t with_raw,
                    dq_batch** out);

/* createIndexIterator(intervals, contained=false) + the unplaced-unmapped tail for one task
 * (AbstractBinarySamSource.java:86-134) with no resident file: the .bai span of the optimized
 * intervals (dq_set_index first) clipped to the chunk is the only part of `path` read -- span
 * chunks closer than 1 MiB are read as one window, each decoded from its exact start pointer --
 * then kernel 4 keeps the overlapping records; if the chunk holds the .bai's start of the last
 * linear bin and traverse_unplaced_unmapped is set, the records with refID -1 from there to EOF
 * follow (queryUnmapped).  One partition in the batch. */
int dq_decode_chunk_filtered(dq_ctx* ctx, const char* path, uint64_t vstart, uint64_t vend,
                             const dq_traversal* tr, int32_t with_raw, dq_batch** out);

/* createIndexIterator(intervals, contained=false) over one chunk, plus the unplaced-unmapped
 * tail when the chunk contains the .bai's start of the last linear bin. */
int dq_decode_filtered(dq_ctx* ctx, uint64_t vstart, uint64_t vend, const dq_traversal* tr,
                       int32_t with_raw, dq_batch** out);

/* getReads for the whole file: every partition, in order (tr may be NULL). */
int dq_read(dq_ctx* ctx, const dq_traversal* tr, int32_t with_raw, dq_batch** out);

/* Run the whole device pipeline on the resident file without copying records back (records
 * stay in HBM); fills stats.  This is the benchmark entry point.  With intervals in tr (needs
 * dq_set_index, as createIndexIterator does; AbstractBinarySamSource.java:86-112), the traversal
 * of every partition as Disq runs it: the .bai span of the optimized intervals clipped to each
 * partition chunk is the only part of the file inflated (the partition plans come from a full run
 * of the open file, made first if there is none); records of the spans are filtered by kernel 4
 * (overlap, contained=false).  stats.n_records = records in the spans, stats.n_filtered = kept,
 * stats.blocks_inflated, stats.ms_span; dq_partition_digests gives the kept count and digest per
 * partition.  With opts.full_traversal, or traverse_unplaced_unmapped, every record of the file is
 * filtered instead (stats.ms_filter; the unplaced tail is not included). */
int dq_run_resident(dq_ctx* ctx, const dq_traversal* tr, dq_stats* stats);

/* Stats of the last pipeline run (the ones dq_run_resident returns). */
int dq_get_stats(dq_ctx* ctx, dq_stats* stats);

/* Per-partition record counts and digests of the last pipeline run, in partition order (the
 * shard's partitions p0..p1-1 for a shard): *n = number of partitions; up to cap entries written.
 * The whole-file digest folds them. */
int dq_partition_digests(dq_ctx* ctx, int64_t* counts, uint64_t* digests, int64_t cap, int64_t* n);

/* Device pointer of the resident decompressed stream (for tests), and its length. */
int dq_debug_inflated(dq_ctx* ctx, uint8_t* host_out, int64_t cap, int64_t* len);

/* Test hook: the GPU record guesser (BamRecordGuesser.checkRecordStart) evaluated at EVERY
 * decompressed position of a whole resident file, as BamRecordGuesserChecker does with a
 * granularity-1 index (D/impl/formats/bam/BamRecordGuesserChecker.java:104-120).  Writes the
 * virtual offsets where it fires, ascending, up to cap; *n = how many there are. */
int dq_debug_guess_all(dq_ctx* ctx, uint64_t* voffs, int64_t cap, int64_t* n);

/* ---- BGZF text (VCF) path ----------------------------------
 * Replaces, for a BGZF-compressed text file, Hadoop's TextInputFormat record reader running over
 * Disq's splittable codecs: BGZFCodec / BGZFEnhancedGzipCodec.createInputStream
 * (D/impl/formats/bgzf/BGZFCodec.java:57-68, BGZFEnhancedGzipCodec.java:41-74) and
 * BGZFSplitCompressionInputStream (BGZFSplitCompressionInputStream.java:14-106) under Hadoop 2.7
 * LineRecordReader, as VcfSource.getVariants uses them (D/impl/formats/vcf/VcfSource.java:88-113).
 * A partition is one FileInputFormat split (same arithmetic as the BAM path); its lines are the
 * values LineRecordReader returns, terminators excluded; drop_header_lines drops the values
 * starting with '#' (VcfSource.java:108).  Parsing a line into a VariantContext is dq_vcf_read's. */
typedef struct dq_text_batch {
  int64_t n_lines;
  int64_t* line_offset;   /* value offset in the file's decompressed stream */
  int32_t* line_len;      /* value length in bytes */
  uint64_t* hash;         /* hash of the value bytes (same function as the record hash) */
  int64_t* data_offset;   /* value k = data[data_offset[k], data_offset[k] + line_len[k]) */
  uint8_t* data;
  int64_t n_bytes;
  int64_t n_partitions;
  int64_t* part_offset;   /* lines of partition p: [part_offset[p], part_offset[p + 1]) */
  uint64_t* part_digest;  /* ordered digest of the partition's line hashes */
} dq_text_batch;

int dq_text_open_memory(dq_ctx* ctx, const uint8_t* bytes, int64_t len);
/* VcfSource.getVariants with intervals (D/impl/formats/vcf/VcfSource.java:88-113, 144-168): the
 * tabix index (the DECOMPRESSED bytes of the .tbi; NULL clears) and the intervals (contig names,
 * 1-based closed starts and ends; contig == NULL or n < 0 clears, n == 0 keeps nothing).  With
 * intervals set, dq_text_run / dq_text_read keep only the splits whose [start, end] overlaps an
 * index block of some interval (TribbleIndexIntervalFilteringTextInputFormat.getSplits) and only
 * the lines whose variant (CHROM, POS .. POS + len(REF) - 1 or INFO END) overlaps an interval
 * (OverlapDetector.overlapsAny); '#' lines are always dropped then.  stats.n_partitions counts
 * the kept splits. */
int dq_text_set_index(dq_ctx* ctx, const uint8_t* tbi, int64_t len);
int dq_text_set_intervals(dq_ctx* ctx, const char* const* contig, const int32_t* start,
                          const int32_t* end, int64_t n);
int dq_text_open_path(dq_ctx* ctx, const char* path);
/* Scan, inflate, line planning and digests; the lines stay in HBM.  stats: n_records = lines
 * kept, n_filtered = '#' lines dropped, digest = whole-file digest of the partition digests. */
int dq_text_run(dq_ctx* ctx, int32_t drop_header_lines, dq_stats* stats);
int dq_text_read(dq_ctx* ctx, int32_t drop_header_lines, dq_text_batch** out);
void dq_text_batch_free(dq_text_batch* b);
/* htsjdk TabixIndexCreator for the open (whole) VCF text file: the DECOMPRESSED tabix bytes, the
 * form dq_text_set_index takes (a .tbi on disk is these bytes as a BGZF file; the rules are in
 * DESIGN.md "Building the .tbi").  Every data line of the file is indexed exactly once, whatever
 * split_size, use_nio, a set index or set intervals say; the context reads as before afterwards.
 * A data line that is not a VCF record, a POS below 1 or an end beyond 2^29, or a file that is
 * not sorted (POS going down inside a contig, a contig coming back) gives DQ_EFORMAT naming the
 * first offender's 0-based line index; no open text file gives DQ_EINVAL.  *out is
 * library-allocated (dq_free); *ms (may be NULL) = device time of the index build alone, after
 * scan, inflate and the terminator scan. */
int dq_text_write_tbi(dq_ctx* ctx, uint8_t** out, int64_t* out_len, double* ms);

/* ---- VCF site decode: VCFCodec.decode --------------------------
 * Every data line of an open text context (dq_text_open_*; a set index and set intervals are
 * honoured) decoded on the device into the site fields htsjdk's AbstractVCFCodec.parseVCFLine
 * computes eagerly; genotypes stay text, as htsjdk's LazyGenotypesContext leaves them.  The rules
 * are DESIGN.md section 15.  The variants are exactly the lines dq_text_read(ctx, 1, ...) returns:
 * partitions, offsets, lengths, hashes and digests are the same.  The header is the stream's
 * leading '#' lines: the ##contig IDs (contig indexes them, -1 for a CHROM that names none) and
 * the #CHROM line, which decides whether lines carry genotype columns; data lines without a #CHROM
 * line give DQ_EFORMAT "VCF header: no #CHROM line".  Every line of the kept splits that does not
 * start with '#' is validated, before the interval filter (Disq decodes, then filters): a malformed
 * one gives DQ_EFORMAT and dq_last_error "VCF line <k>: <what>", k the 0-based index of the first
 * offender among all the file's lines, what one of fields, CHROM, POS, ID, REF, ALT, QUAL, FILTER,
 * INFO.  A BAM or SAM context, no open file or an unknown mode gives DQ_EINVAL.  The dq_text_*
 * calls work as before on the same context afterwards. */
#define DQ_VCF_EXPORT_FIELDS 0   /* columns only, data = NULL */
#define DQ_VCF_EXPORT_SITES  1   /* + each variant's first col_end[7] bytes (columns 1-8) */
#define DQ_VCF_EXPORT_LINES  2   /* + each variant's whole value, as dq_text_read gives it */
/* flags */
#define DQ_VCF_HAS_ID 1
#define DQ_VCF_HAS_QUAL 2
#define DQ_VCF_UNFILTERED 4      /* FILTER "." */
#define DQ_VCF_PASS 8
#define DQ_VCF_INFO_END 16       /* end came from INFO END */
#define DQ_VCF_HAS_GENOTYPES 32  /* a 9th column exists */
#define DQ_VCF_SYMBOLIC 64       /* some ALT is symbolic or a breakend */
#define DQ_VCF_REF_LOWER 128     /* REF holds a lower-case base (htsjdk upper-cases it) */
typedef struct dq_variant_batch {
  int64_t n_variants;
  int64_t* line_offset;    /* exactly dq_text_batch's line_offset, line_len and hash */
  int32_t* line_len;
  uint64_t* hash;
  int32_t* contig;         /* index of the ##contig line whose ID is CHROM, or -1 */
  int32_t* pos;            /* POS */
  int32_t* end;            /* the INFO END value, or POS + len(REF) - 1 */
  uint32_t* flags;         /* DQ_VCF_* */
  double* qual;            /* the QUAL text's binary64 (0 without DQ_VCF_HAS_QUAL) */
  int32_t* col_end;        /* 8 per variant: column c = [c ? col_end[8k+c-1]+1 : 0, col_end[8k+c]) */
  int32_t* n_alt;
  int32_t* n_filter;       /* 0 for "." and PASS */
  int32_t* n_info;         /* 0 for "." */
  int32_t* n_sample_cols;  /* columns after FORMAT */
  int64_t* data_offset;    /* variant k's bytes = data[data_offset[k] ...) (SITES, LINES) */
  uint8_t* data;
  int64_t n_bytes;
  int64_t n_partitions;
  int64_t* part_offset;    /* as dq_text_read(ctx, 1, ...) */
  uint64_t* part_digest;
  int32_t n_contigs;
  int32_t reserved;
  int32_t* contig_name_off; /* n_contigs + 1 offsets into contig_names */
  uint8_t* contig_names;
  int64_t n_qual_host;     /* QUAL texts off the device's exact path, converted by the host's strtod */
} dq_variant_batch;
/* The text run, then validate and decode; the columns stay in HBM.  stats: dq_text_run's, with
 * ms_records = the device time of validate + decode (the text run's own ms_records, its values,
 * hashes and digests, is added to ms_plan) and ms_total including it. */
int dq_vcf_run(dq_ctx* ctx, dq_stats* stats);
int dq_vcf_read(dq_ctx* ctx, int32_t mode, dq_variant_batch** out);
void dq_variant_batch_free(dq_variant_batch* b);

/* ---- VCF genotype decode: createGenotypeMap -------------------
 * The FORMAT column and the sample columns of the variants of dq_vcf_read on the same context --
 * the same lines in the same order and partitions, after the same tabix pruning and overlap filter
 * -- decoded on the device into a dense variants x samples matrix: what htsjdk's
 * AbstractVCFCodec.createGenotypeMap / parseGenotypeAlleles compute when a consumer asks a
 * VariantContext for its genotypes.  The rules are DESIGN.md section 16.  S, the sample count, is 0
 * for a header without a sample (not an error: empty arrays), else the number of columns of the
 * #CHROM line behind the ninth with trailing empty ones dropped.  GT, GQ, DP and FT are read; the
 * other keys' text is reached through cell_off.  Both calls run the site decode first when the
 * context has not (its errors come first, unchanged); then only the variants handed out are
 * checked, as htsjdk parses genotypes lazily: the first failing check gives DQ_EFORMAT and
 * dq_last_error "VCF line <k>: samples", "VCF line <k>: FORMAT" or
 * "VCF line <k>: sample <s>: <GT|GQ|DP|cell>", k as dq_vcf_read counts lines and the lowest
 * offender, s the lowest offending 0-based sample of that line.  dq_vcf_read and the dq_text_*
 * calls work on the same context afterwards.  A BAM or SAM context or no open file gives DQ_EINVAL,
 * a matrix that does not fit DQ_ENOMEM. */
#define DQ_GT_HAS_GT 1      /* the first FORMAT key is GT and the cell has a value for it */
#define DQ_GT_PHASED 2
#define DQ_GT_HAS_GQ 4
#define DQ_GT_HAS_DP 8
#define DQ_GT_FILTERED 16   /* an FT value that is neither "." nor "PASS" */
typedef struct dq_genotype_batch {
  int64_t n_variants;      /* = dq_vcf_read's, row k is its variant k */
  int32_t n_samples;       /* S */
  int32_t max_ploidy;      /* P: the largest ploidy of any cell, at least 1 when S > 0 */
  uint8_t* flags;          /* [n_variants * S], row-major by variant */
  uint8_t* ploidy;         /* [n_variants * S] */
  int16_t* allele;         /* [n_variants * S * P]: allele index, -1 no-call, -2 past the cell's ploidy */
  int32_t* gq;             /* [n_variants * S], -1 when missing */
  int32_t* dp;             /* [n_variants * S], -1 when missing */
  int32_t* cell_off;       /* [n_variants * S]: offset of the sample column's first byte in the line's
                              value (it ends at the next one's offset - 1, the last at line_len) */
  int32_t* sample_name_off; uint8_t* sample_names;   /* S + 1 offsets */
  int64_t n_partitions; int64_t* part_offset;        /* as dq_vcf_read */
  int64_t n_gq_host;       /* GQ texts off the device's digit path, converted by the host's strtod */
} dq_genotype_batch;
/* The site decode when the context has not run it, then the genotype check and decode passes; the
 * matrix stays in HBM.  stats: dq_vcf_run's, with the device time of the two genotype passes added
 * to ms_records (so ms_records = site validate + decode + genotype check + decode) and to
 * ms_total. */
int dq_vcf_genotypes_run(dq_ctx* ctx, dq_stats* stats);
int dq_vcf_genotypes(dq_ctx* ctx, dq_genotype_batch** out);
void dq_genotype_batch_free(dq_genotype_batch* b);

/* ---- VCF INFO decode: parseInfo projected onto keys -----------
 * The INFO column of the variants of dq_vcf_read on the same context -- the same lines in the same
 * order and partitions, after the same tabix pruning and overlap filter -- decoded on the device
 * into one typed column block per requested key (1 to 64 keys): what htsjdk's
 * AbstractVCFCodec.parseInfo leaves in the attribute map for those keys.  The rules are DESIGN.md
 * section 17.  The column splits on ';', a key is the text before a piece's first '=' and matches a
 * requested id byte for byte; the first piece of a key is decoded and a later one only sets
 * DQ_INFO_REPEATED.  "key=" and "key=." are present without a value; a key the header types as Flag
 * with the value "0" is absent (htsjdk's "DB=0").  An explicit type overrides the header's only for
 * how values are converted.  INTEGER elements are '.' (missing) or [-+]?[0-9]+ in int32; FLOAT
 * elements are '.', the QUAL grammar, NaN, Infinity, +Infinity or -Infinity; an empty element is an
 * error for both; FLAG and STRING values are not converted, their span (val_off, val_len, into the
 * line's value, so into a SITES or LINES export of dq_vcf_read) is the access path.
 * Both calls run the site decode first when the context has not (its errors come first,
 * unchanged); then only the variants handed out are checked: the first failing value gives
 * DQ_EFORMAT and dq_last_error "VCF line <k>: INFO <id>", k as dq_vcf_read counts lines and the
 * lowest offender, then the lowest index in keys.  dq_vcf_read, dq_vcf_genotypes and the dq_text_*
 * calls work on the same context afterwards.  DQ_EINVAL: a BAM or SAM context, no open file,
 * n_keys < 1 or > 64, an id that is empty or holds ';', '=', ',', a TAB or a space, the same id
 * twice, an unknown type.  DQ_ENOMEM: the columns do not fit.
 * Not done: Number= checks, VCF 4.3 percent-decoding, the last-wins order of htsjdk's map, keys
 * that were not asked for, copies of String values, BCF. */
#define DQ_INFO_AUTO 0      /* take Type from the header's ##INFO line; no such line: STRING */
#define DQ_INFO_FLAG 1
#define DQ_INFO_INTEGER 2
#define DQ_INFO_FLOAT 3
#define DQ_INFO_STRING 4    /* also Character: the span only */
/* cell flags */
#define DQ_INFO_PRESENT 1   /* the key is in the line's INFO map */
#define DQ_INFO_HAS_VALUE 2 /* it has a value text that is not empty and not "." */
#define DQ_INFO_REPEATED 4  /* the key occurs again later in the line (the first is decoded) */
#define DQ_INFO_I_MISSING INT32_MIN
#define DQ_INFO_F_MISSING_BITS 0x7ff8000000000001ULL /* a quiet NaN with payload 1; "NaN" itself is 0x7ff8000000000000 */
typedef struct dq_info_key { const char* id; int32_t type; int32_t reserved; } dq_info_key;
typedef struct dq_info_batch {
  int64_t n_variants;          /* = dq_vcf_read's; row k is its variant k */
  int32_t n_keys;              /* K */
  int32_t reserved;
  int32_t* key_type;           /* [K] the resolved DQ_INFO_* (never AUTO) */
  int32_t* key_width;          /* [K] W_q: the largest value count of key q over the rows, at least 1 */
  int64_t* key_base;           /* [K] element offset of key q's block in ival (INTEGER) or fval (FLOAT), -1 otherwise */
  uint8_t* flags;              /* [K * n_variants], key-major: cell (q, k) at q * n_variants + k */
  int32_t* n_values;           /* [K * n_variants] ',' pieces of the value text; 0 without HAS_VALUE */
  int32_t* val_off;            /* [K * n_variants] offset of the value text in the line's value, -1 when absent */
  int32_t* val_len;            /* [K * n_variants] */
  int32_t* ival;  int64_t n_ival;  /* value j of (q, k) at key_base[q] + k * W_q + j; INT32_MIN = missing */
  double*  fval;  int64_t n_fval;  /* the same; NaN with payload 1 = missing (DQ_INFO_F_MISSING_BITS) */
  int64_t n_partitions; int64_t* part_offset;   /* as dq_vcf_read */
  int64_t n_float_host;        /* Float texts off the device's exact path, converted by the host's strtod */
} dq_info_batch;
/* The site decode when the context has not run it, then the INFO check and decode passes for these
 * keys; the columns stay in HBM.  stats: dq_vcf_run's, with the device time of the two INFO passes
 * added to ms_records and to ms_total. */
int dq_vcf_info_run(dq_ctx* ctx, const dq_info_key* keys, int32_t n_keys, dq_stats* stats);
int dq_vcf_info(dq_ctx* ctx, const dq_info_key* keys, int32_t n_keys, dq_info_batch** out);
void dq_info_batch_free(dq_info_batch* b);

/* ---- SAM text: SamSource.getReads -----------------------------
 * An uncompressed SAM file read as Disq reads it (D/impl/formats/sam/SamSource.java:36-77): Hadoop
 * TextInputFormat lines per split of PathSplitSource.getPathSplits (a line whose first byte is at s
 * belongs to the split with start < s <= end, offset 0 to the first; LF, CR LF and a lone CR end a
 * line; a UTF-8 BOM is dropped from the first value), '@' lines dropped wherever they stand, every
 * other line through htsjdk SAMLineParser.parseLine and encoded as BAMRecordCodec encodes it.  The
 * rules are DESIGN.md section 13.  After an open the context holds the BAM header built from the
 * leading '@' lines (BAM\1, l_text, each line followed by LF, n_ref, per @SQ l_name, name, NUL, LN):
 * dq_read_header returns it.  dq_sam_run leaves the records in HBM; stats: compressed_bytes =
 * decompressed_bytes = the file's length, n_blocks = 0, n_records, n_partitions (every split is a
 * partition, one in which no line starts an empty one), n_filtered = '@' lines dropped, digest as
 * dq_text_run folds it, ms_plan / ms_records / ms_total; dq_get_stats and dq_partition_digests work
 * after a run.  dq_sam_read returns an ordinary dq_batch (every export mode, the export arena,
 * dq_batch_free): raw = the BAM records' bytes, hash = the hash the BAM path gives the same record,
 * voffset = the offset of the line's first byte in the file (SAM text has no virtual offsets),
 * part_offset / part_digest per split.  A malformed line gives DQ_EFORMAT and dq_last_error
 * "SAM line <k>: <what>": k = the 0-based index of the first offending line in file order, counted
 * over all lines; what = fields, QNAME, FLAG, RNAME, POS, MAPQ, CIGAR, RNEXT, PNEXT, TLEN, SEQ, QUAL
 * or "tag XX".  A BAM or text call on a SAM context, and dq_sam_run / dq_sam_read on any other,
 * give DQ_EINVAL.
 * Out of scope: interval traversal of SAM (no traversal argument), htsjdk's LENIENT / SILENT
 * tolerance of malformed lines (the rules hold whatever dq_opts.stringency says), uncompressed
 * .vcf input, sharded and multi-GPU SAM. */
int dq_sam_open_memory(dq_ctx* ctx, const uint8_t* text, int64_t len);
int dq_sam_open_path(dq_ctx* ctx, const char* path);
int dq_sam_run(dq_ctx* ctx, dq_stats* stats); /* records stay in HBM */
int dq_sam_read(dq_ctx* ctx, int32_t with_raw, dq_batch** out);

/* ---- SAM output: SamSink.save's part file (row f8) --------------------------------------------
 * Records into SAM lines as htsjdk 2.16 SAMTextWriter.getSAMString and TextTagCodec print them,
 * each trimmed as Java's String.trim does (bytes <= 0x20 at both ends) and followed by LF.  The
 * rules are DESIGN.md section 14; floats print as Float.toString does under the JDK 19+ contract.
 * A malformed record gives DQ_EFORMAT and dq_last_error "record <k>: <what>": k = the 0-based
 * index of the first offending record in input order; what = the first failing check of fields
 * (the layout), QNAME, RNAME, CIGAR, RNEXT, QUAL, "tag XX" in that order.  A single line longer
 * than 2^31-1 bytes gives DQ_EINVAL; offsets are 64-bit throughout.
 * Out of scope: CRAM, one file per partition (AnySamSinkMultiple), a header re-encoded from a
 * parsed SAMFileHeader, JDK 8's longer float texts, sharded and multi-GPU SAM output.
 *
 * dq_sam_write: header = the BAM header (dq_read_header's bytes; its references name RNAME/RNEXT).
 * raw = n_records records back to back; raw_offset (may be NULL: the host walks the block_size
 * chain) as dq_batch gives it.  n_records == 0 gives an empty output.  A chain that breaks at
 * record k, or does not end exactly at raw_len (k = n_records), gives "record <k>: fields" unless
 * an earlier record fails. */
int dq_sam_write(dq_ctx* ctx, const uint8_t* header, int64_t header_len, const uint8_t* raw,
                 int64_t raw_len, const int64_t* raw_offset, int64_t n_records, uint8_t** out,
                 int64_t* out_len); /* *out: dq_free */
/* Every record of the open whole file, once, in file order (a BAM context: the index-only run
 * dq_write_bai makes; a SAM context: the records of dq_sam_run).  The text stays in HBM;
 * dq_sam_write_fetch copies it out.  *ms (may be NULL) = device time of the size pass, the scan and
 * the format pass.  A shard, a text (VCF) context, or no open file give DQ_EINVAL.  The context
 * reads as before afterwards, as after dq_write_bai. */
int dq_sam_write_resident(dq_ctx* ctx, int64_t* out_len, double* ms);
int dq_sam_write_fetch(dq_ctx* ctx, uint8_t* host_out, int64_t cap);

/* ---- BAM aux tags projected onto keys -------------------------
 * The optional fields (SAMv1 section 4.2.4) of the records dq_read(ctx, tr, ...) returns on a BAM
 * context -- the same records in the same order and partitions, whether tr is NULL, carries
 * intervals or asks for the unplaced tail, the records DQ_COMPAT_DISQ_EXACT duplicates across a
 * split boundary included, a shard its own partitions -- or of dq_sam_read's on a SAM context (tr
 * must be NULL), decoded on the device into one column block per requested key (1 to 64 keys): what
 * SAMRecord.getAttribute reads for those keys.  The rules are DESIGN.md section 18.  A record's aux
 * region runs from 36 + l_read_name + 4 * n_cigar + (l_seq + 1) / 2 + l_seq to 4 + block_size; a
 * layout that does not fit is the SAM writer's "fields".  The whole chain is walked and validated
 * with the SAM writer's checks (the bytes a type needs are left in the record, Z and H end in a
 * NUL, H is an even number of hex digits, a B array's element type and count, the type byte is
 * known).  An id is two bytes, [A-Za-z][A-Za-z0-9], matched byte for byte; the first occurrence of
 * a key in a record is decoded and a later one only sets DQ_TAG_REPEATED.
 * Errors: the first failing check of the lowest row, in stored order, gives DQ_EFORMAT and
 * dq_last_error "record <k>: fields", "record <k>: tag XX" (XX as dq_sam_write names it; no name
 * when fewer than three bytes are left) or "record <k>: tag XX type" (a requested key whose first
 * occurrence is stored outside the class asked for); k is the 0-based row.  DQ_EINVAL: a text (VCF)
 * context, no open file, tr on a SAM context, n_keys < 1 or > 64, a bad id, the same id twice, an
 * unknown type, and what dq_read refuses.  DQ_ENOMEM: the columns do not fit.  dq_read,
 * dq_sam_read, dq_write_bai and dq_sam_write_resident work on the same context afterwards.
 * Not done: dense values of B arrays and copies of Z/H text (reached through the span); htsjdk's
 * rule for a tag stored twice in one record is not reproduced (its tag codec's source was not at
 * hand to check it against: here the first occurrence wins and the cell says so); the chunk calls
 * (dq_decode_chunk*), multi-GPU wiring and CRAM. */
#define DQ_TAG_ANY 0     /* any stored type: vtype, subtype and span only, nothing converted */
#define DQ_TAG_INT 1     /* stored c C s S i I  (getIntegerAttribute and friends) */
#define DQ_TAG_FLOAT 2   /* stored f */
#define DQ_TAG_CHAR 3    /* stored A */
#define DQ_TAG_STRING 4  /* stored Z: the span is the access path */
/* cell flags */
#define DQ_TAG_PRESENT 1
#define DQ_TAG_REPEATED 4   /* the tag occurs again later in the record; the first is decoded */
typedef struct dq_tag_key { const char* id; int32_t type; int32_t reserved; } dq_tag_key;
typedef struct dq_tag_batch {
  int64_t n_records;      /* = the batch of dq_read (dq_sam_read); row k is its record k */
  int32_t n_keys;         /* K, 1..64 */
  int32_t reserved;
  int32_t* key_type;      /* [K] as asked */
  int64_t* key_base;      /* [K] element offset of key q's block in val (INT, FLOAT, CHAR), else -1 */
  uint8_t* flags;         /* [K * n], key-major: cell (q, k) at q * n + k */
  uint8_t* vtype;         /* [K * n] stored type byte (A c C s S i I f Z H B), 0 when absent */
  uint8_t* subtype;       /* [K * n] element type of a B array, else 0 */
  int32_t* val_off;       /* [K * n] offset of the value's first payload byte in the record, counted
                             from its block_size word (so raw[raw_offset[k] + val_off]); -1 absent.
                             Z/H: first character; B: first element, behind subtype and count */
  int32_t* val_len;       /* [K * n] payload bytes: Z/H without the NUL, B = element size * count */
  uint32_t* val; int64_t n_val; /* cell (q, k) at key_base[q] + k: INT the value extended to 32 bits as
                             its stored type says (for 'I' the uint32 itself; vtype tells), FLOAT the
                             binary32 bits, CHAR the byte; 0 when absent */
  int64_t n_partitions; int64_t* part_offset;   /* as the record batch */
} dq_tag_batch;
/* The pipeline as dq_read (dq_sam_read) runs it, then the tag check and decode passes for these
 * keys; the columns stay in HBM.  stats: the pipeline's, with the device time of the two tag passes
 * added to ms_records and to ms_total. */
int dq_tags_run(dq_ctx* ctx, const dq_traversal* tr, const dq_tag_key* keys, int32_t n_keys, dq_stats* stats);
int dq_tags(dq_ctx* ctx, const dq_traversal* tr, const dq_tag_key* keys, int32_t n_keys, dq_tag_batch** out);
void dq_tag_batch_free(dq_tag_batch* b);

/* ---- BGZF compression: the write path -----------------------
 * Replaces htsjdk BlockCompressedOutputStream under HeaderlessBamOutputFormat.BamRecordWriter
 * (D/impl/formats/bam/HeaderlessBamOutputFormat.java:26-50) and BamSink's header file
 * (BAMFileWriter.writeHeader, D/impl/formats/bam/BamSink.java:46-50): `data` is cut into blocks
 * of 65280 bytes (htsjdk DEFAULT_UNCOMPRESSED_BLOCK_SIZE, the last one shorter), each compressed
 * on the GPU into one BGZF member ('BC' extra field, BSIZE, CRC32, ISIZE).  No EOF terminator is
 * written (BamSink appends BlockCompressedStreamConstants.EMPTY_GZIP_BLOCK once, after all parts).
 * The DEFLATE bit stream is this library's own (LZ77 + a dynamic Huffman code per block, the
 * fixed code when that is shorter, stored when neither fits): the blocks inflate to exactly
 * htsjdk's block contents; the compressed bytes differ from java.util.zip.Deflater's.  *out is
 * malloc'ed (dq_free). */
int dq_bgzf_compress(dq_ctx* ctx, const uint8_t* data, int64_t len, uint8_t** out, int64_t* out_len);
/* The same over the resident decompressed stream of the open file (benchmark / round trip): the
 * result stays in HBM (dq_bgzf_fetch copies it out); *ms = device time. */
int dq_bgzf_compress_resident(dq_ctx* ctx, int64_t* out_len, double* ms);
int dq_bgzf_fetch(dq_ctx* ctx, uint8_t* host_out, int64_t cap);

/* Export arena: batches of this context (dq_read, dq_decode*) place their arrays in `bytes` of
 * pinned host memory, copied by DMA with no staging copies (a batch that does not fit takes heap
 * memory as before): a streaming consumer's recycled buffers, one Spark task's records at a time.
 * The arena holds ONE batch: while it is alive (until dq_batch_free), a batch that would go to
 * the arena and dq_set_export_arena return DQ_EINVAL, and dq_ctx_destroy leaves the arena to the
 * batch, whose dq_batch_free releases it (per-task ownership with auto-close,
 * AutocloseIteratorWrapper.java:26-36).  bytes = 0 releases the arena. */
int dq_set_export_arena(dq_ctx* ctx, int64_t bytes);
void dq_batch_free(dq_batch* b);
void dq_free(void* p);

/* Debug: the device bounds-checked build (`make -C disq_amd/csrc checked` ->
 * libdisq_gpu_checked.so, compiled with -DDQ_CHECKED).  Writes each kernel unit's failed-check
 * count << 32 | largest reported excess << 16 | site bits (K1/K3 kernels, K2 inflate, text
 * with the SAM reader's, the SAM writer's and the tag decode's units folded in, deflate: 4 words) for the current
 * device and resets them; returns 1 in the checked build, 0 in the product build (words all 0). */
int dq_checked_report(uint64_t words[4]);

#ifdef __cplusplus
}
#endif
#endif
