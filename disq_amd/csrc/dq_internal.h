// dq_internal.h -- shared device helpers and kernel launch wrappers of libdisq_gpu.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ------------------------------------------------------------------ status codes (per block/record)
enum : int32_t {
  ST_OK = 0,
  ST_BAD_HEADER = 1,      // BGZF header: not 1f 8b 08 04 / XLEN != 6 (htsjdk BlockGunzipper)
  ST_BAD_BLOCKTYPE = 2,
  ST_BAD_STORED = 3,
  ST_BAD_TABLE = 4,       // over-subscribed / incomplete Huffman code, bad header counts
  ST_BAD_CODE = 5,        // invalid literal/length/distance code
  ST_BAD_DIST = 6,        // distance too far back
  ST_SHORT = 7,           // "Did not inflate expected amount"
  ST_OVERREAD = 8,        // read past the block's deflate data
  ST_CRC = 9,             // CRC32 mismatch (verify_crc)
  ST_ISIZE = 10,          // ISIZE > 65536
  ST_HANG = 11,           // internal: batch loop made no progress
  ST_TEXT_START = 12,     // text split: no block start in the split and none at its end
};

// ------------------------------------------------------------------ DQ_CHECKED
// The device bounds-checked build (`make -C disq_amd/csrc checked` -> libdisq_gpu_checked.so, picked
// up through DQ_GPU_LIB): DQ_CHK(cond, site) counts a failed check and sets bit `site` in this
// translation unit's check words; the access itself goes ahead unchanged (the checks observe the
// kernels, they do not alter them, and nothing traps: a trap would take the GPU down with it).
// dq_checked_report (dq_api.hip) collects every unit's words after a run.  In the product build
// DQ_CHK compiles to nothing.
enum : int {
  CHK_K1_SLOT = 0,   // K1: a candidate's slot outside its chunk's CAP slots; a chain window's block
                     //     outside the block table
  CHK_K2_BITS = 1,   // K2: the bit reader loads a word past the member's deflate data (+ slack);
                     // the header pre-pass asks for a word outside its lane's window
  CHK_K2_IMAGE = 2,  // K2: an emit / stored-copy store outside the LDS output image
  CHK_K2_TABLE = 3,  // K2: a second-level table read outside its alphabet's area
  CHK_K2_LANES = 4,  // K2: per-lane arrays / redo list outside the image tail; the header pre-pass
                     //     stores length words outside its lane's record
  CHK_K2_BM = 5,     // K2: a match-start bitmap word outside the bitmap, or a resolve group of four
                     //     bytes whose start bits are not 0, 1, 2, 4, 8 or 9 (matches are >= 3 long)
  CHK_K2_NXT = 6,    // K2: a resolve next pointer outside the batch window
  CHK_K2_SRC = 7,    // K2: a resolve copy source outside [0, isize)
  CHK_K3_STAGE = 8,  // K3: a record's staged bytes (or their reads) outside the LDS staging
  CHK_K2_LAST = 9,   // K2: a last_start index outside the table
  CHK_Z_BL = 10,     // deflate: a bucket-list slot outside the chunk's position list
  CHK_Z_STAGE = 11,  // deflate: a staged symbol word outside its lane's staging
  CHK_Z_IMAGE = 12,  // deflate: an emitted word outside the LDS deflate image
  CHK_K3_SPEC = 13,  // K3: the LDS-filtered segment speculation differs from seg_spec_kernel<64>
  CHK_BAI = 14,      // .bai build: a linear window, perm slot, chunk or bin outside its table
  CHK_TBI = 15,      // .tbi build: a data-line slot, block, run or name byte outside its table
  CHK_SAM = 15,      // SAM read and write and the tag decode (dq_sam.hip, dq_samw.hip, dq_tags.hip share
                     //     the bit): a line, size, record-byte, line-byte or fix-up slot; a tag row,
                     //     key or value slot
  CHK_VCF = 15,      // VCF site, genotype and INFO decode (dq_vcf.hip, dq_vcf_gt.hip, dq_vcf_info.hip
                     //     share the bit): a line, column row, matrix or INFO cell, LDS offset slot,
                     //     fix-up slot or site byte
};
#ifdef DQ_CHECKED
namespace {
// failed checks, OR of their site bits, the largest excess a failed check reported (this unit)
__device__ unsigned int g_dq_chk[3];
}
#define DQ_CHKV(cond, site, excess)                              \
  do {                                                           \
    if (__builtin_expect(!(cond), 0)) {                          \
      atomicAdd(&g_dq_chk[0], 1u);                               \
      atomicOr(&g_dq_chk[1], 1u << (site));                      \
      atomicMax(&g_dq_chk[2], (unsigned int)(excess));           \
    }                                                            \
  } while (0)
#define DQ_CHK(cond, site) DQ_CHKV(cond, site, 0)
// Host: this unit's words (count << 32 | excess << 16 | site bits), reset; the current device.
#define DQ_CHK_UNIT(name)                                                              \
  uint64_t dq_chk_take_##name() {                                                      \
    unsigned int w[3] = {0, 0, 0}, z[3] = {0, 0, 0};                                   \
    if (hipMemcpyFromSymbol(w, HIP_SYMBOL(g_dq_chk), sizeof w) != hipSuccess) return ~0ull; \
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_dq_chk), z, sizeof z);                        \
    return (uint64_t)w[0] << 32 | (uint64_t)(w[2] & 0xffff) << 16 | (w[1] & 0xffff); \
  }
#else
#define DQ_CHKV(cond, site, excess) ((void)0)
#define DQ_CHK(cond, site) ((void)0)
#define DQ_CHK_UNIT(name) \
  uint64_t dq_chk_take_##name() { return 0; }
#endif

// the name table the SAM and VCF kernels take (dqt::NameTable); a unit that wants the lookup's
// bound counted defines DQT_CHECK before it includes this header
#include "dq_text_core.h"
#include "dq_chain_core.h"

// ------------------------------------------------------------------ hashing
__host__ __device__ inline uint64_t dq_mix64(uint64_t z) {
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ULL;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBULL;
  z ^= z >> 31;
  return z;
}
#define DQ_K_LEN 0x9E3779B97F4A7C15ULL
#define DQ_K_WORD 0xD6E8FEB86659FD93ULL

// ------------------------------------------------------------------ launch wrappers
// All pointers are device pointers; all launches go on `s`.
namespace dq {

using dqc::Cand;      // a BgzfBlockGuesser-visible magic position (dq_chain_core.h)
using dqc::ChainWin;

constexpr int SCAN_CHUNK = 16384;  // bytes of C per scan workgroup
constexpr int SCAN_CAP = 32;       // candidate slots per chunk in the first scan pass
constexpr int SCAN_CAP_BIG = 640;  // slots of a re-scanned chunk (BGZF members are >= 28 bytes)
constexpr int SCAN_OVER_MAX = 1 << 22;  // chunks the second pass can take

// Kernel 1, the block chain by windows of W bytes (dq_chain_core.h; W a multiple of 16).  The chain
// start *d_cstart is 0, or for a shard (find_start) the first position from byte 0 that the
// guesser returns (L if none).
void launch_chain_start(const uint8_t* C, int64_t L, int32_t find_start, unsigned long long* d_cstart,
                        hipStream_t s);
// Speculate, walk and link the nwin >= ceil(L / W) windows, repair broken links, and leave
// tot[0] = the block count, tot[1] = the sum of ISIZE; counts[w] = window w's blocks.  d_dense
// (or nullptr): set, and the results void, when a window's members are under 1 KiB on average --
// the caller then cuts the file into finer windows.
void launch_chain_windows(const uint8_t* C, int64_t L, const unsigned long long* d_cstart,
                          ChainWin* wins, int64_t nwin, int64_t W, int32_t* d_dense, uint16_t* hops,
                          int32_t* d_broken, int32_t* counts, unsigned long long* tot, hipStream_t s);
// The block table from the walked windows (base: exclusive scan of counts; cap entries).  hops (or
// nullptr, in both calls): CHAIN_HOPS 16-bit member sizes per window that the count pass records and
// the emit pass takes instead of walking again.
constexpr int CHAIN_HOPS = 128;
void launch_chain_emit(const uint8_t* C, int64_t L, const unsigned long long* d_cstart,
                       const ChainWin* wins, int64_t nwin, int64_t W, const uint16_t* hops,
                       const int64_t* base, int64_t* blk_pos, int32_t* blk_csize, int32_t* blk_usize,
                       int64_t cap, hipStream_t s);

// BGZF candidate scan of C[0, n) (file offsets; L = readable bytes) for the planners.  Writes each
// chunk's candidates sorted into slots[chunk * SCAN_CAP ...] and its count.
void launch_bgzf_scan(const uint8_t* C, int64_t n, int64_t L, Cand* slots, int64_t cap,
                      int32_t* chunk_counts, int64_t n_chunks, int64_t* d_count,
                      int32_t* over_list, hipStream_t s);
// Pass over the n_over chunks listed in over_list[1..], SCAN_CAP_BIG slots each (over_list[0] = -1
// when one holds more).  With over_map the count goes to chunk_counts[chunk] and
// over_map[chunk] = the chunk's place in the list (the full scan's second pass over chunks with
// more than SCAN_CAP hits); without, to chunk_counts[place] (the planners' listed chunks).
void launch_bgzf_scan_listed(const uint8_t* C, int64_t n, int64_t L, Cand* big, int64_t n_over,
                             int32_t* chunk_counts, int32_t* over_list, int32_t* over_map,
                             hipStream_t s);
// out[offs[ch] + i] = chunk ch's i-th candidate: from big + over_map[ch] * SCAN_CAP_BIG where
// over_map lists it, else from slots + ch * stride.
void launch_gather_slots(const Cand* slots, int64_t stride, const int32_t* counts, const int64_t* offs,
                         int64_t nchunks, Cand* out, int64_t cap, const int32_t* over_map,
                         const Cand* big, hipStream_t s);
// out[0] = the first block index (through sel when given) whose status is not ST_OK.
void launch_first_bad(const int32_t* status, const int32_t* sel, int64_t n, unsigned long long* out,
                      hipStream_t s);
// Exclusive prefix sums; out has n + 1 entries (out[n] = total).  tmp >= 4*ceil(n/1024)+256.
void launch_exclusive_scan_i32(const int32_t* in, int64_t* out, int64_t n, int64_t* tmp,
                               hipStream_t s);
void launch_exclusive_scan_i64(const int64_t* in, int64_t* out, int64_t n, int64_t* tmp,
                               hipStream_t s);

// Kernel 2: fused inflate + CRC32, one workgroup per block (dq_inflate3.hip).  The CRC tables
// live in each device's memory: inflate3_tables(device) initialises them once per device (thread
// safe) and returns that device's table of x^(8n) * ~0 mod P, n = 0..65536 (nullptr on failure).
const uint32_t* inflate3_tables(int device);
// scratch: INFLATE_SCRATCH_BYTES of device memory per launched block (16-byte aligned): the tail
// kernel's descriptors (16 bytes each), then the header pre-pass's records (16 bytes, 32 bytes of
// code-length counts and the 320 code lengths as nibbles each); nullptr: the block kernel decodes
// every deflate block itself.
// tim (DQ_TIMING, else nullptr): INFLATE_TIM_WORDS 64-bit words per launched block, zero filled
constexpr size_t INFLATE_SCRATCH_BYTES = 16 + (16 + 32) + 160;
constexpr size_t INFLATE_TIM_WORDS = 64;  // 32 per block, 16 per tail, 16 per 64 blocks of the pre-pass
void launch_inflate3(const uint8_t* C, const int64_t* blk_pos, const int32_t* blk_csize,
                     const int32_t* blk_usize, const int64_t* uoff, int64_t nblk, uint8_t* U,
                     int32_t* status, int32_t verify_crc, const uint32_t* crc_init, uint64_t* tim,
                     hipStream_t s, const int32_t* sel, int64_t nsel, void* scratch);

// out[0] = sum of (csize - 26) over the blocks; out[1] / out[2] = uoff of the first block starting
// after / at or after x (ulen if none); out[3] = the index of the first block starting after x.
void launch_block_stats(const int64_t* blk_pos, const int32_t* blk_cs, const int64_t* uoff,
                        int64_t nblk, int64_t ulen, int64_t x, uint64_t* out, hipStream_t s);

// Split planning (a2-a4).
constexpr int64_t SPLIT_FROM_SBI = -2;  // SplitPlan.first_blk of a chunk taken from a .sbi
struct SplitPlan {
  int64_t split_start, split_end;
  int64_t first_blk;     // chain index of the first guessed block (-1 none)
  int64_t u_lo, u_hi;    // linear U range scanned by the guesser
  int64_t rec_lin;       // linear U offset of the first record (-1 = empty partition)
  uint64_t vstart, vend;
  int32_t status;        // 0 ok; 100 = needs more data; else error
  int32_t rec_span;      // bytes of the <= 10 records chained from rec_lin (segment sizing)
};
// The planners' candidate list: cand[0, *d_ncand) covers the nrng byte ranges rng (nullptr: the
// whole file); *need_full is set when a planner needs a position outside them.
struct CandList {
  const Cand* cand;
  const int64_t* d_ncand;
  const int64_t* rng;
  int64_t nrng;
  int64_t L;
  int32_t* need_full;
};
void launch_plan_blocks(CandList cl, const int64_t* blk_pos,
                        const int32_t* blk_usize, const int64_t* uoff, const int64_t* d_nblk,
                        SplitPlan* plans, int64_t nsplit, hipStream_t s);
void launch_guess_all(const uint8_t* U, int64_t ulen, int32_t u_is_eof, const int32_t* ref_len,
                      int32_t n_ref, uint8_t* flag, hipStream_t s);
// best: 2 * nsplit words of device scratch
void launch_first_record(const uint8_t* U, int64_t ulen, int32_t u_is_eof, const int32_t* ref_len,
                         int32_t n_ref, const int64_t* blk_pos, const int64_t* uoff,
                         const int64_t* d_nblk, SplitPlan* plans, int64_t nsplit,
                         unsigned long long* best, hipStream_t s);

// Kernel 3: record chain over U from `start_lin`.
struct Seg {
  int64_t start;   // speculated / exact first chain position in the segment (-1 none)
  int64_t exit;    // first chain position >= segment end reached from `start`
  int64_t count;   // records started in [start, segment end)
  int32_t exact;   // bit 1: seg_walk recorded the record starts (SEG_OFF_CAP u16 offsets from the
                   // segment start); a re-walk by seg_fix clears it
  int32_t status;
};
constexpr int SEG_OFF_CAP = 512;  // record starts one segment's walk records (64 KiB segments)
// Segments cover [start_lin, chain_end) (record starts wanted); ulen bounds the readable bytes.
void launch_seg_spec(const uint8_t* U, int64_t ulen, int32_t u_is_eof, int64_t chain_end,
                     const int32_t* ref_len, int32_t n_ref, Seg* segs, int64_t nseg,
                     int64_t seg_bytes, int64_t start_lin, uint16_t* offs, hipStream_t s);
void launch_seg_link(const Seg* segs, int64_t nseg, int64_t seg_bytes, int64_t start_lin,
                     int64_t ulen, int32_t* d_broken, hipStream_t s);
void launch_seg_fix2(const uint8_t* U, int64_t ulen, int32_t u_is_eof, int64_t chain_end,
                     Seg* segs, int64_t nseg,
                     int64_t seg_bytes, int64_t start_lin, int32_t* d_status, hipStream_t s);
void launch_seg_counts(const Seg* segs, int64_t nseg, int64_t* counts, hipStream_t s);
void launch_seg_emit2(const uint8_t* U, int64_t ulen, const Seg* segs, const int64_t* base,
                      int64_t nseg, int64_t* rec_lin, hipStream_t s, const uint16_t* offs = nullptr,
                      int64_t seg_bytes = 0, int64_t start_lin = 0);

// Sparse (windowed) record chains: every window is a run of inflated U bytes (whole-file layout)
// with an exact first record start; segments [seg0, next window's seg0) belong to it.
struct Win {
  int64_t u_start;      // exact first record start
  int64_t u_chain_end;  // record starts wanted: < u_chain_end
  int64_t u_limit;      // end of the inflated bytes (reads past it: status 4, needs more)
  int64_t seg0;         // first segment of the window
  int32_t at_eof;       // the window runs to the end of the file
  int32_t pad;
};
void launch_wseg(const uint8_t* U, const int32_t* ref_len, int32_t n_ref, const Win* wins,
                 int64_t nwin, Seg* segs, int64_t nseg, int64_t seg_bytes, int32_t* d_broken,
                 hipStream_t s);
void launch_wseg_fix(const uint8_t* U, Seg* segs, const Win* wins, int64_t nwin, int64_t nseg,
                     int64_t seg_bytes, int32_t* d_status, hipStream_t s);

struct RecSoA {
  uint64_t* voffset;
  int32_t* block_size;
  int32_t* ref_id;
  int32_t* pos;
  int32_t* l_seq;
  int32_t* next_ref_id;
  int32_t* next_pos;
  int32_t* tlen;
  uint16_t* flag;
  uint16_t* bin;
  uint16_t* n_cigar;
  uint8_t* mapq;
  uint8_t* l_read_name;
  uint64_t* hash;
};
// pt: (ulen >> 16) + 1 int32 scratch (block page table); long_ent: long_list_cap(ulen, nrec)
// entries (the pieces of the records hashed by many threads), long_cnt: one device counter
int64_t long_list_cap(int64_t ulen, int64_t nrec);
void launch_decode_records(const uint8_t* U, int64_t ulen, const int64_t* rec_lin, int64_t nrec,
                           const int64_t* blk_pos, const int64_t* uoff, int64_t nblk, int32_t* pt,
                           RecSoA soa, int32_t* d_status, uint64_t* long_ent, int64_t long_cap,
                           unsigned long long* long_cnt, hipStream_t s);

struct PartRange {
  int64_t begin, end;   // record index range in the chain
  uint64_t digest;
};
void launch_sbi_sample(const uint64_t* voffset, int64_t nrec, int64_t g, uint64_t* out,
                       hipStream_t s);
void launch_partition_ranges(const SplitPlan* plans, int64_t nsplit, const int64_t* rec_lin,
                             const uint64_t* voffset, int64_t nrec, PartRange* parts,
                             int32_t* d_status, hipStream_t s);

// .bai index build (dq_write_bai) over the n resident records.
constexpr uint64_t BAI_UNPLACED = ~0ull;  // key of a record without coordinates
enum : int { BAI_ST_REF = 1, BAI_ST_END = 2, BAI_ST_UNSORTED = 3 };  // *status & 0xff
// key[i] = ref << 16 | bin, endp[i] = exclusive alignment end; *status (all ones) takes the first
// offender (index << 8 | BAI_ST_*), *no_coor (zero) the unplaced count; meta (zero): 5 words per
// reference = ~(first record), last record + 1, mapped, unmapped, last linear window + 1.
void launch_bai_keys(const uint8_t* U, const int64_t* rec_lin, const RecSoA soa, int64_t n,
                     int32_t n_ref, uint64_t* key, int32_t* endp, unsigned long long* meta,
                     unsigned long long* status, unsigned long long* no_coor, hipStream_t s);
// lin (all ones; nwin entries, reference r at win_off[r]): min voffset per 16 kb window
void launch_bai_linear(const uint64_t* key, const int32_t* endp, const int32_t* pos,
                       const uint64_t* voff, int64_t n, const int64_t* win_off, int64_t nwin,
                       unsigned long long* lin, hipStream_t s);
// span[2 r], [2 r + 1] = start of reference r's first record, end of its last (pseudo-bin 37450)
void launch_bai_refspan(const unsigned long long* meta, int32_t n_ref, const uint64_t* voff,
                        int64_t n, uint64_t fin, uint64_t* span, hipStream_t s);
// Stable partition by bin level, levels la and la + 1 per pass: out[i] = (level == la) |
// (level == la + 1) << 32 for the packed scan; perm[base + rank] = i from that scan.
void launch_bai_level_flags(const uint64_t* key, int64_t n, int la, int64_t* out, hipStream_t s);
void launch_bai_level_scatter(const uint64_t* key, int64_t n, int la, const int64_t* scan,
                              int64_t base_a, int64_t base_b, int64_t nplaced, int64_t* perm,
                              hipStream_t s);
// out[j] = (record perm[j] opens a chunk) | (opens a bin) << 32; fin = the final file pointer.
// vend (heads and emit): the pointer after record i when it is not the next record's start (text
// lines with other lines between them, dq_text_write_tbi); nullptr: voff[i + 1], fin after the last
void launch_bai_heads(const uint64_t* key, const uint64_t* voff, int64_t n, uint64_t fin,
                      const int64_t* perm, int64_t nplaced, int64_t* out, hipStream_t s,
                      const uint64_t* vend = nullptr);
// chunks[2 c], [2 c + 1] = begin, end; bins[2 b], [2 b + 1] = key, first chunk
void launch_bai_emit(const uint64_t* key, const uint64_t* voff, int64_t n, uint64_t fin,
                     const int64_t* perm, int64_t nplaced, const int64_t* heads,
                     const int64_t* scan, int64_t nchunk, int64_t nbin, uint64_t* chunks,
                     uint64_t* bins, hipStream_t s, const uint64_t* vend = nullptr);
void launch_bs_plus4(const int32_t* bs, int64_t n, int32_t* out, hipStream_t s);
void launch_add_u64(const uint64_t* in, int64_t n, uint64_t add, uint64_t* out, hipStream_t s);
void launch_partition_digest2(const uint64_t* hash, PartRange* parts, int64_t nparts,
                              hipStream_t s);
void launch_partition_digest_idx(const uint64_t* hash, const int64_t* kept, PartRange* parts,
                                 int64_t nparts, hipStream_t s);

// Record export: record-index ranges -> index list; SoA rows and raw bytes gathered by index into
// compact buffers (idx == nullptr in gather_raw: records first .. first + n - 1).
void launch_ranges_to_idx(const int64_t* begin, const int64_t* out_off, int64_t nranges,
                          int64_t* idx, hipStream_t s);
void launch_gather_soa(const int64_t* idx, int64_t n, const RecSoA src, RecSoA dst, hipStream_t s);
void launch_gather_raw(const uint8_t* U, const int64_t* rec_lin, const int32_t* block_size,
                       const int64_t* idx, int64_t first, int64_t n, const int64_t* out_off,
                       uint8_t* out, hipStream_t s);

// Interval traversal over .bai span chunks (partition order): record range of every chunk, keep
// flags -> compact kept index list, per-partition digests over an index list.
void launch_span_ranges(const uint64_t* voffset, int64_t nrec, const uint64_t* cbeg,
                        const uint64_t* cend, int64_t nchunk, int64_t* first, int64_t* count,
                        hipStream_t s);
void launch_keep_to_i32(const uint8_t* keep, int64_t n, int32_t* out, hipStream_t s);
// Span-run unplaced tail: keep flags of chunk k's entries (idx[off[k]..off[k+1])) = from the first
// record with refID == -1 on (*first: device scratch, initialised to all ones).
void launch_tail_keep(const int64_t* idx, const int64_t* off, int k, const int32_t* ref,
                      unsigned long long* first, uint8_t* keep, int64_t max_n, hipStream_t s);
void launch_gather_i64(const int64_t* src, const int64_t* pos, int64_t n, int64_t* dst,
                       hipStream_t s);
void launch_compact_kept(const int64_t* idx, const uint8_t* keep, const int64_t* off, int64_t n,
                         int64_t* kept, hipStream_t s);

// Kernel 4: interval filter; keep[t] for record idx[t] (or t when idx == NULL).
void launch_interval_filter(const uint8_t* U, const int64_t* rec_lin, const RecSoA soa,
                            const int64_t* idx, int64_t n, const int32_t* iv_ref,
                            const int32_t* iv_start, const int32_t* iv_end,
                            const int32_t* ref_iv_begin, int32_t n_ref, uint8_t* keep,
                            hipStream_t s);

// ------------------------------------------------------------------ BGZF text (VCF) path
struct TextPlan {
  int64_t split_start, split_end;
  int64_t k0, k1;   // the split's lines: indices [k0, k1)
  int64_t b0;       // the split stream's first block (-1 none)
  int32_t status;
  int32_t bom;      // line k0 == 0 starts with a UTF-8 BOM that LineRecordReader strips
};
int64_t text_tiles(int64_t ulen);
void launch_text_terms(const uint8_t* U, int64_t ulen, int32_t* tile_count, const int64_t* tile_off,
                       int64_t* term_pos, bool emit, hipStream_t s);
void launch_text_cr_fills(const uint8_t* U, const int64_t* uoff, const int32_t* blk_us, int64_t nblk,
                          int64_t* last_cr_fill, hipStream_t s);
void launch_text_plan(CandList cl, const int64_t* blk_pos,
                      const int32_t* blk_us, const int64_t* uoff, int64_t nblk, int64_t flen,
                      const uint8_t* U, int64_t ulen, const int64_t* term, int64_t nterm,
                      const int64_t* last_cr_fill, TextPlan* plans, int64_t nsplit, hipStream_t s);
void launch_text_values(const uint8_t* U, int64_t ulen, const int64_t* term, int64_t nterm,
                        const int64_t* idx, int64_t n, int32_t bom, int32_t drop_hash,
                        int64_t* vstart, int32_t* vlen, uint64_t* hash, uint8_t* keep,
                        hipStream_t s);
void launch_text_parts(const int64_t* out_off, const int64_t* koff, int64_t nsplit, PartRange* parts,
                       hipStream_t s);
void launch_text_export(const int64_t* kept, int64_t n, const int64_t* vstart, const int32_t* vlen,
                        const uint64_t* hash, int64_t* o_start, int32_t* o_len, uint64_t* o_hash,
                        hipStream_t s);
void launch_vcf_overlap(const uint8_t* U, const int64_t* vstart, const int32_t* vlen, int64_t n,
                        const uint8_t* names, const int32_t* noff, int32_t nnames,
                        const int32_t* ivbeg, const int32_t* ivstart, const int32_t* ivmaxend,
                        uint8_t* keep, hipStream_t s);
void launch_text_gather(const uint8_t* U, const int64_t* vstart, const int32_t* vlen,
                        const int64_t* kept, const int64_t* out_off, int64_t n, uint8_t* out,
                        hipStream_t s);

// .tbi index build (dq_text_write_tbi, DESIGN.md "Building the .tbi") over the resident lines
// (term: the nterm terminator ends; nl lines, the last one possibly unterminated).
enum : int { TBI_ST_FORMAT = 1, TBI_ST_RANGE = 2, TBI_ST_UNSORTED = 3 };  // *status & 0xff
// flag[k] = line k is a data line (a non-empty value that does not start with '#')
void launch_tbi_lines(const uint8_t* U, int64_t ulen, const int64_t* term, int64_t nterm, int64_t nl,
                      int32_t* flag, hipStream_t s);
// dl[off[k]] = k for the flagged lines (off: exclusive scan of flag; n data lines)
void launch_tbi_compact(const int32_t* flag, const int64_t* off, int64_t nl, int64_t n, int64_t* dl,
                        hipStream_t s);
// Per data line i: pos[i] = POS - 1, endp[i] = end (1-based closed = 0-based exclusive), vs / ve =
// the virtual offsets of its first byte and of the byte after its terminator, head[i] = its CHROM
// differs from the previous data line's; *status (all ones) takes the first offender
// (line index << 8 | TBI_ST_*).
void launch_tbi_keys(const uint8_t* U, int64_t ulen, const int64_t* term, int64_t nterm,
                     const int64_t* dl, int64_t n, const int64_t* uoff, const int64_t* blk_pos,
                     int64_t nblk, uint64_t fin, int32_t* pos, int32_t* endp, uint64_t* vs,
                     uint64_t* ve, int32_t* head, unsigned long long* status, hipStream_t s);
// run = hoff[i] + head[i] - 1 (hoff: exclusive scan of head; nrun runs): key[i] = run << 16 | bin;
// meta (zero): 5 words per run as launch_bai_keys writes them per reference; per run the data-line
// and line index of its head and where its CHROM bytes lie in U (nfirst, nline, nstart, nlen).
void launch_tbi_runs(const uint8_t* U, int64_t ulen, const int64_t* term, int64_t nterm,
                     const int64_t* dl, int64_t n, const int32_t* head, const int64_t* hoff,
                     int64_t nrun, const int32_t* pos, const int32_t* endp, uint64_t* key,
                     unsigned long long* meta, int64_t* nfirst, int64_t* nline, int64_t* nstart,
                     int32_t* nlen, hipStream_t s);
// out[noff[r] ...] = the CHROM bytes of run r (nbytes = noff[nrun])
void launch_tbi_names(const uint8_t* U, const int64_t* nstart, const int32_t* nlen,
                      const int64_t* noff, int64_t nrun, int64_t nbytes, uint8_t* out, hipStream_t s);

// Record hash of the n byte spans base[start[i], start[i] + len[i]): a thread
// per span of up to 2048 bytes, a wave per longer one.  base: readable 16 bytes past every span.
void launch_span_hash(const uint8_t* base, const int64_t* start, const int32_t* len, int64_t n,
                      uint64_t* hash, hipStream_t s);

// ------------------------------------------------------------------ SAM text path (dq_sam.hip)
// Lines of T[0, flen) from its terminator ends: value start and length (terminator excluded, a BOM
// stripped from line 0 when bom), raw start, keep = the value does not start with '@'.
void launch_sam_lines(const uint8_t* T, int64_t flen, const int64_t* term, int64_t nterm, int64_t nl,
                      int32_t bom, int64_t* lstart, int64_t* vstart, int32_t* vlen, uint8_t* keep,
                      hipStream_t s);
// parts[i] = the kept-record range of split i: lines whose first byte s has start < s <= end
// (offset 0 belongs to split 0); splits: nsplit (start, end) pairs; koff: exclusive scan of keep.
void launch_sam_parts(const int64_t* splits, int64_t nsplit, const int64_t* lstart, int64_t nl,
                      const int64_t* koff, PartRange* parts, hipStream_t s);
// Size pass over the n kept lines (kept[j] = line index): status[j], size[j] = 4 + block_size;
// scal[0] (all ones) takes the smallest failing j, scal[1] (zero) the undecided floats.
void launch_sam_sizes(const uint8_t* T, const int64_t* vstart, const int32_t* vlen, int64_t nl,
                      const int64_t* kept, int64_t n, dqt::NameTable refs, int32_t* status, int32_t* size,
                      unsigned long long* scal, hipStream_t s);
// Encode pass: record j at rec[roff[j]], roff[n] = total bytes; SoA rows; undecided floats appended
// to fix (3 words each: byte offset in rec, text offset in T, text length), counted in fix_cnt.
void launch_sam_encode(const uint8_t* T, const int64_t* lstart, const int64_t* vstart,
                       const int32_t* vlen, int64_t nl, const int64_t* kept, int64_t n, dqt::NameTable refs,
                       const int64_t* roff, const int32_t* size, uint8_t* rec, RecSoA soa,
                       int64_t* fix, int64_t fix_cap, unsigned long long* fix_cnt, hipStream_t s);

// ------------------------------------------------------------------ VCF site decode (dq_vcf.hip)
struct VcfCols {           // the columns of dq_variant_batch, one row per variant
  int32_t* contig;
  int32_t* pos;
  int32_t* end;
  uint32_t* flags;
  double* qual;
  int32_t* col_end;        // 8 per variant
  int32_t* n_alt;
  int32_t* n_filter;
  int32_t* n_info;
  int32_t* n_sample_cols;
  int32_t* site_len;       // col_end[8 j + 7] again, contiguous for the scan of the SITES export
};
// Validate pass over the n lines of the text path's list (value start / length, lidx[t] = the
// line's index in the file's line table); '#' lines are skipped.  scal[0] (all ones) takes the
// smallest (line index << 8 | error class), scal[1] (zero) the undecided QUAL texts.
void launch_vcf_validate(const uint8_t* U, int64_t ulen, const int64_t* vstart, const int32_t* vlen,
                         const int64_t* lidx, int64_t n, int32_t G, dqt::NameTable ctg,
                         unsigned long long* scal, hipStream_t s);
// Decode pass over the n kept lines (kept[j] = entry of the list of `total` lines): the columns;
// undecided QUAL texts appended to fix (3 words each: variant, text offset in U, text length),
// counted in fix_cnt.
void launch_vcf_decode(const uint8_t* U, int64_t ulen, const int64_t* vstart, const int32_t* vlen,
                       int64_t total, const int64_t* kept, int64_t n, int32_t G, dqt::NameTable ctg,
                       VcfCols out, int64_t* fix, int64_t fix_cap, unsigned long long* fix_cnt,
                       hipStream_t s);
// out[out_off[j] ...] = U[start[j], start[j] + len[j]) for the n variants (out_off[n] = total bytes)
void launch_vcf_gather(const uint8_t* U, int64_t ulen, const int64_t* start, const int32_t* len,
                       const int64_t* out_off, int64_t n, uint8_t* out, hipStream_t s);

// ------------------------------------------------------------------ VCF genotype decode (dq_vcf_gt.hip)
struct VcfLines {          // the kept variants of a text run, and where the site decode left their columns
  const uint8_t* U;
  int64_t ulen;
  const int64_t* vstart;   // value start / length of the `total` lines of the list
  const int32_t* vlen;
  const int64_t* lidx;     // their indices in the file's line table
  int64_t total;
  const int64_t* kept;     // variant j = entry kept[j] of the list
  int64_t n;
  const int32_t* col_end;  // VcfCols of the same variants: column c of variant j ends at col_end[8 j + c]
};
struct GtIn {              // FORMAT starts at col_end[8 j + 7] + 1
  VcfLines ln;
  const int32_t* n_alt;
  const int32_t* n_sample_cols;
  int32_t S;               // the header's sample count, > 0
};
struct GtCols {            // the arrays of dq_genotype_batch, n * S cells, row-major by variant
  uint8_t* flags;
  uint8_t* ploidy;
  int16_t* allele;         // P per cell
  int32_t* gq;
  int32_t* dp;
  int32_t* cell_off;
};
// Check pass: scal[0] (all ones) takes the smallest dqg::gt_error_key, scal[1] (zero) the largest
// ploidy, scal[2] (zero) the count of GQ texts left to the host; scal[3] is the decode pass's.
void launch_gt_check(GtIn in, unsigned long long* scal, hipStream_t s);
// Decode pass: the matrix at ploidy P; the host's GQ texts appended to fix (3 words each: cell,
// text offset in U, text length), counted in scal[3] (zero).
void launch_gt_decode(GtIn in, GtCols out, int32_t P, int64_t* fix, int64_t fix_cap,
                      unsigned long long* scal, hipStream_t s);

// ------------------------------------------------------------------ VCF INFO decode (dq_vcf_info.hip)
struct InfoIn {            // INFO is [col_end[8 j + 6] + 1, col_end[8 j + 7]) of variant j's value
  VcfLines ln;
  dqt::NameTable keys;     // dqi::InfoKeys in device memory (dq_vcf_info_core.h), n <= 64
  const uint8_t* key_type;
  const uint8_t* key_hflag;
};
struct InfoCols {          // the arrays of dq_info_batch, key-major: cell (q, k) at q * n + k
  uint8_t* flags;
  int32_t* n_values;
  int32_t* val_off;
  int32_t* val_len;
  int32_t* ival;
  int64_t n_ival;
  uint64_t* fval;          // the doubles' bits
  int64_t n_fval;
  const int64_t* key_base; // [K] in device memory
  const int32_t* key_width;
};
// Check pass: scal[0] (all ones) takes the smallest dqi::info_error_key, scal[1] (zero) the count
// of Float texts left to the host; scal[2] is the decode pass's; width[q] (one) takes the largest
// value count of key q.
void launch_info_check(InfoIn in, unsigned long long* scal, int32_t* width, hipStream_t s);
// Decode pass: the columns; the host's Float texts appended to fix (5 words each: key, variant,
// element, text offset in U, text length), counted in scal[2] (zero).
void launch_info_decode(InfoIn in, InfoCols out, int64_t* fix, int64_t fix_cap, unsigned long long* scal,
                        hipStream_t s);

// ------------------------------------------------------------------ SAM writer (dq_samw.hip)
struct SamwRefs {           // the header's reference names by index, see dq_samw_core.h
  const int32_t* name_off;  // n + 1 offsets into names
  const uint8_t* names;
  int32_t n;
};
int32_t samw_tile_bytes();  // line bytes one workgroup's LDS tile takes
// Size pass over the n records at raw[off[j]] (raw_len readable bytes): status[j], size[j] = the
// line's bytes with its LF; scal[0] (all ones) takes the smallest failing j, scal[1] (all ones) the
// smallest j whose line is longer than 2^31-1 bytes.
void launch_samw_sizes(const uint8_t* raw, int64_t raw_len, const int64_t* off, int64_t n,
                       SamwRefs refs, int32_t* status, int64_t* size, unsigned long long* scal,
                       hipStream_t s);
// Format pass: line j at text[loff[j]], loff[n] = total bytes (text: 16-byte aligned for the tile
// path; use_tile 0: every line straight to memory).
void launch_samw_format(const uint8_t* raw, int64_t raw_len, const int64_t* off, int64_t n,
                        SamwRefs refs, const int64_t* loff, uint8_t* text, int32_t use_tile,
                        hipStream_t s);

// ------------------------------------------------------------------ BAM aux tag decode (dq_tags.hip)
struct TagIn {              // row j is record idx[j] (idx == nullptr: first + j) of the nrec resident ones
  const uint8_t* src;       // the records' bytes: record k at src[rec_lin[k]], src_len readable
  int64_t src_len;
  const int64_t* rec_lin;
  const int32_t* block_size;
  const int32_t* l_seq;
  const uint16_t* n_cigar;
  const uint8_t* l_read_name;
  int64_t nrec;
  const int64_t* idx;
  int64_t first, n;
  const uint32_t* key_slot; // dqa::TagKeys in device memory (dq_tags_core.h): TAG_SLOTS slots, n_keys types
  const uint8_t* key_type;
  int32_t n_keys;
};
struct TagCols {            // the arrays of dq_tag_batch, key-major: cell (q, k) at q * n + k
  uint8_t* flags;
  uint8_t* vtype;
  uint8_t* subtype;
  int32_t* val_off;
  int32_t* val_len;
  uint32_t* val;
  int64_t n_val;
  const int64_t* key_base;  // [K] in device memory
};
// Check pass: scal[0] (all ones) takes the smallest dqa::tag_error_key.
void launch_tags_check(TagIn in, unsigned long long* scal, hipStream_t s);
// Decode pass: every cell of the K x n columns.
void launch_tags_decode(TagIn in, TagCols out, hipStream_t s);

// DQ_CHECKED: each kernel unit's check words (count << 32 | site bits), read and reset
uint64_t dq_chk_take_sam();
uint64_t dq_chk_take_samw();
uint64_t dq_chk_take_vcf();
uint64_t dq_chk_take_vcfgt();
uint64_t dq_chk_take_vcfinfo();
uint64_t dq_chk_take_tags();
uint64_t dq_chk_take_kernels();
uint64_t dq_chk_take_inflate();
uint64_t dq_chk_take_text();
uint64_t dq_chk_take_deflate();

// ------------------------------------------------------------------ BGZF deflate (write path)
int64_t bgzf_block_count(int64_t n);
size_t bgzf_stage_bytes(int64_t nblk);
size_t bgzf_meta_bytes(int64_t nblk);
size_t bgzf_slot_bytes(int64_t nblk);  // the blocks' output slots
bool deflate_tables(int device);
// Blocks [blk0, blk0 + nblk) of src[0, n_in) (65280 bytes each) into fixed-size slots: the
// chunk parse kernel, the Huffman kernel, then the code/emit kernel.  tim (DQ_DEFLATE_TIMING): 8
// words per parse workgroup (2 per block), then 8 per block for each of the other two kernels.
void launch_bgzf_deflate(const uint8_t* src, int64_t n_in, int64_t blk0, int64_t nblk,
                         uint32_t* stage, uint32_t* meta, uint8_t* out_slots, int32_t* out_size,
                         uint64_t* tim, hipStream_t s);
// Packs the slots at offsets scanned on the device from the sizes on top of *total (the stream's
// length so far, updated).
void launch_bgzf_pack(const uint8_t* slots, const int32_t* size, int64_t* off, int64_t* total,
                      int64_t nblk, uint8_t* out, hipStream_t s);

}  // namespace dq
