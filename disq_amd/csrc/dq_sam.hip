// dq_sam.hip -- SAM text path: the lines Hadoop's TextInputFormat
// returns per split of an uncompressed SAM file, each encoded into the BAM record htsjdk's
// SAMLineParser + BAMRecordCodec make of it (SamSource.getReads, D/impl/formats/sam/
// SamSource.java:36-77).  The per-line rules are dq_sam_core.h; this file
// holds the kernels around them.  The text is read from the uploaded file bytes (ctx->C, with its
// zero pad), never copied:
//   lines      value start / length, raw start and keep flag ('@' lines are dropped wherever they
//              stand) of every line between the terminator ends the text path's scan found;
//   parts      per split the range of kept lines whose first byte s has start < s <= end
//              (LineRecordReader on an uncompressed split; offset 0 belongs to split 0): two binary
//              searches over the line starts, on the device;
//   sizes      status and record size of every kept line -- a thread per line of up to SAM_LONG
//              bytes, a wave per longer one -- the first failing line by a min over indices;
//   encode     the records back to back in line order at the scanned offsets, the SoA rows from
//              the parsed fields, undecided floats listed for the host.
// voffset is the offset of the line's first byte in the file: SAM text has no virtual offsets.
// Out of scope: interval traversal, LENIENT / SILENT tolerance of malformed lines, sharded and
// multi-GPU SAM.  (SAM output is dq_samw.hip.)
#if defined(__HIP_DEVICE_COMPILE__)
#define DQS_CHECK(cond) DQ_CHK(cond, CHK_SAM)
#define DQT_CHECK(cond) DQ_CHK(cond, CHK_SAM)
#else
#define DQS_CHECK(cond) ((void)0)
#define DQT_CHECK(cond) ((void)0)
#endif
#include "dq_internal.h"
#include "dq_sam_core.h"

namespace dq {
namespace {

constexpr int32_t SAM_LONG = 2048;  // longer lines get a wave (the text path's TV_LONG)

__global__ __launch_bounds__(256) void sam_lines_kernel(const uint8_t* __restrict__ T, int64_t flen,
                                                        const int64_t* __restrict__ term,
                                                        int64_t nterm, int64_t nl, int32_t bom,
                                                        int64_t* __restrict__ lstart,
                                                        int64_t* __restrict__ vstart,
                                                        int32_t* __restrict__ vlen,
                                                        uint8_t* __restrict__ keep) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nl) return;
  DQ_CHK(k - 1 < nterm, CHK_SAM);
  const int64_t a0 = k == 0 ? 0 : term[k - 1] + 1;
  int64_t z = flen;
  if (k < nterm) {
    const int64_t te = term[k];
    DQ_CHK(te >= a0 && te < flen, CHK_SAM);
    z = te;  // exclusive end of the value
    if (T[te] == '\n' && te > a0 && T[te - 1] == '\r') z = te - 1;
  }
  int64_t a = a0;
  if (k == 0 && bom) a = a + 3 <= z ? a + 3 : z;
  lstart[k] = a0;
  vstart[k] = a;
  vlen[k] = (int32_t)(z - a);
  keep[k] = (uint8_t)!(z > a && T[a] == '@');
}

// first index i in [0, n) with start(i) > v, where start(i) = the first byte of line i
__device__ inline int64_t lines_after(const int64_t* __restrict__ lstart, int64_t n, int64_t v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (lstart[mid] <= v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ void sam_parts_kernel(const int64_t* __restrict__ splits, int64_t nsplit,
                                 const int64_t* __restrict__ lstart, int64_t nl,
                                 const int64_t* __restrict__ koff, PartRange* __restrict__ parts) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nsplit) return;
  const int64_t lo = i == 0 ? 0 : lines_after(lstart, nl, splits[2 * i]);
  int64_t hi = lines_after(lstart, nl, splits[2 * i + 1]);
  if (hi < lo) hi = lo;
  DQ_CHK(lo >= 0 && hi <= nl, CHK_SAM);
  parts[i].begin = nl > 0 ? koff[lo] : 0;
  parts[i].end = nl > 0 ? koff[hi] : 0;
  parts[i].digest = 0;
}

// ---- size pass
__global__ __launch_bounds__(256) void sam_size_kernel(const uint8_t* __restrict__ T,
                                                       const int64_t* __restrict__ vstart,
                                                       const int32_t* __restrict__ vlen, int64_t nl,
                                                       const int64_t* __restrict__ kept, int64_t n,
                                                       dqt::NameTable refs, int32_t* __restrict__ status,
                                                       int32_t* __restrict__ size,
                                                       unsigned long long* __restrict__ scal) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int64_t k = kept[j];
  DQ_CHK(k >= 0 && k < nl, CHK_SAM);
  const int32_t len = vlen[k];
  if (len > SAM_LONG) return;  // sam_size_long_kernel
  dqs::SamLineInfo I;
  const int32_t st = dqs::sam_line_size(T + vstart[k], len, refs, &I);
  status[j] = st;
  size[j] = st ? 0 : I.size;
  if (st) atomicMin(&scal[0], (unsigned long long)j);
  if (!st && I.n_undecided) atomicAdd(&scal[1], (unsigned long long)I.n_undecided);
}

// The first 11 TABs of a long line, found by the whole wave 64 bytes at a time (every lane ends
// with the same list): SEQ and QUAL, the bulk of a long read, are not walked by one lane.
__device__ inline dqs::SamTabs wave_tabs(const uint8_t* __restrict__ L, int32_t len, int lane) {
  dqs::SamTabs tb{};
  for (int32_t base = 0; base < len && tb.n < 11; base += 64) {
    const int32_t x = base + lane;
    unsigned long long m = __ballot(x < len && L[x] == '\t');
    while (m && tb.n < 11) {
      const int32_t at = base + (int32_t)__builtin_ctzll(m);
      m &= m - 1;
#pragma unroll
      for (int c = 0; c < 11; c++)  // compile-time indices keep the list in registers
        if (c == tb.n) tb.at[c] = at;
      tb.n++;
    }
  }
  return tb;
}

// One wave per long line: lane 0 walks the columns and tags, the lanes share SEQ and QUAL.
__global__ __launch_bounds__(256) void sam_size_long_kernel(const uint8_t* __restrict__ T,
                                                            const int64_t* __restrict__ vstart,
                                                            const int32_t* __restrict__ vlen,
                                                            int64_t nl,
                                                            const int64_t* __restrict__ kept,
                                                            int64_t n, dqt::NameTable refs,
                                                            int32_t* __restrict__ status,
                                                            int32_t* __restrict__ size,
                                                            unsigned long long* __restrict__ scal) {
  const int lane = threadIdx.x & 63;
  const int64_t nwave = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t j = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); j < n; j += nwave) {
    const int64_t k = kept[j];
    DQ_CHK(k >= 0 && k < nl, CHK_SAM);
    const int32_t len = vlen[k];
    if (len <= SAM_LONG) continue;  // wave-uniform
    const uint8_t* L = T + vstart[k];
    int32_t st = 0, sz = 0, nund = 0, seq_off = 0, qual_off = -1, l_seq = 0;
    const dqs::SamTabs tb = wave_tabs(L, len, lane);
    if (lane == 0) {
      dqs::SamLineInfo I;
      st = dqs::sam_line_walk(L, len, refs, nullptr, 0, &I, nullptr, false, &tb);
      sz = I.size;
      nund = I.n_undecided;
      seq_off = I.seq_off;
      qual_off = I.qual_off;
      l_seq = I.l_seq;
    }
    st = __shfl(st, 0, 64);
    seq_off = __shfl(seq_off, 0, 64);
    qual_off = __shfl(qual_off, 0, 64);
    l_seq = __shfl(l_seq, 0, 64);
    if (st == 0 || st >= dqs::SAM_E_TAG) {  // the SEQ and QUAL bytes rank before the tags
      DQ_CHK(seq_off >= 0 && seq_off + l_seq <= len && (qual_off < 0 || qual_off + l_seq <= len),
             CHK_SAM);
      bool sbad = false, qbad = false;
      const int32_t n8 = l_seq & ~7;  // whole groups of eight: one 8-byte load per lane and step
      for (int32_t i = 8 * lane; i < n8; i += 512) {
        uint32_t pk;
        uint64_t q8;
        sbad |= !dqs::sam_pack8(L + seq_off + i, &pk);
        if (qual_off >= 0) qbad |= !dqs::sam_qual8(L + qual_off + i, &q8);
      }
      for (int32_t i = n8 + lane; i < l_seq; i += 64) {
        sbad |= dqs::sam_seq_code(L[seq_off + i]) < 0;
        if (qual_off >= 0) qbad |= L[qual_off + i] < 33;
      }
      if (__ballot(sbad) != 0) st = dqs::SAM_E_SEQ;
      else if (__ballot(qbad) != 0) st = dqs::SAM_E_QUAL;
    }
    if (lane == 0) {
      status[j] = st;
      size[j] = st ? 0 : sz;
      if (st) atomicMin(&scal[0], (unsigned long long)j);
      if (!st && nund) atomicAdd(&scal[1], (unsigned long long)nund);
    }
  }
}

// ---- encode pass
__device__ inline void store_row(const RecSoA& soa, int64_t j, int64_t line_off,
                                 const dqs::SamLineInfo& I) {
  soa.voffset[j] = (uint64_t)line_off;
  soa.block_size[j] = I.size - 4;
  soa.ref_id[j] = I.ref_id;
  soa.pos[j] = I.pos;
  soa.l_seq[j] = I.l_seq;
  soa.next_ref_id[j] = I.next_ref_id;
  soa.next_pos[j] = I.next_pos;
  soa.tlen[j] = I.tlen;
  soa.flag[j] = I.flag;
  soa.bin[j] = I.bin;
  soa.n_cigar[j] = I.n_cigar;
  soa.mapq[j] = I.mapq;
  soa.l_read_name[j] = I.l_read_name;
}

__global__ __launch_bounds__(256) void sam_encode_kernel(
    const uint8_t* __restrict__ T, const int64_t* __restrict__ lstart,
    const int64_t* __restrict__ vstart, const int32_t* __restrict__ vlen, int64_t nl,
    const int64_t* __restrict__ kept, int64_t n, dqt::NameTable refs, const int64_t* __restrict__ roff,
    const int32_t* __restrict__ size, uint8_t* __restrict__ rec, RecSoA soa, int64_t* __restrict__ fix,
    int64_t fix_cap, unsigned long long* __restrict__ fix_cnt) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int64_t k = kept[j];
  DQ_CHK(k >= 0 && k < nl, CHK_SAM);
  const int32_t len = vlen[k];
  if (len > SAM_LONG) return;  // sam_encode_long_kernel
  const int64_t o = roff[j], total = roff[n];
  const int32_t sz = size[j];
  DQ_CHK(o >= 0 && sz >= 36 && o + sz <= total && roff[j + 1] == o + sz, CHK_SAM);
  if (o < 0 || sz < 36 || o + sz > total) return;  // never store outside the record buffer
  const dqs::SamFixSink fx{fix, fix_cnt, fix_cap, o, vstart[k]};
  dqs::SamLineInfo I;
  const int32_t st = dqs::sam_line_encode(T + vstart[k], len, refs, rec + o, sz, &I, &fx);
  DQ_CHK(st == 0 && I.size == sz, CHK_SAM);
  (void)st;
  store_row(soa, j, lstart[k], I);
}

__global__ __launch_bounds__(256) void sam_encode_long_kernel(
    const uint8_t* __restrict__ T, const int64_t* __restrict__ lstart,
    const int64_t* __restrict__ vstart, const int32_t* __restrict__ vlen, int64_t nl,
    const int64_t* __restrict__ kept, int64_t n, dqt::NameTable refs, const int64_t* __restrict__ roff,
    const int32_t* __restrict__ size, uint8_t* __restrict__ rec, RecSoA soa, int64_t* __restrict__ fix,
    int64_t fix_cap, unsigned long long* __restrict__ fix_cnt) {
  const int lane = threadIdx.x & 63;
  const int64_t nwave = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t j = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); j < n; j += nwave) {
    const int64_t k = kept[j];
    DQ_CHK(k >= 0 && k < nl, CHK_SAM);
    const int32_t len = vlen[k];
    if (len <= SAM_LONG) continue;  // wave-uniform
    const uint8_t* L = T + vstart[k];
    const int64_t o = roff[j], total = roff[n];
    const int32_t sz = size[j];
    DQ_CHK(o >= 0 && sz >= 36 && o + sz <= total && roff[j + 1] == o + sz, CHK_SAM);
    if (o < 0 || sz < 36 || o + sz > total) continue;  // wave-uniform; never store outside the buffer
    int32_t seq_off = 0, qual_off = -1, l_seq = 0, seq_out = 0, qual_out = 0;
    const dqs::SamTabs tb = wave_tabs(L, len, lane);
    if (lane == 0) {
      const dqs::SamFixSink fx{fix, fix_cnt, fix_cap, o, vstart[k]};
      dqs::SamLineInfo I;
      const int32_t st = dqs::sam_line_walk(L, len, refs, rec + o, sz, &I, &fx, false, &tb);
      DQ_CHK(st == 0 && I.size == sz, CHK_SAM);
      (void)st;
      store_row(soa, j, lstart[k], I);
      seq_off = I.seq_off;
      qual_off = I.qual_off;
      l_seq = I.l_seq;
      seq_out = I.seq_out;
      qual_out = I.qual_out;
    }
    seq_off = __shfl(seq_off, 0, 64);
    qual_off = __shfl(qual_off, 0, 64);
    l_seq = __shfl(l_seq, 0, 64);
    seq_out = __shfl(seq_out, 0, 64);
    qual_out = __shfl(qual_out, 0, 64);
    // nothing is stored outside the record, whatever the walk reported
    const bool fits = seq_off >= 0 && seq_off + l_seq <= len && (qual_off < 0 || qual_off + l_seq <= len) &&
                      seq_out >= 36 && qual_out == seq_out + (l_seq + 1) / 2 && qual_out + l_seq <= sz;
    DQ_CHK(fits, CHK_SAM);
    if (!fits) continue;  // wave-uniform
    uint8_t* R = rec + o;
    // whole groups of eight bases / qualities: an 8-byte load, a 4- or 8-byte store per lane and
    // step (consecutive lanes, consecutive words); the tail of up to seven by bytes
    const int32_t n8 = l_seq & ~7;
    for (int32_t i = 8 * lane; i < n8; i += 512) {
      uint32_t pk;
      (void)dqs::sam_pack8(L + seq_off + i, &pk);
      __builtin_memcpy(R + seq_out + (i >> 1), &pk, 4);
      uint64_t q8 = ~0ull;
      if (qual_off >= 0) (void)dqs::sam_qual8(L + qual_off + i, &q8);
      __builtin_memcpy(R + qual_out + i, &q8, 8);
    }
    const int32_t nb = (l_seq + 1) / 2;
    for (int32_t b = (n8 >> 1) + lane; b < nb; b += 64) {  // high nibble first
      const int hi = dqs::sam_seq_code(L[seq_off + 2 * b]);
      const int lo = 2 * b + 1 < l_seq ? dqs::sam_seq_code(L[seq_off + 2 * b + 1]) : 0;
      R[seq_out + b] = (uint8_t)((hi << 4) | (lo & 15));
    }
    for (int32_t i = n8 + lane; i < l_seq; i += 64)
      R[qual_out + i] = qual_off < 0 ? (uint8_t)0xff : (uint8_t)(L[qual_off + i] - 33);
  }
}

}  // namespace

DQ_CHK_UNIT(sam)

void launch_sam_lines(const uint8_t* T, int64_t flen, const int64_t* term, int64_t nterm, int64_t nl,
                      int32_t bom, int64_t* lstart, int64_t* vstart, int32_t* vlen, uint8_t* keep,
                      hipStream_t s) {
  if (nl <= 0) return;
  hipLaunchKernelGGL(sam_lines_kernel, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, s, T, flen,
                     term, nterm, nl, bom, lstart, vstart, vlen, keep);
}

void launch_sam_parts(const int64_t* splits, int64_t nsplit, const int64_t* lstart, int64_t nl,
                      const int64_t* koff, PartRange* parts, hipStream_t s) {
  if (nsplit <= 0) return;
  hipLaunchKernelGGL(sam_parts_kernel, dim3((unsigned)((nsplit + 63) / 64)), dim3(64), 0, s, splits,
                     nsplit, lstart, nl, koff, parts);
}

static unsigned wave_grid(int64_t n) {  // 4 waves per block, grid-stride past 2048 blocks
  const int64_t g = (n + 3) / 4;
  return (unsigned)(g < 1 ? 1 : g > 2048 ? 2048 : g);
}

void launch_sam_sizes(const uint8_t* T, const int64_t* vstart, const int32_t* vlen, int64_t nl,
                      const int64_t* kept, int64_t n, dqt::NameTable refs, int32_t* status, int32_t* size,
                      unsigned long long* scal, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(sam_size_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, T, vstart,
                     vlen, nl, kept, n, refs, status, size, scal);
  hipLaunchKernelGGL(sam_size_long_kernel, dim3(wave_grid(n)), dim3(256), 0, s, T, vstart, vlen, nl,
                     kept, n, refs, status, size, scal);
}

void launch_sam_encode(const uint8_t* T, const int64_t* lstart, const int64_t* vstart,
                       const int32_t* vlen, int64_t nl, const int64_t* kept, int64_t n, dqt::NameTable refs,
                       const int64_t* roff, const int32_t* size, uint8_t* rec, RecSoA soa,
                       int64_t* fix, int64_t fix_cap, unsigned long long* fix_cnt, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(sam_encode_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, T, lstart,
                     vstart, vlen, nl, kept, n, refs, roff, size, rec, soa, fix, fix_cap, fix_cnt);
  hipLaunchKernelGGL(sam_encode_long_kernel, dim3(wave_grid(n)), dim3(256), 0, s, T, lstart, vstart,
                     vlen, nl, kept, n, refs, roff, size, rec, soa, fix, fix_cap, fix_cnt);
}

}  // namespace dq
