// dq_samw.hip -- the SAM writer (row f8): BAM records into the lines SamSink.save writes
// (D/impl/formats/sam/SamSink.java:37: SAMRecord.getSAMString, String.trim, a LF each).  The
// per-record rules are dq_samw_core.h; this file holds the kernels around
// them, in the shape of the reader's (dq_sam.hip):
//   sizes      status and line size of every record -- a thread per record of up to SAMW_LONG
//              bytes, a wave per longer one (lane 0 walks the short columns and the tags, the
//              lanes share QUAL) -- the first failing record and the first line past 2^31-1 bytes
//              by a min over indices;
//   format     the lines back to back at the scanned offsets.  Consecutive records' lines are
//              contiguous, so a workgroup formats its SAMW_RUN records into an LDS tile and streams
//              the tile out in aligned 16-byte stores; a run whose lines exceed the tile, or that
//              holds a long record, writes its short records straight to memory; a long record is
//              written by its wave (lane 0 the short columns and tags, the lanes SEQ and QUAL).
// Both passes run the same walk, with and without an output pointer, and every store of the second
// is bounded by the size the first gave.
// Out of scope: CRAM, one file per partition, sharded and multi-GPU SAM output.
#include "dq_internal.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define DQS_CHECK(cond) DQ_CHK(cond, CHK_SAM)
#else
#define DQS_CHECK(cond) ((void)0)
#endif
#include "dq_samw_core.h"

namespace dq {
namespace {

__device__ inline dqw::RefNames ref_names(const SamwRefs& r) {
  return dqw::RefNames{r.name_off, r.names, r.n};
}

// The record at off: the bytes readable from it (0: the offset itself is out of range) and
// whether a wave takes it (a whole record of more than SAMW_LONG bytes).
__device__ inline int64_t rec_avail(const uint8_t* __restrict__ raw, int64_t raw_len, int64_t off,
                                    bool* is_long) {
  *is_long = false;
  if (off < 0 || off > raw_len - 4) return 0;
  const int64_t avail = raw_len - off;
  const int32_t bs = dqw::rd32(raw + off);
  *is_long = bs >= 32 && 4 + (int64_t)bs <= avail && 4 + (int64_t)bs > dqw::SAMW_LONG;
  return avail;
}

__device__ inline void store_size(int64_t j, int32_t st, int64_t sz, int32_t* __restrict__ status,
                                  int64_t* __restrict__ size, unsigned long long* __restrict__ scal) {
  status[j] = st;
  size[j] = st ? 0 : sz;
  if (st) atomicMin(&scal[0], (unsigned long long)j);
  else if (sz > 0x7fffffffll) atomicMin(&scal[1], (unsigned long long)j);
}

// ---- size pass
__global__ __launch_bounds__(256) void samw_size_kernel(const uint8_t* __restrict__ raw, int64_t raw_len,
                                                        const int64_t* __restrict__ off, int64_t n,
                                                        SamwRefs refs, int32_t* __restrict__ status,
                                                        int64_t* __restrict__ size,
                                                        unsigned long long* __restrict__ scal) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  bool lng;
  const int64_t o = off[j], avail = rec_avail(raw, raw_len, o, &lng);
  if (lng) return;  // samw_size_long_kernel
  dqw::Walk W;
  W.size = 0;
  const int32_t st = avail ? dqw::samw_record_walk(raw + o, avail, ref_names(refs), nullptr, 0, false, false, &W)
                           : (int32_t)dqs::SAM_E_FIELDS;
  store_size(j, st, W.size, status, size, scal);
}

// The wave's scan of a long record's QUAL: every byte 0xFF, a byte above 93.
__device__ inline void wave_qual(const uint8_t* __restrict__ q, int32_t n, int lane, bool* all_ff,
                                 bool* bad) {
  bool ff = true, b = false;
  const int32_t n8 = n & ~7;
  for (int32_t i = 8 * lane; i < n8; i += 512) {
    uint64_t w;
    __builtin_memcpy(&w, q + i, 8);
    dqw::samw_qual8(w, &ff, &b);
  }
  for (int32_t i = n8 + lane; i < n; i += 64) {
    ff = ff && q[i] == 0xff;
    b = b || q[i] > 93;
  }
  *all_ff = __ballot(!ff) == 0;
  *bad = __ballot(b) != 0;
}

__global__ __launch_bounds__(256) void samw_size_long_kernel(const uint8_t* __restrict__ raw,
                                                             int64_t raw_len,
                                                             const int64_t* __restrict__ off, int64_t n,
                                                             SamwRefs refs, int32_t* __restrict__ status,
                                                             int64_t* __restrict__ size,
                                                             unsigned long long* __restrict__ scal) {
  const int lane = threadIdx.x & 63;
  const int64_t nwave = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t j = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); j < n; j += nwave) {
    bool lng;
    const int64_t o = off[j], avail = rec_avail(raw, raw_len, o, &lng);
    if (!lng) continue;  // wave-uniform
    const uint8_t* r = raw + o;
    dqw::Layout L;
    int32_t st = dqw::samw_layout(r, avail, &L);  // every lane, the same answer
    bool all_ff = true, bad = false;
    if (st == 0) wave_qual(r + L.qual_at, L.l_seq, lane, &all_ff, &bad);
    if (lane == 0) {
      dqw::Walk W;
      W.size = 0;
      if (st == 0) st = dqw::samw_record_walk(r, avail, ref_names(refs), nullptr, 0, true, all_ff, &W);
      // QUAL ranks after the fixed columns and before the tags
      if ((st == 0 || st >= dqs::SAM_E_TAG) && L.l_seq > 0 && !all_ff && bad) st = dqs::SAM_E_QUAL;
      store_size(j, st, W.size, status, size, scal);
    }
  }
}

// ---- format pass
__global__ __launch_bounds__(dqw::SAMW_RUN) void samw_format_kernel(
    const uint8_t* __restrict__ raw, int64_t raw_len, const int64_t* __restrict__ off, int64_t n,
    SamwRefs refs, const int64_t* __restrict__ loff, uint8_t* __restrict__ text, int32_t use_tile) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[dqw::SAMW_TILE + 16];
  const int64_t r0 = (int64_t)blockIdx.x * dqw::SAMW_RUN;
  const int64_t r1 = r0 + dqw::SAMW_RUN < n ? r0 + dqw::SAMW_RUN : n;
  const int64_t j = r0 + threadIdx.x;
  const int64_t total = loff[n], g0 = loff[r0], span = loff[r1] - g0;
  bool lng = false;
  int64_t o = 0, avail = 0, lo = 0, sz = 0;
  if (j < r1) {
    o = off[j];
    avail = rec_avail(raw, raw_len, o, &lng);
    lo = loff[j];
    sz = loff[j + 1] - lo;
  }
  const bool ok = j < r1 && !lng && avail > 0 && lo >= g0 && sz >= 1 && lo + sz <= g0 + span &&
                  g0 >= 0 && g0 + span <= total;
  DQ_CHK(j >= r1 || lng || ok, CHK_SAM);
  // one wave: the ballot is the whole workgroup's
  const bool tiled = use_tile && span >= 0 && span <= dqw::SAMW_TILE && __ballot(j < r1 && lng) == 0 &&
                     g0 >= 0 && g0 + span <= total;
  const int32_t shift = (int32_t)(g0 & 15);  // tile[i] goes to text[g0 - shift + i]
  if (ok) {
    dqw::Walk W;
    uint8_t* out = tiled ? tile + shift + (lo - g0) : text + lo;
    const int32_t st = dqw::samw_record_walk(raw + o, avail, ref_names(refs), out, sz, false, false, &W);
    DQ_CHK(st == 0 && W.size == sz, CHK_SAM);
    (void)st;
  }
  if (!tiled) return;  // workgroup-uniform
  __syncthreads();
  const int32_t lim = shift + (int32_t)span;  // tile[shift, lim) holds the run's lines
  uint8_t* base = text + (g0 - shift);        // 16-byte aligned, as text is
  for (int32_t c = 16 * (int32_t)threadIdx.x; c < lim; c += 16 * dqw::SAMW_RUN) {
    if (c >= shift && c + 16 <= lim) {
      *reinterpret_cast<uint4*>(base + c) = *reinterpret_cast<const uint4*>(tile + c);
    } else {  // the run's first and last 16 bytes: the neighbours' bytes are not touched
      for (int32_t b = c < shift ? shift : c; b < c + 16 && b < lim; b++) base[b] = tile[b];
    }
  }
}

__global__ __launch_bounds__(256) void samw_format_long_kernel(
    const uint8_t* __restrict__ raw, int64_t raw_len, const int64_t* __restrict__ off, int64_t n,
    SamwRefs refs, const int64_t* __restrict__ loff, uint8_t* __restrict__ text) {
  const int lane = threadIdx.x & 63;
  const int64_t nwave = (int64_t)gridDim.x * (blockDim.x >> 6);
  const int64_t total = loff[n];
  for (int64_t j = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); j < n; j += nwave) {
    bool lng;
    const int64_t o = off[j], avail = rec_avail(raw, raw_len, o, &lng);
    if (!lng) continue;  // wave-uniform
    const uint8_t* r = raw + o;
    const int64_t lo = loff[j], sz = loff[j + 1] - lo;
    DQ_CHK(lo >= 0 && sz >= 1 && lo + sz <= total, CHK_SAM);
    if (lo < 0 || sz < 1 || lo + sz > total) continue;  // wave-uniform; never store outside the text
    dqw::Layout L;
    if (dqw::samw_layout(r, avail, &L)) continue;  // (the size pass passed it)
    bool all_ff = true, bad = false;
    wave_qual(r + L.qual_at, L.l_seq, lane, &all_ff, &bad);
    int64_t seq_out = 0, qual_out = 0;
    int32_t star = 1;
    if (lane == 0) {
      dqw::Walk W;
      const int32_t st = dqw::samw_record_walk(r, avail, ref_names(refs), text + lo, sz, true, all_ff, &W);
      DQ_CHK(st == 0 && W.size == sz, CHK_SAM);
      (void)st;
      seq_out = W.seq_out;
      qual_out = W.qual_out;
      star = W.qual_star;
    }
    seq_out = __shfl(seq_out, 0, 64);
    qual_out = __shfl(qual_out, 0, 64);
    star = __shfl(star, 0, 64);
    const int32_t ls = L.l_seq;
    // nothing is stored outside the line, whatever the walk reported
    const bool fits = ls > 0 && seq_out >= 0 && qual_out == seq_out + ls + 1 &&
                      qual_out + (star ? 1 : ls) < sz;
    DQ_CHK(fits || ls == 0, CHK_SAM);
    if (!fits) continue;  // wave-uniform
    uint8_t* T = text + lo;
    const uint8_t* sq = r + L.seq_at;
    const uint8_t* ql = r + L.qual_at;
    // whole groups of eight bases / qualities: a 4- or 8-byte load, an 8-byte store per lane and
    // step (consecutive lanes, consecutive words); the tail of up to seven by bytes
    const int32_t n8 = ls & ~7;
    for (int32_t i = 8 * lane; i < n8; i += 512) {
      const uint64_t w = dqw::samw_seq8((uint32_t)dqw::rd32(sq + (i >> 1)));
      __builtin_memcpy(T + seq_out + i, &w, 8);
      if (!star) {
        uint64_t q;
        __builtin_memcpy(&q, ql + i, 8);
        q += 0x2121212121212121ull;  // every byte <= 93: no carry
        __builtin_memcpy(T + qual_out + i, &q, 8);
      }
    }
    for (int32_t i = n8 + lane; i < ls; i += 64) {
      const uint32_t nib = (sq[i >> 1] >> ((i & 1) ? 0 : 4)) & 15u;
      T[seq_out + i] = (uint8_t)dqw::samw_seq8(nib << 4);
      if (!star) T[qual_out + i] = (uint8_t)(ql[i] + 33);
    }
  }
}

}  // namespace

DQ_CHK_UNIT(samw)

int32_t samw_tile_bytes() { return dqw::SAMW_TILE; }

static unsigned wave_grid(int64_t n) {  // 4 waves per block, grid-stride past 2048 blocks
  const int64_t g = (n + 3) / 4;
  return (unsigned)(g < 1 ? 1 : g > 2048 ? 2048 : g);
}

void launch_samw_sizes(const uint8_t* raw, int64_t raw_len, const int64_t* off, int64_t n,
                       SamwRefs refs, int32_t* status, int64_t* size, unsigned long long* scal,
                       hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(samw_size_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, raw, raw_len,
                     off, n, refs, status, size, scal);
  hipLaunchKernelGGL(samw_size_long_kernel, dim3(wave_grid(n)), dim3(256), 0, s, raw, raw_len, off, n,
                     refs, status, size, scal);
}

void launch_samw_format(const uint8_t* raw, int64_t raw_len, const int64_t* off, int64_t n,
                        SamwRefs refs, const int64_t* loff, uint8_t* text, int32_t use_tile,
                        hipStream_t s) {
  if (n <= 0) return;
  if (((uintptr_t)text & 15) != 0) use_tile = 0;  // the tile's 16-byte stores need an aligned text
  hipLaunchKernelGGL(samw_format_kernel, dim3((unsigned)((n + dqw::SAMW_RUN - 1) / dqw::SAMW_RUN)),
                     dim3(dqw::SAMW_RUN), 0, s, raw, raw_len, off, n, refs, loff, text, use_tile);
  hipLaunchKernelGGL(samw_format_long_kernel, dim3(wave_grid(n)), dim3(256), 0, s, raw, raw_len, off, n,
                     refs, loff, text);
}

}  // namespace dq
