// dq_text.hip -- BGZF text (VCF) path: the lines Hadoop's TextInputFormat returns per split of a
// BGZF-compressed text file read through Disq's splittable codecs.
//
// Reference behaviour (restated literally in oracle/disq_oracle.c, dqo_text_split_lines):
//   BGZFCodec.createInputStream (D/impl/formats/bgzf/BGZFCodec.java:57-68): the split's stream
//     starts at adjustedStart = guessNextBGZFPos(start, end).pos (end when there is none);
//   BGZFSplitCompressionInputStream (BGZFSplitCompressionInputStream.java:14-106): reads never
//     cross a block; crossing one returns a single byte of the next block and only then advertises
//     getPos = (that block's address) + 1;
//   Hadoop 2.7 LineRecordReader over CompressedSplitLineReader, 4096-byte fills: the first line is
//     thrown away unless adjustedStart == 0, and another line is read while getPos <= end (or one
//     more when a CR ... LF pair straddled a fill).
// Characterisation used here, on the resident decompressed stream U (kernels 1-2 inflate it):
//   * terminators: LF, CR LF, or a lone CR (LineReader.readDefaultLine); line k starts after
//     terminator k - 1;
//   * before reading line k the reader has fetched up to the end of the fill holding the byte it
//     last examined -- the line's own terminator end, or for a lone CR the byte after it -- so
//     getPos <= end  <=>  that byte lies before block B1, the first block after B0 with
//     address >= end (getPos of block B0 itself is its address);
//   * the extra line: needAdditionalRecord is the value set by the last fill that started right
//     after a CR (fills: B0 at U0 + 4096 m; later blocks at U_b, then U_b + 1 + 4096 m).
#include "dq_internal.h"

#include <algorithm>

namespace dq {
namespace {

constexpr int TT = 256;           // threads per terminator-scan workgroup
constexpr int TBY = 32;           // bytes per thread
constexpr int TILE = TT * TBY;    // 8 KiB of U per workgroup
constexpr int FILL = 4096;        // io.file.buffer.size (core-default.xml), LineReader buffer

// Terminator-end mask of the 32 bytes at x0 (bit i: byte x0 + i ends a line).  U holds >= 256
// readable zero bytes past ulen.
__device__ inline uint32_t term_mask(const uint8_t* __restrict__ U, int64_t ulen, int64_t x0) {
  if (x0 >= ulen) return 0u;
  const uint4 a = *reinterpret_cast<const uint4*>(U + x0);
  const uint4 b = *reinterpret_cast<const uint4*>(U + x0 + 16);
  const uint8_t nxt = U[x0 + 32];
  const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  uint32_t lf = 0, cr = 0;
#pragma unroll
  for (int i = 0; i < 32; i++) {
    const uint8_t c = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
    lf |= (uint32_t)(c == '\n') << i;
    cr |= (uint32_t)(c == '\r') << i;
  }
  // a CR followed by LF is the first half of CR LF; the byte after the window is `nxt`
  const uint32_t lf_next = (lf >> 1) | ((uint32_t)(nxt == '\n') << 31);
  uint32_t m = lf | (cr & ~lf_next);
  const int64_t valid = ulen - x0;
  if (valid < 32) {
    m &= (1u << valid) - 1u;
    // a CR as the stream's last byte ends a line (the zero pad is not an LF)
  }
  return m;
}

template <bool EMIT>
__global__ __launch_bounds__(TT) void text_terms_kernel(const uint8_t* __restrict__ U, int64_t ulen,
                                                        int32_t* __restrict__ tile_count,
                                                        const int64_t* __restrict__ tile_off,
                                                        int64_t* __restrict__ term_pos) {
  __shared__ int32_t wsum[TT / 64];
  const int64_t x0 = (int64_t)blockIdx.x * TILE + (int64_t)threadIdx.x * TBY;
  const uint32_t m = term_mask(U, ulen, x0);
  const int c = __popc(m);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // wave inclusive scan
  int inc = c;
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(inc, d, 64);
    if (lane >= d) inc += y;
  }
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  if (!EMIT) {
    if (threadIdx.x == 0) {
      int t = 0;
      for (int w = 0; w < TT / 64; w++) t += wsum[w];
      tile_count[blockIdx.x] = t;
    }
    return;
  }
  int base = 0;
  for (int w = 0; w < wv; w++) base += wsum[w];
  int64_t o = tile_off[blockIdx.x] + base + inc - c;
  uint32_t mm = m;
  while (mm) {
    const int i = __ffs(mm) - 1;
    mm &= mm - 1;
    term_pos[o++] = x0 + i;
  }
}

__device__ inline int64_t lb_i64(const int64_t* a, int64_t n, int64_t v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

struct Lines {
  const uint8_t* U;
  int64_t ulen;
  const int64_t* term;  // terminator end positions, ascending
  int64_t nterm;
  int64_t nl;           // lines
  __device__ int64_t start(int64_t k) const { return k == 0 ? 0 : term[k - 1] + 1; }
  // the byte the reader last examined before reading line k >= 1
  __device__ int64_t examined(int64_t k) const {
    const int64_t u = term[k - 1] + 1;
    return U[u - 1] == '\r' ? u : u - 1;
  }
};

// Per block: the last fill start f (grid of a block read after the split's first block:
// U_b, U_b + 1 + 4096 m) with U[f - 1] == CR, or -1.
__global__ void text_cr_fills_kernel(const uint8_t* __restrict__ U, const int64_t* __restrict__ uoff,
                                     const int32_t* __restrict__ blk_us, int64_t nblk,
                                     int64_t* __restrict__ last_cr_fill) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nblk) return;
  const int64_t ub = uoff[b], n = blk_us[b];
  int64_t r = -1;
  if (n > 0) {
    if (ub > 0 && U[ub - 1] == '\r') r = ub;
    for (int64_t f = ub + 1; f < ub + n; f += FILL)
      if (U[f - 1] == '\r') r = f;
  }
  last_cr_fill[b] = r;
}

// One thread per split: the line index range [k0, k1) it reads.
__global__ void text_plan_kernel(CandList cl, const int64_t* __restrict__ blk_pos,
                                 const int32_t* __restrict__ blk_us,
                                 const int64_t* __restrict__ uoff, int64_t nblk, int64_t flen,
                                 const uint8_t* __restrict__ U, int64_t ulen,
                                 const int64_t* __restrict__ term, int64_t nterm,
                                 const int64_t* __restrict__ last_cr_fill,
                                 TextPlan* __restrict__ plans, int64_t nsplit) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nsplit) return;
  TextPlan& P = plans[i];
  P.k0 = P.k1 = 0;
  P.b0 = -1;
  P.status = 0;
  P.bom = 0;
  const Cand* __restrict__ cand = cl.cand;
  const int64_t s = P.split_start, e = P.split_end, nc = *cl.d_ncand;
  const dqc::CandView V{cand, nc, cl.rng, cl.nrng, cl.L};
  Lines L{U, ulen, term, nterm, 0};
  L.nl = nterm + ((nterm == 0 ? ulen > 0 : term[nterm - 1] + 1 < ulen) ? 1 : 0);
  // ---- BGZFCodec.createInputStream: guessNextBGZFPos(start, end) (BgzfBlockGuesser.java:76-149)
  int64_t A = -1;
  {
    int64_t p = s;
    for (;;) {
      const int64_t lo = dqc::cand_next(V, p, e);
      if (lo == dqc::CAND_UNKNOWN) {  // outside the scanned ranges: the host scans the whole file
        *cl.need_full = 1;
        return;
      }
      if (lo >= nc) break;
      const Cand c = cand[lo];
      if (c.pos != p && c.pos >= e) break;
      if (c.valid == 1) {
        A = c.pos;
        break;
      }
      if (c.valid == 2) break;
      p = c.pos + 4;
    }
  }
  const bool guessed = A >= 0;
  if (!guessed) A = e;  // adjustedStart = end
  const int64_t j = lb_i64(blk_pos, nblk, A);
  if (j >= nblk || blk_pos[j] != A) {
    // the stream would start inside a block: the reference fails reading it, except at the end
    // of the file (an empty stream)
    if (!guessed && A >= flen) return;
    P.status = guessed ? ST_BAD_HEADER : ST_TEXT_START;
    return;
  }
  P.b0 = j;
  if (blk_us[j] == 0) return;  // an empty block: available() == 0, end of stream
  const int64_t U0 = uoff[j];
  // ---- LineRecordReader.initialize: unless the stream starts at 0, drop the first line
  int64_t k0;
  if (A == 0) {
    k0 = 0;
  } else {
    const int64_t t = lb_i64(term, nterm, U0);
    if (t >= nterm) return;  // the dropped line runs to the end
    k0 = t + 1;
    if (k0 >= L.nl) return;
    if (A > e) return;       // readLine saw getPos > end: finished before the first record
  }
  // ---- the lines read while getPos <= end: examined byte before block B1
  int64_t b1 = lb_i64(blk_pos, nblk, e);
  if (b1 <= j) b1 = j + 1;
  const int64_t lim = b1 < nblk ? uoff[b1] : INT64_MAX;
  int64_t lo = k0 == 0 ? 1 : k0, hi = L.nl;  // line 0 (stream start) is read unconditionally
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (L.examined(mid) < lim) lo = mid + 1;
    else hi = mid;
  }
  int64_t k1 = lo;
  // ---- one more line if the last fill after a CR did not start with LF
  if (k1 < L.nl) {
    const int64_t X = L.examined(k1);
    // block holding X
    int64_t bx = lb_i64(uoff, nblk, X + 1) - 1;
    int64_t f = -1;
    if (bx == j) {
      for (int64_t g = U0 + FILL; g <= X; g += FILL)
        if (U[g - 1] == '\r') f = g;
    } else {
      const int64_t ub = uoff[bx];
      if (U[ub - 1] == '\r') f = ub;
      for (int64_t g = ub + 1; g <= X; g += FILL)
        if (U[g - 1] == '\r') f = g;
      for (int64_t b = bx - 1; f < 0 && b > j; b--) f = last_cr_fill[b];
      if (f < 0)
        for (int64_t g = U0 + FILL; g < U0 + blk_us[j]; g += FILL)
          if (U[g - 1] == '\r') f = g;
    }
    if (f >= 0 && U[f] != '\n') k1++;
  }
  // ---- skipUtfByteOrderMark (line 0 only): a value starting EF BB BF loses those bytes, and a
  //      line of only them with no terminator is no record (newSize 0)
  if (k0 == 0 && k1 > 0) {
    int64_t z = ulen, consumed = ulen;
    if (nterm > 0) {
      const int64_t te = term[0];
      z = (U[te] == '\n' && te > 0 && U[te - 1] == '\r') ? te - 1 : te;
      consumed = te + 1;
    }
    if (z >= 3 && U[0] == 0xEF && U[1] == 0xBB && U[2] == 0xBF) {
      P.bom = 1;
      if (consumed == 3) k1 = 0;
    }
  }
  P.k0 = k0;
  P.k1 = k1 < k0 ? k0 : k1;
}

// Values of the listed lines: offset, length (terminator excluded, BOM stripped from line 0 when
// flagged), hash of the value bytes, keep flag (drop '#' lines when asked).  The hash is the
// record hash of DESIGN.md section 4 (8-byte little-endian words, zero padded, keyed by index):
// a line of up to TV_LONG bytes is hashed by its thread from aligned dword loads (one byte-align
// per half word); a longer line is left to text_long_hash_kernel, a wave per line.
constexpr int64_t TV_LONG = 2048;
__device__ inline uint32_t tv_funnel(uint32_t lo, uint32_t hi, uint32_t sh) {  // (hi:lo) >> 8 sh
  return __builtin_amdgcn_alignbyte(hi, lo, sh);
}
// word k of the value at byte a (len bytes), zero padded past len
__device__ inline uint64_t tv_word(const uint32_t* __restrict__ U32, int64_t a, int64_t len, int64_t k) {
  const int64_t wi = (a >> 2) + 2 * k;
  const uint32_t sh = (uint32_t)(a & 3);
  const uint32_t w0 = U32[wi], w1 = U32[wi + 1], w2 = U32[wi + 2];
  uint64_t w = ((uint64_t)tv_funnel(w1, w2, sh) << 32) | tv_funnel(w0, w1, sh);
  const int64_t rem = len - 8 * k;
  if (rem < 8) w &= (1ull << (8 * rem)) - 1;
  return w;
}
__global__ void text_values_kernel(const uint8_t* __restrict__ U, int64_t ulen,
                                   const int64_t* __restrict__ term, int64_t nterm,
                                   const int64_t* __restrict__ idx, int64_t n, int32_t bom,
                                   int32_t drop_hash, int64_t* __restrict__ vstart,
                                   int32_t* __restrict__ vlen, uint64_t* __restrict__ hash,
                                   uint8_t* __restrict__ keep) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int64_t k = idx[t];
  int64_t a = k == 0 ? 0 : term[k - 1] + 1;
  int64_t z;
  if (k < nterm) {
    const int64_t te = term[k];
    z = te;  // exclusive end of the value
    if (U[te] == '\n' && te > a && U[te - 1] == '\r') z = te - 1;
  } else {
    z = ulen;
  }
  if (k == 0 && bom) a += 3;
  const int64_t len = z - a;
  vstart[t] = a;
  vlen[t] = (int32_t)len;
  keep[t] = (uint8_t)!(drop_hash && len > 0 && U[a] == '#');
  if (len > TV_LONG) return;  // text_long_hash_kernel
  const uint32_t* U32 = reinterpret_cast<const uint32_t*>(U);  // U: 256 bytes of slack past ulen
  uint64_t h = (uint64_t)len * DQ_K_LEN;
  const int64_t nw = (len + 7) / 8;
  for (int64_t w = 0; w < nw; w++) h += dq_mix64(tv_word(U32, a, len, w) ^ ((uint64_t)(w + 1) * DQ_K_WORD));
  hash[t] = dq_mix64(h);
}

// Lines longer than TV_LONG: one wave per line (a grid-stride over the lines' lengths), lane l
// hashing words l, l + 64, ... (the word sum is order-free), summed across the wave.
__global__ __launch_bounds__(256) void text_long_hash_kernel(const uint8_t* __restrict__ U,
                                                             const int64_t* __restrict__ vstart,
                                                             const int32_t* __restrict__ vlen,
                                                             int64_t n, uint64_t* __restrict__ hash) {
  const uint32_t* U32 = reinterpret_cast<const uint32_t*>(U);
  const int lane = threadIdx.x & 63;
  const int64_t nwave = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t t = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); t < n; t += nwave) {
    const int64_t len = vlen[t];
    if (len <= TV_LONG) continue;  // wave-uniform
    const int64_t a = vstart[t];
    uint64_t part = 0;
    const int64_t nw = (len + 7) / 8;
    for (int64_t w = lane; w < nw; w += 64) part += dq_mix64(tv_word(U32, a, len, w) ^ ((uint64_t)(w + 1) * DQ_K_WORD));
    for (int o = 32; o >= 1; o >>= 1) {
      const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)part, o, 64);
      const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(part >> 32), o, 64);
      part += ((uint64_t)hi << 32) | lo;
    }
    if (lane == 0) hash[t] = dq_mix64((uint64_t)len * DQ_K_LEN + part);
  }
}

// The same hash of n byte spans of a buffer (the SAM path's records): spans of up to TV_LONG bytes
// here, a thread each; the longer ones by text_long_hash_kernel.
__global__ __launch_bounds__(256) void span_hash_kernel(const uint8_t* __restrict__ base,
                                                        const int64_t* __restrict__ start,
                                                        const int32_t* __restrict__ slen, int64_t n,
                                                        uint64_t* __restrict__ hash) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int64_t len = slen[t];
  if (len > TV_LONG) return;
  const int64_t a = start[t];
  const uint32_t* B32 = reinterpret_cast<const uint32_t*>(base);
  uint64_t h = (uint64_t)len * DQ_K_LEN;
  const int64_t nw = (len + 7) / 8;
  for (int64_t w = 0; w < nw; w++) h += dq_mix64(tv_word(B32, a, len, w) ^ ((uint64_t)(w + 1) * DQ_K_WORD));
  hash[t] = dq_mix64(h);
}

// Line values gathered into a compact byte buffer: one wave per line.
__global__ __launch_bounds__(256) void text_gather_kernel(const uint8_t* __restrict__ U,
                                                          const int64_t* __restrict__ vstart,
                                                          const int32_t* __restrict__ vlen,
                                                          const int64_t* __restrict__ kept,
                                                          const int64_t* __restrict__ out_off,
                                                          int64_t n, uint8_t* __restrict__ out) {
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= n) return;
  const int64_t t = kept[w];
  const int64_t a = vstart[t], o = out_off[w];
  const int32_t len = vlen[t];
  for (int32_t x = threadIdx.x & 63; x < len; x += 64) out[o + x] = U[a + x];
}

// Partition p's kept lines: positions [koff[out_off[p]], koff[out_off[p + 1]]) of the kept list.
__global__ void text_parts_kernel(const int64_t* __restrict__ out_off, const int64_t* __restrict__ koff,
                                  int64_t nsplit, PartRange* __restrict__ parts) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nsplit) return;
  parts[p].begin = koff[out_off[p]];
  parts[p].end = koff[out_off[p + 1]];
  parts[p].digest = 0;
}

// Kept lines' offset, length and hash in kept order (what crosses PCIe on export).
__global__ void text_export_kernel(const int64_t* __restrict__ kept, int64_t n,
                                   const int64_t* __restrict__ vstart, const int32_t* __restrict__ vlen,
                                   const uint64_t* __restrict__ hash, int64_t* __restrict__ o_start,
                                   int32_t* __restrict__ o_len, uint64_t* __restrict__ o_hash) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t t = kept[i];
  o_start[i] = vstart[t];
  o_len[i] = vlen[t];
  o_hash[i] = hash[t];
}

// VcfSource's OverlapDetector filter (D/impl/formats/vcf/VcfSource.java:108-111) on the raw line:
// VariantContext contig = CHROM, start = POS, end = POS + len(REF) - 1, or the INFO END value when
// present (htsjdk AbstractVCFCodec); kept when some interval of that contig overlaps
// [start, end] (1-based, closed).  Intervals per contig are sorted by start with a running
// maximum of their ends, so one binary search answers overlapsAny.
__device__ inline int64_t vcf_field_end(const uint8_t* U, int64_t x, int64_t z) {
  while (x < z && U[x] != '\t') x++;
  return x;
}
__device__ inline int64_t vcf_int(const uint8_t* U, int64_t x, int64_t z, bool* ok) {
  int64_t v = 0;
  bool any = false, neg = false;
  if (x < z && (U[x] == '-' || U[x] == '+')) neg = U[x++] == '-';
  while (x < z && U[x] >= '0' && U[x] <= '9') {
    v = v * 10 + (U[x++] - '0');
    any = true;
  }
  *ok = any;
  return neg ? -v : v;
}

__global__ void vcf_overlap_kernel(const uint8_t* __restrict__ U, const int64_t* __restrict__ vstart,
                                   const int32_t* __restrict__ vlen, int64_t n,
                                   const uint8_t* __restrict__ names, const int32_t* __restrict__ noff,
                                   int32_t nnames, const int32_t* __restrict__ ivbeg,
                                   const int32_t* __restrict__ ivstart,
                                   const int32_t* __restrict__ ivmaxend, uint8_t* __restrict__ keep) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n || !keep[t]) return;
  const int64_t a = vstart[t], z = a + vlen[t];
  const int64_t c1 = vcf_field_end(U, a, z);
  const int64_t clen = c1 - a;
  int cid = -1;
  for (int i = 0; i < nnames && cid < 0; i++) {
    if (noff[i + 1] - noff[i] != clen) continue;
    bool eq = true;
    for (int64_t k = 0; k < clen && eq; k++) eq = U[a + k] == names[noff[i] + k];
    if (eq) cid = i;
  }
  uint8_t k = 0;
  if (cid >= 0 && c1 < z) {
    bool ok = false;
    const int64_t pos = vcf_int(U, c1 + 1, z, &ok);
    const int64_t f2 = vcf_field_end(U, c1 + 1, z);           // end of POS
    const int64_t f3 = vcf_field_end(U, f2 + 1, z);           // end of ID
    const int64_t f4 = vcf_field_end(U, f3 + 1, z);           // end of REF
    int64_t end = pos + (f4 - (f3 + 1)) - 1;
    const int64_t f5 = vcf_field_end(U, f4 + 1, z);           // ALT
    const int64_t f6 = vcf_field_end(U, f5 + 1, z);           // QUAL
    const int64_t f7 = vcf_field_end(U, f6 + 1, z);           // FILTER
    const int64_t f8 = vcf_field_end(U, f7 + 1, z);           // INFO
    for (int64_t x = f7 + 1; x + 4 <= f8; x++) {              // END= at the start of a key
      if ((x == f7 + 1 || U[x - 1] == ';') && U[x] == 'E' && U[x + 1] == 'N' && U[x + 2] == 'D' &&
          U[x + 3] == '=') {
        bool ok2 = false;
        const int64_t e = vcf_int(U, x + 4, f8, &ok2);
        if (ok2) end = e;
        break;
      }
    }
    if (ok) {
      int lo = ivbeg[cid], hi = ivbeg[cid + 1];  // last interval with start <= end
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)ivstart[mid] <= end) lo = mid + 1;
        else hi = mid;
      }
      if (lo > ivbeg[cid] && (int64_t)ivmaxend[lo - 1] >= pos) k = 1;
    }
  }
  keep[t] = k;
}

// ------------------------------------------------------------------ .tbi index build
// htsjdk TabixIndexCreator / BinningIndexBuilder over the resident lines (DESIGN.md "Building the
// .tbi", dq_text_write_tbi): the front half that turns data lines into the key / voff / endp / pos
// arrays of the .bai kernels (dq_kernels.hip), which then build bins, chunks and the linear index.
struct TLine {
  int64_t a0;  // the line's first byte (a BOM on line 0 included)
  int64_t a;   // start of the value (after the BOM)
  int64_t z;   // end of the value (terminator excluded)
  int64_t nx;  // the byte after the terminator (ulen for a last line without one)
};
__device__ inline TLine tbi_line(const uint8_t* __restrict__ U, int64_t ulen,
                                 const int64_t* __restrict__ term, int64_t nterm, int64_t k) {
  TLine L;
  L.a0 = k == 0 ? 0 : term[k - 1] + 1;
  if (k < nterm) {
    const int64_t te = term[k];
    L.z = (U[te] == '\n' && te > L.a0 && U[te - 1] == '\r') ? te - 1 : te;
    L.nx = te + 1;
  } else {
    L.z = L.nx = ulen;
  }
  L.a = L.a0;
  if (k == 0 && L.z >= 3 && U[0] == 0xEF && U[1] == 0xBB && U[2] == 0xBF) L.a = 3;
  return L;
}

__global__ __launch_bounds__(256) void tbi_lines_kernel(const uint8_t* __restrict__ U, int64_t ulen,
                                                        const int64_t* __restrict__ term,
                                                        int64_t nterm, int64_t nl,
                                                        int32_t* __restrict__ flag) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nl) return;
  const TLine L = tbi_line(U, ulen, term, nterm, k);
  flag[k] = L.z > L.a && U[L.a] != '#';
}

__global__ __launch_bounds__(256) void tbi_compact_kernel(const int32_t* __restrict__ flag,
                                                          const int64_t* __restrict__ off,
                                                          int64_t nl, int64_t n,
                                                          int64_t* __restrict__ dl) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nl || !flag[k]) return;
  const int64_t j = off[k];
  DQ_CHK(j >= 0 && j < n, CHK_TBI);
  dl[j] = k;
}

constexpr int64_t TBI_SAT = (int64_t)1 << 40;  // parsed numbers saturate here (far past 2^29)
// One thread reads one line, so a byte load of a wave touches 64 cache lines: the line is read in
// aligned 8-byte words instead (U is 256-byte aligned with 256 readable bytes past ulen).
__device__ inline uint64_t tbi_load8(const uint8_t* __restrict__ U, int64_t x) {  // 8 bytes at any x
  const uint64_t* p = reinterpret_cast<const uint64_t*>(U + (x & ~(int64_t)7));
  const int sh = (int)(x & 7) * 8;
  const uint64_t lo = p[0];
  return sh ? (lo >> sh) | (p[1] << (64 - sh)) : lo;
}
// bit 7 of every zero byte of w (exact per byte)
__device__ inline uint64_t tbi_zero_bytes(uint64_t w) {
  const uint64_t m = 0x7f7f7f7f7f7f7f7full;
  return ~(((w & m) + m) | w | m);
}
// the first byte equal to ch in [x, z), or z (x itself when x >= z)
__device__ inline int64_t tbi_find(const uint8_t* __restrict__ U, int64_t x, int64_t z, uint8_t ch) {
  if (x >= z) return x;
  const uint64_t pat = 0x0101010101010101ull * ch;
  int64_t base = x & ~(int64_t)7;
  uint64_t w = *reinterpret_cast<const uint64_t*>(U + base) ^ pat;
  const int sh = (int)(x & 7) * 8;
  if (sh) w |= ((uint64_t)1 << sh) - 1;  // the bytes before x match nothing
  for (;;) {
    const uint64_t m = tbi_zero_bytes(w);
    if (m) {
      const int64_t p = base + (__builtin_ctzll(m) >> 3);
      return p < z ? p : z;
    }
    base += 8;
    if (base >= z) return z;
    w = *reinterpret_cast<const uint64_t*>(U + base) ^ pat;
  }
}
// decimal digits of [x, y): the value, *ok = non-empty and digits only
__device__ inline int64_t tbi_digits(const uint8_t* __restrict__ U, int64_t x, int64_t y, bool* ok) {
  int64_t v = 0;
  bool good = x < y;
  for (; x < y && good; x += 8) {
    const uint64_t w = tbi_load8(U, x);
    const int c = (int)min((int64_t)8, y - x);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      if (j < c && good) {
        const uint32_t d = (uint32_t)((w >> (8 * j)) & 0xff) - '0';
        if (d > 9) good = false;
        else v = min(v * 10 + (int64_t)d, TBI_SAT);
      }
    }
  }
  *ok = good;
  return v;
}
// [a, a + n) and [b, b + n) hold the same bytes
__device__ inline bool tbi_same(const uint8_t* __restrict__ U, int64_t a, int64_t b, int64_t n) {
  for (int64_t o = 0; o < n; o += 8) {
    uint64_t d = tbi_load8(U, a + o) ^ tbi_load8(U, b + o);
    if (n - o < 8) d &= ((uint64_t)1 << (8 * (n - o))) - 1;
    if (d) return false;
  }
  return true;
}

struct TRec {
  int64_t c1;        // end of CHROM (the first tab, or the value's end)
  int64_t pos, end;  // POS and the end (1-based, closed), end >= pos
  bool ok;           // at least 4 fields, a CHROM, a decimal POS
};
// CHROM, POS, REF and the INFO END of the value [a, z): nothing past the INFO field is read
__device__ inline TRec tbi_parse(const uint8_t* __restrict__ U, int64_t a, int64_t z) {
  TRec R;
  R.ok = false;
  R.pos = R.end = 0;
  R.c1 = tbi_find(U, a, z, '\t');
  if (R.c1 == a || R.c1 >= z) return R;
  const int64_t f2 = tbi_find(U, R.c1 + 1, z, '\t');  // end of POS
  if (f2 >= z) return R;
  const int64_t f3 = tbi_find(U, f2 + 1, z, '\t');    // end of ID
  if (f3 >= z) return R;
  bool num = false;
  R.pos = tbi_digits(U, R.c1 + 1, f2, &num);
  if (!num) return R;
  int64_t g = tbi_find(U, f3 + 1, z, '\t');           // end of REF
  R.end = R.pos + (g - (f3 + 1)) - 1;
  int nf = 4;
  while (nf < 7 && g < z) {                           // ALT, QUAL, FILTER
    g = tbi_find(U, g + 1, z, '\t');
    nf++;
  }
  if (nf == 7 && g < z) {
    const int64_t i0 = g + 1, i1 = tbi_find(U, i0, z, '\t');  // INFO
    const uint32_t key = 'E' | 'N' << 8 | 'D' << 16 | (uint32_t)'=' << 24;
    for (int64_t x = i0; x + 4 <= i1; x = tbi_find(U, x, i1, ';') + 1) {  // x: the start of a key
      if ((uint32_t)tbi_load8(U, x) != key) continue;
      int64_t y = x + 4;                                     // the first END key decides
      const int64_t ye = tbi_find(U, y, i1, ';');
      bool neg = false, okv = false;
      if (y < ye && (U[y] == '-' || U[y] == '+')) neg = U[y++] == '-';
      const int64_t e = tbi_digits(U, y, ye, &okv);
      if (okv) R.end = neg ? -e : e;
      break;
    }
  }
  if (R.end < R.pos) R.end = R.pos;
  R.ok = true;
  return R;
}

// the block holding byte x < ulen of U: the last block starting at or before x (the non-empty one)
__device__ inline int64_t tbi_block(const int64_t* __restrict__ uoff, int64_t nblk, int64_t x) {
  int64_t lo = 0, hi = nblk;  // first block with uoff > x
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (uoff[mid] <= x) lo = mid + 1;
    else hi = mid;
  }
  const int64_t b = lo - 1;
  DQ_CHK(b >= 0 && b < nblk && x - uoff[b >= 0 ? b : 0] < 65536, CHK_TBI);
  return b < 0 ? 0 : b;
}

__device__ inline int32_t tbi_reg2bin(int32_t beg, int32_t end) {  // SAMv1 section 5.3
  --end;
  if (beg >> 14 == end >> 14) return 4681 + (beg >> 14);
  if (beg >> 17 == end >> 17) return 585 + (beg >> 17);
  if (beg >> 20 == end >> 20) return 73 + (beg >> 20);
  if (beg >> 23 == end >> 23) return 9 + (beg >> 23);
  if (beg >> 26 == end >> 26) return 1 + (beg >> 26);
  return 0;
}

// Keys, one thread per data line: fields, file pointers, the run-head flag (CHROM bytes differ from
// the previous data line's) and the checks against that line.  The first offender goes into
// *status by atomic min (line index << 8 | TBI_ST_*; of one line's faults the lowest code).
__global__ __launch_bounds__(256) void tbi_keys_kernel(
    const uint8_t* __restrict__ U, int64_t ulen, const int64_t* __restrict__ term, int64_t nterm,
    const int64_t* __restrict__ dl, int64_t n, const int64_t* __restrict__ uoff,
    const int64_t* __restrict__ blk_pos, int64_t nblk, uint64_t fin, int32_t* __restrict__ pos,
    int32_t* __restrict__ endp, uint64_t* __restrict__ vs, uint64_t* __restrict__ ve,
    int32_t* __restrict__ head, unsigned long long* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t k = dl[i];
  const TLine L = tbi_line(U, ulen, term, nterm, k);
  const TRec R = tbi_parse(U, L.a, L.z);
  unsigned long long bad = 0;
  if (!R.ok) bad = TBI_ST_FORMAT;
  else if (R.pos < 1 || R.end > ((int64_t)1 << 29)) bad = TBI_ST_RANGE;
  int32_t hd = 1;
  if (i > 0) {
    const TLine P = tbi_line(U, ulen, term, nterm, dl[i - 1]);
    const int64_t p1 = tbi_find(U, P.a, P.z, '\t');
    const bool same = p1 - P.a == R.c1 - L.a && tbi_same(U, P.a, L.a, R.c1 - L.a);
    hd = !same;
    if (same && !bad && p1 < P.z) {  // a malformed previous line is its own, earlier offender
      bool num = false;
      const int64_t pp = tbi_digits(U, p1 + 1, tbi_find(U, p1 + 1, P.z, '\t'), &num);
      if (num && pp > R.pos) bad = TBI_ST_UNSORTED;
    }
  }
  if (bad) atomicMin(status, (unsigned long long)k << 8 | bad);
  pos[i] = bad ? 0 : (int32_t)(R.pos - 1);
  endp[i] = bad ? 1 : (int32_t)R.end;
  // virtual offsets: the block's address << 16 | the offset in the block; the line's end lies in
  // the same block unless the line crosses into a later one, and past the stream it is fin
  const int64_t b = tbi_block(uoff, nblk, L.a0);
  vs[i] = ((uint64_t)blk_pos[b] << 16) | (uint64_t)(L.a0 - uoff[b]);
  uint64_t e = fin;
  if (L.nx < ulen) {
    const int64_t b2 = L.nx < uoff[b + 1] ? b : tbi_block(uoff, nblk, L.nx);
    e = ((uint64_t)blk_pos[b2] << 16) | (uint64_t)(L.nx - uoff[b2]);
  }
  ve[i] = e;
  head[i] = hd;
}

// Runs: run = rank of the line's run head; key = run << 16 | bin.  meta[5 run + 0..4] = ~(first
// data line), last data line + 1, lines, 0, last linear window + 1 (the layout of
// bai_keys_kernel).  The last window is a maximum over the run, wave-reduced so that one lane per
// distinct run of the wave issues the atomic; a run is a contiguous range of data lines, so the
// other words follow from the heads' positions (tbi_meta_kernel) without atomics on one address.
// A run's head records its data-line and line index and where its CHROM bytes lie.
__global__ __launch_bounds__(256) void tbi_runs_kernel(
    const uint8_t* __restrict__ U, int64_t ulen, const int64_t* __restrict__ term, int64_t nterm,
    const int64_t* __restrict__ dl, int64_t n, const int32_t* __restrict__ head,
    const int64_t* __restrict__ hoff, int64_t nrun, const int32_t* __restrict__ pos,
    const int32_t* __restrict__ endp, uint64_t* __restrict__ key,
    unsigned long long* __restrict__ meta, int64_t* __restrict__ nfirst,
    int64_t* __restrict__ nline, int64_t* __restrict__ nstart, int32_t* __restrict__ nlen) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool act = i < n;
  int32_t run = -1, we = -1;
  if (act) {
    const int32_t hd = head[i];
    const int64_t r = hoff[i] + hd - 1;
    DQ_CHK(r >= 0 && r < nrun, CHK_TBI);
    if (r < 0 || r >= nrun) {
      act = false;
    } else {
      run = (int32_t)r;
      const int32_t e = endp[i];
      key[i] = (uint64_t)r << 16 | (uint64_t)tbi_reg2bin(pos[i], e);
      we = (e - 1) >> 14;
      if (hd) {
        const int64_t k = dl[i];
        const TLine L = tbi_line(U, ulen, term, nterm, k);
        nfirst[r] = i;
        nline[r] = k;
        nstart[r] = L.a;
        nlen[r] = (int32_t)min(tbi_find(U, L.a, L.z, '\t') - L.a, (int64_t)INT32_MAX);
      }
    }
  }
  uint64_t rem = __ballot(act);
  while (rem) {
    const int l = __builtin_ctzll(rem);
    const int32_t r = __shfl(run, l);
    const bool mine = act && run == r;
    const uint64_t m = __ballot(mine);
    int32_t wmax = mine ? we : -1;
    for (int o = 32; o > 0; o >>= 1) wmax = max(wmax, __shfl_xor(wmax, o));
    if (lane == l) atomicMax(meta + 5 * (int64_t)r + 4, (unsigned long long)(wmax + 1));
    rem &= ~m;
  }
}
__global__ __launch_bounds__(256) void tbi_meta_kernel(const int64_t* __restrict__ nfirst,
                                                       int64_t nrun, int64_t n,
                                                       unsigned long long* __restrict__ meta) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nrun) return;
  const int64_t first = nfirst[r], last1 = r + 1 < nrun ? nfirst[r + 1] : n;
  DQ_CHK(first >= 0 && first < last1 && last1 <= n, CHK_TBI);
  meta[5 * r + 0] = ~(unsigned long long)first;
  meta[5 * r + 1] = (unsigned long long)last1;
  meta[5 * r + 2] = (unsigned long long)(last1 - first);
}

__global__ __launch_bounds__(256) void tbi_names_kernel(const uint8_t* __restrict__ U,
                                                        const int64_t* __restrict__ nstart,
                                                        const int32_t* __restrict__ nlen,
                                                        const int64_t* __restrict__ noff,
                                                        int64_t nrun, int64_t nbytes,
                                                        uint8_t* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nrun) return;
  const int64_t a = nstart[r], o = noff[r], len = noff[r + 1] - o;  // 0: the host left the run out
  DQ_CHK(o >= 0 && len >= 0 && len <= nlen[r] && o + len <= nbytes, CHK_TBI);
  if (o < 0 || o + len > nbytes) return;
  for (int64_t x = 0; x < len; x++) out[o + x] = U[a + x];
}

}  // namespace

static inline dim3 tbi_grid(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

void launch_tbi_lines(const uint8_t* U, int64_t ulen, const int64_t* term, int64_t nterm, int64_t nl,
                      int32_t* flag, hipStream_t s) {
  if (nl <= 0) return;
  hipLaunchKernelGGL(tbi_lines_kernel, tbi_grid(nl), dim3(256), 0, s, U, ulen, term, nterm, nl, flag);
}

void launch_tbi_compact(const int32_t* flag, const int64_t* off, int64_t nl, int64_t n, int64_t* dl,
                        hipStream_t s) {
  if (nl <= 0) return;
  hipLaunchKernelGGL(tbi_compact_kernel, tbi_grid(nl), dim3(256), 0, s, flag, off, nl, n, dl);
}

void launch_tbi_keys(const uint8_t* U, int64_t ulen, const int64_t* term, int64_t nterm,
                     const int64_t* dl, int64_t n, const int64_t* uoff, const int64_t* blk_pos,
                     int64_t nblk, uint64_t fin, int32_t* pos, int32_t* endp, uint64_t* vs,
                     uint64_t* ve, int32_t* head, unsigned long long* status, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(tbi_keys_kernel, tbi_grid(n), dim3(256), 0, s, U, ulen, term, nterm, dl, n,
                     uoff, blk_pos, nblk, fin, pos, endp, vs, ve, head, status);
}

void launch_tbi_runs(const uint8_t* U, int64_t ulen, const int64_t* term, int64_t nterm,
                     const int64_t* dl, int64_t n, const int32_t* head, const int64_t* hoff,
                     int64_t nrun, const int32_t* pos, const int32_t* endp, uint64_t* key,
                     unsigned long long* meta, int64_t* nfirst, int64_t* nline, int64_t* nstart,
                     int32_t* nlen, hipStream_t s) {
  if (n <= 0 || nrun <= 0) return;
  hipLaunchKernelGGL(tbi_runs_kernel, tbi_grid(n), dim3(256), 0, s, U, ulen, term, nterm, dl, n,
                     head, hoff, nrun, pos, endp, key, meta, nfirst, nline, nstart, nlen);
  hipLaunchKernelGGL(tbi_meta_kernel, tbi_grid(nrun), dim3(256), 0, s, nfirst, nrun, n, meta);
}

void launch_tbi_names(const uint8_t* U, const int64_t* nstart, const int32_t* nlen,
                      const int64_t* noff, int64_t nrun, int64_t nbytes, uint8_t* out, hipStream_t s) {
  if (nrun <= 0) return;
  hipLaunchKernelGGL(tbi_names_kernel, tbi_grid(nrun), dim3(256), 0, s, U, nstart, nlen, noff, nrun,
                     nbytes, out);
}

void launch_vcf_overlap(const uint8_t* U, const int64_t* vstart, const int32_t* vlen, int64_t n,
                        const uint8_t* names, const int32_t* noff, int32_t nnames,
                        const int32_t* ivbeg, const int32_t* ivstart, const int32_t* ivmaxend,
                        uint8_t* keep, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(vcf_overlap_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, U,
                     vstart, vlen, n, names, noff, nnames, ivbeg, ivstart, ivmaxend, keep);
}

void launch_text_parts(const int64_t* out_off, const int64_t* koff, int64_t nsplit, PartRange* parts,
                       hipStream_t s) {
  if (nsplit <= 0) return;
  hipLaunchKernelGGL(text_parts_kernel, dim3((unsigned)((nsplit + 255) / 256)), dim3(256), 0, s,
                     out_off, koff, nsplit, parts);
}

void launch_text_export(const int64_t* kept, int64_t n, const int64_t* vstart, const int32_t* vlen,
                        const uint64_t* hash, int64_t* o_start, int32_t* o_len, uint64_t* o_hash,
                        hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(text_export_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, kept, n,
                     vstart, vlen, hash, o_start, o_len, o_hash);
}

void launch_text_terms(const uint8_t* U, int64_t ulen, int32_t* tile_count, const int64_t* tile_off,
                       int64_t* term_pos, bool emit, hipStream_t s) {
  const int64_t nt = (ulen + TILE - 1) / TILE;
  if (nt <= 0) return;
  if (emit)
    hipLaunchKernelGGL(text_terms_kernel<true>, dim3((unsigned)nt), dim3(TT), 0, s, U, ulen,
                       tile_count, tile_off, term_pos);
  else
    hipLaunchKernelGGL(text_terms_kernel<false>, dim3((unsigned)nt), dim3(TT), 0, s, U, ulen,
                       tile_count, tile_off, term_pos);
}
int64_t text_tiles(int64_t ulen) { return (ulen + TILE - 1) / TILE; }

void launch_span_hash(const uint8_t* base, const int64_t* start, const int32_t* len, int64_t n,
                      uint64_t* hash, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(span_hash_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, base, start,
                     len, n, hash);
  const unsigned g = (unsigned)std::min<int64_t>(2048, (n + 3) / 4);
  hipLaunchKernelGGL(text_long_hash_kernel, dim3(g), dim3(256), 0, s, base, start, len, n, hash);
}

void launch_text_cr_fills(const uint8_t* U, const int64_t* uoff, const int32_t* blk_us, int64_t nblk,
                          int64_t* last_cr_fill, hipStream_t s) {
  if (nblk <= 0) return;
  hipLaunchKernelGGL(text_cr_fills_kernel, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, s, U,
                     uoff, blk_us, nblk, last_cr_fill);
}

void launch_text_plan(CandList cl, const int64_t* blk_pos,
                      const int32_t* blk_us, const int64_t* uoff, int64_t nblk, int64_t flen,
                      const uint8_t* U, int64_t ulen, const int64_t* term, int64_t nterm,
                      const int64_t* last_cr_fill, TextPlan* plans, int64_t nsplit, hipStream_t s) {
  if (nsplit <= 0) return;
  hipLaunchKernelGGL(text_plan_kernel, dim3((unsigned)((nsplit + 63) / 64)), dim3(64), 0, s, cl,
                     blk_pos, blk_us, uoff, nblk, flen, U, ulen, term, nterm, last_cr_fill,
                     plans, nsplit);
}

void launch_text_values(const uint8_t* U, int64_t ulen, const int64_t* term, int64_t nterm,
                        const int64_t* idx, int64_t n, int32_t bom, int32_t drop_hash,
                        int64_t* vstart, int32_t* vlen, uint64_t* hash, uint8_t* keep,
                        hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(text_values_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, U, ulen,
                     term, nterm, idx, n, bom, drop_hash, vstart, vlen, hash, keep);
  const int64_t nwg = std::min<int64_t>((n + 3) / 4, 4096);  // 4 waves per workgroup
  hipLaunchKernelGGL(text_long_hash_kernel, dim3((unsigned)nwg), dim3(256), 0, s, U, vstart, vlen, n,
                     hash);
}

void launch_text_gather(const uint8_t* U, const int64_t* vstart, const int32_t* vlen,
                        const int64_t* kept, const int64_t* out_off, int64_t n, uint8_t* out,
                        hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(text_gather_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, U, vstart,
                     vlen, kept, out_off, n, out);
}

DQ_CHK_UNIT(text)

}  // namespace dq
