// dq_vcf.hip -- VCF site decode: the lines of the BGZF text path
// (dq_text.hip) decoded into the columns htsjdk's VCFCodec.decode computes eagerly, the step
// VcfSource.getVariants runs between the '#' filter and the overlap filter
// (D/impl/formats/vcf/VcfSource.java:102-116).  The per-line rules are dq_vcf_core.h (DESIGN.md
// section 15); this file holds the kernels around them.  They run behind the text pipeline on its
// arrays (value start / length of every line of the kept splits) and read the resident stream U:
//   validate   every line of the kept splits that does not start with '#', before the overlap
//              filter (Disq decodes, then filters): a thread per line of up to VCF_LONG bytes
//              (a block's lines staged in LDS), a wave per longer one; the first failing line by a
//              min over line indices, the undecided QUAL texts counted;
//   decode     the lines that survive the overlap filter, by the same walk, into the columns; the
//              undecided QUAL texts listed for the host;
//   gather     the first col_end[7] bytes of every variant (the SITES export), a wave per line.
// Every load of a line lies in [value start, value start + len); the LDS staging copies whole
// 16-byte words of a block's span of the stream, which end inside the zero bytes behind it.
#if defined(__HIP_DEVICE_COMPILE__)
#define DQV_CHECK(cond) DQ_CHK(cond, CHK_VCF)
#define DQT_CHECK(cond) DQ_CHK(cond, CHK_VCF)
#else
#define DQV_CHECK(cond) ((void)0)
#define DQT_CHECK(cond) ((void)0)
#endif
#include "dq_internal.h"
#include "dq_vcf_core.h"
#include "dq_vcf_stage.h"

namespace dq {
namespace {

constexpr int32_t VCF_LONG = 2048;  // longer lines get a wave (the text path's TV_LONG)

// The first 8 TABs of a long line, found by the whole wave 64 bytes at a time (every lane ends with
// the same list); with `count` the scan goes on to the line's end and counts every TAB.
__device__ inline dqv::VcfTabs wave_tabs(const uint8_t* __restrict__ L, int32_t len, int lane,
                                         bool count) {
  dqv::VcfTabs tb{};
  int32_t total = 0;
  for (int32_t base = 0; base < len && (count || tb.n < 8); base += 64) {
    const int32_t x = base + lane;
    unsigned long long m = __ballot(x < len && L[x] == '\t');
    total += __popcll(m);
    while (m && tb.n < 8) {
      const int32_t at = base + (int32_t)__builtin_ctzll(m);
      m &= m - 1;
#pragma unroll
      for (int c = 0; c < 8; c++)  // compile-time indices keep the list in registers
        if (c == tb.n) tb.at[c] = at;
      tb.n++;
    }
  }
  tb.total = count ? total : -1;
  return tb;
}

// Lane 0 walks a long line's eight site columns; one lane reading memory byte after byte waits a
// full memory latency for each, so the wave first copies those columns -- L[0, the 8th TAB), all a
// walk with the TABs handed in reads -- into its slot of LDS, 64 bytes an instruction.  A site
// longer than the slot (a long INFO, a line without genotype columns) is walked from memory.
constexpr int32_t VCF_WSLOT = 1024;  // LDS bytes per wave
__device__ inline const uint8_t* wave_site(const uint8_t* __restrict__ L, int32_t len, bool G,
                                           const dqv::VcfTabs& tb, int lane, uint8_t* __restrict__ slot) {
  const int32_t site = G ? (tb.n >= 8 ? tb.at[7] : 0) : len;  // wave-uniform
  DQ_CHK(site >= 0 && site <= len, CHK_VCF);
  if (site > VCF_WSLOT || site > len) return L;
  for (int32_t x = lane; x < site; x += 64) slot[x] = L[x];
  __builtin_amdgcn_wave_barrier();  // the wave's LDS stores are issued before lane 0's loads
  return slot;
}

// the line behind entry t of the text path's list: false for a '#' line (the filter of
// VcfSource.java:108)
__device__ inline bool data_line(const uint8_t* __restrict__ U, int64_t ulen, int64_t a, int32_t len) {
  DQ_CHK(a >= 0 && len >= 0 && a + len <= ulen, CHK_VCF);
  return !(len > 0 && U[a] == '#');
}

// ---- the lines of up to VCF_LONG bytes, a thread per line (their staging: dq_vcf_stage.h)
__global__ __launch_bounds__(256) void vcf_validate_kernel(
    const uint8_t* __restrict__ U, int64_t ulen, const int64_t* __restrict__ vstart,
    const int32_t* __restrict__ vlen, const int64_t* __restrict__ lidx, int64_t n, int32_t G,
    dqt::NameTable ctg, unsigned long long* __restrict__ scal) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[VCF_STAGE];
  const int64_t t0 = (int64_t)blockIdx.x * 256, t = t0 + threadIdx.x;
  const StageSpan sp = stage_block(VcfLines{U, ulen, vstart, vlen, lidx, n, nullptr, n, nullptr}, t0, stage);
  if (t >= n) return;
  const int32_t len = vlen[t];
  if (len > VCF_LONG) return;  // vcf_validate_long_kernel
  const int64_t a = vstart[t];
  if (!data_line(U, ulen, a, len)) return;
  dqv::VcfSite S;
  // two calls: the walk's loads are LDS loads in one and memory loads in the other, not flat ones
  const int32_t st = in_stage(sp, a, len)
                         ? dqv::vcf_line_walk(stage + (a - sp.lo), len, G != 0, ctg, nullptr, false, &S)
                         : dqv::vcf_line_walk(U + a, len, G != 0, ctg, nullptr, false, &S);
  if (st) atomicMin(&scal[0], (unsigned long long)lidx[t] << 8 | (unsigned long long)st);
  else if (S.qual_undecided) atomicAdd(&scal[1], 1ull);
}

__global__ __launch_bounds__(256) void vcf_validate_long_kernel(
    const uint8_t* __restrict__ U, int64_t ulen, const int64_t* __restrict__ vstart,
    const int32_t* __restrict__ vlen, const int64_t* __restrict__ lidx, int64_t n, int32_t G,
    dqt::NameTable ctg, unsigned long long* __restrict__ scal) {
  __shared__ uint8_t slots[4 * VCF_WSLOT];
  const int lane = threadIdx.x & 63;
  const int64_t nwave = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t t = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); t < n; t += nwave) {
    const int32_t len = vlen[t];
    if (len <= VCF_LONG) continue;  // wave-uniform
    const int64_t a = vstart[t];
    if (!data_line(U, ulen, a, len)) continue;  // wave-uniform
    const dqv::VcfTabs tb = wave_tabs(U + a, len, lane, false);
    const uint8_t* W = wave_site(U + a, len, G != 0, tb, lane, slots + (threadIdx.x >> 6) * VCF_WSLOT);
    if (lane == 0) {
      dqv::VcfSite S;
      const int32_t st = W == U + a
                             ? dqv::vcf_line_walk(U + a, len, G != 0, ctg, &tb, false, &S)
                             : dqv::vcf_line_walk(slots + (threadIdx.x >> 6) * VCF_WSLOT, len, G != 0,
                                                  ctg, &tb, false, &S);
      if (st) atomicMin(&scal[0], (unsigned long long)lidx[t] << 8 | (unsigned long long)st);
      else if (S.qual_undecided) atomicAdd(&scal[1], 1ull);
    }
  }
}

// ---- decode
__device__ inline void store_site(const VcfCols& o, int64_t j, int64_t n, const dqv::VcfSite& S,
                                  int64_t text_off, int64_t* __restrict__ fix, int64_t fix_cap,
                                  unsigned long long* __restrict__ fix_cnt) {
  DQ_CHK(j >= 0 && j < n, CHK_VCF);
  o.contig[j] = S.contig;
  o.pos[j] = S.pos;
  o.end[j] = S.end;
  o.flags[j] = S.flags;
  o.qual[j] = S.qual;
#pragma unroll
  for (int c = 0; c < 8; c++) o.col_end[8 * j + c] = S.col_end[c];
  o.n_alt[j] = S.n_alt;
  o.n_filter[j] = S.n_filter;
  o.n_info[j] = S.n_info;
  o.n_sample_cols[j] = S.n_sample_cols;
  o.site_len[j] = S.col_end[7];
  if (S.qual_undecided)  // variant, text offset in U, text length
    fix_append<3>(fix, fix_cap, fix_cnt, {j, text_off + S.col_end[4] + 1, S.col_end[5] - S.col_end[4] - 1});
}

// a line the validate pass accepted cannot fail here; should it, the row says so and nothing of it
// is exported as a site
__device__ inline void blank_site(dqv::VcfSite* S) {
  *S = dqv::VcfSite{};
  S->contig = -1;
}

__global__ __launch_bounds__(256) void vcf_decode_kernel(
    const uint8_t* __restrict__ U, int64_t ulen, const int64_t* __restrict__ vstart,
    const int32_t* __restrict__ vlen, int64_t total, const int64_t* __restrict__ kept, int64_t n,
    int32_t G, dqt::NameTable ctg, VcfCols out, int64_t* __restrict__ fix, int64_t fix_cap,
    unsigned long long* __restrict__ fix_cnt) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[VCF_STAGE];
  const int64_t j0 = (int64_t)blockIdx.x * 256, j = j0 + threadIdx.x;
  const StageSpan sp = stage_block(VcfLines{U, ulen, vstart, vlen, nullptr, total, kept, n, nullptr}, j0, stage);
  if (j >= n) return;
  const int64_t t = kept[j];
  DQ_CHK(t >= 0 && t < total, CHK_VCF);
  if (t < 0 || t >= total) return;
  const int32_t len = vlen[t];
  if (len > VCF_LONG) return;  // vcf_decode_long_kernel
  const int64_t a = vstart[t];
  DQ_CHK(a >= 0 && len >= 0 && a + len <= ulen, CHK_VCF);
  dqv::VcfSite S;
  // two calls: the walk's loads are LDS loads in one and memory loads in the other, not flat ones
  const int32_t st = in_stage(sp, a, len)
                         ? dqv::vcf_line_walk(stage + (a - sp.lo), len, G != 0, ctg, nullptr, true, &S)
                         : dqv::vcf_line_walk(U + a, len, G != 0, ctg, nullptr, true, &S);
  DQ_CHK(st == 0, CHK_VCF);
  if (st) blank_site(&S);
  store_site(out, j, n, S, a, fix, fix_cap, fix_cnt);
}

__global__ __launch_bounds__(256) void vcf_decode_long_kernel(
    const uint8_t* __restrict__ U, int64_t ulen, const int64_t* __restrict__ vstart,
    const int32_t* __restrict__ vlen, int64_t total, const int64_t* __restrict__ kept, int64_t n,
    int32_t G, dqt::NameTable ctg, VcfCols out, int64_t* __restrict__ fix, int64_t fix_cap,
    unsigned long long* __restrict__ fix_cnt) {
  __shared__ uint8_t slots[4 * VCF_WSLOT];
  const int lane = threadIdx.x & 63;
  const int64_t nwave = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t j = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); j < n; j += nwave) {
    const int64_t t = kept[j];
    DQ_CHK(t >= 0 && t < total, CHK_VCF);
    if (t < 0 || t >= total) continue;  // wave-uniform
    const int32_t len = vlen[t];
    if (len <= VCF_LONG) continue;  // wave-uniform
    const int64_t a = vstart[t];
    DQ_CHK(a >= 0 && a + len <= ulen, CHK_VCF);
    const dqv::VcfTabs tb = wave_tabs(U + a, len, lane, G != 0);
    const uint8_t* W = wave_site(U + a, len, G != 0, tb, lane, slots + (threadIdx.x >> 6) * VCF_WSLOT);
    if (lane == 0) {
      dqv::VcfSite S;
      const int32_t st = W == U + a
                             ? dqv::vcf_line_walk(U + a, len, G != 0, ctg, &tb, true, &S)
                             : dqv::vcf_line_walk(slots + (threadIdx.x >> 6) * VCF_WSLOT, len, G != 0,
                                                  ctg, &tb, true, &S);
      DQ_CHK(st == 0, CHK_VCF);
      if (st) blank_site(&S);
      store_site(out, j, n, S, a, fix, fix_cap, fix_cnt);
    }
  }
}

// ---- SITES export: variant j's first len[j] bytes at out[out_off[j]], one wave per variant
// (text_gather_kernel's scheme over the compacted starts)
__global__ __launch_bounds__(256) void vcf_gather_kernel(const uint8_t* __restrict__ U, int64_t ulen,
                                                         const int64_t* __restrict__ start,
                                                         const int32_t* __restrict__ len,
                                                         const int64_t* __restrict__ out_off,
                                                         int64_t n, uint8_t* __restrict__ out) {
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= n) return;
  const int64_t a = start[w], o = out_off[w], total = out_off[n];
  const int32_t l = len[w];
  const bool fits = a >= 0 && l >= 0 && a + l <= ulen && o >= 0 && o + l <= total;
  DQ_CHK(fits, CHK_VCF);
  if (!fits) return;  // wave-uniform; never store outside the buffer
  for (int32_t x = threadIdx.x & 63; x < l; x += 64) out[o + x] = U[a + x];
}

}  // namespace

DQ_CHK_UNIT(vcf)

static unsigned wave_grid(int64_t n) {  // 4 waves per block, grid-stride past 2048 blocks
  const int64_t g = (n + 3) / 4;
  return (unsigned)(g < 1 ? 1 : g > 2048 ? 2048 : g);
}

void launch_vcf_validate(const uint8_t* U, int64_t ulen, const int64_t* vstart, const int32_t* vlen,
                         const int64_t* lidx, int64_t n, int32_t G, dqt::NameTable ctg,
                         unsigned long long* scal, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(vcf_validate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, U, ulen,
                     vstart, vlen, lidx, n, G, ctg, scal);
  hipLaunchKernelGGL(vcf_validate_long_kernel, dim3(wave_grid(n)), dim3(256), 0, s, U, ulen, vstart,
                     vlen, lidx, n, G, ctg, scal);
}

void launch_vcf_decode(const uint8_t* U, int64_t ulen, const int64_t* vstart, const int32_t* vlen,
                       int64_t total, const int64_t* kept, int64_t n, int32_t G, dqt::NameTable ctg,
                       VcfCols out, int64_t* fix, int64_t fix_cap, unsigned long long* fix_cnt,
                       hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(vcf_decode_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, U, ulen,
                     vstart, vlen, total, kept, n, G, ctg, out, fix, fix_cap, fix_cnt);
  hipLaunchKernelGGL(vcf_decode_long_kernel, dim3(wave_grid(n)), dim3(256), 0, s, U, ulen, vstart,
                     vlen, total, kept, n, G, ctg, out, fix, fix_cap, fix_cnt);
}

void launch_vcf_gather(const uint8_t* U, int64_t ulen, const int64_t* start, const int32_t* len,
                       const int64_t* out_off, int64_t n, uint8_t* out, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(vcf_gather_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, U, ulen, start,
                     len, out_off, n, out);
}

}  // namespace dq
