// dq_vcf_stage.h -- what the VCF kernels share around their walks (dq_vcf.hip's site walk,
// dq_vcf_gt.hip's genotype walk, dq_vcf_info.hip's INFO walk): the block staging of the
// thread-per-line kernels -- the span of the stream a block's 256 lines cover, copied into LDS --
// a kept variant's line, and the append to a host fix-up list.
#pragma once
#include "dq_internal.h"

namespace dq {
namespace {

// One thread reading its own line loads from 64 cache lines per wave instruction, so a block first
// copies the span of the stream its 256 lines cover into LDS with 16-byte loads (consecutive lanes,
// consecutive words; the lines of the list are ascending in U, so the span runs from the first
// line's start to the last line's end) and the threads walk from there.  A block whose span does
// not fit (long lines among its lines, or kept lines far apart under an interval filter) walks
// from memory; so does a thread whose line lies outside the block's span.  The copy reads whole
// 16-byte words of [lo & ~15, hi): inside the stream, or in the zero bytes behind it.
constexpr int32_t VCF_STAGE = 40960;  // LDS bytes per block: 160 bytes a line

struct StageSpan {
  int64_t lo, hi;  // stage holds the stream's bytes [lo, hi); lo is 16-byte aligned
  bool staged;
};

__device__ inline StageSpan stage_span(const uint8_t* __restrict__ U, int64_t ulen, int64_t first,
                                       int64_t last_end, uint8_t* __restrict__ stage) {
  StageSpan sp;
  sp.lo = first & ~(int64_t)15;
  const int64_t nb = (last_end - sp.lo + 15) & ~(int64_t)15;
  sp.staged = first >= 0 && last_end >= first && last_end <= ulen && nb <= VCF_STAGE;  // block-uniform
  sp.hi = sp.staged ? sp.lo + nb : sp.lo;
  if (sp.staged) {
    for (int64_t i = (int64_t)threadIdx.x * 16; i < nb; i += 256 * 16) {
      DQ_CHK(sp.lo + i + 16 <= ulen + 256 && i + 16 <= VCF_STAGE, CHK_VCF);  // U's zero pad: 256 bytes
      *reinterpret_cast<uint4*>(stage + i) = *reinterpret_cast<const uint4*>(U + sp.lo + i);
    }
  }
  __syncthreads();
  return sp;
}

// The prologue of block j0 / 256 of a thread-per-line kernel over the n kept lines of a list (kept
// == nullptr: over the list's own n lines): the span from the block's first listed line to the end of
// its last one, staged.  Ends in a block barrier (stage_span's).
__device__ inline StageSpan stage_block(const VcfLines& in, int64_t j0, uint8_t* __restrict__ stage) {
  const int64_t jl = j0 + 255 < in.n ? j0 + 255 : in.n - 1;  // j0 < n: the grid has no empty block
  const int64_t tf = in.kept ? in.kept[j0] : j0, tl = in.kept ? in.kept[jl] : jl;
  DQ_CHK(tf >= 0 && tf < in.total && tl >= 0 && tl < in.total, CHK_VCF);
  const bool listed = tf >= 0 && tf < in.total && tl >= 0 && tl < in.total;  // block-uniform
  return stage_span(in.U, in.ulen, listed ? in.vstart[tf] : -1, listed ? in.vstart[tl] + in.vlen[tl] : -1,
                    stage);
}

// the stage holds all of the line U[a, a + len) / where a thread walks that line
__device__ inline bool in_stage(const StageSpan& sp, int64_t a, int32_t len) {
  return sp.staged && a >= sp.lo && a + len <= sp.hi;
}
__device__ inline const uint8_t* stage_line(const StageSpan& sp, const uint8_t* stage, const uint8_t* U,
                                            int64_t a, int32_t len) {
  return in_stage(sp, a, len) ? stage + (a - sp.lo) : U + a;
}

// Variant j's entry *t of the list and its line U[*a, *a + *len): false (a failed check) when
// kept[j] is no entry.  Whether the line lies in U (line_in_u) the caller checks together with its
// own columns, behind their loads, so that no load of variant j waits for another's result.
__device__ inline bool kept_line(const VcfLines& in, int64_t j, int64_t* t, int64_t* a, int32_t* len) {
  *t = in.kept[j];
  DQ_CHK(*t >= 0 && *t < in.total, CHK_VCF);
  if (*t < 0 || *t >= in.total) return false;
  *a = in.vstart[*t];
  *len = in.vlen[*t];
  return true;
}
__device__ inline bool line_in_u(const VcfLines& in, int64_t a, int32_t len) {
  return a >= 0 && len >= 0 && a + len <= in.ulen;
}

// One entry of N words for the host's fix-up pass, behind the cnt entries others appended to fix
// (cap entries: the earlier pass counted them).
template <int N>
__device__ inline void fix_append(int64_t* __restrict__ fix, int64_t cap, unsigned long long* __restrict__ cnt,
                                  const int64_t (&w)[N]) {
  const unsigned long long e = atomicAdd(cnt, 1ull);
  DQ_CHK((int64_t)e < cap, CHK_VCF);
  if ((int64_t)e < cap) {
#pragma unroll
    for (int i = 0; i < N; i++) fix[N * e + i] = w[i];
  }
}

}  // namespace
}  // namespace dq
