// dq_vcf_stage.h -- the block staging of the thread-per-line VCF kernels (dq_vcf.hip's site walk,
// dq_vcf_gt.hip's genotype walk): the span of the stream a block's 256 lines cover, copied into LDS.
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

}  // namespace
}  // namespace dq
