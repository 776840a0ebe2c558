// dq_vcf_gt.hip -- VCF genotype decode: the FORMAT column and the
// sample columns of the variants dq_vcf.hip decoded, into the variants x samples matrix of
// dq_genotype_batch -- what htsjdk's AbstractVCFCodec.createGenotypeMap computes when a consumer
// asks a VariantContext for its genotypes.  The per-cell rules are dq_vcf_gt_core.h (DESIGN.md
// section 16); this file holds the kernels around them.  They run behind the site decode on its
// columns (col_end, n_alt, n_sample_cols of every kept variant) and read the resident stream U:
//   check    the first failing (line, sample, class) by a min, the largest ploidy by a max, the GQ
//            texts left to the host counted; nothing is stored;
//   decode   the same walk with the ploidy known, into the matrix; the host's GQ texts listed.
// The header's sample count S chooses the walk: a thread per line below GT_WAVE_S (a block's lines
// staged in LDS, dq_vcf_stage.h), a wave per line from it on.  Every load of a line lies in
// [value start, value start + len); every store is guarded by its row (j < n, s < S).
#if defined(__HIP_DEVICE_COMPILE__)
#define DQV_CHECK(cond) DQ_CHK(cond, CHK_VCF)
#define DQG_CHECK(cond) DQ_CHK(cond, CHK_VCF)
#define DQT_CHECK(cond) DQ_CHK(cond, CHK_VCF)
#else
#define DQV_CHECK(cond) ((void)0)
#define DQG_CHECK(cond) ((void)0)
#define DQT_CHECK(cond) ((void)0)
#endif
#include "dq_internal.h"
#include "dq_vcf_gt_core.h"
#include "dq_vcf_stage.h"

namespace dq {
namespace {

// sample counts from here on get a wave per line: measured on 512 MB files, both passes, the thread
// walk takes 9.3 ms at 8 samples where the wave walk takes 13.7, and 13.5 at 16 where it takes 9.7
constexpr int32_t GT_WAVE_S = 12;

// a wave's share of LDS: the offsets of the cells its scan has found and not yet decoded, and the
// line's bytes from FORMAT on (a longer tail is read from memory)
constexpr int32_t GT_OFFS = 576;    // a flush leaves room for the 64 TABs of one more ballot
constexpr int32_t GT_WSLOT = 4096;  // bytes

struct HostGqCount {
  int32_t* n;
  __device__ void operator()(int32_t, int32_t, int32_t) const { (*n)++; }
};

struct HostGqList {  // fix-up entries: cell, text offset in U, text length
  int64_t* fix;
  int64_t cap;
  unsigned long long* cnt;
  int64_t cell0, text0;
  __device__ void operator()(int32_t s, int32_t at, int32_t len) const {
    fix_append<3>(fix, cap, cnt, {cell0 + s, text0 + at, len});
  }
};

__device__ inline dqg::GtRow row_of(const GtCols& o, int64_t j, int32_t S, int32_t P) {
  const int64_t c = j * S;
  return dqg::GtRow{o.flags + c, o.ploidy + c, o.allele + c * P, o.gq + c, o.dp + c, o.cell_off + c};
}

__device__ inline void store_blank(const GtCols& o, int64_t cell, int32_t P) {
  o.flags[cell] = 0;
  o.ploidy[cell] = 0;
  for (int32_t i = 0; i < P; i++) o.allele[cell * P + i] = -2;
  o.gq[cell] = -1;
  o.dp[cell] = -1;
  o.cell_off[cell] = 0;
}

__device__ inline int32_t wave_max(int32_t v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const int32_t u = __shfl_xor(v, o);
    v = u > v ? u : v;
  }
  return v;
}

// The variant's line and what the site decode left of it; false (a failed check) when the lists
// disagree.  fmt_at: the byte behind the eighth TAB.
struct GtLineAt {
  int64_t t, a;
  int32_t len, fmt_at, n_alt, nsc;
};
__device__ inline bool line_at(const GtIn& in, int64_t j, GtLineAt* A) {
  if (!kept_line(in.ln, j, &A->t, &A->a, &A->len)) return false;
  A->fmt_at = in.ln.col_end[8 * j + 7] + 1;
  A->n_alt = in.n_alt[j];
  A->nsc = in.n_sample_cols[j];
  const bool ok = line_in_u(in.ln, A->a, A->len) && A->fmt_at >= 1 && A->fmt_at <= A->len;
  DQ_CHK(ok, CHK_VCF);
  return ok;
}

// ---- a thread per line: the few-sample files (a wave per 200-byte line would idle 63 lanes)
template <bool DEC>
__global__ __launch_bounds__(256) void gt_thread_kernel(GtIn in, GtCols out, int32_t P,
                                                         unsigned long long* __restrict__ scal,
                                                         int64_t* __restrict__ fix, int64_t fix_cap) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[VCF_STAGE];
  const int64_t j0 = (int64_t)blockIdx.x * 256, j = j0 + threadIdx.x;
  const StageSpan sp = stage_block(in.ln, j0, stage);
  int32_t maxp = 0;
  GtLineAt A;
  if (j < in.ln.n && line_at(in, j, &A)) {
    const uint8_t* L = stage_line(sp, stage, in.ln.U, A.a, A.len);
    if (DEC) {
      const dqg::GtLine R = dqg::gt_line_walk(L, A.len, A.fmt_at, in.S, A.nsc, A.n_alt, P, row_of(out, j, in.S, P),
                                    HostGqList{fix, fix_cap, scal + 3, j * in.S, A.a});
      // a line the check pass accepted cannot fail here; should it, its cells from the failing one
      // on say nothing
      DQ_CHK(R.st == 0, CHK_VCF);
      if (R.st)
        for (int32_t s = R.sample; s < in.S; s++) store_blank(out, j * in.S + s, P);
    } else {
      int32_t nhost = 0;
      const dqg::GtLine R =
          dqg::gt_line_walk(L, A.len, A.fmt_at, in.S, A.nsc, A.n_alt, 0, dqg::GtRow{}, HostGqCount{&nhost});
      if (R.st) {
        atomicMin(&scal[0], dqg::gt_error_key(in.ln.lidx[A.t], R.sample, R.st));
      } else {
        maxp = R.max_ploidy;
        if (nhost) atomicAdd(&scal[2], (unsigned long long)nhost);
      }
    }
  }
  if (!DEC) {
    maxp = wave_max(maxp);
    if ((threadIdx.x & 63) == 0 && maxp > 0) atomicMax(&scal[1], (unsigned long long)maxp);
  }
}

// ---- a wave per line: the cohort files
// The wave scans the line from its FORMAT column on, 64 bytes a ballot.  A lane holding a TAB knows
// its ordinal -- the TABs before the window plus those below its own lane -- and that TAB opens the
// cell of sample `ordinal` (the first one closes FORMAT), so it writes the cell's start into the
// wave's offset list in LDS: no serial list.  The scanned bytes go to the wave's LDS slot on the way
// when the tail fits.  Once the list is nearly full, or at the line's end, lane i decodes cells
// i, i + 64, ... of the list: the stores of a row are consecutive across lanes.  FORMAT is parsed by
// every lane alike (uniform loads, no broadcast needed).
template <bool DEC>
__global__ __launch_bounds__(256) void gt_wave_kernel(GtIn in, GtCols out, int32_t P,
                                                       unsigned long long* __restrict__ scal,
                                                       int64_t* __restrict__ fix, int64_t fix_cap) {
  __shared__ int32_t offs_all[4 * GT_OFFS];
  __shared__ uint8_t slots[4 * GT_WSLOT];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int32_t* offs = offs_all + w * GT_OFFS;
  uint8_t* slot = slots + w * GT_WSLOT;
  const int64_t nwave = (int64_t)gridDim.x * 4;
  const int32_t S = in.S;
  int32_t maxp = 0;
  for (int64_t j = (int64_t)blockIdx.x * 4 + w; j < in.ln.n; j += nwave) {
    GtLineAt A;
    if (!line_at(in, j, &A)) continue;  // wave-uniform
    if (A.nsc != S) {                   // wave-uniform
      DQ_CHK(!DEC, CHK_VCF);
      if (!DEC && lane == 0) atomicMin(&scal[0], dqg::gt_error_key(in.ln.lidx[A.t], 0, dqg::GT_E_SAMPLES));
      continue;
    }
    // positions from here on count from the FORMAT column's first byte
    const uint8_t* T = in.ln.U + A.a + A.fmt_at;
    const int32_t tl = A.len - A.fmt_at;
    const bool staged = tl <= GT_WSLOT;  // wave-uniform
    const uint8_t* W = staged ? slot : T;
    int32_t cb = 0, cnt = 0;  // the list holds the starts of cells cb, cb + 1, ..., cnt of them; the
                              // TAB before cell 0 closes FORMAT
    bool have_fmt = false, stop = false;
    dqg::GtFormat F{};
    for (int32_t base = 0; base < tl && !stop; base += 64) {
      const int32_t x = base + lane;
      const uint8_t c = x < tl ? T[x] : 0;
      if (staged && x < tl) slot[x] = c;
      const bool tab = x < tl && c == '\t';
      const unsigned long long m = __ballot(tab);
      if (tab) {
        const int32_t o = cnt + (int32_t)__popcll(m & ((1ull << lane) - 1));
        DQ_CHK(o >= 0 && o < GT_OFFS, CHK_VCF);
        if (o < GT_OFFS) offs[o] = x + 1;
      }
      cnt += (int32_t)__popcll(m);
      const bool last = base + 64 >= tl;
      if (!(last || cnt > GT_OFFS - 64)) continue;  // wave-uniform
      // ---- flush: the wave's LDS stores above are read by other lanes below
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (!have_fmt) {
        DQ_CHK(cnt >= 1, CHK_VCF);  // n_sample_cols == S >= 1: a TAB closes FORMAT
        if (cnt < 1) break;
        const int32_t st = dqg::gt_format_parse(W, 0, offs[0] - 1, &F);
        if (st) {
          DQ_CHK(!DEC, CHK_VCF);
          if (!DEC && lane == 0) atomicMin(&scal[0], dqg::gt_error_key(in.ln.lidx[A.t], 0, st));
          break;
        }
        have_fmt = true;
      }
      // the last entry's cell ends where the line does: known only at the line's end
      const int32_t ncell = cnt - (last ? 0 : 1);
      bool bad = false;
      for (int32_t i = lane; i < ncell; i += 64) {
        const int32_t s = cb + i, ca = offs[i], cz = i + 1 < cnt ? offs[i + 1] - 1 : tl;
        DQ_CHK(s < S && ca >= 0 && ca <= cz && cz <= tl, CHK_VCF);
        if (s >= S || ca < 0 || ca > cz || cz > tl) continue;
        const int64_t cell = j * S + s;
        dqg::GtCell C;
        const int32_t st = dqg::gt_cell(W, ca, cz, F, A.n_alt, DEC ? out.allele + cell * P : nullptr, P, &C);
        if (DEC) {
          DQ_CHK(st == 0, CHK_VCF);  // the check pass accepted the cell
          if (st) {
            store_blank(out, cell, P);
            continue;
          }
          if (C.gq_host) HostGqList{fix, fix_cap, scal + 3, cell, A.a + A.fmt_at}(0, C.gq_at, C.gq_len);
          out.flags[cell] = (uint8_t)C.flags;
          out.ploidy[cell] = (uint8_t)C.ploidy;
          out.gq[cell] = C.gq;
          out.dp[cell] = C.dp;
          out.cell_off[cell] = A.fmt_at + ca;
        } else if (st) {
          atomicMin(&scal[0], dqg::gt_error_key(in.ln.lidx[A.t], s, st));
          bad = true;
        } else {
          maxp = C.ploidy > maxp ? C.ploidy : maxp;
          if (C.gq_host) atomicAdd(&scal[2], 1ull);
        }
      }
      if (__any(bad)) stop = true;  // later cells cannot be the line's first offender
      if (!last) {                  // the open cell's start moves to the list's head
        const int32_t carry = offs[cnt - 1];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) offs[0] = carry;
        cb += ncell;
        cnt = 1;
      }
    }
    // the slot and the list are the next line's: its stores wait for this line's loads
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  if (!DEC) {
    maxp = wave_max(maxp);
    if (lane == 0 && maxp > 0) atomicMax(&scal[1], (unsigned long long)maxp);
  }
}

}  // namespace

DQ_CHK_UNIT(vcfgt)

template <bool DEC>
static void launch_gt(GtIn in, GtCols out, int32_t P, unsigned long long* scal, int64_t* fix,
                      int64_t fix_cap, hipStream_t s) {
  if (in.ln.n <= 0 || in.S <= 0) return;
  if (in.S < GT_WAVE_S) {
    hipLaunchKernelGGL(gt_thread_kernel<DEC>, dim3((unsigned)((in.ln.n + 255) / 256)), dim3(256), 0, s, in, out,
                       P, scal, fix, fix_cap);
  } else {  // 4 waves per block, grid-stride past 2048 blocks
    const int64_t g = (in.ln.n + 3) / 4;
    hipLaunchKernelGGL(gt_wave_kernel<DEC>, dim3((unsigned)(g > 2048 ? 2048 : g)), dim3(256), 0, s, in, out,
                       P, scal, fix, fix_cap);
  }
}

void launch_gt_check(GtIn in, unsigned long long* scal, hipStream_t s) {
  launch_gt<false>(in, GtCols{}, 0, scal, nullptr, 0, s);
}

void launch_gt_decode(GtIn in, GtCols out, int32_t P, int64_t* fix, int64_t fix_cap,
                      unsigned long long* scal, hipStream_t s) {
  launch_gt<true>(in, out, P, scal, fix, fix_cap, s);
}

}  // namespace dq
