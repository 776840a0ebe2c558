// dq_chain_core.h -- the BGZF block chain of Kernel 1, shared by the kernels (dq_kernels.hip,
// dq_text.hip) and the host check (tools/chain_check.cpp).
//
// The block table of a file is what a walk from the chain start by htsjdk_block gives: start at
// the first block and hop by BSIZE + 1 (BlockCompressedInputStream reads member after member).  The
// kernels do that walk per window of W bytes (chain_window), all windows at once: every window but the
// first speculates its first block (the first position at or after the window start that both
// BgzfBlockGuesser and htsjdk take for a block), walks from there to the window's end, and the
// links are then checked: window i's exit must be window i + 1's speculated start.  A speculation
// that was a member header inside payload breaks its link and is repaired by a walk from the exact
// exit, so the result is the serial chain whatever was speculated.
//
// The planners (plan_blocks_kernel, text_plan_kernel) walk BgzfBlockGuesser's loop over a sorted
// list of magic positions.  The list covers only byte ranges behind the split starts (CandView);
// cand_next answers "the first listed position at or after p" only where the ranges prove it.
#pragma once
#include <stdint.h>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#define __device__
#endif
#endif

#define DQC_INLINE __host__ __device__ inline __attribute__((always_inline))

// Window sizes.  The host picks W per file: about 16 k windows (one wave each), between CHAIN_W_MIN
// and CHAIN_W_MAX, a power of two.  A window of CHAIN_W_MAX >= 65536 bytes that the chain runs
// through holds a block start (a BGZF member is at most 65536 bytes); finer windows may hold none
// (start = -1), which the link rule passes over.  Where a wide window turns out to hold members
// under 1 KiB on average (a run of empty members is 37 k dependent hops per MiB for one wave), the
// count pass gives up and the file is cut into windows of CHAIN_W_DENSE bytes instead.
#ifndef DQ_CHAIN_W
#define DQ_CHAIN_W (1 << 20)
#endif
#ifndef DQ_CHAIN_W_MIN
#define DQ_CHAIN_W_MIN 4096
#endif

namespace dqc {

constexpr int64_t CHAIN_W_MAX = DQ_CHAIN_W, CHAIN_W_MIN = DQ_CHAIN_W_MIN, CHAIN_W_DENSE = 4096;
static_assert(CHAIN_W_MAX >= 65536, "the widest chain window must hold a block start");
static_assert(CHAIN_W_MIN % 16 == 0 && CHAIN_W_MIN <= CHAIN_W_MAX && (CHAIN_W_MAX & (CHAIN_W_MAX - 1)) == 0 &&
              (CHAIN_W_MIN & (CHAIN_W_MIN - 1)) == 0, "chain windows are searched with 16-byte loads");
inline int64_t chain_window(int64_t L) {  // host: the window for a file of L bytes
  int64_t w = CHAIN_W_MIN;
  while (w < CHAIN_W_MAX && w * 16384 < L) w <<= 1;
  return w;
}

constexpr uint32_t BGZF_MAGIC = 0x04088b1fu;

template <typename B>
DQC_INLINE uint32_t ld16(B p, int64_t i) {
  return (uint32_t)p[i] | ((uint32_t)p[i + 1] << 8);
}
template <typename B>
DQC_INLINE int32_t ld32(B p, int64_t i) {
  return (int32_t)((uint32_t)p[i] | ((uint32_t)p[i + 1] << 8) | ((uint32_t)p[i + 2] << 16) |
                   ((uint32_t)p[i + 3] << 24));
}

// The part of BgzfBlockGuesser.guessNextBGZFPos after a magic match at q
// (BgzfBlockGuesser.java:93-144).  Returns 1 (block), 0 (cancelled: scan resumes at q+4) or
// 2 (an IOException: guessNextBGZFPos returns null).  L = readable bytes.
DQC_INLINE int guesser_at(const uint8_t* C, int64_t q, int64_t L, int32_t* cs, int32_t* us) {
  if (q + 12 > L) return 2;
  int64_t xlen = ld16(C, q + 10);
  int64_t p = q + 12;
  const int64_t sub_end = p + xlen;
  while (p < sub_end) {
    if (p + 4 > L) return 2;
    uint32_t id = (uint32_t)ld32(C, p);
    if (id != 0x00024342u) {
      p += 4 + ld16(C, p + 2);
      continue;
    }
    if (p + 6 > L) return 2;
    int64_t bsize = ld16(C, p + 4);
    p += 6;
    while (p < sub_end) {
      if (p + 4 > L) return 2;
      p += 4 + ld16(C, p + 2);
    }
    if (p != sub_end) return 0;
    p += bsize - xlen - 19 + 4;
    if (p < 0 || p + 4 > L) return 2;
    *cs = (int32_t)(p + 4 - q);
    *us = ld32(C, p);
    return 1;
  }
  return 0;
}

// htsjdk reads blocks one after another by BSIZE at header offset 16 and requires XLEN == 6
// (BlockGunzipper.unzipBlock).  B: the bytes, by index (global memory, or an LDS copy of a piece
// with p and L taken from the piece's start).
template <typename B>
DQC_INLINE int htsjdk_block(B C, int64_t p, int64_t L, int32_t* cs) {
  if (p + 18 > L) return 0;
  if ((uint32_t)ld32(C, p) != BGZF_MAGIC || ld16(C, p + 10) != 6) return 0;
  int32_t c = (int32_t)ld16(C, p + 16) + 1;
  if (c < 26 || p + c > L) return 0;
  *cs = c;
  return 1;
}

// A window's speculated start: a position that the guesser returns and htsjdk reads as the same
// member.
DQC_INLINE int spec_at(const uint8_t* C, int64_t q, int64_t L) {
  int32_t gcs = 0, gus = 0, hcs = 0;
  return guesser_at(C, q, L, &gcs, &gus) == 1 && htsjdk_block(C, q, L, &hcs) && hcs == gcs;
}

// One window of the chain: C[ws, we) with we = min(L, ws + W).
struct ChainWin {
  int64_t start;  // the first block taken in the window: speculated, or exact after a repair (-1 none)
  int64_t exit;   // where the walk from start left the window: the first chain position >= we, or
                  // the position at which it stopped
  int64_t count;  // blocks starting in [start, we)
  int64_t usum;   // sum of their ISIZE (as int32, the way blk_us holds them)
  int32_t stop;   // the walk stopped at exit: no htsjdk block there, the chain ends
  int32_t pad;
};

// The walk of one window from `start`: what chain_walk_kernel does per window with the headers in
// LDS or global memory, here over plain memory.  sink.block(k, p, cs, us) takes block k of the walk.
template <typename Sink>
DQC_INLINE void walk_window(const uint8_t* C, int64_t L, int64_t start, int64_t we, ChainWin* w,
                            Sink& sink) {
  int64_t p = start, n = 0, usum = 0;
  int32_t stop = 0;
  while (p < we) {
    int32_t cs;
    if (!htsjdk_block(C, p, L, &cs)) {
      stop = 1;
      break;
    }
    const int32_t us = ld32(C, p + cs - 4);
    sink.block(n, p, cs, us);
    usum += us;
    n++;
    p += cs;
  }
  w->start = start;
  w->exit = p;
  w->count = n;
  w->usum = usum;
  w->stop = stop;
  w->pad = 0;
}
struct NoSink {
  DQC_INLINE void block(int64_t, int64_t, int32_t, int32_t) {}
};

// The link rule.  `in` is the exit of the last earlier window that took a block and in_stop its
// stop flag; window w (bytes up to we) is consistent with it when the chain enters w exactly at
// its speculated start, or passes over a window that speculated none.
DQC_INLINE bool link_ok(int64_t in, int32_t in_stop, const ChainWin& w, int64_t we) {
  if (in_stop) return false;  // the chain ended before this window: nothing after it counts
  return w.start < 0 ? in >= we : in == w.start;
}

// ------------------------------------------------------------------ planner candidates
struct Cand {          // a BgzfBlockGuesser-visible magic position
  int64_t pos;
  int32_t csize;       // guesser cSize (BSIZE + 1 via the BC subfield)
  int32_t usize;       // ISIZE
  int32_t valid;       // 1 = guessNextBGZFPos would return this block; 0 = magic only; 2 = IOException
  int32_t pad;
};

// The sorted candidate list and the byte ranges it covers: every magic position q with q + 4 <= L
// inside a range is listed.  rng: nrng sorted, disjoint, non-adjacent [begin, end) pairs; nullptr =
// the whole file was scanned.
struct CandView {
  const Cand* c;
  int64_t n;
  const int64_t* rng;
  int64_t nrng;
  int64_t L;  // readable bytes
};

constexpr int64_t CAND_UNKNOWN = -2;  // cand_next: the answer lies outside the scanned ranges

// BgzfBlockGuesser's scan from p inside a split ending at e: the index of the first listed
// position at or after p.  v.n when the scan finds none before it ends (off the data, or its first
// hit would be at or past e, where guessNextBGZFPos stops unless the hit is p itself); CAND_UNKNOWN
// when the scanned ranges cannot tell.
DQC_INLINE int64_t cand_next(const CandView& v, int64_t p, int64_t e) {
  int64_t lo = 0, hi = v.n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (v.c[mid].pos < p) lo = mid + 1;
    else hi = mid;
  }
  if (!v.rng) return lo;
  if (p + 4 > v.L) return v.n;  // no magic fits at or after p
  // the range holding p
  int64_t a = 0, b = v.nrng;
  while (a < b) {
    const int64_t mid = (a + b) >> 1;
    if (v.rng[2 * mid] <= p) a = mid + 1;
    else b = mid;
  }
  if (a == 0 || p >= v.rng[2 * a - 1]) return CAND_UNKNOWN;
  const int64_t rend = v.rng[2 * a - 1];
  if (lo < v.n && v.c[lo].pos < rend) return lo;
  // nothing listed in [p, rend): the next hit, if any, lies at or after rend
  if (rend + 4 > v.L || rend >= e) return v.n;
  return CAND_UNKNOWN;
}

// BgzfBlockSource's blocks of a split that ends at e, from its first block j (BgzfBlockSource.java:
// 63-84: blocks while start <= split end): the last block of the table whose position is <= e,
// never before j.  What `while (jl + 1 < nb && pos[jl + 1] <= e) jl++;` from jl = j gives on an
// ascending table, by an upper-bound search in (j, nb): about log2(nb - j) loads instead of one
// dependent load per block of the split.
DQC_INLINE int64_t last_block_le(const int64_t* pos, int64_t nb, int64_t j, int64_t e) {
  int64_t lo = j + 1, hi = nb;  // the first index in (j, nb) with pos > e lies in [lo, hi]
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (pos[mid] <= e) lo = mid + 1;
    else hi = mid;
  }
  return lo - 1;
}

}  // namespace dqc
