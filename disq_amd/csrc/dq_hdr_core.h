// dq_hdr_core.h -- the header of one DEFLATE block (RFC 1951 3.2.3, 3.2.7) decoded serially: what
// one lane of inflate_header_kernel (dq_inflate3.hip) does for one BGZF block, and what the host
// checks run (tools/hdr_core_check.cpp).  The code-length sequence of a dynamic header is at most
// 316 symbols and strictly serial; one lane decodes it in a few thousand instructions, and 64
// blocks share one wave's instruction stream.
//
// The caller supplies three small objects, so the same text runs over a host buffer and over
// global memory + LDS:
//   Src:  uint32_t word(uint32_t i)        32-bit word i of the compressed data (the source clamps
//                                          i to what it may read: hdr_decode never reads more than
//                                          HDR_WORDS words from the word of the header's first bit).
//                                          The words are asked for in increasing order, the first
//                                          one being the word of the header's first bit, and each
//                                          once: a source may read ahead and keep state
//         void ahead(uint32_t i)           before every length symbol, outside any branch on the
//                                          header's bits: word i is the next one to be asked for,
//                                          at most one word is asked for before the next call, and
//                                          at most six before the first.  A source that reads ahead
//                                          moves its window here (all lanes of a wave at once)
//   Tbl:  void set(uint32_t k, uint32_t v) entry k < 128 of the code-length code's 7-bit decode
//         uint32_t get(uint32_t k)         table (sym << 3 | len, one byte; 0 = no code)
//   Sink: void run(uint32_t i, uint32_t n, uint32_t v)
//                                          the n (1..6) symbol slots from i on have the code length
//                                          v (1..15); slots in the layout the kernels' build_tables
//                                          reads: litlen at [0, 288), distance at [288, 320), a run
//                                          lies in one of them.  Called with increasing i; zero
//                                          lengths are not sent (the sink starts zero filled).
//                                          Summed per v and alphabet, n gives the numbers of codes
//                                          of each length (at most 286 and 30): what a canonical
//                                          code is built from
//         void mark(int k)                 a phase of the decode ends (k = 0 the code-length code's
//                                          lengths are read, 1 its table is filled, 2 the length
//                                          loop is over; not called on every early return): for a
//                                          caller that times the phases, empty otherwise
#pragma once
#include <stdint.h>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#define __device__
#endif
#endif

#define DQH_INLINE __host__ __device__ inline __attribute__((always_inline))

namespace dqh {

enum : int32_t {
  HDR_NONE = 0,  // not a dynamic block (or no room for a block header): the caller's own path
  HDR_DYN = 1,   // a dynamic header, decoded: nlen, ndist, bfinal, end and the lengths are valid
  HDR_ERR = 2,   // a dynamic header the decoder rejects: status says why
};
// the decoder's two error codes (dq_internal.h: ST_BAD_TABLE, ST_OVERREAD)
constexpr int32_t HDR_BAD_TABLE = 4, HDR_OVERREAD = 8;
// words a header can span from the word of its first bit: 17 + 19 * 3 + 316 * 14 bits, a start bit
// of up to 31 and the bit reader's look-ahead of two words
constexpr uint32_t HDR_WORDS = 160;
constexpr int HDR_LENS = 320;  // length slots: 288 litlen + 32 distance

struct HdrInfo {
  int32_t kind, status;
  int32_t nlen, ndist, bfinal;
  uint32_t end;  // bit position after the header (HDR_DYN)
};

// LSB-first reader: at least 32 valid bits after fill()
template <class Src>
struct Bits {
  uint64_t bb;
  uint32_t bc, wp;
  DQH_INLINE void init(Src& S, uint32_t pos) {
    const uint32_t wi = pos >> 5, sh = pos & 31;
    const uint32_t w0 = S.word(wi);
    bb = (((uint64_t)S.word(wi + 1) << 32) | w0) >> sh;
    bc = 64 - sh;
    wp = wi + 2;
  }
  DQH_INLINE void fill(Src& S) {
    if (bc <= 32) {
      bb |= (uint64_t)S.word(wp) << bc;
      bc += 32;
      wp += 1;
    }
  }
  DQH_INLINE uint32_t peek() const { return (uint32_t)bb; }
  DQH_INLINE void skip(uint32_t n) {
    bb >>= n;
    bc -= n;
  }
  DQH_INLINE uint32_t pos() const { return wp * 32 - bc; }
};

// Decode the block header at bit `pos` of a member whose deflate data ends at bit `endbits`.
// Every loop is bounded by construction (19 lengths, 128 table entries, 316 symbols of at most 6
// stored lengths each), and the reader advances at most 17 + 57 + 316 * 14 bits: corrupt input can
// neither spin the caller nor move it past HDR_WORDS words.
template <class Src, class Tbl, class Sink>
DQH_INLINE HdrInfo hdr_decode(Src& S, Tbl& T, Sink& K, uint32_t pos, uint32_t endbits) {
  // the order the code-length code's lengths come in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12,
  // 3, 13, 2, 14, 1, 15), five bits each: twelve in ord_lo, seven in ord_hi (an array of bytes is a
  // load from constant memory per length on the device)
  constexpr uint64_t ord_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 |
                              9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
  constexpr uint64_t ord_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
  HdrInfo R = {HDR_NONE, 0, 0, 0, 0, pos};
  if (pos + 3 > endbits) return R;  // the caller reports it (with the block types it handles)
  Bits<Src> B;
  B.init(S, pos);
  const uint32_t h = B.peek();
  R.bfinal = (int32_t)(h & 1);
  if (((h >> 1) & 3) != 2) return R;
  R.nlen = (int32_t)((h >> 3) & 31) + 257;
  R.ndist = (int32_t)((h >> 8) & 31) + 1;
  const int ncode = (int)((h >> 13) & 15) + 4;
  B.skip(17);
  R.kind = HDR_ERR;
  R.status = HDR_BAD_TABLE;
  if (R.nlen > 286 || R.ndist > 30) return R;
  if (pos + 17 + 3 * (uint32_t)ncode > endbits) {  // the code-length code itself is cut off: what
    R.status = HDR_OVERREAD;                       // follows the member is not judged as a code
    return R;
  }
  // the code-length code's lengths: sym s in bits [3 s, 3 s + 3) of cl; the number of codes of
  // length l in bits [8 l, 8 l + 8) of cnt
  uint64_t cl = 0, cnt = 0;
  for (int i = 0; i < 19; i++) {
    B.fill(S);
    const uint32_t v = i < ncode ? B.peek() & 7 : 0;
    B.skip(i < ncode ? 3 : 0);
    const uint32_t sym = (uint32_t)(i < 12 ? ord_lo >> (5 * i) : ord_hi >> (5 * (i - 12))) & 31;
    cl |= (uint64_t)v << (3 * sym);
    cnt += 1ull << (8 * v);
  }
  // complete and not over-subscribed (as the kernels' clt_entry); the first code of each length
  // in bits [8 l, 8 l + 8) of nxt
  uint64_t nxt = 0;
  {
    int left = 1;
    uint32_t code = 0;
    bool ok = true;
    for (int l = 1; l <= 7; l++) {
      const int c = (int)((cnt >> (8 * l)) & 0xff);
      left = 2 * left - c;  // (negative once over-subscribed: no shift)
      ok = ok && left >= 0;
      nxt |= (uint64_t)(code & 0xff) << (8 * l);
      code = (code + (uint32_t)c) << 1;
    }
    if (!ok || left != 0) return R;
  }
  K.mark(0);
  // the 7-bit decode table: every entry is written exactly once (the code is complete)
  for (int s = 0; s < 19; s++) {
    const uint32_t l = (uint32_t)(cl >> (3 * s)) & 7;
    if (l == 0) continue;
    const uint32_t c = (uint32_t)(nxt >> (8 * l)) & 0xff;
    nxt += 1ull << (8 * l);
    uint32_t r = 0;  // the code, bit-reversed (LSB-first stream)
    for (uint32_t i = 0; i < l; i++) r |= ((c >> i) & 1u) << (l - 1 - i);
    for (uint32_t k = r & 127; k < 128; k += 1u << l) T.set(k, (uint32_t)s << 3 | l);
  }
  K.mark(1);
  // the nlen + ndist lengths; runs (16/17/18) cross from the litlen into the distance alphabet
  const int total = R.nlen + R.ndist;
  int have = 0, prev = -1;
  bool eob = false;
  for (int it = 0; it < 316 && have < total; it++) {
    if (B.pos() > endbits) {
      R.status = HDR_OVERREAD;
      return R;
    }
    S.ahead(B.wp);
    B.fill(S);
    const uint32_t v = B.peek();
    const uint32_t e = T.get(v & 127);
    const uint32_t len = e & 7, sy = e >> 3;
    if (len == 0) return R;  // (unreachable with a complete code; kept as the bound's guard)
    const uint32_t ex = sy < 16 ? 0u : sy == 16 ? 2u : sy == 17 ? 3u : 7u;
    const int xv = (int)((v >> len) & ((1u << ex) - 1));
    B.skip(len + ex);
    const int rep = sy < 16 ? 1 : sy == 18 ? 11 + xv : 3 + xv;
    const int val = sy < 16 ? (int)sy : sy == 16 ? prev : 0;
    if (val < 0) return R;              // a repeat with no length before it
    if (have + rep > total) return R;   // a run past HLIT + HDIST
    if (val != 0) {  // rep <= 6 here: the run's litlen part, or all of it; the rest of a run that
                     // crosses into the distance alphabet
      const int nl = have >= R.nlen ? 0 : have + rep <= R.nlen ? rep : R.nlen - have;
      K.run((uint32_t)(nl ? have : 288 + have - R.nlen), (uint32_t)(nl ? nl : rep), (uint32_t)val);
      if (nl != 0 && nl != rep) K.run(288u, (uint32_t)(rep - nl), (uint32_t)val);
      eob = eob || (have <= 256 && have + rep > 256);
    }
    have += rep;
    prev = val;
  }
  K.mark(2);
  if (have < total) return R;
  R.end = B.pos();
  if (R.end > endbits) {
    R.status = HDR_OVERREAD;
    return R;
  }
  if (!eob) return R;  // an end-of-block code is required
  R.kind = HDR_DYN;
  R.status = 0;
  return R;
}

}  // namespace dqh
