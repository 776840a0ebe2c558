// hdr_core_check -- the serial DEFLATE block-header decoder of disq_amd/csrc/dq_hdr_core.h
// (hdr_decode, what one lane of inflate_header_kernel runs) on the CPU, for
// tests/test_hdr_core_cpu.py:
//   hdr_core_check CASES [counts]
//                            one line per case: kind status nlen ndist bfinal end, then the 320 code
//                            lengths as hex digits (litlen at [0, 288), distance at [288, 320));
//                            with `counts` (tests/test_hdr_counts_cpu.py) then the numbers of litlen
//                            codes of the lengths 1..15 and of distance codes of the lengths 1..15,
//                            as the sink summed them up
// CASES (binary, little endian): per case three u32 -- the byte count n, the header's bit position
// and the bit position of the end of the member's deflate data -- and the n bytes.  As the kernels'
// compressed buffer, the bytes are followed by a zero pad (4096 bytes, allocated exactly: a read
// past it is a sanitizer error), and the reader clamps its word index to HDR_WORDS words from the
// header's first word.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "dq_hdr_core.h"

namespace {

constexpr size_t PAD = 4096;

// The reads are also held against what hdr_decode promises a source that reads ahead: increasing
// word indices from the header's first word, each asked for once, at most six before the first
// ahead() and one between two, and ahead(i) names the next word.  So every word lies in a window
// of WIN words that moves to i at ahead(i) once i is its last word (the pre-pass kernel's HpSrc,
// whose window is no smaller and moves no later).
constexpr uint32_t WIN = 8;
struct Src {
  const uint8_t* p;
  uint32_t base;
  int64_t prev = -1;
  int64_t win = -1;  // first word of the window
  int since = 0;     // words asked for since the last ahead()
  bool aheads = false, kept = true;
  uint32_t word(uint32_t i) {
    if (win < 0) win = i;
    kept = kept && (prev < 0 ? i == base : (int64_t)i == prev + 1) && ++since <= (aheads ? 1 : 6) &&
           i >= win && i < win + WIN;
    prev = i;
    uint32_t v;
    memcpy(&v, p + 4 * (size_t)std::min(i, base + dqh::HDR_WORDS - 1), 4);
    return v;
  }
  void ahead(uint32_t i) {
    kept = kept && (int64_t)i == prev + 1;
    if (i - win >= WIN - 1) win = i;
    aheads = true;
    since = 0;
  }
};
struct Tbl {
  uint8_t t[128];
  int writes = 0;
  void set(uint32_t k, uint32_t v) {
    t[k] = (uint8_t)v;
    writes++;
  }
  uint32_t get(uint32_t k) const { return t[k]; }
};
struct Sink {
  uint8_t lens[dqh::HDR_LENS];
  int cnt[2][16] = {};
  int64_t last = -1;
  bool ordered = true;
  void run(uint32_t i, uint32_t n, uint32_t v) {
    // the device sink relies on increasing slots, runs of 1..6 inside one alphabet and lengths 1..15
    ordered = ordered && (int64_t)i > last && n >= 1 && n <= 6 && v >= 1 && v <= 15 &&
              (i + n <= 288 || (i >= 288 && i + n <= (uint32_t)dqh::HDR_LENS));
    if (!ordered) return;
    last = i + n - 1;
    for (uint32_t k = i; k < i + n; k++) lens[k] = (uint8_t)v;
    cnt[i >= 288][v] += (int)n;
  }
  void mark(int) {}
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2 && !(argc == 3 && !strcmp(argv[2], "counts"))) {
    fprintf(stderr, "usage: hdr_core_check CASES [counts]\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t hd[3];
  while (fread(hd, 4, 3, f) == 3) {
    const uint32_t n = hd[0], pos = hd[1], endbits = hd[2];
    // a heap block of exactly the bytes and the pad
    std::vector<uint8_t> buf((size_t)n + PAD, 0);
    if (n && fread(buf.data(), 1, n, f) != n) return 2;
    if ((uint64_t)(pos >> 5) * 4 + dqh::HDR_WORDS * 4 > buf.size()) return 3;  // the case's own bound
    Src S{buf.data(), pos >> 5};
    Tbl T;
    memset(T.t, 0, sizeof T.t);
    Sink K;
    memset(K.lens, 0, sizeof K.lens);
    const dqh::HdrInfo R = dqh::hdr_decode(S, T, K, pos, endbits);
    if (!K.ordered || T.writes > 128 || !S.kept) return 4;
    printf("%d %d %d %d %d %u ", R.kind, R.status, R.nlen, R.ndist, R.bfinal, R.end);
    for (int i = 0; i < dqh::HDR_LENS; i++) putchar("0123456789abcdef"[K.lens[i] & 15]);
    if (argc == 3)
      for (int a = 0; a < 2; a++)
        for (int l = 1; l <= 15; l++) printf(" %d", K.cnt[a][l]);
    putchar('\n');
  }
  fclose(f);
  return 0;
}
