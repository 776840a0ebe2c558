// chain_check.cpp -- the chain core (disq_amd/csrc/dq_chain_core.h) on the host, for
// tests/test_chain_core_cpu.py: the windowed walk with its link rule and repair as the kernels run
// it (chain_walk / chain_link / chain_fix / chain_emit in dq_kernels.hip), and the planners' guess
// loop over a candidate list that covers byte ranges only.
//
//   chain_check chain FILE W START      window size W (any W >= 1 here: small windows make every
//                                       link case cheap to build), chain start START
//       -> "nblk broken", then one line "pos csize usize" per block
//   chain_check guess FILE P END [R0 R1]...   guessNextBGZFPos(P, END) over the candidates of the
//                                       byte ranges [R0, R1) (none given: the whole file)
//       -> "pos csize usize", "null" or "unknown" (the ranges cannot tell)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dq_chain_core.h"

using namespace dqc;

namespace {

struct Table {
  std::vector<int64_t> pos;
  std::vector<int32_t> cs, us;
  void block(int64_t, int64_t p, int32_t c, int32_t u) {
    pos.push_back(p);
    cs.push_back(c);
    us.push_back(u);
  }
};

int run_chain(const uint8_t* C, int64_t L, int64_t W, int64_t cs0) {
  if (cs0 > L) cs0 = L;
  const int64_t nwin = L > cs0 ? (L - cs0 + W - 1) / W : 1;
  std::vector<ChainWin> wins((size_t)nwin);
  // count pass: speculate and walk every window on its own
  for (int64_t w = 0; w < nwin; w++) {
    const int64_t ws = cs0 + w * W;
    if (ws >= L) {
      wins[(size_t)w] = ChainWin{-1, L, 0, 0, 0, 0};
      continue;
    }
    const int64_t we = ws + W < L ? ws + W : L;
    int64_t start = -1;
    if (w == 0) {
      start = cs0;
    } else {
      for (int64_t q = ws; q < we && start < 0; q++)
        if (q + 4 <= L && (uint32_t)ld32(C, q) == BGZF_MAGIC && spec_at(C, q, L)) start = q;
    }
    if (start < 0) {
      wins[(size_t)w] = ChainWin{-1, ws, 0, 0, 0, 0};
      continue;
    }
    NoSink sink;
    walk_window(C, L, start, we, &wins[(size_t)w], sink);
  }
  // link check
  int broken = 0;
  for (int64_t w = 1; w < nwin; w++) {
    const int64_t ws = cs0 + w * W;
    if (ws >= L) continue;
    int64_t t = w - 1;
    while (t > 0 && wins[(size_t)t].start < 0) t--;
    if (!link_ok(wins[(size_t)t].exit, wins[(size_t)t].stop, wins[(size_t)w], ws + W < L ? ws + W : L))
      broken = 1;
  }
  // repair
  if (broken) {
    int64_t in = wins[0].exit;
    int32_t in_stop = wins[0].stop;
    for (int64_t w = 1; w < nwin; w++) {
      const int64_t ws = cs0 + w * W;
      if (ws >= L) break;
      const int64_t we = ws + W < L ? ws + W : L;
      ChainWin& g = wins[(size_t)w];
      if (in_stop || in >= we) {
        g = ChainWin{-1, in, 0, 0, 0, 0};
        continue;
      }
      if (g.start != in) {
        NoSink sink;
        walk_window(C, L, in, we, &g, sink);
      }
      in = g.exit;
      in_stop = g.stop;
    }
  }
  // emit: every window again from its exact start, count blocks
  Table T;
  for (int64_t w = 0; w < nwin; w++) {
    const ChainWin& g = wins[(size_t)w];
    if (g.start < 0 || g.count == 0) continue;
    const int64_t ws = cs0 + w * W;
    ChainWin again;
    const size_t before = T.pos.size();
    walk_window(C, L, g.start, ws + W < L ? ws + W : L, &again, T);
    if ((int64_t)(T.pos.size() - before) != g.count || again.exit != g.exit || again.usum != g.usum) {
      fprintf(stderr, "window %lld: the emit walk differs from the count walk\n", (long long)w);
      return 2;
    }
  }
  printf("%zu %d\n", T.pos.size(), broken);
  for (size_t i = 0; i < T.pos.size(); i++) printf("%lld %d %d\n", (long long)T.pos[i], T.cs[i], T.us[i]);
  return 0;
}

int run_guess(const uint8_t* C, int64_t L, int64_t p, int64_t e, const std::vector<int64_t>& rng) {
  std::vector<Cand> cand;
  auto scan = [&](int64_t a, int64_t b) {
    for (int64_t q = a; q < b && q + 4 <= L; q++) {
      if ((uint32_t)ld32(C, q) != BGZF_MAGIC) continue;
      Cand c{q, 0, 0, 0, 0};
      const int r = guesser_at(C, q, L, &c.csize, &c.usize);
      c.valid = r == 1 ? 1 : (r == 2 ? 2 : 0);
      cand.push_back(c);
    }
  };
  if (rng.empty()) scan(0, L);
  for (size_t r = 0; r < rng.size(); r += 2) scan(rng[r], rng[r + 1]);
  const CandView V{cand.data(), (int64_t)cand.size(), rng.empty() ? nullptr : rng.data(),
                   (int64_t)rng.size() / 2, L};
  for (;;) {  // the planners' loop (plan_blocks_kernel, text_plan_kernel)
    const int64_t k = cand_next(V, p, e);
    if (k == CAND_UNKNOWN) return puts("unknown"), 0;
    if (k >= V.n) break;
    const Cand c = cand[(size_t)k];
    if (c.pos != p && c.pos >= e) break;
    if (c.valid == 1) return printf("%lld %d %d\n", (long long)c.pos, c.csize, c.usize), 0;
    if (c.valid == 2) break;
    p = c.pos + 4;
  }
  return puts("null"), 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 5) return fprintf(stderr, "usage: chain_check chain FILE W START | guess FILE P END [R0 R1]...\n"), 1;
  FILE* f = fopen(argv[2], "rb");
  if (!f) return perror(argv[2]), 1;
  std::vector<uint8_t> buf;
  uint8_t tmp[65536];
  for (size_t n; (n = fread(tmp, 1, sizeof tmp, f)) > 0;) buf.insert(buf.end(), tmp, tmp + n);
  fclose(f);
  const int64_t L = (int64_t)buf.size();
  uint8_t* C = (uint8_t*)malloc(L ? (size_t)L : 1);  // exactly L bytes: the sanitizer sees a read past them
  if (L) memcpy(C, buf.data(), (size_t)L);
  int rc;
  if (!strcmp(argv[1], "chain")) {
    rc = run_chain(C, L, atoll(argv[3]), atoll(argv[4]));
    free(C);
    return rc;
  }
  std::vector<int64_t> rng;
  for (int i = 5; i + 1 < argc; i += 2) {
    rng.push_back(atoll(argv[i]));
    rng.push_back(atoll(argv[i + 1]));
  }
  rc = run_guess(C, L, atoll(argv[3]), atoll(argv[4]), rng);
  free(C);
  return rc;
}
