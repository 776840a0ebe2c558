// block_range_check.cpp -- dqc::last_block_le (disq_amd/csrc/dq_chain_core.h), the planners' "last
// block of the table at or before the split end", on the host for tests/test_block_range_cpu.py,
// next to the block-by-block loop it replaced in plan_blocks_kernel.
//
//   block_range_check query POSFILE J E [J E]...
//       POSFILE: the block positions, ascending, as little-endian int64
//       -> one line "search linear" per (J, E)
//   block_range_check sweep POSFILE J...
//       for every J given: every E among pos[k] - 1, pos[k], pos[k] + 1 of every block k, one
//       below the first position and far past the last
//       -> "cases mismatches"; exit status 1 on any mismatch (the first ones go to stderr)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "dq_chain_core.h"

namespace {

int64_t linear(const int64_t* pos, int64_t nb, int64_t j, int64_t e) {
  int64_t jl = j;
  while (jl + 1 < nb && pos[jl + 1] <= e) jl++;
  return jl;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) return fprintf(stderr, "usage: block_range_check query POSFILE J E [J E]... | sweep POSFILE J...\n"), 2;
  FILE* f = fopen(argv[2], "rb");
  if (!f) return perror(argv[2]), 2;
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  const int64_t nb = bytes / 8;
  int64_t* pos = (int64_t*)malloc(nb ? (size_t)nb * 8 : 1);  // exactly nb entries: the sanitizer sees a read past them
  if (nb && fread(pos, 8, (size_t)nb, f) != (size_t)nb) return fprintf(stderr, "short read\n"), 2;
  fclose(f);
  int rc = 0;
  if (!strcmp(argv[1], "query")) {
    for (int i = 3; i + 1 < argc; i += 2) {
      const int64_t j = atoll(argv[i]), e = atoll(argv[i + 1]);
      printf("%lld %lld\n", (long long)dqc::last_block_le(pos, nb, j, e), (long long)linear(pos, nb, j, e));
    }
  } else {
    long long cases = 0, bad = 0;
    for (int i = 3; i < argc; i++) {
      const int64_t j = atoll(argv[i]);
      auto one = [&](int64_t e) {
        const int64_t a = dqc::last_block_le(pos, nb, j, e), b = linear(pos, nb, j, e);
        cases++;
        if (a != b && bad++ < 5)
          fprintf(stderr, "j %lld e %lld: search %lld, linear %lld\n", (long long)j, (long long)e, (long long)a, (long long)b);
      };
      for (int64_t k = 0; k < nb; k++)
        for (int64_t d = -1; d <= 1; d++) one(pos[k] + d);
      if (nb) one(pos[0] - 1), one(pos[nb - 1] + (int64_t(1) << 40));
    }
    printf("%lld %lld\n", cases, bad);
    rc = bad ? 1 : 0;
  }
  free(pos);
  return rc;
}
