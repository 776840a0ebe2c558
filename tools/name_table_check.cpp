// name_table_check -- the name table of disq_amd/csrc/dq_text_core.h (name_table_build,
// name_lookup) on the CPU, for tests/test_name_table_cpu.py:
//   name_table_check lookup NAMES QUERIES   the index of every query in the table of NAMES, a line each
//   name_table_check forged A B             the table of A and B with both hash entries set to B's hash:
//                                           the indices of B and of A (the collision scan's byte compare)
// NAMES / QUERIES: a count line, then that many lines, a name each (it may be empty).
#include <stdio.h>

#include <fstream>

#include "dq_text_core.h"

static bool read_list(const char* path, std::vector<std::string>* out) {
  std::ifstream f(path, std::ios::binary);
  std::string line;
  if (!std::getline(f, line)) return false;
  const size_t n = (size_t)std::stoul(line);
  for (size_t i = 0; i < n; i++) {
    if (!std::getline(f, line)) return false;
    out->push_back(line);
  }
  return true;
}

static int32_t lookup(const dqt::NameTable& T, const std::string& q) {
  return dqt::name_lookup(T, (const uint8_t*)q.data(), (int32_t)q.size());
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "lookup" && argc == 4) {
    std::vector<std::string> names, queries;
    if (!read_list(argv[2], &names) || !read_list(argv[3], &queries)) return 2;
    dqt::NameTableHost H;
    dqt::name_table_build(names, &H);
    const dqt::NameTable T = H.view();
    for (const std::string& q : queries) printf("%d\n", lookup(T, q));
    return 0;
  }
  if (mode == "forged" && argc == 4) {
    const std::string a = argv[2], b = argv[3];
    dqt::NameTableHost H;
    dqt::name_table_build({a, b}, &H);
    // equal hashes sort by index: entry 0 is A's, entry 1 is B's, both under B's hash
    H.hash[0] = H.hash[1] = dqt::name_hash((const uint8_t*)b.data(), (int32_t)b.size());
    H.idx[0] = 0;
    H.idx[1] = 1;
    const dqt::NameTable T = H.view();
    printf("%d\n%d\n", lookup(T, b), lookup(T, a));
    return 0;
  }
  fprintf(stderr, "usage: name_table_check lookup NAMES QUERIES | forged A B\n");
  return 2;
}
