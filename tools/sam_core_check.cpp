// sam_core_check.cpp -- the per-line SAM rules of disq_amd/csrc/dq_sam_core.h run on the host, for
// tests/test_sam_core_cpu.py (and, built by hand with -fsanitize=address,undefined, over the same
// inputs).  It compiles the very functions the SAM kernels call.
//
//   sam_core_check records IN.sam OUT.bin
//       the BAM header built from the leading '@' lines (u32 length, bytes), then per line that
//       does not start with '@', in file order: u32 line index, u32 kind (0 record, 1 error),
//       u32 length, and the record's bytes or the error class ("fields", "QNAME", ..., "tag XX").
//       Every record is sized first and encoded into a buffer of exactly that size followed by
//       guard bytes; undecided floats are patched with strtof as the library's host does.  Every
//       line is also walked the way a wave walks a long one (TAB positions handed in, SEQ and QUAL
//       left out) and must come to the same status, size and offsets.
//   sam_core_check floats IN.txt OUT.txt
//       per line of IN (a float text): "OK <bits as 8 hex digits>", "UNDECIDED" or "BAD".
//
//   g++ -O1 -g -std=c++17 -I disq_amd/csrc -o sam_core_check tools/sam_core_check.cpp
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dq_sam_core.h"

using namespace dqs;

static bool slurp(const char* path, std::vector<uint8_t>& out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  uint8_t buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
  fclose(f);
  return true;
}

static void put32(FILE* f, uint32_t v) {
  const uint8_t b[4] = {(uint8_t)v, (uint8_t)(v >> 8), (uint8_t)(v >> 16), (uint8_t)(v >> 24)};
  fwrite(b, 1, 4, f);
}

// LF, CR LF and a lone CR end a line; a last line without a terminator counts.
static void text_lines(const std::vector<uint8_t>& t, std::vector<std::pair<int64_t, int64_t>>& out) {
  const int64_t n = (int64_t)t.size();
  int64_t a = 0, i = 0;
  while (i < n) {
    if (t[i] == '\n') {
      out.push_back({a, i});
      a = ++i;
    } else if (t[i] == '\r') {
      out.push_back({a, i});
      i += (i + 1 < n && t[i + 1] == '\n') ? 2 : 1;
      a = i;
    } else {
      i++;
    }
  }
  if (a < n) out.push_back({a, n});
}

static int records(const char* in, const char* outp) {
  std::vector<uint8_t> t;
  if (!slurp(in, t)) return 2;
  FILE* o = fopen(outp, "wb");
  if (!o) return 2;
  SamHeader H;
  if (sam_header_build(t.data(), (int64_t)t.size(), true, &H) != 0) {
    fprintf(stderr, "bad @SQ line\n");
    return 3;
  }
  put32(o, (uint32_t)H.bam.size());
  fwrite(H.bam.data(), 1, H.bam.size(), o);
  dqt::NameTableHost RT;
  dqt::name_table_build(H.names, &RT);
  const dqt::NameTable R = RT.view();
  std::vector<std::pair<int64_t, int64_t>> lines;
  text_lines(t, lines);
  constexpr int GUARD = 64;
  for (size_t k = 0; k < lines.size(); k++) {
    const int64_t a = lines[k].first, z = lines[k].second;
    if (z > a && t[(size_t)a] == '@') continue;
    // the line in a buffer of its own, so that a read past it is a heap overflow
    std::vector<uint8_t> line(t.begin() + a, t.begin() + z);
    SamLineInfo I;
    const int32_t st = sam_line_size(line.data(), (int32_t)line.size(), R, &I);
    {  // the walk a wave makes of a long line: the TABs handed in, SEQ and QUAL left to the caller
      SamTabs tb{};
      for (int32_t x = 0; x < (int32_t)line.size() && tb.n < 11; x++)
        if (line[(size_t)x] == '\t') tb.at[tb.n++] = x;
      SamLineInfo W;
      const int32_t sw = sam_line_walk(line.data(), (int32_t)line.size(), R, nullptr, 0, &W, nullptr, false, &tb);
      const bool same = st == SAM_OK ? (sw == SAM_OK && W.size == I.size && W.seq_off == I.seq_off &&
                                        W.qual_off == I.qual_off && W.seq_out == I.seq_out)
                                     : (sw == st || st == SAM_E_SEQ || st == SAM_E_QUAL);
      if (!same) {
        fprintf(stderr, "line %zu: the walk with the TABs handed in disagrees (%d vs %d)\n", k, sw, st);
        return 4;
      }
    }
    put32(o, (uint32_t)k);
    if (st != SAM_OK) {
      char buf[8];
      const char* w = sam_status_name(st, buf);
      put32(o, 1);
      put32(o, (uint32_t)strlen(w));
      fwrite(w, 1, strlen(w), o);
      continue;
    }
    std::vector<uint8_t> rec((size_t)I.size + GUARD, 0xA5);
    std::vector<int64_t> ent(3 * (size_t)std::max(1, I.n_undecided));
    unsigned long long cnt = 0;
    const SamFixSink fx{ent.data(), &cnt, I.n_undecided, 0, 0};
    SamLineInfo J;
    const int32_t st2 = sam_line_encode(line.data(), (int32_t)line.size(), R, rec.data(), I.size, &J, &fx);
    bool ok = st2 == SAM_OK && J.size == I.size && (long long)cnt == I.n_undecided;
    for (int g = 0; g < GUARD; g++) ok = ok && rec[(size_t)I.size + g] == 0xA5;
    if (!ok) {
      fprintf(stderr, "line %zu: the encode pass disagrees with the size pass\n", k);
      return 4;
    }
    for (unsigned long long e = 0; e < cnt; e++) {  // the host fix-up of undecided floats
      const std::string s((const char*)line.data() + ent[3 * e + 1], (size_t)ent[3 * e + 2]);
      const float f = strtof(s.c_str(), nullptr);
      memcpy(rec.data() + ent[3 * e], &f, 4);
    }
    put32(o, 0);
    put32(o, (uint32_t)I.size);
    fwrite(rec.data(), 1, (size_t)I.size, o);
  }
  fclose(o);
  return 0;
}

static int floats(const char* in, const char* outp) {
  std::vector<uint8_t> t;
  if (!slurp(in, t)) return 2;
  FILE* o = fopen(outp, "w");
  if (!o) return 2;
  size_t a = 0;
  for (size_t i = 0; i <= t.size(); i++) {
    if (i < t.size() && t[i] != '\n') continue;
    if (i == t.size() && a == i) break;
    std::vector<uint8_t> s(t.begin() + a, t.begin() + i);
    uint32_t bits = 0;
    const int r = sam_parse_float(s.data(), (int32_t)s.size(), &bits);
    if (r == SAM_F_OK) fprintf(o, "OK %08x\n", bits);
    else fprintf(o, r == SAM_F_UNDECIDED ? "UNDECIDED\n" : "BAD\n");
    a = i + 1;
  }
  fclose(o);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "records")) return records(argv[2], argv[3]);
  if (argc == 4 && !strcmp(argv[1], "floats")) return floats(argv[2], argv[3]);
  fprintf(stderr, "usage: sam_core_check records IN.sam OUT.bin | floats IN.txt OUT.txt\n");
  return 1;
}
