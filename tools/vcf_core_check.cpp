// vcf_core_check.cpp -- the per-line VCF rules of disq_amd/csrc/dq_vcf_core.h run on the host, for
// tests/test_vcf_core_cpu.py (and, built with -fsanitize=address,undefined, over the same inputs)
// and as the CPU baseline of tools/vcf_decode_bench.py.  It compiles the very functions the VCF
// kernels call.
//
//   vcf_core_check lines IN.vcf OUT.txt
//       "H <G> <n contigs>" from the leading '#' lines ("H nochrom" and exit status 3 when data
//       lines follow a header without a #CHROM line), then per line that does not start with '#',
//       in file order, "<line index> E <class>" or "<line index> S contig pos end flags qual-bits
//       host col_end*8 n_alt n_filter n_info n_sample_cols" (qual-bits: 16 hex digits; host: the
//       QUAL text was left to strtod, as the library's host does).  Every line is copied into a
//       buffer of its own, so a read past it is a heap overflow, and is also walked the way a wave
//       walks a long one (the TABs handed in); both walks must agree.
//   vcf_core_check quals IN.txt OUT.txt
//       per line of IN (a QUAL text): "OK <bits as 16 hex digits>", "UNDECIDED" or "BAD".
//   vcf_core_check bench IN.vcf THREADS REPS [OUT.bin]
//       the data lines cut into THREADS runs of whole lines, one thread each, decoded REPS times;
//       prints one JSON line (the best wall time); OUT.bin takes the columns, 72 bytes per line:
//       contig pos end flags (4 x i32), qual (f64), col_end (8 x i32), n_alt n_filter n_info
//       n_sample_cols (4 x i32).
//
//   g++ -O2 -g -std=c++17 -pthread -I disq_amd/csrc -o vcf_core_check tools/vcf_core_check.cpp
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "dq_vcf_core.h"

using namespace dqv;

static bool slurp(const char* path, std::vector<uint8_t>& out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  static uint8_t buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
  fclose(f);
  return true;
}

// LF, CR LF and a lone CR end a line; a last line without a terminator counts; a BOM is dropped.
static void text_lines(const std::vector<uint8_t>& t, std::vector<std::pair<int64_t, int64_t>>& out) {
  const int64_t n = (int64_t)t.size();
  int64_t a = (n >= 3 && t[0] == 0xEF && t[1] == 0xBB && t[2] == 0xBF) ? 3 : 0, i = a;
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

static void wave_tabs(const uint8_t* L, int32_t len, VcfTabs* tb) {
  tb->n = 0;
  tb->total = 0;
  for (int32_t x = 0; x < len; x++)
    if (L[x] == '\t') {
      if (tb->n < 8) tb->at[tb->n++] = x;
      tb->total++;
    }
}

static bool same_site(const VcfSite& a, const VcfSite& b) {
  return a.contig == b.contig && a.pos == b.pos && a.end == b.end && a.flags == b.flags &&
         memcmp(&a.qual, &b.qual, 8) == 0 && memcmp(a.col_end, b.col_end, 32) == 0 &&
         a.n_alt == b.n_alt && a.n_filter == b.n_filter && a.n_info == b.n_info &&
         a.n_sample_cols == b.n_sample_cols && a.qual_undecided == b.qual_undecided;
}

static double host_qual(const uint8_t* L, const VcfSite& S) {
  const std::string s((const char*)L + S.col_end[4] + 1, (size_t)(S.col_end[5] - S.col_end[4] - 1));
  return strtod(s.c_str(), nullptr);
}

static int lines(const char* in, const char* outp) {
  std::vector<uint8_t> t;
  if (!slurp(in, t)) return 2;
  FILE* o = fopen(outp, "w");
  if (!o) return 2;
  VcfHeader H;
  vcf_header_parse(t.data(), (int64_t)t.size(), true, &H);
  if (H.has_data && !H.has_chrom) {
    fprintf(o, "H nochrom\n");
    fclose(o);
    return 3;
  }
  fprintf(o, "H %d %zu\n", H.G ? 1 : 0, H.contigs.size());
  dqt::NameTableHost CT;
  dqt::name_table_build(H.contigs, &CT);
  const dqt::NameTable C = CT.view();
  std::vector<std::pair<int64_t, int64_t>> ls;
  text_lines(t, ls);
  for (size_t k = 0; k < ls.size(); k++) {
    const int64_t a = ls[k].first, z = ls[k].second;
    if (z > a && t[(size_t)a] == '#') continue;
    std::vector<uint8_t> line(t.begin() + a, t.begin() + z);
    const int32_t len = (int32_t)line.size();
    VcfSite S{}, V{}, W{};
    const int32_t st = vcf_line_walk(line.data(), len, H.G, C, nullptr, true, &S);
    const int32_t sv = vcf_line_walk(line.data(), len, H.G, C, nullptr, false, &V);  // the validate pass
    VcfTabs tb;
    wave_tabs(line.data(), len, &tb);
    const int32_t sw = vcf_line_walk(line.data(), len, H.G, C, &tb, true, &W);
    if (sv != st || sw != st || (st == VCF_OK && !same_site(S, W))) {
      fprintf(stderr, "line %zu: the walks disagree (%d, %d, %d)\n", k, st, sv, sw);
      return 4;
    }
    if (st != VCF_OK) {
      fprintf(o, "%zu E %s\n", k, vcf_status_name(st));
      continue;
    }
    if (S.qual_undecided) S.qual = host_qual(line.data(), S);
    uint64_t bits;
    memcpy(&bits, &S.qual, 8);
    fprintf(o, "%zu S %d %d %d %u %016llx %d", k, S.contig, S.pos, S.end, S.flags, (unsigned long long)bits,
            S.qual_undecided);
    for (int c = 0; c < 8; c++) fprintf(o, " %d", S.col_end[c]);
    fprintf(o, " %d %d %d %d\n", S.n_alt, S.n_filter, S.n_info, S.n_sample_cols);
  }
  fclose(o);
  return 0;
}

static int quals(const char* in, const char* outp) {
  std::vector<uint8_t> t;
  if (!slurp(in, t)) return 2;
  FILE* o = fopen(outp, "w");
  if (!o) return 2;
  size_t a = 0;
  for (size_t i = 0; i <= t.size(); i++) {
    if (i < t.size() && t[i] != '\n') continue;
    if (i == t.size() && a == i) break;
    std::vector<uint8_t> s(t.begin() + a, t.begin() + i);
    double v = 0;
    const int r = vcf_parse_qual(s.data(), (int32_t)s.size(), &v);
    uint64_t bits;
    memcpy(&bits, &v, 8);
    if (r == VCF_Q_OK) fprintf(o, "OK %016llx\n", (unsigned long long)bits);
    else fprintf(o, r == VCF_Q_UNDECIDED ? "UNDECIDED\n" : "BAD\n");
    a = i + 1;
  }
  fclose(o);
  return 0;
}

struct Row {  // OUT.bin's layout
  int32_t contig, pos, end;
  uint32_t flags;
  double qual;
  int32_t col_end[8];
  int32_t n_alt, n_filter, n_info, n_sample_cols;
};
static_assert(sizeof(Row) == 72, "72 bytes per line");

static int bench(const char* in, int threads, int reps, const char* outp) {
  std::vector<uint8_t> t;
  if (!slurp(in, t)) return 2;
  VcfHeader H;
  vcf_header_parse(t.data(), (int64_t)t.size(), true, &H);
  if (H.has_data && !H.has_chrom) return 3;
  dqt::NameTableHost CT;
  dqt::name_table_build(H.contigs, &CT);
  const dqt::NameTable C = CT.view();
  std::vector<std::pair<int64_t, int64_t>> all, ls;
  text_lines(t, all);
  for (const auto& l : all)
    if (!(l.second > l.first && t[(size_t)l.first] == '#')) ls.push_back(l);
  const size_t n = ls.size();
  std::vector<Row> rows(n);
  std::vector<int> bad((size_t)threads, 0);
  double best = 1e300;
  for (int r = 0; r < reps; r++) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> th;
    for (int w = 0; w < threads; w++)
      th.emplace_back([&, w] {
        const size_t lo = n * (size_t)w / (size_t)threads, hi = n * (size_t)(w + 1) / (size_t)threads;
        for (size_t k = lo; k < hi; k++) {
          const uint8_t* L = t.data() + ls[k].first;
          const int32_t len = (int32_t)(ls[k].second - ls[k].first);
          VcfSite S{};
          if (vcf_line_walk(L, len, H.G, C, nullptr, true, &S) != VCF_OK) {
            bad[(size_t)w]++;
            continue;
          }
          if (S.qual_undecided) S.qual = host_qual(L, S);
          Row& R = rows[k];
          R.contig = S.contig;
          R.pos = S.pos;
          R.end = S.end;
          R.flags = S.flags;
          R.qual = S.qual;
          memcpy(R.col_end, S.col_end, 32);
          R.n_alt = S.n_alt;
          R.n_filter = S.n_filter;
          R.n_info = S.n_info;
          R.n_sample_cols = S.n_sample_cols;
        }
      });
    for (auto& x : th) x.join();
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (ms < best) best = ms;
  }
  int nbad = 0;
  for (int b : bad) nbad += b;
  if (outp) {
    FILE* o = fopen(outp, "wb");
    if (!o) return 2;
    fwrite(rows.data(), sizeof(Row), n, o);
    fclose(o);
  }
  printf("{\"lines\": %zu, \"bytes\": %zu, \"threads\": %d, \"reps\": %d, \"ms_best\": %.3f, \"bad_lines\": %d}\n",
         n, t.size(), threads, reps, best, nbad / (reps > 0 ? reps : 1));
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "lines")) return lines(argv[2], argv[3]);
  if (argc == 4 && !strcmp(argv[1], "quals")) return quals(argv[2], argv[3]);
  if ((argc == 5 || argc == 6) && !strcmp(argv[1], "bench"))
    return bench(argv[2], atoi(argv[3]) > 0 ? atoi(argv[3]) : 1, atoi(argv[4]) > 0 ? atoi(argv[4]) : 1,
                 argc == 6 ? argv[5] : nullptr);
  fprintf(stderr,
          "usage: vcf_core_check lines IN.vcf OUT.txt | quals IN.txt OUT.txt | bench IN.vcf THREADS REPS [OUT.bin]\n");
  return 1;
}
