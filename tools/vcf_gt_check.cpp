// vcf_gt_check.cpp -- the per-cell genotype rules of disq_amd/csrc/dq_vcf_gt_core.h run on the host,
// for tests/test_vcf_gt_core_cpu.py (and, built with -fsanitize=address,undefined, over the same
// inputs) and as the CPU baseline of tools/vcf_gt_bench.py.  It compiles the very functions the
// genotype kernels call.
//
//   vcf_gt_check lines IN.vcf OUT.txt
//       "H <S>" and one "N <name>" per sample from the leading '#' lines, then per line that does
//       not start with '#', in file order: "<k> X" when the site decode (dq_vcf_core.h) rejects it,
//       "<k> E <class> <sample>" (sample -1 for samples and FORMAT), or "<k> G <P>" followed by one
//       " flags,ploidy,gq,host,dp,cell_off,a0/a1/..." per cell (P alleles; host: the GQ text was left
//       to strtod, as the library's host does; P = the line's largest ploidy, at least 1).  Every
//       line is copied into a buffer of its own, so a read past it is a heap overflow.
//   vcf_gt_check bench IN.vcf THREADS REPS [OUT.bin]
//       the data lines cut into THREADS runs of whole lines, one thread each: the site walk for the
//       columns the genotype passes start from (untimed), then the check pass and the decode pass
//       REPS times; prints one JSON line (the best wall time of check + decode); OUT.bin takes
//       n, S, P (3 x i64) and the arrays flags, ploidy (u8), allele (i16, P per cell), gq, dp,
//       cell_off (i32), n * S cells each.
//
//   g++ -O2 -g -std=c++17 -pthread -I disq_amd/csrc -o vcf_gt_check tools/vcf_gt_check.cpp
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "dq_vcf_gt_core.h"

using namespace dqg;

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

struct Header {
  dqv::VcfHeader H;
  dqt::NameTableHost CT;
  std::vector<std::string> names;
  int32_t S = 0;
};

static int read_header(const std::vector<uint8_t>& t, Header* h) {
  dqv::vcf_header_parse(t.data(), (int64_t)t.size(), true, &h->H);
  if (h->H.has_data && !h->H.has_chrom) return 3;
  dqt::name_table_build(h->H.contigs, &h->CT);
  if (h->H.G) gt_header_samples(t.data(), (int64_t)t.size(), &h->names);
  h->S = (int32_t)h->names.size();
  return 0;
}

static int32_t host_gq(const uint8_t* L, int32_t at, int32_t len) {
  const std::string s((const char*)L + at, (size_t)len);
  return gt_round_gq(strtod(s.c_str(), nullptr));
}

static int lines(const char* in, const char* outp) {
  std::vector<uint8_t> t;
  if (!slurp(in, t)) return 2;
  FILE* o = fopen(outp, "w");
  if (!o) return 2;
  Header h;
  if (int rc = read_header(t, &h)) {
    fprintf(o, "H nochrom\n");
    fclose(o);
    return rc;
  }
  fprintf(o, "H %d\n", h.S);
  for (const std::string& nm : h.names) fprintf(o, "N %s\n", nm.c_str());
  const dqt::NameTable C = h.CT.view();
  const int32_t S = h.S;
  std::vector<std::pair<int64_t, int64_t>> ls;
  text_lines(t, ls);
  for (size_t k = 0; k < ls.size(); k++) {
    const int64_t a = ls[k].first, z = ls[k].second;
    if (z > a && t[(size_t)a] == '#') continue;
    std::vector<uint8_t> line(t.begin() + a, t.begin() + z);
    const int32_t len = (int32_t)line.size();
    dqv::VcfSite V{};
    if (dqv::vcf_line_walk(line.data(), len, h.H.G, C, nullptr, true, &V) != dqv::VCF_OK) {
      fprintf(o, "%zu X\n", k);
      continue;
    }
    if (S == 0) {
      fprintf(o, "%zu G 0\n", k);
      continue;
    }
    const int32_t fmt_at = V.col_end[7] + 1;
    int32_t nhost = 0;
    const GtLine R = gt_line_walk(line.data(), len, fmt_at, S, V.n_sample_cols, V.n_alt, 0, GtRow{},
                                  [&](int32_t, int32_t, int32_t) { nhost++; });
    if (R.st) {
      fprintf(o, "%zu E %s %d\n", k, gt_status_name(R.st), R.st >= GT_E_CELL ? R.sample : -1);
      continue;
    }
    const int32_t P = R.max_ploidy > 1 ? R.max_ploidy : 1;
    // every array exactly its size, the allele row included
    std::vector<uint8_t> fl((size_t)S), pl((size_t)S);
    std::vector<int16_t> al((size_t)S * (size_t)P);
    std::vector<int32_t> gq((size_t)S), dp((size_t)S), off((size_t)S);
    std::vector<uint8_t> host((size_t)S, 0);
    struct Fix { int32_t s, at, n; };
    std::vector<Fix> fixes;  // applied behind the walk, which stores a cell after it reports its text
    int32_t nhost2 = 0;
    const GtLine D = gt_line_walk(line.data(), len, fmt_at, S, V.n_sample_cols, V.n_alt, P,
                                  GtRow{fl.data(), pl.data(), al.data(), gq.data(), dp.data(), off.data()},
                                  [&](int32_t s, int32_t at, int32_t n) {
                                    nhost2++;
                                    fixes.push_back({s, at, n});
                                  });
    for (const Fix& f : fixes) {
      host[(size_t)f.s] = 1;
      gq[(size_t)f.s] = host_gq(line.data(), f.at, f.n);
    }
    if (D.st || D.max_ploidy != R.max_ploidy || nhost2 != nhost) {
      fprintf(stderr, "line %zu: the check walk and the decode walk disagree\n", k);
      return 4;
    }
    fprintf(o, "%zu G %d", k, P);
    for (int32_t s = 0; s < S; s++) {
      fprintf(o, " %u,%u,%d,%u,%d,%d,", fl[(size_t)s], pl[(size_t)s], gq[(size_t)s], host[(size_t)s],
              dp[(size_t)s], off[(size_t)s]);
      for (int32_t i = 0; i < P; i++) fprintf(o, i ? "/%d" : "%d", al[(size_t)s * (size_t)P + (size_t)i]);
    }
    fprintf(o, "\n");
  }
  fclose(o);
  return 0;
}

struct LineAt {
  int64_t a;
  int32_t len, fmt_at, n_alt, nsc;
};

static int bench(const char* in, int threads, int reps, const char* outp) {
  std::vector<uint8_t> t;
  if (!slurp(in, t)) return 2;
  Header h;
  if (int rc = read_header(t, &h)) return rc;
  const dqt::NameTable C = h.CT.view();
  const int32_t S = h.S;
  std::vector<std::pair<int64_t, int64_t>> all;
  text_lines(t, all);
  std::vector<LineAt> ls;
  for (const auto& l : all)
    if (!(l.second > l.first && t[(size_t)l.first] == '#')) ls.push_back({l.first, (int32_t)(l.second - l.first), 0, 0, 0});
  const size_t n = ls.size();
  auto parallel = [&](auto&& body) {
    std::vector<std::thread> th;
    for (int w = 0; w < threads; w++)
      th.emplace_back([&, w] { body(w, n * (size_t)w / (size_t)threads, n * (size_t)(w + 1) / (size_t)threads); });
    for (auto& x : th) x.join();
  };
  // the site columns the genotype passes start from (dq_vcf_run's part, untimed)
  std::vector<int> bad((size_t)threads, 0);
  parallel([&](int w, size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; k++) {
      dqv::VcfSite V{};
      if (dqv::vcf_line_walk(t.data() + ls[k].a, ls[k].len, h.H.G, C, nullptr, true, &V) != dqv::VCF_OK) {
        bad[(size_t)w]++;
        ls[k].nsc = -1;
        continue;
      }
      ls[k].fmt_at = V.col_end[7] + 1;
      ls[k].n_alt = V.n_alt;
      ls[k].nsc = V.n_sample_cols;
    }
  });
  const size_t cells = n * (size_t)S;
  std::vector<uint8_t> fl(cells), pl(cells);
  std::vector<int16_t> al;
  std::vector<int32_t> gq(cells), dp(cells), off(cells);
  int32_t P = S > 0 ? 1 : 0;
  double best = 1e300;
  int64_t nhost = 0;
  for (int r = 0; r < reps && S > 0; r++) {
    std::vector<int32_t> maxp((size_t)threads, 0);
    std::vector<int64_t> hostn((size_t)threads, 0);
    const auto t0 = std::chrono::steady_clock::now();
    parallel([&](int w, size_t lo, size_t hi) {  // check
      for (size_t k = lo; k < hi; k++) {
        const GtLine R = gt_line_walk(t.data() + ls[k].a, ls[k].len, ls[k].fmt_at, S, ls[k].nsc, ls[k].n_alt, 0,
                                      GtRow{}, [&](int32_t, int32_t, int32_t) { hostn[(size_t)w]++; });
        if (R.st) bad[(size_t)w]++;
        else if (R.max_ploidy > maxp[(size_t)w]) maxp[(size_t)w] = R.max_ploidy;
      }
    });
    P = 1;
    nhost = 0;
    for (int w = 0; w < threads; w++) {
      if (maxp[(size_t)w] > P) P = maxp[(size_t)w];
      nhost += hostn[(size_t)w];
    }
    al.resize(cells * (size_t)P);
    parallel([&](int, size_t lo, size_t hi) {  // decode, the host's GQ texts converted behind each line
      struct Fix { int32_t s, at, n; };
      std::vector<Fix> fixes;
      for (size_t k = lo; k < hi; k++) {
        const size_t c = k * (size_t)S;
        const uint8_t* L = t.data() + ls[k].a;
        fixes.clear();
        gt_line_walk(L, ls[k].len, ls[k].fmt_at, S, ls[k].nsc, ls[k].n_alt, P,
                     GtRow{&fl[c], &pl[c], &al[c * (size_t)P], &gq[c], &dp[c], &off[c]},
                     [&](int32_t s, int32_t at, int32_t m) { fixes.push_back({s, at, m}); });
        for (const Fix& f : fixes) gq[c + (size_t)f.s] = host_gq(L, f.at, f.n);
      }
    });
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (ms < best) best = ms;
  }
  int nbad = 0;
  for (int b : bad) nbad += b;
  if (outp) {
    FILE* o = fopen(outp, "wb");
    if (!o) return 2;
    const int64_t hd[3] = {(int64_t)n, S, P};
    fwrite(hd, 8, 3, o);
    fwrite(fl.data(), 1, cells, o);
    fwrite(pl.data(), 1, cells, o);
    fwrite(al.data(), 2, al.size(), o);
    fwrite(gq.data(), 4, cells, o);
    fwrite(dp.data(), 4, cells, o);
    fwrite(off.data(), 4, cells, o);
    fclose(o);
  }
  printf("{\"lines\": %zu, \"samples\": %d, \"max_ploidy\": %d, \"bytes\": %zu, \"threads\": %d, \"reps\": %d, "
         "\"ms_best\": %.3f, \"n_gq_host\": %lld, \"bad_lines\": %d}\n",
         n, S, P, t.size(), threads, reps, S > 0 ? best : 0.0, (long long)nhost, nbad);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "lines")) return lines(argv[2], argv[3]);
  if ((argc == 5 || argc == 6) && !strcmp(argv[1], "bench"))
    return bench(argv[2], atoi(argv[3]) > 0 ? atoi(argv[3]) : 1, atoi(argv[4]) > 0 ? atoi(argv[4]) : 1,
                 argc == 6 ? argv[5] : nullptr);
  fprintf(stderr, "usage: vcf_gt_check lines IN.vcf OUT.txt | bench IN.vcf THREADS REPS [OUT.bin]\n");
  return 1;
}
