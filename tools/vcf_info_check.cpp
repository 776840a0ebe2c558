// vcf_info_check.cpp -- the INFO rules of disq_amd/csrc/dq_vcf_info_core.h run on the host, for
// tests/test_vcf_info_core_cpu.py (and, built with -fsanitize=address,undefined, over the same
// inputs) and as the CPU baseline of tools/vcf_info_bench.py.  It compiles the very functions the
// INFO kernels call.  KEYS is a ','-separated list of ids, each optionally followed by ":<type>"
// (0 auto, 1 Flag, 2 Integer, 3 Float, 4 String).
//
//   vcf_info_check lines IN.vcf KEYS OUT.txt
//       "K <q> <id> <resolved type> <header Flag>" per key ("K bad <reason>" for a refused list),
//       then per line that does not start with '#', in file order: "<k> X" when the site decode
//       (dq_vcf_core.h) rejects it, "<k> E <q>" (the lowest failing key), or "<k> C" followed by
//       one " flags,n_values,val_off,val_len,host,v0/v1/..." per key (Integer values in decimal,
//       Float values as the 16 hex digits of their bits after the host's strtod of the texts left
//       to it, host their number; "-" without values).  Every INFO column is copied into a buffer of
//       exactly its length and every value row has exactly its size, so a stray access is a heap
//       overflow.
//   vcf_info_check bench IN.vcf KEYS THREADS REPS [OUT.bin]
//       the data lines cut into THREADS runs of whole lines, one thread each: the site walk for
//       col_end (untimed), then the check pass and the decode pass REPS times; prints one JSON line
//       (the best wall time of check + decode); OUT.bin takes n, K, n_ival, n_fval, n_float_host
//       (5 x i64), key_type, key_width (i32 x K), key_base (i64 x K), then flags (u8), n_values,
//       val_off, val_len (i32), K * n cells each, key-major, then ival (i32) and fval (f64).
//
//   g++ -O2 -g -std=c++17 -pthread -I disq_amd/csrc -o vcf_info_check tools/vcf_info_check.cpp
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "dq_vcf_info_core.h"

using namespace dqi;

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

struct Setup {
  dqv::VcfHeader H;
  dqt::NameTableHost CT;
  InfoKeysHost KT;
  std::vector<std::string> ids;
  const char* why = nullptr;
};

static int setup(const std::vector<uint8_t>& t, const char* keys, Setup* S) {
  dqv::vcf_header_parse(t.data(), (int64_t)t.size(), true, &S->H);
  if (S->H.has_data && !S->H.has_chrom) return 3;
  dqt::name_table_build(S->H.contigs, &S->CT);
  std::map<std::string, int32_t> types;
  info_header_types(t.data(), (int64_t)t.size(), &types);
  std::vector<int32_t> ty;
  const std::string ks(keys);
  for (size_t b = 0; b <= ks.size();) {
    size_t e = ks.find(',', b);
    if (e == std::string::npos) e = ks.size();
    std::string id = ks.substr(b, e - b);
    int32_t want = INFO_AUTO;
    const size_t c = id.rfind(':');
    if (c != std::string::npos) {
      want = atoi(id.c_str() + c + 1);
      id.resize(c);
    }
    S->ids.push_back(id);
    ty.push_back(want);
    b = e + 1;
  }
  S->why = info_key_table_build(S->ids, ty, types, &S->KT);
  return 0;
}

static uint64_t host_float(const uint8_t* L, int32_t at, int32_t len) {
  const std::string s((const char*)L + at, (size_t)len);
  const double v = strtod(s.c_str(), nullptr);
  uint64_t u;
  memcpy(&u, &v, 8);
  return u;
}

struct CountSink {  // the check pass: value counts per key, the host's texts counted
  std::vector<int32_t>& nv;
  int64_t nhost = 0;
  void ival(int32_t, int32_t, int32_t) {}
  void fval(int32_t, int32_t, uint64_t) {}
  void host(int32_t, int32_t, int32_t, int32_t) { nhost++; }
  void repeated(int32_t) {}
  void cell(int32_t q, const InfoCell& C) { nv[(size_t)q] = C.n_values; }
};

struct RowSink {  // one line's decode into rows of exactly their size
  const uint8_t* L;
  InfoCell* cells;
  int32_t** iv;
  uint64_t** fv;
  int32_t* nhost;
  void ival(int32_t q, int32_t j, int32_t v) { iv[q][j] = v; }
  void fval(int32_t q, int32_t j, uint64_t b) { fv[q][j] = b; }
  void host(int32_t q, int32_t j, int32_t at, int32_t len) {
    fv[q][j] = host_float(L, at, len);
    nhost[q]++;
  }
  void repeated(int32_t q) { cells[q].flags |= INFO_REPEATED; }
  void cell(int32_t q, const InfoCell& C) { cells[q] = C; }
};

static int lines(const char* in, const char* keys, const char* outp) {
  std::vector<uint8_t> t;
  if (!slurp(in, t)) return 2;
  FILE* o = fopen(outp, "w");
  if (!o) return 2;
  Setup S;
  if (int rc = setup(t, keys, &S)) {
    fprintf(o, "H nochrom\n");
    fclose(o);
    return rc;
  }
  if (S.why) {
    fprintf(o, "K bad %s\n", S.why);
    fclose(o);
    return 0;
  }
  const InfoKeys T = S.KT.view();
  const size_t K = (size_t)T.tab.n;
  for (size_t q = 0; q < K; q++) fprintf(o, "K %zu %s %d %d\n", q, S.ids[q].c_str(), T.type[q], T.hflag[q]);
  const dqt::NameTable C = S.CT.view();
  std::vector<std::pair<int64_t, int64_t>> ls;
  text_lines(t, ls);
  for (size_t k = 0; k < ls.size(); k++) {
    const int64_t a = ls[k].first, z = ls[k].second;
    if (z > a && t[(size_t)a] == '#') continue;
    dqv::VcfSite V{};
    if (dqv::vcf_line_walk(t.data() + a, (int32_t)(z - a), S.H.G, C, nullptr, true, &V) != dqv::VCF_OK) {
      fprintf(o, "%zu X\n", k);
      continue;
    }
    const int32_t ia = V.col_end[6] + 1, iz = V.col_end[7], il = iz - ia;
    std::vector<uint8_t> col(t.begin() + a + ia, t.begin() + a + iz);  // exactly the INFO column
    std::vector<int32_t> nv(K, 0);
    CountSink cs{nv};
    const int32_t bad = info_line_walk(col.data(), 0, il, T, cs);
    if (bad >= 0) {
      fprintf(o, "%zu E %d\n", k, bad);
      continue;
    }
    std::vector<std::vector<int32_t>> iv(K);
    std::vector<std::vector<uint64_t>> fv(K);
    std::vector<int32_t*> ivp(K);
    std::vector<uint64_t*> fvp(K);
    for (size_t q = 0; q < K; q++) {
      if (T.type[q] == INFO_INTEGER) iv[q].resize((size_t)nv[q]);
      if (T.type[q] == INFO_FLOAT) fv[q].resize((size_t)nv[q]);
      ivp[q] = iv[q].data();
      fvp[q] = fv[q].data();
    }
    std::vector<InfoCell> cells(K);
    std::vector<int32_t> nhost(K, 0);
    RowSink rs{col.data(), cells.data(), ivp.data(), fvp.data(), nhost.data()};
    int64_t hosts = 0;
    if (info_line_walk(col.data(), 0, il, T, rs) >= 0) {
      fprintf(stderr, "line %zu: the check walk and the decode walk disagree\n", k);
      return 4;
    }
    for (int32_t h : nhost) hosts += h;
    if (hosts != cs.nhost) {
      fprintf(stderr, "line %zu: the check walk and the decode walk disagree on the host's texts\n", k);
      return 4;
    }
    fprintf(o, "%zu C", k);
    for (size_t q = 0; q < K; q++) {
      const InfoCell& c = cells[q];
      if (c.n_values != nv[q]) return 4;
      fprintf(o, " %d,%d,%d,%d,%d,", c.flags, c.n_values, c.val_off < 0 ? -1 : c.val_off + ia, c.val_len, nhost[q]);
      if (iv[q].empty() && fv[q].empty()) fprintf(o, "-");
      for (size_t j = 0; j < iv[q].size(); j++) fprintf(o, j ? "/%d" : "%d", iv[q][j]);
      for (size_t j = 0; j < fv[q].size(); j++) fprintf(o, j ? "/%016llx" : "%016llx", (unsigned long long)fv[q][j]);
    }
    fprintf(o, "\n");
  }
  fclose(o);
  return 0;
}

struct LineAt {
  int64_t a;
  int32_t len, ia, iz;
};

struct MaxSink {  // the check pass of the bench: widths, the host's texts counted
  int32_t* width;
  int64_t nhost = 0;
  void ival(int32_t, int32_t, int32_t) {}
  void fval(int32_t, int32_t, uint64_t) {}
  void host(int32_t, int32_t, int32_t, int32_t) { nhost++; }
  void repeated(int32_t) {}
  void cell(int32_t q, const InfoCell& C) {
    if (C.n_values > width[q]) width[q] = C.n_values;
  }
};

struct ColSink {  // the decode pass of the bench: the key-major columns of dq_info_batch
  const uint8_t* L;
  size_t n, k;
  const uint8_t* type;
  const int32_t* width;
  const int64_t* base;
  uint8_t* flags;
  int32_t *nval, *off, *len, *iv;
  uint64_t* fv;
  void ival(int32_t q, int32_t j, int32_t v) { iv[(size_t)base[q] + k * (size_t)width[q] + (size_t)j] = v; }
  void fval(int32_t q, int32_t j, uint64_t b) { fv[(size_t)base[q] + k * (size_t)width[q] + (size_t)j] = b; }
  void host(int32_t q, int32_t j, int32_t at, int32_t m) { fval(q, j, host_float(L, at, m)); }
  void repeated(int32_t q) { flags[(size_t)q * n + k] |= INFO_REPEATED; }
  void cell(int32_t q, const InfoCell& C) {
    const size_t c = (size_t)q * n + k;
    flags[c] = (uint8_t)C.flags;
    nval[c] = C.n_values;
    off[c] = C.val_off;
    len[c] = C.val_len;
    for (int32_t j = C.n_values; j < width[q]; j++) {
      if (type[q] == INFO_INTEGER) ival(q, j, INFO_I_MISSING);
      if (type[q] == INFO_FLOAT) fval(q, j, INFO_F_MISSING_BITS);
    }
  }
};

static int bench(const char* in, const char* keys, int threads, int reps, const char* outp) {
  std::vector<uint8_t> t;
  if (!slurp(in, t)) return 2;
  Setup S;
  if (int rc = setup(t, keys, &S)) return rc;
  if (S.why) {
    fprintf(stderr, "%s\n", S.why);
    return 1;
  }
  const InfoKeys T = S.KT.view();
  const size_t K = (size_t)T.tab.n;
  const dqt::NameTable C = S.CT.view();
  std::vector<std::pair<int64_t, int64_t>> all;
  text_lines(t, all);
  std::vector<LineAt> ls;
  for (const auto& l : all)
    if (!(l.second > l.first && t[(size_t)l.first] == '#')) ls.push_back({l.first, (int32_t)(l.second - l.first), 0, 0});
  const size_t n = ls.size();
  auto parallel = [&](auto&& body) {
    std::vector<std::thread> th;
    for (int w = 0; w < threads; w++)
      th.emplace_back([&, w] { body(w, n * (size_t)w / (size_t)threads, n * (size_t)(w + 1) / (size_t)threads); });
    for (auto& x : th) x.join();
  };
  // the column ends the INFO passes start from (dq_vcf_run's part, untimed)
  std::vector<int> bad((size_t)threads, 0);
  parallel([&](int w, size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; k++) {
      dqv::VcfSite V{};
      if (dqv::vcf_line_walk(t.data() + ls[k].a, ls[k].len, S.H.G, C, nullptr, false, &V) != dqv::VCF_OK) {
        bad[(size_t)w]++;
        ls[k].ia = ls[k].iz = -1;
        continue;
      }
      ls[k].ia = V.col_end[6] + 1;
      ls[k].iz = V.col_end[7];
    }
  });
  const size_t cells = n * K;
  std::vector<uint8_t> fl(cells);
  std::vector<int32_t> nval(cells), off(cells), len(cells), iv, width(K, 1);
  std::vector<uint64_t> fv;
  std::vector<int64_t> base(K, -1);
  double best = 1e300;
  int64_t nhost = 0;
  for (int r = 0; r < reps; r++) {
    std::vector<std::vector<int32_t>> wd((size_t)threads, std::vector<int32_t>(K, 1));
    std::vector<int64_t> hostn((size_t)threads, 0);
    const auto t0 = std::chrono::steady_clock::now();
    parallel([&](int w, size_t lo, size_t hi) {  // check
      MaxSink ms{wd[(size_t)w].data()};
      for (size_t k = lo; k < hi; k++) {
        if (ls[k].ia < 0) continue;
        if (info_line_walk(t.data() + ls[k].a, ls[k].ia, ls[k].iz, T, ms) >= 0) bad[(size_t)w]++;
      }
      hostn[(size_t)w] = ms.nhost;
    });
    nhost = 0;
    int64_t nival = 0, nfval = 0;
    for (size_t q = 0; q < K; q++) {
      width[q] = 1;
      for (int w = 0; w < threads; w++) width[q] = std::max(width[q], wd[(size_t)w][q]);
      base[q] = -1;
      if (T.type[q] == INFO_INTEGER) base[q] = nival, nival += (int64_t)n * width[q];
      if (T.type[q] == INFO_FLOAT) base[q] = nfval, nfval += (int64_t)n * width[q];
    }
    for (int w = 0; w < threads; w++) nhost += hostn[(size_t)w];
    iv.resize((size_t)nival);
    fv.resize((size_t)nfval);
    parallel([&](int, size_t lo, size_t hi) {  // decode, the host's Float texts converted on the way
      for (size_t k = lo; k < hi; k++) {
        ColSink cs{t.data() + ls[k].a, n,          k,          T.type,    width.data(), base.data(),
                   fl.data(),          nval.data(), off.data(), len.data(), iv.data(),    fv.data()};
        if (ls[k].ia < 0) {
          for (size_t q = 0; q < K; q++) cs.cell((int32_t)q, info_blank());
          continue;
        }
        info_line_walk(t.data() + ls[k].a, ls[k].ia, ls[k].iz, T, cs);
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
    const int64_t hd[5] = {(int64_t)n, (int64_t)K, (int64_t)iv.size(), (int64_t)fv.size(), nhost};
    std::vector<int32_t> ty(K);
    for (size_t q = 0; q < K; q++) ty[q] = T.type[q];
    fwrite(hd, 8, 5, o);
    fwrite(ty.data(), 4, K, o);
    fwrite(width.data(), 4, K, o);
    fwrite(base.data(), 8, K, o);
    fwrite(fl.data(), 1, cells, o);
    fwrite(nval.data(), 4, cells, o);
    fwrite(off.data(), 4, cells, o);
    fwrite(len.data(), 4, cells, o);
    fwrite(iv.data(), 4, iv.size(), o);
    fwrite(fv.data(), 8, fv.size(), o);
    fclose(o);
  }
  printf("{\"lines\": %zu, \"keys\": %zu, \"bytes\": %zu, \"threads\": %d, \"reps\": %d, \"ms_best\": %.3f, "
         "\"n_float_host\": %lld, \"bad_lines\": %d}\n",
         n, K, t.size(), threads, reps, best, (long long)nhost, nbad);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 5 && !strcmp(argv[1], "lines")) return lines(argv[2], argv[3], argv[4]);
  if ((argc == 6 || argc == 7) && !strcmp(argv[1], "bench"))
    return bench(argv[2], argv[3], atoi(argv[4]) > 0 ? atoi(argv[4]) : 1, atoi(argv[5]) > 0 ? atoi(argv[5]) : 1,
                 argc == 7 ? argv[6] : nullptr);
  fprintf(stderr, "usage: vcf_info_check lines IN.vcf KEYS OUT.txt | bench IN.vcf KEYS THREADS REPS [OUT.bin]\n");
  return 1;
}
