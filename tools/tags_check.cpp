// tags_check.cpp -- the aux tag rules of disq_amd/csrc/dq_tags_core.h run on the host, for
// tests/test_tags_core_cpu.py (and, built with -fsanitize=address,undefined, over the same inputs)
// and as the CPU baseline of tools/tags_bench.py.  It compiles the very functions the tag kernels
// call.  IN.bin holds BAM records back to back, each with its block_size word (the raw bytes of a
// DQ_EXPORT_RAW batch).  KEYS is a ','-separated list of two-byte ids, each optionally followed by
// ":<type>" (0 any, 1 int, 2 float, 3 char, 4 string).
//
//   tags_check records IN.bin KEYS OUT.txt
//       "K <q> <id> <type>" per key ("K bad <reason>" for a refused list), then per record, in file
//       order: "<k> E <what>" (fields, tag XX, tag XX type: the first failing check) or "<k> C"
//       followed by one " flags,vtype,subtype,val_off,val_len,val" per key.  A block_size chain
//       that breaks at record k is its "fields" and ends the output.  Every record is copied into
//       a buffer of exactly its 4 + block_size bytes, so a stray access is a heap overflow.
//   tags_check bench IN.bin KEYS THREADS REPS
//       the records cut into THREADS runs, one thread each: the geometry from the records' heads
//       (untimed, what the records stage leaves in its columns), then the check walk and the decode
//       walk into key-major columns REPS times; prints one JSON line (the best wall time of check +
//       decode, records, aux bytes, a checksum of the columns).
//
//   g++ -O2 -g -std=c++17 -pthread -I disq_amd/csrc -o tags_check tools/tags_check.cpp
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "dq_tags_core.h"

using namespace dqa;

static bool slurp(const char* path, std::vector<uint8_t>& out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  static uint8_t buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
  fclose(f);
  return true;
}

struct Keys {
  std::vector<std::string> ids;
  std::vector<int32_t> types;
  uint32_t slot[TAG_SLOTS];
  uint8_t type[64];
  const char* why = nullptr;
  TagKeys view() const { return TagKeys{slot, type, (int32_t)ids.size()}; }
};

static void parse_keys(const char* arg, Keys* K) {
  const std::string ks(arg);
  size_t a = 0;
  while (a <= ks.size()) {
    size_t e = ks.find(',', a);
    if (e == std::string::npos) e = ks.size();
    std::string id = ks.substr(a, e - a);
    int32_t ty = TAG_ANY;
    const size_t c = id.find(':');
    if (c != std::string::npos) {
      ty = atoi(id.c_str() + c + 1);
      id = id.substr(0, c);
    }
    K->ids.push_back(id);
    K->types.push_back(ty);
    a = e + 1;
  }
  if (K->ids.size() > 64) {
    K->why = "1 to 64 keys are taken";
    return;
  }
  std::vector<const char*> p;
  for (auto& s : K->ids) p.push_back(s.c_str());
  K->why = tag_keys_build(p.data(), K->types.data(), (int32_t)p.size(), K->slot, K->type);
}

static int32_t rd32(const uint8_t* p) { return (int32_t)tag_rd32(p); }

// The record's geometry from its head, as the records stage stores it in its columns.
struct Geo {
  int32_t bs, l_rn, n_cig, l_seq;
};
static Geo geo_of(const uint8_t* r) {
  return Geo{rd32(r), r[12], (int32_t)tag_rd16(r + 16), rd32(r + 20)};
}

struct Cell {
  int32_t flags = 0, vtype = 0, subtype = 0, val_off = -1, val_len = 0;
  uint32_t val = 0;
};
struct CellSink {
  Cell* c;
  void cell(int32_t q, const Tag& T, int32_t val_off, uint32_t v) {
    c[q] = Cell{TAG_PRESENT, T.ty, T.sub, val_off, (int32_t)T.len, v};
  }
  void repeated(int32_t q) { c[q].flags |= TAG_REPEATED; }
};

static int cmd_records(const char* in, const char* keys, const char* outp) {
  std::vector<uint8_t> raw;
  if (!slurp(in, raw)) return 2;
  Keys K;
  parse_keys(keys, &K);
  FILE* o = fopen(outp, "wb");
  if (!o) return 2;
  if (K.why) {
    fprintf(o, "K bad %s\n", K.why);
    fclose(o);
    return 0;
  }
  const int32_t nk = (int32_t)K.ids.size();
  for (int32_t q = 0; q < nk; q++) fprintf(o, "K %d %s %d\n", q, K.ids[q].c_str(), K.types[q]);
  const int64_t n = (int64_t)raw.size();
  int64_t p = 0;
  for (int64_t k = 0; p < n; k++) {
    int32_t bs = -1;
    if (p + 4 <= n) bs = rd32(raw.data() + p);
    if (bs < 32 || p + 4 + (int64_t)bs > n) {  // (a record of fewer than 36 bytes has no head to read)
      fprintf(o, "%lld E fields\n", (long long)k);
      break;
    }
    const int64_t sz = 4 + (int64_t)bs;
    uint8_t* r = (uint8_t*)malloc((size_t)sz);  // exactly the record
    memcpy(r, raw.data() + p, (size_t)sz);
    const Geo g = geo_of(r);
    int64_t aux_at, end;
    int32_t err = 0;
    std::vector<Cell> cells((size_t)nk);
    if (!tag_region(g.bs, g.l_rn, g.n_cig, g.l_seq, &aux_at, &end)) {
      err = TAG_E_FIELDS << 16;
    } else {
      const int64_t len = end - aux_at;
      uint8_t* a = (uint8_t*)malloc((size_t)(len > 0 ? len : 1));  // exactly the aux region
      memcpy(a, r + aux_at, (size_t)len);
      CellSink sink{cells.data()};
      uint64_t seen;
      err = tags_walk(a, len, aux_at, K.view(), sink, &seen);
      free(a);
    }
    if (err) {
      char nb[16];
      fprintf(o, "%lld E %s\n", (long long)k, tag_error_name(err, nb));
    } else {
      fprintf(o, "%lld C", (long long)k);
      for (const Cell& c : cells)
        fprintf(o, " %d,%d,%d,%d,%d,%u", c.flags, c.vtype, c.subtype, c.val_off, c.val_len, c.val);
      fprintf(o, "\n");
    }
    free(r);
    p += sz;
  }
  fclose(o);
  return 0;
}

struct Cols {
  int64_t n;
  std::vector<uint8_t> flags, vtype, subtype;
  std::vector<int32_t> val_off, val_len;
  std::vector<uint32_t> val;
  std::vector<int64_t> base;
};
struct ColSink {
  Cols& o;
  int64_t k;
  void value(int32_t q, uint32_t v) {
    if (o.base[(size_t)q] >= 0) o.val[(size_t)(o.base[(size_t)q] + k)] = v;
  }
  void cell(int32_t q, const Tag& T, int32_t val_off, uint32_t v) {
    const size_t c = (size_t)((int64_t)q * o.n + k);
    o.flags[c] = TAG_PRESENT;
    o.vtype[c] = T.ty;
    o.subtype[c] = T.sub;
    o.val_off[c] = val_off;
    o.val_len[c] = (int32_t)T.len;
    value(q, v);
  }
  void repeated(int32_t q) { o.flags[(size_t)((int64_t)q * o.n + k)] |= TAG_REPEATED; }
  void blank(int32_t q) {
    const size_t c = (size_t)((int64_t)q * o.n + k);
    o.flags[c] = o.vtype[c] = o.subtype[c] = 0;
    o.val_off[c] = -1;
    o.val_len[c] = 0;
    value(q, 0);
  }
};

static int cmd_bench(const char* in, const char* keys, int threads, int reps) {
  std::vector<uint8_t> raw;
  if (!slurp(in, raw)) return 2;
  Keys K;
  parse_keys(keys, &K);
  if (K.why) return 3;
  const int32_t nk = (int32_t)K.ids.size();
  std::vector<int64_t> off;
  std::vector<Geo> geo;
  const int64_t len = (int64_t)raw.size();
  for (int64_t p = 0; p + 36 <= len;) {
    const int32_t bs = rd32(raw.data() + p);
    if (bs < 32 || p + 4 + (int64_t)bs > len) break;
    off.push_back(p);
    geo.push_back(geo_of(raw.data() + p));
    p += 4 + (int64_t)bs;
  }
  const int64_t n = (int64_t)off.size();
  Cols C;
  C.n = n;
  const size_t cells = (size_t)nk * (size_t)n;
  C.flags.resize(cells);
  C.vtype.resize(cells);
  C.subtype.resize(cells);
  C.val_off.resize(cells);
  C.val_len.resize(cells);
  int64_t nval = 0;
  for (int32_t q = 0; q < nk; q++) {
    const bool has = K.types[q] == TAG_INT || K.types[q] == TAG_FLOAT || K.types[q] == TAG_CHAR;
    C.base.push_back(has ? nval : -1);
    if (has) nval += n;
  }
  C.val.resize((size_t)nval);
  if (threads < 1) threads = 1;
  std::vector<int64_t> bad((size_t)threads), aux((size_t)threads);
  double best = 1e30;
  for (int rep = 0; rep < reps; rep++) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> th;
    for (int t = 0; t < threads; t++)
      th.emplace_back([&, t] {
        const int64_t a = n * t / threads, b = n * (t + 1) / threads;
        int64_t nbad = 0, naux = 0;
        for (int pass = 0; pass < 2; pass++)
          for (int64_t k = a; k < b; k++) {
            const uint8_t* r = raw.data() + off[(size_t)k];
            const Geo& g = geo[(size_t)k];
            int64_t aux_at, end;
            if (!tag_region(g.bs, g.l_rn, g.n_cig, g.l_seq, &aux_at, &end)) {
              nbad += pass == 0;
              continue;
            }
            uint64_t seen = 0;
            if (pass == 0) {
              NullSink s;
              nbad += tags_walk(r + aux_at, end - aux_at, aux_at, K.view(), s, &seen) != 0;
              naux += end - aux_at;
            } else {
              ColSink s{C, k};
              if (tags_walk(r + aux_at, end - aux_at, aux_at, K.view(), s, &seen)) continue;
              for (int32_t q = 0; q < nk; q++)
                if (!(seen >> q & 1)) s.blank(q);
            }
          }
        bad[(size_t)t] = nbad;
        aux[(size_t)t] = naux;
      });
    for (auto& x : th) x.join();
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (ms < best) best = ms;
  }
  int64_t nbad = 0, naux = 0;
  for (int t = 0; t < threads; t++) {
    nbad += bad[(size_t)t];
    naux += aux[(size_t)t];
  }
  uint64_t sum = 0;
  for (size_t c = 0; c < cells; c++) sum = sum * 1099511628211ull + C.flags[c] + ((uint64_t)C.vtype[c] << 8) + (uint32_t)C.val_off[c];
  for (uint32_t v : C.val) sum = sum * 1099511628211ull + v;
  printf("{\"records\": %lld, \"keys\": %d, \"threads\": %d, \"aux_bytes\": %lld, \"bad_records\": %lld, "
         "\"ms_best\": %.3f, \"checksum\": \"%016llx\"}\n",
         (long long)n, nk, threads, (long long)naux, (long long)nbad, best, (unsigned long long)sum);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 5 && !strcmp(argv[1], "records")) return cmd_records(argv[2], argv[3], argv[4]);
  if (argc == 6 && !strcmp(argv[1], "bench")) return cmd_bench(argv[2], argv[3], atoi(argv[4]), atoi(argv[5]));
  fprintf(stderr, "usage: tags_check records IN.bin KEYS OUT.txt | tags_check bench IN.bin KEYS THREADS REPS\n");
  return 1;
}
