// sam_write_check.cpp -- the per-record rules of disq_amd/csrc/dq_samw_core.h run on the host, for
// tests/test_sam_write_cpu.py (and, built by hand with -fsanitize=address,undefined, over the same
// inputs).  It compiles the very functions the SAM writer's kernels call.
//
//   sam_write_check lines IN.bin OUT.bin
//       IN: u32 n_ref, per reference u32 length + name bytes; u32 n_records, per record u32 length +
//       its bytes (block_size word included; a length that is not 4 + block_size is the chain error
//       "fields").  OUT per record: u32 kind (0 line, 1 error), u32 length, the line's bytes (LF
//       included) or the error class ("fields", "QNAME", ..., "tag XX").  Every line is sized
//       first and written into a buffer of exactly that size followed by guard bytes; every record
//       is also walked the way a wave walks a long one (SEQ and QUAL stepped over) and must come to
//       the same status, size and offsets.
//   sam_write_check floats IN.txt OUT.txt
//       per line of IN (a bit pattern, 8 hex digits): Float.toString of that binary32.
//
//   g++ -O1 -g -std=c++17 -I disq_amd/csrc -o sam_write_check tools/sam_write_check.cpp
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dq_samw_core.h"

using namespace dqw;

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

static int lines(const char* in, const char* outp) {
  std::vector<uint8_t> t;
  if (!slurp(in, t)) return 2;
  FILE* o = fopen(outp, "wb");
  if (!o) return 2;
  size_t p = 0;
  auto get32 = [&](uint32_t* v) {
    if (p + 4 > t.size()) return false;
    memcpy(v, &t[p], 4);
    p += 4;
    return true;
  };
  uint32_t nref = 0, nrec = 0;
  if (!get32(&nref)) return 3;
  std::vector<uint8_t> names;
  std::vector<int32_t> off{0};
  for (uint32_t r = 0; r < nref; r++) {
    uint32_t ln;
    if (!get32(&ln) || p + ln > t.size()) return 3;
    names.insert(names.end(), t.begin() + p, t.begin() + p + ln);
    off.push_back((int32_t)names.size());
    p += ln;
  }
  names.push_back(0);
  const RefNames R{off.data(), names.data(), (int32_t)nref};
  if (!get32(&nrec)) return 3;
  constexpr int GUARD = 64;
  for (uint32_t k = 0; k < nrec; k++) {
    uint32_t ln;
    if (!get32(&ln) || p + ln > t.size()) return 3;
    // the record in a buffer of its own, so that a read past it is a heap overflow
    std::vector<uint8_t> rec(t.begin() + p, t.begin() + p + ln);
    p += ln;
    Walk W;
    int32_t st = samw_record_walk(rec.data(), (int64_t)ln, R, nullptr, 0, false, false, &W);
    if (st != dqs::SAM_E_FIELDS && W.L.end != (int64_t)ln) st = dqs::SAM_E_FIELDS;  // the chain
    if (st == dqs::SAM_OK || st >= dqs::SAM_E_TAG || st == dqs::SAM_E_QUAL) {
      // the walk lane 0 of a wave makes: QUAL scanned by the caller, SEQ and QUAL stepped over
      bool all_ff = true, bad = false;
      for (int32_t i = 0; i < W.L.l_seq; i++) {
        all_ff = all_ff && rec[(size_t)W.L.qual_at + i] == 0xff;
        bad = bad || rec[(size_t)W.L.qual_at + i] > 93;
      }
      Walk V;
      int32_t sv = samw_record_walk(rec.data(), (int64_t)ln, R, nullptr, 0, true, all_ff, &V);
      if ((sv == dqs::SAM_OK || sv >= dqs::SAM_E_TAG) && !all_ff && bad) sv = dqs::SAM_E_QUAL;
      const bool same = sv == st && (st != dqs::SAM_OK || (V.size == W.size && V.seq_out == W.seq_out &&
                                                           V.qual_out == W.qual_out &&
                                                           V.qual_star == W.qual_star));
      if (!same) {
        fprintf(stderr, "record %u: the walk that steps over SEQ and QUAL disagrees (%d vs %d)\n", k, sv, st);
        return 4;
      }
    }
    if (st != dqs::SAM_OK) {
      char buf[8];
      const char* w = dqs::sam_status_name(st, buf);
      put32(o, 1);
      put32(o, (uint32_t)strlen(w));
      fwrite(w, 1, strlen(w), o);
      continue;
    }
    std::vector<uint8_t> line((size_t)W.size + GUARD, 0xA5);
    Walk J;
    const int32_t st2 = samw_record_walk(rec.data(), (int64_t)ln, R, line.data(), W.size, false, false, &J);
    bool ok = st2 == dqs::SAM_OK && J.size == W.size;
    for (int g = 0; g < GUARD; g++) ok = ok && line[(size_t)W.size + g] == 0xA5;
    if (!ok) {
      fprintf(stderr, "record %u: the format pass disagrees with the size pass\n", k);
      return 4;
    }
    put32(o, 0);
    put32(o, (uint32_t)W.size);
    fwrite(line.data(), 1, (size_t)W.size, o);
  }
  fclose(o);
  return 0;
}

static int floats(const char* in, const char* outp) {
  FILE* f = fopen(in, "r");
  FILE* o = fopen(outp, "w");
  if (!f || !o) return 2;
  char ln[64];
  while (fgets(ln, sizeof ln, f)) {
    const uint32_t bits = (uint32_t)strtoul(ln, nullptr, 16);
    uint8_t buf[32];
    Sink s{buf, (int64_t)sizeof buf};
    put_float(s, bits);
    if (s.over || s.pos > 16) return 4;
    fwrite(buf, 1, (size_t)s.pos, o);
    fputc('\n', o);
  }
  fclose(f);
  fclose(o);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "lines")) return lines(argv[2], argv[3]);
  if (argc == 4 && !strcmp(argv[1], "floats")) return floats(argv[2], argv[3]);
  fprintf(stderr, "usage: sam_write_check lines IN.bin OUT.bin | floats IN.txt OUT.txt\n");
  return 1;
}
