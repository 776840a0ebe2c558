// dq_vcf_info_core.h -- the per-line rules of the VCF INFO decode: the
// INFO column of a data line against a list of requested keys, as the cells of dq_info_batch --
// what htsjdk's AbstractVCFCodec.parseInfo leaves in a VariantContext's attribute map for those
// keys.  One header for the host and the device: the kernels of dq_vcf_info.hip, the library's host
// side and tools/vcf_info_check.cpp compile the same functions, and one walk serves the check pass
// and the decode pass (they differ in their sink), so the two cannot disagree.  Every load lies in
// the INFO column L[a, z) (L the line's value; the site decode found a and z).
//
// Not done here: Number= checks, VCF 4.3 percent-decoding, the last-wins order of htsjdk's map (the
// first piece of a key is decoded, as section 15 decided for END), keys that were not asked for,
// copies of String values (the span is the access path), BCF.
#pragma once
#include "dq_vcf_core.h"

#ifndef DQI_CHECK  // dq_vcf_info.hip counts a failed bound here in the bounds-checked build
#define DQI_CHECK(cond) ((void)0)
#endif

namespace dqi {

enum : int32_t { INFO_AUTO = 0, INFO_FLAG = 1, INFO_INTEGER = 2, INFO_FLOAT = 3, INFO_STRING = 4 };
enum : int32_t { INFO_PRESENT = 1, INFO_HAS_VALUE = 2, INFO_REPEATED = 4 };  // cell flags
constexpr int32_t INFO_MAX_KEYS = 64;  // a line's seen keys are one 64-bit mask
constexpr int32_t INFO_I_MISSING = -2147483647 - 1;
constexpr uint64_t INFO_F_MISSING_BITS = 0x7ff8000000000001ull;  // a quiet NaN with payload 1
constexpr uint64_t INFO_F_NAN_BITS = 0x7ff8000000000000ull;      // Java's Double.NaN
constexpr uint64_t INFO_F_INF_BITS = 0x7ff0000000000000ull;

// ------------------------------------------------------------------ the requested keys
// tab: the ids as a name table (dq_text_core.h), key q its name q; type: the resolved conversion
// type of key q; hflag: the header's ##INFO line types key q as Flag.  Built on the host
// (info_key_table_build).
struct InfoKeys {
  dqt::NameTable tab;
  const uint8_t* type;
  const uint8_t* hflag;
};

// ------------------------------------------------------------------ one cell
struct InfoCell {
  int32_t flags, n_values, val_off, val_len;
};
DQT_INLINE InfoCell info_blank() { return InfoCell{0, 0, -1, 0}; }

DQT_INLINE bool info_is(const uint8_t* t, int32_t n, const char* w, int32_t wn) {
  if (n != wn) return false;
  for (int32_t i = 0; i < n; i++)
    if (t[i] != (uint8_t)w[i]) return false;
  return true;
}

// One element of a Float value: '.', the QUAL grammar, or Java Double.valueOf's NaN, Infinity,
// +Infinity, -Infinity.  0: *bits holds the value; 1: the host's strtod converts it; 2: refused.
DQT_INLINE int info_float(const uint8_t* t, int32_t n, uint64_t* bits) {
  *bits = INFO_F_MISSING_BITS;
  if (n == 1 && t[0] == '.') return 0;
  if (n >= 3 && (t[0] == 'N' || t[0] == 'I' || t[1] == 'I')) {
    if (info_is(t, n, "NaN", 3)) return *bits = INFO_F_NAN_BITS, 0;
    if (info_is(t, n, "Infinity", 8) || info_is(t, n, "+Infinity", 9)) return *bits = INFO_F_INF_BITS, 0;
    if (info_is(t, n, "-Infinity", 9)) return *bits = INFO_F_INF_BITS | 1ull << 63, 0;
    return 2;
  }
  double v;
  const int r = dqv::vcf_parse_qual(t, n, &v);
  if (r == dqv::VCF_Q_BAD) return 2;
  union {
    double d;
    uint64_t u;
  } c;
  c.d = v;
  *bits = c.u;
  return r == dqv::VCF_Q_UNDECIDED ? 1 : 0;
}

// The ',' pieces of the value text L[va, vz) of a key of `type`: *nv their number.  INTEGER and FLOAT
// elements go to the sink (ival(j, v) / fval(j, bits) / host(j, at, len): element j is left to the
// host's strtod, text L[at, at + len)); false at the first element that fails its grammar.
template <class Sink>
DQT_INLINE bool info_values(const uint8_t* L, int32_t va, int32_t vz, int32_t type, int32_t* nv, Sink& sink) {
  int32_t j = 0;
  for (int32_t b = va;;) {
    int32_t e = b;
    while (e < vz && L[e] != ',') e++;
    const int32_t n = e - b;
    if (type == INFO_INTEGER) {
      int32_t v = INFO_I_MISSING;
      if (n == 0) return false;
      if (!(n == 1 && L[b] == '.') && !dqv::vcf_int32(L + b, n, &v)) return false;
      sink.ival(j, v);
    } else if (type == INFO_FLOAT) {
      uint64_t bits;
      if (n == 0) return false;
      const int r = info_float(L + b, n, &bits);
      if (r == 2) return false;
      sink.fval(j, bits);
      if (r == 1) sink.host(j, b, n);
    }
    j++;
    if (e >= vz) break;
    b = e + 1;
  }
  *nv = j;
  return true;
}

// The piece L[.., pe) whose key ends at ke (ke == pe: no '='), for a key of conversion `type` that
// the header types as Flag or not (hflag).  False when a value fails its grammar (*C blank then).
template <class Sink>
DQT_INLINE bool info_cell(const uint8_t* L, int32_t ke, int32_t pe, int32_t type, bool hflag, InfoCell* C,
                          Sink& sink) {
  *C = info_blank();
  if (ke >= pe) {  // no '=': in the map (true for a Flag, the missing value otherwise)
    C->flags = INFO_PRESENT;
    return true;
  }
  const int32_t va = ke + 1, n = pe - va;
  if (hflag && n == 1 && L[va] == '0') return true;  // "DB=0": htsjdk leaves it out of the map
  C->flags = INFO_PRESENT;
  C->val_off = va;
  C->val_len = n;
  if (n == 0 || (n == 1 && L[va] == '.')) return true;  // "key=" and "key=.": the missing value
  C->flags |= INFO_HAS_VALUE;
  if (info_values(L, va, pe, type, &C->n_values, sink)) return true;
  *C = info_blank();
  return false;
}

// the end of the key that starts at b: the first '=' or ';' or z
DQT_INLINE int32_t info_key_end(const uint8_t* L, int32_t b, int32_t z) {
  int32_t e = b;
  while (e < z && L[e] != '=' && L[e] != ';') e++;
  return e;
}
DQT_INLINE int32_t info_piece_end(const uint8_t* L, int32_t b, int32_t z) {
  int32_t e = b;
  while (e < z && L[e] != ';') e++;
  return e;
}

template <class Sink>
struct InfoKeySink {  // a line sink seen from one key's cell
  Sink& s;
  int32_t q;
  DQT_INLINE void ival(int32_t j, int32_t v) { s.ival(q, j, v); }
  DQT_INLINE void fval(int32_t j, uint64_t bits) { s.fval(q, j, bits); }
  DQT_INLINE void host(int32_t j, int32_t at, int32_t len) { s.host(q, j, at, len); }
};

// ------------------------------------------------------------------ the line walk
// Walks the INFO column L[a, z) of a line byte by byte.  Every requested key gets exactly one
// sink.cell(q, C) -- the first piece with that key, or a blank cell when no piece has it -- after
// its elements (sink.ival / fval / host, see info_values), and sink.repeated(q) behind that when
// a later piece has the same key.  Returns the lowest index of a key whose value failed, or -1.
template <class Sink>
DQT_INLINE int32_t info_line_walk(const uint8_t* L, int32_t a, int32_t z, const InfoKeys& T, Sink& sink) {
  uint64_t seen = 0, rep = 0;
  int32_t bad = -1;
  if (!(z - a == 1 && L[a] == '.')) {
    for (int32_t b = a; b < z;) {
      DQI_CHECK(b >= a && b < z);
      const int32_t ke = info_key_end(L, b, z);
      const int32_t pe = ke < z && L[ke] == '=' ? info_piece_end(L, ke, z) : ke;
      const int32_t q = dqt::name_lookup(T.tab, L + b, ke - b);
      if (q >= 0) {
        const uint64_t bit = 1ull << q;
        if (seen & bit) {
          rep |= bit;
        } else {
          seen |= bit;
          InfoCell C;
          InfoKeySink<Sink> ks{sink, q};
          if (!info_cell(L, ke, pe, T.type[q], T.hflag[q] != 0, &C, ks) && (bad < 0 || q < bad)) bad = q;
          sink.cell(q, C);
        }
      }
      b = pe + 1;
    }
  }
  for (int32_t q = 0; q < T.tab.n; q++) {
    if (!(seen >> q & 1)) sink.cell(q, info_blank());
    else if (rep >> q & 1) sink.repeated(q);
  }
  return bad;
}

// first offender: the lowest line, then the lowest key index
DQT_INLINE unsigned long long info_error_key(int64_t line, int32_t q) {
  return (unsigned long long)line << 8 | (unsigned long long)(q & 0xff);
}

}  // namespace dqi

// ------------------------------------------------------------------ host side: header and key list
#include <map>
#include <string>
#include <vector>

namespace dqi {

// The ##INFO lines of the header text t[0, n): ID -> type, a repeated ID keeps its first line.  Per
// line the values of the first ','-separated pieces starting with "ID=" and "Type=", pieces lying
// between '<' and the last '>' (the ##contig rule: quoted commas are not honoured).
inline void info_header_types(const uint8_t* t, int64_t n, std::map<std::string, int32_t>* M) {
  M->clear();
  int64_t a = (n >= 3 && t[0] == 0xEF && t[1] == 0xBB && t[2] == 0xBF) ? 3 : 0;
  while (a < n && t[a] == '#') {
    int64_t z = a;
    while (z < n && t[z] != '\n' && t[z] != '\r') z++;
    const std::string line((const char*)t + a, (size_t)(z - a));
    if (line.compare(0, 8, "##INFO=<") == 0) {
      size_t end = line.rfind('>');
      if (end == std::string::npos || end < 8) end = line.size();
      std::string id, ty;
      bool hid = false, hty = false;
      for (size_t b = 8; b <= end;) {
        size_t e = line.find(',', b);
        if (e == std::string::npos || e > end) e = end;
        if (!hid && e - b >= 3 && line.compare(b, 3, "ID=") == 0) id = line.substr(b + 3, e - b - 3), hid = true;
        if (!hty && e - b >= 5 && line.compare(b, 5, "Type=") == 0) ty = line.substr(b + 5, e - b - 5), hty = true;
        b = e + 1;
      }
      if (hid && !M->count(id))
        (*M)[id] = ty == "Flag" ? INFO_FLAG : ty == "Integer" ? INFO_INTEGER : ty == "Float" ? INFO_FLOAT : INFO_STRING;
    }
    a = z;
    while (a < n && (t[a] == '\n' || t[a] == '\r')) a++;
  }
}

struct InfoKeysHost {
  dqt::NameTableHost tab;
  std::vector<uint8_t> type, hflag;
  InfoKeys view() const { return InfoKeys{tab.view(), type.data(), hflag.data()}; }
};

// 0, or the reason the list is refused: the count, an id that is empty or holds one of ";=,\t ", an
// id given twice, an unknown type.  types: AUTO takes the header's, STRING without a line.
inline const char* info_key_table_build(const std::vector<std::string>& ids, const std::vector<int32_t>& types,
                                        const std::map<std::string, int32_t>& header, InfoKeysHost* T) {
  const size_t K = ids.size();
  if (K < 1 || K > (size_t)INFO_MAX_KEYS || types.size() != K) return "1 to 64 keys are taken";
  *T = InfoKeysHost{};
  for (size_t q = 0; q < K; q++) {
    const std::string& id = ids[q];
    if (id.empty() || id.find_first_of(";=,\t ") != std::string::npos) return "an INFO key is empty or holds ';', '=', ',', a TAB or a space";
    for (size_t p = 0; p < q; p++)
      if (ids[p] == id) return "an INFO key is given twice";
    if (types[q] < INFO_AUTO || types[q] > INFO_STRING) return "unknown INFO type";
    const auto h = header.find(id);
    const int32_t ht = h == header.end() ? 0 : h->second;
    T->type.push_back((uint8_t)(types[q] != INFO_AUTO ? types[q] : ht ? ht : INFO_STRING));
    T->hflag.push_back(ht == INFO_FLAG ? 1 : 0);
  }
  dqt::name_table_build(ids, &T->tab);
  return nullptr;
}

}  // namespace dqi
