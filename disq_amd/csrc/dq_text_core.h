// dq_text_core.h -- what the text decoders' per-line rules share (dq_sam_core.h, dq_vcf_core.h and
// the headers on top of them): the host fallback of __host__ / __device__, the signed-decimal
// parser of the integer columns, and the name table that resolves @SQ names, ##contig IDs and
// requested INFO keys.  One header for the host and the device, like the rule headers themselves.
#pragma once
#include <stdint.h>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#define __device__
#endif
#endif

#define DQT_INLINE __host__ __device__ inline
#ifndef DQT_CHECK  // a kernel unit counts a failed bound here in the bounds-checked build: it defines
#define DQT_CHECK(cond) ((void)0)  // the macro before its first include (dq_internal.h includes this)
#endif

namespace dqt {

// ------------------------------------------------------------------ numbers
DQT_INLINE bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }

// [-+]?[0-9]+ (the sign only when sgn) within [lo, hi]; any number of digits.  *v is set whenever
// the text has the form, in range or not.
DQT_INLINE bool parse_dec(const uint8_t* t, int32_t n, bool sgn, int64_t lo, int64_t hi, int64_t* v) {
  int32_t i = 0;
  bool neg = false;
  if (sgn && n > 0 && (t[0] == '-' || t[0] == '+')) {
    neg = t[0] == '-';
    i = 1;
  }
  if (i >= n) return false;
  int64_t x = 0;
  for (; i < n; i++) {
    if (!is_digit(t[i])) return false;
    if (x < (1ll << 40)) x = x * 10 + (t[i] - '0');  // saturates far above every range
  }
  if (neg) x = -x;
  *v = x;
  return x >= lo && x <= hi;
}

// ------------------------------------------------------------------ names
// hash: FNV-1a of every name, sorted ascending, ties by name index (so equal names resolve to the
// first, as list.index does); idx: the name index of each sorted entry; the bytes of name r are
// names[name_off[r], name_off[r + 1]).  Built on the host (name_table_build).
struct NameTable {
  const uint64_t* hash;
  const int32_t* idx;
  const int32_t* name_off;  // n + 1 offsets into names, by name index
  const uint8_t* names;
  int32_t n;
};

DQT_INLINE uint64_t name_hash(const uint8_t* p, int32_t n) {
  uint64_t h = 0xcbf29ce484222325ULL;
  for (int32_t i = 0; i < n; i++) h = (h ^ p[i]) * 0x100000001b3ULL;
  return h;
}

// The index of the first name equal to p[0, n) byte for byte, or -1 (always, of an empty table).
DQT_INLINE int32_t name_lookup(const NameTable& T, const uint8_t* p, int32_t n) {
  const uint64_t h = name_hash(p, n);
  int32_t lo = 0, hi = T.n;
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    if (T.hash[mid] < h) lo = mid + 1;
    else hi = mid;
  }
  for (; lo < T.n && T.hash[lo] == h; lo++) {
    const int32_t r = T.idx[lo];
    DQT_CHECK(r >= 0 && r < T.n);
    const int32_t a = T.name_off[r];
    if (T.name_off[r + 1] - a != n) continue;
    bool eq = true;
    for (int32_t i = 0; i < n && eq; i++) eq = T.names[a + i] == p[i];
    if (eq) return r;
  }
  return -1;
}

}  // namespace dqt

// ------------------------------------------------------------------ host side: building the table
#include <algorithm>
#include <string>
#include <utility>
#include <vector>

namespace dqt {

struct NameTableHost {
  std::vector<uint64_t> hash;
  std::vector<int32_t> idx, name_off;
  std::vector<uint8_t> names;
  NameTable view() const {
    return NameTable{hash.data(), idx.data(), name_off.data(), names.data(), (int32_t)idx.size()};
  }
};

inline void name_table_build(const std::vector<std::string>& names, NameTableHost* T) {
  const size_t n = names.size();
  T->name_off.assign(1, 0);
  T->names.clear();
  std::vector<std::pair<uint64_t, int32_t>> key;
  for (size_t r = 0; r < n; r++) {
    T->names.insert(T->names.end(), names[r].begin(), names[r].end());
    T->name_off.push_back((int32_t)T->names.size());
    key.push_back({name_hash((const uint8_t*)names[r].data(), (int32_t)names[r].size()), (int32_t)r});
  }
  std::sort(key.begin(), key.end());
  T->hash.resize(n);
  T->idx.resize(n);
  for (size_t i = 0; i < n; i++) {
    T->hash[i] = key[i].first;
    T->idx[i] = key[i].second;
  }
  T->names.push_back(0);  // never empty
}

}  // namespace dqt
