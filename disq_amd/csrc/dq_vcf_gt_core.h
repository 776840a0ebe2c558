// dq_vcf_gt_core.h -- the per-cell rules of the VCF genotype decode: the
// FORMAT column and the sample columns of a data line, as htsjdk's
// AbstractVCFCodec.createGenotypeMap / parseGenotypeAlleles read them, into the cells of
// dq_genotype_batch.  One header for the host and the device: the kernels of dq_vcf_gt.hip, the
// library's host side and tools/vcf_gt_check.cpp compile the same functions.  One cell function
// (gt_cell) validates and produces, so the check pass and the decode pass cannot disagree.  Every
// load lies in [L + a, L + z) of the piece a function is handed.
#pragma once
#include "dq_vcf_core.h"

#ifndef DQG_CHECK  // dq_vcf_gt.hip counts a failed bound here in the bounds-checked build
#define DQG_CHECK(cond) ((void)0)
#endif

namespace dqg {

using dqt::is_digit;
using dqv::vcf_int32;

// ------------------------------------------------------------------ error classes, in check order
enum : int32_t {
  GT_OK = 0,
  GT_E_SAMPLES = 1,  // line: n_sample_cols != S
  GT_E_FORMAT = 2,   // line: column 9
  GT_E_CELL = 3,     // cell: more values than keys
  GT_E_GT = 4,
  GT_E_GQ = 5,
  GT_E_DP = 6,
};

inline const char* gt_status_name(int32_t st) {
  static const char* const names[] = {"ok", "samples", "FORMAT", "cell", "GT", "GQ", "DP"};
  return st >= 0 && st <= 6 ? names[st] : "?";
}

// dq_genotype_batch.flags (include/disq_gpu.h DQ_GT_*)
enum : uint32_t { GT_HAS_GT = 1, GT_PHASED = 2, GT_HAS_GQ = 4, GT_HAS_DP = 8, GT_FILTERED = 16 };

constexpr int32_t GT_MAX_PLOIDY = 255;
constexpr int32_t GT_MAX_ALLELE = 32767;

// The first failing (line, sample, class) as one word a minimum orders: the line index above the
// sample above the class; a line-level class (samples, FORMAT) carries sample 0.
DQT_INLINE unsigned long long gt_error_key(int64_t line, int32_t sample, int32_t st) {
  return (unsigned long long)line << 32 | (unsigned long long)(uint32_t)sample << 8 | (unsigned long long)st;
}

// ------------------------------------------------------------------ FORMAT
struct GtFormat {
  int32_t nkeys;       // ':' count + 1
  int32_t gt;          // 1: the first key is GT
  int32_t gq, dp, ft;  // the key's index, or -1
};

// Column 9 = L[a, z).  An empty column, GT anywhere but first and GT, GQ, DP or FT twice fail.
DQT_INLINE int32_t gt_format_parse(const uint8_t* L, int32_t a, int32_t z, GtFormat* F) {
  F->nkeys = 0;
  F->gt = 0;
  F->gq = F->dp = F->ft = -1;
  if (z <= a) return GT_E_FORMAT;
  int32_t k = 0;
  for (int32_t b = a;;) {
    int32_t e = b;
    while (e < z && L[e] != ':') e++;
    if (e - b == 2) {
      const uint8_t c0 = L[b], c1 = L[b + 1];
      if (c0 == 'G' && c1 == 'T') {
        if (k != 0) return GT_E_FORMAT;
        F->gt = 1;
      } else if (c0 == 'G' && c1 == 'Q') {
        if (F->gq >= 0) return GT_E_FORMAT;
        F->gq = k;
      } else if (c0 == 'D' && c1 == 'P') {
        if (F->dp >= 0) return GT_E_FORMAT;
        F->dp = k;
      } else if (c0 == 'F' && c1 == 'T') {
        if (F->ft >= 0) return GT_E_FORMAT;
        F->ft = k;
      }
    }
    k++;
    if (e >= z) break;
    b = e + 1;
  }
  F->nkeys = k;
  return GT_OK;
}

// ------------------------------------------------------------------ GQ
// The device's own GQ texts, [-+]?[0-9]{1,9}(\.[0-9]{0,6})?, rounded from the digits as Java's
// (int) Math.round(Double.valueOf(text)) rounds their binary64: text and tie point (k + 0.5) both
// have at most 15 significant digits, so the conversion to binary64, which is monotonic and maps
// decimals of up to 15 digits one to one, cannot move the text's value across the tie.
DQT_INLINE bool gt_gq_digits(const uint8_t* t, int32_t n, int32_t* v) {
  int32_t i = 0;
  bool neg = false;
  if (i < n && (t[i] == '-' || t[i] == '+')) neg = t[i++] == '-';
  int32_t ip = 0, ni = 0;
  for (; i < n && is_digit(t[i]); i++, ni++) {
    if (ni >= 9) return false;
    ip = ip * 10 + (t[i] - '0');
  }
  if (ni == 0) return false;
  int32_t nf = 0, first = 0;
  bool rest = false;  // a non-zero digit past the first fractional one
  if (i < n && t[i] == '.') {
    i++;
    for (; i < n && is_digit(t[i]); i++, nf++) {
      if (nf >= 6) return false;
      if (nf == 0) first = t[i] - '0';
      else rest |= t[i] != '0';
    }
  }
  if (i != n) return false;
  // ties go toward +infinity: up at .5 for x >= 0, down only strictly past .5 for x < 0
  *v = neg ? -ip - ((first > 5 || (first == 5 && rest)) ? 1 : 0) : ip + (first >= 5 ? 1 : 0);
  return true;
}

// Java (int) Math.round(double): the nearest integer, ties toward +infinity, clamped to int64, the
// low 32 bits kept.  The host's step after strtod for the GQ texts off the digit path.
inline int32_t gt_round_gq(double x) {
  if (x != x) return 0;
  int64_t r;
  if (x >= 9223372036854775807.0) {
    r = INT64_MAX;
  } else if (x <= -9223372036854775808.0) {
    r = INT64_MIN;
  } else {
    double f = __builtin_floor(x);
    if (x - f >= 0.5) f += 1.0;  // x - floor(x) is exact
    r = f >= 9223372036854775807.0 ? INT64_MAX : (int64_t)f;
  }
  return (int32_t)(uint32_t)(uint64_t)r;
}

// ------------------------------------------------------------------ a cell
struct GtCell {
  uint32_t flags;
  int32_t ploidy;
  int32_t gq, dp;          // -1 when missing
  int32_t gq_host;         // the GQ text is left to the host's strtod (gq = 0 until then)
  int32_t gq_at, gq_len;   // that text, as an offset from L
};

DQT_INLINE void gt_cell_blank(GtCell* C) {
  C->flags = 0;
  C->ploidy = 0;
  C->gq = C->dp = -1;
  C->gq_host = 0;
  C->gq_at = C->gq_len = 0;
}

// The sample column L[a, z) under the keys F of a line with n_alt ALT alleles.  al: nullptr, or P
// slots that take the allele indices (-1 a no-call, -2 past the ploidy).  Returns GT_OK and fills
// *C, or the class of the first failing check in the order cell, GT, GQ, DP.
DQT_INLINE int32_t gt_cell(const uint8_t* L, int32_t a, int32_t z, const GtFormat& F, int32_t n_alt,
                           int16_t* al, int32_t P, GtCell* C) {
  gt_cell_blank(C);
  DQG_CHECK(a >= 0 && a <= z);
  // the values of the keys that are read: value i belongs to key i, empty pieces kept
  int32_t gta = -1, gtz = -1, gqa = -1, gqz = -1, dpa = -1, dpz = -1, fta = -1, ftz = -1;
  int32_t k = 0;
  for (int32_t b = a, x = a;; x++) {
    if (x >= z || L[x] == ':') {
      if (k == 0 && F.gt) gta = b, gtz = x;
      if (k == F.gq) gqa = b, gqz = x;
      if (k == F.dp) dpa = b, dpz = x;
      if (k == F.ft) fta = b, ftz = x;
      k++;
      if (x >= z) break;
      b = x + 1;
    }
  }
  if (k > F.nkeys) return GT_E_CELL;
  uint32_t fl = 0;
  // ---- GT: tokens between '/', '|' and '\', empty ones dropped (StringTokenizer)
  int32_t np = 0;
  if (gta >= 0) {
    fl |= GT_HAS_GT;
    int32_t tb = gta;
    for (int32_t x = gta; x <= gtz; x++) {
      const uint8_t c = x < gtz ? L[x] : (uint8_t)'/';
      if (c != '/' && c != '|' && c != '\\') continue;
      if (c == '|' && x < gtz) fl |= GT_PHASED;
      if (x > tb) {
        int32_t v = -1;
        if (!(x - tb == 1 && L[tb] == '.')) {
          if (!vcf_int32(L + tb, x - tb, &v)) return GT_E_GT;
          if (v < 0 || v > n_alt || v > GT_MAX_ALLELE) return GT_E_GT;
        }
        if (np >= GT_MAX_PLOIDY) return GT_E_GT;
        if (al) {
          DQG_CHECK(np < P);
          if (np < P) al[np] = (int16_t)v;
        }
        np++;
      }
      tb = x + 1;
    }
  }
  if (al)
    for (int32_t i = np; i < P; i++) al[i] = -2;
  C->ploidy = np;
  // ---- GQ
  if (gqa >= 0) {
    const uint8_t* t = L + gqa;
    const int32_t n = gqz - gqa;
    if (!((n == 1 && t[0] == '.') || (n == 2 && t[0] == '-' && t[1] == '1'))) {
      int32_t v = 0;
      if (!gt_gq_digits(t, n, &v)) {
        double q;
        if (dqv::vcf_parse_qual(t, n, &q) == dqv::VCF_Q_BAD) return GT_E_GQ;
        C->gq_host = 1;
        C->gq_at = gqa;
        C->gq_len = n;
      }
      C->gq = v;
      fl |= GT_HAS_GQ;
    }
  }
  // ---- DP
  if (dpa >= 0 && !(dpz - dpa == 1 && L[dpa] == '.')) {
    int32_t v = 0;
    if (!vcf_int32(L + dpa, dpz - dpa, &v)) return GT_E_DP;
    C->dp = v;
    fl |= GT_HAS_DP;
  }
  // ---- FT: not validated
  if (fta >= 0) {
    const int32_t n = ftz - fta;
    const bool pass = n == 4 && L[fta] == 'P' && L[fta + 1] == 'A' && L[fta + 2] == 'S' && L[fta + 3] == 'S';
    if (!(n == 1 && L[fta] == '.') && !pass) fl |= GT_FILTERED;
  }
  C->flags = fl;
  return GT_OK;
}

// ------------------------------------------------------------------ a line, cell after cell
// The row of one variant in the matrix: its first cell in every array; flags == nullptr in the
// check pass, which stores nothing.
struct GtRow {
  uint8_t* flags;
  uint8_t* ploidy;
  int16_t* allele;  // P per cell
  int32_t* gq;
  int32_t* dp;
  int32_t* cell_off;
};

struct GtLine {
  int32_t st;          // GT_OK or the class of the first failing check
  int32_t sample;      // the failing cell (0 for a line-level class)
  int32_t max_ploidy;
};

// Walks the value L[0, len) of a data line from its FORMAT column at fmt_at (the byte behind the
// eighth TAB): nsc, the line's sample columns, against S; FORMAT; then the S cells left to right.
// host_gq(sample, text offset, text length) is called for every GQ text left to the host.  The way
// a thread of dq_vcf_gt.hip and the host walk a line; a wave shares the cells among its lanes.
template <typename HostGq>
DQT_INLINE GtLine gt_line_walk(const uint8_t* L, int32_t len, int32_t fmt_at, int32_t S, int32_t nsc,
                               int32_t n_alt, int32_t P, const GtRow& row, HostGq&& host_gq) {
  GtLine R{GT_OK, 0, 0};
  if (nsc != S) {
    R.st = GT_E_SAMPLES;
    return R;
  }
  DQG_CHECK(fmt_at >= 0 && fmt_at <= len);
  int32_t x = fmt_at;
  while (x < len && L[x] != '\t') x++;
  GtFormat F;
  if ((R.st = gt_format_parse(L, fmt_at, x, &F))) return R;
  for (int32_t s = 0; s < S; s++) {
    DQG_CHECK(x < len);  // nsc == S: a TAB opens every cell
    if (x >= len) break;
    const int32_t a = x + 1;
    int32_t z = a;
    while (z < len && L[z] != '\t') z++;
    GtCell C;
    const int32_t st = gt_cell(L, a, z, F, n_alt, row.flags ? row.allele + (int64_t)s * P : nullptr, P, &C);
    if (st) {
      R.st = st;
      R.sample = s;
      return R;
    }
    if (C.ploidy > R.max_ploidy) R.max_ploidy = C.ploidy;
    if (C.gq_host) host_gq(s, C.gq_at, C.gq_len);
    if (row.flags) {
      row.flags[s] = (uint8_t)C.flags;
      row.ploidy[s] = (uint8_t)C.ploidy;
      row.gq[s] = C.gq;
      row.dp[s] = C.dp;
      row.cell_off[s] = a;
    }
    x = z;
  }
  return R;
}

}  // namespace dqg

// ------------------------------------------------------------------ host side: the sample names
namespace dqg {

// The columns of the first #CHROM line among the leading '#' lines of t[0, n) behind the ninth,
// trailing empty ones dropped (Java String.split): the sample names.  Lines end as in
// dqv::vcf_header_parse.
inline void gt_header_samples(const uint8_t* t, int64_t n, std::vector<std::string>* names) {
  names->clear();
  int64_t a = (n >= 3 && t[0] == 0xEF && t[1] == 0xBB && t[2] == 0xBF) ? 3 : 0;
  while (a < n) {
    int64_t z = a;
    while (z < n && t[z] != '\n' && t[z] != '\r') z++;
    if (t[a] != '#' || z == a) return;
    if (z - a >= 6 && std::string((const char*)t + a, 6) == "#CHROM") {
      int col = 0;
      for (int64_t b = a;; col++) {
        int64_t e = b;
        while (e < z && t[e] != '\t') e++;
        if (col >= 9) names->push_back(std::string((const char*)t + b, (size_t)(e - b)));
        if (e >= z) break;
        b = e + 1;
      }
      while (!names->empty() && names->back().empty()) names->pop_back();
      return;
    }
    if (z >= n) return;
    a = (t[z] == '\r' && z + 1 < n && t[z + 1] == '\n') ? z + 2 : z + 1;
  }
}

}  // namespace dqg
