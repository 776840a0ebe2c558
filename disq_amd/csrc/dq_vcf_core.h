// dq_vcf_core.h -- the per-line rules of the VCF site decode: the eight
// columns htsjdk's AbstractVCFCodec.parseVCFLine reads eagerly, as the fields of dq_variant_batch.
// One header for the host and the device: the kernels of dq_vcf.hip, the library's host side and
// tools/vcf_core_check.cpp compile the same functions.  One walk (vcf_line_walk) validates and
// produces, so the validate pass and the decode pass cannot disagree.  Every load of a line lies in
// [L, L + len).
#pragma once
#include "dq_text_core.h"

#ifndef DQV_CHECK  // dq_vcf.hip counts a failed bound here in the bounds-checked build
#define DQV_CHECK(cond) ((void)0)
#endif

namespace dqv {

using dqt::is_digit;
using dqt::NameTable;  // the ##contig IDs, by contig index

// ------------------------------------------------------------------ error classes, in check order
enum : int32_t {
  VCF_OK = 0,
  VCF_E_FIELDS = 1,
  VCF_E_CHROM = 2,
  VCF_E_POS = 3,
  VCF_E_ID = 4,
  VCF_E_REF = 5,
  VCF_E_ALT = 6,
  VCF_E_QUAL = 7,
  VCF_E_FILTER = 8,
  VCF_E_INFO = 9,
};

inline const char* vcf_status_name(int32_t st) {
  static const char* const names[] = {"ok",  "fields", "CHROM",  "POS", "ID",
                                      "REF", "ALT",    "QUAL",   "FILTER", "INFO"};
  return st >= 0 && st <= 9 ? names[st] : "?";
}

// dq_variant_batch.flags (include/disq_gpu.h DQ_VCF_*)
enum : uint32_t {
  VCF_HAS_ID = 1,
  VCF_HAS_QUAL = 2,
  VCF_UNFILTERED = 4,
  VCF_PASS = 8,
  VCF_INFO_END = 16,
  VCF_HAS_GENOTYPES = 32,
  VCF_SYMBOLIC = 64,
  VCF_REF_LOWER = 128,
};

// ------------------------------------------------------------------ small predicates
DQT_INLINE bool vcf_base(uint8_t c) {  // ACGTNacgtn
  const uint8_t u = c & 0xDF;
  return (c >= 'A') && (u == 'A' || u == 'C' || u == 'G' || u == 'T' || u == 'N');
}
DQT_INLINE uint8_t vcf_fold(uint8_t c) { return (c >= 'a' && c <= 'z') ? (uint8_t)(c - 32) : c; }
DQT_INLINE bool vcf_same_nocase(const uint8_t* a, int32_t na, const uint8_t* b, int32_t nb) {
  if (na != nb) return false;
  for (int32_t i = 0; i < na; i++)
    if (vcf_fold(a[i]) != vcf_fold(b[i])) return false;
  return true;
}

// Java Integer.valueOf: [-+]?[0-9]+ with a value in int32.
DQT_INLINE bool vcf_int32(const uint8_t* t, int32_t n, int32_t* v) {
  int64_t x;
  if (!dqt::parse_dec(t, n, true, -2147483648ll, 2147483647ll, &x)) return false;
  *v = (int32_t)x;
  return true;
}

// ------------------------------------------------------------------ QUAL
enum : int { VCF_Q_OK = 0, VCF_Q_UNDECIDED = 1, VCF_Q_BAD = 2 };

DQT_INLINE double vcf_pow10(int e) {  // 10^e, 0 <= e <= 22: every one a binary64 exactly
  const double t[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                        1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
  return t[e];
}

// [-+]?([0-9]+\.?[0-9]*|\.[0-9]+)([eE][-+]?[0-9]+)? -- VCF_Q_BAD otherwise.  The exact fast path:
// a text with an integer digit, at most 15 significant digits (an integer below 2^53; zeros may
// follow them) and a decimal exponent of that integer in -22..22, so one
// IEEE multiply or divide of two exact operands rounds correctly; a zero mantissa is zero whatever
// the exponent.  Every other text is VCF_Q_UNDECIDED (*v = 0): the host converts it with strtod.
DQT_INLINE int vcf_parse_qual(const uint8_t* t, int32_t n, double* v) {
  *v = 0.0;
  int32_t i = 0;
  bool neg = false;
  if (i < n && (t[i] == '-' || t[i] == '+')) neg = t[i++] == '-';
  uint64_t m = 0;
  int32_t nsig = 0, drop = 0, nint = 0, nfrac = 0;
  int64_t e10 = 0;
  bool more = false;  // a non-zero digit past the 15th significant one
  for (; i < n && is_digit(t[i]); i++, nint++) {
    const int d = t[i] - '0';
    if (nsig == 0 && d == 0) continue;
    if (nsig < 15) {
      m = m * 10 + (uint64_t)d;
      nsig++;
    } else {
      if (d) more = true;
      if (drop < (1 << 20)) drop++;  // integer digits left out scale the value up
    }
  }
  if (i < n && t[i] == '.') {
    i++;
    for (; i < n && is_digit(t[i]); i++, nfrac++) {
      const int d = t[i] - '0';
      if (nsig == 0 && d == 0) {
        if (e10 > -(1 << 20)) e10--;
        continue;
      }
      if (nsig < 15) {
        m = m * 10 + (uint64_t)d;
        nsig++;
        if (e10 > -(1 << 20)) e10--;
      } else if (d) {
        more = true;
      }
    }
    if (nint == 0 && nfrac == 0) return VCF_Q_BAD;
  } else if (nint == 0) {
    return VCF_Q_BAD;
  }
  e10 += drop;
  if (i < n && (t[i] == 'e' || t[i] == 'E')) {
    i++;
    bool eneg = false;
    if (i < n && (t[i] == '-' || t[i] == '+')) eneg = t[i++] == '-';
    if (i >= n || !is_digit(t[i])) return VCF_Q_BAD;
    int64_t ex = 0;
    for (; i < n && is_digit(t[i]); i++)
      if (ex < (1 << 20)) ex = ex * 10 + (t[i] - '0');
    e10 += eneg ? -ex : ex;
  }
  if (i != n) return VCF_Q_BAD;
  if (more || nint == 0) return VCF_Q_UNDECIDED;  // the ".5" form is the host's as well
  double r;
  if (m == 0) {
    r = 0.0;
  } else if (e10 >= 0 && e10 <= 22) {
    r = (double)m * vcf_pow10((int)e10);
  } else if (e10 < 0 && e10 >= -22) {
    r = (double)m / vcf_pow10((int)-e10);
  } else {
    return VCF_Q_UNDECIDED;
  }
  *v = neg ? -r : r;
  return VCF_Q_OK;
}

// ------------------------------------------------------------------ the line walk
// The positions of a line's first eight TABs (n of them, at most 8) and, when counted, the number
// of all its TABs.  A wave finds them together for a long line; a thread finds its own.
struct VcfTabs {
  int32_t at[8];
  int32_t n;
  int32_t total;  // all TABs of the line, or -1 when not counted
};

struct VcfSite {
  int32_t contig, pos, end;
  uint32_t flags;
  double qual;         // 0 when missing or undecided
  int32_t col_end[8];  // column c = [c ? col_end[c - 1] + 1 : 0, col_end[c])
  int32_t n_alt, n_filter, n_info, n_sample_cols;
  int32_t qual_undecided;  // the QUAL text is left to the host's strtod
};

// Walks the value L[0, len) of a data line.  G: the header names a sample.  tabs: the TAB list a
// wave made, or nullptr (the walk finds them; it counts the TABs past the eighth only when S is
// wanted in full, want_cols).  Returns VCF_OK and fills *S, or the class of the first failing check.
DQT_INLINE int32_t vcf_line_walk(const uint8_t* L, int32_t len, bool G, const NameTable& C,
                                 const VcfTabs* tabs, bool want_cols, VcfSite* S) {
  VcfTabs own;
  if (!tabs) {
    own.n = 0;
    own.total = -1;
    int32_t x = 0;
    for (; x < len && own.n < 8; x++) {
      DQV_CHECK(x >= 0 && x < len);
      if (L[x] == '\t') {
#pragma unroll
        for (int c = 0; c < 8; c++)  // compile-time indices keep the list in registers
          if (c == own.n) own.at[c] = x;
        own.n++;
      }
    }
    if (want_cols && G && own.n == 8) {
      int32_t t = 8;
      for (; x < len; x++) t += L[x] == '\t';
      own.total = t;
    }
    tabs = &own;
  }
  // ---- fields
  if (G ? tabs->n < 8 : tabs->n != 7) return VCF_E_FIELDS;
  int32_t ce[8];
#pragma unroll
  for (int c = 0; c < 7; c++) ce[c] = tabs->at[c];
  ce[7] = G ? tabs->at[7] : len;
  DQV_CHECK(ce[0] >= 0 && ce[7] <= len);
#pragma unroll
  for (int c = 0; c < 8; c++) S->col_end[c] = ce[c];
  uint32_t fl = G ? (uint32_t)VCF_HAS_GENOTYPES : 0u;
  S->n_sample_cols = G ? (tabs->total >= 8 ? tabs->total - 8 : 0) : 0;
  // ---- CHROM
  if (ce[0] == 0) return VCF_E_CHROM;
  S->contig = C.n > 0 ? dqt::name_lookup(C, L, ce[0]) : -1;  // no ##contig lines: no hash either
  // ---- POS
  int32_t pos = 0;
  if (!vcf_int32(L + ce[0] + 1, ce[1] - ce[0] - 1, &pos)) return VCF_E_POS;
  S->pos = pos;
  // ---- ID
  {
    const int32_t a = ce[1] + 1, n = ce[2] - a;
    if (n == 0) return VCF_E_ID;
    if (!(n == 1 && L[a] == '.')) fl |= VCF_HAS_ID;
  }
  // ---- REF
  const int32_t ra = ce[2] + 1, rn = ce[3] - ra;
  if (rn == 0) return VCF_E_REF;
  for (int32_t i = 0; i < rn; i++) {
    const uint8_t c = L[ra + i];
    if (!vcf_base(c)) return VCF_E_REF;
    if (c >= 'a') fl |= VCF_REF_LOWER;
  }
  // ---- ALT
  {
    const int32_t a0 = ce[3] + 1, z = ce[4];
    int32_t na = 0;
    if (!(z - a0 == 1 && L[a0] == '.')) {
      int32_t a = a0;
      for (;;) {
        int32_t e = a;
        bool brk = false, bases = true;
        for (; e < z && L[e] != ','; e++) {
          const uint8_t c = L[e];
          brk |= c == '[' || c == ']';
          bases &= vcf_base(c);
        }
        const int32_t n = e - a;
        if (n == 0) return VCF_E_ALT;
        const bool sym = (L[a] == '<' && L[e - 1] == '>') || brk;
        if (!(sym || bases || (n == 1 && L[a] == '*'))) return VCF_E_ALT;
        if (sym) fl |= VCF_SYMBOLIC;
        if (vcf_same_nocase(L + a, n, L + ra, rn)) return VCF_E_ALT;  // "Duplicate allele"
        for (int32_t b = a0; b < a;) {  // the earlier pieces
          int32_t be = b;
          while (L[be] != ',') be++;  // ends before a: a piece's ',' precedes it
          if (vcf_same_nocase(L + a, n, L + b, be - b)) return VCF_E_ALT;
          b = be + 1;
        }
        na++;
        if (e >= z) break;
        a = e + 1;
        if (a >= z) return VCF_E_ALT;  // a trailing ',': an empty last piece
      }
    }
    S->n_alt = na;
  }
  // ---- QUAL
  {
    const int32_t a = ce[4] + 1, n = ce[5] - a;
    S->qual = 0.0;
    S->qual_undecided = 0;
    if (!(n == 1 && L[a] == '.')) {
      double q;
      const int r = vcf_parse_qual(L + a, n, &q);
      if (r == VCF_Q_BAD) return VCF_E_QUAL;
      fl |= VCF_HAS_QUAL;
      S->qual = q;
      S->qual_undecided = r == VCF_Q_UNDECIDED;
    }
  }
  // ---- FILTER
  {
    const int32_t a = ce[5] + 1, z = ce[6], n = z - a;
    int32_t nf = 0;
    if (n == 0) return VCF_E_FILTER;
    if (n == 1 && L[a] == '0') return VCF_E_FILTER;
    if (n == 1 && L[a] == '.') {
      fl |= VCF_UNFILTERED;
    } else if (n == 4 && L[a] == 'P' && L[a + 1] == 'A' && L[a + 2] == 'S' && L[a + 3] == 'S') {
      fl |= VCF_PASS;
    } else {
      for (int32_t b = a;;) {
        int32_t e = b;
        while (e < z && L[e] != ';') e++;
        if (e - b == 4 && L[b] == 'P' && L[b + 1] == 'A' && L[b + 2] == 'S' && L[b + 3] == 'S')
          return VCF_E_FILTER;
        nf++;
        if (e >= z) break;
        b = e + 1;
      }
    }
    S->n_filter = nf;
  }
  // ---- INFO
  int64_t end = (int64_t)pos + rn - 1;
  {
    const int32_t a = ce[6] + 1, z = ce[7], n = z - a;
    if (n == 0) return VCF_E_INFO;
    for (int32_t i = a; i < z; i++)
      if (L[i] == ' ') return VCF_E_INFO;
    int32_t ni = 0;
    if (!(n == 1 && L[a] == '.')) {
      bool seen = false;
      for (int32_t b = a;;) {
        int32_t e = b;
        while (e < z && L[e] != ';') e++;
        ni++;
        // key END: the piece is "END" or starts with "END="
        if (!seen && e - b >= 3 && L[b] == 'E' && L[b + 1] == 'N' && L[b + 2] == 'D' &&
            (e - b == 3 || L[b + 3] == '=')) {
          seen = true;
          int32_t ev = 0;
          if (e - b == 3 || !vcf_int32(L + b + 4, e - b - 4, &ev)) return VCF_E_INFO;
          end = ev;
          fl |= VCF_INFO_END;
        }
        if (e >= z) break;
        b = e + 1;
      }
    }
    S->n_info = ni;
  }
  S->end = (int32_t)(uint32_t)(uint64_t)end;  // Java int arithmetic: wraps past 2^31 - 1
  S->flags = fl;
  return VCF_OK;
}

// ------------------------------------------------------------------ host side: the header
struct VcfHeader {
  bool has_chrom = false;  // a #CHROM line was seen
  bool has_data = false;   // a line that does not start with '#' follows the header
  bool G = false;          // the #CHROM line names a sample: a non-empty tenth column
  std::vector<std::string> contigs;  // the IDs of the ##contig lines, in order
};

// The leading '#' lines of t[0, n) (LF, CR LF or a lone CR end a line; a UTF-8 BOM is dropped).
// whole: t is the whole stream.  Returns 1 when the header may run past a prefix, else 0.
inline int vcf_header_parse(const uint8_t* t, int64_t n, bool whole, VcfHeader* H) {
  *H = VcfHeader{};
  int64_t a = (n >= 3 && t[0] == 0xEF && t[1] == 0xBB && t[2] == 0xBF) ? 3 : 0;
  while (a < n) {
    int64_t z = a;
    while (z < n && t[z] != '\n' && t[z] != '\r') z++;
    if (z >= n && !whole) return 1;  // the line may go on
    if (t[a] != '#' || z == a) {
      H->has_data = true;
      return 0;
    }
    const std::string line((const char*)t + a, (size_t)(z - a));
    if (line.compare(0, 6, "#CHROM") == 0 && !H->has_chrom) {
      H->has_chrom = true;
      int col = 0;
      size_t b = 0;
      for (;;) {
        const size_t e = line.find('\t', b);
        const size_t ce = e == std::string::npos ? line.size() : e;
        if (col == 9 && ce > b) H->G = true;
        if (e == std::string::npos) break;
        b = e + 1;
        col++;
      }
    } else if (line.compare(0, 10, "##contig=<") == 0) {
      size_t end = line.rfind('>');
      if (end == std::string::npos || end < 10) end = line.size();
      std::string id;
      bool found = false;
      for (size_t b = 10; b <= end && !found;) {
        size_t e = line.find(',', b);
        if (e == std::string::npos || e > end) e = end;
        if (e - b >= 3 && line.compare(b, 3, "ID=") == 0) {
          id = line.substr(b + 3, e - b - 3);
          found = true;
        }
        b = e + 1;
      }
      if (found) H->contigs.push_back(id);
    }
    if (z >= n) break;
    a = (t[z] == '\r' && z + 1 < n && t[z + 1] == '\n') ? z + 2 : z + 1;
    if (t[z] == '\r' && z + 1 >= n && !whole) return 1;
  }
  if (!whole) return 1;  // only '#' lines so far
  return 0;
}

}  // namespace dqv
