// dq_sam_core.h -- the per-line rules of the SAM text path: one SAM line
// into one BAM record as htsjdk SAMLineParser.parseLine + BAMRecordCodec.encode + BinaryTagCodec
// do it, restated by tests/samutil.py (sam_line_to_bam_record), whose order of checks this keeps so
// that the first error of a line is the same one.  The kernels of dq_sam.hip and the host program
// tools/sam_core_check.cpp compile the same functions.  The @SQ names are a dqt::NameTable, the
// integer columns dqt::parse_dec (dq_text_core.h, which also holds the __HIPCC__ guards).
//
// One walk serves both passes: with out == nullptr it validates and sizes the record, with out set
// it writes the bytes; so the size a record was given and the bytes it gets cannot disagree.
#pragma once
#include <stdint.h>

#include "dq_sam_pow5.h"
#include "dq_text_core.h"

#ifndef DQS_CHECK  // dq_sam.hip counts a failed bound here in the bounds-checked build
#define DQS_CHECK(cond) ((void)0)
#endif

namespace dqs {

using dqt::is_digit;
using dqt::NameTable;  // the @SQ names, by reference index
using dqt::parse_dec;

// Line status: 0, a column (the spelling of samutil.SamError.what is sam_status_name's), or
// SAM_E_TAG | (bytes of the tag name present, 0..2) << 16 | name[0] << 8 | name[1].
enum : int32_t {
  SAM_OK = 0,
  SAM_E_FIELDS = 1,
  SAM_E_QNAME = 2,
  SAM_E_FLAG = 3,
  SAM_E_RNAME = 4,
  SAM_E_POS = 5,
  SAM_E_MAPQ = 6,
  SAM_E_CIGAR = 7,
  SAM_E_RNEXT = 8,
  SAM_E_PNEXT = 9,
  SAM_E_TLEN = 10,
  SAM_E_SEQ = 11,
  SAM_E_QUAL = 12,
  SAM_E_TAG = 1 << 24,
};

// Host: "fields", "QNAME", ..., "tag XX" into buf (>= 8 bytes).
inline const char* sam_status_name(int32_t st, char* buf) {
  static const char* const col[] = {"ok",    "fields", "QNAME", "FLAG", "RNAME", "POS", "MAPQ",
                                    "CIGAR", "RNEXT",  "PNEXT", "TLEN", "SEQ",   "QUAL"};
  if (st >= 0 && st <= SAM_E_QUAL) return col[st];
  const int k = (st >> 16) & 3;
  buf[0] = 't';
  buf[1] = 'a';
  buf[2] = 'g';
  buf[3] = ' ';
  if (k > 0) buf[4] = (char)((st >> 8) & 0xff);
  if (k > 1) buf[5] = (char)(st & 0xff);
  buf[4 + k] = 0;
  return buf;
}

DQT_INLINE int32_t sam_tag_error(const uint8_t* f, int32_t n) {
  const int32_t k = n < 2 ? n : 2;
  return SAM_E_TAG | (k << 16) | ((k > 0 ? (int32_t)f[0] : 0) << 8) | (k > 1 ? (int32_t)f[1] : 0);
}

// ------------------------------------------------------------------ numbers
DQT_INLINE void sam_mul64(uint64_t a, uint64_t b, uint64_t* hi, uint64_t* lo) {
#if defined(__HIP_DEVICE_COMPILE__)
  *lo = a * b;
  *hi = __umul64hi(a, b);
#else
  const unsigned __int128 p = (unsigned __int128)a * b;
  *lo = (uint64_t)p;
  *hi = (uint64_t)(p >> 64);
#endif
}

enum : int { SAM_F_OK = 0, SAM_F_UNDECIDED = 1, SAM_F_BAD = 2 };

// A float text [-+]?[0-9]*\.?[0-9]+([eE][-+]?[0-9]+)? into the correctly rounded binary32 (round
// to nearest even, as strtof and Float.parseFloat): up to 19 significant digits w and the decimal
// exponent q, then the Eisel-Lemire conversion (D. Lemire, "Number parsing at a gigabyte per
// second", 2021): w * 5^q from a 64 x 64 -> 128 bit product against the normalised 128-bit power
// of five, refined by the low half when the first product leaves the rounding open.
// SAM_F_UNDECIDED (bits = 0): non-zero digits past the 19th, or a product that cannot tell which
// side of a rounding boundary the value lies on; the caller converts those texts with strtof.
DQT_INLINE int sam_parse_float(const uint8_t* t, int32_t n, uint32_t* bits) {
  static constexpr uint64_t POW5[DQ_SAM_POW5_QMAX - DQ_SAM_POW5_QMIN + 1][2] = {DQ_SAM_POW5_TABLE};
  *bits = 0;
  int32_t i = 0;
  bool neg = false;
  if (i < n && (t[i] == '-' || t[i] == '+')) neg = t[i++] == '-';
  uint64_t w = 0;
  int nd = 0;          // significant digits taken into w
  int64_t q = 0;       // value = w * 10^q (+ the dropped digits)
  bool dropped = false;
  int32_t ni = 0, nf = 0;
  for (; i < n && is_digit(t[i]); i++, ni++) {
    const uint32_t d = t[i] - '0';
    if (nd == 0 && d == 0) continue;  // leading zeros
    if (nd < 19) {
      w = w * 10 + d;
      nd++;
    } else {
      dropped |= d != 0;
      q++;
    }
  }
  const bool dot = i < n && t[i] == '.';
  if (dot) {
    for (i++; i < n && is_digit(t[i]); i++, nf++) {
      const uint32_t d = t[i] - '0';
      if (nd < 19) {
        w = w * 10 + d;
        if (nd > 0 || d) nd++;
        q--;
      } else {
        dropped |= d != 0;
      }
    }
  }
  if (nf == 0 && (dot || ni == 0)) return SAM_F_BAD;
  if (i < n && (t[i] == 'e' || t[i] == 'E')) {
    i++;
    bool eneg = false;
    if (i < n && (t[i] == '-' || t[i] == '+')) eneg = t[i++] == '-';
    int64_t x = 0;
    int32_t nx = 0;
    for (; i < n && is_digit(t[i]); i++, nx++)
      if (x < 1000000) x = x * 10 + (t[i] - '0');
    if (nx == 0) return SAM_F_BAD;
    q += eneg ? -x : x;
  }
  if (i != n) return SAM_F_BAD;
  const uint32_t sign = neg ? 0x80000000u : 0u;
  *bits = sign;
  if (w == 0) return SAM_F_OK;  // +-0
  if (dropped) {
    *bits = 0;
    return SAM_F_UNDECIDED;
  }
  // w < 10^19: below 10^-64 the value is under half the smallest subnormal (2^-150), above 10^38
  // over the largest finite binary32
  if (q < DQ_SAM_POW5_QMIN) return SAM_F_OK;
  if (q > DQ_SAM_POW5_QMAX) {
    *bits = sign | 0x7f800000u;
    return SAM_F_OK;
  }
  int lz = __builtin_clzll(w);
  w <<= lz;
  const uint64_t* P = POW5[q - DQ_SAM_POW5_QMIN];
  uint64_t hi, lo;
  sam_mul64(w, P[0], &hi, &lo);
  // 23 + 3 bits are needed; when the bits below them are all ones the truncated low half of the
  // power could still carry into them
  if ((hi & (~0ull >> 26)) == (~0ull >> 26)) {
    uint64_t hi2, lo2;
    sam_mul64(w, P[1], &hi2, &lo2);
    lo += hi2;
    if (hi2 > lo) hi++;
    if (lo == ~0ull && (q < -27 || q > 55)) {  // still open: the ambiguous case
      *bits = 0;
      return SAM_F_UNDECIDED;
    }
  }
  const int upper = (int)(hi >> 63);
  uint64_t m = hi >> (upper + 64 - 23 - 3);
  // floor(log2(5^q)) + q + 63 = ((152170 + 65536) * q >> 16) + 63; binary32's minimum exponent -127
  int32_t p2 = (int32_t)(((217706 * q) >> 16) + 63) + upper - lz + 127;
  if (p2 <= 0) {  // subnormal (or zero)
    if (-p2 + 1 >= 64) return SAM_F_OK;
    m >>= -p2 + 1;
    m += m & 1;
    m >>= 1;
    *bits = sign | (uint32_t)m;  // m == 2^23 is the smallest normal: the same bits
    return SAM_F_OK;
  }
  // exactly half way between two floats: only when 5^q fits the 64-bit multiplication
  if (lo <= 1 && q >= -17 && q <= 10 && (m & 3) == 1 && (m << (upper + 64 - 23 - 3)) == hi) m &= ~1ull;
  m += m & 1;
  m >>= 1;
  if (m >= (2ull << 23)) {
    m = 1ull << 23;
    p2++;
  }
  m &= ~(1ull << 23);
  if (p2 >= 0xff) {
    *bits = sign | 0x7f800000u;
    return SAM_F_OK;
  }
  *bits = sign | ((uint32_t)p2 << 23) | (uint32_t)m;
  return SAM_F_OK;
}

// ------------------------------------------------------------------ the line walk
DQT_INLINE int sam_seq_code(uint8_t c) {  // =ACMGRSVTWYHKDBN in either case, '.' as N; else -1
  if (c == '.') return 15;
  if (c >= 'a' && c <= 'z') c = (uint8_t)(c - 32);
  switch (c) {
    case '=': return 0;
    case 'A': return 1;
    case 'C': return 2;
    case 'M': return 3;
    case 'G': return 4;
    case 'R': return 5;
    case 'S': return 6;
    case 'V': return 7;
    case 'T': return 8;
    case 'W': return 9;
    case 'Y': return 10;
    case 'H': return 11;
    case 'K': return 12;
    case 'D': return 13;
    case 'B': return 14;
    case 'N': return 15;
    default: return -1;
  }
}

DQT_INLINE int sam_cigar_code(uint8_t c) {  // MIDNSHP=X
  switch (c) {
    case 'M': return 0;
    case 'I': return 1;
    case 'D': return 2;
    case 'N': return 3;
    case 'S': return 4;
    case 'H': return 5;
    case 'P': return 6;
    case '=': return 7;
    case 'X': return 8;
    default: return -1;
  }
}

DQT_INLINE int32_t sam_reg2bin(int32_t beg, int32_t end) {
  end -= 1;
  if (beg >> 14 == end >> 14) return 4681 + (beg >> 14);
  if (beg >> 17 == end >> 17) return 585 + (beg >> 17);
  if (beg >> 20 == end >> 20) return 73 + (beg >> 20);
  if (beg >> 23 == end >> 23) return 9 + (beg >> 23);
  if (beg >> 26 == end >> 26) return 1 + (beg >> 26);
  return 0;
}

struct SamLineInfo {
  int32_t size;  // 4 + block_size
  int32_t ref_id, pos, l_seq, next_ref_id, next_pos, tlen;
  uint16_t flag, bin, n_cigar;
  uint8_t mapq, l_read_name;
  int32_t seq_off, qual_off;  // SEQ and QUAL in the line (qual_off -1: QUAL is '*')
  int32_t seq_out, qual_out;  // packed SEQ and QUAL in the record
  int32_t n_undecided;        // float texts sam_parse_float left to the host
};

// Where an encode reports the floats it could not decide: 3 words per entry (byte offset of the
// 4-byte slot, offset of the text, its length), each made absolute by out_base / text_base.
struct SamFixSink {
  int64_t* ent;
  unsigned long long* cnt;
  int64_t cap;
  int64_t out_base, text_base;
};

struct SamOut {  // a counting or writing byte sink; nothing is stored at or past lim
  uint8_t* p;
  int32_t o;
  int32_t lim;
  DQT_INLINE void put8(uint32_t v) {
    if (p) {
      DQS_CHECK(o < lim);
      if (o < lim) p[o] = (uint8_t)v;
    }
    o++;
  }
  DQT_INLINE void put16(uint32_t v) {
    put8(v);
    put8(v >> 8);
  }
  DQT_INLINE void put32(uint32_t v) {
    put16(v);
    put16(v >> 16);
  }
  // whole little-endian words: one store each (the alignment is the record's, arbitrary)
  DQT_INLINE void put_w32(uint32_t v) {
    if (p) {
      DQS_CHECK(o + 4 <= lim);
      if (o + 4 <= lim) __builtin_memcpy(p + o, &v, 4);
    }
    o += 4;
  }
  DQT_INLINE void put_w64(uint64_t v) {
    if (p) {
      DQS_CHECK(o + 8 <= lim);
      if (o + 8 <= lim) __builtin_memcpy(p + o, &v, 8);
    }
    o += 8;
  }
};

// Eight bases at src (one 8-byte load) -> their four packed bytes as a little-endian word; false
// when one of them is no base.
DQT_INLINE bool sam_pack8(const uint8_t* src, uint32_t* pk) {
  uint64_t w;
  __builtin_memcpy(&w, src, 8);
  uint32_t v = 0;
  bool ok = true;
#pragma unroll
  for (int b = 0; b < 8; b++) {
    const int c = sam_seq_code((uint8_t)(w >> (8 * b)));
    ok &= c >= 0;
    v |= (uint32_t)(c & 15) << (8 * (b >> 1) + ((b & 1) ? 0 : 4));
  }
  *pk = v;
  return ok;
}

// Eight quality bytes at src minus 33 each; false when one of them is below 33.
DQT_INLINE bool sam_qual8(const uint8_t* src, uint64_t* out) {
  uint64_t w;
  __builtin_memcpy(&w, src, 8);
  uint64_t v = 0;
  bool ok = true;
#pragma unroll
  for (int b = 0; b < 8; b++) {
    const uint32_t c = (uint32_t)(w >> (8 * b)) & 0xff;
    ok &= c >= 33;
    v |= (uint64_t)((c - 33) & 0xff) << (8 * b);
  }
  *out = v;
  return ok;
}

DQT_INLINE void sam_poke32(uint8_t* p, int32_t o, uint32_t v) {
  p[o] = (uint8_t)v;
  p[o + 1] = (uint8_t)(v >> 8);
  p[o + 2] = (uint8_t)(v >> 16);
  p[o + 3] = (uint8_t)(v >> 24);
}

// One float value of a tag: validated, sized, written (a zero and a fix-up entry when undecided).
DQT_INLINE bool sam_put_float(const uint8_t* L, int32_t a, int32_t n, SamOut& O, SamLineInfo* I,
                              const SamFixSink* fx) {
  uint32_t bits;
  const int r = sam_parse_float(L + a, n, &bits);
  if (r == SAM_F_BAD) return false;
  if (r == SAM_F_UNDECIDED) {
    I->n_undecided++;
    if (O.p && fx) {
#if defined(__HIP_DEVICE_COMPILE__)
      const int64_t slot = (int64_t)atomicAdd(fx->cnt, 1ull);
#else
      const int64_t slot = (int64_t)(*fx->cnt)++;
#endif
      DQS_CHECK(slot < fx->cap);
      if (slot < fx->cap) {
        fx->ent[3 * slot] = fx->out_base + O.o;
        fx->ent[3 * slot + 1] = fx->text_base + a;
        fx->ent[3 * slot + 2] = n;
      }
    }
  }
  O.put32(bits);
  return true;
}

// The walk.  out == nullptr: validate and size; else write the record's I->size bytes, none of them
// at or past out + out_cap (the size the size pass gave).  bulk:
// SEQ's and QUAL's bytes are checked and written here; without it the caller does both from
// I->seq_off / qual_off / seq_out / qual_out (a wave per long line), and a status of SAM_OK or a
// tag error is then final only once the caller has found no SEQ or QUAL byte error, which rank
// before the tags.
// tabs: the positions of the line's first 11 TABs, all of them when it has fewer (a wave that found
// them together hands them in; with nullptr the walk looks for them itself).
struct SamTabs {
  int32_t at[11];
  int32_t n;
};

DQT_INLINE int32_t sam_line_walk(const uint8_t* L, int32_t len, const NameTable& R, uint8_t* out,
                                 int32_t out_cap, SamLineInfo* I, const SamFixSink* fx, bool bulk,
                                 const SamTabs* tabs = nullptr) {
  *I = SamLineInfo{};
  I->qual_off = -1;
  // ---- the eleven mandatory columns
  int32_t fs[11], fe[11];
  int32_t p = 0;
#pragma unroll
  for (int c = 0; c < 11; c++) {
    fs[c] = p;
    if (tabs) {
      p = c < tabs->n ? tabs->at[c] : len;
    } else {
      while (p < len && L[p] != '\t') p++;
    }
    fe[c] = p;
    if (c < 10) {
      if (p >= len) return SAM_E_FIELDS;
      p++;
    }
  }
  const int32_t tags_at = fe[10];
  const int32_t lname = fe[0] - fs[0];
  if (lname < 1 || lname > 254) return SAM_E_QNAME;
  int64_t v;
  if (!parse_dec(L + fs[1], fe[1] - fs[1], false, 0, 65535, &v)) return SAM_E_FLAG;
  const int32_t flag = (int32_t)v;
  int32_t ref = -1;
  if (!(fe[2] - fs[2] == 1 && L[fs[2]] == '*')) {
    ref = dqt::name_lookup(R, L + fs[2], fe[2] - fs[2]);
    if (ref < 0) return SAM_E_RNAME;
  }
  if (!parse_dec(L + fs[3], fe[3] - fs[3], false, 0, 2147483647ll, &v)) return SAM_E_POS;
  const int32_t beg = (int32_t)(v - 1);
  if (!parse_dec(L + fs[4], fe[4] - fs[4], false, 0, 255, &v)) return SAM_E_MAPQ;
  const int32_t mapq = (int32_t)v;
  int32_t nref = -1;
  if (fe[6] - fs[6] == 1 && L[fs[6]] == '=') {
    nref = ref;
  } else if (!(fe[6] - fs[6] == 1 && L[fs[6]] == '*')) {
    nref = dqt::name_lookup(R, L + fs[6], fe[6] - fs[6]);
    if (nref < 0) return SAM_E_RNEXT;
  }
  if (!parse_dec(L + fs[7], fe[7] - fs[7], false, 0, 2147483647ll, &v)) return SAM_E_PNEXT;
  const int32_t npos = (int32_t)(v - 1);
  if (!parse_dec(L + fs[8], fe[8] - fs[8], true, -2147483648ll, 2147483647ll, &v)) return SAM_E_TLEN;
  const int32_t tlen = (int32_t)v;
  const bool seq_star = fe[9] - fs[9] == 1 && L[fs[9]] == '*';
  const bool qual_star = fe[10] - fs[10] == 1 && L[fs[10]] == '*';
  const int32_t l_seq = seq_star ? 0 : fe[9] - fs[9];
  if (!seq_star && l_seq < 1) return SAM_E_SEQ;
  if (!qual_star && fe[10] - fs[10] != l_seq) return SAM_E_QUAL;
  // ---- CIGAR: (<digits><op>)+, op in MIDNSHP=X, 1 <= len < 2^28 in at most 10 digits
  SamOut O{out, 36, out_cap};
  for (int32_t i = fs[0]; i < fe[0]; i++) O.put8(L[i]);
  O.put8(0);
  int32_t ncig = 0;
  int64_t reflen = 0;
  if (!(fe[5] - fs[5] == 1 && L[fs[5]] == '*')) {
    int32_t x = fs[5];
    if (x >= fe[5]) return SAM_E_CIGAR;
    while (x < fe[5]) {
      int64_t n = 0;
      int32_t nd = 0;
      for (; x < fe[5] && is_digit(L[x]); x++, nd++)
        if (nd < 11) n = n * 10 + (L[x] - '0');
      if (nd == 0 || x >= fe[5]) return SAM_E_CIGAR;
      const int k = sam_cigar_code(L[x++]);
      if (k < 0 || nd > 10 || n < 1 || n > (1 << 28) - 1) return SAM_E_CIGAR;
      if (k == 0 || k == 2 || k == 3 || k == 7 || k == 8) reflen += n;
      O.put32((uint32_t)n << 4 | (uint32_t)k);
      ncig++;
    }
    if (ncig > 65535) return SAM_E_CIGAR;
  }
  I->seq_off = fs[9];
  I->qual_off = qual_star ? -1 : fs[10];
  I->seq_out = O.o;
  I->qual_out = O.o + (l_seq + 1) / 2;
  I->l_seq = l_seq;
  // ---- SEQ (4-bit codes, high nibble first) and QUAL (minus 33, or 0xFF throughout)
  if (bulk) {  // eight bytes of the line per load, whole words per store; the tails by bytes
    int32_t i = 0;
    for (; i + 8 <= l_seq; i += 8) {
      uint32_t pk;
      if (!sam_pack8(L + fs[9] + i, &pk)) return SAM_E_SEQ;
      O.put_w32(pk);
    }
    for (; i < l_seq; i += 2) {
      const int a = sam_seq_code(L[fs[9] + i]);
      const int b = i + 1 < l_seq ? sam_seq_code(L[fs[9] + i + 1]) : 0;
      if (a < 0 || b < 0) return SAM_E_SEQ;
      O.put8((uint32_t)a << 4 | (uint32_t)b);
    }
    i = 0;
    for (; i + 8 <= l_seq; i += 8) {
      uint64_t q8 = ~0ull;
      if (!qual_star && !sam_qual8(L + fs[10] + i, &q8)) return SAM_E_QUAL;
      O.put_w64(q8);
    }
    for (; i < l_seq; i++) {
      if (qual_star) {
        O.put8(0xff);
      } else {
        const uint8_t c = L[fs[10] + i];
        if (c < 33) return SAM_E_QUAL;
        O.put8((uint32_t)c - 33);
      }
    }
  } else {
    O.o = I->qual_out + l_seq;
  }
  // ---- tags
  p = tags_at;
  while (p < len) {  // L[p] is the TAB before the next tag
    const int32_t a = ++p;
    while (p < len && L[p] != '\t') p++;
    const int32_t n = p - a;
    const uint8_t* f = L + a;
    const int32_t bad = sam_tag_error(f, n);
    if (n < 5 || f[2] != ':' || f[4] != ':') return bad;
    const uint8_t ty = f[3];
    const int32_t va = a + 5, vn = n - 5;
    const uint8_t* val = L + va;
    O.put8(f[0]);
    O.put8(f[1]);
    if (ty == 'A') {
      if (vn != 1 || val[0] < 33 || val[0] > 126) return bad;
      O.put8('A');
      O.put8(val[0]);
    } else if (ty == 'i') {
      if (!parse_dec(val, vn, true, -2147483648ll, 4294967295ll, &v)) return bad;
      if (v > 2147483647ll) {
        O.put8('I');
        O.put32((uint32_t)v);
      } else if (v > 65535) {
        O.put8('i');
        O.put32((uint32_t)v);
      } else if (v > 32767) {
        O.put8('S');
        O.put16((uint32_t)v);
      } else if (v > 255) {
        O.put8('s');
        O.put16((uint32_t)v);
      } else if (v > 127) {
        O.put8('C');
        O.put8((uint32_t)v);
      } else if (v >= -128) {
        O.put8('c');
        O.put8((uint32_t)v);
      } else if (v >= -32768) {
        O.put8('s');
        O.put16((uint32_t)v);
      } else {
        O.put8('i');
        O.put32((uint32_t)v);
      }
    } else if (ty == 'Z') {
      O.put8('Z');
      for (int32_t i = 0; i < vn; i++) O.put8(val[i]);
      O.put8(0);
    } else if (ty == 'H') {
      if (vn & 1) return bad;
      O.put8('H');
      for (int32_t i = 0; i < vn; i++) {
        const uint8_t c = val[i];
        if (!(is_digit(c) || (c >= 'A' && c <= 'F'))) return bad;
        O.put8(c);
      }
      O.put8(0);
    } else if (ty == 'f') {
      O.put8('f');
      if (!sam_put_float(L, va, vn, O, I, fx)) return bad;
    } else if (ty == 'B') {
      if (vn < 1) return bad;
      const uint8_t sub = val[0];
      int64_t lo = 0, hi = 0;
      int w = 0;  // bytes per value
      switch (sub) {
        case 'c': lo = -128, hi = 127, w = 1; break;
        case 'C': lo = 0, hi = 255, w = 1; break;
        case 's': lo = -32768, hi = 32767, w = 2; break;
        case 'S': lo = 0, hi = 65535, w = 2; break;
        case 'i': lo = -2147483648ll, hi = 2147483647ll, w = 4; break;
        case 'I': lo = 0, hi = 4294967295ll, w = 4; break;
        case 'f': w = 4; break;
        default: return bad;
      }
      if (vn > 1 && val[1] != ',') return bad;
      O.put8('B');
      O.put8(sub);
      const int32_t cnt_at = O.o;
      O.put32(0);
      int32_t cnt = 0;
      int32_t x = 1;  // at the ',' before the next value
      while (x < vn) {
        const int32_t ia = ++x;
        while (x < vn && val[x] != ',') x++;
        if (sub == 'f') {
          if (!sam_put_float(L, va + ia, x - ia, O, I, fx)) return bad;
        } else {
          if (!parse_dec(val + ia, x - ia, true, lo, hi, &v)) return bad;
          if (w == 1) O.put8((uint32_t)v);
          else if (w == 2) O.put16((uint32_t)v);
          else O.put32((uint32_t)v);
        }
        cnt++;
      }
      if (out && cnt_at + 4 <= out_cap) sam_poke32(out, cnt_at, (uint32_t)cnt);
    } else {
      return bad;
    }
  }
  // ---- the fixed 36 bytes; bin = reg2bin(pos, end): end 0 for an unmapped read (flag 0x4), else
  //      pos + the CIGAR's reference length, and pos + 1 when that is <= 0
  int32_t end = (flag & 4) ? 0 : (int32_t)(uint32_t)((int64_t)beg + reflen);
  if (end <= 0) end = beg + 1;
  const int32_t bin = sam_reg2bin(beg, end) & 0xffff;
  I->size = O.o;
  I->ref_id = ref;
  I->pos = beg;
  I->next_ref_id = nref;
  I->next_pos = npos;
  I->tlen = tlen;
  I->flag = (uint16_t)flag;
  I->bin = (uint16_t)bin;
  I->n_cigar = (uint16_t)ncig;
  I->mapq = (uint8_t)mapq;
  I->l_read_name = (uint8_t)(lname + 1);
  if (out && out_cap >= 36) {
    sam_poke32(out, 0, (uint32_t)(O.o - 4));
    sam_poke32(out, 4, (uint32_t)ref);
    sam_poke32(out, 8, (uint32_t)beg);
    out[12] = (uint8_t)(lname + 1);
    out[13] = (uint8_t)mapq;
    out[14] = (uint8_t)bin;
    out[15] = (uint8_t)(bin >> 8);
    out[16] = (uint8_t)ncig;
    out[17] = (uint8_t)(ncig >> 8);
    out[18] = (uint8_t)flag;
    out[19] = (uint8_t)(flag >> 8);
    sam_poke32(out, 20, (uint32_t)l_seq);
    sam_poke32(out, 24, (uint32_t)nref);
    sam_poke32(out, 28, (uint32_t)npos);
    sam_poke32(out, 32, (uint32_t)tlen);
  }
  return SAM_OK;
}

// Size pass: validates every column and tag; I->size = the record's bytes (4 + block_size).
DQT_INLINE int32_t sam_line_size(const uint8_t* line, int32_t len, const NameTable& R, SamLineInfo* I) {
  return sam_line_walk(line, len, R, nullptr, 0, I, nullptr, true);
}

// Encode pass over a line the size pass accepted: writes the I->size bytes at out.
DQT_INLINE int32_t sam_line_encode(const uint8_t* line, int32_t len, const NameTable& R, uint8_t* out,
                                   int32_t out_cap, SamLineInfo* I, const SamFixSink* fx) {
  return sam_line_walk(line, len, R, out, out_cap, I, fx, true);
}

// ------------------------------------------------------------------ host: the header
// The leading '@' lines of a SAM text as a BAM header (samutil.sam_header_to_bam): BAM\1, l_text,
// every such line followed by LF, n_ref, then per @SQ line l_name, name, NUL, LN.  `whole`: t is the
// whole file (else a prefix: returns 1 when the header may run past it).  -1: a bad @SQ line.
struct SamHeader {
  std::vector<uint8_t> bam;
  std::vector<std::string> names;
  std::vector<int32_t> lens;
};

inline int sam_header_build(const uint8_t* t, int64_t n, bool whole, SamHeader* H) {
  H->bam.clear();
  H->names.clear();
  H->lens.clear();
  std::string text;
  int64_t p = 0;
  while (p < n && t[p] == '@') {
    int64_t e = p;
    while (e < n && t[e] != '\n' && t[e] != '\r') e++;
    int64_t nx = e + 1;
    if (e >= n) {
      if (!whole) return 1;
      nx = n;
    } else if (t[e] == '\r') {
      if (e + 1 < n) nx = t[e + 1] == '\n' ? e + 2 : e + 1;
      else if (!whole) return 1;
    }
    const std::string line((const char*)t + p, (size_t)(e - p));
    text += line;
    text += '\n';
    if (line.compare(0, 4, "@SQ\t") == 0) {
      std::string sn, ln;
      bool has_sn = false, has_ln = false;
      size_t a = 4;
      while (a <= line.size()) {
        size_t b = line.find('\t', a);
        if (b == std::string::npos) b = line.size();
        const std::string f = line.substr(a, b - a);
        const size_t c = f.find(':');
        if (c != std::string::npos) {
          if (f.compare(0, c, "SN") == 0) sn = f.substr(c + 1), has_sn = true;
          if (f.compare(0, c, "LN") == 0) ln = f.substr(c + 1), has_ln = true;
        }
        a = b + 1;
      }
      int64_t v = 0;
      if (!has_sn || !has_ln ||
          !parse_dec((const uint8_t*)ln.data(), (int32_t)ln.size(), true, -2147483648ll, 2147483647ll, &v))
        return -1;
      H->names.push_back(sn);
      H->lens.push_back((int32_t)v);
    }
    p = nx;
  }
  if (p >= n && !whole) return 1;
  auto put32 = [&](uint32_t v) {
    for (int k = 0; k < 4; k++) H->bam.push_back((uint8_t)(v >> (8 * k)));
  };
  H->bam.assign({'B', 'A', 'M', 1});
  put32((uint32_t)text.size());
  H->bam.insert(H->bam.end(), text.begin(), text.end());
  put32((uint32_t)H->names.size());
  for (size_t r = 0; r < H->names.size(); r++) {
    put32((uint32_t)H->names[r].size() + 1);
    H->bam.insert(H->bam.end(), H->names[r].begin(), H->names[r].end());
    H->bam.push_back(0);
    put32((uint32_t)H->lens[r]);
  }
  return 0;
}

}  // namespace dqs
