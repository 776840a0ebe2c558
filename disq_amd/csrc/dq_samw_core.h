// dq_samw_core.h -- the per-record rules of the SAM writer: one BAM record
// into one SAM line as htsjdk SAMTextWriter.getSAMString + TextTagCodec print it, trimmed as Java's
// String.trim does and followed by LF (SamSink.save), restated by tests/samwriteutil.py
// (record_to_sam_line), whose order of checks this keeps so that the first error of a record is the
// same one.  The kernels of dq_samw.hip and the host program tools/sam_write_check.cpp compile the
// same functions (the __HIPCC__ guards of dq_text_core.h).
//
// One walk serves both passes: with out == nullptr it validates and sizes the line, with out set it
// writes the bytes, every store bounded by the size the first pass gave; so a line can never get
// more bytes than it was sized for.  The tag chain is stepped through with dq_tags_core.h's tag_next,
// which the tag decode (dq_tags.hip) shares.
#pragma once
#include <stdint.h>

#include "dq_sam_core.h"
#include "dq_samw_pow5.h"
#include "dq_tags_core.h"

namespace dqw {

constexpr int32_t SAMW_LONG = 2048;   // records of more bytes (4 + block_size) get a wave
constexpr int32_t SAMW_RUN = 64;      // records one workgroup formats into one LDS tile
constexpr int32_t SAMW_TILE = 32752;  // most line bytes of a run the tile takes (+ 16 of alignment)

// The header's reference names by index: names[name_off[r], name_off[r + 1]).
struct RefNames {
  const int32_t* name_off;
  const uint8_t* names;
  int32_t n;
};

// ------------------------------------------------------------------ the line being written
// String.trim is folded into the sink: bytes <= 0x20 before the first larger one are dropped, and
// `keep` is the end of the last larger one, which is where the line ends.
struct Sink {
  uint8_t* out;   // nullptr: size only
  int64_t cap;    // bytes out may take
  int64_t pos = 0, keep = 0;
  bool started = false;
  bool over = false;  // a byte that belongs to the line did not fit
};

DQT_INLINE void put(Sink& s, uint8_t b) {
  if (!s.started) {
    if (b <= 0x20) return;
    s.started = true;
  }
  if (s.out) {
    if (s.pos < s.cap) s.out[s.pos] = b;
    else if (b > 0x20) s.over = true;
  }
  s.pos++;
  if (b > 0x20) s.keep = s.pos;
}

DQT_INLINE void put_bytes(Sink& s, const uint8_t* p, int64_t n) {
  for (int64_t i = 0; i < n; i++) put(s, p[i]);
}

// Two digits of q < 100: the tens in the low byte.
DQT_INLINE uint32_t dec2(uint32_t q) {
  const uint32_t t = (q * 103u) >> 10;
  return t | ((q - 10u * t) << 8);
}

// The eight digits of x < 10^8 as ASCII, the first digit in the low byte (divisions by constants:
// multiply and shift).
DQT_INLINE uint64_t dec8(uint32_t x) {
  const uint32_t hi = x / 10000u, lo = x - hi * 10000u;
  const uint32_t a = hi / 100u, b = hi - a * 100u, c = lo / 100u, d = lo - c * 100u;
  const uint64_t w = (uint64_t)dec2(a) | (uint64_t)dec2(b) << 16 | (uint64_t)dec2(c) << 32 |
                     (uint64_t)dec2(d) << 48;
  return w + 0x3030303030303030ull;
}

DQT_INLINE int dec_len(uint32_t v) {  // v < 10^9
  return v < 10u ? 1 : v < 100u ? 2 : v < 1000u ? 3 : v < 10000u ? 4 : v < 100000u ? 5 :
         v < 1000000u ? 6 : v < 10000000u ? 7 : v < 100000000u ? 8 : 9;
}

DQT_INLINE void put_u32(Sink& s, uint32_t v) {
  uint32_t low = v;
  int n;
  if (v >= 100000000u) {
    const uint32_t top = v / 100000000u;  // 1 .. 42
    low = v - top * 100000000u;
    if (top >= 10u) put(s, (uint8_t)('0' + top / 10u));
    put(s, (uint8_t)('0' + top % 10u));
    n = 8;
  } else {
    n = dec_len(v);
  }
  const uint64_t w = dec8(low) >> (8 * (8 - n));
  for (int i = 0; i < n; i++) put(s, (uint8_t)(w >> (8 * i)));
}

DQT_INLINE void put_i32(Sink& s, int32_t v) {
  if (v < 0) {
    put(s, '-');
    put_u32(s, 0u - (uint32_t)v);
  } else {
    put_u32(s, (uint32_t)v);
  }
}

// ------------------------------------------------------------------ Float.toString
DQT_INLINE uint32_t mul_shift32(uint32_t m, uint64_t factor, int32_t shift) {  // shift > 32
  const uint64_t b0 = (uint64_t)m * (uint32_t)factor, b1 = (uint64_t)m * (uint32_t)(factor >> 32);
  return (uint32_t)(((b0 >> 32) + b1) >> (shift - 32));
}
DQT_INLINE int32_t pow5bits(int32_t e) { return (int32_t)(((uint32_t)e * 1217359u) >> 19) + 1; }
DQT_INLINE int32_t log10_pow2(int32_t e) { return (int32_t)(((uint32_t)e * 78913u) >> 18); }
DQT_INLINE int32_t log10_pow5(int32_t e) { return (int32_t)(((uint32_t)e * 732923u) >> 20); }
DQT_INLINE bool multiple_of_pow5(uint32_t v, int32_t p) {
  int32_t c = 0;
  while (v != 0 && v % 5u == 0) {
    v /= 5u;
    c++;
  }
  return c >= p;
}

// The shortest decimal of a finite non-zero binary32 (sign ignored): value = *digits * 10^*e10,
// *digits without trailing zeros.  Of the decimals that read back to the same bits (round to
// nearest, ties to even) those with the fewest digits, of these the nearest, on a tie the even one
// (the Ryu scheme, Adams 2018: the value and both ends of its rounding interval, scaled by a power
// of ten with one 32 x 64-bit product each, lose digits together while they still differ).
DQT_INLINE void samw_shortest(uint32_t bits, uint32_t* digits, int32_t* e10) {
  static constexpr uint64_t INV[DQ_SAMW_POW5_INV_N] = {DQ_SAMW_POW5_INV_TABLE};
  static constexpr uint64_t POW[DQ_SAMW_POW5_N] = {DQ_SAMW_POW5_TABLE};
  const uint32_t frac = bits & 0x7fffffu, ex = (bits >> 23) & 0xffu;
  const int32_t e2 = (ex == 0 ? 1 : (int32_t)ex) - 127 - 23 - 2;
  const uint32_t m2 = ex == 0 ? frac : (frac | 1u << 23);
  const bool accept = (m2 & 1u) == 0;
  const uint32_t mv = 4u * m2, mp = 4u * m2 + 2u;
  const uint32_t mm_shift = (frac != 0 || ex <= 1) ? 1u : 0u;
  const uint32_t mm = 4u * m2 - 1u - mm_shift;
  uint32_t vr, vp, vm;
  int32_t exp10;
  bool vm_tz = false, vr_tz = false;
  uint32_t last = 0;
  if (e2 >= 0) {
    const int32_t q = log10_pow2(e2);
    exp10 = q;
    const int32_t k = DQ_SAMW_POW5_INV_BITS + pow5bits(q) - 1;
    const int32_t i = -e2 + q + k;
    DQS_CHECK(q >= 0 && q < DQ_SAMW_POW5_INV_N);
    vr = mul_shift32(mv, INV[q], i);
    vp = mul_shift32(mp, INV[q], i);
    vm = mul_shift32(mm, INV[q], i);
    if (q != 0 && (vp - 1u) / 10u <= vm / 10u) {
      const int32_t l = DQ_SAMW_POW5_INV_BITS + pow5bits(q - 1) - 1;
      last = mul_shift32(mv, INV[q - 1], -e2 + q - 1 + l) % 10u;
    }
    if (q <= 9) {
      if (mv % 5u == 0) vr_tz = multiple_of_pow5(mv, q);
      else if (accept) vm_tz = multiple_of_pow5(mm, q);
      else vp -= multiple_of_pow5(mp, q) ? 1u : 0u;
    }
  } else {
    const int32_t q = log10_pow5(-e2);
    exp10 = q + e2;
    const int32_t i = -e2 - q;
    const int32_t k = pow5bits(i) - DQ_SAMW_POW5_BITS;
    int32_t j = q - k;
    DQS_CHECK(i >= 0 && i + 1 < DQ_SAMW_POW5_N);
    vr = mul_shift32(mv, POW[i], j);
    vp = mul_shift32(mp, POW[i], j);
    vm = mul_shift32(mm, POW[i], j);
    if (q != 0 && (vp - 1u) / 10u <= vm / 10u) {
      j = q - 1 - (pow5bits(i + 1) - DQ_SAMW_POW5_BITS);
      last = mul_shift32(mv, POW[i + 1], j) % 10u;
    }
    if (q <= 1) {
      vr_tz = true;
      if (accept) vm_tz = mm_shift == 1u;
      else --vp;
    } else if (q < 31) {
      vr_tz = (mv & ((1u << (q - 1)) - 1u)) == 0;
    }
  }
  int32_t removed = 0;
  uint32_t o;
  if (vm_tz || vr_tz) {
    while (vp / 10u > vm / 10u) {
      vm_tz = vm_tz && vm % 10u == 0;
      vr_tz = vr_tz && last == 0;
      last = vr % 10u;
      vr /= 10u;
      vp /= 10u;
      vm /= 10u;
      removed++;
    }
    if (vm_tz) {
      while (vm % 10u == 0) {
        vr_tz = vr_tz && last == 0;
        last = vr % 10u;
        vr /= 10u;
        vp /= 10u;
        vm /= 10u;
        removed++;
      }
    }
    if (vr_tz && last == 5u && vr % 2u == 0) last = 4u;  // exactly half: to even
    o = vr + (((vr == vm && (!accept || !vm_tz)) || last >= 5u) ? 1u : 0u);
  } else {
    while (vp / 10u > vm / 10u) {
      last = vr % 10u;
      vr /= 10u;
      vp /= 10u;
      vm /= 10u;
      removed++;
    }
    o = vr + ((vr == vm || last >= 5u) ? 1u : 0u);
  }
  int32_t e = exp10 + removed;
  while (o != 0 && o % 10u == 0) {
    o /= 10u;
    e++;
  }
  // Float.toString renders two digits, and where one would do it takes the nearest two-digit
  // decimal.  That is digit.0 unless two-digit decimals lie closer together than floats do, which
  // holds below about 1.05e-42 only: the subnormals m * 2^-149, m < 1024.  There x = m * 5^46 /
  // 2^103 = value * 10^46 >= 14, rounded to two digits with exact integers.
  if (o < 10u && ex == 0 && frac < 1024u) {
    uint64_t hi, lo, t;
    dqs::sam_mul64((uint64_t)frac, DQ_SAMW_POW5_46_LO, &t, &lo);
    hi = (uint64_t)frac * DQ_SAMW_POW5_46_HI + t;
    const uint32_t ip = (uint32_t)(hi >> 39);  // floor(x) < 14400
    const uint32_t p = ip >= 10000u ? 1000u : ip >= 1000u ? 100u : ip >= 100u ? 10u : 1u;
    uint32_t c = ip / p;
    const uint64_t hi2 = hi << 1 | lo >> 63, lo2 = lo << 1;  // 2 x against (2 c + 1) p
    const uint64_t rhs = (uint64_t)((2u * c + 1u) * p) << 39;
    if (hi2 > rhs || (hi2 == rhs && lo2 != 0)) c++;  // (no ties: 10^-j is no dyadic number)
    int32_t pe = p == 1000u ? 3 : p == 100u ? 2 : p == 10u ? 1 : 0;
    if (c == 100u) {
      c = 10u;
      pe++;
    }
    if (c % 10u == 0) {
      c /= 10u;
      pe++;
    }
    o = c;
    e = pe - 46;
  }
  *digits = o;
  *e10 = e;
}

// Float.toString (the JDK 19+ contract) of the binary32 with these bits: at most 16 bytes.
DQT_INLINE void put_float(Sink& s, uint32_t bits) {
  const uint32_t frac = bits & 0x7fffffu, ex = (bits >> 23) & 0xffu;
  if (ex == 0xffu && frac != 0) {
    put(s, 'N');
    put(s, 'a');
    put(s, 'N');
    return;
  }
  if (bits >> 31) put(s, '-');
  if (ex == 0xffu) {
    const uint64_t w = 0x7974696e69666e49ull;  // "Infinity"
    for (int i = 0; i < 8; i++) put(s, (uint8_t)(w >> (8 * i)));
    return;
  }
  if (ex == 0 && frac == 0) {
    put(s, '0');
    put(s, '.');
    put(s, '0');
    return;
  }
  uint32_t o;
  int32_t e;
  samw_shortest(bits, &o, &e);
  const int n = dec_len(o);                // 1 .. 9 digits
  const int32_t e10 = e + n - 1;           // exponent of the first digit
  const uint32_t top = o / 100000000u;     // the digits as nine characters, zero padded
  const uint64_t w = dec8(o - top * 100000000u);
  auto digit = [&](int i) -> uint8_t {     // digit i of the n
    const int j = 9 - n + i;
    return j == 0 ? (uint8_t)('0' + top) : (uint8_t)(w >> (8 * (j - 1)));
  };
  if (e10 >= -3 && e10 <= 6) {             // 1e-3 <= |x| < 1e7: plain
    if (e10 < 0) {
      put(s, '0');
      put(s, '.');
      for (int32_t z = 0; z < -e10 - 1; z++) put(s, '0');
      for (int i = 0; i < n; i++) put(s, digit(i));
    } else {
      for (int i = 0; i <= e10; i++) put(s, i < n ? digit(i) : (uint8_t)'0');
      put(s, '.');
      if (n <= e10 + 1) put(s, '0');
      for (int i = e10 + 1; i < n; i++) put(s, digit(i));
    }
  } else {
    put(s, digit(0));
    put(s, '.');
    if (n == 1) put(s, '0');
    for (int i = 1; i < n; i++) put(s, digit(i));
    put(s, 'E');
    put_i32(s, e10);
  }
}

// ------------------------------------------------------------------ one record
DQT_INLINE int32_t rd32(const uint8_t* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return (int32_t)v;
}
DQT_INLINE uint32_t rd16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }

struct Layout {     // byte offsets from the block_size word
  int64_t end;      // 4 + block_size
  int64_t cig_at, seq_at, qual_at, tags_at;
  int32_t l_rn, n_cig, l_seq;
};

// The fixed part and the parts it sizes must lie inside the record, the record inside `avail`.
DQT_INLINE int32_t samw_layout(const uint8_t* r, int64_t avail, Layout* L) {
  if (avail < 36) return dqs::SAM_E_FIELDS;
  const int32_t bs = rd32(r);
  if (bs < 32 || 4 + (int64_t)bs > avail) return dqs::SAM_E_FIELDS;
  L->end = 4 + (int64_t)bs;
  L->l_rn = r[12];
  L->n_cig = (int32_t)rd16(r + 16);
  L->l_seq = rd32(r + 20);
  if (L->l_seq < 0) return dqs::SAM_E_FIELDS;
  L->cig_at = 36 + L->l_rn;
  L->seq_at = L->cig_at + 4 * (int64_t)L->n_cig;
  L->qual_at = L->seq_at + ((int64_t)L->l_seq + 1) / 2;
  L->tags_at = L->qual_at + L->l_seq;
  if (L->tags_at > L->end) return dqs::SAM_E_FIELDS;
  return dqs::SAM_OK;
}

// Eight qualities: all 0xFF, or one above 93 (0xFF in a partly filled array included)?
DQT_INLINE void samw_qual8(uint64_t w, bool* all_ff, bool* bad) {
  *all_ff = *all_ff && w == ~0ull;
  const uint64_t H = 0x8080808080808080ull;
  *bad = *bad || ((w | ((w & ~H) + 0x2222222222222222ull)) & H) != 0;  // 94 + 34 = 128
}

// Four packed bytes (the first in the low byte) into eight bases, the first in the low byte.
DQT_INLINE uint64_t samw_seq8(uint32_t pk) {
  const uint64_t T0 = 0x52474d43413dull | 0x5653ull << 48;  // "=ACMGRSV"
  const uint64_t T1 = 0x4e42444b48595754ull;                // "TWYHKDBN"
  uint64_t o = 0;
  for (int i = 0; i < 8; i++) {
    const uint32_t nib = (pk >> (8 * (i >> 1) + ((i & 1) ? 0 : 4))) & 15u;
    o |= (((nib & 8u) ? T1 : T0) >> (8 * (nib & 7u)) & 0xffull) << (8 * i);
  }
  return o;
}

struct Walk {
  Layout L;
  int64_t size;               // line bytes, the LF included
  int64_t seq_out, qual_out;  // where SEQ and QUAL start in the line
  bool qual_star;
};

// The line of the record at r (avail bytes readable).  bulk_skip: SEQ and QUAL are neither read nor
// written, only stepped over (a wave shares them; the caller has scanned QUAL and says whether it
// prints as '*').  Returns the first failing check: fields, QNAME, RNAME, CIGAR, RNEXT, QUAL, then
// the tags as stored.
DQT_INLINE int32_t samw_record_walk(const uint8_t* r, int64_t avail, const RefNames& R, uint8_t* out,
                                    int64_t cap, bool bulk_skip, bool qual_star_in, Walk* W) {
  Layout& L = W->L;
  W->size = 0;
  W->seq_out = W->qual_out = 0;
  W->qual_star = true;
  int32_t st = samw_layout(r, avail, &L);
  if (st) return st;
  if (L.l_rn < 2) return dqs::SAM_E_QNAME;
  const int32_t ref = rd32(r + 4), nref = rd32(r + 24);
  if (ref < -1 || ref >= R.n) return dqs::SAM_E_RNAME;
  Sink s{out, cap};
  put_bytes(s, r + 36, L.l_rn - 1);
  put(s, '\t');
  put_u32(s, rd16(r + 18));  // FLAG
  put(s, '\t');
  if (ref < 0) put(s, '*');
  else put_bytes(s, R.names + R.name_off[ref], R.name_off[ref + 1] - R.name_off[ref]);
  put(s, '\t');
  put_i32(s, (int32_t)((uint32_t)rd32(r + 8) + 1u));  // POS: Java's int wraps
  put(s, '\t');
  put_u32(s, r[13]);  // MAPQ
  put(s, '\t');
  if (L.n_cig == 0) put(s, '*');
  for (int32_t c = 0; c < L.n_cig; c++) {
    const uint32_t w = (uint32_t)rd32(r + L.cig_at + 4 * (int64_t)c);
    if ((w & 15u) > 8u) return dqs::SAM_E_CIGAR;
    put_u32(s, w >> 4);
    const uint32_t op = w & 15u;  // "MIDNSHP=" and 'X'
    put(s, op < 8u ? (uint8_t)(0x3d5048534e44494dull >> (8 * op)) : (uint8_t)'X');
  }
  put(s, '\t');
  if (nref < -1 || nref >= R.n) return dqs::SAM_E_RNEXT;
  if (nref < 0) put(s, '*');
  else if (nref == ref) put(s, '=');
  else put_bytes(s, R.names + R.name_off[nref], R.name_off[nref + 1] - R.name_off[nref]);
  put(s, '\t');
  put_i32(s, (int32_t)((uint32_t)rd32(r + 28) + 1u));  // PNEXT
  put(s, '\t');
  put_i32(s, rd32(r + 32));  // TLEN
  put(s, '\t');
  // ---- SEQ and QUAL
  const int32_t n = L.l_seq;
  const uint8_t* sq = r + L.seq_at;
  const uint8_t* ql = r + L.qual_at;
  bool star = n == 0 || qual_star_in;
  if (!bulk_skip && n > 0) {  // QUAL decides its own size: '*' when every byte is 0xFF
    bool all_ff = true, bad = false;
    int32_t i = 0;
    for (; i + 8 <= n; i += 8) {
      uint64_t w;
      __builtin_memcpy(&w, ql + i, 8);
      samw_qual8(w, &all_ff, &bad);
    }
    for (; i < n; i++) {
      all_ff = all_ff && ql[i] == 0xff;
      bad = bad || ql[i] > 93;
    }
    star = all_ff;
    if (!all_ff && bad) return dqs::SAM_E_QUAL;
  }
  W->qual_star = star;
  W->seq_out = s.pos;
  if (n == 0) {
    put(s, '*');
  } else if (bulk_skip) {
    s.pos += n;  // (the line has started: FLAG's digits)
    s.keep = s.pos;
  } else {
    int32_t i = 0;
    for (; i + 8 <= n; i += 8) {
      const uint64_t w = samw_seq8((uint32_t)rd32(sq + (i >> 1)));
      for (int b = 0; b < 8; b++) put(s, (uint8_t)(w >> (8 * b)));
    }
    for (; i < n; i++) {
      const uint32_t nib = (sq[i >> 1] >> ((i & 1) ? 0 : 4)) & 15u;
      put(s, (uint8_t)(samw_seq8(nib << 4)));
    }
  }
  put(s, '\t');
  W->qual_out = s.pos;
  if (star) {
    put(s, '*');
  } else if (bulk_skip) {
    s.pos += n;
    s.keep = s.pos;
  } else {
    for (int32_t i = 0; i < n; i++) put(s, (uint8_t)(ql[i] + 33));
  }
  // ---- tags, in stored order (dq_tags_core.h locates and validates each one)
  int64_t p = L.tags_at;
  const int64_t end = L.end;
  while (p < end) {
    dqa::Tag T;
    const int32_t err = dqa::tag_next(r, p, end, &T);
    if (err) return err;
    const uint8_t ty = T.ty;
    const uint8_t* v = r + T.at;
    put(s, '\t');
    put(s, r[p]);
    put(s, r[p + 1]);
    put(s, ':');
    if (ty == 'A') {
      put(s, 'A');
      put(s, ':');
      put(s, v[0]);
    } else if (ty == 'f') {
      put(s, 'f');
      put(s, ':');
      put_float(s, (uint32_t)rd32(v));
    } else if (ty == 'Z' || ty == 'H') {
      put(s, ty);
      put(s, ':');
      if (ty == 'Z') {
        put_bytes(s, v, T.len);
      } else {
        for (int64_t i = 0; i < T.len; i++) {
          const uint8_t c = v[i];
          put(s, c >= 'a' && c <= 'f' ? (uint8_t)(c - 32) : c);
        }
      }
    } else if (ty == 'B') {
      const uint8_t sub = T.sub;
      const int sz = sub == 'f' ? 4 : dqa::tag_int_size(sub);
      put(s, 'B');
      put(s, ':');
      put(s, sub);
      for (int32_t k = 0; k < T.count; k++) {
        const uint8_t* e = v + (int64_t)sz * k;
        put(s, ',');
        if (sub == 'c') put_i32(s, (int8_t)e[0]);
        else if (sub == 'C') put_u32(s, e[0]);
        else if (sub == 's') put_i32(s, (int16_t)rd16(e));
        else if (sub == 'S') put_u32(s, rd16(e));
        else if (sub == 'i') put_i32(s, rd32(e));
        else if (sub == 'I') put_u32(s, (uint32_t)rd32(e));
        else put_float(s, (uint32_t)rd32(e));
      }
    } else {  // c C s S i I: tag_next knows no other type
      put(s, 'i');
      put(s, ':');
      if (ty == 'c') put_i32(s, (int8_t)v[0]);
      else if (ty == 'C') put_u32(s, v[0]);
      else if (ty == 's') put_i32(s, (int16_t)rd16(v));
      else if (ty == 'S') put_u32(s, rd16(v));
      else if (ty == 'i') put_i32(s, rd32(v));
      else put_u32(s, (uint32_t)rd32(v));
    }
    p = T.next;
  }
  // String.trim has cut the line at `keep`; saveAsTextFile's LF follows
  W->size = s.keep + 1;
  if (out) {
    DQS_CHECK(!s.over && s.keep + 1 == cap);
    if (s.keep < cap) out[s.keep] = '\n';
  }
  return dqs::SAM_OK;
}

}  // namespace dqw
