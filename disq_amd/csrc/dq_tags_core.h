// dq_tags_core.h -- the rules of a BAM record's optional fields (SAMv1 section 4.2.4; DESIGN.md
// section 18): one tag of the chain located and validated (tag_next), and the whole chain of a
// record projected onto the caller's keys (tags_walk), restated by tests/tagutil.py.  The SAM
// writer's record walk (dq_samw_core.h) steps through the chain with the same tag_next, so the two
// units cannot disagree on what a well-formed tag is or how a bad one is named.  The kernels of
// dq_tags.hip and the host program tools/tags_check.cpp compile the same functions (the __HIPCC__
// guards of dq_text_core.h).
#pragma once
#include <stdint.h>

#include "dq_sam_core.h"

namespace dqa {

// dq_tag_key.type / dq_tag_batch.flags (include/disq_gpu.h)
enum : int32_t { TAG_ANY = 0, TAG_INT = 1, TAG_FLOAT = 2, TAG_CHAR = 3, TAG_STRING = 4 };
enum : int32_t { TAG_PRESENT = 1, TAG_REPEATED = 4 };
constexpr int32_t TAG_MAX_KEYS = 64;

// ------------------------------------------------------------------ one tag
struct Tag {
  uint8_t ty, sub;  // the stored type byte; a B array's element type, else 0
  int32_t count;    // a B array's elements, else 0
  int64_t at;       // first payload byte (Z/H: first character; B: first element)
  int64_t len;      // payload bytes (Z/H: without the NUL; B: element size * count)
  int64_t next;     // the tag behind this one
};

DQT_INLINE uint32_t tag_rd16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
DQT_INLINE uint32_t tag_rd32(const uint8_t* p) {
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

DQT_INLINE int tag_int_size(uint8_t ty) {
  return (ty == 'c' || ty == 'C') ? 1 : (ty == 's' || ty == 'S') ? 2 : (ty == 'i' || ty == 'I') ? 4 : 0;
}

// The first NUL of A[p, end), or end.  Eight bytes a step where eight are left (the classic
// has-zero-byte test); no byte outside [p, end) is read.
DQT_INLINE int64_t tag_find_nul(const uint8_t* A, int64_t p, int64_t end) {
  while (p + 8 <= end) {
    uint64_t w;
    __builtin_memcpy(&w, A + p, 8);
    const uint64_t z = (w - 0x0101010101010101ull) & ~w & 0x8080808080808080ull;
    if (z) {
      int64_t i = 0;
      while (A[p + i] != 0) i++;  // < 8
      return p + i;
    }
    p += 8;
  }
  while (p < end && A[p] != 0) p++;
  return p;
}

// The tag at A[p, end), p < end: 0 and *T, or the error as the SAM writer names it
// (dqs::sam_tag_error: no name where fewer than three bytes are left, else the tag's two name
// bytes).  The checks: the bytes a type needs are left in the record; Z and H end in a NUL; H has
// an even number of hex digits; a B array's element type is one of cCsSiIf, its count is not
// negative and its elements are left in the record; the type byte is known.  A B array is stepped
// over by its count, never element by element.
DQT_INLINE int32_t tag_next(const uint8_t* A, int64_t p, int64_t end, Tag* T) {
  if (end - p < 3) return dqs::sam_tag_error(A + p, 0);
  const int32_t err = dqs::sam_tag_error(A + p, 2);
  const uint8_t ty = A[p + 2];
  p += 3;
  const int64_t left = end - p;
  T->ty = ty;
  T->sub = 0;
  T->count = 0;
  T->at = p;
  if (ty == 'A' || ty == 'f' || tag_int_size(ty)) {
    const int sz = ty == 'A' ? 1 : ty == 'f' ? 4 : tag_int_size(ty);
    if (left < sz) return err;
    T->len = sz;
    T->next = p + sz;
  } else if (ty == 'Z' || ty == 'H') {
    const int64_t z = tag_find_nul(A, p, end);
    if (z >= end) return err;
    if (ty == 'H') {
      if ((z - p) & 1) return err;
      for (int64_t i = p; i < z; i++) {
        const uint8_t c = A[i];
        if (!((c >= 'a' && c <= 'f') || (c >= 'A' && c <= 'F') || (c >= '0' && c <= '9'))) return err;
      }
    }
    T->len = z - p;
    T->next = z + 1;
  } else if (ty == 'B') {
    if (left < 5) return err;
    const uint8_t sub = A[p];
    const int32_t cnt = (int32_t)tag_rd32(A + p + 1);
    p += 5;
    const int sz = sub == 'f' ? 4 : tag_int_size(sub);
    if (sz == 0 || cnt < 0 || (int64_t)sz * cnt > end - p) return err;
    T->sub = sub;
    T->count = cnt;
    T->at = p;
    T->len = (int64_t)sz * cnt;
    T->next = p + T->len;
  } else {
    return err;
  }
  return 0;
}

// ------------------------------------------------------------------ the caller's keys
// A key's id is its two bytes as a 16-bit number (the first byte low).  The table is an open-addressed
// hash of 128 slots (at most 64 keys): a slot is id | q << 16 | 1 << 31, zero when empty.
constexpr int32_t TAG_SLOTS = 128;
struct TagKeys {
  const uint32_t* slot;  // [TAG_SLOTS]
  const uint8_t* type;   // [n] TAG_*
  int32_t n;
};
DQT_INLINE uint32_t tag_slot_of(uint32_t id) { return ((id * 40503u) >> 7) & (TAG_SLOTS - 1); }

DQT_INLINE int32_t tag_lookup(const TagKeys& K, uint32_t id) {
  uint32_t s = tag_slot_of(id);
  for (int32_t i = 0; i < TAG_SLOTS; i++) {  // an empty slot ends the probe: at most 64 are taken
    const uint32_t e = K.slot[s];
    if (e == 0) return -1;
    if ((e & 0xffffu) == id) return (int32_t)((e >> 16) & 0x7fu);
    s = (s + 1) & (TAG_SLOTS - 1);
  }
  return -1;
}

// Host: the table of n ids (two bytes each); nullptr, or why the list is refused.
inline const char* tag_keys_build(const char* const* ids, const int32_t* types, int32_t n, uint32_t* slot,
                                  uint8_t* type) {
  if (n < 1 || n > TAG_MAX_KEYS) return "1 to 64 keys are taken";
  for (int32_t i = 0; i < TAG_SLOTS; i++) slot[i] = 0;
  for (int32_t q = 0; q < n; q++) {
    const char* s = ids[q];
    if (!s) return "a key without an id";
    const uint8_t a = (uint8_t)s[0], b = a ? (uint8_t)s[1] : 0;
    const bool alpha = (a >= 'A' && a <= 'Z') || (a >= 'a' && a <= 'z');
    const bool alnum = (b >= 'A' && b <= 'Z') || (b >= 'a' && b <= 'z') || (b >= '0' && b <= '9');
    if (!alpha || !alnum || s[2] != 0) return "a tag id is two bytes, [A-Za-z][A-Za-z0-9]";
    if (types[q] < TAG_ANY || types[q] > TAG_STRING) return "unknown key type";
    const uint32_t id = (uint32_t)a | (uint32_t)b << 8;
    uint32_t h = tag_slot_of(id);
    while (slot[h]) {
      if ((slot[h] & 0xffffu) == id) return "the same id twice";
      h = (h + 1) & (TAG_SLOTS - 1);
    }
    slot[h] = id | (uint32_t)q << 16 | 1u << 31;
    type[q] = (uint8_t)types[q];
  }
  return nullptr;
}

// Is a stored type byte of the class a key asked for?
DQT_INLINE bool tag_class_ok(int32_t want, uint8_t ty) {
  return want == TAG_ANY || (want == TAG_INT && tag_int_size(ty) != 0) || (want == TAG_FLOAT && ty == 'f') ||
         (want == TAG_CHAR && ty == 'A') || (want == TAG_STRING && ty == 'Z');
}

// The 32 bits a cell's value takes: INT the value extended as its stored type says, FLOAT the
// binary32 bits, CHAR the byte; 0 for every other class.
DQT_INLINE uint32_t tag_value(int32_t want, const Tag& T, const uint8_t* A) {
  const uint8_t* v = A + T.at;
  if (want == TAG_INT) {
    switch (T.ty) {
      case 'c': return (uint32_t)(int32_t)(int8_t)v[0];
      case 'C': return v[0];
      case 's': return (uint32_t)(int32_t)(int16_t)tag_rd16(v);
      case 'S': return tag_rd16(v);
      default: return tag_rd32(v);  // i, I
    }
  }
  if (want == TAG_FLOAT) return tag_rd32(v);
  if (want == TAG_CHAR) return v[0];
  return 0;
}

// ------------------------------------------------------------------ errors
// A row's first failing check, ordered for a minimum over rows: row << 20 | kind << 16 | the two
// name bytes.  The kinds: the record's layout ("fields"), a tag the walk refuses without a name
// ("tag ") or with one ("tag XX"), a requested key stored as another class ("tag XX type").
enum : int32_t { TAG_E_FIELDS = 1, TAG_E_TAG0 = 2, TAG_E_TAG = 3, TAG_E_TYPE = 4 };
DQT_INLINE int32_t tag_err_of_sam(int32_t st) {  // a dqs::sam_tag_error status
  return ((st >> 16) & 3) == 2 ? (TAG_E_TAG << 16 | (st & 0xffff)) : (TAG_E_TAG0 << 16);
}
DQT_INLINE uint64_t tag_error_key(int64_t row, int32_t err) { return (uint64_t)row << 20 | (uint32_t)err; }
// Host: "fields", "tag ", "tag XX", "tag XX type" into buf (>= 16 bytes).
inline const char* tag_error_name(int32_t err, char* buf) {
  const int kind = err >> 16;
  if (kind == TAG_E_FIELDS) return "fields";
  int n = 0;
  for (const char* s = "tag "; *s; s++) buf[n++] = *s;
  if (kind != TAG_E_TAG0) {
    buf[n++] = (char)((err >> 8) & 0xff);  // sam_tag_error keeps name[0] in the high byte
    buf[n++] = (char)(err & 0xff);
  }
  if (kind == TAG_E_TYPE)
    for (const char* s = " type"; *s; s++) buf[n++] = *s;
  buf[n] = 0;
  return buf;
}

// Where a record's aux region lies, from the fields the records stage keeps in its columns: the
// bytes [*aux_at, *end) counted from the block_size word.  False: the layout does not fit, the SAM
// writer's "fields" (samw_layout's checks on the same four numbers).
DQT_INLINE bool tag_region(int32_t block_size, int32_t l_read_name, int32_t n_cigar, int32_t l_seq,
                           int64_t* aux_at, int64_t* end) {
  if (block_size < 32 || l_seq < 0) return false;
  *end = 4 + (int64_t)block_size;
  *aux_at = 36 + (int64_t)l_read_name + 4 * (int64_t)n_cigar + ((int64_t)l_seq + 1) / 2 + l_seq;
  return *aux_at <= *end;
}

// ------------------------------------------------------------------ one record's chain
// The chain A[0, len) -- the aux region, which starts aux_at bytes behind the record's block_size
// word -- walked and validated whole; a requested key's first occurrence goes to sink.cell(q, tag,
// val_off, value), a later one to sink.repeated(q).  Returns 0 or the first failing check in
// stored order; *seen has bit q set for every key met.
template <class Sink>
DQT_INLINE int32_t tags_walk(const uint8_t* A, int64_t len, int64_t aux_at, const TagKeys& K, Sink& sink,
                             uint64_t* seen) {
  uint64_t have = 0;
  int64_t p = 0;
  *seen = 0;
  while (p < len) {
    Tag T;
    const int32_t st = tag_next(A, p, len, &T);
    if (st) return tag_err_of_sam(st);
    const uint32_t id = tag_rd16(A + p);
    const int32_t q = tag_lookup(K, id);
    if (q >= 0 && q < K.n) {
      if (have >> q & 1) {
        sink.repeated(q);
      } else {
        have |= 1ull << q;
        const int32_t want = K.type[q];
        // sam_tag_error's order of the name bytes
        if (!tag_class_ok(want, T.ty)) return TAG_E_TYPE << 16 | (int32_t)((id & 0xff) << 8 | id >> 8);
        sink.cell(q, T, (int32_t)(aux_at + T.at), tag_value(want, T, A));
      }
    }
    p = T.next;
  }
  *seen = have;
  return 0;
}

struct NullSink {
  DQT_INLINE void cell(int32_t, const Tag&, int32_t, uint32_t) {}
  DQT_INLINE void repeated(int32_t) {}
};

}  // namespace dqa
