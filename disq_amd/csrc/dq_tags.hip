// dq_tags.hip -- BAM aux tag decode: the optional fields of the
// records dq_read (dq_sam_read) returns, projected onto the caller's keys as the typed, key-major
// columns of dq_tag_batch -- what SAMRecord.getAttribute of those keys reads.  The per-record rules
// are dq_tags_core.h; this file holds the kernels around them.  They run
// behind the records stage on its resident columns: a row's record index, its offset in the stream
// (rec_lin) and the four numbers that place its aux region (block_size, l_read_name, n_cigar,
// l_seq) are read from the columns with coalesced loads, never from the record's head.
//   check    the first failing (row, check) by a min; nothing is stored;
//   decode   the same walk into the columns, every store guarded by its key, its row and the
//            value block's size; the cells of the keys a record lacks are stored blank.
// A thread owns a row: the chain is serial.  It walks a copy of its aux region in an LDS slot
// (TAG_SLOT below), or the region itself in memory when that is longer.  The key table (128 hash
// slots of a two-byte id and its key index, the types and the value bases) sits in LDS.  Every load
// of a record lies in its aux region [aux_at, 4 + block_size), which is checked to lie in the stream.
#include <cstdlib>

#include "dq_internal.h"
#include "dq_tags_core.h"

namespace dq {
namespace {

// How the aux bytes reach their thread.  A thread that walks its chain in memory loads it a byte at
// a time, 64 records' cache lines to a wave instruction; so it first copies its aux region into an
// LDS slot of its own with 16-byte loads and walks the copy, where the region is at most TAG_SLOT
// bytes; a longer one is walked in memory.  Measured against the two alternatives on a short-read
// file (17.6 M records of 324 bytes, 36.6 aux bytes on average) and a long-read one (48,853
// records, 35.5 aux bytes), both passes, keys [NM] / [NM AS XS RG] / all six, interleaved in one
// process (profiles/f12_tags_stage_ab_wgs.json, _longread.json):
//   the slot                                        3.36 / 3.34 / 3.40 ms    0.0244 / 0.0273 / 0.0284 ms
//   straight from memory                            7.10 / 7.36 / 7.45 ms    0.0242 / 0.0269 / 0.0280 ms
//   the span of the stream a block's 256 records
//   cover copied into LDS (up to 60 KiB, as
//   dq_vcf_stage.h stages lines)                    5.60 / 6.06 / 6.28 ms    0.0247 / 0.0276 / 0.0288 ms
// The span copy moves the rest of each record too, some eight bytes for every aux byte, and leaves
// room for two workgroups' LDS on a CU; it is not kept.  DQ_TAGS_STAGE=0 in the environment sends
// every record down the memory walk (tools/tags_bench.py --ab, and the tests of that path).
// The figures above were taken with the slots 128 bytes apart, where every lane's slot starts 32
// words behind its neighbour's (the same few LDS banks, which would explain the sweep; no counter
// was read).  Slot size and stride on the short-read file, same key lists
// (profiles/f12_tags_slot_sweep.txt): 128 / 128 3.38 / 3.38 / 3.44 ms, 128 / 132 2.27 / 2.57 / 2.72,
// 128 / 136 2.60 / 2.85 / 3.00, 128 / 144 2.25 / 2.52 / 2.67, 192 / 192 2.77 / 3.05 / 3.21, 64 / 64
// 2.19 / 2.32 / 2.46, 64 / 68 2.06 / 2.31 / 2.45, 64 / 72 2.39 / 2.64 / 2.79.  A stride of 36 words
// is the best of the 128-byte slots and keeps the 16-byte copies; a 64-byte slot is a few per
// cent faster there but would send every record with more aux bytes down the memory walk.
constexpr int32_t TAG_SLOT = 128;    // aux bytes a slot takes
constexpr int32_t TAG_STRIDE = 144;  // bytes from one thread's slot to the next

struct KeyLds {
  uint32_t slot[dqa::TAG_SLOTS];
  int64_t base[64];
  uint8_t type[64];
};

__device__ inline void keys_load(KeyLds& K, const TagIn& in, const TagCols* out) {
  const int t = threadIdx.x;
  if (t < dqa::TAG_SLOTS) K.slot[t] = in.key_slot[t];
  if (t < 64) {
    const bool on = t < in.n_keys;
    K.type[t] = on ? in.key_type[t] : 0;
    K.base[t] = on && out ? out->key_base[t] : -1;
  }
  __syncthreads();
}

struct DecodeSink {
  const TagCols& o;
  const KeyLds& K;
  int32_t nk;
  int64_t n, k;  // rows, this row
  __device__ bool row(int32_t q) const {
    const bool ok = q >= 0 && q < nk && k >= 0 && k < n;
    DQ_CHK(ok, CHK_SAM);
    return ok;
  }
  __device__ void value(int32_t q, uint32_t v) {
    const int64_t b = K.base[q];
    if (b < 0) return;  // ANY and STRING keys have no value block
    const bool ok = b + k < o.n_val;
    DQ_CHK(ok, CHK_SAM);
    if (ok) o.val[b + k] = v;
  }
  __device__ void cell(int32_t q, const dqa::Tag& T, int32_t val_off, uint32_t v) {
    if (!row(q)) return;
    const int64_t c = (int64_t)q * n + k;
    o.flags[c] = (uint8_t)dqa::TAG_PRESENT;
    o.vtype[c] = T.ty;
    o.subtype[c] = T.sub;
    o.val_off[c] = val_off;
    o.val_len[c] = (int32_t)T.len;
    value(q, v);
  }
  __device__ void repeated(int32_t q) {
    if (row(q)) o.flags[(int64_t)q * n + k] |= (uint8_t)dqa::TAG_REPEATED;  // this thread's own cell
  }
  __device__ void blank(int32_t q) {
    if (!row(q)) return;
    const int64_t c = (int64_t)q * n + k;
    o.flags[c] = 0;
    o.vtype[c] = 0;
    o.subtype[c] = 0;
    o.val_off[c] = -1;
    o.val_len[c] = 0;
    value(q, 0);
  }
};

// Row j's record: its index, where it lies in the stream and its aux region; false: "fields".
struct RowAt {
  int64_t lin, aux_at, end;
};
__device__ inline bool row_at(const TagIn& in, int64_t j, RowAt* R) {
  const int64_t k = in.idx ? in.idx[j] : in.first + j;
  DQ_CHK(k >= 0 && k < in.nrec, CHK_SAM);
  if (k < 0 || k >= in.nrec) return false;
  R->lin = in.rec_lin[k];
  if (!dqa::tag_region(in.block_size[k], in.l_read_name[k], in.n_cigar[k], in.l_seq[k], &R->aux_at, &R->end))
    return false;
  return R->lin >= 0 && R->lin + R->end <= in.src_len;
}

template <bool DEC>
__global__ __launch_bounds__(256) void tags_kernel(TagIn in, TagCols out, unsigned long long* __restrict__ scal,
                                                   int32_t use_slot) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[256 * TAG_STRIDE];
  __shared__ KeyLds K;
  keys_load(K, in, DEC ? &out : nullptr);
  const int64_t n = in.n, j0 = (int64_t)blockIdx.x * 256, j = j0 + threadIdx.x;
  if (j >= n) return;
  RowAt R;
  const bool fits = row_at(in, j, &R);
  if (!fits) {
    if (!DEC) atomicMin(&scal[0], dqa::tag_error_key(j, dqa::TAG_E_FIELDS << 16));
    DQ_CHK(!DEC, CHK_SAM);  // the check pass stops a run before the decode pass sees such a row
    return;
  }
  const int64_t len = R.end - R.aux_at;
  const uint8_t* A = in.src + R.lin + R.aux_at;
  if (use_slot && len <= TAG_SLOT) {
    uint8_t* slot = stage + (int32_t)threadIdx.x * TAG_STRIDE;
    constexpr int W = TAG_STRIDE % 16 == 0 ? 16 : TAG_STRIDE % 8 == 0 ? 8 : 4;  // the slots' alignment
    int64_t i = 0;
    for (; i + W <= len; i += W) {
      if (W == 16) {
        uint4 w;
        __builtin_memcpy(&w, A + i, 16);
        *reinterpret_cast<uint4*>(slot + i) = w;
      } else if (W == 8) {
        uint2 w;
        __builtin_memcpy(&w, A + i, 8);
        *reinterpret_cast<uint2*>(slot + i) = w;
      } else {
        uint32_t w;
        __builtin_memcpy(&w, A + i, 4);
        *reinterpret_cast<uint32_t*>(slot + i) = w;
      }
    }
    for (; i < len; i++) slot[i] = A[i];
    A = slot;
  }
  const dqa::TagKeys T{K.slot, K.type, in.n_keys};
  uint64_t seen = 0;
  if (DEC) {
    DecodeSink sink{out, K, in.n_keys, n, j};
    const int32_t bad = dqa::tags_walk(A, len, R.aux_at, T, sink, &seen);
    (void)bad;
    DQ_CHK(bad == 0, CHK_SAM);  // the check pass accepted the record
    for (int32_t q = 0; q < in.n_keys; q++)
      if (!(seen >> q & 1)) sink.blank(q);
  } else {
    dqa::NullSink sink;
    const int32_t bad = dqa::tags_walk(A, len, R.aux_at, T, sink, &seen);
    if (bad) atomicMin(&scal[0], dqa::tag_error_key(j, bad));
  }
}

static_assert(TAG_STRIDE >= TAG_SLOT && TAG_STRIDE % 4 == 0 && 256 * TAG_STRIDE <= 48 * 1024,
              "256 slots of whole words");

}  // namespace

DQ_CHK_UNIT(tags)

// 1, or 0 with DQ_TAGS_STAGE=0 in the environment, read at every launch: tools/tags_bench.py runs
// both walks in turn in one process
static int32_t tags_use_slot() {
  const char* e = getenv("DQ_TAGS_STAGE");
  return e && e[0] == '0' && e[1] == 0 ? 0 : 1;
}

void launch_tags_check(TagIn in, unsigned long long* scal, hipStream_t s) {
  if (in.n <= 0 || in.n_keys <= 0 || in.n_keys > dqa::TAG_MAX_KEYS) return;
  hipLaunchKernelGGL(tags_kernel<false>, dim3((unsigned)((in.n + 255) / 256)), dim3(256), 0, s, in, TagCols{}, scal,
                     tags_use_slot());
}

void launch_tags_decode(TagIn in, TagCols out, hipStream_t s) {
  if (in.n <= 0 || in.n_keys <= 0 || in.n_keys > dqa::TAG_MAX_KEYS) return;
  hipLaunchKernelGGL(tags_kernel<true>, dim3((unsigned)((in.n + 255) / 256)), dim3(256), 0, s, in, out, nullptr,
                     tags_use_slot());
}

}  // namespace dq
