// dq_vcf_info.hip -- VCF INFO decode: the INFO column of the variants
// dq_vcf.hip decoded, projected onto the caller's keys as the typed, key-major columns of
// dq_info_batch -- what htsjdk's AbstractVCFCodec.parseInfo leaves for VariantContext.getAttribute
// of those keys.  The per-line rules are dq_vcf_info_core.h; this file holds
// the kernels around them.  They run behind the site decode on its col_end (INFO is
// [col_end[6] + 1, col_end[7]) of a variant's value, no TAB search) and read the resident stream U:
//   check    the first failing (line, key) by a min, every key's largest value count by a max, the
//            Float texts left to the host counted; nothing is stored;
//   decode   the same walk with the widths known, into the columns; the host's Float texts listed.
// The INFO column's length chooses the walk, not the line's: a thread per variant up to INFO_WAVE
// bytes (a block's lines staged in LDS where their span fits, dq_vcf_stage.h), a wave per variant
// above it.  The key table (sorted hashes, offsets, types, bases, widths and up to INFO_IDS_LDS id
// bytes; a longer list's ids, read only behind a hash match, stay in memory) sits in LDS.  Every
// load of a line lies in its INFO column or in the stage; every store is guarded by its key, row
// and element index.
#include <cstdlib>

#if defined(__HIP_DEVICE_COMPILE__)
#define DQV_CHECK(cond) DQ_CHK(cond, CHK_VCF)
#define DQI_CHECK(cond) DQ_CHK(cond, CHK_VCF)
#define DQT_CHECK(cond) DQ_CHK(cond, CHK_VCF)
#else
#define DQV_CHECK(cond) ((void)0)
#define DQI_CHECK(cond) ((void)0)
#define DQT_CHECK(cond) ((void)0)
#endif
#include "dq_internal.h"
#include "dq_vcf_info_core.h"
#include "dq_vcf_stage.h"

namespace dq {
namespace {

// INFO columns longer than this get a wave.  Measured with one sites-only file sent down either
// walk (621 k lines, both passes, 1 / 4 / 12 keys): at 256 bytes of INFO the thread walk takes
// 1.84 / 2.07 / 2.38 ms where the wave walk takes 2.71 / 4.05 / 4.41; at 512 bytes 4.16 / 4.41 / 4.68
// against 3.80 / 4.93 / 5.33; at 1024 bytes 8.36 / 8.60 / 8.90 against 5.30 / 6.38 / 6.82 (DESIGN.md
// section 17).  Above it are the annotation columns (CSQ=, ANN=).
constexpr int32_t INFO_WAVE = 512;
constexpr int32_t INFO_WSLOT = 4096;  // a wave's LDS copy of its INFO column (a longer one is read from memory)

constexpr int32_t INFO_IDS_LDS = 1024;  // id bytes a block keeps in LDS (a longer list's stay in memory)

struct KeyLds {
  uint64_t hash[64];
  int64_t base[64];
  int32_t idx[64];
  int32_t id_off[65];
  int32_t width[64];
  uint8_t type[64];
  uint8_t hflag[64];
  uint8_t ids[INFO_IDS_LDS];
};

// out: the decode pass's columns (their bases and widths), or nullptr.  Ends in a block barrier.
__device__ inline void keys_load(KeyLds& K, const InfoIn& in, const InfoCols* out) {
  const dqt::NameTable& k = in.keys;
  const int t = threadIdx.x;
  if (t < 64) {
    const bool on = t < k.n;
    K.hash[t] = on ? k.hash[t] : ~0ull;
    K.idx[t] = on ? k.idx[t] : 0;
    K.type[t] = on ? in.key_type[t] : 0;
    K.hflag[t] = on ? in.key_hflag[t] : 0;
    K.base[t] = on && out ? out->key_base[t] : -1;
    K.width[t] = on && out ? out->key_width[t] : 0;
  }
  if (t < 65) K.id_off[t] = t <= k.n ? k.name_off[t] : 0;
  const int32_t nb = k.n >= 0 && k.n <= 64 ? k.name_off[k.n] : 0;  // block-uniform
  if (nb <= INFO_IDS_LDS)
    for (int32_t i = t; i < nb; i += (int32_t)blockDim.x) K.ids[i] = k.names[i];
  __syncthreads();
}

__device__ inline dqi::InfoKeys keys_view(const KeyLds& K, const dqt::NameTable& k) {
  const int32_t n = k.n < 64 ? k.n : 64;
  const bool in_lds = n >= 0 && K.id_off[n] <= INFO_IDS_LDS;  // as keys_load decided
  return dqi::InfoKeys{{K.hash, K.idx, K.id_off, in_lds ? K.ids : k.names, n}, K.type, K.hflag};
}

struct CheckSink {
  int32_t* width;  // [K] in memory
  int32_t nk;
  int32_t nhost;
  __device__ void ival(int32_t, int32_t, int32_t) {}
  __device__ void fval(int32_t, int32_t, uint64_t) {}
  __device__ void host(int32_t, int32_t, int32_t, int32_t) { nhost++; }
  __device__ void repeated(int32_t) {}
  __device__ void cell(int32_t q, const dqi::InfoCell& C) {
    DQ_CHK(q >= 0 && q < nk, CHK_VCF);
    // nearly every cell has one value: the load keeps them off the atomic
    if (C.n_values > 1 && q >= 0 && q < nk && C.n_values > __atomic_load_n(&width[q], __ATOMIC_RELAXED))
      atomicMax(&width[q], C.n_values);
  }
};

struct DecodeSink {
  const InfoCols& o;
  const KeyLds& K;
  int32_t nk;
  int64_t n, k;     // rows, this row
  int64_t text0;    // the line's value start in U
  int32_t off0;     // what the walk's positions lack to offsets in the line's value
  int64_t* fix;
  int64_t fix_cap;
  unsigned long long* cnt;
  __device__ bool row(int32_t q) const {
    const bool ok = q >= 0 && q < nk && k >= 0 && k < n;
    DQ_CHK(ok, CHK_VCF);
    return ok;
  }
  __device__ void ival(int32_t q, int32_t j, int32_t v) {
    if (!row(q)) return;
    const int32_t W = K.width[q];
    const int64_t e = K.base[q] + k * W + j;
    const bool ok = j >= 0 && j < W && K.base[q] >= 0 && e < o.n_ival;  // the check pass saw this element
    DQ_CHK(ok, CHK_VCF);
    if (ok) o.ival[e] = v;
  }
  __device__ void fval(int32_t q, int32_t j, uint64_t bits) {
    if (!row(q)) return;
    const int32_t W = K.width[q];
    const int64_t e = K.base[q] + k * W + j;
    const bool ok = j >= 0 && j < W && K.base[q] >= 0 && e < o.n_fval;
    DQ_CHK(ok, CHK_VCF);
    if (ok) o.fval[e] = bits;
  }
  __device__ void host(int32_t q, int32_t j, int32_t at, int32_t len) {
    fix_append<5>(fix, fix_cap, cnt, {q, k, j, text0 + off0 + at, len});
  }
  __device__ void cell(int32_t q, const dqi::InfoCell& C) {
    if (!row(q)) return;
    const int64_t c = (int64_t)q * n + k;
    o.flags[c] = (uint8_t)C.flags;
    o.n_values[c] = C.n_values;
    o.val_off[c] = C.val_off < 0 ? -1 : C.val_off + off0;
    o.val_len[c] = C.val_len;
    const int32_t ty = K.type[q];
    if (ty == dqi::INFO_INTEGER)
      for (int32_t j = C.n_values; j < K.width[q]; j++) ival(q, j, dqi::INFO_I_MISSING);
    else if (ty == dqi::INFO_FLOAT)
      for (int32_t j = C.n_values; j < K.width[q]; j++) fval(q, j, dqi::INFO_F_MISSING_BITS);
  }
  __device__ void repeated(int32_t q) {
    if (row(q)) o.flags[(int64_t)q * n + k] |= (uint8_t)dqi::INFO_REPEATED;
  }
};

// The variant's line and its INFO column [ia, iz) in the line's value; false (a failed check) when
// the lists disagree.
struct InfoLineAt {
  int64_t t, a;
  int32_t len, ia, iz;
};
__device__ inline bool line_at(const InfoIn& in, int64_t j, InfoLineAt* A) {
  if (!kept_line(in.ln, j, &A->t, &A->a, &A->len)) return false;
  A->ia = in.ln.col_end[8 * j + 6] + 1;
  A->iz = in.ln.col_end[8 * j + 7];
  const bool ok = line_in_u(in.ln, A->a, A->len) && A->ia >= 1 && A->ia <= A->iz && A->iz <= A->len;
  DQ_CHK(ok, CHK_VCF);
  return ok;
}

// ---- a thread per variant: INFO columns of up to INFO_WAVE bytes
template <bool DEC>
__global__ __launch_bounds__(256) void info_thread_kernel(InfoIn in, InfoCols out,
                                                           unsigned long long* __restrict__ scal,
                                                           int32_t* __restrict__ width,
                                                           int64_t* __restrict__ fix, int64_t fix_cap,
                                                           int32_t wave_at) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[VCF_STAGE];
  __shared__ KeyLds K;
  keys_load(K, in, DEC ? &out : nullptr);
  const int64_t n = in.ln.n, j0 = (int64_t)blockIdx.x * 256, j = j0 + threadIdx.x;
  const StageSpan sp = stage_block(in.ln, j0, stage);
  InfoLineAt A;
  if (j >= n || !line_at(in, j, &A) || A.iz - A.ia > wave_at) return;  // the longer ones: info_wave_kernel
  const uint8_t* L = stage_line(sp, stage, in.ln.U, A.a, A.len);
  const dqi::InfoKeys T = keys_view(K, in.keys);
  if (DEC) {
    DecodeSink sink{out, K, T.tab.n, n, j, A.a, 0, fix, fix_cap, scal + 2};
    const int32_t bad = dqi::info_line_walk(L, A.ia, A.iz, T, sink);
    (void)bad;
    DQ_CHK(bad < 0, CHK_VCF);  // the check pass accepted the line (a failing cell is stored blank)
  } else {
    CheckSink sink{width, T.tab.n, 0};
    const int32_t bad = dqi::info_line_walk(L, A.ia, A.iz, T, sink);
    if (bad >= 0) atomicMin(&scal[0], dqi::info_error_key(in.ln.lidx[A.t], bad));
    else if (sink.nhost) atomicAdd(&scal[1], (unsigned long long)sink.nhost);
  }
}

// ---- a wave per variant: the long INFO columns
// A wave takes 64 variants at a time, a lane each, and a ballot over their INFO lengths names the
// long ones among them; those it walks one after the other.  The lanes read the column 64 bytes an
// instruction (into the wave's LDS slot on the way when it fits); a lane whose byte opens a piece
// -- the column's first byte, or the one behind a ';' -- hashes that piece's key and looks it up,
// and a requested key's lowest piece offset is settled by a minimum in LDS (the first piece wins), a
// count beside it telling of repeats.  Then lane q decodes key q's winning piece with the cell rules
// of the thread walk and stores its cell, or the blank one: a long value list is walked by its lane
// alone.
template <bool DEC>
__global__ __launch_bounds__(256) void info_wave_kernel(InfoIn in, InfoCols out,
                                                         unsigned long long* __restrict__ scal,
                                                         int32_t* __restrict__ width,
                                                         int64_t* __restrict__ fix, int64_t fix_cap,
                                                         int32_t wave_at) {
  __shared__ KeyLds K;
  __shared__ int32_t first_all[4 * 64], cnt_all[4 * 64];
  __shared__ uint8_t slots[4 * INFO_WSLOT];
  keys_load(K, in, DEC ? &out : nullptr);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int32_t* first = first_all + w * 64;
  int32_t* cnt = cnt_all + w * 64;
  uint8_t* slot = slots + w * INFO_WSLOT;
  const dqi::InfoKeys T = keys_view(K, in.keys);
  const int64_t nchunk = (in.ln.n + 63) / 64, nwave = (int64_t)gridDim.x * 4;
  int32_t nhost = 0;
  for (int64_t c = (int64_t)blockIdx.x * 4 + w; c < nchunk; c += nwave) {
    const int64_t jm = c * 64 + lane;
    int32_t mylen = 0;
    if (jm < in.ln.n) mylen = in.ln.col_end[8 * jm + 7] - in.ln.col_end[8 * jm + 6] - 1;
    unsigned long long m = __ballot(mylen > wave_at);
    while (m) {  // wave-uniform
      const int64_t j = c * 64 + (int64_t)__builtin_ctzll(m);
      m &= m - 1;
      InfoLineAt A;
      if (!line_at(in, j, &A)) continue;
      // positions from here on count from the INFO column's first byte
      const uint8_t* P = in.ln.U + A.a + A.ia;
      const int32_t il = A.iz - A.ia;
      const bool staged = il <= INFO_WSLOT;  // wave-uniform
      first[lane] = 0x7fffffff;
      cnt[lane] = 0;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      for (int32_t base = 0; base < il; base += 64) {
        const int32_t x = base + lane;
        if (x >= il) continue;
        if (staged) slot[x] = P[x];
        if (x == 0 || P[x - 1] == ';') {
          const int32_t ke = dqi::info_key_end(P, x, il);
          const int32_t q = dqt::name_lookup(T.tab, P + x, ke - x);
          if (q >= 0) {
            atomicMin(&first[q], x);
            atomicAdd(&cnt[q], 1);
          }
        }
      }
      // the wave's LDS stores and atomics above are read by other lanes below
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (lane < T.tab.n) {
        const int32_t q = lane, f = first[q];
        const uint8_t* W = staged ? slot : P;
        dqi::InfoCell C = dqi::info_blank();
        const bool has = f >= 0 && f < il;
        DQ_CHK(has || f == 0x7fffffff, CHK_VCF);
        if (DEC) {
          DecodeSink sink{out, K, T.tab.n, in.ln.n, j, A.a, A.ia, fix, fix_cap, scal + 2};
          if (has) {
            const int32_t ke = dqi::info_key_end(W, f, il);
            const int32_t pe = ke < il && W[ke] == '=' ? dqi::info_piece_end(W, ke, il) : ke;
            dqi::InfoKeySink<DecodeSink> ks{sink, q};
            const bool ok = dqi::info_cell(W, ke, pe, K.type[q], K.hflag[q] != 0, &C, ks);
            (void)ok;
            DQ_CHK(ok, CHK_VCF);  // the check pass accepted the cell
          }
          sink.cell(q, C);
          if (has && cnt[q] > 1) sink.repeated(q);
        } else if (has) {
          CheckSink sink{width, T.tab.n, 0};
          const int32_t ke = dqi::info_key_end(W, f, il);
          const int32_t pe = ke < il && W[ke] == '=' ? dqi::info_piece_end(W, ke, il) : ke;
          dqi::InfoKeySink<CheckSink> ks{sink, q};
          if (!dqi::info_cell(W, ke, pe, K.type[q], K.hflag[q] != 0, &C, ks))
            atomicMin(&scal[0], dqi::info_error_key(in.ln.lidx[A.t], q));
          else
            nhost += sink.nhost;
          sink.cell(q, C);
        }
      }
      // the slot and the two lists are the next variant's: its stores wait for this one's loads
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  }
  if (!DEC && nhost) atomicAdd(&scal[1], (unsigned long long)nhost);
}

}  // namespace

DQ_CHK_UNIT(vcfinfo)

// INFO_WAVE, or DQ_INFO_WAVE from the environment: tools/vcf_info_bench.py sends one file down
// either walk with it (0: every variant to the wave walk; a large value: every one to the threads)
static int32_t info_wave_at() {
  static const int32_t at = [] {
    const char* e = getenv("DQ_INFO_WAVE");
    const long v = e && *e ? strtol(e, nullptr, 10) : (long)INFO_WAVE;
    return (int32_t)(v < 0 ? 0 : v > 0x7fffffff ? 0x7fffffff : v);
  }();
  return at;
}

template <bool DEC>
static void launch_info(InfoIn in, InfoCols out, unsigned long long* scal, int32_t* width, int64_t* fix,
                        int64_t fix_cap, hipStream_t s) {
  if (in.ln.n <= 0 || in.keys.n <= 0 || in.keys.n > dqi::INFO_MAX_KEYS) return;
  hipLaunchKernelGGL(info_thread_kernel<DEC>, dim3((unsigned)((in.ln.n + 255) / 256)), dim3(256), 0, s, in, out,
                     scal, width, fix, fix_cap, info_wave_at());
  const int64_t g = ((in.ln.n + 63) / 64 + 3) / 4;  // 4 waves per block, 64 variants a wave and step
  hipLaunchKernelGGL(info_wave_kernel<DEC>, dim3((unsigned)(g > 2048 ? 2048 : g)), dim3(256), 0, s, in, out,
                     scal, width, fix, fix_cap, info_wave_at());
}

void launch_info_check(InfoIn in, unsigned long long* scal, int32_t* width, hipStream_t s) {
  launch_info<false>(in, InfoCols{}, scal, width, nullptr, 0, s);
}

void launch_info_decode(InfoIn in, InfoCols out, int64_t* fix, int64_t fix_cap, unsigned long long* scal,
                        hipStream_t s) {
  launch_info<true>(in, out, scal, nullptr, fix, fix_cap, s);
}

}  // namespace dq
