// EmbeddingBag forward from an 8-bit row-wise quantized table (`q8`, include/ce_api.h) for gfx950: evaluation and
// serving only, there is no backward.  A row of D elements is 16 + D bytes -- scale, bias (fp32), 8 zero bytes, D uint8
// codes -- i.e. 4 + D / 4 dwords, and element i is fmaf((float)code[i], scale, bias): one explicit fma.
// The two kernels are k_bag_fwd and k_bag_fwd_keys of ce_bag.hip with another row type and the same lane geometry: a
// lane group of G lanes owns a row, a lane owns 4 consecutive elements per chunk -- here ONE dword of codes, four
// byte-to-float conversions and four fmas -- and stores them as 16 bytes of fp32 or 8 bytes of a 16-bit type,
// non-temporally.  Rows in flight are held as codes (1 dword per chunk, not 4), so the kernels need fewer registers
// than the fp32 forms at the same depth.
// scale and bias are one 8-byte load per row that EVERY lane of the group issues at the same address: the lanes of
// one load instruction that hit one address are served by one request, and it sits in the same 128-byte line as the
// row's first codes, which the group fetches anyway -- while one lane loading and the others shuffling would put a
// ds_bpermute (G up to 64 lanes: no DPP form) between every row load and its first use.
// A 144-byte row (D = 128) always spans two 128-byte lines: the format's price.
#include <algorithm>

#include "ce_common.h"

namespace ce {
namespace {

struct Q8Params {
  const uint32_t* weight;   // the table as dwords: row r starts at r * rowdw
  void* dst;                // out (elements of the activation type AT)
  const int64_t* indices;
  const void* offsets;
  const float* psw;
  const unsigned long long* keys;   // key-driven form: source-row keys of ce_bag_presort_window_src
  int64_t nnz;
  int32_t num_bags;
  int32_t rowlen;           // 4-element chunks per row (dim / 4)
  int32_t rowdw;            // dwords per row (4 + rowlen)
  int32_t g_log2;           // log2(lanes per group)
  int32_t off64;
  int32_t include_last;
  int32_t mode;
  int32_t hookF;            // 0 = plain [num_bags, D]
  int32_t hookB;            // num_bags / hookF
  uint32_t num_rows;        // lookups outside [0, num_rows) take no part
};

typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr int kHeaderDw = CE_Q8_HEADER_BYTES / 4;
constexpr int kIdxStage = 2048;              // indices of one 64-bag tile staged in LDS (8 KB per wave)
constexpr int kSegLen = 16384;               // the window presort's segment (keys are padded to whole segments)
constexpr unsigned kExclFlag = 0x80000000u;  // owner-exclusive keys carry it in the low word: not part of the row

__device__ __forceinline__ int ld_off(const Q8Params& p, int i) {
  if (p.offsets == nullptr) return i;
  return p.off64 ? (int)((const int64_t*)p.offsets)[i] : ((const int32_t*)p.offsets)[i];
}
__device__ __forceinline__ int bag_end(const Q8Params& p, int b) {
  return (p.include_last || b + 1 < p.num_bags) ? ld_off(p, b + 1) : (int)p.nnz;
}
// row of the [B, F, D] output that feature-major bag g = f*B + b lands in
__device__ __forceinline__ int64_t out_row(const Q8Params& p, int g) {
  if (p.hookF == 0) return g;
  int f = g / p.hookB;
  int b = g - f * p.hookB;
  return (int64_t)b * p.hookF + f;
}

template <typename T>
__device__ __forceinline__ void store_out(T* p, T v) {
  __builtin_nontemporal_store(v, p);
}

// a lane's 4 elements of a row: byte k of the code dword is element k (v_cvt_f32_ubyte0..3), then the fma
__device__ __forceinline__ f32x4 dequant4(uint32_t c, f32x2 sb) {
  return f32x4{__builtin_fmaf((float)(c & 0xffu), sb.x, sb.y), __builtin_fmaf((float)((c >> 8) & 0xffu), sb.x, sb.y),
               __builtin_fmaf((float)((c >> 16) & 0xffu), sb.x, sb.y), __builtin_fmaf((float)(c >> 24), sb.x, sb.y)};
}

// The general forward.  STAGE: tiles with multi-id bags stage their indices in LDS; U: rows in flight per lane group
// of a single-id tile; the general tile loop keeps 8.  A row that takes no part is held as codes 0, scale 0, bias 0.
template <int NCH, bool STAGE, int U, typename AT>
__global__ __launch_bounds__(256) void k_bag_fwd_q8(Q8Params p) {
  using A = Act<AT, f32x4>;
  __shared__ int lds_idx[STAGE ? 4 : 1][STAGE ? kIdxStage : 1];
  const int lane = threadIdx.x & 63;
  const int G = 1 << p.g_log2;
  const int gpw = 64 >> p.g_log2;
  const int grp = lane >> p.g_log2;
  const int gl = lane & (G - 1);
  const int wpb = blockDim.x >> 6;
  const int64_t wave = (int64_t)blockIdx.x * wpb + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * wpb;
  const uint32_t* __restrict__ W = p.weight;
  typename A::V* __restrict__ O = (typename A::V*)p.dst;
  const int rowlen = p.rowlen;
  const int rowdw = p.rowdw;
  const int ntiles = (p.num_bags + 63) >> 6;

  for (int64_t tile = wave; tile < ntiles; tile += nwaves) {
    const int b0 = (int)(tile << 6);
    const int nb = min(64, p.num_bags - b0);
    int lo = 0, hi = 0;
    if (lane < nb) {
      lo = ld_off(p, b0 + lane);
      hi = bag_end(p, b0 + lane);
    }
    const bool single = (hi - lo == 1) || (lane >= nb);
    if (__all(single)) {
      // ---- single-id tile: indexed row dequantization, U rows in flight per lane group
      int idx = 0;
      float w = 1.f;
      if (lane < nb) {
        idx = (int)p.indices[lo];
        if (p.psw) w = p.psw[lo];
      }
      for (int base = 0; base < nb; base += gpw * U) {
        uint32_t q[U][NCH];
        f32x2 sb[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int bi = base + u * gpw + grp;
          const int ri = __shfl(idx, bi & 63);
          const bool on = bi < nb && (uint32_t)ri < p.num_rows;
          const uint32_t* row = W + (int64_t)ri * rowdw;
          sb[u] = f32x2{0.f, 0.f};
          if (on) sb[u] = *(const f32x2*)row;
#pragma unroll
          for (int c = 0; c < NCH; ++c) {
            const int ch = gl + c * G;
            q[u][c] = 0u;
            if (on && ch < rowlen) q[u][c] = row[kHeaderDw + ch];
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int bi = base + u * gpw + grp;
          const float wi = __shfl(w, bi & 63);
          if (bi < nb) {
            const int64_t orow = out_row(p, b0 + bi);
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
              const int ch = gl + c * G;
              if (ch < rowlen) {
                const f32x4 v = dequant4(q[u][c], sb[u]);
                const f32x4 val = p.psw ? v * wi : v;
                store_out(&O[orow * rowlen + ch], A::down(val));
              }
            }
          }
        }
      }
    } else {
      // ---- general tile: the 64 bags' indices are one contiguous range, staged in LDS with coalesced loads; each lane
      // group walks its bag with 8 rows in flight
      const int t_lo = __shfl(lo, 0);
      const int t_hi = __shfl(hi, nb - 1);
      const int t_n = t_hi - t_lo;
      const bool staged = STAGE && t_n <= kIdxStage;
      int* sidx = &lds_idx[STAGE ? (threadIdx.x >> 6) : 0][0];
      if (staged) {
        for (int k = lane; k < t_n; k += 64) sidx[k] = (int)p.indices[t_lo + k];
      }
      __builtin_amdgcn_wave_barrier();
      for (int base = 0; base < nb; base += gpw) {
        const int bi = base + grp;
        int blo = __shfl(lo, bi & 63);
        int bhi = __shfl(hi, bi & 63);
        if (bi >= nb) blo = bhi = 0;
        f32x4 acc[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) acc[c] = vzero<f32x4>();
        for (int j = blo; j < bhi; j += 8) {
          int r[8];
          float w[8];
#pragma unroll
          for (int t = 0; t < 8; ++t) {
            r[t] = -1;
            w[t] = 1.f;
            if (j + t < bhi) {
              r[t] = staged ? sidx[j + t - t_lo] : (int)p.indices[j + t];
              if (p.psw) w[t] = p.psw[j + t];
            }
          }
          uint32_t q[8][NCH];
          f32x2 sb[8];
#pragma unroll
          for (int t = 0; t < 8; ++t) {
            const bool on = (uint32_t)r[t] < p.num_rows;
            const uint32_t* row = W + (int64_t)r[t] * rowdw;
            sb[t] = f32x2{0.f, 0.f};
            if (on) sb[t] = *(const f32x2*)row;
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
              const int ch = gl + c * G;
              q[t][c] = 0u;
              if (on && ch < rowlen) q[t][c] = row[kHeaderDw + ch];
            }
          }
#pragma unroll
          for (int t = 0; t < 8; ++t) {
            if (j + t < bhi) {
#pragma unroll
              for (int c = 0; c < NCH; ++c) {
                const f32x4 v = dequant4(q[t][c], sb[t]);
                acc[c] = p.psw ? acc[c] + v * w[t] : acc[c] + v;
              }
            }
          }
        }
        if (p.mode == CE_MODE_MEAN && bhi - blo > 1) {
          const float inv = 1.f / (float)(bhi - blo);
#pragma unroll
          for (int c = 0; c < NCH; ++c) acc[c] = acc[c] * inv;
        }
        if (bi < nb) {
          const int64_t orow = out_row(p, b0 + bi);
#pragma unroll
          for (int c = 0; c < NCH; ++c) {
            const int ch = gl + c * G;
            if (ch < rowlen) store_out(&O[orow * rowlen + ch], A::down(acc[c]));
          }
        }
      }
    }
  }
}

// The key-driven forward (k_bag_fwd_keys' walk: contiguous equal shares of the window's keys, staged through a
// group-private LDS slice, R keys per step).  A row is loaded and dequantized ONCE per run of equal rows -- `prev` is
// the fp32 row -- and stored, rounded, to every output row of the run.  An ignored lookup (row 0xffffffff) gets a zero
// row; padding keys (~0) are skipped.
template <int NCH, int R, typename AT>
__global__ __launch_bounds__(256, 4) void k_bag_fwd_keys_q8(Q8Params p, int64_t total) {
  using A = Act<AT, f32x4>;
  __shared__ unsigned long long lk[256 * (R > 4 ? R : 4)];
  const int tid = threadIdx.x;
  const int G = 1 << p.g_log2;
  const int ngroups = 256 >> p.g_log2;
  const int grp = tid >> p.g_log2;
  const int gl = tid & (G - 1);
  const int rowlen = p.rowlen;
  const int rowdw = p.rowdw;
  const uint32_t* __restrict__ W = p.weight;
  typename A::V* __restrict__ O = (typename A::V*)p.dst;
  const unsigned long long* __restrict__ keys = p.keys;
  const int64_t all_groups = (int64_t)gridDim.x * ngroups;
  const int64_t round = R > 16 ? R : 16;
  const int64_t share = ((total + all_groups - 1) / all_groups + round - 1) / round * round;
  const int64_t s0 = ((int64_t)blockIdx.x * ngroups + grp) * share;
  const int64_t s1 = min(total, s0 + share);
  if (s0 >= s1) return;
  const int kc = 4 * G > R ? 4 * G : R;
  unsigned long long* mylk = lk + grp * kc;
  f32x4 prev[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) prev[c] = vzero<f32x4>();
  uint32_t prev_row = 0xffffffffu;          // "ignored": a zero row, which is what prev holds
  for (int64_t c0 = s0; c0 < s1; c0 += kc) {
    for (int k = gl; k < kc; k += G) mylk[k] = c0 + k < s1 ? keys[c0 + k] : ~0ull;
    const int64_t c1 = min(s1, c0 + kc);
    for (int64_t q0 = c0; q0 < c1; q0 += R) {
      uint32_t q[R][NCH];
      f32x2 sb[R];
      uint32_t heads = 0;
      uint32_t last = prev_row;
#pragma unroll
      for (int t = 0; t < R; ++t) {
        const unsigned long long k = mylk[(int)(q0 - c0) + t];
        const bool on = k != ~0ull;
        const uint32_t rw = (uint32_t)(k >> 32);
        const bool head = on && rw != last;
        if (on) last = rw;
        if (head) heads |= 1u << t;
        const bool ld = head && rw < p.num_rows;
        const uint32_t* row = W + (int64_t)rw * rowdw;
        sb[t] = f32x2{0.f, 0.f};
        if (ld) sb[t] = *(const f32x2*)row;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const int ch = gl + c * G;
          q[t][c] = 0u;
          if (ld && ch < rowlen) q[t][c] = row[kHeaderDw + ch];
        }
      }
      __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0): every head of the step has arrived
#pragma unroll
      for (int t = 0; t < R; ++t) {
        const unsigned long long k = mylk[(int)(q0 - c0) + t];
        if (k == ~0ull) continue;              // padding (group-uniform)
        if ((heads >> t) & 1) {
#pragma unroll
          for (int c = 0; c < NCH; ++c) prev[c] = dequant4(q[t][c], sb[t]);   // a new run: dequantized once
        }
        const int64_t orow = (int64_t)((uint32_t)k & ~kExclFlag);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const int ch = gl + c * G;
          if (ch < rowlen) store_out(&O[orow * rowlen + ch], A::down(prev[c]));
        }
      }
      prev_row = last;
    }
  }
}

template <int NCH> constexpr int tile_unroll_q8() { return NCH == 1 ? 16 : (NCH == 2 ? 4 : 2); }
template <int NCH> constexpr int keys_unroll_q8() { return NCH == 1 ? 16 : (NCH == 2 ? 8 : 4); }

template <int N_> struct Chunks { static constexpr int NCH = N_; };
template <typename F> void for_q8(int nch, int act, F&& f) {
  auto chunks = [&](auto a) {
    if (nch == 1) f(Chunks<1>{}, a); else if (nch == 2) f(Chunks<2>{}, a); else f(Chunks<4>{}, a);
  };
  for_act(act, chunks);
}

// what both entries refuse from their arguments alone, and the row geometry (the fp32 vector form's: dim / 4 chunks)
int q8_check(int32_t dim, const void* weight, const void* out, int32_t act_dtype, int64_t num_rows, RowGeom& r) {
  CE_REQUIRE(weight && out, CE_ERR_INVALID, "null pointer");
  CE_REQUIRE_ROWS(num_rows);
  CE_REQUIRE(al16(weight) && act_aligned(out, act_dtype), CE_ERR_INVALID,
             "a q8 table must be 16-byte aligned and its output on the vector boundary");
  return row_geometry(dim, true, r);
}

}  // namespace
}  // namespace ce

using namespace ce;

#define CE_REQUIRE_Q8_DIM(dim)                                                         \
  CE_REQUIRE(ce_q8_row_bytes(dim) != 0, CE_ERR_UNSUPPORTED,                            \
             "a q8 table needs dim %% 16 == 0 and 16 <= dim <= 1024 (got %d)", (int)(dim))

extern "C" int ce_bag_forward_q8(const void* weight, int64_t num_rows, int32_t dim, const int64_t* indices, int64_t nnz,
                                 const void* offsets, int32_t offsets_are_i64, int64_t num_bags,
                                 int32_t include_last_offset, const float* per_sample_weights, int32_t mode,
                                 int64_t hook_features, void* out, int32_t act_dtype, ce_stream_t stream) {
  CE_REQUIRE_ACT(act_dtype);
  CE_REQUIRE_Q8_DIM(dim);
  if (num_bags == 0) return CE_OK;
  CE_REQUIRE(indices || nnz == 0, CE_ERR_INVALID, "null pointer");
  CE_REQUIRE(offsets || num_bags == nnz, CE_ERR_INVALID,
             "offsets == NULL states one id per bag (offsets = arange): num_bags must equal nnz");
  CE_REQUIRE(num_bags >= 0 && nnz >= 0, CE_ERR_INVALID, "negative sizes");
  CE_REQUIRE(num_bags < (int64_t)INT32_MAX - 64 && nnz < (int64_t)INT32_MAX, CE_ERR_UNSUPPORTED,
             "more than 2^31 bags / lookups in one launch");
  CE_REQUIRE(mode == CE_MODE_SUM || mode == CE_MODE_MEAN, CE_ERR_UNSUPPORTED, "mode must be sum or mean");
  CE_REQUIRE(!(mode == CE_MODE_MEAN && per_sample_weights), CE_ERR_INVALID, "per_sample_weights needs mode='sum'");
  CE_REQUIRE(hook_features >= 0 && (hook_features == 0 || num_bags % hook_features == 0), CE_ERR_INVALID,
             "hook_features must divide num_bags");
  RowGeom r;
  int rc = q8_check(dim, weight, out, act_dtype, num_rows, r);
  if (rc) return rc;
  Q8Params p{};
  p.weight = (const uint32_t*)weight;
  p.dst = out;
  p.indices = indices;
  p.offsets = offsets;
  p.psw = per_sample_weights;
  p.nnz = nnz;
  p.num_bags = (int32_t)num_bags;
  p.rowlen = r.rowlen;
  p.rowdw = kHeaderDw + r.rowlen;
  p.g_log2 = r.g_log2;
  p.off64 = offsets_are_i64;
  p.include_last = include_last_offset;
  p.mode = mode;
  p.hookF = (int32_t)hook_features;
  p.hookB = hook_features ? (int32_t)(num_bags / hook_features) : 0;
  p.num_rows = (uint32_t)num_rows;
  dim3 grid(grid_for(cdiv(num_bags, 64), 4)), block(256);
  const bool stage = nnz != num_bags;      // multi-id bags possible
  hipStream_t s = (hipStream_t)stream;
  for_q8(r.nch, act_dtype, [&](auto l, auto a) {
    using AT = typename decltype(a)::AT;
    constexpr int N = decltype(l)::NCH, U = tile_unroll_q8<N>();
    if (stage) hipLaunchKernelGGL((k_bag_fwd_q8<N, true, U, AT>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((k_bag_fwd_q8<N, false, U, AT>), grid, block, 0, s, p);
  });
  CE_LAUNCH_CHECK();
  return CE_OK;
}

extern "C" int ce_bag_forward_src_keys_q8(const void* weight, int64_t num_rows, int32_t dim, int64_t nnz,
                                          const uint64_t* src_keys, void* out, int32_t act_dtype, ce_stream_t stream) {
  CE_REQUIRE_ACT(act_dtype);
  CE_REQUIRE_Q8_DIM(dim);
  if (nnz == 0) return CE_OK;
  CE_REQUIRE(src_keys, CE_ERR_INVALID, "null pointer");
  CE_REQUIRE(nnz > 0, CE_ERR_INVALID, "negative sizes");
  CE_REQUIRE(nnz < (int64_t)INT32_MAX, CE_ERR_UNSUPPORTED, "more than 2^31 lookups in one launch");
  RowGeom r;
  int rc = q8_check(dim, weight, out, act_dtype, num_rows, r);
  if (rc) return rc;
  Q8Params p{};
  p.weight = (const uint32_t*)weight;
  p.dst = out;
  p.keys = (const unsigned long long*)src_keys;
  p.nnz = nnz;
  p.rowlen = r.rowlen;
  p.rowdw = kHeaderDw + r.rowlen;
  p.g_log2 = r.g_log2;
  p.num_rows = (uint32_t)num_rows;
  const int64_t total = cdiv(nnz, kSegLen) * kSegLen;       // keys are padded to whole segments
  // 16 workgroups per CU, like the fp32 form; small inputs: one share of >= 16 keys per lane group
  const int ngroups = 256 >> p.g_log2;
  const int64_t shares = cdiv(total, (int64_t)ngroups * 16);
  const dim3 g((unsigned)std::max<int64_t>(1, std::min<int64_t>((int64_t)kNumCU * 16, shares))), b(256);
  hipStream_t s = (hipStream_t)stream;
  for_q8(r.nch, act_dtype, [&](auto l, auto a) {
    using AT = typename decltype(a)::AT;
    constexpr int N = decltype(l)::NCH, R = keys_unroll_q8<N>();
    hipLaunchKernelGGL((k_bag_fwd_keys_q8<N, R, AT>), g, b, 0, s, p, total);
  });
  CE_LAUNCH_CHECK();
  return CE_OK;
}
