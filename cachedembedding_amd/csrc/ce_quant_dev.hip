// Device-side quantizer of the row-wise quantized table formats `q8` and `q4`: the rows ce_host_quantize_q8 / _q4
// (ce_quant.cpp) write, byte for byte, from rows that already sit in device memory.  The formats, the formula and what
// is refused are stated once, in include/ce_api.h.
//
// The arithmetic is the host's: fp32 IEEE, one rounding per operation, nothing contracted (the pragma below), plain `/`
// (hipcc's default correctly rounded divide, subnormal operands and quotients included), rintf for the ties-to-even
// rounding.  No fast-math form of anything is used in this file.
//
// Lane geometry, the bag kernels' (row_geometry, ce_common.h): G <= 64 lanes own one row, a lane holds the 4 consecutive
// elements of chunk gl + k * G for k < NCH <= 4, a row never leaves a wave.  min / max are butterflies of shuffles inside
// the group, "is every element finite" is one ballot; no LDS, no barrier.
#include <float.h>
#include <math.h>

#include "ce_common.h"

#pragma clang fp contract(off)

namespace ce {

typedef uint16_t u16x4 __attribute__((ext_vector_type(4)));

// exact up-conversions of the 16-bit source types, in integer arithmetic (ce_quant.cpp's)
__device__ __forceinline__ float qd_bf16_to_f32(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }
__device__ __forceinline__ float qd_f16_to_f32(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
  const uint32_t e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
  uint32_t x;
  if (e == 0x1fu) x = sign | 0x7f800000u | (m << 13);                      // inf / NaN
  else if (e != 0) x = sign | ((e + 112u) << 23) | (m << 13);
  else x = __float_as_uint((float)m * (1.0f / 16777216.0f)) | sign;       // subnormal half: m * 2^-24, exact
  return __uint_as_float(x);
}

// a lane's 4 elements of one chunk, as fp32: 16 bytes of an fp32 source, 8 bytes of a 16-bit one
struct SrcF32 {
  typedef f32x4 V;
  static __device__ __forceinline__ f32x4 up(V a) { return a; }
};
struct SrcBF16 {
  typedef u16x4 V;
  static __device__ __forceinline__ f32x4 up(V a) {
    return f32x4{qd_bf16_to_f32(a.x), qd_bf16_to_f32(a.y), qd_bf16_to_f32(a.z), qd_bf16_to_f32(a.w)};
  }
};
struct SrcF16 {
  typedef u16x4 V;
  static __device__ __forceinline__ f32x4 up(V a) {
    return f32x4{qd_f16_to_f32(a.x), qd_f16_to_f32(a.y), qd_f16_to_f32(a.z), qd_f16_to_f32(a.w)};
  }
};

__device__ __forceinline__ uint32_t qd_code(float x, float lo, float scale, float top) {
  const float d = x - lo;
  float t = rintf(d / scale);                              // ties to even (the default rounding mode)
  t = t < 0.0f ? 0.0f : (t > top ? top : t);
  return (uint32_t)(int)t;
}

__global__ void k_quant_first_bad_init(int64_t* first_bad) { *first_bad = INT64_MAX; }

// BITS = 8: a chunk's codes are one dword at byte 16 + 4 * chunk of the row -- 4 contiguous bytes per lane.
// BITS = 4: they are 16 bits at byte 16 + 2 * chunk; the lanes gl and gl ^ 1 hold neighbouring chunks (G and rowlen are
// even), the even one stores the dword of both.
template <typename S, int NCH, int BITS>
__global__ __launch_bounds__(256) void k_quantize_rows(const typename S::V* __restrict__ src, int64_t n_rows, int rowlen,
                                                       int g_log2, uint8_t* __restrict__ dst, int64_t row_bytes,
                                                       unsigned long long* first_bad) {
  constexpr float top = BITS == 4 ? 15.0f : 255.0f;
  const int G = 1 << g_log2;
  const int lane = threadIdx.x & 63;
  const int gl = threadIdx.x & (G - 1);
  const unsigned long long group_mask = (G == 64 ? ~0ull : ((1ull << G) - 1ull)) << (lane & ~(G - 1));
  const int64_t gstride = ((int64_t)gridDim.x * blockDim.x) >> g_log2;
  for (int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> g_log2; r < n_rows; r += gstride) {
    const typename S::V* row = src + r * rowlen;
    f32x4 x[NCH];
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int c = gl + k * G;
      if (c < rowlen) x[k] = S::up(row[c]);
    }
    // lo is the FIRST element equal to the minimum, in index order, as the host's `lo = v < lo ? v : lo` leaves it (the
    // sign of a zero minimum is stored): (value, index) pairs, the lower index wins among equals.  A lane's elements come
    // in ascending index order, so `<` alone keeps its first.
    float lo = INFINITY, hi = -INFINITY;
    int li = INT32_MAX;
    bool bad = false;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int c = gl + k * G;
      if (c < rowlen) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float v = x[k][j];
          bad |= !(fabsf(v) <= FLT_MAX);                   // NaN and +-inf
          if (v < lo) { lo = v; li = 4 * c + j; }
          hi = v > hi ? v : hi;
        }
      }
    }
    for (int m = 1; m < G; m <<= 1) {
      const float olo = __shfl_xor(lo, m), ohi = __shfl_xor(hi, m);
      const int oli = __shfl_xor(li, m);
      if (olo < lo || (olo == lo && oli < li)) { lo = olo; li = oli; }
      hi = ohi > hi ? ohi : hi;
    }
    const float range = hi - lo;
    bad |= !(range <= FLT_MAX);
    if ((__ballot(bad) & group_mask) != 0ull) {            // (a bad row's destination is unspecified: left as it is)
      if (gl == 0) atomicMin(first_bad, (unsigned long long)r);
      continue;
    }
    float scale = range / top;
    const bool flat = scale == 0.0f;
    if (flat) scale = 0.0f;                                // (never -0)
    uint8_t* out = dst + r * row_bytes;
    if (gl == 0) *(uint4*)out = uint4{__float_as_uint(scale), __float_as_uint(lo), 0u, 0u};
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int c = gl + k * G;
      uint32_t q = 0u;
      if (c < rowlen && !flat) {
        if (BITS == 8) {
          q = qd_code(x[k].x, lo, scale, top) | (qd_code(x[k].y, lo, scale, top) << 8) |
              (qd_code(x[k].z, lo, scale, top) << 16) | (qd_code(x[k].w, lo, scale, top) << 24);
        } else {
          q = qd_code(x[k].x, lo, scale, top) | (qd_code(x[k].y, lo, scale, top) << 4) |
              (qd_code(x[k].z, lo, scale, top) << 8) | (qd_code(x[k].w, lo, scale, top) << 12);
        }
      }
      if (BITS == 8) {
        if (c < rowlen) *(uint32_t*)(out + CE_Q8_HEADER_BYTES + 4 * c) = q;
      } else {
        const uint32_t odd = __shfl_xor(q, 1);             // (outside every condition: both lanes of the pair take part)
        if (c < rowlen && (gl & 1) == 0) *(uint32_t*)(out + CE_Q4_HEADER_BYTES + 2 * c) = q | (odd << 16);
      }
    }
  }
}

struct QdQ8 {
  static constexpr int kBits = 8;
  static constexpr const char* kDimMsg = "a q8 table needs dim %% 16 == 0 and 16 <= dim <= 1024 (got %d)";
  static bool dim_ok(int32_t dim) { return dim >= 16 && dim <= 1024 && dim % 16 == 0; }
  static int64_t row_bytes(int32_t dim) { return CE_Q8_HEADER_BYTES + (int64_t)dim; }
};
struct QdQ4 {
  static constexpr int kBits = 4;
  static constexpr const char* kDimMsg = "a q4 table needs dim %% 32 == 0 and 32 <= dim <= 1024 (got %d)";
  static bool dim_ok(int32_t dim) { return dim >= 32 && dim <= 1024 && dim % 32 == 0; }
  static int64_t row_bytes(int32_t dim) { return CE_Q4_HEADER_BYTES + (int64_t)dim / 2; }
};

template <typename P>
static int quantize_rows_dev(const void* src, int32_t src_dtype, int64_t n_rows, int32_t dim, void* dst,
                             int64_t* first_bad, ce_stream_t stream) {
  // the host entries' checks, in their order and with their words; nothing below them has touched HIP
  CE_REQUIRE(src_dtype == CE_ACT_F32 || src_dtype == CE_ACT_BF16 || src_dtype == CE_ACT_F16, CE_ERR_INVALID,
             "src_dtype %d: CE_ACT_F32, CE_ACT_BF16 or CE_ACT_F16", (int)src_dtype);
  CE_REQUIRE(P::dim_ok(dim), CE_ERR_UNSUPPORTED, P::kDimMsg, (int)dim);
  CE_REQUIRE(n_rows >= 0, CE_ERR_INVALID, "negative n_rows");
  if (n_rows == 0) return CE_OK;
  CE_REQUIRE(src && dst && first_bad, CE_ERR_INVALID, "null pointer");
  CE_REQUIRE(act_aligned(src, src_dtype), CE_ERR_INVALID, "src must be %d-byte aligned",
             src_dtype == CE_ACT_F32 ? 16 : 8);
  CE_REQUIRE(al16(dst), CE_ERR_INVALID, "dst must be 16-byte aligned");
  CE_REQUIRE((((uintptr_t)first_bad) & 7) == 0, CE_ERR_INVALID, "first_bad must be 8-byte aligned");
  RowGeom g;
  int rc = row_geometry(dim, true, g);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_quant_first_bad_init, dim3(1), dim3(1), 0, s, first_bad);
  CE_LAUNCH_CHECK();
  const int blocks = grid_for(n_rows, 256 >> g.g_log2);
  auto launch = [&](auto st, auto nch) {
    using S = decltype(st);
    hipLaunchKernelGGL((k_quantize_rows<S, decltype(nch)::value, P::kBits>), dim3(blocks), dim3(256), 0, s,
                       (const typename S::V*)src, n_rows, g.rowlen, g.g_log2, (uint8_t*)dst, P::row_bytes(dim),
                       (unsigned long long*)first_bad);
  };
  auto by_nch = [&](auto st) {
    if (g.nch == 1) launch(st, std::integral_constant<int, 1>{});
    else if (g.nch == 2) launch(st, std::integral_constant<int, 2>{});
    else launch(st, std::integral_constant<int, 4>{});
  };
  if (src_dtype == CE_ACT_F32) by_nch(SrcF32{});
  else if (src_dtype == CE_ACT_BF16) by_nch(SrcBF16{});
  else by_nch(SrcF16{});
  CE_LAUNCH_CHECK();
  return CE_OK;
}

}  // namespace ce

extern "C" int ce_quantize_rows_q8(const void* src, int32_t src_dtype, int64_t n_rows, int32_t dim, void* dst,
                                   int64_t* first_bad, ce_stream_t stream) {
  return ce::quantize_rows_dev<ce::QdQ8>(src, src_dtype, n_rows, dim, dst, first_bad, stream);
}
extern "C" int ce_quantize_rows_q4(const void* src, int32_t src_dtype, int64_t n_rows, int32_t dim, void* dst,
                                   int64_t* first_bad, ce_stream_t stream) {
  return ce::quantize_rows_dev<ce::QdQ4>(src, src_dtype, n_rows, dim, dst, first_bad, stream);
}
