// Host-side quantizer / dequantizer of the row-wise quantized table formats `q8` (8 bits) and `q4` (4 bits): one
// template over the format (plain C++, no HIP: it builds on its own with a small main that supplies ce::set_error and
// ce_cpu_budget).  The formats, the formula and what is refused are stated once, in include/ce_api.h; the arithmetic
// here is fp32 IEEE, one rounding per operation, nothing contracted: the only fused operation is the dequantizer's
// explicit fmaf.
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#include "ce_api.h"

#pragma STDC FP_CONTRACT OFF

extern "C" int32_t ce_cpu_budget(void);

namespace ce {

void set_error(const char* fmt, ...);

// exact up-conversions of the 16-bit source types, in integer arithmetic
static inline float bf16_to_f32(uint16_t h) {
  const uint32_t x = (uint32_t)h << 16;
  float f;
  memcpy(&f, &x, 4);
  return f;
}
static inline float f16_to_f32(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
  const uint32_t e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
  uint32_t x;
  if (e == 0x1fu) {
    x = sign | 0x7f800000u | (m << 13);                  // inf / NaN
  } else if (e != 0) {
    x = sign | ((e + 112u) << 23) | (m << 13);
  } else {
    float f = (float)m * (1.0f / 16777216.0f);           // subnormal half: m * 2^-24, exact
    memcpy(&x, &f, 4);
    x |= sign;
  }
  float f;
  memcpy(&f, &x, 4);
  return f;
}

// rows [a, b) split over at most `threads` threads (capped by ce_cpu_budget()), a chunk of at least 4096 rows each
template <typename F>
static void for_rows(int64_t n, int threads, F fn) {
  threads = std::max(1, std::min<int>(threads, ce_cpu_budget()));
  const int t = (int)std::min<int64_t>(threads, std::max<int64_t>(1, n / 4096));
  if (t <= 1) {
    fn(0, n);
    return;
  }
  std::vector<std::thread> pool;
  const int64_t per = (n + t - 1) / t;
  for (int i = 0; i < t; ++i) {
    const int64_t lo = i * per, hi = std::min<int64_t>(n, lo + per);
    if (lo >= hi) break;
    pool.emplace_back([=] { fn(lo, hi); });
  }
  for (auto& th : pool) th.join();
}

// The two formats: the highest code, which dims a table may have, the bytes of a row's codes, how codes are packed
// (pack: code(i) for every element i, in order) and unpacked (each: f(i, code)).  q8: a byte per element.
struct Q8Fmt {
  static constexpr int kMax = 255;
  static constexpr const char* kDimMsg = "a q8 table needs dim %% 16 == 0 and 16 <= dim <= 1024 (got %d)";
  static bool dim_ok(int32_t dim) { return dim >= 16 && dim <= 1024 && dim % 16 == 0; }
  static size_t code_bytes(int32_t dim) { return (size_t)dim; }
  template <typename F> static inline void pack(uint8_t* q, int32_t dim, F code) {
    for (int32_t i = 0; i < dim; ++i) q[i] = code(i);
  }
  template <typename F> static inline void each(const uint8_t* q, int32_t dim, F f) {
    for (int32_t i = 0; i < dim; ++i) f(i, q[i]);
  }
};
// q4: two elements per byte, the even one in the low nibble; both nibbles of every byte are written
struct Q4Fmt {
  static constexpr int kMax = 15;
  static constexpr const char* kDimMsg = "a q4 table needs dim %% 32 == 0 and 32 <= dim <= 1024 (got %d)";
  static bool dim_ok(int32_t dim) { return dim >= 32 && dim <= 1024 && dim % 32 == 0; }
  static size_t code_bytes(int32_t dim) { return (size_t)dim / 2; }
  template <typename F> static inline void pack(uint8_t* q, int32_t dim, F code) {
    for (int32_t i = 0; i < dim; i += 2) {
      const uint8_t even = code(i), odd = code(i + 1);
      q[i >> 1] = (uint8_t)(even | (odd << 4));
    }
  }
  template <typename F> static inline void each(const uint8_t* q, int32_t dim, F f) {
    for (int32_t i = 0; i < dim; i += 2) {
      const uint8_t b = q[i >> 1];
      f(i, (uint8_t)(b & 15u));
      f(i + 1, (uint8_t)(b >> 4));
    }
  }
};
static_assert(CE_Q4_HEADER_BYTES == CE_Q8_HEADER_BYTES, "one header for both formats");
constexpr size_t kHeaderBytes = CE_Q8_HEADER_BYTES;
template <typename P> static inline size_t row_bytes(int32_t dim) { return kHeaderBytes + P::code_bytes(dim); }

// one row: x[dim] (already fp32) -> scale, bias, zero pad, codes.  false: the row holds a NaN or an infinity (or its
// range overflows fp32)
template <typename P>
static inline bool quantize_row(const float* x, int32_t dim, uint8_t* out) {
  float lo = x[0], hi = x[0];
  bool finite = true;
  for (int32_t i = 0; i < dim; ++i) {
    const float v = x[i];
    finite &= fabsf(v) <= FLT_MAX;                       // false for NaN and +-inf
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
  }
  const float range = hi - lo;
  if (!finite || !(range <= FLT_MAX)) return false;
  constexpr float top = (float)P::kMax;
  float scale = range / top;
  uint8_t* q = out + kHeaderBytes;
  if (scale == 0.0f) {
    scale = 0.0f;                                        // (never -0)
    memset(q, 0, P::code_bytes(dim));
  } else {
    P::pack(q, dim, [=](int32_t i) {
      const float d = x[i] - lo;
      float t = rintf(d / scale);                        // ties to even (the default rounding mode)
      t = t < 0.0f ? 0.0f : (t > top ? top : t);
      return (uint8_t)(int)t;
    });
  }
  memcpy(out, &scale, 4);
  memcpy(out + 4, &lo, 4);
  memset(out + 8, 0, 8);
  return true;
}

// the same loop twice: where the CPU has a hardware fma, fmaf is one instruction, not a call into libm
template <typename P>
__attribute__((target("fma"))) static void dequantize_rows_fma(const uint8_t* src, int64_t a, int64_t b, int32_t dim,
                                                               float* dst) {
  const size_t rb = row_bytes<P>(dim);
  for (int64_t r = a; r < b; ++r) {
    float scale, bias;
    memcpy(&scale, src + (size_t)r * rb, 4);
    memcpy(&bias, src + (size_t)r * rb + 4, 4);
    float* out = dst + (size_t)r * dim;
    P::each(src + (size_t)r * rb + kHeaderBytes, dim,
            [=](int32_t i, uint8_t q) __attribute__((target("fma"))) { out[i] = __builtin_fmaf((float)q, scale, bias); });
  }
}
template <typename P>
static void dequantize_rows_plain(const uint8_t* src, int64_t a, int64_t b, int32_t dim, float* dst) {
  const size_t rb = row_bytes<P>(dim);
  for (int64_t r = a; r < b; ++r) {
    float scale, bias;
    memcpy(&scale, src + (size_t)r * rb, 4);
    memcpy(&bias, src + (size_t)r * rb + 4, 4);
    float* out = dst + (size_t)r * dim;
    P::each(src + (size_t)r * rb + kHeaderBytes, dim, [=](int32_t i, uint8_t q) { out[i] = fmaf((float)q, scale, bias); });
  }
}

}  // namespace ce

using namespace ce;

#define CE_Q_REQUIRE(cond, code, ...) \
  do {                                \
    if (!(cond)) {                    \
      ce::set_error(__VA_ARGS__);     \
      return (code);                  \
    }                                 \
  } while (0)

template <typename P>
static int host_quantize(const void* src, int32_t src_dtype, int64_t n_rows, int32_t dim, void* dst, int threads) {
  CE_Q_REQUIRE(src_dtype == CE_ACT_F32 || src_dtype == CE_ACT_BF16 || src_dtype == CE_ACT_F16, CE_ERR_INVALID,
               "src_dtype %d: CE_ACT_F32, CE_ACT_BF16 or CE_ACT_F16", (int)src_dtype);
  CE_Q_REQUIRE(P::dim_ok(dim), CE_ERR_UNSUPPORTED, P::kDimMsg, (int)dim);
  CE_Q_REQUIRE(n_rows >= 0, CE_ERR_INVALID, "negative n_rows");
  if (n_rows == 0) return CE_OK;
  CE_Q_REQUIRE(src && dst, CE_ERR_INVALID, "null pointer");
  const size_t rb = row_bytes<P>(dim);
  uint8_t* out = (uint8_t*)dst;
  std::atomic<int64_t> first_bad{INT64_MAX};
  for_rows(n_rows, threads, [&, dim, src_dtype](int64_t a, int64_t b) {
    float buf[1024];
    for (int64_t r = a; r < b; ++r) {
      const float* x;
      if (src_dtype == CE_ACT_F32) {
        x = (const float*)src + (size_t)r * dim;
      } else {
        const uint16_t* h = (const uint16_t*)src + (size_t)r * dim;
        if (src_dtype == CE_ACT_BF16) for (int32_t i = 0; i < dim; ++i) buf[i] = bf16_to_f32(h[i]);
        else for (int32_t i = 0; i < dim; ++i) buf[i] = f16_to_f32(h[i]);
        x = buf;
      }
      if (!quantize_row<P>(x, dim, out + (size_t)r * rb)) {
        int64_t cur = first_bad.load();
        while (r < cur && !first_bad.compare_exchange_weak(cur, r)) {}
        return;                                          // rows of this share are ascending: r is its first
      }
    }
  });
  const int64_t bad = first_bad.load();
  CE_Q_REQUIRE(bad == INT64_MAX, CE_ERR_INVALID,
               "row %lld holds a NaN or an infinity (or its range overflows fp32): it cannot be quantized",
               (long long)bad);
  return CE_OK;
}

template <typename P>
static int host_dequantize(const void* src, int64_t n_rows, int32_t dim, float* dst, int threads) {
  CE_Q_REQUIRE(P::dim_ok(dim), CE_ERR_UNSUPPORTED, P::kDimMsg, (int)dim);
  CE_Q_REQUIRE(n_rows >= 0, CE_ERR_INVALID, "negative n_rows");
  if (n_rows == 0) return CE_OK;
  CE_Q_REQUIRE(src && dst, CE_ERR_INVALID, "null pointer");
  __builtin_cpu_init();
  const bool hw_fma = __builtin_cpu_supports("fma");
  const uint8_t* in = (const uint8_t*)src;
  for_rows(n_rows, threads, [=](int64_t a, int64_t b) {
    if (hw_fma) dequantize_rows_fma<P>(in, a, b, dim, dst);
    else dequantize_rows_plain<P>(in, a, b, dim, dst);
  });
  return CE_OK;
}

extern "C" size_t ce_q8_row_bytes(int32_t dim) { return Q8Fmt::dim_ok(dim) ? row_bytes<Q8Fmt>(dim) : 0; }
extern "C" int ce_host_quantize_q8(const void* src, int32_t src_dtype, int64_t n_rows, int32_t dim, void* dst,
                                   int threads) {
  return host_quantize<Q8Fmt>(src, src_dtype, n_rows, dim, dst, threads);
}
extern "C" int ce_host_dequantize_q8(const void* src, int64_t n_rows, int32_t dim, float* dst, int threads) {
  return host_dequantize<Q8Fmt>(src, n_rows, dim, dst, threads);
}

extern "C" size_t ce_q4_row_bytes(int32_t dim) { return Q4Fmt::dim_ok(dim) ? row_bytes<Q4Fmt>(dim) : 0; }
extern "C" int ce_host_quantize_q4(const void* src, int32_t src_dtype, int64_t n_rows, int32_t dim, void* dst,
                                   int threads) {
  return host_quantize<Q4Fmt>(src, src_dtype, n_rows, dim, dst, threads);
}
extern "C" int ce_host_dequantize_q4(const void* src, int64_t n_rows, int32_t dim, float* dst, int threads) {
  return host_dequantize<Q4Fmt>(src, n_rows, dim, dst, threads);
}
