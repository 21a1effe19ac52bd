// Shared helpers for the HIP sources of libce_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <sched.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <type_traits>

#include "ce_api.h"

namespace ce {

void set_error(const char* fmt, ...);

#define CE_HIP_CHECK(expr)                                                              \
  do {                                                                                  \
    hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess) {                                                             \
      ce::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return CE_ERR_HIP;                                                                \
    }                                                                                   \
  } while (0)

#define CE_REQUIRE(cond, code, ...)  \
  do {                               \
    if (!(cond)) {                   \
      ce::set_error(__VA_ARGS__);    \
      return (code);                 \
    }                                \
  } while (0)

#define CE_LAUNCH_CHECK() CE_HIP_CHECK(hipGetLastError())

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <typename VT> __device__ __forceinline__ VT vzero();
template <> __device__ __forceinline__ float vzero<float>() { return 0.f; }
template <> __device__ __forceinline__ f32x4 vzero<f32x4>() { return f32x4{0.f, 0.f, 0.f, 0.f}; }

// Activation type AT of the bag kernels (API 6 additions: CE_ACT_*): what the forward's output and the backward's
// grad_out are stored as.  The table, the accumulation and the update stay fp32, and a lane keeps the same elements of
// a row whatever AT is: Act<AT, VT>::V is the memory form of a lane's VT (VT itself for fp32; 4 x 16 bit = 8 bytes for
// f32x4, one 16-bit scalar for float).  down() is the plain cast -- round-to-nearest-even, NaN stays NaN
// (v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32) --, up() is exact.
typedef __bf16 bf16_t;
typedef _Float16 f16_t;
typedef bf16_t bf16x4 __attribute__((ext_vector_type(4)));
typedef f16_t f16x4 __attribute__((ext_vector_type(4)));

template <typename AT, typename VT> struct Act;
template <typename VT> struct Act<float, VT> {
  typedef VT V;
  static __device__ __forceinline__ VT up(V a) { return a; }
  static __device__ __forceinline__ V down(VT v) { return v; }
};
#define CE_ACT16(AT, AT4)                                                                                     \
  template <> struct Act<AT, float> {                                                                         \
    typedef AT V;                                                                                             \
    static __device__ __forceinline__ float up(V a) { return (float)a; }                                      \
    static __device__ __forceinline__ V down(float v) { return (AT)v; }                                       \
  };                                                                                                          \
  template <> struct Act<AT, f32x4> {                                                                         \
    typedef AT4 V;                                                                                            \
    static __device__ __forceinline__ f32x4 up(V a) { return __builtin_convertvector(a, f32x4); }             \
    static __device__ __forceinline__ V down(f32x4 v) { return __builtin_convertvector(v, AT4); }             \
  };
CE_ACT16(bf16_t, bf16x4)
CE_ACT16(f16_t, f16x4)
#undef CE_ACT16

static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// MI355X: 256 CUs; memory-bound grid-stride kernels are capped at 8 blocks of 256 per CU.
constexpr int kNumCU = 256;
constexpr int kMaxBlocks = kNumCU * 8;

static inline int grid_for(int64_t work_items, int per_block) {
  int64_t b = cdiv(work_items, per_block);
  if (b < 1) b = 1;
  if (b > kMaxBlocks) b = kMaxBlocks;
  return (int)b;
}

// The bag layout of a window's batches, as ce_bag_presort_window_src takes it: batch b's offsets start
// offsets_batch_stride elements after batch b - 1's (offsets == nullptr: one id per bag, in order).
struct BagLayout {
  const void* offsets;
  int32_t offsets_are_i64;
  int64_t offsets_batch_stride, num_bags;
  int32_t include_last_offset;
  int64_t hook_features;
};

// ce_bag.hip, for the cache manager (ce_cache.hip): the window presort with the cache op's last step folded in.
// slots_io holds the ROW of every id (what k_mark left there; -1 = no lookup); the kernel turns it into the slot in
// place (inverted[row]; -1 everywhere when *status != CE_OK) and writes the window's keys in the same pass -- instead
// of k_slots writing 8 bytes per id that the presort reads straight back.  lay as ce_bag_presort_window_src;
// src_keys == 0: keys = row << 32 | lookup in segment (ce_bag_presort_window).
int presort_window_from_rows(int64_t* slots_io, int64_t nnz_per_batch, int64_t n_batches, int64_t num_rows,
                             const int32_t* inverted, const int* status, int32_t src_keys, const BagLayout& lay,
                             uint64_t* keys_out, hipStream_t stream);

// ce_host.hip: pins the CALLING thread to the CPUs of the current GPU's NUMA node (sysfs local_cpulist of its PCI
// function, intersected with the CPUs the process may use); no-op when that cannot be read or CE_NUMA_BIND=0.  For
// the library's own threads only -- the swap workers, their helpers and the first touch of ce_host_alloc -- so that
// the host table and the staging buffers sit behind the GPU's own root complex.
void bind_thread_near_gpu();
// the same CPU set for threads that have not selected the device themselves (taken by their creator); false = none
bool near_gpu_cpus(cpu_set_t* out);

// ce_sort.hip, for the sorted fused update (ce_bag_adagrad.hip): the call's lookups stably radix-sorted by row.
// rows[t] ascending, a valid row's lookups in ascending lookup position, every ignored lookup (slot outside
// [0, num_rows)) behind them with rows[t] == num_rows; lookups[t] = position of the lookup in the call, bag_of[j] = bag
// of lookup j (-1: no bag covers it).  The arrays live in `workspace` (sorted_rows_bytes(nnz) bytes, 256-byte
// aligned, nothing in it needs initialising).
struct SortedRows {
  const int32_t* rows;
  const int32_t* lookups;
  const int32_t* bag_of;
};
size_t sorted_rows_bytes(int64_t nnz);
int sorted_rows(const int64_t* indices, int64_t nnz, int64_t num_rows, const void* offsets, int off64,
                int64_t num_bags, int include_last, void* workspace, hipStream_t s,
                SortedRows& out, bool covered_only = false);

// How the lanes of a launch hold one embedding row.  Vector form: a lane's chunk is 16 B (f32x4); it needs dim % 4 == 0
// and `aligned` -- every row pointer of the launch on its vector boundary.  Scalar form otherwise: one float per chunk.
// A power-of-two group of at most 64 lanes works on a row and a lane holds nch = 1, 2 or 4 chunks of it (3 rounds up
// to 4; the kernels mask chunks past rowlen), so the vector form ends at dim = 1024 and the scalar one at 256.
struct RowGeom {
  bool vec;
  int rowlen;   // chunks per row
  int g_log2;   // log2(lanes per row)
  int nch;      // chunks per lane
};

static inline int row_geometry(int32_t dim, bool aligned, RowGeom& r) {
  r.vec = dim % 4 == 0 && aligned;
  r.rowlen = r.vec ? dim / 4 : dim;
  int g = 1;
  r.g_log2 = 0;
  while (g < r.rowlen && g < 64) { g <<= 1; ++r.g_log2; }
  const int need = (r.rowlen - 1) / g + 1;
  r.nch = 1;
  while (r.nch < need) r.nch <<= 1;
  CE_REQUIRE(r.nch <= 4, CE_ERR_UNSUPPORTED, "embedding dim %d too large for this build", dim);
  return CE_OK;
}

static inline bool al16(const void* q) { return (((uintptr_t)q) & 15) == 0; }
// an activation tensor on its vector boundary: a lane's 4 elements are 16 bytes of fp32 and 8 bytes of a 16-bit type
// (the alignment that rows of dim % 4 == 0 elements keep there: dim = 20, 100 included)
static inline bool act_aligned(const void* q, int act) { return (((uintptr_t)q) & (act == CE_ACT_F32 ? 15 : 7)) == 0; }

#define CE_REQUIRE_ROWS(num_rows) \
  CE_REQUIRE((num_rows) > 0 && (num_rows) < (int64_t)INT32_MAX, CE_ERR_INVALID, "num_rows out of range")

#define CE_REQUIRE_ACT(act)                                                                            \
  CE_REQUIRE((act) == CE_ACT_F32 || (act) == CE_ACT_BF16 || (act) == CE_ACT_F16, CE_ERR_INVALID,       \
             "unknown activation dtype %d (CE_ACT_F32 / CE_ACT_BF16 / CE_ACT_F16)", (int)(act))

// A 16-bit TABLE (ce_*_w16): bf16 / fp16 rows that are whole 16-byte units, vector lanes only.  Arguments alone decide.
static inline int w16_check(int32_t weight_dtype, int32_t dim) {
  CE_REQUIRE(weight_dtype == CE_ACT_BF16 || weight_dtype == CE_ACT_F16, CE_ERR_INVALID,
             "weight_dtype %d: a 16-bit table is CE_ACT_BF16 or CE_ACT_F16", (int)weight_dtype);
  CE_REQUIRE(dim > 0, CE_ERR_INVALID, "embedding dim must be positive");
  CE_REQUIRE(dim % 8 == 0 && dim <= 1024, CE_ERR_UNSUPPORTED,
             "a 16-bit table needs dim %% 8 == 0 and dim <= 1024 (got %d)", (int)dim);
  return CE_OK;
}

// An ADAM-LAYOUT table (ce_*_adam): fp32 rows w | m | v of 3 * dim elements whose three parts are whole 16-byte
// units, vector lanes only.  The argument alone decides.
#define CE_REQUIRE_ADAM_DIM(dim)                                                                 \
  CE_REQUIRE((dim) % 4 == 0 && (dim) >= 4 && (dim) <= 1024, CE_ERR_UNSUPPORTED,                  \
             "an Adam-layout table needs dim %% 4 == 0 and 4 <= dim <= 1024 (got %d)", (int)(dim))

// The one place that turns the run-time lane shape and activation code into template arguments: f is a generic lambda
// and gets a tag to read the types from (typename decltype(l)::VT, decltype(l)::NCH, typename decltype(a)::AT).
template <typename VT_, int NCH_> struct Lanes {
  typedef VT_ VT;
  static constexpr int NCH = NCH_;
};
template <typename AT_> struct ActTag { typedef AT_ AT; };

// the vector lane shapes alone (a table that has no scalar form): f(Lanes<f32x4, N>)
template <typename F> static inline void for_vec_lanes(int nch, F&& f) {
  if (nch == 1) f(Lanes<f32x4, 1>{}); else if (nch == 2) f(Lanes<f32x4, 2>{}); else f(Lanes<f32x4, 4>{});
}

template <typename F> static inline void for_lanes(bool vec, int nch, F&& f) {
  if (vec) {
    for_vec_lanes(nch, f);
  } else {
    if (nch == 1) f(Lanes<float, 1>{}); else if (nch == 2) f(Lanes<float, 2>{}); else f(Lanes<float, 4>{});
  }
}

template <typename F> static inline void for_act(int act, F&& f) {
  if (act == CE_ACT_F32) f(ActTag<float>{}); else if (act == CE_ACT_BF16) f(ActTag<bf16_t>{}); else f(ActTag<f16_t>{});
}

// a 16-bit table's lanes (always f32x4 chunks) and row type: f(Lanes<f32x4, N>, ActTag<WT>)
template <typename F> static inline void for_w16(int nch, int weight_dtype, F&& f) {
  auto lanes = [&](auto w) { for_vec_lanes(nch, [&](auto l) { f(l, w); }); };
  if (weight_dtype == CE_ACT_BF16) lanes(ActTag<bf16_t>{}); else lanes(ActTag<f16_t>{});
}

// the one place that turns (weight_dtype, RowGeom) into the table's row type and the lane shape of a launch:
// f(Lanes<VT, N>, ActTag<WT>) -- an fp32 table in either lane form, a 16-bit table in vector lanes.  (The q8 table,
// forward only, is added by the forwards' own for_table_act in ce_bag.hip: the updates that dispatch here have no q8 form.)
template <typename F> static inline void for_table(int weight_dtype, const RowGeom& r, F&& f) {
  if (weight_dtype == CE_ACT_F32) for_lanes(r.vec, r.nch, [&](auto l) { f(l, ActTag<float>{}); });
  else for_w16(r.nch, weight_dtype, f);
}

}  // namespace ce
