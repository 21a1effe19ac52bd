// Fused optimizer updates of the cached table: exact row-wise Adagrad (FBGEMM's EXACT_ROWWISE_ADAGRAD; the reference's
// baseline maps --adagrad to it: baselines/dlrm_main.py:698-702) on fp32, bf16 and fp16 rows, and SGD on bf16 / fp16
// rows; each, and Adam, also with a lazy weight decay -- L2 or decoupled: the ce_*_wd entries, the WD = true
// instantiations, DESIGN.md 3.12.  Per step and per UNIQUE row r looked up (without decay):
//   g = sum of the step's gradient rows of r ;  m[r] += sum_d g[d]^2 / D ;  W[r] -= lr * g / (sqrt(m[r]) + eps)
// (SGD: W[r] -= lr * g).  "Exact": the non-linear update sees the row's whole gradient of the batch, so duplicate
// lookups are folded across the whole batch first.  Three ways to fold:
//   * cache-sized accumulator (ce_bag_backward_rowwise_adagrad*, ce_bag_backward_update*_w16): k_mark_* flags the
//     step's slots, the dense backward (ce_bag.hip) scatters into acc[num_rows, D] by atomics, k_rows_apply walks the
//     flags and updates every flagged slot;
//   * step-sized accumulator (ce_bag_backward_update_compact*): the flagged slots are numbered first, the
//     same backward scatters into acc[min(nnz, num_rows), D], k_compact_apply walks the list;
//   * deterministic, no accumulator (ce_bag_backward_update_sorted): the lookups are sorted by row and
//     k_sorted_fold / k_sorted_combine fold a row's gradient in registers, in lookup order.
// The two atomic forms hand a row's folded gradient to update_row(), which holds the whole arithmetic of the update --
// spelled out, with contraction off -- so they agree bit for bit by construction; tests/test_gpu_fused_update_bits.py
// pins those bits.  The sorted form keeps its own copy of the update (sorted_apply_row, its own walk, its own checks in
// the entry): DESIGN.md 3.5 says why.  No host synchronisation, no allocation, launch shapes fixed by the arguments (a
// backward can be captured into a hipGraph).  The momentum is indexed by host-table row (row_of_slot = cached_idx_map)
// and never moves with the cache; a slot maps to one row for the whole step, so folding by slot is folding by row.
// Adam (ce_bag_backward_adam*) is a third arithmetic of update_row on an fp32 table whose rows carry
// their own moments (w | m | v): the two atomic folds above, unchanged, hand it the same folded gradient.  Partial
// row-wise Adam (ce_bag_backward_pradam*) is a fourth: rows w | m, the second moment one fp32 per table
// row where row-wise Adagrad keeps its momentum, fed by the mean of the row's squared gradient.  Element-wise Adagrad
// (ce_bag_backward_adagrad*; torch.optim.Adagrad, FBGEMM's EXACT_ADAGRAD) is a fifth: rows w | h, h the
// per-element sums of squared gradients, the rate lr / (1 + (t - 1) lr_decay) formed on the device from the step count.
// Gradient clipping (the ce_*_clip entries, the CLIP = true instantiations) acts on a row's folded
// gradient g -- what update_row / sorted_apply_row receive -- FIRST, and everything that used g then uses the clipped g:
// the L2 decay's h = g + wd * w, row-wise Adagrad's sum h^2 / D, Adam's m' and v', partial row-wise Adam's ss, the step
// (torch's order, clip_grad_* before optimizer.step(), and FBGEMM's).  fp32, contraction off, c the threshold by value:
//   CE_CLIP_NONE      the covered entry's update, by the covered entry's kernels: its bits
//   CE_CLIP_VALUE     per element:  g = g < -c ? -c : (g > c ? c : g)                   (a NaN stays a NaN, as torch.clamp)
//   CE_CLIP_ROW_NORM  ss = sum_d g[d]^2 in lane_sq_sum's spelled-out order for the table's type, then the xor tree across
//                     the lane group, widest stride first (the reduction row-wise Adagrad already runs);
//                     n = sqrtf(ss) ; k = c / (n + 1e-6f) ; if (k < 1.f) g[d] = g[d] * k       (clip_grad_norm_, per row)
// Row-wise Adagrad and partial row-wise Adam then sum the squares of the clipped (and decayed) gradient themselves: a
// second reduction, not k^2 * ss.  Clipping does not change which rows a call names -- the mark rule depends on the
// decay alone -- and a slot whose momentum or v index lies outside its array is still untouched.  clip_row is the one
// spelling, so a row looked up once in a call gets the same bits from all three folds.
// The three in-row arithmetics have the deterministic fold as well (ce_bag_backward_adam_sorted / _pradam_sorted /
// _adagrad_sorted): k_in_row_fold folds every chunk into a partial row, k_in_row_apply hands a row's
// whole gradient to update_row -- no copy of the update there.
#include "ce_common.h"

namespace ce {

// ---------------------------------------------------------------------------------------------------------------
// The update of one row

// what update_row reads: the argument structs of the atomic forms' kernels embed it
struct UpdateArgs {
  void* weight;                       // [num_rows, D] of WT
  const int32_t* row_of_slot;         // NULL: momentum is indexed by slot
  float* momentum;                    // [momentum_rows]
  int64_t momentum_rows;
  uint64_t seed;                      // stochastic rounding only, as the step counter
  const unsigned long long* counter;
  int32_t rowlen;                     // chunks per row
  int32_t g_log2;                     // log2(lanes per row)
  int32_t dim;
  float lr;
  float eps;
  const float* lr_dev;                // non-NULL (the ce_*_lrdev entries): the learning rate is *lr_dev, `lr` is not read
  // Adam only (`weight` is then [num_rows, 3 * D]: w | m | v; `counter` is the caller's step count)
  // element-wise Adagrad (`weight` is [num_rows, 2 * D]: w | h; `counter` is the caller's step count) has no betas:
  // its lr_decay lies where beta1 does, so that every other kernel's arguments stay where they were
  union {
    double beta1;
    double lr_decay;
  };
  double beta2;
  float omb1, omb2;                   // (float)(1.0 - beta): the fp64 difference, rounded once
  // weight decay (the ce_*_wd entries, the WD = true instantiations): CE_WD_L2 or CE_WD_DECOUPLED
  float wd;
  int32_t wd_mode;
};

// the launch's learning rate: uniform, so a kernel reads it once per thread, at its top, and hands it to update_row
__device__ __forceinline__ float learning_rate(const UpdateArgs& a) { return a.lr_dev ? *a.lr_dev : a.lr; }

// Adam's step size lr * c_t, c_t = sqrt(1 - beta2^t) / (1 - beta1^t) in fp64 from the step count as the call's first
// launch left it, rounded once: uniform like the learning rate, so a kernel works it out once per thread, at its top
__device__ __forceinline__ float adam_step_size(const UpdateArgs& a) {
#pragma clang fp contract(off)
  const double t = (double)*a.counter;
  const float c = (float)(sqrt(1.0 - pow(a.beta2, t)) / (1.0 - pow(a.beta1, t)));
  return learning_rate(a) * c;
}

// The decoupled decay's factor f = (float)(1.0 - (double)lr * (double)wd), lr the launch's learning rate (Adam: lr, not
// lr * c_t): uniform like the learning rate -- and read from *lr_dev with it, so a replayed graph follows a schedule in
// the decay as well -- so a kernel works it out once per thread, at its top.  The L2 form does not look at it.
__device__ __forceinline__ float decay_factor(float lr, float wd) { return (float)(1.0 - (double)lr * (double)wd); }

// Element-wise Adagrad's rate: clr_d = lr / (1 + (t - 1) * lr_decay) in fp64, t the step count as the
// call's first launch left it.  The step is (float)clr_d and the decoupled decay's factor (float)(1.0 - clr_d * wd), so
// a replayed graph follows a schedule and the step count in both.  Uniform: once per thread, at the kernel's top.
__device__ __forceinline__ double adagrad_rate(const UpdateArgs& a) {
#pragma clang fp contract(off)
  const double t = (double)*a.counter;
  return (double)learning_rate(a) / (1.0 + (t - 1.0) * a.lr_decay);
}
__device__ __forceinline__ float adagrad_decay_factor(double clr, float wd) {
#pragma clang fp contract(off)
  return (float)(1.0 - clr * (double)wd);
}

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// Stochastic rounding in integer arithmetic on the fp32 bit pattern: a uniform integer below the dropped bits is added
// to the magnitude and the sum truncated -- the neighbour farther from zero is taken with probability
// (dropped bits) / 2^k, a representable x (dropped bits zero) never moves.  Everything else takes the nearest cast.
__device__ __forceinline__ bf16_t round_stochastic(float x, uint32_t rnd, bf16_t) {
  const uint32_t b = __float_as_uint(x);
  const uint32_t t = b + (rnd & 0xffffu);
  // NaN / inf, or a carry past the largest finite value
  if ((b & 0x7f800000u) == 0x7f800000u || (t & 0x7f800000u) == 0x7f800000u) return (bf16_t)x;
  return __builtin_bit_cast(bf16_t, (uint16_t)(t >> 16));
}
__device__ __forceinline__ f16_t round_stochastic(float x, uint32_t rnd, f16_t) {
  const uint32_t b = __float_as_uint(x);
  const uint32_t mag = b & 0x7fffffffu;
  // fp16 normals below the largest finite value: 2^-14 <= |x| < 65504 (NaN / inf / subnormal results: nearest)
  if (mag < 0x38800000u || mag >= 0x477fe000u) return (f16_t)x;
  const uint32_t t = (b + (rnd & 0x1fffu)) & ~0x1fffu;       // 13 dropped bits; at most 65504: exact in fp16
  return (f16_t)__uint_as_float(t);
}

// Sum of a lane's squares, SPELLED OUT: this is the specification, not a reading of what a compiler
// made of `ss += x^2 + y^2 + z^2 + w^2`.  A chunk's four squares are either rounded one by one and added ("plain":
// ((x^2 + y^2) + z^2) + w^2) or folded into a chain of fused multiply-adds ("chain": fma(w, w, fma(z, z, fma(x, x,
// y * y)))).  fp32 table: the lane's LAST chunk plain, the chunks before it chains; 16-bit table: chains only; scalar
// lanes: one chain over the lane's elements, started by the second one (g1 * g1, then fma g0, g2, g3).  Chunk sums are
// added in chunk order.
__device__ __forceinline__ float sq_plain(f32x4 v) {
#pragma clang fp contract(off)
  const float xx = v.x * v.x, yy = v.y * v.y, zz = v.z * v.z, ww = v.w * v.w;
  return ((xx + yy) + zz) + ww;
}
__device__ __forceinline__ float sq_chain(f32x4 v) {
#pragma clang fp contract(off)
  return __builtin_fmaf(v.w, v.w, __builtin_fmaf(v.z, v.z, __builtin_fmaf(v.x, v.x, v.y * v.y)));
}
template <typename WT, int NCH>
__device__ __forceinline__ float lane_sq_sum(const f32x4 (&g)[NCH]) {
#pragma clang fp contract(off)
  constexpr bool w32 = std::is_same<WT, float>::value;
  float ss = (w32 && NCH == 1) ? sq_plain(g[0]) : sq_chain(g[0]);
#pragma unroll
  for (int c = 1; c < NCH; ++c) ss = ss + ((w32 && c == NCH - 1) ? sq_plain(g[c]) : sq_chain(g[c]));
  return ss;
}
template <typename WT, int NCH>
__device__ __forceinline__ float lane_sq_sum(const float (&g)[NCH]) {
#pragma clang fp contract(off)
  // as in sq_chain, the SECOND square is the one rounded on its own and the first is fused onto it
  if (NCH == 1) return g[0] * g[0];
  float ss = __builtin_fmaf(g[0], g[0], g[NCH > 1 ? 1 : 0] * g[NCH > 1 ? 1 : 0]);
#pragma unroll
  for (int c = 2; c < NCH; ++c) ss = __builtin_fmaf(g[c], g[c], ss);
  return ss;
}

// w - g * m with ONE rounding per element
__device__ __forceinline__ float fnma(float g, float m, float w) { return __builtin_fmaf(-g, m, w); }
__device__ __forceinline__ f32x4 fnma(f32x4 g, float m, f32x4 w) {
  return __builtin_elementwise_fma(-g, f32x4{m, m, m, m}, w);
}

// the key of a step's random bits (0 where nothing is rounded stochastically): the step counter lives in the workspace
// and the first launch of the step adds one to it, so a replayed graph draws fresh bits every step
template <bool STOCH> __device__ __forceinline__ uint64_t step_key(const UpdateArgs& a) {
  return STOCH ? mix64(a.seed + 0xD6E8FEB86659FD93ull * *a.counter) : 0;
}

// The whole update of the row in slot s from g, its folded gradient of the step, with the learning rate lr (zero in chunks past rowlen), by the
// row's lane group (lane gl of G; every lane of the group must be here: the reduction shuffles across it).
//   adagrad: ss = sum of the group's lane_sq_sum (xor tree, widest stride first); r outside the momentum: nothing
//            happens; m[r] = m[r] + ss / D (lane 0 writes); mult = lr / (sqrt(m[r]) + eps).   sgd: mult = lr.
//   x = fma(-g, mult, up(W[s])) per element; W[s] = x (fp32), nearest(x), or round_stochastic(x, 16 bits of
//   mix64(mix64(step_key ^ r) + chunk index) per element).
//   ADAM (an fp32 table of rows w | m | v, vector lanes; lr is adam_step_size; `adagrad` is not looked at), per element:
//     m' = m + omb1 * (g - m) ; v' = v + omb2 * (g * g - v) ; w' = w - lr * (m' / (sqrtf(v') + eps))
//   every operation rounded on its own (torch.optim.SparseAdam's); no reduction, no state outside the row.
//   WD (weight decay, lazy: the rows a step names decay once, in that step; f is decay_factor), with w = up(W[s]) read
//   ONCE, before the reduction, and kept in registers up to the store:
//     CE_WD_L2:        h = g + wd * w per element (the product rounded, then the sum); the update above with h for g
//                      everywhere -- the sum of squares, the momentum, the moments, the step;
//     CE_WD_DECOUPLED: w_d = w * f per element; the update above with w_d for w and the raw g.
//   A slot the Adagrad update does not touch (r outside the momentum) gets no decay either.
// the step of one element from its new moments: lr * (m / (sqrtf(v) + eps)), division and square root correctly rounded
__device__ __forceinline__ float adam_delta(float lr, float eps, float m, float v) {
#pragma clang fp contract(off)
  const float q = m / (sqrtf(v) + eps);
  return lr * q;
}

// Gradient clipping (the ce_*_clip entries, the CLIP = true instantiations), of a row's folded gradient
// in its lane group's registers, BEFORE everything that reads it (the decay's h, the sums of squares, the moments, the
// step).  Every lane of the group must be here: the norm's reduction shuffles across it.  c > 0, +inf included.
//   CE_CLIP_VALUE:    per element g = g < -c ? -c : (g > c ? c : g)  (a NaN stays a NaN, as torch.clamp);
//   CE_CLIP_ROW_NORM: ss = the group's lane_sq_sum<WT> (xor tree, widest stride first) ; n = sqrtf(ss) ;
//                     k = c / (n + 1e-6f) ; if (k < 1.f) g = g * k per element  (clip_grad_norm_, the row its own parameter).
// Chunks past rowlen hold zeros and keep them.  This is the ONE spelling: update_row and sorted_apply_row both call it.
struct RowClip {
  float c = 0.f;
  int mode = CE_CLIP_NONE;
};
__device__ __forceinline__ float clip_value(float g, float c) { return g < -c ? -c : (g > c ? c : g); }
__device__ __forceinline__ f32x4 clip_value(f32x4 g, float c) {
  return f32x4{clip_value(g.x, c), clip_value(g.y, c), clip_value(g.z, c), clip_value(g.w, c)};
}
template <typename WT, typename VT, int NCH>
__device__ __forceinline__ void clip_row(VT (&g)[NCH], RowClip k, int G) {
#pragma clang fp contract(off)
  if (k.mode == CE_CLIP_VALUE) {                             // (uniform)
#pragma unroll
    for (int c = 0; c < NCH; ++c) g[c] = clip_value(g[c], k.c);
  } else if (k.mode == CE_CLIP_ROW_NORM) {
    float ss = lane_sq_sum<WT, NCH>(g);
    for (int off = G >> 1; off > 0; off >>= 1) ss = ss + __shfl_xor(ss, off, G);
    const float n = sqrtf(ss);
    const float scale = k.c / (n + 1e-6f);
    // `if (scale < 1.f) g = g * scale`, as a select per chunk: lane groups of one wave differ in `scale`, and a branch
    // would hold a saved exec mask in two scalar registers that k_sorted_fold does not have
    const bool shrink = scale < 1.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const VT t = g[c] * scale;
      g[c] = shrink ? t : g[c];
    }
  }
}

//   ROWV (with ADAM: partial row-wise Adam, an fp32 table of rows w | m; the second moment is momentum[r], one fp32 per
//   table row as in adagrad, and r outside it: nothing happens, no decay either), h the gradient after the decay:
//     ss = sum of the group's lane_sq_sum<float> of h (xor tree, widest stride first) ;
//     v' = v[r] + omb2 * (ss / D - v[r]) (lane 0 writes) ; m' = m + omb1 * (h - m) ; w' = w - lr * (m' / (sqrtf(v') + eps))
//   CLIP (then WD as well: the decay's mode is read at run time, and CE_WD_NONE is the decoupled form with f = 1, which
//   multiplies exactly): clip_row on a copy of g, then the WD update of that copy -- in every arm the clip stands in
//   front of the decay, and everything behind it is the code the unclipped instantiation runs.
//   ELEM (element-wise Adagrad, torch.optim.Adagrad; DESIGN.md 3.15: an fp32 table of rows w | s, vector lanes; lr is
//   (float)adagrad_rate, f adagrad_decay_factor; `adagrad` is not looked at), h the gradient after the decay, per element:
//     s' = s + h * h ; w' = w - lr * (h / (sqrtf(s') + eps))
//   every operation rounded on its own; no reduction, no state outside the row; w and s read once and written once.
template <typename VT, typename WT, int NCH, bool STOCH, bool ADAM = false, bool WD = false, bool ROWV = false,
          bool CLIP = false, bool ELEM = false>
__device__ __forceinline__ void update_row(const UpdateArgs& a, float lr, uint64_t step_key, int64_t s,
                                           const VT (&g)[NCH], int gl, int G, bool adagrad, float f = 1.f,
                                           RowClip clip = RowClip{}) {
#pragma clang fp contract(off)
  using T = Act<WT, VT>;
  if constexpr (CLIP) {
    static_assert(WD, "the clipped instantiations take the decay as a run-time mode");
    VT cg[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) cg[c] = g[c];
    clip_row<WT, VT, NCH>(cg, clip, G);
    update_row<VT, WT, NCH, STOCH, ADAM, true, ROWV, false, ELEM>(a, lr, step_key, s, cg, gl, G, adagrad, f);
    return;
  }
  const bool l2 = WD && a.wd_mode == CE_WD_L2;               // uniform
  static_assert(!STOCH || (sizeof(WT) == 2 && sizeof(VT) == 16), "stochastic rounding: a 16-bit table, vector lanes");
  static_assert(!ROWV || ADAM, "a row-wise second moment: Adam only");
  static_assert(!ELEM || (!ADAM && !ROWV), "element-wise Adagrad: an arithmetic of its own, no moments");
  if constexpr (ELEM) {
    static_assert(std::is_same<WT, float>::value && sizeof(VT) == 16 && !STOCH,
                  "element-wise Adagrad: an fp32 table, vector lanes");
    f32x4* R = (f32x4*)a.weight + s * 2 * (int64_t)a.rowlen;      // w: [0, rowlen), the sums of squares behind it
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int idx = gl + c * G;
      if (idx >= a.rowlen) continue;
      f32x4 gc = g[c];
      f32x4 w = R[idx], h = R[a.rowlen + idx];
      if constexpr (WD) {
        if (l2) gc = gc + w * a.wd; else w = w * f;
      }
      h = h + gc * gc;                           // (elementwise, each operation rounded: contraction is off)
      w = w - f32x4{adam_delta(lr, a.eps, gc.x, h.x), adam_delta(lr, a.eps, gc.y, h.y), adam_delta(lr, a.eps, gc.z, h.z),
                    adam_delta(lr, a.eps, gc.w, h.w)};
      R[idx] = w;
      R[a.rowlen + idx] = h;
    }
    return;
  }
  if constexpr (ADAM && ROWV) {
    static_assert(std::is_same<WT, float>::value && sizeof(VT) == 16 && !STOCH, "Adam: an fp32 table, vector lanes");
    f32x4* R = (f32x4*)a.weight + s * 2 * (int64_t)a.rowlen;      // w: [0, rowlen), m: [rowlen, 2 rowlen)
    const int64_t r = a.row_of_slot ? (int64_t)a.row_of_slot[s] : s;
    // WD: the row as it was (zero past rowlen, so h is zero there as g is) and hg, the gradient the update sees
    f32x4 w0[WD ? NCH : 1], hg[WD ? NCH : 1];
    if constexpr (WD) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int idx = gl + c * G;
        w0[c] = idx < a.rowlen ? R[idx] : vzero<f32x4>();
        hg[c] = g[c];
        if (l2) hg[c] = g[c] + w0[c] * a.wd; else w0[c] = w0[c] * f;
      }
    }
    float ss;
    if constexpr (WD) ss = lane_sq_sum<float, NCH>(hg); else ss = lane_sq_sum<float, NCH>(g);
    for (int off = G >> 1; off > 0; off >>= 1) ss = ss + __shfl_xor(ss, off, G);
    if (r < 0 || r >= a.momentum_rows) return;
    const float v0 = a.momentum[r];
    const float v = v0 + (ss / (float)a.dim - v0) * a.omb2;
    if (gl == 0) a.momentum[r] = v;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int idx = gl + c * G;
      if (idx >= a.rowlen) continue;
      f32x4 gc, w;
      if constexpr (WD) { gc = hg[c]; w = w0[c]; } else { gc = g[c]; w = R[idx]; }
      f32x4 m = R[a.rowlen + idx];
      m = m + (gc - m) * a.omb1;
      w = w - f32x4{adam_delta(lr, a.eps, m.x, v), adam_delta(lr, a.eps, m.y, v), adam_delta(lr, a.eps, m.z, v),
                    adam_delta(lr, a.eps, m.w, v)};
      R[idx] = w;
      R[a.rowlen + idx] = m;
    }
    return;
  }
  if constexpr (ADAM) {
    static_assert(std::is_same<WT, float>::value && sizeof(VT) == 16 && !STOCH, "Adam: an fp32 table, vector lanes");
    f32x4* R = (f32x4*)a.weight + s * 3 * (int64_t)a.rowlen;      // w: [0, rowlen), m: [rowlen, 2 rowlen), v behind it
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int idx = gl + c * G;
      if (idx >= a.rowlen) continue;
      f32x4 gc = g[c];
      f32x4 w = R[idx], m = R[a.rowlen + idx], v = R[2 * a.rowlen + idx];
      if constexpr (WD) {
        if (l2) gc = gc + w * a.wd; else w = w * f;
      }
      m = m + (gc - m) * a.omb1;                 // (elementwise, each operation rounded: contraction is off)
      v = v + (gc * gc - v) * a.omb2;
      w = w - f32x4{adam_delta(lr, a.eps, m.x, v.x), adam_delta(lr, a.eps, m.y, v.y), adam_delta(lr, a.eps, m.z, v.z),
                    adam_delta(lr, a.eps, m.w, v.w)};
      R[idx] = w;
      R[a.rowlen + idx] = m;
      R[2 * a.rowlen + idx] = v;
    }
    return;
  }
  typename T::V* W = (typename T::V*)a.weight + s * a.rowlen;
  const int64_t r = a.row_of_slot ? (int64_t)a.row_of_slot[s] : s;
  float mult = lr;
  // WD: the row as it was (zero past rowlen, so h is zero there as g is) and hg, the gradient the update sees
  VT w0[WD ? NCH : 1], hg[WD ? NCH : 1];
  if constexpr (WD) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int idx = gl + c * G;
      w0[c] = idx < a.rowlen ? T::up(W[idx]) : vzero<VT>();
      hg[c] = g[c];
      if (l2) hg[c] = g[c] + w0[c] * a.wd; else w0[c] = w0[c] * f;
    }
  }
  if (adagrad) {
    float ss;
    if constexpr (WD) ss = lane_sq_sum<WT, NCH>(hg); else ss = lane_sq_sum<WT, NCH>(g);
    for (int off = G >> 1; off > 0; off >>= 1) ss = ss + __shfl_xor(ss, off, G);
    if (r < 0 || r >= a.momentum_rows) return;
    const float mr = a.momentum[r] + ss / (float)a.dim;
    mult = lr / (sqrtf(mr) + a.eps);
    if (gl == 0) a.momentum[r] = mr;
  }
  uint64_t row_key = 0;
  if (STOCH) row_key = mix64(step_key ^ (uint64_t)r);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int idx = gl + c * G;
    if (idx >= a.rowlen) continue;
    VT x;
    if constexpr (WD) x = fnma(hg[c], mult, w0[c]); else x = fnma(g[c], mult, T::up(W[idx]));
    if constexpr (STOCH) {
      const uint64_t h = mix64(row_key + (uint64_t)idx);         // 16 bits for each of the chunk's 4 elements
      typename T::V o;
      o.x = round_stochastic(x.x, (uint32_t)h, WT{});
      o.y = round_stochastic(x.y, (uint32_t)(h >> 16), WT{});
      o.z = round_stochastic(x.z, (uint32_t)(h >> 32), WT{});
      o.w = round_stochastic(x.w, (uint32_t)(h >> 48), WT{});
      W[idx] = o;
    } else {
      W[idx] = T::down(x);
    }
  }
}

// a lane's chunks of one row of an fp32 buffer: read (zero past rowlen), and written back as zero
template <typename VT, int NCH>
__device__ __forceinline__ void load_row(VT (&g)[NCH], const VT* row, int gl, int G, int rowlen) {
#pragma unroll
  for (int c = 0; c < NCH; ++c) g[c] = gl + c * G < rowlen ? row[gl + c * G] : vzero<VT>();
}
template <typename VT, int NCH> __device__ __forceinline__ void zero_row(VT* row, int gl, int G, int rowlen) {
#pragma unroll
  for (int c = 0; c < NCH; ++c)
    if (gl + c * G < rowlen) row[gl + c * G] = vzero<VT>();
}

// ---------------------------------------------------------------------------------------------------------------
// The wave walk: one wave per 64 consecutive positions (grid-stride), the positions that hold work handed to the
// wave's lane groups in rounds.

struct LaneGroup {
  int G, lane, q, gl, ngw;            // lanes per group; lane in the wave; group in the wave; lane in the group; groups
  int64_t wave, nwaves;
};
__device__ __forceinline__ LaneGroup lane_group(int g_log2) {
  LaneGroup l;
  l.G = 1 << g_log2;
  l.lane = threadIdx.x & 63;
  l.q = l.lane >> g_log2;
  l.gl = l.lane & (l.G - 1);
  l.ngw = 64 >> g_log2;
  l.wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  l.nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  return l;
}

// body(i) once for every lane i of the wave whose `pred` is set, run by a whole lane group: group q takes the q-th
// lowest set bit, the round's ngw bits leave the mask, and the lanes of a group that got no bit skip the body (so a
// sub-wave shuffle inside it sees whole groups).  Every lane of the wave must call this.  The body captures BY VALUE:
// by reference the kernel's locals are reached through the closure, which costs registers.
template <typename F> __device__ __forceinline__ void for_each_flagged(bool pred, const LaneGroup& l, F&& body) {
  unsigned long long m = __ballot(pred);
  while (m) {
    unsigned long long mm = m;
    for (int k = 0; k < l.q; ++k) mm &= mm - 1;
    for (int k = 0; k < l.ngw; ++k) m &= m - 1;
    if (mm == 0) continue;
    body(__ffsll((long long)mm) - 1);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Cache-sized accumulator.  The workspace (acc + flags, zero-filled by its owner once and left zero-filled by every
// call, so no memset runs between steps) and, for a 16-bit table, one 64-bit step counter behind it.  fp32 atomics
// cannot land on 16-bit rows and a 16-bit atomic per partial sum would round once per lookup, so there the step's
// gradient is folded into the fp32 accumulator as well and the row is rounded ONCE.

// flags[slot] = 1 for every slot the step looks up (plain byte stores; racing writers all store the same value); the
// first launch of a step also counts it (counter: NULL where nothing reads it, an fp32 table)
__global__ __launch_bounds__(256) void k_mark_slots(const int64_t* __restrict__ slots, int64_t n, uint32_t num_rows,
                                                    uint8_t* __restrict__ flags, unsigned long long* counter) {
  if (counter && blockIdx.x == 0 && threadIdx.x == 0) *counter = *counter + 1;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t s = slots[i];
    if (s >= 0 && s < (int64_t)num_rows) flags[s] = 1;
  }
}

// k_mark_slots for Adam and for every update with weight decay, where a row that is merely flagged CHANGES (its moments
// decay, its weights decay): only the lookups some bag covers -- positions [offsets[0], end of the last bag) -- flag
// their slot.  The counter is the caller's step count (Adam), the workspace's, or NULL.
__global__ __launch_bounds__(256) void k_mark_slots_covered(const int64_t* __restrict__ slots, int64_t n,
                                                            uint32_t num_rows, const void* __restrict__ offsets,
                                                            int off64, int64_t num_bags, int include_last,
                                                            uint8_t* __restrict__ flags, unsigned long long* counter) {
  if (counter && blockIdx.x == 0 && threadIdx.x == 0) *counter = *counter + 1;
  int64_t lo = off64 ? ((const int64_t*)offsets)[0] : ((const int32_t*)offsets)[0];
  int64_t hi = n;
  if (include_last) hi = off64 ? ((const int64_t*)offsets)[num_bags] : ((const int32_t*)offsets)[num_bags];
  if (lo < 0) lo = 0;
  if (hi > n) hi = n;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += stride) {
    const int64_t s = slots[i];
    if (s >= 0 && s < (int64_t)num_rows) flags[s] = 1;
  }
}

// source-row keys (row << 32 | grad_out row); row 0xffffffff = ignored lookup / padding of the last segment
__global__ __launch_bounds__(256) void k_mark_keys(const unsigned long long* __restrict__ keys, int64_t n,
                                                   uint32_t num_rows, uint8_t* __restrict__ flags,
                                                   unsigned long long* counter) {
  if (counter && blockIdx.x == 0 && threadIdx.x == 0) *counter = *counter + 1;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint32_t s = (uint32_t)(keys[i] >> 32);
    if (s < num_rows) flags[s] = 1;
  }
}

struct ApplyArgs {
  UpdateArgs u;
  float* acc;                // [num_rows, D], zero outside a call
  uint8_t* flags;            // [num_rows], zero outside a call
  uint32_t num_rows;
  RowClip clip;              // the CLIP = true instantiations only
};

// a wave reads 64 flags at once, and a lane group per flagged slot reads acc, updates the row and writes acc and the
// flag back to zero
template <typename VT, typename WT, int NCH, bool ADAGRAD, bool STOCH, bool ADAM = false, bool WD = false,
          bool ROWV = false, bool CLIP = false, bool ELEM = false>
__global__ __launch_bounds__(256) void k_rows_apply(ApplyArgs a) {
  const LaneGroup l = lane_group(a.u.g_log2);
  VT* A = (VT*)a.acc;
  const uint64_t key = step_key<STOCH>(a.u);
  const float lr = ELEM ? (float)adagrad_rate(a.u) : (ADAM ? adam_step_size(a.u) : learning_rate(a.u));
  const float f = !WD ? 1.f
                      : (ELEM ? adagrad_decay_factor(adagrad_rate(a.u), a.u.wd)
                              : decay_factor(learning_rate(a.u), a.u.wd));
  for (int64_t base = l.wave * 64; base < (int64_t)a.num_rows; base += l.nwaves * 64) {
    const int64_t mine = base + l.lane;
    const bool flagged = mine < (int64_t)a.num_rows && a.flags[mine] != 0;
    for_each_flagged(flagged, l, [=](int i) {
      const int64_t s = base + i;
      VT g[NCH];
      load_row(g, A + s * a.u.rowlen, l.gl, l.G, a.u.rowlen);
      update_row<VT, WT, NCH, STOCH, ADAM, WD, ROWV, CLIP, ELEM>(a.u, lr, key, s, g, l.gl, l.G, ADAGRAD, f, a.clip);
      zero_row<VT, NCH>(A + s * a.u.rowlen, l.gl, l.G, a.u.rowlen);
    });
    if (flagged) a.flags[mine] = 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Deterministic, accumulator-free form (ce_bag_backward_update_sorted).  The lookups are stably sorted
// by row (sorted_rows, ce_sort.hip), so a row's lookups are one run in ascending lookup position.  The run is cut into
// chunks of CE_SORTED_CHUNK positions counted from the START OF THE RUN; a lane group folds one chunk sequentially from
// zero in registers (k_sorted_fold).  A run of one chunk is applied right there; the chunks of a longer run go to a
// partial row each and a second launch (k_sorted_combine) adds a run's partials in ascending chunk order and applies
// the row once.  Nothing depends on the grid, on the slot a row sits in or on timing.
// Partial rows: the chunk that starts at sorted position p takes row 2 * (p / 64) + (first chunk of its run).  Runs
// that own partial rows are longer than 64, so an aligned block of 64 positions holds at most one run start of that
// kind and at most one later chunk start: 2 * ceil(nnz / 64) rows, no compaction, no counter.
// A 16-bit row is stored with the nearest cast; CE_ROUND_STOCHASTIC on a 16-bit table is refused by the entry.
static_assert(CE_SORTED_CHUNK == 64, "the partial-row numbering and the wave walk assume 64 positions per chunk");

struct SortedArgs {
  void* weight;                // [num_rows, D] of WT
  const void* grad_out;        // of AT
  float* partials;             // [2 * ceil(nnz / 64), D]
  const int32_t* rows_sorted;
  const int32_t* lookup_sorted;
  const int32_t* bag_of;
  const void* offsets;
  const float* psw;
  const int32_t* row_of_slot;
  float* momentum;
  int64_t momentum_rows;
  int64_t nnz;
  int64_t num_bags;
  int32_t num_rows;
  int32_t rowlen, g_log2, dim, off64, include_last, mode, hookF, hookB, adagrad;
  float lr;
  float eps;
  float wd;                    // weight decay (the WD = true instantiations): CE_WD_L2 or CE_WD_DECOUPLED
  int32_t wd_mode;             // (the CLIP = true instantiations: CE_WD_NONE as well, with wd = 0)
  float clip;                  // gradient clipping (the CLIP = true instantiations): CE_CLIP_VALUE or CE_CLIP_ROW_NORM
  int32_t clip_mode;
};

// first position of the run of `row` that holds position p (rows ascending, rows[p] == row): gallop back, then bisect
__device__ __forceinline__ int64_t run_start(const int32_t* __restrict__ rows, int64_t p, int32_t row) {
  int64_t hi = p, lo = p - 1, step = 1;
  while (lo >= 0 && rows[lo] == row) {
    hi = lo;
    step <<= 1;
    lo = p - step;
  }
  if (lo < 0) lo = -1;
  while (hi - lo > 1) {                          // rows[hi] == row, lo == -1 or rows[lo] != row
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (rows[mid] == row) hi = mid; else lo = mid;
  }
  return hi;
}

// The decay's three uniform values of a sorted launch, worked out once per thread at the top of the kernel.  parked():
// the same values moved into VECTOR registers.  k_sorted_fold without decay already uses every scalar register the
// compiler may hand out (NCH = 4: 106), so three more scalars that live across its fold loop would be spilled; a lane
// has vector registers to spare, and a value the compiler cannot see to be uniform stays in one.
struct SortedDecay {
  float wd = 0.f, f = 1.f;     // CE_WD_L2's factor of w in h; CE_WD_DECOUPLED's factor of w (decay_factor of the float lr)
  int l2 = 0;
  RowClip clip;                // the CLIP = true instantiations: the threshold and the mode, parked like the rest
};
__device__ __forceinline__ float parked(float x) {
  float v;
  asm volatile("v_mov_b32 %0, %1" : "=v"(v) : "s"(x));
  return v;
}
__device__ __forceinline__ int64_t parked(int64_t x) {
  const uint32_t lo = __float_as_uint(parked(__uint_as_float((uint32_t)x)));
  const uint32_t hi = __float_as_uint(parked(__uint_as_float((uint32_t)((uint64_t)x >> 32))));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ SortedDecay sorted_decay(const SortedArgs& a, bool park) {
  SortedDecay d;
  d.wd = a.wd;
  d.f = decay_factor(a.lr, a.wd);
  d.l2 = a.wd_mode == CE_WD_L2;
  if (park) {
    d.wd = parked(d.wd);
    d.f = parked(d.f);
    d.l2 = __float_as_int(parked(__int_as_float(d.l2)));
  }
  return d;
}
// the same for a clipped launch: the decay's values (CE_WD_NONE: wd = 0, so f = 1 and l2 = 0) and the clip's two
__device__ __forceinline__ SortedDecay sorted_decay_clip(const SortedArgs& a, bool park) {
  SortedDecay d = sorted_decay(a, park);
  d.clip.c = a.clip;
  d.clip.mode = a.clip_mode;
  if (park) {
    d.clip.c = parked(d.clip.c);
    d.clip.mode = __float_as_int(parked(__int_as_float(d.clip.mode)));
  }
  return d;
}

// the update of one row by its lane group: g = the row's whole gradient of the step (zero in chunks past rowlen).
// WD: the decayed update, its terms spelled as update_row spells them (the row read once, before the reduction; f is
// decay_factor of the float lr) -- a row looked up once gets the bits of the atomic forms.
// CLIP (then WD as well, as in update_row): clip_row on a copy of g, then the WD update of that copy.
template <typename VT, typename WT, int NCH, bool WD = false, bool CLIP = false>
__device__ __forceinline__ void sorted_apply_row(const SortedArgs& a, int64_t s, const VT (&g)[NCH], int gl, int G,
                                                 SortedDecay d = SortedDecay{}) {
  using T = Act<WT, VT>;
  if constexpr (CLIP) {
    static_assert(WD, "the clipped instantiations take the decay as a run-time mode");
    VT cg[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) cg[c] = g[c];
    // the mode comes back out of its parked register only here, so the branch on it is a scalar one: a branch on a
    // vector register would hold a saved exec mask in two more scalars across clip_row
    clip_row<WT, VT, NCH>(cg, RowClip{d.clip.c, __builtin_amdgcn_readfirstlane(d.clip.mode)}, G);
    sorted_apply_row<VT, WT, NCH, true, false>(a, s, cg, gl, G, d);
    return;
  }
  typename T::V* W = (typename T::V*)a.weight;
  if constexpr (WD) {
#pragma clang fp contract(off)
    const bool l2 = d.l2 != 0;
    const float f = d.f;
    typename T::V* Ws = W + s * a.rowlen;
    const int64_t r = a.row_of_slot ? (int64_t)a.row_of_slot[s] : s;
    VT w0[NCH], hg[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int idx = gl + c * G;
      w0[c] = idx < a.rowlen ? T::up(Ws[idx]) : vzero<VT>();
      hg[c] = g[c];
      if (l2) hg[c] = g[c] + w0[c] * d.wd; else w0[c] = w0[c] * f;
    }
    float mult = a.lr;
    if (a.adagrad) {
      float ss = lane_sq_sum<WT, NCH>(hg);
      for (int off = G >> 1; off > 0; off >>= 1) ss = ss + __shfl_xor(ss, off, G);
      if (r < 0 || r >= a.momentum_rows) return;
      const float mr = a.momentum[r] + ss / (float)a.dim;
      mult = a.lr / (sqrtf(mr) + a.eps);
      if (gl == 0) a.momentum[r] = mr;
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int idx = gl + c * G;
      if (idx < a.rowlen) Ws[idx] = T::down(fnma(hg[c], mult, w0[c]));
    }
    return;
  }
  float ss = lane_sq_sum<WT, NCH>(g);
  const int64_t r = a.row_of_slot ? (int64_t)a.row_of_slot[s] : s;
  float mult = a.lr;
  bool update = true;
  if (a.adagrad) {
    for (int off = G >> 1; off > 0; off >>= 1) ss += __shfl_xor(ss, off, G);
    update = r >= 0 && r < a.momentum_rows;
    if (update) {
      const float mr = a.momentum[r] + ss / (float)a.dim;
      mult = a.lr / (sqrtf(mr) + a.eps);
      if (gl == 0) a.momentum[r] = mr;
    }
  }
  if (!update) return;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int idx = gl + c * G;
    if (idx < a.rowlen) W[s * a.rowlen + idx] = T::down(T::up(W[s * a.rowlen + idx]) - g[c] * mult);
  }
}

// one wave per 64 consecutive sorted positions (grid-stride): every lane finds out whether its position starts a chunk,
// the chunk heads are handed to the wave's lane groups in rounds (the walk for_each_flagged wraps, written out)
template <typename VT, typename AT, typename WT, int NCH, bool WD = false, bool CLIP = false>
__global__ __launch_bounds__(256) void k_sorted_fold(SortedArgs a) {
  using TA = Act<AT, VT>;
  SortedDecay dec;
  if constexpr (CLIP) dec = sorted_decay_clip(a, true);
  else if constexpr (WD) dec = sorted_decay(a, true);
  const int G = 1 << a.g_log2;
  const int lane = threadIdx.x & 63;
  const int q = lane >> a.g_log2;
  const int gl = lane & (G - 1);
  const int ngw = 64 >> a.g_log2;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const typename TA::V* GO = (const typename TA::V*)a.grad_out;
  VT* P = (VT*)a.partials;
  const int32_t* __restrict__ rows = a.rows_sorted;
  // the walk's stride: a clipped launch parks it too -- it lives across everything, `base` is a vector value anyway,
  // and its two scalar registers are the two the clip's branches need
  int64_t stride = nwaves * 64;
  if constexpr (CLIP) stride = parked(stride);
  for (int64_t base = wave * 64; base < a.nnz; base += stride) {
    const int64_t mine = base + lane;
    bool head = false;
    if (mine < a.nnz) {
      const int32_t row = rows[mine];
      // ignored lookups carry the key num_rows and lie behind every valid row: they start nothing
      if ((uint32_t)row < (uint32_t)a.num_rows)
        head = ((mine - run_start(rows, mine, row)) & (CE_SORTED_CHUNK - 1)) == 0;
    }
    unsigned long long m = __ballot(head);
    while (m) {
      unsigned long long mm = m;
      for (int k = 0; k < q; ++k) mm &= mm - 1;          // this group's chunk: the q-th lowest head
      for (int k = 0; k < ngw; ++k) m &= m - 1;
      if (mm == 0) continue;
      const int64_t p = base + (__ffsll((long long)mm) - 1);
      const int32_t row = rows[p];
      const bool first = p == 0 || rows[p - 1] != row;                                   // first chunk of its run
      const bool more = p + CE_SORTED_CHUNK < a.nnz && rows[p + CE_SORTED_CHUNK] == row;   // a chunk follows
      VT g[NCH];
#pragma unroll
      for (int c = 0; c < NCH; ++c) g[c] = vzero<VT>();
      const int64_t end = p + CE_SORTED_CHUNK < a.nnz ? p + CE_SORTED_CHUNK : a.nnz;
      for (int64_t t = p; t < end && rows[t] == row; ++t) {
        const int32_t j = a.lookup_sorted[t];
        const int64_t bag = a.bag_of[j];
        if (bag < 0 || bag >= a.num_bags) continue;        // a lookup no bag covers
        float sc = a.psw ? a.psw[j] : 1.f;
        if (a.mode == CE_MODE_MEAN) {
          const int64_t lo = a.off64 ? ((const int64_t*)a.offsets)[bag] : ((const int32_t*)a.offsets)[bag];
          const int64_t hi = (a.include_last || bag + 1 < a.num_bags)
                                 ? (a.off64 ? ((const int64_t*)a.offsets)[bag + 1] : ((const int32_t*)a.offsets)[bag + 1])
                                 : a.nnz;
          if (hi - lo > 1) sc = sc / (float)(hi - lo);
        }
        int64_t orow = bag;
        if (a.hookF) {
          const int64_t f = bag / a.hookB;
          orow = (bag - f * a.hookB) * a.hookF + f;
        }
        {
#pragma clang fp contract(off)      // the specification: the term s_j g_j is rounded before it is added
#pragma unroll
          for (int c = 0; c < NCH; ++c) {
            const int idx = gl + c * G;
            if (idx < a.rowlen) {
              const VT v = TA::up(GO[orow * a.rowlen + idx]);
              g[c] = (sc == 1.f) ? g[c] + v : g[c] + v * sc;
            }
          }
        }
      }
      if (first && !more) {
        sorted_apply_row<VT, WT, NCH, WD, CLIP>(a, (int64_t)row, g, gl, G, dec);
      } else {
        const int64_t prow = 2 * (p >> 6) + (first ? 1 : 0);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const int idx = gl + c * G;
          if (idx < a.rowlen) P[prow * a.rowlen + idx] = g[c];
        }
      }
    }
  }
}

// the runs of more than one chunk: the head of such a run adds its partial rows in ascending chunk order and applies
template <typename VT, typename WT, int NCH, bool WD = false, bool CLIP = false>
__global__ __launch_bounds__(256) void k_sorted_combine(SortedArgs a) {
  SortedDecay dec;
  if constexpr (CLIP) dec = sorted_decay_clip(a, false);
  else if constexpr (WD) dec = sorted_decay(a, false);
  const int G = 1 << a.g_log2;
  const int lane = threadIdx.x & 63;
  const int q = lane >> a.g_log2;
  const int gl = lane & (G - 1);
  const int ngw = 64 >> a.g_log2;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const VT* P = (const VT*)a.partials;
  const int32_t* __restrict__ rows = a.rows_sorted;
  for (int64_t base = wave * 64; base < a.nnz; base += nwaves * 64) {
    const int64_t mine = base + lane;
    bool head = false;
    if (mine + CE_SORTED_CHUNK < a.nnz) {
      const int32_t row = rows[mine];
      head = (uint32_t)row < (uint32_t)a.num_rows && (mine == 0 || rows[mine - 1] != row) &&
             rows[mine + CE_SORTED_CHUNK] == row;
    }
    unsigned long long m = __ballot(head);
    while (m) {
      unsigned long long mm = m;
      for (int k = 0; k < q; ++k) mm &= mm - 1;
      for (int k = 0; k < ngw; ++k) m &= m - 1;
      if (mm == 0) continue;
      const int64_t p = base + (__ffsll((long long)mm) - 1);
      const int32_t row = rows[p];
      VT g[NCH];
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int idx = gl + c * G;
        g[c] = idx < a.rowlen ? P[(2 * (p >> 6) + 1) * a.rowlen + idx] : vzero<VT>();
      }
      for (int64_t t = p + CE_SORTED_CHUNK; t < a.nnz && rows[t] == row; t += CE_SORTED_CHUNK) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const int idx = gl + c * G;
          if (idx < a.rowlen) g[c] = g[c] + P[(2 * (t >> 6)) * a.rowlen + idx];
        }
      }
      sorted_apply_row<VT, WT, NCH, WD, CLIP>(a, (int64_t)row, g, gl, G, dec);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Step-sized accumulator (ce_bag_backward_update_compact*).  The cache-sized form folds the step's
// gradient into acc[num_rows, D]; a step touches at most cap = min(nnz, num_rows) distinct slots, so here the flagged
// slots are numbered 0 .. U-1 in ascending order and the SAME dense backward scatters into acc[cap, D] through the
// renumbered indices / keys.  One stream, no host synchronisation, no allocation, launch shapes fixed by the arguments
// (U stays on the device and is read by the apply kernel):
//   1. k_mark_*: flags[slot] = 1, the step counter += 1 (a 16-bit table);
//   2. k_compact_count + k_compact_emit: list[u] = the u-th flagged slot, cidx[slot] = u, U; the flags go back to zero;
//   3. k_compact_remap_slots / _keys: slots -> cidx[slot] (-1 outside [0, num_rows)), row << 32 | x -> cidx[row] << 32 | x;
//   4. ce_bag_backward_dense_act / _dense_src_act (unchanged) into acc[cap, D] with num_rows = cap;
//   5. k_compact_apply: a lane group per u < U updates the row in slot list[u] and zeroes acc[u].
// cidx is written for flagged slots only and read for flagged slots only (a lookup the remap reads was marked in this
// call), so it is never initialised and never cleared; list and the remap buffer likewise.
constexpr int kCompactRounds = 16;                                   // 64-slot ballots per wave
constexpr int kCompactWave = 64 * kCompactRounds;                    // consecutive slots per wave
static_assert(CE_COMPACT_BLOCK == 4 * kCompactWave, "a scan workgroup is four waves of kCompactRounds ballots");

__device__ __forceinline__ int compact_wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// flagged slots of every scan workgroup (CE_COMPACT_BLOCK consecutive slots): one lane per slot and round
__global__ __launch_bounds__(256) void k_compact_count(const uint8_t* __restrict__ flags, uint32_t num_rows,
                                                       int32_t* __restrict__ blk_count) {
  __shared__ int wcnt[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t base = (int64_t)blockIdx.x * CE_COMPACT_BLOCK + w * kCompactWave + lane;
  int n = 0;
#pragma unroll
  for (int r = 0; r < kCompactRounds; ++r) {
    const int64_t s = base + r * 64;
    n += __popcll(__ballot(s < (int64_t)num_rows && flags[s] != 0));
  }
  if (lane == 0) wcnt[w] = n;
  __syncthreads();
  if (threadIdx.x == 0) blk_count[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

// every workgroup adds up the counts of the workgroups before its own (k_free_emit's cross-block prefix: a few KB out
// of L2, no scan launch), the waves' totals go through LDS, a lane's place in its round is a popcount of the ballot
// below it.  Nothing returns from an atomic.  u < cap always holds when the flags came from this call's mark (at most
// min(nnz, num_rows) distinct slots); a slot past it -- a workspace that was not zero -- is dropped, never written.
__global__ __launch_bounds__(256) void k_compact_emit(uint8_t* __restrict__ flags, uint32_t num_rows,
                                                      const int32_t* __restrict__ blk_count, int32_t* __restrict__ cidx,
                                                      int32_t* __restrict__ list, uint32_t cap, int32_t* __restrict__ n_out) {
  __shared__ int wbefore[4];
  __shared__ int wcnt[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int part = 0;
  for (int i = threadIdx.x; i < (int)blockIdx.x; i += 256) part += blk_count[i];
  part = compact_wave_sum(part);
  const int64_t base = (int64_t)blockIdx.x * CE_COMPACT_BLOCK + w * kCompactWave + lane;
  unsigned long long b[kCompactRounds];
  int n = 0;
#pragma unroll
  for (int r = 0; r < kCompactRounds; ++r) {
    const int64_t s = base + r * 64;
    const bool f = s < (int64_t)num_rows && flags[s] != 0;
    b[r] = __ballot(f);
    n += __popcll(b[r]);
    if (f) flags[s] = 0;
  }
  if (lane == 0) {
    wbefore[w] = part;
    wcnt[w] = n;
  }
  __syncthreads();
  const long long before = (long long)wbefore[0] + wbefore[1] + wbefore[2] + wbefore[3];
  long long pos = before;
  for (int k = 0; k < w; ++k) pos += wcnt[k];
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int r = 0; r < kCompactRounds; ++r) {
    if ((b[r] >> lane) & 1ull) {
      const int64_t s = base + r * 64;
      const long long u = pos + __popcll(b[r] & below);
      if (u < (long long)cap) list[u] = (int32_t)s;
      cidx[s] = u < (long long)cap ? (int32_t)u : -1;
    }
    pos += __popcll(b[r]);
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    const long long total = before + wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    *n_out = (int32_t)(total < (long long)cap ? total : (long long)cap);
  }
}

__global__ __launch_bounds__(256) void k_compact_remap_slots(const int64_t* __restrict__ slots, int64_t n,
                                                             uint32_t num_rows, const int32_t* __restrict__ cidx,
                                                             uint32_t cap, int64_t* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t s = slots[i];
    int64_t c = -1;
    if (s >= 0 && s < (int64_t)num_rows) c = cidx[s];
    out[i] = (uint64_t)c < (uint64_t)cap ? c : -1;          // (a number outside [0, cap) is never handed on)
  }
}

// keys = row << 32 | low word (the lookup's place in its segment, or the row of grad_out it reads): the low word and
// the order stay, so rows that were adjacent stay adjacent (the map is injective on flagged slots).  Padding (~0) and
// ignored rows stay what they are; a row outside [0, num_rows) -- which no presort writes -- becomes ignored: all ones
// in the segment-sorted form (whole_key), 0xffffffff in the row half of a source-row key.
__global__ __launch_bounds__(256) void k_compact_remap_keys(const unsigned long long* __restrict__ keys, int64_t n,
                                                            uint32_t num_rows, const int32_t* __restrict__ cidx,
                                                            uint32_t cap, int whole_key,
                                                            unsigned long long* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const unsigned long long k = keys[i];
    const uint32_t row = (uint32_t)(k >> 32);
    unsigned long long o = whole_key ? ~0ull : (k | 0xffffffff00000000ull);
    if (k == ~0ull) {
      o = k;
    } else if (row < num_rows) {
      const uint32_t c = (uint32_t)cidx[row];
      if (c < cap) o = ((unsigned long long)c << 32) | (k & 0xffffffffull);
    }
    out[i] = o;
  }
}

struct CompactArgs {
  UpdateArgs u;
  float* acc;                // [cap, D], zero outside a call
  const int32_t* list;       // [cap]: list[u] = the u-th flagged slot
  const int32_t* n_list;     // U, written by k_compact_emit
  int32_t adagrad;
  RowClip clip;              // the CLIP = true instantiations only
};

// one lane group per list entry (grid-stride over u < U; the grid is sized by cap)
template <typename VT, typename WT, int NCH, bool STOCH, bool ADAM = false, bool WD = false, bool ROWV = false,
          bool CLIP = false, bool ELEM = false>
__global__ __launch_bounds__(256) void k_compact_apply(CompactArgs a) {
  const int G = 1 << a.u.g_log2;
  const int gl = threadIdx.x & (G - 1);
  const int64_t grp = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> a.u.g_log2;
  const int64_t ngrp = ((int64_t)gridDim.x * blockDim.x) >> a.u.g_log2;
  VT* A = (VT*)a.acc;
  const int64_t n = *a.n_list;
  const uint64_t key = step_key<STOCH>(a.u);
  const float lr = ELEM ? (float)adagrad_rate(a.u) : (ADAM ? adam_step_size(a.u) : learning_rate(a.u));
  const float f = !WD ? 1.f
                      : (ELEM ? adagrad_decay_factor(adagrad_rate(a.u), a.u.wd)
                              : decay_factor(learning_rate(a.u), a.u.wd));
  for (int64_t u = grp; u < n; u += ngrp) {          // group-uniform
    VT g[NCH];
    load_row(g, A + u * a.u.rowlen, gl, G, a.u.rowlen);
    update_row<VT, WT, NCH, STOCH, ADAM, WD, ROWV, CLIP, ELEM>(a.u, lr, key, (int64_t)a.list[u], g, gl, G, a.adagrad,
                                                               f, a.clip);
    zero_row<VT, NCH>(A + u * a.u.rowlen, gl, G, a.u.rowlen);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Deterministic, accumulator-free form for the tables that carry their state in the row (ce_bag_backward_adam_sorted /
// _pradam_sorted / _adagrad_sorted).  The fold is 3.5's, to the letter: the sort, chunks of
// CE_SORTED_CHUNK positions counted from the start of the run, each folded sequentially from zero, the partial rows
// added in ascending chunk order.  The update is update_row's -- the arms the atomic forms run -- so a row gets the bits
// of CE_ACC_CACHE / CE_ACC_STEP given the same folded gradient.  The work is split differently from 3.5's pair:
//   1. k_count_step: the caller's step count += 1, the call's first launch;
//   2. sorted_rows(covered_only): a lookup no bag covers heads nothing, as k_mark_slots_covered flags nothing for it;
//   3. k_in_row_fold ONLY folds: every chunk, the only chunk of a short run included, goes to a partial row;
//   4. k_in_row_apply: the head of every run adds its partial rows and calls update_row once.
// k_sorted_fold folds AND applies, and at NCH = 4 it holds every scalar register there is; the in-row arms bring more
// uniforms (the step size, omb1, omb2, eps, f, the clip).  Here no kernel holds both sets.  The price: the chunk that
// starts at sorted position p takes partial row p -- nnz rows of D floats, where 3.5 needs 2 * ceil(nnz / 64) -- and a
// row looked up once pays one write and one read of D floats.  The partial rows are D floats wide whatever the layout.

__global__ void k_count_step(unsigned long long* step) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *step = *step + 1;
}

struct InRowSortedArgs {
  UpdateArgs u;                // k_in_row_apply only
  const void* grad_out;        // of AT
  float* partials;             // [nnz, D]: row p = the chunk that starts at sorted position p
  const int32_t* rows_sorted;
  const int32_t* lookup_sorted;
  const int32_t* bag_of;
  const void* offsets;
  const float* psw;
  int64_t nnz;
  int64_t num_bags;
  int32_t num_rows;
  int32_t rowlen, g_log2, off64, include_last, mode, hookF, hookB;
  RowClip clip;                // the CLIP = true instantiations of k_in_row_apply only
};

// k_sorted_fold's walk and fold loop; every chunk is written to its partial row and nothing is applied
template <typename AT, int NCH>
__global__ __launch_bounds__(256) void k_in_row_fold(InRowSortedArgs a) {
  using VT = f32x4;
  using TA = Act<AT, VT>;
  const int G = 1 << a.g_log2;
  const int lane = threadIdx.x & 63;
  const int q = lane >> a.g_log2;
  const int gl = lane & (G - 1);
  const int ngw = 64 >> a.g_log2;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const typename TA::V* GO = (const typename TA::V*)a.grad_out;
  VT* P = (VT*)a.partials;
  const int32_t* __restrict__ rows = a.rows_sorted;
  for (int64_t base = wave * 64; base < a.nnz; base += nwaves * 64) {
    const int64_t mine = base + lane;
    bool head = false;
    if (mine < a.nnz) {
      const int32_t row = rows[mine];
      // ignored and uncovered lookups carry the key num_rows and lie behind every valid row: they start nothing
      if ((uint32_t)row < (uint32_t)a.num_rows)
        head = ((mine - run_start(rows, mine, row)) & (CE_SORTED_CHUNK - 1)) == 0;
    }
    unsigned long long m = __ballot(head);
    while (m) {
      unsigned long long mm = m;
      for (int k = 0; k < q; ++k) mm &= mm - 1;          // this group's chunk: the q-th lowest head
      for (int k = 0; k < ngw; ++k) m &= m - 1;
      if (mm == 0) continue;
      const int64_t p = base + (__ffsll((long long)mm) - 1);
      const int32_t row = rows[p];
      VT g[NCH];
#pragma unroll
      for (int c = 0; c < NCH; ++c) g[c] = vzero<VT>();
      const int64_t end = p + CE_SORTED_CHUNK < a.nnz ? p + CE_SORTED_CHUNK : a.nnz;
      for (int64_t t = p; t < end && rows[t] == row; ++t) {
        const int32_t j = a.lookup_sorted[t];
        const int64_t bag = a.bag_of[j];
        if (bag < 0 || bag >= a.num_bags) continue;        // (covered_only: no such lookup carries a valid row)
        float sc = a.psw ? a.psw[j] : 1.f;
        if (a.mode == CE_MODE_MEAN) {
          const int64_t lo = a.off64 ? ((const int64_t*)a.offsets)[bag] : ((const int32_t*)a.offsets)[bag];
          const int64_t hi = (a.include_last || bag + 1 < a.num_bags)
                                 ? (a.off64 ? ((const int64_t*)a.offsets)[bag + 1] : ((const int32_t*)a.offsets)[bag + 1])
                                 : a.nnz;
          if (hi - lo > 1) sc = sc / (float)(hi - lo);
        }
        int64_t orow = bag;
        if (a.hookF) {
          const int64_t f = bag / a.hookB;
          orow = (bag - f * a.hookB) * a.hookF + f;
        }
        {
#pragma clang fp contract(off)      // the specification: the term s_j g_j is rounded before it is added
#pragma unroll
          for (int c = 0; c < NCH; ++c) {
            const int idx = gl + c * G;
            if (idx < a.rowlen) {
              const VT v = TA::up(GO[orow * a.rowlen + idx]);
              g[c] = (sc == 1.f) ? g[c] + v : g[c] + v * sc;
            }
          }
        }
      }
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int idx = gl + c * G;
        if (idx < a.rowlen) P[p * a.rowlen + idx] = g[c];
      }
    }
  }
}

// the head of every run of a valid row adds the run's partial rows in ascending chunk order and updates the row once
template <int NCH, bool ADAM, bool WD, bool ROWV, bool CLIP, bool ELEM>
__global__ __launch_bounds__(256) void k_in_row_apply(InRowSortedArgs a) {
  using VT = f32x4;
  const LaneGroup l = lane_group(a.g_log2);
  const VT* P = (const VT*)a.partials;
  const int32_t* __restrict__ rows = a.rows_sorted;
  const float lr = ELEM ? (float)adagrad_rate(a.u) : adam_step_size(a.u);
  const float f = !WD ? 1.f
                      : (ELEM ? adagrad_decay_factor(adagrad_rate(a.u), a.u.wd)
                              : decay_factor(learning_rate(a.u), a.u.wd));
  for (int64_t base = l.wave * 64; base < a.nnz; base += l.nwaves * 64) {
    const int64_t mine = base + l.lane;
    bool head = false;
    if (mine < a.nnz) {
      const int32_t row = rows[mine];
      head = (uint32_t)row < (uint32_t)a.num_rows && (mine == 0 || rows[mine - 1] != row);
    }
    for_each_flagged(head, l, [=](int i) {
      const int64_t p = base + i;
      const int32_t row = rows[p];
      VT g[NCH];
      load_row(g, P + p * a.rowlen, l.gl, l.G, a.rowlen);
      for (int64_t t = p + CE_SORTED_CHUNK; t < a.nnz && rows[t] == row; t += CE_SORTED_CHUNK) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const int idx = l.gl + c * l.G;
          if (idx < a.rowlen) g[c] = g[c] + P[t * a.rowlen + idx];
        }
      }
      update_row<VT, float, NCH, false, ADAM, WD, ROWV, CLIP, ELEM>(a.u, lr, 0, (int64_t)row, g, l.gl, l.G, false, f,
                                                                    a.clip);
    });
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Host side: the workspaces, the one check, the launches

static inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

// cache-sized: acc, flags, and the step counter of a 16-bit table
struct ApplyWs {
  float* acc;
  uint8_t* flags;
  unsigned long long* counter;        // NULL for an fp32 table
  size_t bytes;
};

static ApplyWs carve_apply(void* ws, int64_t num_rows, int32_t dim, bool w16) {
  ApplyWs w{};
  char* p = (char*)ws;
  size_t o = 0;
  w.acc = (float*)(p + o);     o = al256(o + (size_t)num_rows * dim * 4);
  w.flags = (uint8_t*)(p + o); o = al256(o + (size_t)num_rows);
  if (w16) {
    w.counter = (unsigned long long*)(p + o);
    o += 256;
  }
  w.bytes = o;
  return w;
}

// sorted: the sort arrays, then the partial rows; nothing in it needs initialising
struct SortedWs {
  void* sort;
  float* partials;
  size_t bytes;
};

static SortedWs carve_sorted(void* ws, int64_t nnz, int32_t dim) {
  const int64_t n = nnz < 1 ? 1 : nnz;
  SortedWs w{};
  char* p = (char*)ws;
  size_t o = 0;
  w.sort = p + o;                           o = al256(o + sorted_rows_bytes(n));
  w.partials = (float*)(p + o);             o = al256(o + (size_t)(2 * cdiv(n, CE_SORTED_CHUNK)) * (size_t)dim * 4);
  w.bytes = o;
  return w;
}

// step-sized: what must be zero outside a call (flags, acc) and the step counter, then what needs no initialising.
// The layout depends on num_rows, nnz and dim: a workspace serves ONE such triple (its owner zero-fills it again,
// counter apart, before it serves another).
struct CompactWs {
  unsigned long long* counter;
  int32_t* n_list;
  uint8_t* flags;            // [num_rows]
  float* acc;                // [cap, dim]
  int32_t* cidx;             // [num_rows]
  int32_t* blk_count;        // [ceil(num_rows / CE_COMPACT_BLOCK)]
  int32_t* list;             // [cap]
  void* remap;               // [ce_bag_presort_len(nnz)] x 8 bytes
  int64_t cap;
  size_t bytes;
};

static CompactWs carve_compact(void* ws, int64_t num_rows, int64_t nnz, int32_t dim) {
  CompactWs w{};
  w.cap = nnz < num_rows ? nnz : num_rows;
  char* p = (char*)ws;
  size_t o = 0;
  w.counter = (unsigned long long*)(p + o);  o += 256;
  w.n_list = (int32_t*)(p + o);              o += 256;
  w.flags = (uint8_t*)(p + o);               o = al256(o + (size_t)num_rows);
  w.acc = (float*)(p + o);                   o = al256(o + (size_t)w.cap * dim * 4);
  w.cidx = (int32_t*)(p + o);                o = al256(o + (size_t)num_rows * 4);
  w.blk_count = (int32_t*)(p + o);           o = al256(o + (size_t)cdiv(num_rows, CE_COMPACT_BLOCK) * 4);
  w.list = (int32_t*)(p + o);                o = al256(o + (size_t)w.cap * 4);
  w.remap = p + o;                           o = al256(o + (size_t)ce_bag_presort_len(nnz) * 8);
  w.bytes = o;
  return w;
}

constexpr int32_t kOptAdam = 2;       // beside CE_OPT_*: library-internal, no `optimizer` argument takes it
constexpr int32_t kOptPartialAdam = 3;   // partial row-wise Adam (rows w | m, the second moment in `momentum`): likewise
constexpr int32_t kOptElemAdagrad = 4;   // element-wise Adagrad (rows w | h, the sums of squares in the row): likewise

// the arguments every update entry has (the fp32 Adagrad entries: CE_ACT_F32, CE_OPT_ROWWISE_ADAGRAD, CE_ROUND_NEAREST)
struct UpdateCall {
  void* weight;
  int32_t weight_dtype;
  int64_t num_rows;
  int32_t dim;
  int64_t nnz;
  const void* grad_out;
  int32_t act;
  const int32_t* row_of_slot;
  float* momentum;
  int64_t momentum_rows;
  float lr, eps;
  int32_t optimizer, rounding;
  uint64_t seed;
  void* workspace;
  size_t workspace_bytes;
  const float* lr_dev = nullptr;      // the ce_*_lrdev entries: the learning rate in device memory (`lr` is then 0)
  // the ce_bag_backward_adam* entries (optimizer = kOptAdam, an fp32 table of rows w | m | v): the caller's step count
  // takes the place of the workspace's counter
  unsigned long long* step = nullptr;
  double beta1 = 0.0, beta2 = 0.0;
  // the ce_bag_backward_adagrad* entries (optimizer = kOptElemAdagrad, an fp32 table of rows w | h): `step` as for Adam
  double lr_decay = 0.0;
  // the ce_*_wd entries: weight decay (decay() false: the call is the covered entry's, kernels and all)
  float wd = 0.f;
  int32_t wd_mode = CE_WD_NONE;
  // the ce_*_clip entries: gradient clipping (clipped() false: the call is the covered entry's, kernels and all)
  float clip = 0.f;
  int32_t clip_mode = CE_CLIP_NONE;
  bool decay() const { return wd_mode != CE_WD_NONE && wd != 0.f; }
  bool clipped() const { return clip_mode != CE_CLIP_NONE; }
  bool w16() const { return weight_dtype != CE_ACT_F32; }
  bool adagrad() const { return optimizer == CE_OPT_ROWWISE_ADAGRAD; }
  bool adam() const { return optimizer == kOptAdam || optimizer == kOptPartialAdam; }
  bool rowv() const { return optimizer == kOptPartialAdam; }     // (then adam() holds as well)
  bool elem() const { return optimizer == kOptElemAdagrad; }
  // the state travels in the row and the caller's step count is counted: a row that is merely flagged changes
  bool in_row() const { return adam() || elem(); }
  bool stochastic() const { return rounding == CE_ROUND_STOCHASTIC; }
};

static UpdateArgs update_args(const UpdateCall& c, const RowGeom& r, const unsigned long long* counter) {
  UpdateArgs u{};
  u.weight = c.weight;
  u.row_of_slot = c.row_of_slot;
  u.momentum = c.momentum;
  u.momentum_rows = c.momentum_rows;
  u.seed = c.seed;
  u.counter = counter;
  u.rowlen = r.rowlen;
  u.g_log2 = r.g_log2;
  u.dim = c.dim;
  u.lr = c.lr;
  u.eps = c.eps;
  u.lr_dev = c.lr_dev;
  if (c.elem()) u.lr_decay = c.lr_decay; else u.beta1 = c.beta1;
  u.beta2 = c.beta2;
  u.omb1 = (float)(1.0 - c.beta1);
  u.omb2 = (float)(1.0 - c.beta2);
  // (a clipped launch reads the decay's mode at run time: a call without decay is CE_WD_NONE with wd = 0 there)
  u.wd = c.decay() ? c.wd : 0.f;
  u.wd_mode = c.decay() ? c.wd_mode : CE_WD_NONE;
  return u;
}

// the two checks the ce_*_wd entries add, behind their leading checks and before everything else (also for nnz == 0)
static int wd_check(float wd, int32_t wd_mode) {
  CE_REQUIRE(wd_mode == CE_WD_NONE || wd_mode == CE_WD_L2 || wd_mode == CE_WD_DECOUPLED, CE_ERR_INVALID,
             "unknown weight_decay_mode %d (CE_WD_NONE / CE_WD_L2 / CE_WD_DECOUPLED)", (int)wd_mode);
  CE_REQUIRE(wd >= 0.f, CE_ERR_INVALID, "weight_decay must be >= 0");
  return CE_OK;
}

// the two checks the ce_*_clip entries add, directly behind the decay's (also for nnz == 0); every other entry passes
// 0 / CE_CLIP_NONE
static int clip_check(float clip, int32_t clip_mode) {
  CE_REQUIRE(clip_mode == CE_CLIP_NONE || clip_mode == CE_CLIP_VALUE || clip_mode == CE_CLIP_ROW_NORM, CE_ERR_INVALID,
             "unknown grad_clip_mode %d (CE_CLIP_NONE / CE_CLIP_VALUE / CE_CLIP_ROW_NORM)", (int)clip_mode);
  CE_REQUIRE(clip_mode == CE_CLIP_NONE || clip > 0.f, CE_ERR_INVALID, "grad_clip must be > 0");
  return CE_OK;
}

// which instantiations a call launches: a clipped call the CLIP ones (decay or not: they read its mode at run time), a
// call that decays the WD ones, every other call the instantiations from before the decay
template <bool W, bool C> struct UpdateKind {
  static constexpr bool WD = W, CLIP = C;
};
template <typename F> static inline void for_decay(bool decay, bool clipped, F&& f) {
  if (clipped) f(UpdateKind<true, true>{});
  else if (decay) f(UpdateKind<true, false>{});
  else f(UpdateKind<false, false>{});
}

// How the entries' checks differ -- everything else is the same conditions in the same order.
struct EntryRules {
  bool w16_only;             // ce_*_w16: CE_ACT_F32 is no table of theirs
  const char* not_taken;     // non-NULL: a (table, optimizer, rounding) the entry does not take: CE_ERR_UNSUPPORTED
  bool nnz_in_range;         // nnz sizes the workspace: it must lie in [0, 2^31) here (the others look at it later)
  size_t (*workspace)(int64_t num_rows, int64_t nnz, int32_t dim);
};

// Everything an atomic update entry (cache-sized or step-sized accumulator) can refuse, from the arguments alone and BEFORE its first launch (no HIP call either): the
// workspace stays as it was on every error.  r: the lane shape of the launch that updates the rows.  The row geometry
// is first asked for with the weakest alignment of all the call's launches (weight, grad_out; the accumulators are
// 256-byte aligned by their carve): a dim that fits the scalar form fits the vector form.
static int update_check(const UpdateCall& c, const EntryRules& e, RowGeom& r) {
  CE_REQUIRE_ACT(c.act);
  if (!e.w16_only)
    CE_REQUIRE(c.weight_dtype == CE_ACT_F32 || c.weight_dtype == CE_ACT_BF16 || c.weight_dtype == CE_ACT_F16,
               CE_ERR_INVALID, "unknown weight_dtype %d (CE_ACT_F32 / CE_ACT_BF16 / CE_ACT_F16)", (int)c.weight_dtype);
  const bool w16 = e.w16_only || c.w16();
  if (w16) {
    int rc = w16_check(c.weight_dtype, c.dim);
    if (rc) return rc;
  }
  CE_REQUIRE(c.optimizer == CE_OPT_SGD || c.optimizer == CE_OPT_ROWWISE_ADAGRAD, CE_ERR_INVALID,
             "unknown optimizer %d (CE_OPT_SGD / CE_OPT_ROWWISE_ADAGRAD)", (int)c.optimizer);
  CE_REQUIRE(c.rounding == CE_ROUND_NEAREST || c.rounding == CE_ROUND_STOCHASTIC, CE_ERR_INVALID,
             "unknown rounding %d (CE_ROUND_NEAREST / CE_ROUND_STOCHASTIC)", (int)c.rounding);
  CE_REQUIRE(!e.not_taken, CE_ERR_UNSUPPORTED, "%s", e.not_taken);
  CE_REQUIRE(c.weight && c.grad_out && c.workspace, CE_ERR_INVALID, "null pointer");
  CE_REQUIRE(c.dim > 0, CE_ERR_INVALID, "dim must be positive");
  CE_REQUIRE(c.num_rows > 0 && c.num_rows < (int64_t)INT32_MAX, CE_ERR_INVALID, "num_rows out of range");
  CE_REQUIRE(!e.nnz_in_range || (c.nnz >= 0 && c.nnz < (int64_t)INT32_MAX), CE_ERR_INVALID, "nnz out of range");
  CE_REQUIRE(c.lr >= 0.f, CE_ERR_INVALID, "lr must be >= 0");
  if (c.adagrad()) {
    CE_REQUIRE(c.momentum && c.momentum_rows > 0, CE_ERR_INVALID, "row-wise Adagrad needs its momentum");
    CE_REQUIRE(c.eps > 0.f, CE_ERR_INVALID, "eps must be > 0");
  }
  CE_REQUIRE(c.workspace_bytes >= e.workspace(c.num_rows, c.nnz, c.dim), CE_ERR_INVALID, "workspace too small");
  CE_REQUIRE((((uintptr_t)c.workspace) & 255) == 0, CE_ERR_INVALID, "workspace must be 256-byte aligned");
  CE_REQUIRE(!w16 || al16(c.weight), CE_ERR_INVALID, "a 16-bit table must be 16-byte aligned");
  int rc = row_geometry(c.dim, al16(c.weight) && act_aligned(c.grad_out, c.act), r);
  if (rc) return rc;
  // the scatter into acc takes the vector or the scalar form by grad_out's alignment, the apply pass by the table's
  return row_geometry(c.dim, al16(c.weight), r);
}

static void launch_mark(const void* src, bool keys, int64_t n, int64_t num_rows, uint8_t* flags,
                        unsigned long long* counter, hipStream_t s) {
  const dim3 g(grid_for(n, 256)), b(256);
  if (keys)
    hipLaunchKernelGGL(k_mark_keys, g, b, 0, s, (const unsigned long long*)src, n, (uint32_t)num_rows, flags, counter);
  else
    hipLaunchKernelGGL(k_mark_slots, g, b, 0, s, (const int64_t*)src, n, (uint32_t)num_rows, flags, counter);
}

// the lookups of the slots + offsets entries
struct SlotLookups {
  const int64_t* indices;
  const void* offsets;
  int32_t off64;
  int64_t num_bags;
  int32_t include_last;
  const float* psw;
  int32_t mode;
  int64_t hookF;
  const uint64_t* presorted;
};

// the mark pass of a call: the slots of L (Adam, weight decay: of the lookups a bag covers -- there a row that is
// merely flagged changes) or, L == NULL, the row halves of `keys` (an uncovered lookup's key is all ones already)
static void launch_mark_call(const UpdateCall& c, const SlotLookups* L, const void* keys, int64_t n, uint8_t* flags,
                             unsigned long long* counter, hipStream_t s) {
  if (L && (c.in_row() || c.decay()))
    hipLaunchKernelGGL(k_mark_slots_covered, dim3(grid_for(n, 256)), dim3(256), 0, s, L->indices, n,
                       (uint32_t)c.num_rows, L->offsets, (int)L->off64, L->num_bags, (int)L->include_last, flags, counter);
  else
    launch_mark(L ? (const void*)L->indices : keys, !L, n, c.num_rows, flags, counter, s);
}

// The cache-sized update after its check: mark `n` slots / keys of `src`, scatter(acc) = the caller's dense backward,
// apply.  An fp32 table is row-wise Adagrad with its rows stored as they are; a 16-bit table takes either optimizer and
// either rounding.
template <typename Scatter>
static int update_cache_sized(const UpdateCall& c, const RowGeom& r, const SlotLookups* L, const void* keys, int64_t n,
                              hipStream_t s, Scatter&& scatter) {
  const ApplyWs ws = carve_apply(c.workspace, c.num_rows, c.dim, c.w16());
  unsigned long long* counter = c.in_row() ? c.step : ws.counter;
  launch_mark_call(c, L, keys, n, ws.flags, counter, s);
  CE_LAUNCH_CHECK();
  int rc = scatter(ws.acc);
  if (rc) return rc;
  ApplyArgs a{};
  a.u = update_args(c, r, counter);
  a.acc = ws.acc;
  a.flags = ws.flags;
  a.num_rows = (uint32_t)c.num_rows;
  a.clip = RowClip{c.clip, c.clip_mode};
  const dim3 g(grid_for(cdiv(c.num_rows, 64), 4)), b(256);
  const bool ada = c.adagrad(), st = c.stochastic();
  for_decay(c.decay(), c.clipped(), [&](auto d) {
    constexpr bool WD = decltype(d)::WD, CL = decltype(d)::CLIP;
    if (c.elem())
      for_vec_lanes(r.nch, [&](auto l) {
        hipLaunchKernelGGL((k_rows_apply<f32x4, float, decltype(l)::NCH, false, false, false, WD, false, CL, true>), g, b,
                           0, s, a);
      });
    else if (c.rowv())
      for_vec_lanes(r.nch, [&](auto l) {
        hipLaunchKernelGGL((k_rows_apply<f32x4, float, decltype(l)::NCH, false, false, true, WD, true, CL>), g, b, 0, s,
                           a);
      });
    else if (c.adam())
      for_vec_lanes(r.nch, [&](auto l) {
        hipLaunchKernelGGL((k_rows_apply<f32x4, float, decltype(l)::NCH, false, false, true, WD, false, CL>), g, b, 0, s,
                           a);
      });
    else for_table(c.weight_dtype, r, [&](auto l, auto w) {
      using VT = typename decltype(l)::VT;
      using WT = typename decltype(w)::AT;
      constexpr int N = decltype(l)::NCH;
      if constexpr (std::is_same<WT, float>::value)
        hipLaunchKernelGGL((k_rows_apply<VT, float, N, true, false, false, WD, false, CL>), g, b, 0, s, a);
      else if (ada && st) hipLaunchKernelGGL((k_rows_apply<VT, WT, N, true, true, false, WD, false, CL>), g, b, 0, s, a);
      else if (ada) hipLaunchKernelGGL((k_rows_apply<VT, WT, N, true, false, false, WD, false, CL>), g, b, 0, s, a);
      else if (st) hipLaunchKernelGGL((k_rows_apply<VT, WT, N, false, true, false, WD, false, CL>), g, b, 0, s, a);
      else hipLaunchKernelGGL((k_rows_apply<VT, WT, N, false, false, false, WD, false, CL>), g, b, 0, s, a);
    });
  });
  CE_LAUNCH_CHECK();
  return CE_OK;
}

static int launch_compact_scan(int64_t num_rows, const CompactWs& ws, hipStream_t s) {
  const dim3 g((unsigned)cdiv(num_rows, CE_COMPACT_BLOCK)), b(256);
  hipLaunchKernelGGL(k_compact_count, g, b, 0, s, ws.flags, (uint32_t)num_rows, ws.blk_count);
  hipLaunchKernelGGL(k_compact_emit, g, b, 0, s, ws.flags, (uint32_t)num_rows, ws.blk_count, ws.cidx, ws.list,
                     (uint32_t)ws.cap, ws.n_list);
  CE_LAUNCH_CHECK();
  return CE_OK;
}

static int launch_compact_apply(const UpdateCall& c, const RowGeom& r, const CompactWs& ws, hipStream_t s) {
  CompactArgs a{};
  a.u = update_args(c, r, c.in_row() ? c.step : ws.counter);
  a.acc = ws.acc;
  a.list = ws.list;
  a.n_list = ws.n_list;
  a.adagrad = c.adagrad();
  a.clip = RowClip{c.clip, c.clip_mode};
  const dim3 g(grid_for(ws.cap, 256 >> r.g_log2)), b(256);
  for_decay(c.decay(), c.clipped(), [&](auto d) {
    constexpr bool WD = decltype(d)::WD, CL = decltype(d)::CLIP;
    if (c.elem())
      for_vec_lanes(r.nch, [&](auto l) {
        hipLaunchKernelGGL((k_compact_apply<f32x4, float, decltype(l)::NCH, false, false, WD, false, CL, true>), g, b, 0,
                           s, a);
      });
    else if (c.rowv())
      for_vec_lanes(r.nch, [&](auto l) {
        hipLaunchKernelGGL((k_compact_apply<f32x4, float, decltype(l)::NCH, false, true, WD, true, CL>), g, b, 0, s, a);
      });
    else if (c.adam())
      for_vec_lanes(r.nch, [&](auto l) {
        hipLaunchKernelGGL((k_compact_apply<f32x4, float, decltype(l)::NCH, false, true, WD, false, CL>), g, b, 0, s, a);
      });
    else for_table(c.weight_dtype, r, [&](auto l, auto w) {
      using VT = typename decltype(l)::VT;
      using WT = typename decltype(w)::AT;
      constexpr int N = decltype(l)::NCH;
      if constexpr (std::is_same<WT, float>::value)
        hipLaunchKernelGGL((k_compact_apply<VT, float, N, false, false, WD, false, CL>), g, b, 0, s, a);
      else if (c.stochastic())
        hipLaunchKernelGGL((k_compact_apply<VT, WT, N, true, false, WD, false, CL>), g, b, 0, s, a);
      else
        hipLaunchKernelGGL((k_compact_apply<VT, WT, N, false, false, WD, false, CL>), g, b, 0, s, a);
    });
  });
  CE_LAUNCH_CHECK();
  return CE_OK;
}

// what the step-sized entries do not take
static const char* compact_not_taken(const UpdateCall& c) {
  if (!c.w16() && !c.adagrad())
    return "CE_OPT_SGD on an fp32 table folds straight into the rows: it has no accumulator to compact";
  if (c.w16() && c.adagrad() && c.stochastic())
    return "row-wise Adagrad with CE_ROUND_STOCHASTIC on a 16-bit table is not taken with the step-sized accumulator";
  return nullptr;
}

// the fp32 table's cache-sized update is row-wise Adagrad only (the by-value entries have no optimizer argument)
static EntryRules fp32_rules(const UpdateCall& c) {
  return {false,
          c.adagrad() ? nullptr
                      : "CE_OPT_SGD on an fp32 table folds straight into the rows: it has no accumulator "
                        "(ce_bag_backward_sgd_lrdev / _sgd_src_lrdev)",
          false, [](int64_t R, int64_t, int32_t D) { return carve_apply(nullptr, R, D, false).bytes; }};
}
static const EntryRules kW16Rules{
    true, nullptr, false, [](int64_t R, int64_t, int32_t D) { return carve_apply(nullptr, R, D, true).bytes; }};
static EntryRules compact_rules(const UpdateCall& c) {
  return {false, compact_not_taken(c), true,
          [](int64_t R, int64_t n, int32_t D) { return carve_compact(nullptr, R, n, D).bytes; }};
}

// the dense backward of the call's lookups into acc[rows, dim], reading `idx` / `keys` in place of the caller's
static int scatter_slots(float* acc, int64_t rows, const UpdateCall& c, const SlotLookups& L, const int64_t* idx,
                         const uint64_t* keys, ce_stream_t stream) {
  return ce_bag_backward_dense_act(acc, rows, c.dim, idx, c.nnz, L.offsets, L.off64, L.num_bags, L.include_last, L.psw,
                                   L.mode, L.hookF, c.grad_out, c.act, keys, stream);
}

// ---- The entries' bodies.  A by-value entry and the ce_*_lrdev entry that covers it are ONE function each: c.lr_dev is
// NULL (the learning rate is c.lr) or the device pointer (c.lr is 0 and passes the host's range check; the kernels of
// the apply pass read *c.lr_dev).  Checks, their order and the launch sequence are written once.

// fp32 table, row-wise Adagrad, cache-sized accumulator.  nnz == 0 returns before the arguments are looked at.
static int adagrad_fp32_slots(const UpdateCall& c, const SlotLookups& L, ce_stream_t stream) {
  CE_REQUIRE_ACT(c.act);
  if (L.num_bags == 0 || c.nnz == 0) return CE_OK;
  RowGeom r;
  int rc = update_check(c, fp32_rules(c), r);
  if (rc) return rc;
  CE_REQUIRE(L.indices && L.offsets, CE_ERR_INVALID, "null pointer");
  return update_cache_sized(c, r, &L, nullptr, c.nnz, (hipStream_t)stream, [&](float* acc) {
    return scatter_slots(acc, c.num_rows, c, L, L.indices, L.presorted, stream);
  });
}

static int adagrad_fp32_src(const UpdateCall& c, const uint64_t* src_keys, ce_stream_t stream) {
  CE_REQUIRE_ACT(c.act);
  if (c.nnz == 0) return CE_OK;
  RowGeom r;
  int rc = update_check(c, fp32_rules(c), r);
  if (rc) return rc;
  CE_REQUIRE(src_keys, CE_ERR_INVALID, "null pointer");
  return update_cache_sized(c, r, nullptr, src_keys, ce_bag_presort_len(c.nnz), (hipStream_t)stream, [&](float* acc) {
    return ce_bag_backward_dense_src_act(acc, c.num_rows, c.dim, c.nnz, c.grad_out, c.act, src_keys, stream);
  });
}

// 16-bit table, either optimizer, cache-sized accumulator.  Here and below nnz == 0 returns AFTER the check.
static int update_w16_slots(const UpdateCall& c, const SlotLookups& L, ce_stream_t stream) {
  RowGeom r;
  int rc = update_check(c, kW16Rules, r);
  if (rc) return rc;
  if (L.num_bags == 0 || c.nnz == 0) return CE_OK;
  CE_REQUIRE(L.indices && L.offsets, CE_ERR_INVALID, "null pointer");
  CE_REQUIRE(L.num_bags > 0 && c.nnz > 0 && L.num_bags < (int64_t)INT32_MAX - 64 && c.nnz < (int64_t)INT32_MAX,
             CE_ERR_INVALID, "sizes out of range");
  CE_REQUIRE(L.mode == CE_MODE_SUM || (L.mode == CE_MODE_MEAN && !L.psw), CE_ERR_INVALID,
             "mode must be sum, or mean without per_sample_weights");
  CE_REQUIRE(L.hookF >= 0 && (L.hookF == 0 || L.num_bags % L.hookF == 0), CE_ERR_INVALID,
             "hook_features must divide num_bags");
  return update_cache_sized(c, r, &L, nullptr, c.nnz, (hipStream_t)stream, [&](float* acc) {
    return scatter_slots(acc, c.num_rows, c, L, L.indices, L.presorted, stream);
  });
}

static int update_w16_src(const UpdateCall& c, const uint64_t* src_keys, ce_stream_t stream) {
  RowGeom r;
  int rc = update_check(c, kW16Rules, r);
  if (rc) return rc;
  if (c.nnz == 0) return CE_OK;
  CE_REQUIRE(src_keys && c.nnz > 0 && c.nnz < (int64_t)INT32_MAX, CE_ERR_INVALID, "null keys or nnz out of range");
  return update_cache_sized(c, r, nullptr, src_keys, ce_bag_presort_len(c.nnz), (hipStream_t)stream, [&](float* acc) {
    return ce_bag_backward_dense_src_act(acc, c.num_rows, c.dim, c.nnz, c.grad_out, c.act, src_keys, stream);
  });
}

// step-sized accumulator: mark, compact, remap, the dense backward into acc[cap, D], apply over the list
static int compact_slots_run(const UpdateCall& c, const RowGeom& r, const SlotLookups& L, ce_stream_t stream) {
  int rc;
  if (L.num_bags == 0 || c.nnz == 0) return CE_OK;
  CE_REQUIRE(L.indices && L.offsets, CE_ERR_INVALID, "null pointer");
  CE_REQUIRE(L.num_bags > 0 && L.num_bags < (int64_t)INT32_MAX - 64, CE_ERR_INVALID, "sizes out of range");
  CE_REQUIRE(L.mode == CE_MODE_SUM || (L.mode == CE_MODE_MEAN && !L.psw), CE_ERR_INVALID,
             "mode must be sum, or mean without per_sample_weights");
  CE_REQUIRE(L.hookF >= 0 && (L.hookF == 0 || L.num_bags % L.hookF == 0), CE_ERR_INVALID,
             "hook_features must divide num_bags");
  hipStream_t s = (hipStream_t)stream;
  const CompactWs ws = carve_compact(c.workspace, c.num_rows, c.nnz, c.dim);
  launch_mark_call(c, &L, nullptr, c.nnz, ws.flags, c.in_row() ? c.step : (c.w16() ? ws.counter : nullptr), s);
  rc = launch_compact_scan(c.num_rows, ws, s);
  if (rc) return rc;
  // segment-sorted keys hold the rows themselves: with them the scatter never reads `indices`, so only they are remapped
  const int64_t* idx = L.indices;
  const uint64_t* keys = nullptr;
  if (L.presorted) {
    const int64_t total = ce_bag_presort_len(c.nnz);
    hipLaunchKernelGGL(k_compact_remap_keys, dim3(grid_for(total, 256)), dim3(256), 0, s,
                       (const unsigned long long*)L.presorted, total, (uint32_t)c.num_rows, ws.cidx, (uint32_t)ws.cap, 1,
                       (unsigned long long*)ws.remap);
    keys = (const uint64_t*)ws.remap;
  } else {
    hipLaunchKernelGGL(k_compact_remap_slots, dim3(grid_for(c.nnz, 256)), dim3(256), 0, s, L.indices, c.nnz,
                       (uint32_t)c.num_rows, ws.cidx, (uint32_t)ws.cap, (int64_t*)ws.remap);
    idx = (const int64_t*)ws.remap;
  }
  CE_LAUNCH_CHECK();
  rc = scatter_slots(ws.acc, ws.cap, c, L, idx, keys, stream);
  if (rc) return rc;
  return launch_compact_apply(c, r, ws, s);
}

static int update_compact_slots(const UpdateCall& c, const SlotLookups& L, ce_stream_t stream) {
  RowGeom r;
  int rc = update_check(c, compact_rules(c), r);
  if (rc) return rc;
  return compact_slots_run(c, r, L, stream);
}

static int compact_src_run(const UpdateCall& c, const RowGeom& r, const uint64_t* src_keys, ce_stream_t stream) {
  int rc;
  if (c.nnz == 0) return CE_OK;
  CE_REQUIRE(src_keys, CE_ERR_INVALID, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  const CompactWs ws = carve_compact(c.workspace, c.num_rows, c.nnz, c.dim);
  const int64_t total = ce_bag_presort_len(c.nnz);
  launch_mark_call(c, nullptr, src_keys, total, ws.flags, c.in_row() ? c.step : (c.w16() ? ws.counter : nullptr), s);
  rc = launch_compact_scan(c.num_rows, ws, s);
  if (rc) return rc;
  hipLaunchKernelGGL(k_compact_remap_keys, dim3(grid_for(total, 256)), dim3(256), 0, s,
                     (const unsigned long long*)src_keys, total, (uint32_t)c.num_rows, ws.cidx, (uint32_t)ws.cap, 0,
                     (unsigned long long*)ws.remap);
  CE_LAUNCH_CHECK();
  rc = ce_bag_backward_dense_src_act(ws.acc, ws.cap, c.dim, c.nnz, c.grad_out, c.act, (const uint64_t*)ws.remap, stream);
  if (rc) return rc;
  return launch_compact_apply(c, r, ws, s);
}

static int update_compact_src(const UpdateCall& c, const uint64_t* src_keys, ce_stream_t stream) {
  RowGeom r;
  int rc = update_check(c, compact_rules(c), r);
  if (rc) return rc;
  return compact_src_run(c, r, src_keys, stream);
}

// ---- Adam (ce_bag_backward_adam / _adam_src): an fp32 table whose rows are w | m | v.  Either
// accumulator's pipeline as it stands -- the accumulators are [., dim] as for any fp32 table -- with the mark pass
// counting the caller's step and update_row's Adam arithmetic in the apply pass.

static size_t adam_workspace(int64_t num_rows, int64_t nnz, int32_t dim, int32_t accumulator) {
  return accumulator == CE_ACC_STEP ? carve_compact(nullptr, num_rows, nnz, dim).bytes
                                    : carve_apply(nullptr, num_rows, dim, false).bytes;
}

// Everything an Adam entry refuses, from the arguments alone, before its first launch and before any HIP call; the
// order is the header's.  r: the lane shape of the apply pass (vector lanes: the dim rule and the alignment see to it).
static int adam_check(const UpdateCall& c, int32_t accumulator, RowGeom& r) {
  CE_REQUIRE(c.step, CE_ERR_INVALID, "step: null device pointer");
  CE_REQUIRE(accumulator == CE_ACC_CACHE || accumulator == CE_ACC_STEP, CE_ERR_INVALID,
             "unknown accumulator %d (CE_ACC_CACHE / CE_ACC_STEP)", (int)accumulator);
  int rc = wd_check(c.wd, c.wd_mode);       // (the ce_*_adam_wd entries: the entries without decay pass 0 / CE_WD_NONE)
  if (rc) return rc;
  rc = clip_check(c.clip, c.clip_mode);     // (the ce_*_clip entries: the others pass 0 / CE_CLIP_NONE)
  if (rc) return rc;
  CE_REQUIRE(c.beta1 >= 0.0 && c.beta1 < 1.0 && c.beta2 >= 0.0 && c.beta2 < 1.0, CE_ERR_INVALID,
             "beta1 and beta2 must lie in [0, 1)");
  CE_REQUIRE(c.lr_decay >= 0.0, CE_ERR_INVALID, "lr_decay must be >= 0");       // (a NaN fails it; Adam passes 0)
  CE_REQUIRE(c.eps >= 0.f, CE_ERR_INVALID, "eps must be >= 0");
  CE_REQUIRE(c.lr_dev || c.lr >= 0.f, CE_ERR_INVALID, "lr must be >= 0");
  CE_REQUIRE_ACT(c.act);
  CE_REQUIRE_ADAM_DIM(c.dim);
  CE_REQUIRE(c.weight && c.grad_out && c.workspace, CE_ERR_INVALID, "null pointer");
  CE_REQUIRE(!c.rowv() || (c.momentum && c.momentum_rows > 0), CE_ERR_INVALID,
             "partial row-wise Adam needs its second moment: v, v_rows > 0");
  CE_REQUIRE(c.num_rows > 0 && c.num_rows < (int64_t)INT32_MAX, CE_ERR_INVALID, "num_rows out of range");
  CE_REQUIRE(c.nnz >= 0 && c.nnz < (int64_t)INT32_MAX, CE_ERR_INVALID, "nnz out of range");
  CE_REQUIRE(al16(c.weight) && (((uintptr_t)c.step) & 7) == 0, CE_ERR_INVALID,
             "an Adam-layout table must be 16-byte aligned (and step 8-byte aligned)");
  CE_REQUIRE((((uintptr_t)c.workspace) & 255) == 0, CE_ERR_INVALID, "workspace must be 256-byte aligned");
  CE_REQUIRE(c.workspace_bytes >= adam_workspace(c.num_rows, c.nnz, c.dim, accumulator), CE_ERR_INVALID,
             "workspace too small");
  return row_geometry(c.dim, true, r);
}

// the second moment of a partial row-wise Adam call (ce_bag_backward_pradam*): v[v_rows], indexed by table row
struct RowMoment {
  const int32_t* row_of_slot;
  float* v;
  int64_t v_rows;
};

// rv: NULL for the Adam layout (rows w | m | v), the row-wise second moment of a partial row-wise Adam call (rows w | m)
static UpdateCall adam_call(float* weight, int64_t num_rows, int32_t dim, int64_t nnz, const void* grad_out, int32_t act,
                            double beta1, double beta2, float lr, const float* lr_dev, float eps, int64_t* step,
                            void* workspace, size_t workspace_bytes, float wd = 0.f, int32_t wd_mode = CE_WD_NONE,
                            const RowMoment* rv = nullptr, RowClip clip = RowClip{}) {
  UpdateCall c{weight, CE_ACT_F32, num_rows, dim, nnz, grad_out, act, rv ? rv->row_of_slot : nullptr,
               rv ? rv->v : nullptr, rv ? rv->v_rows : 0, lr_dev ? 0.f : lr, eps,
               rv ? kOptPartialAdam : kOptAdam, CE_ROUND_NEAREST, 0, workspace, workspace_bytes, lr_dev};
  c.step = (unsigned long long*)step;
  c.beta1 = beta1;
  c.beta2 = beta2;
  c.wd = wd;
  c.wd_mode = wd_mode;
  c.clip = clip.c;
  c.clip_mode = clip.mode;
  return c;
}

// Which covered entry a ce_*_lrdev call is, from its accumulator and its table; `run` gets the call as that entry
// takes it.  lr == NULL and an unknown accumulator are refused first: before anything the covered entry looks at.
template <typename Fp32, typename W16, typename Compact>
static int lrdev_dispatch(UpdateCall c, int32_t accumulator, Fp32&& fp32, W16&& w16, Compact&& compact) {
  CE_REQUIRE(c.lr_dev, CE_ERR_INVALID, "lr: null device pointer");
  CE_REQUIRE(accumulator == CE_ACC_CACHE || accumulator == CE_ACC_STEP, CE_ERR_INVALID,
             "unknown accumulator %d (CE_ACC_CACHE / CE_ACC_STEP)", (int)accumulator);
  if (accumulator == CE_ACC_STEP) return compact(c);
  if (c.weight_dtype != CE_ACT_F32) return w16(c);
  c.rounding = CE_ROUND_NEAREST;      // an fp32 row is stored as it is: the covered entry has neither argument
  c.seed = 0;
  return fp32(c);
}

// a ce_*_wd / ce_*_clip update call: the accumulator code, the two decay checks, the two clip checks (a _wd call
// carries 0 / CE_CLIP_NONE), then the covered entry as lrdev_dispatch picks it (lr_dev == NULL: the learning rate by value)
template <typename Fp32, typename W16, typename Compact>
static int wd_dispatch(UpdateCall c, int32_t accumulator, Fp32&& fp32, W16&& w16, Compact&& compact) {
  CE_REQUIRE(accumulator == CE_ACC_CACHE || accumulator == CE_ACC_STEP, CE_ERR_INVALID,
             "unknown accumulator %d (CE_ACC_CACHE / CE_ACC_STEP)", (int)accumulator);
  int rc = wd_check(c.wd, c.wd_mode);
  if (rc) return rc;
  rc = clip_check(c.clip, c.clip_mode);
  if (rc) return rc;
  if (accumulator == CE_ACC_STEP) return compact(c);
  if (c.weight_dtype != CE_ACT_F32) return w16(c);
  c.rounding = CE_ROUND_NEAREST;
  c.seed = 0;
  return fp32(c);
}

}  // namespace ce

using namespace ce;

// ---- fp32 table, row-wise Adagrad, cache-sized accumulator

extern "C" size_t ce_bag_backward_rowwise_adagrad_workspace(int64_t num_rows, int32_t dim) {
  if (num_rows < 0 || dim < 0) return 0;
  return carve_apply(nullptr, num_rows, dim, false).bytes;
}

// grad_out of the activation type act_dtype: the scatter reads it natively, acc and everything after it are fp32
extern "C" int ce_bag_backward_rowwise_adagrad_act(float* weight, int64_t num_rows, int32_t dim, const int64_t* indices,
                                                   int64_t nnz, const void* offsets, int32_t offsets_are_i64,
                                                   int64_t num_bags, int32_t include_last_offset,
                                                   const float* per_sample_weights, int32_t mode,
                                                   int64_t hook_features, const void* grad_out, int32_t act_dtype,
                                                   const uint64_t* presorted, const int32_t* row_of_slot,
                                                   float* momentum, int64_t momentum_rows, float lr, float eps,
                                                   void* workspace, size_t workspace_bytes, ce_stream_t stream) {
  const UpdateCall c{weight, CE_ACT_F32, num_rows, dim, nnz, grad_out, act_dtype, row_of_slot, momentum, momentum_rows,
                     lr, eps, CE_OPT_ROWWISE_ADAGRAD, CE_ROUND_NEAREST, 0, workspace, workspace_bytes};
  return adagrad_fp32_slots(c, {indices, offsets, offsets_are_i64, num_bags, include_last_offset, per_sample_weights,
                                mode, hook_features, presorted}, stream);
}

extern "C" int ce_bag_backward_rowwise_adagrad(float* weight, int64_t num_rows, int32_t dim, const int64_t* indices,
                                               int64_t nnz, const void* offsets, int32_t offsets_are_i64,
                                               int64_t num_bags, int32_t include_last_offset,
                                               const float* per_sample_weights, int32_t mode, int64_t hook_features,
                                               const float* grad_out, const uint64_t* presorted,
                                               const int32_t* row_of_slot, float* momentum, int64_t momentum_rows,
                                               float lr, float eps, void* workspace, size_t workspace_bytes,
                                               ce_stream_t stream) {
  return ce_bag_backward_rowwise_adagrad_act(weight, num_rows, dim, indices, nnz, offsets, offsets_are_i64, num_bags,
                                             include_last_offset, per_sample_weights, mode, hook_features, grad_out,
                                             CE_ACT_F32, presorted, row_of_slot, momentum, momentum_rows, lr, eps,
                                             workspace, workspace_bytes, stream);
}

extern "C" int ce_bag_backward_rowwise_adagrad_src_act(float* weight, int64_t num_rows, int32_t dim, int64_t nnz,
                                                       const void* grad_out, int32_t act_dtype,
                                                       const uint64_t* src_keys, const int32_t* row_of_slot,
                                                       float* momentum, int64_t momentum_rows, float lr, float eps,
                                                       void* workspace, size_t workspace_bytes, ce_stream_t stream) {
  const UpdateCall c{weight, CE_ACT_F32, num_rows, dim, nnz, grad_out, act_dtype, row_of_slot, momentum, momentum_rows,
                     lr, eps, CE_OPT_ROWWISE_ADAGRAD, CE_ROUND_NEAREST, 0, workspace, workspace_bytes};
  return adagrad_fp32_src(c, src_keys, stream);
}

extern "C" int ce_bag_backward_rowwise_adagrad_src(float* weight, int64_t num_rows, int32_t dim, int64_t nnz,
                                                   const float* grad_out, const uint64_t* src_keys,
                                                   const int32_t* row_of_slot, float* momentum,
                                                   int64_t momentum_rows, float lr, float eps, void* workspace,
                                                   size_t workspace_bytes, ce_stream_t stream) {
  return ce_bag_backward_rowwise_adagrad_src_act(weight, num_rows, dim, nnz, grad_out, CE_ACT_F32, src_keys,
                                                 row_of_slot, momentum, momentum_rows, lr, eps, workspace,
                                                 workspace_bytes, stream);
}

// ---- 16-bit table, either optimizer, cache-sized accumulator

extern "C" size_t ce_bag_backward_w16_workspace(int64_t num_rows, int32_t dim) {
  if (num_rows < 0 || dim < 0) return 0;
  return carve_apply(nullptr, num_rows, dim, true).bytes;
}

extern "C" int ce_bag_backward_update_w16(void* weight, int32_t weight_dtype, int64_t num_rows, int32_t dim,
                                          const int64_t* indices, int64_t nnz, const void* offsets,
                                          int32_t offsets_are_i64, int64_t num_bags, int32_t include_last_offset,
                                          const float* per_sample_weights, int32_t mode, int64_t hook_features,
                                          const void* grad_out, int32_t act_dtype, const uint64_t* presorted,
                                          const int32_t* row_of_slot, float* momentum, int64_t momentum_rows, float lr,
                                          float eps, int32_t optimizer, int32_t rounding, uint64_t seed,
                                          void* workspace, size_t workspace_bytes, ce_stream_t stream) {
  const UpdateCall c{weight, weight_dtype, num_rows, dim, nnz, grad_out, act_dtype, row_of_slot, momentum,
                     momentum_rows, lr, eps, optimizer, rounding, seed, workspace, workspace_bytes};
  return update_w16_slots(c, {indices, offsets, offsets_are_i64, num_bags, include_last_offset, per_sample_weights, mode,
                              hook_features, presorted}, stream);
}

extern "C" int ce_bag_backward_update_src_w16(void* weight, int32_t weight_dtype, int64_t num_rows, int32_t dim,
                                              int64_t nnz, const void* grad_out, int32_t act_dtype,
                                              const uint64_t* src_keys, const int32_t* row_of_slot, float* momentum,
                                              int64_t momentum_rows, float lr, float eps, int32_t optimizer,
                                              int32_t rounding, uint64_t seed, void* workspace,
                                              size_t workspace_bytes, ce_stream_t stream) {
  const UpdateCall c{weight, weight_dtype, num_rows, dim, nnz, grad_out, act_dtype, row_of_slot, momentum,
                     momentum_rows, lr, eps, optimizer, rounding, seed, workspace, workspace_bytes};
  return update_w16_src(c, src_keys, stream);
}

// ---- step-sized accumulator

extern "C" size_t ce_bag_backward_update_compact_workspace(int64_t num_rows, int64_t nnz, int32_t dim) {
  if (num_rows < 0 || num_rows >= (int64_t)INT32_MAX || nnz < 0 || nnz >= (int64_t)INT32_MAX || dim < 0) return 0;
  return carve_compact(nullptr, num_rows, nnz, dim).bytes;
}

extern "C" int ce_bag_backward_update_compact(void* weight, int32_t weight_dtype, int64_t num_rows, int32_t dim,
                                              const int64_t* indices, int64_t nnz, const void* offsets,
                                              int32_t offsets_are_i64, int64_t num_bags, int32_t include_last_offset,
                                              const float* per_sample_weights, int32_t mode, int64_t hook_features,
                                              const void* grad_out, int32_t act_dtype, const uint64_t* presorted,
                                              const int32_t* row_of_slot, float* momentum, int64_t momentum_rows,
                                              float lr, float eps, int32_t optimizer, int32_t rounding, uint64_t seed,
                                              void* workspace, size_t workspace_bytes, ce_stream_t stream) {
  const UpdateCall c{weight, weight_dtype, num_rows, dim, nnz, grad_out, act_dtype, row_of_slot, momentum,
                     momentum_rows, lr, eps, optimizer, rounding, seed, workspace, workspace_bytes};
  return update_compact_slots(c, {indices, offsets, offsets_are_i64, num_bags, include_last_offset, per_sample_weights,
                                  mode, hook_features, presorted}, stream);
}

extern "C" int ce_bag_backward_update_compact_src(void* weight, int32_t weight_dtype, int64_t num_rows, int32_t dim,
                                                  int64_t nnz, const void* grad_out, int32_t act_dtype,
                                                  const uint64_t* src_keys, const int32_t* row_of_slot,
                                                  float* momentum, int64_t momentum_rows, float lr, float eps,
                                                  int32_t optimizer, int32_t rounding, uint64_t seed, void* workspace,
                                                  size_t workspace_bytes, ce_stream_t stream) {
  const UpdateCall c{weight, weight_dtype, num_rows, dim, nnz, grad_out, act_dtype, row_of_slot, momentum,
                     momentum_rows, lr, eps, optimizer, rounding, seed, workspace, workspace_bytes};
  return update_compact_src(c, src_keys, stream);
}

// ---- the learning rate in device memory: the three pairs above behind one pair of entries

extern "C" int ce_bag_backward_update_lrdev(void* weight, int32_t weight_dtype, int64_t num_rows, int32_t dim,
                                            const int64_t* indices, int64_t nnz, const void* offsets,
                                            int32_t offsets_are_i64, int64_t num_bags, int32_t include_last_offset,
                                            const float* per_sample_weights, int32_t mode, int64_t hook_features,
                                            const void* grad_out, int32_t act_dtype, const uint64_t* presorted,
                                            const int32_t* row_of_slot, float* momentum, int64_t momentum_rows,
                                            const float* lr, float eps, int32_t optimizer, int32_t rounding,
                                            uint64_t seed, int32_t accumulator, void* workspace, size_t workspace_bytes,
                                            ce_stream_t stream) {
  const UpdateCall c{weight, weight_dtype, num_rows, dim, nnz, grad_out, act_dtype, row_of_slot, momentum,
                     momentum_rows, 0.f, eps, optimizer, rounding, seed, workspace, workspace_bytes, lr};
  const SlotLookups L{indices, offsets, offsets_are_i64, num_bags, include_last_offset, per_sample_weights, mode,
                      hook_features, presorted};
  return lrdev_dispatch(c, accumulator, [&](const UpdateCall& u) { return adagrad_fp32_slots(u, L, stream); },
                        [&](const UpdateCall& u) { return update_w16_slots(u, L, stream); },
                        [&](const UpdateCall& u) { return update_compact_slots(u, L, stream); });
}

extern "C" int ce_bag_backward_update_src_lrdev(void* weight, int32_t weight_dtype, int64_t num_rows, int32_t dim,
                                                int64_t nnz, const void* grad_out, int32_t act_dtype,
                                                const uint64_t* src_keys, const int32_t* row_of_slot, float* momentum,
                                                int64_t momentum_rows, const float* lr, float eps, int32_t optimizer,
                                                int32_t rounding, uint64_t seed, int32_t accumulator, void* workspace,
                                                size_t workspace_bytes, ce_stream_t stream) {
  const UpdateCall c{weight, weight_dtype, num_rows, dim, nnz, grad_out, act_dtype, row_of_slot, momentum,
                     momentum_rows, 0.f, eps, optimizer, rounding, seed, workspace, workspace_bytes, lr};
  return lrdev_dispatch(c, accumulator, [&](const UpdateCall& u) { return adagrad_fp32_src(u, src_keys, stream); },
                        [&](const UpdateCall& u) { return update_w16_src(u, src_keys, stream); },
                        [&](const UpdateCall& u) { return update_compact_src(u, src_keys, stream); });
}

// ---- deterministic, accumulator-free: sort, fold + apply, combine + apply

extern "C" size_t ce_bag_backward_update_sorted_workspace(int64_t num_rows, int64_t nnz, int32_t dim) {
  (void)num_rows;
  if (nnz < 0 || nnz >= (int64_t)INT32_MAX || dim <= 0) return 0;
  return carve_sorted(nullptr, nnz, dim).bytes;
}

// ce_bag_backward_update_sorted (weight_decay 0, CE_WD_NONE), ce_bag_backward_update_sorted_wd (grad_clip 0, CE_CLIP_NONE)
// and ce_bag_backward_update_sorted_clip are this one function
static int update_sorted(void* weight, int32_t weight_dtype, int64_t num_rows, int32_t dim, const int64_t* indices,
                         int64_t nnz, const void* offsets, int32_t offsets_are_i64, int64_t num_bags,
                         int32_t include_last_offset, const float* per_sample_weights, int32_t mode,
                         int64_t hook_features, const void* grad_out, int32_t act_dtype, const int32_t* row_of_slot,
                         float* momentum, int64_t momentum_rows, float lr, float eps, float weight_decay,
                         int32_t weight_decay_mode, float grad_clip, int32_t grad_clip_mode, int32_t optimizer,
                         int32_t rounding, uint64_t seed, void* workspace, size_t workspace_bytes, ce_stream_t stream) {
  // everything that can be refused, from the arguments alone: no launch, no HIP call before the last check
  {
    int rc = wd_check(weight_decay, weight_decay_mode);
    if (rc) return rc;
    rc = clip_check(grad_clip, grad_clip_mode);
    if (rc) return rc;
  }
  const bool decay = weight_decay_mode != CE_WD_NONE && weight_decay != 0.f;
  const bool clipped = grad_clip_mode != CE_CLIP_NONE;
  CE_REQUIRE_ACT(act_dtype);
  CE_REQUIRE(weight_dtype == CE_ACT_F32 || weight_dtype == CE_ACT_BF16 || weight_dtype == CE_ACT_F16, CE_ERR_INVALID,
             "unknown weight_dtype %d (CE_ACT_F32 / CE_ACT_BF16 / CE_ACT_F16)", (int)weight_dtype);
  const bool w16 = weight_dtype != CE_ACT_F32;
  if (w16) {
    int rc = w16_check(weight_dtype, dim);
    if (rc) return rc;
  }
  CE_REQUIRE(optimizer == CE_OPT_SGD || optimizer == CE_OPT_ROWWISE_ADAGRAD, CE_ERR_INVALID,
             "unknown optimizer %d (CE_OPT_SGD / CE_OPT_ROWWISE_ADAGRAD)", (int)optimizer);
  CE_REQUIRE(rounding == CE_ROUND_NEAREST || rounding == CE_ROUND_STOCHASTIC, CE_ERR_INVALID,
             "unknown rounding %d (CE_ROUND_NEAREST / CE_ROUND_STOCHASTIC)", (int)rounding);
  (void)seed;     // part of the update entries' common tail; only stochastic rounding would read it
  CE_REQUIRE(!w16 || rounding == CE_ROUND_NEAREST, CE_ERR_UNSUPPORTED,
             "CE_ROUND_STOCHASTIC on a 16-bit table: the sorted update rounds to nearest only");
  CE_REQUIRE(weight && grad_out && workspace, CE_ERR_INVALID, "null pointer");
  CE_REQUIRE(dim > 0, CE_ERR_INVALID, "dim must be positive");
  CE_REQUIRE(num_rows > 0 && num_rows < (int64_t)INT32_MAX && nnz >= 0 && nnz < (int64_t)INT32_MAX && num_bags >= 0 &&
                 num_bags < (int64_t)INT32_MAX,
             CE_ERR_UNSUPPORTED, "sizes beyond 2^31");
  CE_REQUIRE(lr >= 0.f, CE_ERR_INVALID, "lr must be >= 0");
  if (optimizer == CE_OPT_ROWWISE_ADAGRAD) {
    CE_REQUIRE(momentum && momentum_rows > 0, CE_ERR_INVALID, "row-wise Adagrad needs its momentum");
    CE_REQUIRE(eps > 0.f, CE_ERR_INVALID, "eps must be > 0");
  }
  CE_REQUIRE(mode == CE_MODE_SUM || mode == CE_MODE_MEAN, CE_ERR_UNSUPPORTED, "mode must be sum or mean");
  CE_REQUIRE(hook_features >= 0 && hook_features < (int64_t)INT32_MAX &&
                 (hook_features == 0 || num_bags % hook_features == 0),
             CE_ERR_INVALID, "hook_features must divide num_bags");
  CE_REQUIRE((((uintptr_t)workspace) & 255) == 0, CE_ERR_INVALID, "workspace must be 256-byte aligned");
  CE_REQUIRE(workspace_bytes >= ce_bag_backward_update_sorted_workspace(num_rows, nnz, dim), CE_ERR_INVALID,
             "workspace too small");
  const bool aligned = al16(weight) && act_aligned(grad_out, act_dtype);
  CE_REQUIRE(!w16 || aligned, CE_ERR_INVALID,
             "a 16-bit table must be 16-byte aligned and its gradient on the vector boundary");
  RowGeom r;
  int rc = row_geometry(dim, aligned, r);
  if (rc) return rc;
  if (num_bags == 0 || nnz == 0) return CE_OK;
  CE_REQUIRE(indices && offsets, CE_ERR_INVALID, "null pointer");

  hipStream_t s = (hipStream_t)stream;
  const SortedWs ws = carve_sorted(workspace, nnz, dim);
  SortedRows sr{};
  // with decay a row that merely heads a run changes: the lookups no bag covers must head none
  rc = sorted_rows(indices, nnz, num_rows, offsets, offsets_are_i64, num_bags, include_last_offset, ws.sort,
                   s, sr, decay);
  if (rc) return rc;
  SortedArgs a{};
  a.weight = weight;
  a.grad_out = grad_out;
  a.partials = ws.partials;
  a.rows_sorted = sr.rows;
  a.lookup_sorted = sr.lookups;
  a.bag_of = sr.bag_of;
  a.offsets = offsets;
  a.psw = per_sample_weights;
  a.row_of_slot = row_of_slot;
  a.momentum = momentum;
  a.momentum_rows = momentum_rows;
  a.nnz = nnz;
  a.num_bags = num_bags;
  a.num_rows = (int32_t)num_rows;
  a.rowlen = r.rowlen;
  a.g_log2 = r.g_log2;
  a.dim = dim;
  a.off64 = offsets_are_i64;
  a.include_last = include_last_offset;
  a.mode = mode;
  a.hookF = (int)hook_features;
  a.hookB = hook_features ? (int)(num_bags / hook_features) : 0;
  a.adagrad = optimizer == CE_OPT_ROWWISE_ADAGRAD;
  a.lr = lr;
  a.eps = eps;
  // (a clipped launch reads the decay's mode at run time: a call without decay is CE_WD_NONE with wd = 0 there)
  a.wd = decay ? weight_decay : 0.f;
  a.wd_mode = decay ? weight_decay_mode : CE_WD_NONE;
  a.clip = grad_clip;
  a.clip_mode = grad_clip_mode;
  const dim3 g(grid_for(cdiv(nnz, 64), 4)), b(256);
  for_decay(decay, clipped, [&](auto d) {
    constexpr bool WD = decltype(d)::WD, CL = decltype(d)::CLIP;
    if (w16) {
      for_w16(r.nch, weight_dtype, [&](auto l, auto w) {
        using WT = typename decltype(w)::AT;
        constexpr int N = decltype(l)::NCH;
        for_act(act_dtype, [&](auto at) {
          hipLaunchKernelGGL((k_sorted_fold<f32x4, typename decltype(at)::AT, WT, N, WD, CL>), g, b, 0, s, a);
        });
        hipLaunchKernelGGL((k_sorted_combine<f32x4, WT, N, WD, CL>), g, b, 0, s, a);
      });
    } else {
      for_lanes(r.vec, r.nch, [&](auto l) {
        using VT = typename decltype(l)::VT;
        constexpr int N = decltype(l)::NCH;
        for_act(act_dtype, [&](auto at) {
          hipLaunchKernelGGL((k_sorted_fold<VT, typename decltype(at)::AT, float, N, WD, CL>), g, b, 0, s, a);
        });
        hipLaunchKernelGGL((k_sorted_combine<VT, float, N, WD, CL>), g, b, 0, s, a);
      });
    }
  });
  CE_LAUNCH_CHECK();
  return CE_OK;
}

extern "C" int ce_bag_backward_update_sorted(void* weight, int32_t weight_dtype, int64_t num_rows, int32_t dim,
                                             const int64_t* indices, int64_t nnz, const void* offsets,
                                             int32_t offsets_are_i64, int64_t num_bags, int32_t include_last_offset,
                                             const float* per_sample_weights, int32_t mode, int64_t hook_features,
                                             const void* grad_out, int32_t act_dtype, const int32_t* row_of_slot,
                                             float* momentum, int64_t momentum_rows, float lr, float eps,
                                             int32_t optimizer, int32_t rounding, uint64_t seed, void* workspace,
                                             size_t workspace_bytes, ce_stream_t stream) {
  return update_sorted(weight, weight_dtype, num_rows, dim, indices, nnz, offsets, offsets_are_i64, num_bags,
                       include_last_offset, per_sample_weights, mode, hook_features, grad_out, act_dtype, row_of_slot,
                       momentum, momentum_rows, lr, eps, 0.f, CE_WD_NONE, 0.f, CE_CLIP_NONE, optimizer, rounding, seed,
                       workspace, workspace_bytes, stream);
}

extern "C" int ce_bag_backward_update_sorted_wd(void* weight, int32_t weight_dtype, int64_t num_rows, int32_t dim,
                                                const int64_t* indices, int64_t nnz, const void* offsets,
                                                int32_t offsets_are_i64, int64_t num_bags, int32_t include_last_offset,
                                                const float* per_sample_weights, int32_t mode, int64_t hook_features,
                                                const void* grad_out, int32_t act_dtype, const int32_t* row_of_slot,
                                                float* momentum, int64_t momentum_rows, float lr, float eps,
                                                float weight_decay, int32_t weight_decay_mode, int32_t optimizer,
                                                int32_t rounding, uint64_t seed, void* workspace,
                                                size_t workspace_bytes, ce_stream_t stream) {
  return update_sorted(weight, weight_dtype, num_rows, dim, indices, nnz, offsets, offsets_are_i64, num_bags,
                       include_last_offset, per_sample_weights, mode, hook_features, grad_out, act_dtype, row_of_slot,
                       momentum, momentum_rows, lr, eps, weight_decay, weight_decay_mode, 0.f, CE_CLIP_NONE, optimizer,
                       rounding, seed, workspace, workspace_bytes, stream);
}

extern "C" int ce_bag_backward_update_sorted_clip(void* weight, int32_t weight_dtype, int64_t num_rows, int32_t dim,
                                                  const int64_t* indices, int64_t nnz, const void* offsets,
                                                  int32_t offsets_are_i64, int64_t num_bags,
                                                  int32_t include_last_offset, const float* per_sample_weights,
                                                  int32_t mode, int64_t hook_features, const void* grad_out,
                                                  int32_t act_dtype, const int32_t* row_of_slot, float* momentum,
                                                  int64_t momentum_rows, float lr, float eps, float weight_decay,
                                                  int32_t weight_decay_mode, float grad_clip, int32_t grad_clip_mode,
                                                  int32_t optimizer, int32_t rounding, uint64_t seed, void* workspace,
                                                  size_t workspace_bytes, ce_stream_t stream) {
  return update_sorted(weight, weight_dtype, num_rows, dim, indices, nnz, offsets, offsets_are_i64, num_bags,
                       include_last_offset, per_sample_weights, mode, hook_features, grad_out, act_dtype, row_of_slot,
                       momentum, momentum_rows, lr, eps, weight_decay, weight_decay_mode, grad_clip, grad_clip_mode,
                       optimizer, rounding, seed, workspace, workspace_bytes, stream);
}

// ---- weight decay for the atomic updates: the pair of ce_bag_backward_update_lrdev / _src_lrdev with the learning
// rate in Adam's convention (lr_dev == NULL: by value) and the decay behind eps

// ce_bag_backward_update_wd (grad_clip 0, CE_CLIP_NONE) and ce_bag_backward_update_clip are one function; the _src
// pair likewise
extern "C" int ce_bag_backward_update_clip(void* weight, int32_t weight_dtype, int64_t num_rows, int32_t dim,
                                           const int64_t* indices, int64_t nnz, const void* offsets,
                                           int32_t offsets_are_i64, int64_t num_bags, int32_t include_last_offset,
                                           const float* per_sample_weights, int32_t mode, int64_t hook_features,
                                           const void* grad_out, int32_t act_dtype, const uint64_t* presorted,
                                           const int32_t* row_of_slot, float* momentum, int64_t momentum_rows, float lr,
                                           const float* lr_dev, float eps, float weight_decay,
                                           int32_t weight_decay_mode, float grad_clip, int32_t grad_clip_mode,
                                           int32_t optimizer, int32_t rounding, uint64_t seed, int32_t accumulator,
                                           void* workspace, size_t workspace_bytes, ce_stream_t stream) {
  UpdateCall c{weight, weight_dtype, num_rows, dim, nnz, grad_out, act_dtype, row_of_slot, momentum,
               momentum_rows, lr_dev ? 0.f : lr, eps, optimizer, rounding, seed, workspace, workspace_bytes, lr_dev};
  c.wd = weight_decay;
  c.wd_mode = weight_decay_mode;
  c.clip = grad_clip;
  c.clip_mode = grad_clip_mode;
  const SlotLookups L{indices, offsets, offsets_are_i64, num_bags, include_last_offset, per_sample_weights, mode,
                      hook_features, presorted};
  return wd_dispatch(c, accumulator, [&](const UpdateCall& u) { return adagrad_fp32_slots(u, L, stream); },
                     [&](const UpdateCall& u) { return update_w16_slots(u, L, stream); },
                     [&](const UpdateCall& u) { return update_compact_slots(u, L, stream); });
}

extern "C" int ce_bag_backward_update_wd(void* weight, int32_t weight_dtype, int64_t num_rows, int32_t dim,
                                         const int64_t* indices, int64_t nnz, const void* offsets,
                                         int32_t offsets_are_i64, int64_t num_bags, int32_t include_last_offset,
                                         const float* per_sample_weights, int32_t mode, int64_t hook_features,
                                         const void* grad_out, int32_t act_dtype, const uint64_t* presorted,
                                         const int32_t* row_of_slot, float* momentum, int64_t momentum_rows, float lr,
                                         const float* lr_dev, float eps, float weight_decay, int32_t weight_decay_mode,
                                         int32_t optimizer, int32_t rounding, uint64_t seed, int32_t accumulator,
                                         void* workspace, size_t workspace_bytes, ce_stream_t stream) {
  return ce_bag_backward_update_clip(weight, weight_dtype, num_rows, dim, indices, nnz, offsets, offsets_are_i64,
                                     num_bags, include_last_offset, per_sample_weights, mode, hook_features, grad_out,
                                     act_dtype, presorted, row_of_slot, momentum, momentum_rows, lr, lr_dev, eps,
                                     weight_decay, weight_decay_mode, 0.f, CE_CLIP_NONE, optimizer, rounding, seed,
                                     accumulator, workspace, workspace_bytes, stream);
}

extern "C" int ce_bag_backward_update_src_clip(void* weight, int32_t weight_dtype, int64_t num_rows, int32_t dim,
                                               int64_t nnz, const void* grad_out, int32_t act_dtype,
                                               const uint64_t* src_keys, const int32_t* row_of_slot, float* momentum,
                                               int64_t momentum_rows, float lr, const float* lr_dev, float eps,
                                               float weight_decay, int32_t weight_decay_mode, float grad_clip,
                                               int32_t grad_clip_mode, int32_t optimizer, int32_t rounding,
                                               uint64_t seed, int32_t accumulator, void* workspace,
                                               size_t workspace_bytes, ce_stream_t stream) {
  UpdateCall c{weight, weight_dtype, num_rows, dim, nnz, grad_out, act_dtype, row_of_slot, momentum,
               momentum_rows, lr_dev ? 0.f : lr, eps, optimizer, rounding, seed, workspace, workspace_bytes, lr_dev};
  c.wd = weight_decay;
  c.wd_mode = weight_decay_mode;
  c.clip = grad_clip;
  c.clip_mode = grad_clip_mode;
  return wd_dispatch(c, accumulator, [&](const UpdateCall& u) { return adagrad_fp32_src(u, src_keys, stream); },
                     [&](const UpdateCall& u) { return update_w16_src(u, src_keys, stream); },
                     [&](const UpdateCall& u) { return update_compact_src(u, src_keys, stream); });
}

extern "C" int ce_bag_backward_update_src_wd(void* weight, int32_t weight_dtype, int64_t num_rows, int32_t dim,
                                             int64_t nnz, const void* grad_out, int32_t act_dtype,
                                             const uint64_t* src_keys, const int32_t* row_of_slot, float* momentum,
                                             int64_t momentum_rows, float lr, const float* lr_dev, float eps,
                                             float weight_decay, int32_t weight_decay_mode, int32_t optimizer,
                                             int32_t rounding, uint64_t seed, int32_t accumulator, void* workspace,
                                             size_t workspace_bytes, ce_stream_t stream) {
  return ce_bag_backward_update_src_clip(weight, weight_dtype, num_rows, dim, nnz, grad_out, act_dtype, src_keys,
                                         row_of_slot, momentum, momentum_rows, lr, lr_dev, eps, weight_decay,
                                         weight_decay_mode, 0.f, CE_CLIP_NONE, optimizer, rounding, seed, accumulator,
                                         workspace, workspace_bytes, stream);
}

// ---- Adam on an Adam-layout table (rows w | m | v)

extern "C" size_t ce_bag_backward_adam_workspace(int64_t num_rows, int64_t nnz, int32_t dim, int32_t accumulator) {
  if (num_rows < 0 || num_rows >= (int64_t)INT32_MAX || nnz < 0 || nnz >= (int64_t)INT32_MAX || dim < 0) return 0;
  if (accumulator != CE_ACC_CACHE && accumulator != CE_ACC_STEP) return 0;
  return adam_workspace(num_rows, nnz, dim, accumulator);
}

// the body of every entry whose table carries its state in the row (Adam, partial row-wise Adam, element-wise Adagrad):
// the check, then either accumulator's pipeline
static int in_row_slots(const UpdateCall& c, const SlotLookups& L, int32_t accumulator, ce_stream_t stream) {
  RowGeom r;
  int rc = adam_check(c, accumulator, r);
  if (rc) return rc;
  if (accumulator == CE_ACC_STEP) return compact_slots_run(c, r, L, stream);
  if (L.num_bags == 0 || c.nnz == 0) return CE_OK;
  CE_REQUIRE(L.indices && L.offsets, CE_ERR_INVALID, "null pointer");
  CE_REQUIRE(L.num_bags > 0 && L.num_bags < (int64_t)INT32_MAX - 64, CE_ERR_INVALID, "sizes out of range");
  CE_REQUIRE(L.mode == CE_MODE_SUM || (L.mode == CE_MODE_MEAN && !L.psw), CE_ERR_INVALID,
             "mode must be sum, or mean without per_sample_weights");
  CE_REQUIRE(L.hookF >= 0 && (L.hookF == 0 || L.num_bags % L.hookF == 0), CE_ERR_INVALID,
             "hook_features must divide num_bags");
  return update_cache_sized(c, r, &L, nullptr, c.nnz, (hipStream_t)stream, [&](float* acc) {
    return scatter_slots(acc, c.num_rows, c, L, L.indices, L.presorted, stream);
  });
}

static int in_row_src(const UpdateCall& c, const uint64_t* src_keys, int32_t accumulator, ce_stream_t stream) {
  RowGeom r;
  int rc = adam_check(c, accumulator, r);
  if (rc) return rc;
  if (accumulator == CE_ACC_STEP) return compact_src_run(c, r, src_keys, stream);
  if (c.nnz == 0) return CE_OK;
  CE_REQUIRE(src_keys, CE_ERR_INVALID, "null pointer");
  return update_cache_sized(c, r, nullptr, src_keys, ce_bag_presort_len(c.nnz), (hipStream_t)stream, [&](float* acc) {
    return ce_bag_backward_dense_src_act(acc, c.num_rows, c.dim, c.nnz, c.grad_out, c.act, src_keys, stream);
  });
}

// ce_bag_backward_adam (weight_decay 0, CE_WD_NONE) and ce_bag_backward_adam_wd are one function; the _src pair likewise
static int adam_slots(float* weight, int64_t num_rows, int32_t dim, const int64_t* indices, int64_t nnz,
                      const void* offsets, int32_t offsets_are_i64, int64_t num_bags, int32_t include_last_offset,
                      const float* per_sample_weights, int32_t mode, int64_t hook_features, const void* grad_out,
                      int32_t act_dtype, const uint64_t* presorted, double beta1, double beta2, float lr,
                      const float* lr_dev, float eps, float weight_decay, int32_t weight_decay_mode, int64_t* step,
                      int32_t accumulator, void* workspace, size_t workspace_bytes, ce_stream_t stream,
                      const RowMoment* rv = nullptr, RowClip clip = RowClip{}) {
  const UpdateCall c = adam_call(weight, num_rows, dim, nnz, grad_out, act_dtype, beta1, beta2, lr, lr_dev, eps, step,
                                 workspace, workspace_bytes, weight_decay, weight_decay_mode, rv, clip);
  const SlotLookups L{indices, offsets, offsets_are_i64, num_bags, include_last_offset, per_sample_weights, mode,
                      hook_features, presorted};
  return in_row_slots(c, L, accumulator, stream);
}

static int adam_src(float* weight, int64_t num_rows, int32_t dim, int64_t nnz, const void* grad_out, int32_t act_dtype,
                    const uint64_t* src_keys, double beta1, double beta2, float lr, const float* lr_dev, float eps,
                    float weight_decay, int32_t weight_decay_mode, int64_t* step, int32_t accumulator, void* workspace,
                    size_t workspace_bytes, ce_stream_t stream, const RowMoment* rv = nullptr,
                    RowClip clip = RowClip{}) {
  const UpdateCall c = adam_call(weight, num_rows, dim, nnz, grad_out, act_dtype, beta1, beta2, lr, lr_dev, eps, step,
                                 workspace, workspace_bytes, weight_decay, weight_decay_mode, rv, clip);
  return in_row_src(c, src_keys, accumulator, stream);
}

extern "C" int ce_bag_backward_adam(float* weight, int64_t num_rows, int32_t dim, const int64_t* indices, int64_t nnz,
                                    const void* offsets, int32_t offsets_are_i64, int64_t num_bags,
                                    int32_t include_last_offset, const float* per_sample_weights, int32_t mode,
                                    int64_t hook_features, const void* grad_out, int32_t act_dtype,
                                    const uint64_t* presorted, double beta1, double beta2, float lr, const float* lr_dev,
                                    float eps, int64_t* step, int32_t accumulator, void* workspace,
                                    size_t workspace_bytes, ce_stream_t stream) {
  return adam_slots(weight, num_rows, dim, indices, nnz, offsets, offsets_are_i64, num_bags, include_last_offset,
                    per_sample_weights, mode, hook_features, grad_out, act_dtype, presorted, beta1, beta2, lr, lr_dev, eps,
                    0.f, CE_WD_NONE, step, accumulator, workspace, workspace_bytes, stream);
}

extern "C" int ce_bag_backward_adam_wd(float* weight, int64_t num_rows, int32_t dim, const int64_t* indices, int64_t nnz,
                                       const void* offsets, int32_t offsets_are_i64, int64_t num_bags,
                                       int32_t include_last_offset, const float* per_sample_weights, int32_t mode,
                                       int64_t hook_features, const void* grad_out, int32_t act_dtype,
                                       const uint64_t* presorted, double beta1, double beta2, float lr,
                                       const float* lr_dev, float eps, float weight_decay, int32_t weight_decay_mode,
                                       int64_t* step, int32_t accumulator, void* workspace, size_t workspace_bytes,
                                       ce_stream_t stream) {
  return adam_slots(weight, num_rows, dim, indices, nnz, offsets, offsets_are_i64, num_bags, include_last_offset,
                    per_sample_weights, mode, hook_features, grad_out, act_dtype, presorted, beta1, beta2, lr, lr_dev, eps,
                    weight_decay, weight_decay_mode, step, accumulator, workspace, workspace_bytes, stream);
}

extern "C" int ce_bag_backward_adam_src(float* weight, int64_t num_rows, int32_t dim, int64_t nnz, const void* grad_out,
                                        int32_t act_dtype, const uint64_t* src_keys, double beta1, double beta2, float lr,
                                        const float* lr_dev, float eps, int64_t* step, int32_t accumulator,
                                        void* workspace, size_t workspace_bytes, ce_stream_t stream) {
  return adam_src(weight, num_rows, dim, nnz, grad_out, act_dtype, src_keys, beta1, beta2, lr, lr_dev, eps, 0.f,
                  CE_WD_NONE, step, accumulator, workspace, workspace_bytes, stream);
}

extern "C" int ce_bag_backward_adam_src_wd(float* weight, int64_t num_rows, int32_t dim, int64_t nnz,
                                           const void* grad_out, int32_t act_dtype, const uint64_t* src_keys,
                                           double beta1, double beta2, float lr, const float* lr_dev, float eps,
                                           float weight_decay, int32_t weight_decay_mode, int64_t* step,
                                           int32_t accumulator, void* workspace, size_t workspace_bytes,
                                           ce_stream_t stream) {
  return adam_src(weight, num_rows, dim, nnz, grad_out, act_dtype, src_keys, beta1, beta2, lr, lr_dev, eps, weight_decay,
                  weight_decay_mode, step, accumulator, workspace, workspace_bytes, stream);
}

// ---- partial row-wise Adam on a table of rows w | m: the Adam entries with decay, and the second
// moment -- row_of_slot, v[v_rows], indexed by table row like row-wise Adagrad's momentum -- before beta1.  The
// accumulators are [., dim] as for any fp32 table, so the workspace is the Adam entries'.

extern "C" size_t ce_bag_backward_pradam_workspace(int64_t num_rows, int64_t nnz, int32_t dim, int32_t accumulator) {
  return ce_bag_backward_adam_workspace(num_rows, nnz, dim, accumulator);
}

extern "C" int ce_bag_backward_pradam(float* weight, int64_t num_rows, int32_t dim, const int64_t* indices, int64_t nnz,
                                      const void* offsets, int32_t offsets_are_i64, int64_t num_bags,
                                      int32_t include_last_offset, const float* per_sample_weights, int32_t mode,
                                      int64_t hook_features, const void* grad_out, int32_t act_dtype,
                                      const uint64_t* presorted, const int32_t* row_of_slot, float* v, int64_t v_rows,
                                      double beta1, double beta2, float lr, const float* lr_dev, float eps,
                                      float weight_decay, int32_t weight_decay_mode, int64_t* step, int32_t accumulator,
                                      void* workspace, size_t workspace_bytes, ce_stream_t stream) {
  const RowMoment rv{row_of_slot, v, v_rows};
  return adam_slots(weight, num_rows, dim, indices, nnz, offsets, offsets_are_i64, num_bags, include_last_offset,
                    per_sample_weights, mode, hook_features, grad_out, act_dtype, presorted, beta1, beta2, lr, lr_dev, eps,
                    weight_decay, weight_decay_mode, step, accumulator, workspace, workspace_bytes, stream, &rv);
}

extern "C" int ce_bag_backward_pradam_src(float* weight, int64_t num_rows, int32_t dim, int64_t nnz, const void* grad_out,
                                          int32_t act_dtype, const uint64_t* src_keys, const int32_t* row_of_slot,
                                          float* v, int64_t v_rows, double beta1, double beta2, float lr,
                                          const float* lr_dev, float eps, float weight_decay, int32_t weight_decay_mode,
                                          int64_t* step, int32_t accumulator, void* workspace, size_t workspace_bytes,
                                          ce_stream_t stream) {
  const RowMoment rv{row_of_slot, v, v_rows};
  return adam_src(weight, num_rows, dim, nnz, grad_out, act_dtype, src_keys, beta1, beta2, lr, lr_dev, eps, weight_decay,
                  weight_decay_mode, step, accumulator, workspace, workspace_bytes, stream, &rv);
}

// ---- gradient clipping for the Adam entries: the _wd / pradam lists with `grad_clip, grad_clip_mode`
// directly behind weight_decay_mode

extern "C" int ce_bag_backward_adam_clip(float* weight, int64_t num_rows, int32_t dim, const int64_t* indices,
                                         int64_t nnz, const void* offsets, int32_t offsets_are_i64, int64_t num_bags,
                                         int32_t include_last_offset, const float* per_sample_weights, int32_t mode,
                                         int64_t hook_features, const void* grad_out, int32_t act_dtype,
                                         const uint64_t* presorted, double beta1, double beta2, float lr,
                                         const float* lr_dev, float eps, float weight_decay, int32_t weight_decay_mode,
                                         float grad_clip, int32_t grad_clip_mode, int64_t* step, int32_t accumulator,
                                         void* workspace, size_t workspace_bytes, ce_stream_t stream) {
  return adam_slots(weight, num_rows, dim, indices, nnz, offsets, offsets_are_i64, num_bags, include_last_offset,
                    per_sample_weights, mode, hook_features, grad_out, act_dtype, presorted, beta1, beta2, lr, lr_dev, eps,
                    weight_decay, weight_decay_mode, step, accumulator, workspace, workspace_bytes, stream, nullptr,
                    RowClip{grad_clip, grad_clip_mode});
}

extern "C" int ce_bag_backward_adam_src_clip(float* weight, int64_t num_rows, int32_t dim, int64_t nnz,
                                             const void* grad_out, int32_t act_dtype, const uint64_t* src_keys,
                                             double beta1, double beta2, float lr, const float* lr_dev, float eps,
                                             float weight_decay, int32_t weight_decay_mode, float grad_clip,
                                             int32_t grad_clip_mode, int64_t* step, int32_t accumulator,
                                             void* workspace, size_t workspace_bytes, ce_stream_t stream) {
  return adam_src(weight, num_rows, dim, nnz, grad_out, act_dtype, src_keys, beta1, beta2, lr, lr_dev, eps, weight_decay,
                  weight_decay_mode, step, accumulator, workspace, workspace_bytes, stream, nullptr,
                  RowClip{grad_clip, grad_clip_mode});
}

extern "C" int ce_bag_backward_pradam_clip(float* weight, int64_t num_rows, int32_t dim, const int64_t* indices,
                                           int64_t nnz, const void* offsets, int32_t offsets_are_i64, int64_t num_bags,
                                           int32_t include_last_offset, const float* per_sample_weights, int32_t mode,
                                           int64_t hook_features, const void* grad_out, int32_t act_dtype,
                                           const uint64_t* presorted, const int32_t* row_of_slot, float* v,
                                           int64_t v_rows, double beta1, double beta2, float lr, const float* lr_dev,
                                           float eps, float weight_decay, int32_t weight_decay_mode, float grad_clip,
                                           int32_t grad_clip_mode, int64_t* step, int32_t accumulator, void* workspace,
                                           size_t workspace_bytes, ce_stream_t stream) {
  const RowMoment rv{row_of_slot, v, v_rows};
  return adam_slots(weight, num_rows, dim, indices, nnz, offsets, offsets_are_i64, num_bags, include_last_offset,
                    per_sample_weights, mode, hook_features, grad_out, act_dtype, presorted, beta1, beta2, lr, lr_dev, eps,
                    weight_decay, weight_decay_mode, step, accumulator, workspace, workspace_bytes, stream, &rv,
                    RowClip{grad_clip, grad_clip_mode});
}

extern "C" int ce_bag_backward_pradam_src_clip(float* weight, int64_t num_rows, int32_t dim, int64_t nnz,
                                               const void* grad_out, int32_t act_dtype, const uint64_t* src_keys,
                                               const int32_t* row_of_slot, float* v, int64_t v_rows, double beta1,
                                               double beta2, float lr, const float* lr_dev, float eps,
                                               float weight_decay, int32_t weight_decay_mode, float grad_clip,
                                               int32_t grad_clip_mode, int64_t* step, int32_t accumulator,
                                               void* workspace, size_t workspace_bytes, ce_stream_t stream) {
  const RowMoment rv{row_of_slot, v, v_rows};
  return adam_src(weight, num_rows, dim, nnz, grad_out, act_dtype, src_keys, beta1, beta2, lr, lr_dev, eps, weight_decay,
                  weight_decay_mode, step, accumulator, workspace, workspace_bytes, stream, &rv,
                  RowClip{grad_clip, grad_clip_mode});
}

// ---- element-wise Adagrad on a table of rows w | h: the clipped Adam entries' lists with lr_decay in
// the betas' place; decay and clip are in from the start.  The accumulators are [., dim] as for any fp32 table, so the
// workspace is the Adam entries'.

static UpdateCall adagrad_call(float* weight, int64_t num_rows, int32_t dim, int64_t nnz, const void* grad_out,
                               int32_t act, double lr_decay, float lr, const float* lr_dev, float eps, float wd,
                               int32_t wd_mode, RowClip clip, int64_t* step, void* workspace, size_t workspace_bytes) {
  UpdateCall c = adam_call(weight, num_rows, dim, nnz, grad_out, act, 0.0, 0.0, lr, lr_dev, eps, step, workspace,
                           workspace_bytes, wd, wd_mode, nullptr, clip);
  c.optimizer = kOptElemAdagrad;
  c.lr_decay = lr_decay;
  return c;
}

extern "C" size_t ce_bag_backward_adagrad_workspace(int64_t num_rows, int64_t nnz, int32_t dim, int32_t accumulator) {
  return ce_bag_backward_adam_workspace(num_rows, nnz, dim, accumulator);
}

extern "C" int ce_bag_backward_adagrad(float* weight, int64_t num_rows, int32_t dim, const int64_t* indices, int64_t nnz,
                                       const void* offsets, int32_t offsets_are_i64, int64_t num_bags,
                                       int32_t include_last_offset, const float* per_sample_weights, int32_t mode,
                                       int64_t hook_features, const void* grad_out, int32_t act_dtype,
                                       const uint64_t* presorted, double lr_decay, float lr, const float* lr_dev,
                                       float eps, float weight_decay, int32_t weight_decay_mode, float grad_clip,
                                       int32_t grad_clip_mode, int64_t* step, int32_t accumulator, void* workspace,
                                       size_t workspace_bytes, ce_stream_t stream) {
  const UpdateCall c = adagrad_call(weight, num_rows, dim, nnz, grad_out, act_dtype, lr_decay, lr, lr_dev, eps,
                                    weight_decay, weight_decay_mode, RowClip{grad_clip, grad_clip_mode}, step, workspace,
                                    workspace_bytes);
  const SlotLookups L{indices, offsets, offsets_are_i64, num_bags, include_last_offset, per_sample_weights, mode,
                      hook_features, presorted};
  return in_row_slots(c, L, accumulator, stream);
}

extern "C" int ce_bag_backward_adagrad_src(float* weight, int64_t num_rows, int32_t dim, int64_t nnz,
                                           const void* grad_out, int32_t act_dtype, const uint64_t* src_keys,
                                           double lr_decay, float lr, const float* lr_dev, float eps, float weight_decay,
                                           int32_t weight_decay_mode, float grad_clip, int32_t grad_clip_mode,
                                           int64_t* step, int32_t accumulator, void* workspace, size_t workspace_bytes,
                                           ce_stream_t stream) {
  const UpdateCall c = adagrad_call(weight, num_rows, dim, nnz, grad_out, act_dtype, lr_decay, lr, lr_dev, eps,
                                    weight_decay, weight_decay_mode, RowClip{grad_clip, grad_clip_mode}, step, workspace,
                                    workspace_bytes);
  return in_row_src(c, src_keys, accumulator, stream);
}

// ---- deterministic, accumulator-free updates of the in-row layouts: count the step, sort, fold,
// apply.  The lists are those of ce_bag_backward_adam_clip / _pradam_clip / _adagrad without `presorted` and
// `accumulator`.

extern "C" size_t ce_bag_backward_in_row_sorted_workspace(int64_t num_rows, int64_t nnz, int32_t dim) {
  (void)num_rows;
  if (nnz < 0 || nnz >= (int64_t)INT32_MAX || dim <= 0) return 0;
  const int64_t n = nnz < 1 ? 1 : nnz;
  return al256(sorted_rows_bytes(n)) + al256((size_t)n * (size_t)dim * 4);
}

// Everything the three entries refuse, from the arguments alone, before the first launch and before any HIP call; the
// order is the header's.  Then: the step, the sort, the fold, the apply.
static int in_row_sorted(const UpdateCall& c, const SlotLookups& L, ce_stream_t stream) {
  CE_REQUIRE(c.step, CE_ERR_INVALID, "step: null device pointer");
  int rc = wd_check(c.wd, c.wd_mode);
  if (rc) return rc;
  rc = clip_check(c.clip, c.clip_mode);
  if (rc) return rc;
  CE_REQUIRE(c.beta1 >= 0.0 && c.beta1 < 1.0 && c.beta2 >= 0.0 && c.beta2 < 1.0, CE_ERR_INVALID,
             "beta1 and beta2 must lie in [0, 1)");
  CE_REQUIRE(c.lr_decay >= 0.0, CE_ERR_INVALID, "lr_decay must be >= 0");       // (a NaN fails it; Adam passes 0)
  CE_REQUIRE(c.eps >= 0.f, CE_ERR_INVALID, "eps must be >= 0");
  CE_REQUIRE(c.lr_dev || c.lr >= 0.f, CE_ERR_INVALID, "lr must be >= 0");
  CE_REQUIRE_ACT(c.act);
  CE_REQUIRE(c.weight && c.grad_out && c.workspace, CE_ERR_INVALID, "null pointer");
  CE_REQUIRE(!c.rowv() || (c.momentum && c.momentum_rows > 0), CE_ERR_INVALID,
             "partial row-wise Adam needs its second moment: v, v_rows > 0");
  CE_REQUIRE(c.dim > 0, CE_ERR_INVALID, "dim must be positive");
  CE_REQUIRE(c.num_rows > 0 && c.num_rows < (int64_t)INT32_MAX, CE_ERR_INVALID, "num_rows out of range");
  CE_REQUIRE(c.nnz >= 0 && c.nnz < (int64_t)INT32_MAX, CE_ERR_INVALID, "nnz out of range");
  CE_REQUIRE(L.num_bags >= 0 && L.num_bags < (int64_t)INT32_MAX - 64, CE_ERR_INVALID, "num_bags out of range");
  CE_REQUIRE(L.mode == CE_MODE_SUM || L.mode == CE_MODE_MEAN, CE_ERR_UNSUPPORTED, "mode must be sum or mean");
  CE_REQUIRE(L.hookF >= 0 && L.hookF < (int64_t)INT32_MAX && (L.hookF == 0 || L.num_bags % L.hookF == 0),
             CE_ERR_INVALID, "hook_features must divide num_bags");
  CE_REQUIRE(al16(c.weight) && (((uintptr_t)c.step) & 7) == 0 && act_aligned(c.grad_out, c.act), CE_ERR_INVALID,
             "an in-row table must be 16-byte aligned, step 8-byte aligned and grad_out on the vector boundary");
  CE_REQUIRE((((uintptr_t)c.workspace) & 255) == 0, CE_ERR_INVALID, "workspace must be 256-byte aligned");
  CE_REQUIRE(c.workspace_bytes >= ce_bag_backward_in_row_sorted_workspace(c.num_rows, c.nnz, c.dim), CE_ERR_INVALID,
             "workspace too small");
  CE_REQUIRE_ADAM_DIM(c.dim);
  RowGeom r;
  rc = row_geometry(c.dim, true, r);
  if (rc) return rc;
  if (L.num_bags == 0 || c.nnz == 0) return CE_OK;
  CE_REQUIRE(L.indices && L.offsets, CE_ERR_INVALID, "null pointer");

  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_count_step, dim3(1), dim3(64), 0, s, c.step);
  char* sort_ws = (char*)c.workspace;
  float* partials = (float*)(sort_ws + al256(sorted_rows_bytes(c.nnz)));
  SortedRows sr{};
  rc = sorted_rows(L.indices, c.nnz, c.num_rows, L.offsets, L.off64, L.num_bags, L.include_last, sort_ws, s, sr, true);
  if (rc) return rc;
  InRowSortedArgs a{};
  a.u = update_args(c, r, c.step);
  a.grad_out = c.grad_out;
  a.partials = partials;
  a.rows_sorted = sr.rows;
  a.lookup_sorted = sr.lookups;
  a.bag_of = sr.bag_of;
  a.offsets = L.offsets;
  a.psw = L.psw;
  a.nnz = c.nnz;
  a.num_bags = L.num_bags;
  a.num_rows = (int32_t)c.num_rows;
  a.rowlen = r.rowlen;
  a.g_log2 = r.g_log2;
  a.off64 = L.off64;
  a.include_last = L.include_last;
  a.mode = L.mode;
  a.hookF = (int)L.hookF;
  a.hookB = L.hookF ? (int)(L.num_bags / L.hookF) : 0;
  a.clip = RowClip{c.clip, c.clip_mode};
  const dim3 g(grid_for(cdiv(c.nnz, 64), 4)), b(256);
  for_vec_lanes(r.nch, [&](auto l) {
    constexpr int N = decltype(l)::NCH;
    for_act(c.act, [&](auto at) {
      hipLaunchKernelGGL((k_in_row_fold<typename decltype(at)::AT, N>), g, b, 0, s, a);
    });
    for_decay(c.decay(), c.clipped(), [&](auto d) {
      constexpr bool WD = decltype(d)::WD, CL = decltype(d)::CLIP;
      if (c.elem()) hipLaunchKernelGGL((k_in_row_apply<N, false, WD, false, CL, true>), g, b, 0, s, a);
      else if (c.rowv()) hipLaunchKernelGGL((k_in_row_apply<N, true, WD, true, CL, false>), g, b, 0, s, a);
      else hipLaunchKernelGGL((k_in_row_apply<N, true, WD, false, CL, false>), g, b, 0, s, a);
    });
  });
  CE_LAUNCH_CHECK();
  return CE_OK;
}

extern "C" int ce_bag_backward_adam_sorted(float* weight, int64_t num_rows, int32_t dim, const int64_t* indices,
                                           int64_t nnz, const void* offsets, int32_t offsets_are_i64, int64_t num_bags,
                                           int32_t include_last_offset, const float* per_sample_weights, int32_t mode,
                                           int64_t hook_features, const void* grad_out, int32_t act_dtype, double beta1,
                                           double beta2, float lr, const float* lr_dev, float eps, float weight_decay,
                                           int32_t weight_decay_mode, float grad_clip, int32_t grad_clip_mode,
                                           int64_t* step, void* workspace, size_t workspace_bytes, ce_stream_t stream) {
  const UpdateCall c = adam_call(weight, num_rows, dim, nnz, grad_out, act_dtype, beta1, beta2, lr, lr_dev, eps, step,
                                 workspace, workspace_bytes, weight_decay, weight_decay_mode, nullptr,
                                 RowClip{grad_clip, grad_clip_mode});
  const SlotLookups L{indices, offsets, offsets_are_i64, num_bags, include_last_offset, per_sample_weights, mode,
                      hook_features, nullptr};
  return in_row_sorted(c, L, stream);
}

extern "C" int ce_bag_backward_pradam_sorted(float* weight, int64_t num_rows, int32_t dim, const int64_t* indices,
                                             int64_t nnz, const void* offsets, int32_t offsets_are_i64, int64_t num_bags,
                                             int32_t include_last_offset, const float* per_sample_weights, int32_t mode,
                                             int64_t hook_features, const void* grad_out, int32_t act_dtype,
                                             const int32_t* row_of_slot, float* v, int64_t v_rows, double beta1,
                                             double beta2, float lr, const float* lr_dev, float eps, float weight_decay,
                                             int32_t weight_decay_mode, float grad_clip, int32_t grad_clip_mode,
                                             int64_t* step, void* workspace, size_t workspace_bytes,
                                             ce_stream_t stream) {
  const RowMoment rv{row_of_slot, v, v_rows};
  const UpdateCall c = adam_call(weight, num_rows, dim, nnz, grad_out, act_dtype, beta1, beta2, lr, lr_dev, eps, step,
                                 workspace, workspace_bytes, weight_decay, weight_decay_mode, &rv,
                                 RowClip{grad_clip, grad_clip_mode});
  const SlotLookups L{indices, offsets, offsets_are_i64, num_bags, include_last_offset, per_sample_weights, mode,
                      hook_features, nullptr};
  return in_row_sorted(c, L, stream);
}

extern "C" int ce_bag_backward_adagrad_sorted(float* weight, int64_t num_rows, int32_t dim, const int64_t* indices,
                                              int64_t nnz, const void* offsets, int32_t offsets_are_i64,
                                              int64_t num_bags, int32_t include_last_offset,
                                              const float* per_sample_weights, int32_t mode, int64_t hook_features,
                                              const void* grad_out, int32_t act_dtype, double lr_decay, float lr,
                                              const float* lr_dev, float eps, float weight_decay,
                                              int32_t weight_decay_mode, float grad_clip, int32_t grad_clip_mode,
                                              int64_t* step, void* workspace, size_t workspace_bytes,
                                              ce_stream_t stream) {
  const UpdateCall c = adagrad_call(weight, num_rows, dim, nnz, grad_out, act_dtype, lr_decay, lr, lr_dev, eps,
                                    weight_decay, weight_decay_mode, RowClip{grad_clip, grad_clip_mode}, step, workspace,
                                    workspace_bytes);
  const SlotLookups L{indices, offsets, offsets_are_i64, num_bags, include_last_offset, per_sample_weights, mode,
                      hook_features, nullptr};
  return in_row_sorted(c, L, stream);
}
